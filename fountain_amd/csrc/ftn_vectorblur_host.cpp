/*
 * ftn_vectorblur_host.cpp -- C entry points of include/fountain_hip_vectorblur.h: the refusals, the workspace size, the host twin of the
 * kernels and the host-buffer entry.
 *
 * The per-pixel code is ftn_vectorblur.h's, shared with the kernels; the refusals' shared parts and the device buffers of the host-buffer
 * entry are the stages' scaffold's (ftn_stage_host.h).
 */
#include "ftn_stage_host.h"
#include "ftn_vectorblur.h"

using namespace ftn;

namespace {

/* refusals (3) to (7) of the header */
int params_check(const ftn_vectorblur_params* p) {
    if (p->taps < 1 || p->taps > FTN_VECTORBLUR_MAX_TAPS) return fail(FTN_ERR_INVALID_ARGUMENT, "vector blur taps must be 1..64");
    if (p->flags != 0) return fail(FTN_ERR_INVALID_ARGUMENT, "unknown ftn_vectorblur_params.flags bits");
    if (p->reserved[0] != 0 || p->reserved[1] != 0 || p->reserved[2] != 0) return fail(FTN_ERR_INVALID_ARGUMENT, "ftn_vectorblur_params.reserved must be 0");
    if (!is_finite(p->shutter) || !is_finite(p->max_radius) || !is_finite(p->depth_extent))
        return fail(FTN_ERR_INVALID_ARGUMENT, "shutter, max_radius and depth_extent of ftn_vectorblur_params must be finite");
    if (!(p->shutter >= 0.0f && p->shutter <= 1.0f) || !(p->max_radius > 0.0f && p->max_radius <= (float)FTN_VECTORBLUR_MAX_RADIUS) || !(p->depth_extent > 0.0f))
        return fail(FTN_ERR_INVALID_ARGUMENT, "ftn_vectorblur_params out of range: shutter in [0, 1], max_radius in (0, 16] (a blur stays within the 16 x 16 tiles around "
                                              "its own), depth_extent > 0");
    return FTN_OK;
}

/* refusals (1) to (7) */
int call_check(const void* rgb, const void* motion2, int32_t w, int32_t h, const ftn_vectorblur_params* p, const void* out_rgb) {
    if (!rgb || !motion2 || !p || !out_rgb) return fail(FTN_ERR_INVALID_ARGUMENT, "null argument");
    int rc;
    if ((rc = image_check(w, h)) || (rc = params_check(p))) return rc;
    return FTN_OK;
}

/* steps 1 to 3 into `recs`, the workspace's layout */
void velocities(const float* motion2, const float* gb12, const VbPlan& plan, const VbCall& e, VbRec* recs) {
    const int w = plan.w, h = plan.h;
    const size_t n = (size_t)w * (size_t)h, tiles = (size_t)plan.tiles_x * (size_t)plan.tiles_y;
    VbRec* const tile_recs = recs + plan.tile_off;
    VbRec* const nb_recs = recs + plan.nb_off;
    /* step 1 */
    parallel_for(n, [&](size_t i0, size_t i1) {
        for (size_t i = i0; i < i1; i++)
            recs[i] = vb_velocity(motion2[2 * i], motion2[2 * i + 1], gb12 ? vb_depth(gb12[12 * i + 9], gb12[12 * i + 10]) : 0.0f, e);
    });
    /* step 2: a tile per iteration, its pixels in row-major order */
    parallel_for(tiles, [&](size_t t0, size_t t1) {
        for (size_t t = t0; t < t1; t++) {
            const int x0 = (int)(t % (size_t)plan.tiles_x) * FTN_VB_TILE, y0 = (int)(t / (size_t)plan.tiles_x) * FTN_VB_TILE;
            float best = -1.0f;
            uint32_t best_i = 0xffffffffu;
            for (int y = y0; y < std::min(y0 + FTN_VB_TILE, h); y++)
                for (int x = x0; x < std::min(x0 + FTN_VB_TILE, w); x++) {
                    const uint32_t i = (uint32_t)y * (uint32_t)w + (uint32_t)x;
                    const float key = vb_key(recs[i]);
                    if (vb_before(key, i, best, best_i)) { best = key; best_i = i; }
                }
            tile_recs[t] = VbRec{recs[best_i].x, recs[best_i].y, best, 0.0f};
        }
    });
    /* step 3 */
    parallel_for(tiles, [&](size_t t0, size_t t1) {
        for (size_t t = t0; t < t1; t++) {
            const int tx = (int)(t % (size_t)plan.tiles_x), ty = (int)(t / (size_t)plan.tiles_x);
            VbRec best = tile_recs[t];
            uint32_t best_i = (uint32_t)t;
            for (int j = -1; j <= 1; j++)
                for (int i = -1; i <= 1; i++) {
                    const int nx = tx + i, ny = ty + j;
                    if (nx < 0 || ny < 0 || nx >= plan.tiles_x || ny >= plan.tiles_y) continue;
                    const uint32_t ti = (uint32_t)ny * (uint32_t)plan.tiles_x + (uint32_t)nx;
                    if (vb_before(tile_recs[ti].l, ti, best.l, best_i)) { best = tile_recs[ti]; best_i = ti; }
                }
            nb_recs[t] = best;
        }
    });
}

}  // namespace

extern "C" {

static_assert(sizeof(ftn_vectorblur_params) == 32, "ABI");
static_assert(sizeof(VbRec) == 16, "the workspace's records");
int ftn_vectorblur_abi_version(void) { return FTN_VECTORBLUR_ABI_VERSION; }

void ftn_vectorblur_params_default(ftn_vectorblur_params* p) {
    if (!p) return;
    p->taps = 16;
    p->flags = 0;
    p->shutter = 0.5f;
    p->max_radius = 16.0f;
    p->depth_extent = 0.01f;
    p->reserved[0] = p->reserved[1] = p->reserved[2] = 0;
}

int ftn_vectorblur_workspace_size(int32_t w, int32_t h, size_t* bytes) {
    if (!bytes) return fail(FTN_ERR_INVALID_ARGUMENT, "null argument");
    int rc;
    if ((rc = image_check(w, h))) return rc;
    *bytes = vb_plan(w, h).recs * sizeof(VbRec);
    return FTN_OK;
}

int ftn_vectorblur_device(const void* rgb, const void* motion2, const void* gb12, int32_t w, int32_t h, const ftn_vectorblur_params* p, void* out_rgb, void* workspace,
                          void* stream) {
    int rc;
    if ((rc = call_check(rgb, motion2, w, h, p, out_rgb))) return rc;
    const VbPlan plan = vb_plan(w, h);
    const size_t n = (size_t)w * (size_t)h * sizeof(float);
    const Range r_rgb = {rgb, 3 * n, 16}, r_mo = {motion2, 2 * n, 16}, r_gb = {gb12, 12 * n, 16}, r_out = {out_rgb, 3 * n, 16}, r_ws = {workspace, plan.recs * sizeof(VbRec), 16};
    if (!workspace) return fail(FTN_ERR_INVALID_ARGUMENT, "null workspace");
    if ((rc = overlap_check({r_out, r_ws}, {r_rgb, r_mo, r_gb}, "out_rgb overlaps an input or the workspace, or the workspace overlaps an input"))) return rc;
    if ((rc = align_check({r_rgb, r_mo, r_gb, r_out, r_ws}, "misaligned buffer: rgb, motion2, gb12, out_rgb and the workspace need 16 bytes"))) return rc;
    if ((rc = need_device())) return rc;
    return launched(launch_vectorblur((const float*)rgb, (const float*)motion2, (const float*)gb12, plan, vb_make(*p), (float*)out_rgb, (VbRec*)workspace, (hipStream_t)stream),
                    "vector blur");
}

int ftn_vectorblur(const float* rgb, const float* motion2, const float* gb12, int32_t w, int32_t h, const ftn_vectorblur_params* p, float* out_rgb, int32_t device) {
    int rc;
    if ((rc = call_check(rgb, motion2, w, h, p, out_rgb))) return rc;
    if ((rc = need_device()) || (rc = set_device(device))) return rc;
    const size_t n = (size_t)w * (size_t)h;
    StageBufs bufs;
    float *d_rgb, *d_mo, *d_gb, *d_out;                            /* (d_gb is null where the caller gave no G-buffer) */
    VbRec* d_ws;
    if ((rc = bufs.upload(rgb, 3 * n, &d_rgb)) || (rc = bufs.upload(motion2, 2 * n, &d_mo)) || (rc = bufs.upload(gb12, 12 * n, &d_gb)) || (rc = bufs.alloc(3 * n, &d_out)) ||
        (rc = bufs.alloc(vb_plan(w, h).recs, &d_ws)))
        return rc;
    if ((rc = ftn_vectorblur_device(d_rgb, d_mo, d_gb, w, h, p, d_out, d_ws, nullptr))) return rc;
    return bufs.copy_back(out_rgb, d_out, 3 * n);
}

int ftn_vectorblur_velocities_cpu(const float* motion2, const float* gb12, int32_t w, int32_t h, const ftn_vectorblur_params* p, void* workspace) {
    if (!motion2 || !p || !workspace) return fail(FTN_ERR_INVALID_ARGUMENT, "null argument");
    int rc;
    if ((rc = image_check(w, h)) || (rc = params_check(p))) return rc;
    velocities(motion2, gb12, vb_plan(w, h), vb_make(*p), (VbRec*)workspace);
    return FTN_OK;
}

int ftn_vectorblur_cpu(const float* rgb, const float* motion2, const float* gb12, int32_t w, int32_t h, const ftn_vectorblur_params* p, float* out_rgb) {
    int rc;
    if ((rc = call_check(rgb, motion2, w, h, p, out_rgb))) return rc;
    const size_t n = (size_t)w * (size_t)h;
    if (overlaps(Range{out_rgb, 3 * n * sizeof(float), 4}, Range{rgb, 3 * n * sizeof(float), 4})) return fail(FTN_ERR_INVALID_ARGUMENT, "out_rgb overlaps rgb");
    const VbPlan plan = vb_plan(w, h);
    const VbCall e = vb_make(*p);
    std::vector<VbRec> ws(plan.recs);
    const VbRec* const recs = ws.data();
    const VbRec* const nb_recs = recs + plan.nb_off;
    velocities(motion2, gb12, plan, e, ws.data());
    /* step 4: the offsets of a tile are made again whenever a thread's run of pixels enters another tile */
    parallel_for(n, [&](size_t i0, size_t i1) {
        VbOffset off[FTN_VECTORBLUR_MAX_TAPS];
        size_t have = (size_t)-1;
        VbRec nb = {0.0f, 0.0f, 0.0f, 0.0f};
        for (size_t i = i0; i < i1; i++) {
            const int y = (int)(i / (size_t)w), x = (int)(i % (size_t)w);
            const size_t t = (size_t)(y / FTN_VB_TILE) * (size_t)plan.tiles_x + (size_t)(x / FTN_VB_TILE);
            if (t != have) {
                have = t; nb = nb_recs[t];
                for (int k = 0; k < e.taps; k++) off[k] = vb_offset(k, e.taps, nb);
            }
            const Vb3 o = vb_gather_pixel(x, y, w, h, nb, off, e,
                                          [&](int qx, int qy) { const float* const q = rgb + 3 * ((size_t)qy * (size_t)w + (size_t)qx); return Vb3{q[0], q[1], q[2]}; },
                                          [&](int qx, int qy) { return recs[(size_t)qy * (size_t)w + (size_t)qx]; });
            out_rgb[3 * i] = o.r; out_rgb[3 * i + 1] = o.g; out_rgb[3 * i + 2] = o.b;
        }
    });
    return FTN_OK;
}

}  /* extern "C" */
