/*
 * ftn_bloom_host.cpp -- C entry points of include/fountain_hip_bloom.h: the refusals, the workspace size, the host twin of the kernels
 * and the host-buffer entry.
 *
 * The per-pixel code is ftn_bloom.h's, shared with the kernels; the refusals' shared parts and the device buffers of the host-buffer
 * entry are the stages' scaffold's (ftn_stage_host.h).
 */
#include "ftn_stage_host.h"
#include "ftn_bloom.h"

#include <cstring>

using namespace ftn;

namespace {

int levels_check(int32_t levels) {
    if (levels < 0 || levels > FTN_BLOOM_MAX_LEVELS) return fail(FTN_ERR_INVALID_ARGUMENT, "bloom levels must be 0..12");
    return FTN_OK;
}

bool unit(float v) { return v >= 0.0f && v <= 1.0f; }

/* refusals (3) to (7) of the header */
int params_check(const ftn_bloom_params* p) {
    int rc = levels_check(p->levels); if (rc) return rc;
    if (p->flags & ~FTN_BLOOM_KARIS) return fail(FTN_ERR_INVALID_ARGUMENT, "unknown ftn_bloom_params.flags bits");
    if (p->reserved != 0) return fail(FTN_ERR_INVALID_ARGUMENT, "ftn_bloom_params.reserved must be 0");
    if (!is_finite(p->strength) || !is_finite(p->scatter) || !is_finite(p->threshold) || !is_finite(p->knee) || !is_finite(p->clamp_max))
        return fail(FTN_ERR_INVALID_ARGUMENT, "strength, scatter, threshold, knee and clamp_max of ftn_bloom_params must be finite");
    if (!unit(p->strength) || !unit(p->scatter) || !unit(p->knee) || !(p->threshold >= 0.0f) || !(p->clamp_max > 0.0f && p->clamp_max <= 1e30f))
        return fail(FTN_ERR_INVALID_ARGUMENT, "ftn_bloom_params out of range: strength, scatter and knee in [0, 1], threshold >= 0, clamp_max in (0, 1e30]");
    return FTN_OK;
}

bool is_copy(const BloomPlan& plan, const ftn_bloom_params* p) { return plan.L == 0 || p->strength == 0.0f; }

}  // namespace

extern "C" {

static_assert(sizeof(ftn_bloom_params) == 32, "ABI");
int ftn_bloom_abi_version(void) { return FTN_BLOOM_ABI_VERSION; }

void ftn_bloom_params_default(ftn_bloom_params* p) {
    if (!p) return;
    p->levels = 6;
    p->flags = 0;
    p->strength = 0.04f;
    p->scatter = 0.7f;
    p->threshold = 0.0f;
    p->knee = 0.5f;
    p->clamp_max = 65504.0f;
    p->reserved = 0;
}

int ftn_bloom_workspace_size(int32_t w, int32_t h, int32_t levels, size_t* bytes) {
    if (!bytes) return fail(FTN_ERR_INVALID_ARGUMENT, "null argument");
    int rc;
    if ((rc = image_check(w, h)) || (rc = levels_check(levels))) return rc;
    *bytes = bloom_plan(w, h, levels).floats * sizeof(float);
    return FTN_OK;
}

int ftn_bloom_device(const void* rgb, int32_t w, int32_t h, const ftn_bloom_params* p, void* out_rgb, void* workspace, void* stream) {
    if (!rgb || !p || !out_rgb) return fail(FTN_ERR_INVALID_ARGUMENT, "null argument");
    int rc;
    if ((rc = image_check(w, h)) || (rc = params_check(p))) return rc;
    const BloomPlan plan = bloom_plan(w, h, p->levels);
    const size_t n_rgb = 3 * (size_t)w * (size_t)h * sizeof(float);
    const Range r_rgb = {rgb, n_rgb, 16}, r_out = {out_rgb, n_rgb, 16}, r_ws = {workspace, plan.floats * sizeof(float), 16};
    if (r_ws.bytes && !workspace) return fail(FTN_ERR_INVALID_ARGUMENT, "null workspace");
    if ((rc = overlap_check({r_out, r_ws}, {r_rgb}, "out_rgb overlaps the input or the workspace, or the workspace overlaps the input"))) return rc;
    if ((rc = align_check({r_rgb, r_out, r_ws}, "misaligned buffer: rgb, out_rgb and the workspace need 16 bytes"))) return rc;
    if ((rc = need_device())) return rc;
    return launched(launch_bloom((const float*)rgb, plan, bloom_make(*p), is_copy(plan, p), (float*)out_rgb, (float*)workspace, (hipStream_t)stream), "bloom");
}

int ftn_bloom(const float* rgb, int32_t w, int32_t h, const ftn_bloom_params* p, float* out_rgb, int32_t device) {
    if (!rgb || !p || !out_rgb) return fail(FTN_ERR_INVALID_ARGUMENT, "null argument");
    int rc;
    if ((rc = image_check(w, h)) || (rc = params_check(p))) return rc;
    if ((rc = need_device()) || (rc = set_device(device))) return rc;
    const size_t n3 = 3 * (size_t)w * (size_t)h;
    StageBufs bufs;
    float *d_rgb, *d_out, *d_ws;                                   /* (d_ws is null where the plan needs no workspace) */
    if ((rc = bufs.upload(rgb, n3, &d_rgb)) || (rc = bufs.alloc(n3, &d_out)) || (rc = bufs.alloc(bloom_plan(w, h, p->levels).floats, &d_ws))) return rc;
    if ((rc = ftn_bloom_device(d_rgb, w, h, p, d_out, d_ws, nullptr))) return rc;
    return bufs.copy_back(out_rgb, d_out, n3);
}

int ftn_bloom_cpu(const float* rgb, int32_t w, int32_t h, const ftn_bloom_params* p, float* out_rgb) {
    if (!rgb || !p || !out_rgb) return fail(FTN_ERR_INVALID_ARGUMENT, "null argument");
    int rc;
    if ((rc = image_check(w, h)) || (rc = params_check(p))) return rc;
    const BloomPlan plan = bloom_plan(w, h, p->levels);
    const size_t n = (size_t)w * (size_t)h;
    if (is_copy(plan, p)) { memmove(out_rgb, rgb, 3 * n * sizeof(float)); return FTN_OK; }
    const BloomCall e = bloom_make(*p);
    const bool karis = (p->flags & FTN_BLOOM_KARIS) != 0;
    /* D_0 = P at full resolution (the kernels keep it in LDS only), then one array per level */
    std::vector<std::vector<float>> lv((size_t)plan.L + 1);
    lv[0].resize(3 * n);
    parallel_for(n, [&](size_t i0, size_t i1) {
        for (size_t i = i0; i < i1; i++) {
            const Bloom3 v = bloom_pre(rgb[3 * i], rgb[3 * i + 1], rgb[3 * i + 2], e);
            lv[0][3 * i] = v.r; lv[0][3 * i + 1] = v.g; lv[0][3 * i + 2] = v.b;
        }
    });
    for (int k = 0; k < plan.L; k++) {
        const int ws = plan.w[k], hs = plan.h[k], wd = plan.w[k + 1], hd = plan.h[k + 1];
        const float* const src = lv[k].data();
        lv[k + 1].resize(3 * (size_t)wd * (size_t)hd);
        float* const dst = lv[k + 1].data();
        const bool first_karis = karis && k == 0;
        parallel_for((size_t)wd * (size_t)hd, [&](size_t i0, size_t i1) {
            for (size_t i = i0; i < i1; i++) {
                const long long y = (long long)(i / (size_t)wd), x = (long long)(i % (size_t)wd);
                auto tap = [&](int ti, int tj) {
                    const long long gx = std::min<long long>(std::max<long long>(2 * x - 1 + ti, 0), ws - 1), gy = std::min<long long>(std::max<long long>(2 * y - 1 + tj, 0), hs - 1);
                    const float* const q = src + 3 * ((size_t)gy * (size_t)ws + (size_t)gx);
                    BloomTap t = {q[0], q[1], q[2], 0.0f};
                    if (first_karis) t.k = bloom_karis_k(t.r, t.g, t.b);
                    return t;
                };
                const Bloom3 o = first_karis ? bloom_down_pixel<true>(tap) : bloom_down_pixel<false>(tap);
                dst[3 * i] = o.r; dst[3 * i + 1] = o.g; dst[3 * i + 2] = o.b;
            }
        });
    }
    auto up = [](const float* coarse, int wc, int hc, int x, int y) {
        return bloom_up_pixel(x, y, wc, hc, [&](int, int, int cx, int cy) {
            const float* const q = coarse + 3 * ((size_t)cy * (size_t)wc + (size_t)cx);
            return Bloom3{q[0], q[1], q[2]};
        });
    };
    for (int k = plan.L - 1; k >= 1; k--) {
        const int wf = plan.w[k];
        float* const fine = lv[k].data();
        const float* const coarse = lv[k + 1].data();
        parallel_for((size_t)wf * (size_t)plan.h[k], [&](size_t i0, size_t i1) {
            for (size_t i = i0; i < i1; i++) {
                const Bloom3 u = up(coarse, plan.w[k + 1], plan.h[k + 1], (int)(i % (size_t)wf), (int)(i / (size_t)wf));
                fine[3 * i] = bloom_blend(fine[3 * i], u.r, e); fine[3 * i + 1] = bloom_blend(fine[3 * i + 1], u.g, e); fine[3 * i + 2] = bloom_blend(fine[3 * i + 2], u.b, e);
            }
        });
    }
    const float* const u1 = lv[1].data();
    const float* const P = lv[0].data();
    parallel_for(n, [&](size_t i0, size_t i1) {
        for (size_t i = i0; i < i1; i++) {
            const Bloom3 B = up(u1, plan.w[1], plan.h[1], (int)(i % (size_t)w), (int)(i / (size_t)w));
            out_rgb[3 * i] = bloom_composite(rgb[3 * i], B.r, P[3 * i], e);
            out_rgb[3 * i + 1] = bloom_composite(rgb[3 * i + 1], B.g, P[3 * i + 1], e);
            out_rgb[3 * i + 2] = bloom_composite(rgb[3 * i + 2], B.b, P[3 * i + 2], e);
        }
    });
    return FTN_OK;
}

}  /* extern "C" */
