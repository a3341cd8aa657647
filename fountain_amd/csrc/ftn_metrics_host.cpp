/*
 * ftn_metrics_host.cpp -- C entry points of include/fountain_hip_metrics.h: the refusals, the workspace size, the resolve, the host twin
 * of the kernels and the host-buffer entry.
 *
 * The per-element code is ftn_metrics.h's, shared with the kernels; the refusals' shared parts and the device buffers of the host-buffer
 * entry are the stages' scaffold's (ftn_stage_host.h).  The twin works tile by tile as the kernels do (a tile is written from its own
 * inputs alone, so the number of host threads changes nothing) and sums with the header's tree written as the recursion it is.
 */
#include "ftn_stage_host.h"
#include "ftn_metrics.h"

#include <cmath>
#include <cstring>
#include <limits>

using namespace ftn;

namespace {

/* refusals (3) to (7) of the header */
int flags_check(uint32_t flags) {
    if (flags & ~FTN_METRICS_SSIM) return fail(FTN_ERR_INVALID_ARGUMENT, "unknown ftn_metrics_params.flags bits");
    return FTN_OK;
}

int params_check(const ftn_metrics_params* p, int32_t w, int32_t h, const void* ssim_map) {
    int rc = flags_check(p->flags); if (rc) return rc;
    if (p->reserved != 0) return fail(FTN_ERR_INVALID_ARGUMENT, "ftn_metrics_params.reserved must be 0");
    if (!is_finite(p->peak) || !is_finite(p->rel_eps) || !(p->peak > 0.0f) || !(p->rel_eps > 0.0f))
        return fail(FTN_ERR_INVALID_ARGUMENT, "peak and rel_eps of ftn_metrics_params must be finite and above 0");
    if ((p->flags & FTN_METRICS_SSIM) && (w < kMetricsTaps || h < kMetricsTaps))
        return fail(FTN_ERR_INVALID_ARGUMENT, "FTN_METRICS_SSIM needs an image of at least 11 x 11 pixels");
    if (ssim_map && !(p->flags & FTN_METRICS_SSIM)) return fail(FTN_ERR_INVALID_ARGUMENT, "an ssim_map needs FTN_METRICS_SSIM");
    return FTN_OK;
}

void weights(double (&g)[kMetricsTaps]) {
    double e[kMetricsTaps], s = 0.0;
    for (int k = 0; k < kMetricsTaps; k++) { const double d = (double)(k - kMetricsRadius); e[k] = std::exp(-(d * d) / 4.5); s = s + e[k]; }
    for (int k = 0; k < kMetricsTaps; k++) g[k] = e[k] / s;
}

MetricsCall metrics_make(const ftn_metrics_params& p, int32_t w, int32_t h) {
    MetricsCall e;
    e.eps = (double)p.rel_eps;
    const double k1 = 0.01 * (double)p.peak, k2 = 0.03 * (double)p.peak;
    e.C1 = k1 * k1; e.C2 = k2 * k2;
    weights(e.g);
    e.w = w; e.h = h;
    e.tiles_x = ((uint32_t)w + kMetricsTile - 1) / kMetricsTile;
    e.n_tiles = e.tiles_x * (((uint32_t)h + kMetricsTile - 1) / kMetricsTile);
    return e;
}

/* S[lo, lo + n) of the header, n a power of two */
double tree(const double* v, size_t n) { return n == 1 ? v[0] : tree(v, n / 2) + tree(v + n / 2, n / 2); }

/* one tile: its record, and the maps' pixels */
void tile_cpu(const float* test, const float* ref, const MetricsCall& e, bool ssim, uint32_t tile, MetricsRec* rec, float* err_map, float* ssim_map) {
    const float nan = u2f(0x7fc00000u);
    const int ty = (int)(tile / e.tiles_x), tx = (int)(tile - (uint32_t)ty * e.tiles_x), x0 = tx * kMetricsTile, y0 = ty * kMetricsTile;
    static thread_local double slot[FTN_METRICS_SUMS][kMetricsSlots];
    memset(slot, 0, sizeof(slot));
    rec->max_abs = -1.0; rec->max_index = 0xffffffffu; rec->n_nonfinite = 0; rec->n_different = 0; rec->n_windows = 0;
    for (int ly = 0; ly < kMetricsTile && y0 + ly < e.h; ly++) {
        for (int lx = 0; lx < kMetricsTile && x0 + lx < e.w; lx++) {
            const size_t p = (size_t)(y0 + ly) * (size_t)e.w + (size_t)(x0 + lx);
            const int q = ly * kMetricsTile + lx;
            const float *pa = test + 3 * p, *pb = ref + 3 * p;
            const MetricsPoint pt = metrics_point(pa[0], pa[1], pa[2], pb[0], pb[1], pb[2], e.eps);
            if (pt.different) rec->n_different++;
            if (pt.bad) rec->n_nonfinite++;
            else {
                slot[0][q] = pt.SE; slot[1][q] = pt.AE; slot[2][q] = pt.REL; slot[3][q] = pt.SM; slot[4][q] = pt.se[0]; slot[5][q] = pt.se[1]; slot[6][q] = pt.se[2];
                if (metrics_max_beats(pt.max_ae, (uint32_t)p, rec->max_abs, rec->max_index)) { rec->max_abs = pt.max_ae; rec->max_index = (uint32_t)p; }
            }
            if (err_map) err_map[p] = pt.bad ? nan : (float)(pt.SE / 3.0);
        }
    }
    if (ssim) {
        /* the halo: where each of its pixels lies in the image (-1 outside), and which are bad */
        long long at[kMetricsHalo][kMetricsHalo];
        bool bad[kMetricsHalo][kMetricsHalo];
        for (int hy = 0; hy < kMetricsHalo; hy++) {
            for (int hx = 0; hx < kMetricsHalo; hx++) {
                const int gx = x0 - kMetricsRadius + hx, gy = y0 - kMetricsRadius + hy;
                const long long g = (gx >= 0 && gx < e.w && gy >= 0 && gy < e.h) ? (long long)gy * e.w + gx : -1ll;
                at[hy][hx] = g;
                bad[hy][hx] = false;
                if (g >= 0)
                    for (int c = 0; c < 3; c++) bad[hy][hx] |= !metrics_finite(test[3 * g + c]) || !metrics_finite(ref[3 * g + c]);
            }
        }
        bool window[kMetricsTile][kMetricsTile];
        for (int ly = 0; ly < kMetricsTile; ly++) {
            for (int lx = 0; lx < kMetricsTile; lx++) {
                const int x = x0 + lx, y = y0 + ly;
                bool ok = x >= kMetricsRadius && x < e.w - kMetricsRadius && y >= kMetricsRadius && y < e.h - kMetricsRadius;
                for (int j = 0; ok && j < kMetricsTaps; j++)
                    for (int i = 0; i < kMetricsTaps; i++) ok &= !bad[ly + j][lx + i];
                window[ly][lx] = ok;
            }
        }
        float a[kMetricsHalo][kMetricsHalo], b[kMetricsHalo][kMetricsHalo];
        static thread_local Ssim5 H[kMetricsHalo][kMetricsTile];
        double ssim_p[kMetricsTile][kMetricsTile];
        for (int c = 0; c < 3; c++) {
            for (int hy = 0; hy < kMetricsHalo; hy++) {
                for (int hx = 0; hx < kMetricsHalo; hx++) {
                    const bool use = at[hy][hx] >= 0 && !bad[hy][hx];
                    a[hy][hx] = use ? test[3 * at[hy][hx] + c] : 0.0f;
                    b[hy][hx] = use ? ref[3 * at[hy][hx] + c] : 0.0f;
                }
            }
            for (int r = 0; r < kMetricsHalo; r++)
                for (int cx = 0; cx < kMetricsTile; cx++)
                    H[r][cx] = metrics_hpass(e.g, [&](int k, float* fa, float* fb) { *fa = a[r][cx + k]; *fb = b[r][cx + k]; });
            for (int ly = 0; ly < kMetricsTile; ly++) {
                for (int lx = 0; lx < kMetricsTile; lx++) {
                    if (!window[ly][lx]) continue;
                    const double v = metrics_ssim(metrics_vpass(e.g, [&](int k) { return H[ly + k][lx]; }), e.C1, e.C2);
                    ssim_p[ly][lx] = c == 0 ? v : ssim_p[ly][lx] + v;
                }
            }
        }
        for (int ly = 0; ly < kMetricsTile && y0 + ly < e.h; ly++) {
            for (int lx = 0; lx < kMetricsTile && x0 + lx < e.w; lx++) {
                if (window[ly][lx]) { slot[7][ly * kMetricsTile + lx] = ssim_p[ly][lx]; rec->n_windows++; }
                if (ssim_map) ssim_map[(size_t)(y0 + ly) * (size_t)e.w + (size_t)(x0 + lx)] = window[ly][lx] ? (float)(ssim_p[ly][lx] / 3.0) : nan;
            }
        }
    }
    for (int i = 0; i < FTN_METRICS_SUMS; i++) rec->sum[i] = tree(slot[i], kMetricsSlots);
}

/* refusals (1) to (7) of the host-buffer entry and the twin */
int host_check(const float* test, const float* ref, int32_t w, int32_t h, const ftn_metrics_params* p, const void* result, const void* ssim_map) {
    if (!test || !ref || !p || !result) return fail(FTN_ERR_INVALID_ARGUMENT, "null argument");
    int rc;
    if ((rc = image_check(w, h)) || (rc = params_check(p, w, h, ssim_map))) return rc;
    return FTN_OK;
}

}  // namespace

extern "C" {

static_assert(sizeof(ftn_metrics_params) == 16 && sizeof(ftn_metrics_totals) == 112 && sizeof(ftn_metrics_result) == 136, "ABI");
int ftn_metrics_abi_version(void) { return FTN_METRICS_ABI_VERSION; }

void ftn_metrics_params_default(ftn_metrics_params* p) {
    if (!p) return;
    p->flags = 0;
    p->peak = 1.0f;
    p->rel_eps = 1e-2f;
    p->reserved = 0;
}

int ftn_metrics_workspace_size(int32_t w, int32_t h, uint32_t flags, size_t* bytes) {
    if (!bytes) return fail(FTN_ERR_INVALID_ARGUMENT, "null argument");
    int rc;
    if ((rc = image_check(w, h)) || (rc = flags_check(flags))) return rc;
    ftn_metrics_params p;
    ftn_metrics_params_default(&p);
    *bytes = metrics_workspace_bytes(metrics_make(p, w, h).n_tiles);
    return FTN_OK;
}

int ftn_metrics_ssim_weights(double g[FTN_METRICS_SSIM_TAPS]) {
    if (!g) return fail(FTN_ERR_INVALID_ARGUMENT, "null argument");
    double v[kMetricsTaps];
    weights(v);
    memcpy(g, v, sizeof(v));
    return FTN_OK;
}

int ftn_metrics_resolve(const ftn_metrics_totals* t, const ftn_metrics_params* p, ftn_metrics_result* r) {
    if (!t || !p || !r) return fail(FTN_ERR_INVALID_ARGUMENT, "null argument");
    if (!is_finite(p->peak) || !(p->peak > 0.0f)) return fail(FTN_ERR_INVALID_ARGUMENT, "peak and rel_eps of ftn_metrics_params must be finite and above 0");
    if (t->n_nonfinite > t->n_pixels) return fail(FTN_ERR_INVALID_ARGUMENT, "ftn_metrics_totals counts more bad pixels than pixels");
    const double nan = std::numeric_limits<double>::quiet_NaN(), peak = (double)p->peak;
    const uint64_t n = t->n_pixels - t->n_nonfinite;
    const double n3 = 3.0 * (double)n;
    r->mse = n ? t->sum[0] / n3 : nan;
    r->rmse = n ? std::sqrt(r->mse) : nan;
    r->mae = n ? t->sum[1] / n3 : nan;
    r->rel_mse = n ? t->sum[2] / n3 : nan;
    r->smape = n ? t->sum[3] / n3 : nan;
    r->psnr = !n ? nan : (r->mse == 0.0 ? std::numeric_limits<double>::infinity() : 10.0 * std::log10(peak * peak / r->mse));
    r->ssim = t->n_ssim_windows ? t->sum[7] / (3.0 * (double)t->n_ssim_windows) : nan;
    for (int c = 0; c < 3; c++) r->mse_rgb[c] = n ? t->sum[4 + c] / (double)n : nan;
    r->max_abs = n ? t->max_abs : nan;
    r->max_abs_index = t->max_abs_index;
    r->n_pixels = t->n_pixels; r->n = n; r->n_nonfinite = t->n_nonfinite; r->n_different = t->n_different; r->n_ssim_windows = t->n_ssim_windows;
    return FTN_OK;
}

int ftn_metrics_device(const void* test, const void* ref, int32_t w, int32_t h, const ftn_metrics_params* p, void* totals, void* err_map, void* ssim_map,
                       void* tile_sums, void* workspace, void* stream) {
    int rc;
    if ((rc = host_check((const float*)test, (const float*)ref, w, h, p, totals, ssim_map))) return rc;
    const MetricsCall e = metrics_make(*p, w, h);
    const size_t n = (size_t)w * (size_t)h;
    const Range r_test = {test, 3 * n * sizeof(float), 16}, r_ref = {ref, 3 * n * sizeof(float), 16}, r_tot = {totals, sizeof(ftn_metrics_totals), 16},
                r_err = {err_map, n * sizeof(float), 16}, r_ssim = {ssim_map, n * sizeof(float), 16},
                r_tiles = {tile_sums, (size_t)e.n_tiles * FTN_METRICS_SUMS * sizeof(double), 16}, r_ws = {workspace, metrics_workspace_bytes(e.n_tiles), 16};
    if (!workspace) return fail(FTN_ERR_INVALID_ARGUMENT, "null workspace");
    if ((rc = overlap_check({r_tot, r_err, r_ssim, r_tiles, r_ws}, {r_test, r_ref}, "an output or the workspace overlaps an input",
                            "two of the outputs and the workspace overlap"))) return rc;
    if ((rc = align_check({r_test, r_ref, r_tot, r_err, r_ssim, r_tiles, r_ws}, "misaligned buffer: test, ref, the outputs and the workspace need 16 bytes"))) return rc;
    if ((rc = need_device())) return rc;
    return launched(launch_metrics((const float*)test, (const float*)ref, e, (p->flags & FTN_METRICS_SSIM) != 0, (ftn_metrics_totals*)totals, (float*)err_map,
                                   (float*)ssim_map, (double*)tile_sums, (MetricsRec*)workspace, (hipStream_t)stream), "metrics");
}

int ftn_metrics(const float* test, const float* ref, int32_t w, int32_t h, const ftn_metrics_params* p, ftn_metrics_result* result, ftn_metrics_totals* totals,
                float* err_map, float* ssim_map, double* tile_sums, int32_t device) {
    int rc;
    if ((rc = host_check(test, ref, w, h, p, result, ssim_map))) return rc;
    if ((rc = need_device()) || (rc = set_device(device))) return rc;
    const size_t n = (size_t)w * (size_t)h, n_tiles = metrics_make(*p, w, h).n_tiles;
    StageBufs bufs;
    float *d_test, *d_ref = nullptr, *d_err, *d_ssim;
    double* d_tiles;
    unsigned char* d_ws;
    ftn_metrics_totals* d_tot;
    if ((rc = bufs.upload(test, 3 * n, &d_test)) || (ref != test && (rc = bufs.upload(ref, 3 * n, &d_ref))) || (rc = bufs.alloc(1, &d_tot)) ||
        (rc = bufs.alloc(err_map ? n : 0, &d_err)) || (rc = bufs.alloc(ssim_map ? n : 0, &d_ssim)) ||
        (rc = bufs.alloc(tile_sums ? n_tiles * FTN_METRICS_SUMS : 0, &d_tiles)) || (rc = bufs.alloc(metrics_workspace_bytes(n_tiles), &d_ws))) return rc;
    if ((rc = ftn_metrics_device(d_test, ref == test ? d_test : d_ref, w, h, p, d_tot, d_err, d_ssim, d_tiles, d_ws, nullptr))) return rc;
    ftn_metrics_totals t;
    if ((rc = bufs.copy_back(&t, (const ftn_metrics_totals*)d_tot, 1)) || (rc = bufs.copy_back(err_map, (const float*)d_err, n)) ||
        (rc = bufs.copy_back(ssim_map, (const float*)d_ssim, n)) || (rc = bufs.copy_back(tile_sums, (const double*)d_tiles, n_tiles * FTN_METRICS_SUMS))) return rc;
    if (totals) *totals = t;
    return ftn_metrics_resolve(&t, p, result);
}

int ftn_metrics_cpu(const float* test, const float* ref, int32_t w, int32_t h, const ftn_metrics_params* p, ftn_metrics_result* result, ftn_metrics_totals* totals,
                    float* err_map, float* ssim_map, double* tile_sums) {
    int rc;
    if ((rc = host_check(test, ref, w, h, p, result, ssim_map))) return rc;
    const MetricsCall e = metrics_make(*p, w, h);
    const bool ssim = (p->flags & FTN_METRICS_SSIM) != 0;
    const size_t n = (size_t)w * (size_t)h, n_tiles = e.n_tiles;
    std::vector<MetricsRec> recs(n_tiles);
    /* parallel_for sizes its threads by pixels; each takes the tiles of its share */
    parallel_for(n, [&](size_t i0, size_t i1) {
        const size_t t0 = i0 * n_tiles / n, t1 = i1 * n_tiles / n;       /* below 2^31 * 2^23 */
        for (size_t t = t0; t < t1; t++) tile_cpu(test, ref, e, ssim, (uint32_t)t, &recs[t], err_map, ssim_map);
    });
    size_t padded = 1;
    while (padded < n_tiles) padded <<= 1;
    ftn_metrics_totals t;
    std::vector<double> v(padded);
    for (int i = 0; i < FTN_METRICS_SUMS; i++) {
        std::fill(v.begin(), v.end(), 0.0);
        for (size_t k = 0; k < n_tiles; k++) v[k] = recs[k].sum[i];
        t.sum[i] = tree(v.data(), padded);
    }
    double max_abs = -1.0;
    uint32_t max_index = 0xffffffffu;
    t.n_pixels = n; t.n_nonfinite = 0; t.n_different = 0; t.n_ssim_windows = 0;
    for (const MetricsRec& r : recs) {
        if (metrics_max_beats(r.max_abs, r.max_index, max_abs, max_index)) { max_abs = r.max_abs; max_index = r.max_index; }
        t.n_nonfinite += r.n_nonfinite; t.n_different += r.n_different; t.n_ssim_windows += r.n_windows;
    }
    t.max_abs = max_abs >= 0.0 ? max_abs : 0.0;
    t.max_abs_index = max_abs >= 0.0 ? max_index : 0;
    if (tile_sums)
        for (size_t k = 0; k < n_tiles; k++) memcpy(tile_sums + FTN_METRICS_SUMS * k, recs[k].sum, sizeof(recs[k].sum));
    if (totals) *totals = t;
    return ftn_metrics_resolve(&t, p, result);
}

}  /* extern "C" */
