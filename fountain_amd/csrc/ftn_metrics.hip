/*
 * ftn_metrics.hip -- the kernels and the device driver of the measuring stage (include/fountain_hip_metrics.h).  The per-element code is
 * ftn_metrics.h's, shared with the host twin; this file needs no scene internals and is its own translation unit.  No kernel uses an
 * atomic: a thread owns a slot, a workgroup a tile or a block of records, and every sum is the header's tree.
 *
 *   k_metrics_tile<SSIM>   a workgroup of 256 threads per 16 x 16 tile, thread ly * 16 + lx for the tile's slot of that number.  The
 *                          pointwise terms come from the thread's own pixel.  With SSIM the workgroup first marks the bad pixels of the
 *                          26 x 26 halo, then per channel stages the halo of both images in LDS (rows of 48 floats: the 32 lanes of a
 *                          half-wave read two rows at 16 consecutive columns, and a stride of 16 mod 32 banks keeps the rows apart),
 *                          runs the horizontal pass of the five planes into LDS (5 planes of 26 x 16 binary64; a half-wave then reads 32
 *                          consecutive 8-byte words, all 64 banks once) and the vertical pass from there.  Without SSIM none of that is
 *                          compiled in.  The tile's tree: the slots of a wavefront are an aligned subtree of 64, summed by exchanging
 *                          with lane ^ 1, ^ 2, ... ^ 32 (both partners form the same sum, addition being commutative), and the four
 *                          wavefronts' sums meet in LDS as (w0 + w1) + (w2 + w3).
 *   k_metrics_total<FINAL> a workgroup per 256 contiguous records, a subtree of the total's tree, summed the same way over `span` slots
 *                          (256, or the level's padded size where that is less); records past the level's end read as +0.0.  A level
 *                          of more than 256 records leaves one record per workgroup; the last level writes ftn_metrics_totals.
 */
#include "ftn_metrics.h"
#include <algorithm>

namespace ftn {

constexpr int kT = kMetricsTile, kHalo = kMetricsHalo, kStride = 48, kHItems = kHalo * kT;
static_assert(kT * kT == 256 && kStride >= kHalo && kStride % 32 == 16, "one slot per thread; rows of the halo 16 banks apart");

/* what a thread carries into a tree: its slot's eight values, its candidate for the largest difference, its counts */
struct MetricsLane { double v[FTN_METRICS_SUMS]; double max_abs; uint32_t max_index, n_nonfinite, n_different, n_windows; };

/* the header's pairwise tree over the workgroup's first `span` slots (a power of two, the same for every thread), slot = threadIdx.x;
 * the counts and the largest difference, which no order changes, ride along.  The result is thread 0's. */
__device__ __forceinline__ void metrics_block_tree(MetricsLane& s, uint32_t span) {
    __shared__ double s_sum[4][FTN_METRICS_SUMS], s_max[4];
    __shared__ uint32_t s_cnt[4][4];
    for (uint32_t m = 1; m < 64u && m < span; m <<= 1) {
#pragma unroll
        for (int i = 0; i < FTN_METRICS_SUMS; i++) s.v[i] = s.v[i] + __shfl_xor(s.v[i], (int)m);
    }
    for (int m = 1; m < 64; m <<= 1) {
        const double om = __shfl_xor(s.max_abs, m);
        const uint32_t oi = __shfl_xor(s.max_index, m);
        if (metrics_max_beats(om, oi, s.max_abs, s.max_index)) { s.max_abs = om; s.max_index = oi; }
        s.n_nonfinite += __shfl_xor(s.n_nonfinite, m); s.n_different += __shfl_xor(s.n_different, m); s.n_windows += __shfl_xor(s.n_windows, m);
    }
    const uint32_t wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63u) == 0u) {
#pragma unroll
        for (int i = 0; i < FTN_METRICS_SUMS; i++) s_sum[wave][i] = s.v[i];
        s_max[wave] = s.max_abs;
        s_cnt[wave][0] = s.max_index; s_cnt[wave][1] = s.n_nonfinite; s_cnt[wave][2] = s.n_different; s_cnt[wave][3] = s.n_windows;
    }
    __syncthreads();
    if (threadIdx.x == 0u) {
        if (span > 64u) {
#pragma unroll
            for (int i = 0; i < FTN_METRICS_SUMS; i++) {
                double r = s_sum[0][i] + s_sum[1][i];
                if (span > 128u) r = r + (s_sum[2][i] + s_sum[3][i]);
                s.v[i] = r;
            }
        }
        for (int k = 1; k < 4; k++) {
            if (metrics_max_beats(s_max[k], s_cnt[k][0], s.max_abs, s.max_index)) { s.max_abs = s_max[k]; s.max_index = s_cnt[k][0]; }
            s.n_nonfinite += s_cnt[k][1]; s.n_different += s_cnt[k][2]; s.n_windows += s_cnt[k][3];
        }
    }
}

__device__ __forceinline__ void metrics_store(MetricsRec* r, const MetricsLane& s) {
#pragma unroll
    for (int i = 0; i < FTN_METRICS_SUMS; i++) r->sum[i] = s.v[i];
    r->max_abs = s.max_abs; r->max_index = s.max_index; r->n_nonfinite = s.n_nonfinite; r->n_different = s.n_different; r->n_windows = s.n_windows;
}

template <bool SSIM>
__global__ void __launch_bounds__(256) k_metrics_tile(const float* __restrict__ test, const float* __restrict__ ref, MetricsCall e, MetricsRec* __restrict__ recs,
                                                      float* __restrict__ err_map, float* __restrict__ ssim_map, double* __restrict__ tile_sums) {
    __shared__ float s_a[SSIM ? kHalo * kStride : 1], s_b[SSIM ? kHalo * kStride : 1];
    __shared__ double s_h[SSIM ? 5 * kHItems : 1];
    __shared__ unsigned char s_bad[SSIM ? kHalo * kHalo : 1], s_hbad[SSIM ? kHItems : 1];
    const uint32_t tile = blockIdx.x, tile_y = tile / e.tiles_x, tile_x = tile - tile_y * e.tiles_x;
    const int t = (int)threadIdx.x, lx = t & (kT - 1), ly = t >> 4, x = (int)tile_x * kT + lx, y = (int)tile_y * kT + ly;
    const bool inside = x < e.w && y < e.h;
    const size_t p = (size_t)y * (size_t)e.w + (size_t)x;            /* below 2^31 where inside */
    const float nan = u2f(0x7fc00000u);

    MetricsLane s;
#pragma unroll
    for (int i = 0; i < FTN_METRICS_SUMS; i++) s.v[i] = 0.0;
    s.max_abs = -1.0; s.max_index = 0xffffffffu; s.n_nonfinite = 0u; s.n_different = 0u; s.n_windows = 0u;
    if (inside) {
        const float* const pa = test + 3u * p;
        const float* const pb = ref + 3u * p;
        const MetricsPoint pt = metrics_point(pa[0], pa[1], pa[2], pb[0], pb[1], pb[2], e.eps);
        s.n_different = pt.different ? 1u : 0u;
        if (pt.bad) s.n_nonfinite = 1u;
        else {
            s.v[0] = pt.SE; s.v[1] = pt.AE; s.v[2] = pt.REL; s.v[3] = pt.SM; s.v[4] = pt.se[0]; s.v[5] = pt.se[1]; s.v[6] = pt.se[2];
            s.max_abs = pt.max_ae; s.max_index = (uint32_t)p;
        }
        if (err_map) err_map[p] = pt.bad ? nan : (float)(pt.SE / 3.0);
    }

    if (SSIM) {
        const int hx0 = (int)tile_x * kT - kMetricsRadius, hy0 = (int)tile_y * kT - kMetricsRadius;
        /* the halo's pixel q = hy * 26 + hx: its place in the image, or -1 outside it */
        auto halo_pixel = [&](int q, int* hy, int* hx) -> long long {
            *hy = q / kHalo; *hx = q - *hy * kHalo;
            const int gx = hx0 + *hx, gy = hy0 + *hy;
            return (gx >= 0 && gx < e.w && gy >= 0 && gy < e.h) ? (long long)gy * e.w + gx : -1ll;
        };
        for (int q = t; q < kHalo * kHalo; q += 256) {
            int hy, hx;
            const long long g = halo_pixel(q, &hy, &hx);
            bool bad = false;
            if (g >= 0) {
                const float* const pa = test + 3u * (size_t)g;
                const float* const pb = ref + 3u * (size_t)g;
                bad = !(metrics_finite(pa[0]) && metrics_finite(pa[1]) && metrics_finite(pa[2]) && metrics_finite(pb[0]) && metrics_finite(pb[1]) && metrics_finite(pb[2]));
            }
            s_bad[q] = bad ? 1 : 0;                                   /* read back below by the thread that wrote it, and after a barrier */
        }
        const bool interior = inside && x >= kMetricsRadius && x < e.w - kMetricsRadius && y >= kMetricsRadius && y < e.h - kMetricsRadius;
        double ssim_p = 0.0;                                          /* (ssim_0 + ssim_1) + ssim_2, channel by channel */
        uint32_t bad_in_window = 0u;
#pragma unroll 1
        for (int c = 0; c < 3; c++) {
            __syncthreads();                                          /* the channel before has been read */
            for (int q = t; q < kHalo * kHalo; q += 256) {
                int hy, hx;
                const long long g = halo_pixel(q, &hy, &hx);
                const bool use = g >= 0 && !s_bad[q];
                s_a[hy * kStride + hx] = use ? test[3u * (size_t)g + (size_t)c] : 0.0f;
                s_b[hy * kStride + hx] = use ? ref[3u * (size_t)g + (size_t)c] : 0.0f;
            }
            __syncthreads();
            for (int q = t; q < kHItems; q += 256) {
                const int r = q >> 4, cx = q & (kT - 1);
                const Ssim5 m = metrics_hpass(e.g, [&](int k, float* a, float* b) { *a = s_a[r * kStride + cx + k]; *b = s_b[r * kStride + cx + k]; });
                s_h[q] = m.a; s_h[kHItems + q] = m.b; s_h[2 * kHItems + q] = m.aa; s_h[3 * kHItems + q] = m.bb; s_h[4 * kHItems + q] = m.ab;
                if (c == 0) {
                    uint32_t n = 0u;
                    for (int k = 0; k < kMetricsTaps; k++) n += s_bad[r * kHalo + cx + k];
                    s_hbad[q] = (unsigned char)n;
                }
            }
            __syncthreads();
            if (interior) {
                const Ssim5 m = metrics_vpass(e.g, [&](int k) {
                    const int q = (ly + k) * kT + lx;
                    return Ssim5{s_h[q], s_h[kHItems + q], s_h[2 * kHItems + q], s_h[3 * kHItems + q], s_h[4 * kHItems + q]};
                });
                const double v = metrics_ssim(m, e.C1, e.C2);
                ssim_p = c == 0 ? v : ssim_p + v;
                if (c == 0)
                    for (int k = 0; k < kMetricsTaps; k++) bad_in_window += s_hbad[(ly + k) * kT + lx];
            }
        }
        const bool window = interior && bad_in_window == 0u;
        if (window) { s.v[7] = ssim_p; s.n_windows = 1u; }
        if (inside && ssim_map) ssim_map[p] = window ? (float)(s.v[7] / 3.0) : nan;
    }

    metrics_block_tree(s, 256u);
    if (t == 0) {
        metrics_store(recs + tile, s);
        if (tile_sums) {
#pragma unroll
            for (int i = 0; i < FTN_METRICS_SUMS; i++) tile_sums[(size_t)FTN_METRICS_SUMS * tile + i] = s.v[i];
        }
    }
}

template <bool FINAL>
__global__ void __launch_bounds__(256) k_metrics_total(const MetricsRec* __restrict__ in, uint32_t n, uint32_t span, MetricsRec* __restrict__ out,
                                                       ftn_metrics_totals* __restrict__ totals, uint64_t n_pixels) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    MetricsLane s;
#pragma unroll
    for (int k = 0; k < FTN_METRICS_SUMS; k++) s.v[k] = 0.0;
    s.max_abs = -1.0; s.max_index = 0xffffffffu; s.n_nonfinite = 0u; s.n_different = 0u; s.n_windows = 0u;
    if (threadIdx.x < span && i < n) {
        const MetricsRec r = in[i];
#pragma unroll
        for (int k = 0; k < FTN_METRICS_SUMS; k++) s.v[k] = r.sum[k];
        s.max_abs = r.max_abs; s.max_index = r.max_index; s.n_nonfinite = r.n_nonfinite; s.n_different = r.n_different; s.n_windows = r.n_windows;
    }
    metrics_block_tree(s, span);
    if (threadIdx.x != 0u) return;
    if (!FINAL) { metrics_store(out + blockIdx.x, s); return; }
#pragma unroll
    for (int k = 0; k < FTN_METRICS_SUMS; k++) totals->sum[k] = s.v[k];
    const bool any = s.max_abs >= 0.0;
    totals->max_abs = any ? s.max_abs : 0.0;
    totals->max_abs_index = any ? (uint64_t)s.max_index : 0ull;
    totals->n_pixels = n_pixels; totals->n_nonfinite = s.n_nonfinite; totals->n_different = s.n_different; totals->n_ssim_windows = s.n_windows;
}

hipError_t launch_metrics(const float* test, const float* ref, const MetricsCall& e, bool ssim, ftn_metrics_totals* totals, float* err_map, float* ssim_map,
                          double* tile_sums, MetricsRec* workspace, hipStream_t stream) {
    if (ssim) hipLaunchKernelGGL(k_metrics_tile<true>, dim3(e.n_tiles), dim3(256), 0, stream, test, ref, e, workspace, err_map, ssim_map, tile_sums);
    else hipLaunchKernelGGL(k_metrics_tile<false>, dim3(e.n_tiles), dim3(256), 0, stream, test, ref, e, workspace, err_map, ssim_map, tile_sums);
    const uint64_t n_pixels = (uint64_t)e.w * (uint64_t)e.h;
    const MetricsRec* in = workspace;
    uint32_t n = e.n_tiles;
    while (n > 256u) {                                               /* a level's padded size is then a multiple of 256: whole subtrees */
        const uint32_t blocks = (n + 255u) / 256u;
        MetricsRec* const out = const_cast<MetricsRec*>(in) + n;
        hipLaunchKernelGGL(k_metrics_total<false>, dim3(blocks), dim3(256), 0, stream, in, n, 256u, out, (ftn_metrics_totals*)nullptr, n_pixels);
        in = out; n = blocks;
    }
    uint32_t span = 1u;
    while (span < n) span <<= 1;
    hipLaunchKernelGGL(k_metrics_total<true>, dim3(1), dim3(256), 0, stream, in, n, span, (MetricsRec*)nullptr, totals, n_pixels);
    return hipGetLastError();
}

}  // namespace ftn
