/*
 * ftn_bloom.hip -- the kernels and the device driver of the bloom stage (include/fountain_hip_bloom.h).  The per-pixel code is
 * ftn_bloom.h's, shared with the host twin; this file needs no scene internals and is its own translation unit.  Every kernel is a
 * gather: a thread writes the pixels it owns from what it reads, with no atomics, so nothing depends on the launch shape.
 *
 *   k_bloom_down<PRE, KARIS>  a workgroup makes a 32 x 8 tile of a level from the 66 x 18 pixels of the finer one under it, which it
 *                             first stages in LDS, one plane per channel: neighbouring outputs share half their 4 x 4 footprint, so a
 *                             source pixel is fetched once per tile rather than four times.  A plane's row is 34 float2; a thread reads
 *                             its taps as float2 pairs (columns 2x - 1, 2x and 2x + 1, 2x + 2), 8 bytes per lane at a stride of 8
 *                             bytes, which no two lanes of a half-wave send to one bank.  PRE: the source is the input image and the
 *                             prefilter runs while staging (P is never stored at full resolution); KARIS adds a fourth plane, 1 / (1 + Y).
 *   k_bloom_up_blend          U_k = D_k (1 - scatter) + up(U_{k+1}) scatter, in place over D_k, a pixel per thread
 *   k_bloom_composite         four pixels per thread: three 16-byte loads of the input, the tent over U_1, the prefilter again, three
 *                             16-byte stores; the last n mod 4 pixels go through a scalar tail.  Four pixels of one row share their
 *                             tents' coarse pixels, 2 rows of 4 columns, which the thread fetches once: 8 12-byte loads instead of
 *                             16.  With a fetch per pixel the kernel ran at 3.8 TB/s, with the shared fetch at 4.9 TB/s, on the same
 *                             bytes from memory.  A group that straddles a row end fetches per pixel.
 *   k_bloom_copy              the exact copy of strength 0 or no level, a kernel so that a captured graph holds kernel nodes only
 */
#include "ftn_bloom.h"
#include <algorithm>

namespace ftn {

constexpr int kTX = FTN_BLOOM_TILE_X, kTY = FTN_BLOOM_TILE_Y, kFW = 2 * kTX + 2, kFH = 2 * kTY + 2, kPW = kFW / 2 + 1;
static_assert(kTX * kTY == 256, "one output per thread");

template <bool PRE, bool KARIS>
__global__ void __launch_bounds__(256) k_bloom_down(const float* __restrict__ src, int ws, int hs, float* __restrict__ dst, int wd, int hd, uint32_t tiles_x,
                                                    BloomCall e) {
    __shared__ float2 s_r[kFH][kPW], s_g[kFH][kPW], s_b[kFH][kPW], s_k[KARIS ? kFH : 1][kPW];
    const uint32_t tile_y = blockIdx.x / tiles_x, tile_x = blockIdx.x - tile_y * tiles_x;
    const int ox = (int)tile_x * kTX, oy = (int)tile_y * kTY;
    const long long fx0 = 2ll * ox - 1, fy0 = 2ll * oy - 1;
    for (int q = threadIdx.x; q < kFW * kFH; q += 256) {
        const int ty = q / kFW, tx = q - ty * kFW;
        const int gx = (int)std::min<long long>(std::max<long long>(fx0 + tx, 0), ws - 1), gy = (int)std::min<long long>(std::max<long long>(fy0 + ty, 0), hs - 1);
        const float* const p = src + 3u * ((size_t)gy * (size_t)ws + (size_t)gx);
        Bloom3 v = {p[0], p[1], p[2]};
        if (PRE) v = bloom_pre(v.r, v.g, v.b, e);
        reinterpret_cast<float*>(s_r[ty])[tx] = v.r; reinterpret_cast<float*>(s_g[ty])[tx] = v.g; reinterpret_cast<float*>(s_b[ty])[tx] = v.b;
        if (KARIS) reinterpret_cast<float*>(s_k[ty])[tx] = bloom_karis_k(v.r, v.g, v.b);
    }
    __syncthreads();
    const int lx = threadIdx.x & (kTX - 1), ly = threadIdx.x / kTX, x = ox + lx, y = oy + ly;
    if (x >= wd || y >= hd) return;
    const Bloom3 o = bloom_down_pixel<KARIS>([&](int i, int j) {
        const int row = 2 * ly + j, col = lx + (i >> 1);
        const float2 r = s_r[row][col], g = s_g[row][col], b = s_b[row][col];
        BloomTap t;
        t.r = (i & 1) ? r.y : r.x; t.g = (i & 1) ? g.y : g.x; t.b = (i & 1) ? b.y : b.x;
        t.k = 0.0f;
        if (KARIS) { const float2 k = s_k[row][col]; t.k = (i & 1) ? k.y : k.x; }
        return t;
    });
    float* const d = dst + 3u * ((size_t)y * (size_t)wd + (size_t)x);
    d[0] = o.r; d[1] = o.g; d[2] = o.b;
}

/* up(C)(x, y) from global memory */
__device__ __forceinline__ Bloom3 bloom_up_global(const float* __restrict__ coarse, int wc, int hc, int x, int y) {
    return bloom_up_pixel(x, y, wc, hc, [&](int, int, int cx, int cy) {
        const float* const p = coarse + 3u * ((size_t)cy * (size_t)wc + (size_t)cx);
        return Bloom3{p[0], p[1], p[2]};
    });
}

__global__ void __launch_bounds__(256) k_bloom_up_blend(float* __restrict__ fine, int wf, uint32_t n, const float* __restrict__ coarse, int wc, int hc, BloomCall e) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const int y = (int)(i / (uint32_t)wf), x = (int)(i - (uint32_t)y * (uint32_t)wf);
    const Bloom3 u = bloom_up_global(coarse, wc, hc, x, y);
    float* const d = fine + 3u * (size_t)i;
    d[0] = bloom_blend(d[0], u.r, e); d[1] = bloom_blend(d[1], u.g, e); d[2] = bloom_blend(d[2], u.b, e);
}

/* step 4 for pixel (x, y): its three input channels in, its three output channels into o */
__device__ __forceinline__ void bloom_composite_pixel(float r, float g, float b, int x, int y, const float* __restrict__ u1, int wc, int hc, BloomCall e, float* o) {
    const Bloom3 B = bloom_up_global(u1, wc, hc, x, y), P = bloom_pre(r, g, b, e);
    o[0] = bloom_composite(r, B.r, P.r, e); o[1] = bloom_composite(g, B.g, P.g, e); o[2] = bloom_composite(b, B.b, P.b, e);
}

/* the same for a pixel whose tent starts O columns into the 2 x 4 coarse pixels its group of four has fetched */
template <int O>
__device__ __forceinline__ void bloom_composite_fetched(const Bloom3 (&C)[2][4], float r, float g, float b, int x, int y, int wc, int hc, BloomCall e, float* o) {
    const Bloom3 B = bloom_up_pixel(x, y, wc, hc, [&](int i, int j, int, int) { return C[j][O + i]; }), P = bloom_pre(r, g, b, e);
    o[0] = bloom_composite(r, B.r, P.r, e); o[1] = bloom_composite(g, B.g, P.g, e); o[2] = bloom_composite(b, B.b, P.b, e);
}

__global__ void __launch_bounds__(256) k_bloom_composite(const float* __restrict__ rgb, uint32_t w, uint32_t n, const float* __restrict__ u1, int wc, int hc, BloomCall e,
                                                         float* __restrict__ out) {
    const uint32_t n4 = n >> 2, q = blockIdx.x * 256u + threadIdx.x;
    if (q < n4) {
        const float4* const p = reinterpret_cast<const float4*>(rgb) + 3u * (size_t)q;
        const float4 a = p[0], b = p[1], c = p[2];
        /* each of the four pixels has its own (x, y): a group may straddle the end of a row */
        uint32_t y = (4u * q) / w, x = 4u * q - y * w;
        float o[12];
        if (x + 3u < w) {
            /* all four in one row: their tents lie in coarse columns (x - 1) >> 1 ... + 3 of two coarse rows, fetched once (8 pixels for
             * 16); pixel t's tent starts ((x + t - 1) >> 1) - ((x - 1) >> 1) columns in: 0, 1, 1, 2 for even x and 0, 0, 1, 1 for odd x */
            const int xi = (int)x, yi = (int)y, base = (xi - 1) >> 1, y0 = (yi - 1) >> 1;
            Bloom3 C[2][4];
#pragma unroll
            for (int j = 0; j < 2; j++) {
#pragma unroll
                for (int i = 0; i < 4; i++) {
                    const float* const t = u1 + 3u * ((size_t)bloom_clampi(y0 + j, hc - 1) * (size_t)wc + (size_t)bloom_clampi(base + i, wc - 1));
                    C[j][i] = Bloom3{t[0], t[1], t[2]};
                }
            }
            if (x & 1u) {
                bloom_composite_fetched<0>(C, a.x, a.y, a.z, xi, yi, wc, hc, e, o);
                bloom_composite_fetched<0>(C, a.w, b.x, b.y, xi + 1, yi, wc, hc, e, o + 3);
                bloom_composite_fetched<1>(C, b.z, b.w, c.x, xi + 2, yi, wc, hc, e, o + 6);
                bloom_composite_fetched<1>(C, c.y, c.z, c.w, xi + 3, yi, wc, hc, e, o + 9);
            } else {
                bloom_composite_fetched<0>(C, a.x, a.y, a.z, xi, yi, wc, hc, e, o);
                bloom_composite_fetched<1>(C, a.w, b.x, b.y, xi + 1, yi, wc, hc, e, o + 3);
                bloom_composite_fetched<1>(C, b.z, b.w, c.x, xi + 2, yi, wc, hc, e, o + 6);
                bloom_composite_fetched<2>(C, c.y, c.z, c.w, xi + 3, yi, wc, hc, e, o + 9);
            }
        } else {
            bloom_composite_pixel(a.x, a.y, a.z, (int)x, (int)y, u1, wc, hc, e, o);
            if (++x == w) { x = 0u; y++; }
            bloom_composite_pixel(a.w, b.x, b.y, (int)x, (int)y, u1, wc, hc, e, o + 3);
            if (++x == w) { x = 0u; y++; }
            bloom_composite_pixel(b.z, b.w, c.x, (int)x, (int)y, u1, wc, hc, e, o + 6);
            if (++x == w) { x = 0u; y++; }
            bloom_composite_pixel(c.y, c.z, c.w, (int)x, (int)y, u1, wc, hc, e, o + 9);
        }
        float4* const d = reinterpret_cast<float4*>(out) + 3u * (size_t)q;
        d[0] = make_float4(o[0], o[1], o[2], o[3]); d[1] = make_float4(o[4], o[5], o[6], o[7]); d[2] = make_float4(o[8], o[9], o[10], o[11]);
    }
    if (q < (n & 3u)) {
        const uint32_t i = 4u * n4 + q, y = i / w, x = i - y * w;
        const float* const p = rgb + 3u * (size_t)i;
        float o[3];
        bloom_composite_pixel(p[0], p[1], p[2], (int)x, (int)y, u1, wc, hc, e, o);
        float* const d = out + 3u * (size_t)i;
        d[0] = o[0]; d[1] = o[1]; d[2] = o[2];
    }
}

/* words = 3 n floats as bit patterns: n16 16-byte groups, then the last words mod 4 */
__global__ void __launch_bounds__(256) k_bloom_copy(const uint32_t* __restrict__ src, size_t words, uint32_t* __restrict__ dst) {
    const size_t n16 = words >> 2, q = (size_t)blockIdx.x * 256u + threadIdx.x;
    if (q < n16) reinterpret_cast<uint4*>(dst)[q] = reinterpret_cast<const uint4*>(src)[q];
    if (q < (words & 3u)) dst[4u * n16 + q] = src[4u * n16 + q];
}

template <bool PRE, bool KARIS>
static void launch_down(const float* src, int ws, int hs, float* dst, int wd, int hd, const BloomCall& e, hipStream_t stream) {
    const uint32_t tiles_x = ((uint32_t)wd + kTX - 1) / kTX, tiles_y = ((uint32_t)hd + kTY - 1) / kTY;
    hipLaunchKernelGGL((k_bloom_down<PRE, KARIS>), dim3(tiles_x * tiles_y), dim3(256), 0, stream, src, ws, hs, dst, wd, hd, tiles_x, e);
}

hipError_t launch_bloom(const float* rgb, const BloomPlan& plan, const BloomCall& e, bool copy, float* out_rgb, float* workspace, hipStream_t stream) {
    const size_t n = (size_t)plan.w[0] * (size_t)plan.h[0];
    if (copy) {
        const size_t words = 3 * n;
        hipLaunchKernelGGL(k_bloom_copy, dim3((unsigned)std::max<size_t>(1, ((words >> 2) + 255) / 256)), dim3(256), 0, stream, reinterpret_cast<const uint32_t*>(rgb),
                           words, reinterpret_cast<uint32_t*>(out_rgb));
        return hipGetLastError();
    }
    auto level = [&](int k) { return workspace + plan.off[k]; };
    if (e.flags & FTN_BLOOM_KARIS) launch_down<true, true>(rgb, plan.w[0], plan.h[0], level(1), plan.w[1], plan.h[1], e, stream);
    else launch_down<true, false>(rgb, plan.w[0], plan.h[0], level(1), plan.w[1], plan.h[1], e, stream);
    for (int k = 1; k < plan.L; k++) launch_down<false, false>(level(k), plan.w[k], plan.h[k], level(k + 1), plan.w[k + 1], plan.h[k + 1], e, stream);
    for (int k = plan.L - 1; k >= 1; k--) {
        const uint32_t nk = (uint32_t)plan.w[k] * (uint32_t)plan.h[k];
        hipLaunchKernelGGL(k_bloom_up_blend, dim3((nk + 255u) / 256u), dim3(256), 0, stream, level(k), plan.w[k], nk, level(k + 1), plan.w[k + 1], plan.h[k + 1], e);
    }
    hipLaunchKernelGGL(k_bloom_composite, dim3((unsigned)std::max<size_t>(1, ((n >> 2) + 255) / 256)), dim3(256), 0, stream, rgb, (uint32_t)plan.w[0], (uint32_t)n,
                       level(1), plan.w[1], plan.h[1], e, out_rgb);
    return hipGetLastError();
}

}  // namespace ftn
