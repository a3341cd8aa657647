/*
 * ftn_vectorblur.hip -- the kernels and the device driver of the vector-blur stage (include/fountain_hip_vectorblur.h).  The per-pixel
 * code is ftn_vectorblur.h's, shared with the host twin; this file needs no scene internals and is its own translation unit.  Every kernel
 * is a gather: a thread writes what it owns from what it reads, with no atomics, so nothing depends on the launch shape.
 *
 *   k_vb_velocity_tilemax  steps 1 and 2 in one pass, a workgroup of 256 per 16 x 16 tile and a thread per pixel: the thread writes its
 *                          pixel's record, then the workgroup reduces (key, pixel index) in LDS by vb_before, a total order, so the
 *                          tree's shape does not matter; threads beyond a clipped tile's edge enter with key -1, below every pixel's.
 *   k_vb_neighbour         step 3, a thread per tile over its up-to-nine neighbours
 *   k_vb_gather            step 4, a workgroup per tile and a thread per pixel.  The tile's tap offsets are computed once, by its first
 *                          `taps` threads, into LDS.  Every tap of the tile is the tile shifted by one offset, so a wave's loads are
 *                          four rows of 16 consecutive pixels, 192 bytes of colour and 256 bytes of records each, and neighbouring
 *                          taps and tiles find each other's lines in the caches.  The taps are read from global memory: staging the
 *                          box the taps sweep (at most 48 x 48 pixels, five planes of LDS) was built and measured, and was slower
 *                          at every tap count.
 */
#include "ftn_vectorblur.h"

namespace ftn {

constexpr int kT = FTN_VB_TILE;
static_assert(kT * kT == 256, "one pixel per thread");

__global__ void __launch_bounds__(256) k_vb_velocity_tilemax(const float2* __restrict__ motion2, const float* __restrict__ gb12, int w, int h, uint32_t tiles_x, VbCall e,
                                                             VbRec* __restrict__ recs, VbRec* __restrict__ tile_recs) {
    __shared__ float s_key[256];
    __shared__ uint32_t s_idx[256];
    const uint32_t tile_y = blockIdx.x / tiles_x, tile_x = blockIdx.x - tile_y * tiles_x;
    const int x = (int)tile_x * kT + (int)(threadIdx.x & (kT - 1)), y = (int)tile_y * kT + (int)(threadIdx.x / kT);
    float key = -1.0f;
    uint32_t idx = 0xffffffffu;
    VbRec r = {0.0f, 0.0f, 0.0f, 0.0f};
    if (x < w && y < h) {
        idx = (uint32_t)y * (uint32_t)w + (uint32_t)x;
        const float2 m = motion2[idx];
        const float z = gb12 ? vb_depth(gb12[12u * (size_t)idx + 9u], gb12[12u * (size_t)idx + 10u]) : 0.0f;
        r = vb_velocity(m.x, m.y, z, e);
        recs[idx] = r;
        key = vb_key(r);
    }
    s_key[threadIdx.x] = key; s_idx[threadIdx.x] = idx;
    __syncthreads();
    for (uint32_t step = 128u; step > 0u; step >>= 1) {
        if (threadIdx.x < step) {
            const float k2 = s_key[threadIdx.x + step];
            const uint32_t i2 = s_idx[threadIdx.x + step];
            if (vb_before(k2, i2, s_key[threadIdx.x], s_idx[threadIdx.x])) { s_key[threadIdx.x] = k2; s_idx[threadIdx.x] = i2; }
        }
        __syncthreads();
    }
    /* the winner writes its tile's record from its own pixel's (every tile has a pixel, so s_idx[0] is one) */
    if (idx == s_idx[0]) tile_recs[blockIdx.x] = VbRec{r.x, r.y, key, 0.0f};
}

__global__ void __launch_bounds__(256) k_vb_neighbour(const VbRec* __restrict__ tile_recs, int tiles_x, int tiles_y, uint32_t tiles, VbRec* __restrict__ nb_recs) {
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t >= tiles) return;
    const int ty = (int)(t / (uint32_t)tiles_x), tx = (int)(t - (uint32_t)ty * (uint32_t)tiles_x);
    VbRec best = tile_recs[t];
    uint32_t best_i = t;
    for (int j = -1; j <= 1; j++) {
        for (int i = -1; i <= 1; i++) {
            const int nx = tx + i, ny = ty + j;
            if (nx < 0 || ny < 0 || nx >= tiles_x || ny >= tiles_y) continue;
            const uint32_t ti = (uint32_t)ny * (uint32_t)tiles_x + (uint32_t)nx;
            const VbRec r = tile_recs[ti];
            if (vb_before(r.l, ti, best.l, best_i)) { best = r; best_i = ti; }
        }
    }
    nb_recs[t] = best;
}

__global__ void __launch_bounds__(256) k_vb_gather(const float* __restrict__ rgb, const VbRec* __restrict__ recs, const VbRec* __restrict__ nb_recs, int w, int h,
                                                   uint32_t tiles_x, VbCall e, float* __restrict__ out) {
    __shared__ VbOffset s_off[FTN_VECTORBLUR_MAX_TAPS];
    const uint32_t tile_y = blockIdx.x / tiles_x, tile_x = blockIdx.x - tile_y * tiles_x;
    const VbRec n = nb_recs[blockIdx.x];
    if (n.l > 0.25f && (int)threadIdx.x < e.taps) s_off[threadIdx.x] = vb_offset((int)threadIdx.x, e.taps, n);      /* (read only where n.l > 0.25) */
    __syncthreads();
    const int x = (int)tile_x * kT + (int)(threadIdx.x & (kT - 1)), y = (int)tile_y * kT + (int)(threadIdx.x / kT);
    if (x >= w || y >= h) return;
    const Vb3 o = vb_gather_pixel(x, y, w, h, n, s_off, e,
                                  [&](int qx, int qy) { const float* const p = rgb + 3u * ((size_t)qy * (size_t)w + (size_t)qx); return Vb3{p[0], p[1], p[2]}; },
                                  [&](int qx, int qy) { return recs[(size_t)qy * (size_t)w + (size_t)qx]; });
    float* const d = out + 3u * ((size_t)y * (size_t)w + (size_t)x);
    d[0] = o.r; d[1] = o.g; d[2] = o.b;
}

hipError_t launch_vectorblur(const float* rgb, const float* motion2, const float* gb12, const VbPlan& plan, const VbCall& e, float* out_rgb, VbRec* workspace,
                             hipStream_t stream) {
    const uint32_t tiles = (uint32_t)plan.tiles_x * (uint32_t)plan.tiles_y;
    VbRec* const tile_recs = workspace + plan.tile_off;
    VbRec* const nb_recs = workspace + plan.nb_off;
    hipLaunchKernelGGL(k_vb_velocity_tilemax, dim3(tiles), dim3(256), 0, stream, reinterpret_cast<const float2*>(motion2), gb12, plan.w, plan.h, (uint32_t)plan.tiles_x, e,
                       workspace, tile_recs);
    hipLaunchKernelGGL(k_vb_neighbour, dim3((tiles + 255u) / 256u), dim3(256), 0, stream, tile_recs, plan.tiles_x, plan.tiles_y, tiles, nb_recs);
    hipLaunchKernelGGL(k_vb_gather, dim3(tiles), dim3(256), 0, stream, rgb, workspace, nb_recs, plan.w, plan.h, (uint32_t)plan.tiles_x, e, out_rgb);
    return hipGetLastError();
}

}  // namespace ftn
