/*
 * ftn_temporal.hip -- the kernel and device driver of temporal reprojection and accumulation (include/fountain_hip_temporal.h).  The
 * per-pixel code is ftn_temporal.h's, shared with the host twin; this file needs no scene internals and is its own translation unit.
 *
 *   k_tp_accumulate   one launch per frame, 16 x 16 pixels per workgroup over a grid-stride loop of tiles, one pixel per thread: under
 *                     small motion the four taps of a wave's pixels fall on a few neighbouring lines of the previous frame.  The frame's
 *                     constants, both cameras' matrices among them, are one kernel argument.
 */
#include "ftn_temporal.h"
#include <algorithm>

namespace ftn {

/* workgroup b of the grid-stride loop covers the 16 x 16 tile b of the image (tiles row-major).  MOTION: the frame comes with its mv8
 * (include/fountain_hip_motion.h); without it the argument is not looked at and the kernel is the static scene's */
template <bool MOTION>
__global__ void __launch_bounds__(256) k_tp_accumulate(const float* __restrict__ rgb, const float* __restrict__ gb12, const float* __restrict__ var4,
                                                       const float* __restrict__ prev_gb12, const float4* __restrict__ prev_hist, TpFrame F,
                                                       float4* __restrict__ out_hist, float* __restrict__ out_rgb, float* __restrict__ out_var4,
                                                       const float* __restrict__ mv8) {
    const uint32_t tiles_x = ((uint32_t)F.w + 15u) / 16u, n_tiles = tiles_x * (((uint32_t)F.h + 15u) / 16u);
    for (uint32_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
        const int x = (int)((t % tiles_x) * 16u + threadIdx.x), y = (int)((t / tiles_x) * 16u + threadIdx.y);
        if (x >= F.w || y >= F.h) continue;
        tp_accumulate_pixel(rgb, gb12, var4, prev_gb12, prev_hist, F, x, y, out_hist, out_rgb, out_var4, MOTION ? mv8 : nullptr);
    }
}

hipError_t launch_temporal(const float* rgb, const float* gb12, const float* var4, const float* prev_gb12, const float4* prev_hist,
                           const TpFrame& frame, float4* out_hist, float* out_rgb, float* out_var4, hipStream_t stream, const float* mv8) {
    const size_t n_tiles = (((size_t)frame.w + 15) / 16) * (((size_t)frame.h + 15) / 16);
    const unsigned grid = (unsigned)std::min<size_t>(n_tiles, 65536);
    if (mv8) hipLaunchKernelGGL(k_tp_accumulate<true>, dim3(grid), dim3(16, 16), 0, stream, rgb, gb12, var4, prev_gb12, prev_hist, frame, out_hist, out_rgb,
                                out_var4, mv8);
    else hipLaunchKernelGGL(k_tp_accumulate<false>, dim3(grid), dim3(16, 16), 0, stream, rgb, gb12, var4, prev_gb12, prev_hist, frame, out_hist, out_rgb,
                            out_var4, mv8);
    return hipGetLastError();
}

}  // namespace ftn
