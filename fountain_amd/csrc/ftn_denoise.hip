/*
 * ftn_denoise.hip -- the kernels and device driver of the a-trous denoiser (include/fountain_hip_denoise.h).  The per-pixel math is
 * ftn_denoise.h's, shared with the host twin; this file needs no scene internals and is its own translation unit.
 *
 *   k_dn_prepare   one thread per pixel: demodulated colour {u, m} and the features {n, c}, {x, z}, each one float4 store
 *   k_dn_atrous    one launch per level, 16 x 16 pixels per workgroup, one pixel per thread; colour ping-pongs between two workspace
 *                  buffers, and the last level writes out_rgb remodulated.  A template on the level's constants: DnLevel for ftn_denoise,
 *                  DnGuidedLevel for ftn_denoise_guided (include/fountain_hip_denoise_guided.h), whose colour buffers hold {u, nu}
 *   k_dng_prepare  k_dn_prepare for the guided filter: {u, nu} from rgb, gb12 and var4
 */
#include "ftn_denoise.h"
#include <algorithm>

namespace ftn {

__global__ void __launch_bounds__(256) k_dn_prepare(const float* __restrict__ rgb, const float* __restrict__ gb12, size_t n, uint32_t flags,
                                                    float albedo_eps, float4* __restrict__ col, float4* __restrict__ fnc, float4* __restrict__ fxz) {
    for (size_t i = (size_t)blockIdx.x * 256u + threadIdx.x; i < n; i += (size_t)gridDim.x * 256u)
        dn_prepare_pixel(rgb + 3 * i, gb12 + 12 * i, flags, albedo_eps, col + i, fnc + i, fxz + i);
}

__global__ void __launch_bounds__(256) k_dng_prepare(const float* __restrict__ rgb, const float* __restrict__ gb12, const float* __restrict__ var4,
                                                     size_t n, uint32_t flags, float albedo_eps, float4* __restrict__ col, float4* __restrict__ fnc,
                                                     float4* __restrict__ fxz) {
    for (size_t i = (size_t)blockIdx.x * 256u + threadIdx.x; i < n; i += (size_t)gridDim.x * 256u)
        dn_guided_prepare_pixel(rgb + 3 * i, gb12 + 12 * i, var4 + 4 * i, flags, albedo_eps, col + i, fnc + i, fxz + i);
}

/* workgroup b of the grid-stride loop covers the 16 x 16 tile b of the image (tiles row-major); out_rgb != null on the last level */
template <class Level>
__global__ void __launch_bounds__(256) k_dn_atrous(const float4* __restrict__ col_in, const float4* __restrict__ fnc, const float4* __restrict__ fxz,
                                                   int w, int h, Level L, float4* __restrict__ col_out, const float* __restrict__ gb12,
                                                   uint32_t flags, float albedo_eps, float* __restrict__ out_rgb) {
    const uint32_t tiles_x = ((uint32_t)w + 15u) / 16u, n_tiles = tiles_x * (((uint32_t)h + 15u) / 16u);
    for (uint32_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
        const int x = (int)((t % tiles_x) * 16u + threadIdx.x), y = (int)((t / tiles_x) * 16u + threadIdx.y);
        if (x >= w || y >= h) continue;
        const float4 u = dn_atrous_pixel(col_in, fnc, fxz, w, h, x, y, L);
        const size_t p = (size_t)y * (size_t)w + (size_t)x;
        if (out_rgb) dn_finish_pixel(u, gb12 + 12 * p, flags, albedo_eps, out_rgb + 3 * p);
        else col_out[p] = u;
    }
}

/* the levels launches of both filters, after their prepare kernel has filled col[0], fnc and fxz */
template <class Params, class MakeLevel>
static void launch_levels(const float* gb12, int w, int h, const Params& params, MakeLevel make_level, float* out_rgb, float4* workspace,
                          hipStream_t stream) {
    const size_t n = (size_t)w * (size_t)h;
    float4 *col[2] = {workspace, workspace + n}, *fnc = workspace + 2 * n, *fxz = workspace + 3 * n;
    const size_t n_tiles = (((size_t)w + 15) / 16) * (((size_t)h + 15) / 16);
    const unsigned grid_a = (unsigned)std::min<size_t>(n_tiles, 65536);
    for (int i = 0; i < params.levels; i++) {
        const bool last = i == params.levels - 1;
        hipLaunchKernelGGL(k_dn_atrous, dim3(grid_a), dim3(16, 16), 0, stream, (const float4*)col[i & 1], (const float4*)fnc, (const float4*)fxz,
                           w, h, make_level(params, i), col[(i + 1) & 1], gb12, params.flags, params.albedo_eps, last ? out_rgb : nullptr);
    }
}

static unsigned prepare_grid(size_t n) { return (unsigned)std::min<size_t>((n + 255) / 256, 65536); }

hipError_t launch_denoise(const float* rgb, const float* gb12, int w, int h, const ftn_denoise_params& params, float* out_rgb,
                          float4* workspace, hipStream_t stream) {
    const size_t n = (size_t)w * (size_t)h;
    if (params.levels == 0) return hipMemcpyAsync(out_rgb, rgb, 3 * n * sizeof(float), hipMemcpyDeviceToDevice, stream);
    hipLaunchKernelGGL(k_dn_prepare, dim3(prepare_grid(n)), dim3(256), 0, stream, rgb, gb12, n, params.flags, params.albedo_eps, workspace,
                       workspace + 2 * n, workspace + 3 * n);
    launch_levels(gb12, w, h, params, dn_level, out_rgb, workspace, stream);
    return hipGetLastError();
}

hipError_t launch_denoise_guided(const float* rgb, const float* gb12, const float* var4, int w, int h, const ftn_denoise_guided_params& params,
                                 float* out_rgb, float4* workspace, hipStream_t stream) {
    const size_t n = (size_t)w * (size_t)h;
    if (params.levels == 0) return hipMemcpyAsync(out_rgb, rgb, 3 * n * sizeof(float), hipMemcpyDeviceToDevice, stream);
    hipLaunchKernelGGL(k_dng_prepare, dim3(prepare_grid(n)), dim3(256), 0, stream, rgb, gb12, var4, n, params.flags, params.albedo_eps, workspace,
                       workspace + 2 * n, workspace + 3 * n);
    launch_levels(gb12, w, h, params, dn_guided_level, out_rgb, workspace, stream);
    return hipGetLastError();
}

}  // namespace ftn
