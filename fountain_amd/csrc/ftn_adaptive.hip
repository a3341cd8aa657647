/*
 * ftn_adaptive.hip -- the device side of per-tile adaptive sampling (include/fountain_hip_adaptive.h): the per-round decision and the
 * per-pixel sample counts.  The rounds themselves are wavefront_moments calls over the active tiles.
 *
 * A unit of its own: of the pipeline it needs only RenderParams, DTile and MomentAcc.
 */
#include "ftn_adaptive.h"

namespace ftn {

/* ================================================================== the decision after a round
 * k_wf_accumulate's slot layout: one workgroup per active tile, one thread per pixel slot (x = slot & 15, y = slot >> 4).  Each thread
 * forms the ftn_pixel and ftn_moment_pixel that k_film_resolve and k_mo_merge would write into zero buffers now (adaptive_pixel_sums)
 * and applies the criterion; slots outside the tile or the crop vote yes.  The workgroup's AND is the tile's flag.  96 bytes read per
 * pixel when a sample spilled (six float4), 32 otherwise; no scratch, no atomics. */
__global__ void __launch_bounds__(256) k_ad_tile_converged(RenderParams P, MomentAcc M, const DTile* __restrict__ tiles, float t, float a,
                                                           uint8_t* __restrict__ flags) {
    const DTile tile = tiles[blockIdx.x];
    const int px = tile.x0 + (int)(threadIdx.x & 15u), py = tile.y0 + (int)(threadIdx.x >> 4);
    int ok = 1;
    if (px < tile.x1 && py < tile.y1 && px >= P.crop[0] && px < P.crop[2] && py >= P.crop[1] && py < P.crop[3]) {
        const size_t i = (size_t)(py - P.crop[1]) * (size_t)(P.crop[2] - P.crop[0]) + (size_t)(px - P.crop[0]);
        const bool spilled = P.stats->bc_writes != 0;
        const float4 zero = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        float pix[4], m[4];
        adaptive_pixel_sums(P.accA[i], spilled ? P.accB[i] : zero, spilled ? P.accC[i] : zero,
                            M.own[i], spilled ? M.in_tile[i] : zero, spilled ? M.other_tile[i] : zero, spilled, pix, m);
        ok = adaptive_pixel_converged(pix, m, t, a) ? 1 : 0;
    }
    ok = __syncthreads_and(ok);
    if (threadIdx.x == 0) flags[blockIdx.x] = (uint8_t)(ok ? 1u : 0u);
}
void launch_adaptive_decide(const RenderParams& P, const MomentAcc& M, const DTile* tiles, uint32_t n, float t, float a, uint8_t* flags, hipStream_t stream) {
    if (n == 0) return;
    hipLaunchKernelGGL(k_ad_tile_converged, dim3(n), dim3(256), 0, stream, P, M, tiles, t, a, flags);
}

/* ================================================================== the final per-pixel counts: one workgroup per tile, one thread per slot */
__global__ void __launch_bounds__(256) k_ad_counts(const DTile* __restrict__ tiles, const uint32_t* __restrict__ counts, int cx0, int cy0, int cx1,
                                                   int cy1, uint32_t* __restrict__ out) {
    const DTile tile = tiles[blockIdx.x];
    const int px = tile.x0 + (int)(threadIdx.x & 15u), py = tile.y0 + (int)(threadIdx.x >> 4);
    if (px < tile.x1 && py < tile.y1 && px >= cx0 && px < cx1 && py >= cy0 && py < cy1)
        out[(size_t)(py - cy0) * (size_t)(cx1 - cx0) + (size_t)(px - cx0)] = counts[blockIdx.x];
}
void launch_adaptive_counts(const RenderParams& P, const DTile* tiles, const uint32_t* counts, uint32_t n, uint32_t* out, hipStream_t stream) {
    if (n == 0) return;
    hipLaunchKernelGGL(k_ad_counts, dim3(n), dim3(256), 0, stream, tiles, counts, P.crop[0], P.crop[1], P.crop[2], P.crop[3], out);
}

}  // namespace ftn
