/*
 * ftn_moments.hip -- per-pixel second moments of the camera samples' radiance (include/fountain_hip_moments.h), beside the beauty.
 *
 * A unit of its own: the driver is a wavefront_render call (ftn_wavefront.h) with a per-pass hook, and k_mo_accumulate shares the
 * film context and the layout of a pass's buffers with the beauty's kernels through ftn_wf_common.h.
 */
#include "ftn_wf_common.h"
#include "ftn_moments.h"
#include <algorithm>

namespace ftn {

/* ================================================================== second moments (include/fountain_hip_moments.h)
 * wavefront_render leaves the radiance of a pass's samples in WfBuffers::rad (path id = slot * samples + s) until the next pass
 * overwrites it.  wavefront_moments hooks k_mo_accumulate behind every pass's k_wf_accumulate, on the same stream, to add the squares of
 * those samples: the beauty's kernels run exactly as in ftn_render. */

/* one sample's squares into every pixel of its box-filter footprint (film_add's rule): the own pixel in registers, others into the
 * in-tile or other-tile sum by atomics */
__device__ inline void mo_film_add(const MomentAcc& M, const FilmCtx& F, V2 p_film, float4 q, int own_x, int own_y, float4* acc) {
    const FilmFootprint fp = film_footprint(F, p_film);
    for (int y = fp.y0; y < fp.y1; y++)
        for (int x = fp.x0; x < fp.x1; x++) {
            if (x == own_x && y == own_y) { acc->x += q.x; acc->y += q.y; acc->z += q.z; acc->w += q.w; continue; }
            const bool in_tile = x >= F.sb[0] && x < F.sb[2] && y >= F.sb[1] && y < F.sb[3];
            float* f = reinterpret_cast<float*>((in_tile ? M.in_tile : M.other_tile) + film_idx(F, x, y));
            atomicAdd(f + 0, q.x); atomicAdd(f + 1, q.y); atomicAdd(f + 2, q.z); atomicAdd(f + 3, q.w);
        }
}

/* k_wf_accumulate's structure for the four squares: one thread per pixel slot adds its samples in sample order; the workgroup stages
 * MO_ACC_CHUNK samples of its 256 slots through LDS with coalesced loads.  The beauty's statistics (spill, bc_writes, NaN) are the
 * beauty kernel's: this one counts nothing. */
#define MO_ACC_CHUNK 8u
__global__ void __launch_bounds__(256) k_mo_accumulate(RenderParams P, WfBuffers W, MomentAcc M) {
    __shared__ float4 s_rad[256 * MO_ACC_CHUNK];
    const uint32_t slot = blockIdx.x * 256u + threadIdx.x;
    const FilmSlot fs = film_slot(P, W.n_slots, slot);
    const bool valid = fs.valid, in_crop = fs.in_crop; const int px = fs.px, py = fs.py; const size_t ai = fs.ai;
    float4 acc = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (in_crop) acc = M.own[ai];
    const size_t block_first = (size_t)blockIdx.x * 256u * W.samples;          /* first path of this workgroup's 256 slots */
    for (uint32_t s0 = 0; s0 < W.samples; s0 += MO_ACC_CHUNK) {
        const uint32_t n = W.samples - s0 < MO_ACC_CHUNK ? W.samples - s0 : MO_ACC_CHUNK;
        for (uint32_t e = threadIdx.x; e < 256u * n; e += 256u) {                /* n consecutive samples of slot e / n */
            const uint32_t sl = e / n, k = e - sl * n;
            const size_t p = block_first + (size_t)sl * W.samples + s0 + k;
            if (p < W.n_paths) s_rad[sl * MO_ACC_CHUNK + k] = W.rad[p];
        }
        __syncthreads();
        if (valid) {
            for (uint32_t k = 0; k < n; k++) {
                const float4 l = s_rad[threadIdx.x * MO_ACC_CHUNK + k];
                float xyz[3];
                rgb_to_xyz(Rgb(l.x, l.y, l.z), xyz);
                const float4 q = make_float4(l.x * l.x, l.y * l.y, l.z * l.z, xyz[1] * xyz[1]);
                /* the sample's film position: the first two draws of its stream, exactly as k_wf_generate made them */
                Rng crng; crng.seed(indexed_key(P.seed, px, py, W.first_sample + s0 + k));
                const V2 j = crng.next2();
                mo_film_add(M, fs.F, V2((float)px + j.x, (float)py + j.y), q, in_crop ? px : FTN_OWN_NONE, py, &acc);
            }
        }
        __syncthreads();
    }
    if (valid && in_crop) M.own[ai] = acc;
}

/* after the last pass: out += own + in-tile, then out += other-tile (the spill sums are only read when a sample left its own pixel) */
__global__ void __launch_bounds__(256) k_mo_merge(MomentAcc M, float4* __restrict__ out, size_t n, const DevStats* __restrict__ stats) {
    const bool spilled = stats->bc_writes != 0;
    for (size_t i = (size_t)blockIdx.x * 256u + threadIdx.x; i < n; i += (size_t)gridDim.x * 256u) {
        const float4 a = M.own[i], zero = make_float4(0.0f, 0.0f, 0.0f, 0.0f), b = spilled ? M.in_tile[i] : zero;
        float4 o = out[i];
        o.x += a.x + b.x; o.y += a.y + b.y; o.z += a.z + b.z; o.w += a.w + b.w;
        if (spilled) { const float4 c = M.other_tile[i]; o.x += c.x; o.y += c.y; o.z += c.z; o.w += c.w; }
        out[i] = o;
    }
}
void launch_moments_merge(const RenderParams& P, const MomentAcc& M, float4* out, hipStream_t stream) {
    const size_t n = (size_t)std::max(0, P.crop[2] - P.crop[0]) * (size_t)std::max(0, P.crop[3] - P.crop[1]);
    if (n == 0) return;
    hipLaunchKernelGGL(k_mo_merge, dim3((unsigned)std::min<size_t>((n + 255) / 256, 4096)), dim3(256), 0, stream, M, out, n, (const DevStats*)P.stats);
}

__global__ void __launch_bounds__(256) k_mo_resolve(const float* __restrict__ pix, const float* __restrict__ m, size_t n, float* __restrict__ out4) {
    for (size_t i = (size_t)blockIdx.x * 256u + threadIdx.x; i < n; i += (size_t)gridDim.x * 256u) moments_resolve_pixel(pix + 4 * i, m + 4 * i, out4 + 4 * i);
}
void launch_moments_resolve(const float* pix, const float* m, size_t n, float* out4, hipStream_t stream) {
    if (n == 0) return;
    hipLaunchKernelGGL(k_mo_resolve, dim3((unsigned)std::min<size_t>((n + 255) / 256, 4096)), dim3(256), 0, stream, pix, m, n, out4);
}

static void moments_pass(void* ctx, const RenderParams& P, const WfBuffers& W, hipStream_t stream) {
    hipLaunchKernelGGL(k_mo_accumulate, dim3((W.n_slots + 255) / 256), dim3(256), 0, stream, P, W, *static_cast<const MomentAcc*>(ctx));
}
int wavefront_moments(WavefrontState** state, const RenderParams& P, const std::vector<DTile>& tiles, bool count, bool count_production,
                      const MomentAcc& M, hipStream_t stream, WavefrontTimes* times) {
    return wavefront_render(state, P, tiles, count, stream, times, count_production, moments_pass, const_cast<MomentAcc*>(&M));
}

}  // namespace ftn
