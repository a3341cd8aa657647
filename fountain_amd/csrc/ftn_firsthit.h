/*
 * ftn_firsthit.h -- the device code the first-hit passes share under wf_first_hit_passes (ftn_wf_internal.h): ftn_gbuffer.hip,
 * ftn_idmatte.hip, ftn_ao.hip, ftn_motion.hip and ftn_lightpass.hip include it, nothing else does.
 *
 *   the shade prologue   fh_first_hit: what the closest-hit trace found for a path -- nothing, a null material (the ray is spawned on
 *                        and the caller pushes the path), or the surface the pass records; fh_sample: a path's pixel and sample index
 *   the film of sums     fh_film_add, k_fh_accumulate, k_fh_merge and fh_merge for the four passes whose output is per-pixel float sums
 *                        (the mattes keep tables and a foreign list of their own); a pass describes itself with a traits type (below)
 *   small kernels        k_fh_shadow_reset before a launch of the any-hit kernels, fh_per_pixel under the resolve entries
 */
#ifndef FTN_FIRSTHIT_H
#define FTN_FIRSTHIT_H
#include "ftn_wf_internal.h"
#include <algorithm>

namespace ftn {

/* the crop window's pixel count (ftn_stage_host.h has the host files' twin over a ftn_film_desc) */
inline size_t fh_crop_pixels(const RenderParams& P) { return (size_t)std::max(0, P.crop[2] - P.crop[0]) * (size_t)std::max(0, P.crop[3] - P.crop[1]); }

/* ================================================================== the shade prologue */
/* pixel and sample index of path p: 256 slots per tile (x = slot & 15, y = (slot >> 4) & 15), W.samples paths per slot */
struct FhSample { int px, py; uint32_t sample; };
__device__ inline FhSample fh_sample(const RenderParams& P, const WfBuffers& W, uint32_t p) {
    const uint32_t slot = p / W.samples, sidx = p % W.samples;
    const DTile tile = P.tiles[slot >> 8];
    return FhSample{tile.x0 + (int)(slot & 15u), tile.y0 + (int)((slot >> 4) & 15u), W.first_sample + sidx};
}

/* Path p of this round.  FH_MISS: the ray left the scene (nothing else is set).  FH_THROUGH: it hit a null material; the ray spawned on
 * along the same direction (path.rs:77-80) stands in W.ray and the caller pushes p into the next round's queue.  FH_SURFACE: *ray0, *h and
 * *si describe the first surface with a material.  The ray is loaded only for a hit */
enum FhHit { FH_MISS, FH_THROUGH, FH_SURFACE };
__device__ inline FhHit fh_first_hit(const DScene& S, const WfBuffers& W, uint32_t p, DRay* ray0, DHit* h, DSI* si) {
    *h = load_hit(W, p);
    if (h->prim < 0) return FH_MISS;
    const float4 ro = W.ray[2 * (size_t)p], rdv = W.ray[2 * (size_t)p + 1];
    ray0->o = V3(ro.x, ro.y, ro.z); ray0->d = V3(rdv.x, rdv.y, rdv.z); ray0->t_max = rdv.w; ray0->time = 0.0f;
    make_interaction(S, *h, *ray0, si);
    if (si->mat >= 0) return FH_SURFACE;
    const DRay nr = spawn_ray(si->hit, ray0->d);
    W.ray[2 * (size_t)p] = make_float4(nr.o.x, nr.o.y, nr.o.z, 0.0f); W.ray[2 * (size_t)p + 1] = make_float4(nr.d.x, nr.d.y, nr.d.z, nr.t_max);
    return FH_THROUGH;
}

/* ================================================================== the film of sums
 * A pass's traits type T:
 *   OUT      floats per crop pixel in the caller's buffer
 *   SUMS     how many of them the pass adds into, the first ones: values ..., hit weight, weight
 *   REC      float4s staged per path, CHUNK samples of a slot staged at a time (256 * CHUNK * REC float4 of LDS)
 *   load(G, W, p, j)          staged float4 j of path p
 *   unpack(r, v, &adds)       the staged record r -> whether the sample has a surface, its SUMS - 2 values, and in bit k of adds whether
 *                             this sample adds value k at all: a value that is not added stays not added (no + 0.0f), in the pixel's
 *                             registers and in the spill atomics alike */
struct FhFilm {
    float* out;           /* T::OUT floats per crop pixel, added into */
    float4* spill[3];     /* per crop pixel, the samples whose footprint leaves their own pixel (atomics; added into out at the end): sum k in
                           * component k & 3 of plane k >> 2; zero before the call, left non-zero where P.stats->bc_writes says so */
    float4* rec;          /* the per-path records: the path integrator's 64-byte pd records, free in a first-hit pass (set by the pass's setup) */
};
inline FhFilm fh_film(const RenderParams& P, float* d_out) { return FhFilm{d_out, {P.accA, P.accB, P.accC}, nullptr}; }
__device__ inline float* fh_spill(const FhFilm& G, size_t i, int k) { return reinterpret_cast<float*>(G.spill[k >> 2] + i) + (k & 3); }

/* one sample's record into every pixel of its box-filter footprint (film_add): the own pixel in registers, others into the spill sums */
template <class T>
__device__ inline void fh_film_add(const FhFilm& G, const FilmCtx& F, V2 p_film, const float4* r, int own_x, int own_y, float* acc, uint32_t* spill, uint32_t* bc_writes) {
    constexpr int NV = T::SUMS - 2;
    const FilmFootprint fp = film_footprint(F, p_film);
    float v[NV]; uint32_t adds = 0;
    const bool hit = T::unpack(r, v, &adds);
    int touched = 0;
    for (int y = fp.y0; y < fp.y1; y++)
        for (int x = fp.x0; x < fp.x1; x++) {
            touched++;
            if (x == own_x && y == own_y) {
                if (hit) {
#pragma unroll
                    for (int k = 0; k < NV; k++)
                        if (adds & (1u << k)) acc[k] += v[k] * 1.0f;        /* value * filter weight (box: 1.0) */
                    acc[NV] += 1.0f;
                }
                acc[NV + 1] += 1.0f;
                continue;
            }
            const size_t i = film_idx(F, x, y);
            if (hit) {
#pragma unroll
                for (int k = 0; k < NV; k++)
                    if (adds & (1u << k)) atomicAdd(fh_spill(G, i, k), v[k] * 1.0f);
                atomicAdd(fh_spill(G, i, NV), 1.0f);
            }
            atomicAdd(fh_spill(G, i, NV + 1), 1.0f);
            (*bc_writes)++;
        }
    if (touched != 1) (*spill)++;
}

/* One thread per pixel slot adds its samples in sample order into the caller's buffer; the workgroup stages T::CHUNK samples of its 256
 * slots (T::REC float4 each, the consecutive ones of a slot read by consecutive threads) through LDS, as k_wf_accumulate does. */
template <class T>
__global__ void __launch_bounds__(256) k_fh_accumulate(RenderParams P, WfBuffers W, FhFilm G) {
    constexpr uint32_t C = T::CHUNK, N = T::REC;
    __shared__ float4 s_rec[256 * C * N];
    const uint32_t slot = blockIdx.x * 256u + threadIdx.x;
    uint32_t spill = 0, bc = 0;
    const FilmSlot fs = film_slot(P, W.n_slots, slot);
    const bool valid = fs.valid, in_crop = fs.in_crop; const int px = fs.px, py = fs.py; const size_t ai = fs.ai;
    float acc[T::SUMS];
#pragma unroll
    for (int k = 0; k < T::SUMS; k++) acc[k] = in_crop ? G.out[T::OUT * ai + k] : 0.0f;
    const size_t block_first = (size_t)blockIdx.x * 256u * W.samples;          /* first path of this workgroup's 256 slots */
    for (uint32_t s0 = 0; s0 < W.samples; s0 += C) {
        const uint32_t n = W.samples - s0 < C ? W.samples - s0 : C;
        for (uint32_t e = threadIdx.x; e < 256u * N * n; e += 256u) {          /* the N n consecutive float4 of slot e / (N n) */
            const uint32_t sl = e / (N * n), kn = e - sl * N * n;
            const size_t p = block_first + (size_t)sl * W.samples + s0 + kn / N;
            /* (a slot outside its tile has no path: its record is whatever an earlier pass left, and nothing reads what is staged for it) */
            if (p < W.n_paths) s_rec[sl * C * N + kn] = T::load(G, W, p, kn % N);
        }
        __syncthreads();
        if (valid) {
            for (uint32_t k = 0; k < n; k++) {
                /* the sample's film position: the first two draws of its stream, exactly as k_wf_generate made them */
                Rng crng; crng.seed(indexed_key(P.seed, px, py, W.first_sample + s0 + k));
                const V2 j = crng.next2();
                fh_film_add<T>(G, fs.F, V2((float)px + j.x, (float)py + j.y), &s_rec[(threadIdx.x * C + k) * N], in_crop ? px : FTN_OWN_NONE, py, acc, &spill, &bc);
            }
        }
        __syncthreads();
    }
    if (valid && in_crop) {
#pragma unroll
        for (int k = 0; k < T::SUMS; k++) G.out[T::OUT * ai + k] = acc[k];
    }
    if (spill) atomicAdd(&P.stats->spill_samples, (unsigned long long)spill);       /* rare */
    if (bc) atomicAdd(&P.stats->bc_writes, (unsigned long long)bc);
}

/* after the last pass: the spill sums into the caller's buffer (nothing to do when no sample left its own pixel) */
__device__ inline float fh_component(const float4& v, int c) { return c == 0 ? v.x : c == 1 ? v.y : c == 2 ? v.z : v.w; }
template <class T>
__global__ void __launch_bounds__(256) k_fh_merge(FhFilm G, size_t n, const DevStats* __restrict__ stats) {
    constexpr int PLANES = (T::SUMS + 3) / 4;
    if (stats->bc_writes == 0) return;
    for (size_t i = (size_t)blockIdx.x * 256u + threadIdx.x; i < n; i += (size_t)gridDim.x * 256u) {
        float4 s[PLANES];
#pragma unroll
        for (int j = 0; j < PLANES; j++) s[j] = G.spill[j][i];
        if (fh_component(s[(T::SUMS - 1) >> 2], (T::SUMS - 1) & 3) == 0.0f) continue;          /* the weight: no sample reached this pixel from another */
#pragma unroll
        for (int k = 0; k < T::SUMS; k++) G.out[T::OUT * i + k] += fh_component(s[k >> 2], k & 3);
    }
}

/* What follows wf_first_hit_passes (rc: its status) in a pass with a film of sums: the merge, unless the call failed or launched nothing
 * (no record buffer: no tiles or no samples) */
template <class T>
__attribute__((visibility("hidden"))) int fh_merge(int rc, const RenderParams& P, const FhFilm& G, hipStream_t stream) {
    if (rc || !G.rec) return rc;
    const size_t npix = fh_crop_pixels(P);
    if (npix) hipLaunchKernelGGL(k_fh_merge<T>, dim3((unsigned)std::min<size_t>((npix + 255) / 256, 4096)), dim3(256), 0, stream, G, npix, (const DevStats*)P.stats);
    WF_TRY(hipGetLastError());
    return FTN_OK;
}

/* ================================================================== small kernels */
/* before a launch of the any-hit kernels from a pass's secondary stage: the trace kernels' queue heads and their hand-back queues
 * (k_wf_round_reset's work), and the any-hit queue's length -- 0 where a kernel pushes the rays behind this, their number where they are
 * copied in */
static __global__ void __launch_bounds__(64) k_fh_shadow_reset(WfBuffers W, uint32_t n_shadow) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    static_assert(WFC_HEADS_END == WFC_EXC_FIRST, "the two ranges are cleared as one");
    for (int i = WFC_HEADS_FIRST; i < WFC_EXC_END; i++) W.counters[CTR(i)] = 0;
    W.counters[CTR(WFC_SHADOW)] = n_shadow;
}

/* f(i) for every i < n, one thread per element over a grid-stride loop: the resolve entries' launcher.  f: a struct of the pointers with
 * a __device__ operator()(size_t) */
template <class F>
__global__ void __launch_bounds__(256) k_fh_per_pixel(size_t n, F f) {
    for (size_t i = (size_t)blockIdx.x * 256u + threadIdx.x; i < n; i += (size_t)gridDim.x * 256u) f(i);
}
template <class F>
__attribute__((visibility("hidden"))) hipError_t fh_per_pixel(size_t n, hipStream_t stream, F f) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_fh_per_pixel<F>, dim3((unsigned)std::min<size_t>((n + 255) / 256, 4096)), dim3(256), 0, stream, n, f);
    return hipGetLastError();
}

}  // namespace ftn
#endif
