/*
 * ftn_ao.hip -- the ambient-occlusion pass (include/fountain_hip_ao.h) on the wavefront pipeline.
 *
 * A unit of its own, like ftn_gbuffer.hip: the kernels are here and share ftn_wf_common.h with the beauty's; the passes and their
 * pass-through rounds are wf_first_hit_passes' (ftn_wf_internal.h, ftn_wavefront.hip), which wavefront_ao hands the launches of k_ao_shade
 * and k_ao_accumulate and, as the driver's one pass with a secondary stage, the occlusion steps between them: per step one k_ao_step and
 * one launch of the production any-hit kernels (launch_trace: the eight-box kernel for triangle-only scenes, the four-box one with spheres).
 */
#include "ftn_wf_internal.h"
#include "ftn_ao.h"
#include <algorithm>
#include <cstring>

namespace ftn {

/* ================================================================== ambient occlusion (include/fountain_hip_ao.h)
 * A path's 64-byte record (the path integrator's pd record, free in a first-hit pass), as k_ao_shade leaves it:
 *     {p, -} {p_err, flags} {n, -} {bent, count}
 * flags: AO_HIT a surface was recorded, AO_FLIP its hemisphere stands on -n.  count = -1 marks a sample without a surface, so that
 * k_ao_accumulate reads the fourth float4 alone: 16 bytes per path instead of the whole record. */
enum : uint32_t { AO_HIT = 1u, AO_FLIP = 2u };
struct AoParams {
    float* out;           /* 8 floats per crop pixel (ftn_ao_pixel), added into */
    float4 *spillA, *spillB;   /* per crop pixel, the samples whose footprint leaves their own pixel (atomics; added into out at the end):
                                * {open, bent} {hit weight, weight, -, -} */
    float4* rec;          /* 4 float4 per path (above) */
    uint32_t* hits;       /* the paths that recorded a surface, in no particular order; their number is counters[WFC_ACTIVE_B] */
    uint32_t rays; float radius;
};

/* one thread per queued ray: the hit it found is either recorded or passed through (k_gb_shade without a material lookup) */
__global__ void __launch_bounds__(256) k_ao_shade(RenderParams P, WfBuffers W, AoParams G, const uint32_t* __restrict__ q_in, const uint32_t* count_in,
                                                  uint32_t* q_out, uint32_t* count_out) {
    const DScene& S = P.S;
    const uint32_t qi = blockIdx.x * 256u + threadIdx.x;
    bool push = false, recorded = false;
    uint32_t p = 0;
    if (qi < *count_in) {
        p = q_in[qi];
        const float4 ro = W.ray[2 * (size_t)p], rdv = W.ray[2 * (size_t)p + 1];
        DRay ray0; ray0.o = V3(ro.x, ro.y, ro.z); ray0.d = V3(rdv.x, rdv.y, rdv.z); ray0.t_max = rdv.w; ray0.time = 0.0f;
        const DHit h = load_hit(W, p);
        float4 r0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), r1 = r0, r2 = r0, r3 = make_float4(0.0f, 0.0f, 0.0f, -1.0f);       /* a miss */
        if (h.prim >= 0) {
            DSI si; make_interaction(S, h, ray0, &si);
            if (si.mat < 0) {
                const DRay nr = spawn_ray(si.hit, ray0.d);
                W.ray[2 * (size_t)p] = make_float4(nr.o.x, nr.o.y, nr.o.z, 0.0f); W.ray[2 * (size_t)p + 1] = make_float4(nr.d.x, nr.d.y, nr.d.z, nr.t_max);
                push = true;
            } else {
                const uint32_t flags = AO_HIT | (ao_flipped(si.hit.n, si.wo) ? AO_FLIP : 0u);
                r0 = make_float4(si.hit.p.x, si.hit.p.y, si.hit.p.z, 0.0f);
                r1 = make_float4(si.hit.p_err.x, si.hit.p_err.y, si.hit.p_err.z, __uint_as_float(flags));
                r2 = make_float4(si.hit.n.x, si.hit.n.y, si.hit.n.z, 0.0f);
                r3 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                recorded = true;
            }
        }
        if (!push) { float4* R = G.rec + 4 * (size_t)p; R[0] = r0; R[1] = r1; R[2] = r2; R[3] = r3; }
    }
    const bool pred[2] = {push, recorded};
    const uint32_t val[2] = {p, p};
    uint32_t* const qs[2] = {q_out, G.hits};
    uint32_t* const cs[2] = {count_out, &W.counters[CTR(WFC_ACTIVE_B)]};
    block_push<2>(pred, val, qs, cs);
}

/* before every step: the any-hit queue's length, the trace kernels' queue heads and their hand-back queues (k_wf_round_reset's work) */
__global__ void __launch_bounds__(64) k_ao_step_reset(WfBuffers W) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    static_assert(WFC_HEADS_END == WFC_EXC_FIRST, "the two ranges are cleared as one");
    for (int i = WFC_HEADS_FIRST; i < WFC_EXC_END; i++) W.counters[CTR(i)] = 0;
    W.counters[CTR(WFC_SHADOW)] = 0;
}

/* Step k, one thread per recorded surface: folds the answer to ray k - 1 into the record (its direction is still in the path's shadow-ray
 * slot) and, unless k == rays, makes ray k from draws 5 + 2k and 6 + 2k of the sample's stream and queues it.  One launch per step. */
__global__ void __launch_bounds__(256) k_ao_step(RenderParams P, WfBuffers W, AoParams G, uint32_t k) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    bool push = false;
    uint32_t p = 0;
    if (i < W.counters[CTR(WFC_ACTIVE_B)]) {
        p = G.hits[i];
        float4* R = G.rec + 4 * (size_t)p;
        if (k > 0 && !W.occluded[p]) {
            const float4 d = W.sh[2 * (size_t)p + 1];
            float4 b = R[3];
            b.x += d.x; b.y += d.y; b.z += d.z; b.w += 1.0f;
            R[3] = b;
        }
        if (k < G.rays) {
            const float4 r0 = R[0], r1 = R[1], r2 = R[2];
            const uint32_t slot = p / W.samples, sidx = p % W.samples;
            const DTile tile = P.tiles[slot >> 8];
            const int px = tile.x0 + (int)(slot & 15u), py = tile.y0 + (int)((slot >> 4) & 15u);
            Rng rng; rng.seed(indexed_key(P.seed, px, py, W.first_sample + sidx));
            rng.skip(5u + 2u * k);
            const V2 u = rng.next2();
            const V3 n(r2.x, r2.y, r2.z);
            const AoRay r = ao_ray(V3(r0.x, r0.y, r0.z), V3(r1.x, r1.y, r1.z), n, ao_facing_normal(n, (__float_as_uint(r1.w) & AO_FLIP) != 0u), u);
            W.sh[2 * (size_t)p] = make_float4(r.o.x, r.o.y, r.o.z, 0.0f); W.sh[2 * (size_t)p + 1] = make_float4(r.d.x, r.d.y, r.d.z, G.radius);
            push = true;
        }
    }
    const bool pred[1] = {push};
    const uint32_t val[1] = {p};
    uint32_t* const qs[1] = {W.q_shadow};
    uint32_t* const cs[1] = {&W.counters[CTR(WFC_SHADOW)]};
    block_push<1>(pred, val, qs, cs);
}

/* one sample's sums into every pixel of its box-filter footprint (film_add): the own pixel in registers, others into the spill sums */
__device__ inline void ao_film_add(const AoParams& G, const FilmCtx& F, V2 p_film, float4 r, int own_x, int own_y, float* acc, uint32_t* spill, uint32_t* bc_writes) {
    const FilmFootprint fp = film_footprint(F, p_film);
    const bool hit = r.w >= 0.0f;
    const float v[4] = {r.w, r.x, r.y, r.z};
    int touched = 0;
    for (int y = fp.y0; y < fp.y1; y++)
        for (int x = fp.x0; x < fp.x1; x++) {
            touched++;
            if (x == own_x && y == own_y) {
                if (hit) {
#pragma unroll
                    for (int k = 0; k < 4; k++) acc[k] += v[k] * 1.0f;        /* value * filter weight (box: 1.0) */
                    acc[4] += 1.0f;
                }
                acc[5] += 1.0f;
                continue;
            }
            const size_t i = film_idx(F, x, y);
            float* a = reinterpret_cast<float*>(G.spillA + i);
            float* b = reinterpret_cast<float*>(G.spillB + i);
            if (hit) {
#pragma unroll
                for (int k = 0; k < 4; k++) atomicAdd(a + k, v[k] * 1.0f);
                atomicAdd(b, 1.0f);
            }
            atomicAdd(b + 1, 1.0f);
            (*bc_writes)++;
        }
    if (touched != 1) (*spill)++;
}

/* One thread per pixel slot adds its samples in sample order into the caller's buffer; the workgroup stages AO_ACC_CHUNK samples of its
 * 256 slots (the fourth float4 of each path's record) through LDS, consecutive threads reading consecutive paths, as k_gb_accumulate does. */
#define AO_ACC_CHUNK 8u
__global__ void __launch_bounds__(256) k_ao_accumulate(RenderParams P, WfBuffers W, AoParams G) {
    __shared__ float4 s_rec[256 * AO_ACC_CHUNK];
    const uint32_t slot = blockIdx.x * 256u + threadIdx.x;
    uint32_t spill = 0, bc = 0;
    const FilmSlot fs = film_slot(P, W.n_slots, slot);
    const bool valid = fs.valid, in_crop = fs.in_crop; const int px = fs.px, py = fs.py; const size_t ai = fs.ai;
    float acc[6];
#pragma unroll
    for (int k = 0; k < 6; k++) acc[k] = in_crop ? G.out[8 * ai + k] : 0.0f;
    const size_t block_first = (size_t)blockIdx.x * 256u * W.samples;          /* first path of this workgroup's 256 slots */
    for (uint32_t s0 = 0; s0 < W.samples; s0 += AO_ACC_CHUNK) {
        const uint32_t n = W.samples - s0 < AO_ACC_CHUNK ? W.samples - s0 : AO_ACC_CHUNK;
        for (uint32_t e = threadIdx.x; e < 256u * n; e += 256u) {                /* n consecutive samples of slot e / n */
            const uint32_t sl = e / n, k = e - sl * n;
            const size_t p = block_first + (size_t)sl * W.samples + s0 + k;
            if (p < W.n_paths) s_rec[sl * AO_ACC_CHUNK + k] = G.rec[4 * p + 3];
        }
        __syncthreads();
        if (valid) {
            for (uint32_t k = 0; k < n; k++) {
                /* the sample's film position: the first two draws of its stream, exactly as k_wf_generate made them */
                Rng crng; crng.seed(indexed_key(P.seed, px, py, W.first_sample + s0 + k));
                const V2 j = crng.next2();
                ao_film_add(G, fs.F, V2((float)px + j.x, (float)py + j.y), s_rec[threadIdx.x * AO_ACC_CHUNK + k], in_crop ? px : FTN_OWN_NONE, py, acc, &spill, &bc);
            }
        }
        __syncthreads();
    }
    if (valid && in_crop) {
#pragma unroll
        for (int k = 0; k < 6; k++) G.out[8 * ai + k] = acc[k];
    }
    if (spill) atomicAdd(&P.stats->spill_samples, (unsigned long long)spill);       /* rare */
    if (bc) atomicAdd(&P.stats->bc_writes, (unsigned long long)bc);
}

/* after the last pass: the spill sums into the caller's buffer (nothing to do when no sample left its own pixel) */
__global__ void __launch_bounds__(256) k_ao_merge(AoParams G, size_t n, const DevStats* __restrict__ stats) {
    if (stats->bc_writes == 0) return;
    for (size_t i = (size_t)blockIdx.x * 256u + threadIdx.x; i < n; i += (size_t)gridDim.x * 256u) {
        const float4 a = G.spillA[i], b = G.spillB[i];
        if (b.y == 0.0f) continue;
        const float add[6] = {a.x, a.y, a.z, a.w, b.x, b.y};
#pragma unroll
        for (int k = 0; k < 6; k++) G.out[8 * i + k] += add[k];
    }
}

__global__ void __launch_bounds__(256) k_ao_resolve(const float* __restrict__ in, size_t n, uint32_t rays, float* __restrict__ out6) {
    for (size_t i = (size_t)blockIdx.x * 256u + threadIdx.x; i < n; i += (size_t)gridDim.x * 256u) ao_resolve_pixel(in + 8 * i, rays, out6 + 6 * i);
}
void launch_ao_resolve(const float* in, size_t n, uint32_t rays, float* out6, hipStream_t stream) {
    if (n == 0) return;
    const unsigned grid = (unsigned)std::min<size_t>((n + 255) / 256, 4096);
    hipLaunchKernelGGL(k_ao_resolve, dim3(grid), dim3(256), 0, stream, in, n, rays, out6);
}

int wavefront_ao(WavefrontState** state, const RenderParams& P, const std::vector<DTile>& tiles, uint32_t rays, float radius, int count_mode, float* d_out,
                 float4* spill_a, float4* spill_b, hipStream_t stream, double* trace_ms_out, AoTimes* times) {
    AoParams G;
    G.out = d_out; G.spillA = spill_a; G.spillB = spill_b; G.rec = nullptr; G.hits = nullptr; G.rays = rays; G.radius = radius;
    double any_ms = 0.0; unsigned long long any_launches = 0;
    WfFirstHitPass pass;
    pass.what = "the ambient occlusion";
    /* the path integrator's 64-byte records; the list of recorded surfaces in q_active[1], whose count k_wf_reset starts every pass at zero
     * (q_active[0] is as free, but its count starts at the number of camera samples) */
    pass.setup = [&](WavefrontState* st, uint32_t) { G.rec = st->pd; G.hits = st->W.q_active[1]; return FTN_OK; };
    pass.shade = [&](const WfBuffers& W, const uint32_t* q_in, const uint32_t* count_in, uint32_t* q_out, uint32_t* count_out, dim3 grid, hipStream_t sm) {
        hipLaunchKernelGGL(k_ao_shade, grid, dim3(256), 0, sm, P, W, G, q_in, count_in, q_out, count_out);
    };
    pass.secondary = [&](WavefrontState* st, const WfBuffers& W, size_t lds, unsigned trace_grid_max, hipStream_t sm) -> int {
        const uint32_t n_hit = st->host_counters[CTR(WFC_ACTIVE_B)];      /* the driver's last poll: behind the last shade launch of the pass */
        if (n_hit == 0) return FTN_OK;
        const dim3 grid((n_hit + 255) / 256);
        const unsigned tg = std::min<unsigned>(trace_grid_max, (2 * W.n_paths + 255) / 256);
        const bool spheres = P.S.n_spheres != 0;
        int pending = 0;                                                  /* event pairs recorded and not yet read: ev[2 i], ev[2 i + 1] */
        auto collect = [&]() -> int {
            if (pending == 0) return FTN_OK;
            WF_TRY(hipEventSynchronize(st->ev[2 * pending - 1]));
            for (int i = 0; i < pending; i++) { float ms = 0.0f; (void)hipEventElapsedTime(&ms, st->ev[2 * i], st->ev[2 * i + 1]); any_ms += ms; }
            pending = 0;
            return FTN_OK;
        };
        for (uint32_t k = 0; k <= rays; k++) {
            hipLaunchKernelGGL(k_ao_step_reset, dim3(1), dim3(64), 0, sm, W);
            hipLaunchKernelGGL(k_ao_step, grid, dim3(256), 0, sm, P, W, G, k);
            if (k == rays) break;                                         /* the last step only folds */
            WF_TRY(hipEventRecord(st->ev[2 * pending], sm));
            launch_trace(st, true, count_mode, spheres, tg, lds, sm, P, W, W.q_shadow, &W.counters[CTR(WFC_SHADOW)], &W.counters[CTR(WFC_HEAD_ANY)], n_hit);
            WF_TRY(hipEventRecord(st->ev[2 * pending + 1], sm));
            any_launches++;
            if (++pending == 32) { const int rc = collect(); if (rc) return rc; }
        }
        return collect();
    };
    pass.accumulate = [&](const WfBuffers& W, dim3 grid, hipStream_t sm) { hipLaunchKernelGGL(k_ao_accumulate, grid, dim3(256), 0, sm, P, W, G); };
    const int rc = wf_first_hit_passes(state, P, tiles, pass, stream, trace_ms_out);
    if (times) { times->any_ms = any_ms; times->any_launches = any_launches; }
    if (rc || !G.rec) return rc;          /* (no record buffer: no tiles or no samples, nothing was launched) */
    const size_t npix = (size_t)std::max(0, P.crop[2] - P.crop[0]) * (size_t)std::max(0, P.crop[3] - P.crop[1]);
    if (npix) hipLaunchKernelGGL(k_ao_merge, dim3((unsigned)std::min<size_t>((npix + 255) / 256, 4096)), dim3(256), 0, stream, G, npix, (const DevStats*)P.stats);
    WF_TRY(hipGetLastError());
    return FTN_OK;
}

}  // namespace ftn
