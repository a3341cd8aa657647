/*
 * ftn_ao.hip -- the ambient-occlusion pass (include/fountain_hip_ao.h) on the wavefront pipeline.
 *
 * A unit of its own, like ftn_gbuffer.hip: k_ao_shade and k_ao_step are here and share ftn_wf_common.h with the beauty's kernels; the passes
 * and their pass-through rounds are wf_first_hit_passes' (ftn_wf_internal.h, ftn_wavefront.hip), which wavefront_ao hands the launches of
 * k_ao_shade and of the shared film's accumulate kernel (ftn_firsthit.h) for AoFilm and, as a pass with a secondary stage, the occlusion
 * steps between them: per step one k_ao_step and one launch of the production any-hit kernels (launch_trace: the eight-box kernel for
 * triangle-only scenes, the four-box one with spheres).
 */
#include "ftn_firsthit.h"
#include "ftn_ao.h"
#include <cstring>

namespace ftn {

/* ================================================================== ambient occlusion (include/fountain_hip_ao.h)
 * A path's 64-byte record (the path integrator's pd record, free in a first-hit pass), as k_ao_shade leaves it:
 *     {p, -} {p_err, flags} {n, -} {bent, count}
 * flags: AO_HIT a surface was recorded, AO_FLIP its hemisphere stands on -n.  count = -1 marks a sample without a surface, so that
 * the accumulate kernel reads the fourth float4 alone: 16 bytes per path instead of the whole record. */
enum : uint32_t { AO_HIT = 1u, AO_FLIP = 2u };
struct AoParams {
    FhFilm film;          /* 8 floats per crop pixel (ftn_ao_pixel), the first 6 added into; 4 float4 per path (above) */
    uint32_t* hits;       /* the paths that recorded a surface, in no particular order; their number is counters[WFC_ACTIVE_B] */
    uint32_t rays; float radius;
};
struct AoFilm {           /* sums: open, bent, hit weight, weight */
    static constexpr int OUT = 8, SUMS = 6;
    static constexpr uint32_t REC = 1, CHUNK = 8;
    __device__ static float4 load(const FhFilm& G, const WfBuffers&, size_t p, uint32_t) { return G.rec[4 * p + 3]; }
    __device__ static bool unpack(const float4* r, float* v, uint32_t* adds) {
        v[0] = r->w; v[1] = r->x; v[2] = r->y; v[3] = r->z;
        *adds = ~0u;
        return r->w >= 0.0f;
    }
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
        DRay ray0; DHit h; DSI si;
        const FhHit found = fh_first_hit(S, W, p, &ray0, &h, &si);
        push = found == FH_THROUGH;
        float4 r0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), r1 = r0, r2 = r0, r3 = make_float4(0.0f, 0.0f, 0.0f, -1.0f);       /* a miss */
        if (found == FH_SURFACE) {
            const uint32_t flags = AO_HIT | (ao_flipped(si.hit.n, si.wo) ? AO_FLIP : 0u);
            r0 = make_float4(si.hit.p.x, si.hit.p.y, si.hit.p.z, 0.0f);
            r1 = make_float4(si.hit.p_err.x, si.hit.p_err.y, si.hit.p_err.z, __uint_as_float(flags));
            r2 = make_float4(si.hit.n.x, si.hit.n.y, si.hit.n.z, 0.0f);
            r3 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            recorded = true;
        }
        if (!push) { float4* R = G.film.rec + 4 * (size_t)p; R[0] = r0; R[1] = r1; R[2] = r2; R[3] = r3; }
    }
    const bool pred[2] = {push, recorded};
    const uint32_t val[2] = {p, p};
    uint32_t* const qs[2] = {q_out, G.hits};
    uint32_t* const cs[2] = {count_out, &W.counters[CTR(WFC_ACTIVE_B)]};
    block_push<2>(pred, val, qs, cs);
}

/* Step k, one thread per recorded surface: folds the answer to ray k - 1 into the record (its direction is still in the path's shadow-ray
 * slot) and, unless k == rays, makes ray k from draws 5 + 2k and 6 + 2k of the sample's stream and queues it.  One launch per step. */
__global__ void __launch_bounds__(256) k_ao_step(RenderParams P, WfBuffers W, AoParams G, uint32_t k) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    bool push = false;
    uint32_t p = 0;
    if (i < W.counters[CTR(WFC_ACTIVE_B)]) {
        p = G.hits[i];
        float4* R = G.film.rec + 4 * (size_t)p;
        if (k > 0 && !W.occluded[p]) {
            const float4 d = W.sh[2 * (size_t)p + 1];
            float4 b = R[3];
            b.x += d.x; b.y += d.y; b.z += d.z; b.w += 1.0f;
            R[3] = b;
        }
        if (k < G.rays) {
            const float4 r0 = R[0], r1 = R[1], r2 = R[2];
            const FhSample cs = fh_sample(P, W, p);
            Rng rng; rng.seed(indexed_key(P.seed, cs.px, cs.py, cs.sample));
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

struct AoResolve {
    const float* in; uint32_t rays; float* out6;
    __device__ void operator()(size_t i) const { ao_resolve_pixel(in + 8 * i, rays, out6 + 6 * i); }
};
hipError_t launch_ao_resolve(const float* in, size_t n, uint32_t rays, float* out6, hipStream_t stream) { return fh_per_pixel(n, stream, AoResolve{in, rays, out6}); }

int wavefront_ao(WavefrontState** state, const RenderParams& P, const std::vector<DTile>& tiles, uint32_t rays, float radius, int count_mode, float* d_out,
                 hipStream_t stream, double* trace_ms_out, WavefrontTimes* times) {
    AoParams G;
    G.film = fh_film(P, d_out); G.hits = nullptr; G.rays = rays; G.radius = radius;
    double any_ms = 0.0; unsigned long long any_launches = 0;
    WfFirstHitPass pass;
    pass.what = "the ambient occlusion";
    /* the path integrator's 64-byte records; the list of recorded surfaces in q_active[1], whose count k_wf_reset starts every pass at zero
     * (q_active[0] is as free, but its count starts at the number of camera samples) */
    pass.setup = [&](WavefrontState* st, uint32_t) { G.film.rec = st->pd; G.hits = st->W.q_active[1]; return FTN_OK; };
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
            hipLaunchKernelGGL(k_fh_shadow_reset, dim3(1), dim3(64), 0, sm, W, 0u);          /* k_ao_step pushes this step's rays */
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
    pass.accumulate = [&](const WfBuffers& W, dim3 grid, hipStream_t sm) { hipLaunchKernelGGL(k_fh_accumulate<AoFilm>, grid, dim3(256), 0, sm, P, W, G.film); };
    const int rc = wf_first_hit_passes(state, P, tiles, pass, stream, trace_ms_out);
    if (times) { times->any_ms = any_ms; times->any_launches = any_launches; }
    return fh_merge<AoFilm>(rc, P, G.film, stream);
}

}  // namespace ftn
