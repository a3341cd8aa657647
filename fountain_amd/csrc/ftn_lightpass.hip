/*
 * ftn_lightpass.hip -- the light-group pass (include/fountain_hip_lightpass.h) on the wavefront pipeline.
 *
 * A unit of its own, like ftn_ao.hip: k_lp_shade is here and shares ftn_wf_common.h with the beauty's kernels; the passes and their
 * pass-through rounds are wf_first_hit_passes' (ftn_wf_internal.h, ftn_wavefront.hip), which wavefront_lightpass hands the launches of
 * k_lp_shade and of the shared film's accumulate kernel (ftn_firsthit.h) for LpFilm and, as a pass with a secondary stage, the one
 * shadow-ray launch between them: k_fh_shadow_reset, k_lp_fill and one launch of the production any-hit kernels (launch_trace: the
 * eight-box kernel for triangle-only scenes, the four-box one with spheres).
 */
#include "ftn_firsthit.h"
#include "ftn_lightpass.h"
#include <cstring>

namespace ftn {

/* ================================================================== light groups (include/fountain_hip_lightpass.h)
 * Of a path's 64-byte record (the path integrator's pd record, free in a first-hit pass) the pass uses the first float4, as k_lp_shade
 * leaves it: {e.rgb, state}.  state: LP_HIT a surface was recorded, LP_RAY its shadow ray stands in the path's W.sh slot and its answer
 * will stand in W.occluded[p]; 0 marks a sample without a surface.  The accumulate kernel reads 16 bytes per path, and one byte more for
 * the paths with a ray. */
enum : uint32_t { LP_HIT = 1u, LP_RAY = 2u, LP_OCCLUDED = 4u /* set while staging, never stored */ };
struct LpParams {
    FhFilm film;          /* 8 floats per crop pixel (ftn_lightpass_pixel); 4 float4 per path, the first one used (above) */
    uint32_t* rays;       /* the paths with a shadow ray, in no particular order; their number is counters[WFC_ACTIVE_B] */
    const uint32_t* lights;    /* the group's indices into S.lights, strictly increasing; NULL: the identity (all lights) */
    uint32_t n_lights;
};
struct LpFilm {           /* sums: lit, unshadowed, hit weight, weight */
    static constexpr int OUT = 8, SUMS = 8;
    static constexpr uint32_t REC = 1, CHUNK = 8;
    /* the shadow ray's answer folded into the state word (the index stays inside occluded[] for a slot without a path, too) */
    __device__ static float4 load(const FhFilm& G, const WfBuffers& W, size_t p, uint32_t) {
        float4 r = G.rec[4 * p];
        const uint32_t state = __float_as_uint(r.w);
        if ((state & LP_RAY) && W.occluded[p]) r.w = __uint_as_float(state | LP_OCCLUDED);
        return r;
    }
    /* the term is added to unshadowed for every surface, to lit only where its shadow ray was traced and found nothing */
    __device__ static bool unpack(const float4* r, float* v, uint32_t* adds) {
        const uint32_t state = __float_as_uint(r->w);
        v[0] = r->x; v[1] = r->y; v[2] = r->z; v[3] = r->x; v[4] = r->y; v[5] = r->z;
        *adds = (state & (LP_RAY | LP_OCCLUDED)) == LP_RAY ? 0x3fu : 0x38u;
        return (state & LP_HIT) != 0u;
    }
};

/* one thread per queued ray: the hit it found is either passed through (k_gb_shade without a material lookup) or recorded with the
 * term of the one light sample the header defines and, where that term is not black, its shadow ray */
__global__ void __launch_bounds__(256) k_lp_shade(RenderParams P, WfBuffers W, LpParams G, const uint32_t* __restrict__ q_in, const uint32_t* count_in,
                                                  uint32_t* q_out, uint32_t* count_out) {
    const DScene& S = P.S;
    const uint32_t qi = blockIdx.x * 256u + threadIdx.x;
    bool push = false, traced = false;
    uint32_t p = 0;
    if (qi < *count_in) {
        p = q_in[qi];
        DRay ray0; DHit h; DSI si;
        const FhHit found = fh_first_hit(S, W, p, &ray0, &h, &si);
        push = found == FH_THROUGH;
        float4 r0 = make_float4(0.0f, 0.0f, 0.0f, __uint_as_float(0u));       /* a miss */
        if (found == FH_SURFACE) {
            Rgb e(0.0f);
            if (G.n_lights > 0u) {
                /* the sample's stream behind its camera sample: draw 5 picks the light, draws 6 and 7 sample it */
                const FhSample cs = fh_sample(P, W, p);
                Rng rng; rng.seed(indexed_key(P.seed, cs.px, cs.py, cs.sample));
                rng.skip(5u);
                const uint32_t k = lp_select(rng.next(), G.n_lights);
                const V2 ul = rng.next2();
                const uint32_t li = G.lights ? G.lights[k] : k;
                const DLiSample ls = light_sample(S, S.lights[li], si.hit, ul);
                if (lp_term(si.hit.n, si.shading_n, si.wo, ls.radiance, ls.wi, ls.pdf, G.n_lights, &e)) {
                    const LpRay sr = lp_shadow_ray(si.hit.p, si.hit.p_err, si.hit.n, ls.p1.p, ls.p1.p_err, ls.p1.n);
                    W.sh[2 * (size_t)p] = make_float4(sr.o.x, sr.o.y, sr.o.z, 0.0f); W.sh[2 * (size_t)p + 1] = make_float4(sr.d.x, sr.d.y, sr.d.z, sr.t_max);
                    traced = true;
                }
            }
            r0 = make_float4(e.r, e.g, e.b, __uint_as_float(LP_HIT | (traced ? LP_RAY : 0u)));
        }
        if (!push) G.film.rec[4 * (size_t)p] = r0;
    }
    const bool pred[2] = {push, traced};
    const uint32_t val[2] = {p, p};
    uint32_t* const qs[2] = {q_out, G.rays};
    uint32_t* const cs[2] = {count_out, &W.counters[CTR(WFC_ACTIVE_B)]};
    block_push<2>(pred, val, qs, cs);
}

/* before the shadow-ray launch, behind k_fh_shadow_reset: the rounds used q_shadow for their pass-throughs, so the list of rays is copied
 * into it behind them */
__global__ void __launch_bounds__(256) k_lp_fill(WfBuffers W, LpParams G, uint32_t n_rays) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < n_rays) W.q_shadow[i] = G.rays[i];
}

struct LpResolve {
    const float* in; float* out8;
    __device__ void operator()(size_t i) const { lp_resolve_pixel(in + 8 * i, out8 + 8 * i); }
};
hipError_t launch_lp_resolve(const float* in, size_t n, float* out8, hipStream_t stream) { return fh_per_pixel(n, stream, LpResolve{in, out8}); }

/* the relighting step: one thread per pixel, the groups in increasing order */
__global__ void __launch_bounds__(256) k_lp_compose(const float* __restrict__ gb12, const float* __restrict__ res8, uint32_t groups, LpGains gains, size_t n,
                                                    float* __restrict__ rgb) {
    for (size_t i = (size_t)blockIdx.x * 256u + threadIdx.x; i < n; i += (size_t)gridDim.x * 256u) lp_compose_pixel(gb12 + 12 * i, res8, i, n, groups, gains, rgb + 3 * i);
}
hipError_t launch_lp_compose(const float* gb12, const float* res8, uint32_t groups, const LpGains& gains, size_t n, float* rgb, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    const unsigned grid = (unsigned)std::min<size_t>((n + 255) / 256, 4096);
    hipLaunchKernelGGL(k_lp_compose, dim3(grid), dim3(256), 0, stream, gb12, res8, groups, gains, n, rgb);
    return hipGetLastError();
}

int wavefront_lightpass(WavefrontState** state, const RenderParams& P, const std::vector<DTile>& tiles, const uint32_t* d_lights, uint32_t n_lights, int count_mode,
                        float* d_out, hipStream_t stream, double* trace_ms_out, WavefrontTimes* times) {
    LpParams G;
    G.film = fh_film(P, d_out); G.rays = nullptr; G.lights = d_lights; G.n_lights = n_lights;
    double any_ms = 0.0; unsigned long long any_launches = 0;
    WfFirstHitPass pass;
    pass.what = "the light pass";
    /* the path integrator's 64-byte records; the list of shadow rays in q_active[1], whose count k_wf_reset starts every pass at zero
     * (q_active[0] is as free, but its count starts at the number of camera samples) */
    pass.setup = [&](WavefrontState* st, uint32_t) { G.film.rec = st->pd; G.rays = st->W.q_active[1]; return FTN_OK; };
    pass.shade = [&](const WfBuffers& W, const uint32_t* q_in, const uint32_t* count_in, uint32_t* q_out, uint32_t* count_out, dim3 grid, hipStream_t sm) {
        hipLaunchKernelGGL(k_lp_shade, grid, dim3(256), 0, sm, P, W, G, q_in, count_in, q_out, count_out);
    };
    pass.secondary = [&](WavefrontState* st, const WfBuffers& W, size_t lds, unsigned trace_grid_max, hipStream_t sm) -> int {
        const uint32_t n_rays = st->host_counters[CTR(WFC_ACTIVE_B)];     /* the driver's last poll: behind the last shade launch of the pass */
        if (n_rays == 0) return FTN_OK;
        const unsigned tg = std::min<unsigned>(trace_grid_max, (2 * W.n_paths + 255) / 256);
        hipLaunchKernelGGL(k_fh_shadow_reset, dim3(1), dim3(64), 0, sm, W, n_rays);
        hipLaunchKernelGGL(k_lp_fill, dim3((n_rays + 255) / 256), dim3(256), 0, sm, W, G, n_rays);
        WF_TRY(hipEventRecord(st->ev[0], sm));
        launch_trace(st, true, count_mode, P.S.n_spheres != 0, tg, lds, sm, P, W, W.q_shadow, &W.counters[CTR(WFC_SHADOW)], &W.counters[CTR(WFC_HEAD_ANY)], n_rays);
        WF_TRY(hipEventRecord(st->ev[1], sm));
        WF_TRY(hipEventSynchronize(st->ev[1]));
        float ms = 0.0f; (void)hipEventElapsedTime(&ms, st->ev[0], st->ev[1]);
        any_ms += ms; any_launches++;
        return FTN_OK;
    };
    pass.accumulate = [&](const WfBuffers& W, dim3 grid, hipStream_t sm) { hipLaunchKernelGGL(k_fh_accumulate<LpFilm>, grid, dim3(256), 0, sm, P, W, G.film); };
    const int rc = wf_first_hit_passes(state, P, tiles, pass, stream, trace_ms_out);
    if (times) { times->any_ms = any_ms; times->any_launches = any_launches; }
    return fh_merge<LpFilm>(rc, P, G.film, stream);
}

}  // namespace ftn
