/*
 * ftn_lightpass.hip -- the light-group pass (include/fountain_hip_lightpass.h) on the wavefront pipeline.
 *
 * A unit of its own, like ftn_ao.hip: the kernels are here and share ftn_wf_common.h with the beauty's; the passes and their pass-through
 * rounds are wf_first_hit_passes' (ftn_wf_internal.h, ftn_wavefront.hip), which wavefront_lightpass hands the launches of k_lp_shade and
 * k_lp_accumulate and, as the driver's second pass with a secondary stage, the one shadow-ray launch between them: k_lp_reset, k_lp_fill
 * and one launch of the production any-hit kernels (launch_trace: the eight-box kernel for triangle-only scenes, the four-box one with
 * spheres).
 */
#include "ftn_wf_internal.h"
#include "ftn_lightpass.h"
#include <algorithm>
#include <cstring>

namespace ftn {

/* ================================================================== light groups (include/fountain_hip_lightpass.h)
 * Of a path's 64-byte record (the path integrator's pd record, free in a first-hit pass) the pass uses the first float4, as k_lp_shade
 * leaves it: {e.rgb, state}.  state: LP_HIT a surface was recorded, LP_RAY its shadow ray stands in the path's W.sh slot and its answer
 * will stand in W.occluded[p]; 0 marks a sample without a surface.  k_lp_accumulate reads 16 bytes per path, and one byte more for the
 * paths with a ray. */
enum : uint32_t { LP_HIT = 1u, LP_RAY = 2u, LP_OCCLUDED = 4u /* set while staging, never stored */ };
struct LpParams {
    float* out;           /* 8 floats per crop pixel (ftn_lightpass_pixel), added into */
    float4 *spillA, *spillB;   /* per crop pixel, the samples whose footprint leaves their own pixel (atomics; added into out at the end):
                                * {lit, hit weight} {unshadowed, weight} */
    float4* rec;          /* 4 float4 per path, the first one used (above) */
    uint32_t* rays;       /* the paths with a shadow ray, in no particular order; their number is counters[WFC_ACTIVE_B] */
    const uint32_t* lights;    /* the group's indices into S.lights, strictly increasing; NULL: the identity (all lights) */
    uint32_t n_lights;
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
        const float4 ro = W.ray[2 * (size_t)p], rdv = W.ray[2 * (size_t)p + 1];
        DRay ray0; ray0.o = V3(ro.x, ro.y, ro.z); ray0.d = V3(rdv.x, rdv.y, rdv.z); ray0.t_max = rdv.w; ray0.time = 0.0f;
        const DHit h = load_hit(W, p);
        float4 r0 = make_float4(0.0f, 0.0f, 0.0f, __uint_as_float(0u));       /* a miss */
        if (h.prim >= 0) {
            DSI si; make_interaction(S, h, ray0, &si);
            if (si.mat < 0) {
                const DRay nr = spawn_ray(si.hit, ray0.d);
                W.ray[2 * (size_t)p] = make_float4(nr.o.x, nr.o.y, nr.o.z, 0.0f); W.ray[2 * (size_t)p + 1] = make_float4(nr.d.x, nr.d.y, nr.d.z, nr.t_max);
                push = true;
            } else {
                Rgb e(0.0f);
                if (G.n_lights > 0u) {
                    /* the sample's stream behind its camera sample: draw 5 picks the light, draws 6 and 7 sample it */
                    const uint32_t slot = p / W.samples, sidx = p % W.samples;
                    const DTile tile = P.tiles[slot >> 8];
                    const int px = tile.x0 + (int)(slot & 15u), py = tile.y0 + (int)((slot >> 4) & 15u);
                    Rng rng; rng.seed(indexed_key(P.seed, px, py, W.first_sample + sidx));
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
        }
        if (!push) G.rec[4 * (size_t)p] = r0;
    }
    const bool pred[2] = {push, traced};
    const uint32_t val[2] = {p, p};
    uint32_t* const qs[2] = {q_out, G.rays};
    uint32_t* const cs[2] = {count_out, &W.counters[CTR(WFC_ACTIVE_B)]};
    block_push<2>(pred, val, qs, cs);
}

/* before the shadow-ray launch: the trace kernels' queue heads and their hand-back queues (k_wf_round_reset's work), and the any-hit
 * queue's length: the rounds used q_shadow for their pass-throughs, so the list of rays is copied into it behind them (k_lp_fill) */
__global__ void __launch_bounds__(64) k_lp_reset(WfBuffers W, uint32_t n_rays) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    static_assert(WFC_HEADS_END == WFC_EXC_FIRST, "the two ranges are cleared as one");
    for (int i = WFC_HEADS_FIRST; i < WFC_EXC_END; i++) W.counters[CTR(i)] = 0;
    W.counters[CTR(WFC_SHADOW)] = n_rays;
}
__global__ void __launch_bounds__(256) k_lp_fill(WfBuffers W, LpParams G, uint32_t n_rays) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < n_rays) W.q_shadow[i] = G.rays[i];
}

/* one sample's sums into every pixel of its box-filter footprint (film_add): the own pixel in registers, others into the spill sums */
__device__ inline void lp_film_add(const LpParams& G, const FilmCtx& F, V2 p_film, float4 r, int own_x, int own_y, float* acc, uint32_t* spill, uint32_t* bc_writes) {
    const FilmFootprint fp = film_footprint(F, p_film);
    const uint32_t state = __float_as_uint(r.w);
    const bool hit = (state & LP_HIT) != 0u, open = (state & (LP_RAY | LP_OCCLUDED)) == LP_RAY;
    const float v[3] = {r.x, r.y, r.z};
    int touched = 0;
    for (int y = fp.y0; y < fp.y1; y++)
        for (int x = fp.x0; x < fp.x1; x++) {
            touched++;
            if (x == own_x && y == own_y) {
                if (hit) {
#pragma unroll
                    for (int k = 0; k < 3; k++) {        /* value * filter weight (box: 1.0) */
                        if (open) acc[k] += v[k] * 1.0f;
                        acc[3 + k] += v[k] * 1.0f;
                    }
                    acc[6] += 1.0f;
                }
                acc[7] += 1.0f;
                continue;
            }
            const size_t i = film_idx(F, x, y);
            float* a = reinterpret_cast<float*>(G.spillA + i);
            float* b = reinterpret_cast<float*>(G.spillB + i);
            if (hit) {
#pragma unroll
                for (int k = 0; k < 3; k++) {
                    if (open) atomicAdd(a + k, v[k] * 1.0f);
                    atomicAdd(b + k, v[k] * 1.0f);
                }
                atomicAdd(a + 3, 1.0f);
            }
            atomicAdd(b + 3, 1.0f);
            (*bc_writes)++;
        }
    if (touched != 1) (*spill)++;
}

/* One thread per pixel slot adds its samples in sample order into the caller's buffer; the workgroup stages LP_ACC_CHUNK samples of its
 * 256 slots (the first float4 of each path's record, and the shadow ray's answer folded into its state word) through LDS, consecutive
 * threads reading consecutive paths, as k_ao_accumulate does. */
#define LP_ACC_CHUNK 8u
__global__ void __launch_bounds__(256) k_lp_accumulate(RenderParams P, WfBuffers W, LpParams G) {
    __shared__ float4 s_rec[256 * LP_ACC_CHUNK];
    const uint32_t slot = blockIdx.x * 256u + threadIdx.x;
    uint32_t spill = 0, bc = 0;
    const FilmSlot fs = film_slot(P, W.n_slots, slot);
    const bool valid = fs.valid, in_crop = fs.in_crop; const int px = fs.px, py = fs.py; const size_t ai = fs.ai;
    float acc[8];
#pragma unroll
    for (int k = 0; k < 8; k++) acc[k] = in_crop ? G.out[8 * ai + k] : 0.0f;
    const size_t block_first = (size_t)blockIdx.x * 256u * W.samples;          /* first path of this workgroup's 256 slots */
    for (uint32_t s0 = 0; s0 < W.samples; s0 += LP_ACC_CHUNK) {
        const uint32_t n = W.samples - s0 < LP_ACC_CHUNK ? W.samples - s0 : LP_ACC_CHUNK;
        for (uint32_t e = threadIdx.x; e < 256u * n; e += 256u) {                /* n consecutive samples of slot e / n */
            const uint32_t sl = e / n, k = e - sl * n;
            const size_t p = block_first + (size_t)sl * W.samples + s0 + k;
            if (p < W.n_paths) {
                float4 r = G.rec[4 * p];
                const uint32_t state = __float_as_uint(r.w);
                /* (a slot outside its tile has no path: its record is whatever an earlier pass left, and nothing reads what is staged for
                 * it; the index stays inside occluded[] either way) */
                if ((state & LP_RAY) && W.occluded[p]) r.w = __uint_as_float(state | LP_OCCLUDED);
                s_rec[sl * LP_ACC_CHUNK + k] = r;
            }
        }
        __syncthreads();
        if (valid) {
            for (uint32_t k = 0; k < n; k++) {
                /* the sample's film position: the first two draws of its stream, exactly as k_wf_generate made them */
                Rng crng; crng.seed(indexed_key(P.seed, px, py, W.first_sample + s0 + k));
                const V2 j = crng.next2();
                lp_film_add(G, fs.F, V2((float)px + j.x, (float)py + j.y), s_rec[threadIdx.x * LP_ACC_CHUNK + k], in_crop ? px : FTN_OWN_NONE, py, acc, &spill, &bc);
            }
        }
        __syncthreads();
    }
    if (valid && in_crop) {
#pragma unroll
        for (int k = 0; k < 8; k++) G.out[8 * ai + k] = acc[k];
    }
    if (spill) atomicAdd(&P.stats->spill_samples, (unsigned long long)spill);       /* rare */
    if (bc) atomicAdd(&P.stats->bc_writes, (unsigned long long)bc);
}

/* after the last pass: the spill sums into the caller's buffer (nothing to do when no sample left its own pixel) */
__global__ void __launch_bounds__(256) k_lp_merge(LpParams G, size_t n, const DevStats* __restrict__ stats) {
    if (stats->bc_writes == 0) return;
    for (size_t i = (size_t)blockIdx.x * 256u + threadIdx.x; i < n; i += (size_t)gridDim.x * 256u) {
        const float4 a = G.spillA[i], b = G.spillB[i];
        if (b.w == 0.0f) continue;
        const float add[8] = {a.x, a.y, a.z, b.x, b.y, b.z, a.w, b.w};
#pragma unroll
        for (int k = 0; k < 8; k++) G.out[8 * i + k] += add[k];
    }
}

__global__ void __launch_bounds__(256) k_lp_resolve(const float* __restrict__ in, size_t n, float* __restrict__ out8) {
    for (size_t i = (size_t)blockIdx.x * 256u + threadIdx.x; i < n; i += (size_t)gridDim.x * 256u) lp_resolve_pixel(in + 8 * i, out8 + 8 * i);
}
hipError_t launch_lp_resolve(const float* in, size_t n, float* out8, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    const unsigned grid = (unsigned)std::min<size_t>((n + 255) / 256, 4096);
    hipLaunchKernelGGL(k_lp_resolve, dim3(grid), dim3(256), 0, stream, in, n, out8);
    return hipGetLastError();
}

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
                        float* d_out, float4* spill_a, float4* spill_b, hipStream_t stream, double* trace_ms_out, LpTimes* times) {
    LpParams G;
    G.out = d_out; G.spillA = spill_a; G.spillB = spill_b; G.rec = nullptr; G.rays = nullptr; G.lights = d_lights; G.n_lights = n_lights;
    double any_ms = 0.0; unsigned long long any_launches = 0;
    WfFirstHitPass pass;
    pass.what = "the light pass";
    /* the path integrator's 64-byte records; the list of shadow rays in q_active[1], whose count k_wf_reset starts every pass at zero
     * (q_active[0] is as free, but its count starts at the number of camera samples) */
    pass.setup = [&](WavefrontState* st, uint32_t) { G.rec = st->pd; G.rays = st->W.q_active[1]; return FTN_OK; };
    pass.shade = [&](const WfBuffers& W, const uint32_t* q_in, const uint32_t* count_in, uint32_t* q_out, uint32_t* count_out, dim3 grid, hipStream_t sm) {
        hipLaunchKernelGGL(k_lp_shade, grid, dim3(256), 0, sm, P, W, G, q_in, count_in, q_out, count_out);
    };
    pass.secondary = [&](WavefrontState* st, const WfBuffers& W, size_t lds, unsigned trace_grid_max, hipStream_t sm) -> int {
        const uint32_t n_rays = st->host_counters[CTR(WFC_ACTIVE_B)];     /* the driver's last poll: behind the last shade launch of the pass */
        if (n_rays == 0) return FTN_OK;
        const unsigned tg = std::min<unsigned>(trace_grid_max, (2 * W.n_paths + 255) / 256);
        hipLaunchKernelGGL(k_lp_reset, dim3(1), dim3(64), 0, sm, W, n_rays);
        hipLaunchKernelGGL(k_lp_fill, dim3((n_rays + 255) / 256), dim3(256), 0, sm, W, G, n_rays);
        WF_TRY(hipEventRecord(st->ev[0], sm));
        launch_trace(st, true, count_mode, P.S.n_spheres != 0, tg, lds, sm, P, W, W.q_shadow, &W.counters[CTR(WFC_SHADOW)], &W.counters[CTR(WFC_HEAD_ANY)], n_rays);
        WF_TRY(hipEventRecord(st->ev[1], sm));
        WF_TRY(hipEventSynchronize(st->ev[1]));
        float ms = 0.0f; (void)hipEventElapsedTime(&ms, st->ev[0], st->ev[1]);
        any_ms += ms; any_launches++;
        return FTN_OK;
    };
    pass.accumulate = [&](const WfBuffers& W, dim3 grid, hipStream_t sm) { hipLaunchKernelGGL(k_lp_accumulate, grid, dim3(256), 0, sm, P, W, G); };
    const int rc = wf_first_hit_passes(state, P, tiles, pass, stream, trace_ms_out);
    if (times) { times->any_ms = any_ms; times->any_launches = any_launches; }
    if (rc || !G.rec) return rc;          /* (no record buffer: no tiles or no samples, nothing was launched) */
    const size_t npix = (size_t)std::max(0, P.crop[2] - P.crop[0]) * (size_t)std::max(0, P.crop[3] - P.crop[1]);
    if (npix) hipLaunchKernelGGL(k_lp_merge, dim3((unsigned)std::min<size_t>((npix + 255) / 256, 4096)), dim3(256), 0, stream, G, npix, (const DevStats*)P.stats);
    WF_TRY(hipGetLastError());
    return FTN_OK;
}

}  // namespace ftn
