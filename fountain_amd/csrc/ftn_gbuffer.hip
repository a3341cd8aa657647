/*
 * ftn_gbuffer.hip -- the first-hit G-buffer pass (include/fountain_hip_gbuffer.h) on the wavefront pipeline.
 *
 * A unit of its own: the driver uses the wavefront pipeline through ftn_wf_internal.h (the scene's WavefrontState and its buffers, the
 * pass plan, the traversal launches, the launchers of k_wf_reset and k_wf_generate), the kernels share ftn_wf_common.h with the beauty's.
 */
#include "ftn_wf_internal.h"
#include "ftn_texture.h"
#include "ftn_gbuffer.h"
#include <algorithm>
#include <cstring>

namespace ftn {

/* ================================================================== first-hit G-buffer (include/fountain_hip_gbuffer.h)
 * The camera samples of ftn_render for the same sampler, tiles and film: k_wf_generate makes the camera rays from the sample keys, the
 * production closest-hit kernels trace them, and k_gb_shade records the first surface that has a material.  A null-material hit spawns
 * the ray on along the same direction (path.rs:77-80) into the other queue and the round repeats, at most GB_MAX_PASS_THROUGH times.
 * k_gb_accumulate then adds the pass's samples of every pixel in sample order, as k_wf_accumulate adds the beauty's. */
#define GB_MAX_PASS_THROUGH 4096u
struct GbParams {
    float w2c[16];        /* camera_to_world.inv: camera-space z of a hit (transform.rs:224) */
    float* out;           /* 12 floats per crop pixel (ftn_gbuffer_pixel), added into */
    float4 *spillA, *spillB, *spillC;   /* per crop pixel, the samples whose footprint leaves their own pixel (atomics; added into out at the end):
                                         * {albedo, hit weight} {shading normal, weight} {p, camera-space z} */
    float4* rec;          /* 3 float4 per path: {albedo, hit ? 1 : 0} {shading normal, camera-space z} {p, 0} */
};

/* the albedo the first BSDF of the beauty is built from: each parameter clamped as compute_scattering_functions clamps it */
__device__ inline Rgb gb_albedo(const ftn_material& m) {
    const Rgb a(m.a[0], m.a[1], m.a[2]), b(m.b[0], m.b[1], m.b[2]);
    switch (m.type) {
        case FTN_MAT_MATTE: return clamp_positive(a);                              /* matte.rs:39 */
        case FTN_MAT_MIRROR: return clamp_positive(a);                             /* mirror.rs:24 */
        case FTN_MAT_METAL: return fresnel_conductor(1.0f, Rgb(1.0f), a, b);       /* FresnelConductor{1, eta, k} at normal incidence */
        case FTN_MAT_PLASTIC: return a + b;                                        /* plastic.rs:27-32: not clamped */
        default: return clamp_positive(a) + clamp_positive(b);                     /* glass.rs:54-55 */
    }
}

/* one thread per queued ray: the hit it found is either recorded or passed through */
template <bool TEX>
__global__ void __launch_bounds__(256) k_gb_shade(RenderParams P, WfBuffers W, GbParams G, const uint32_t* __restrict__ q_in, const uint32_t* count_in,
                                                  uint32_t* q_out, uint32_t* count_out) {
    const DScene& S = P.S;
    const uint32_t qi = blockIdx.x * 256u + threadIdx.x;
    bool push = false;
    uint32_t p = 0;
    if (qi < *count_in) {
        p = q_in[qi];
        const float4 ro = W.ray[2 * (size_t)p], rdv = W.ray[2 * (size_t)p + 1];
        DRay ray0; ray0.o = V3(ro.x, ro.y, ro.z); ray0.d = V3(rdv.x, rdv.y, rdv.z); ray0.t_max = rdv.w; ray0.time = 0.0f;
        const DHit h = load_hit(W, p);
        float4 r0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), r1 = r0, r2 = r0;       /* a miss */
        if (h.prim >= 0) {
            DSI si; make_interaction(S, h, ray0, &si);
            if (si.mat < 0) {
                const DRay nr = spawn_ray(si.hit, ray0.d);
                W.ray[2 * (size_t)p] = make_float4(nr.o.x, nr.o.y, nr.o.z, 0.0f); W.ray[2 * (size_t)p + 1] = make_float4(nr.d.x, nr.d.y, nr.d.z, nr.t_max);
                push = true;
            } else {
                ftn_material m = S.materials[si.mat];
                if (TEX && material_is_textured(S, si.mat)) {
                    /* the camera ray's differentials, as the beauty's first shading pass rebuilds them (k_wf_shade): the path integrator hands
                     * them on unchanged through null-material pass-throughs */
                    const uint32_t slot = p / W.samples, sidx = p % W.samples;
                    const DTile tile = P.tiles[slot >> 8];
                    const int px = tile.x0 + (int)(slot & 15u), py = tile.y0 + (int)((slot >> 4) & 15u);
                    Rng crng; crng.seed(indexed_key(P.seed, px, py, W.first_sample + sidx));
                    const V2 j = crng.next2(); const V2 p_film((float)px + j.x, (float)py + j.y); const V2 p_lens = crng.next2(); const float time_u = crng.next();
                    const DRay cam = camera_ray(P.C, p_film, p_lens, time_u);
                    const DRayDiff rd = camera_ray_diff(P.C, p_film, p_lens, cam, 1.0f / sqrtf((float)P.spp));
                    DSIX ex; DSI s2; make_interaction(S, h, ray0, &s2, &ex);
                    const DTexDiffs td = compute_tex_diffs(si.hit.p, si.hit.n, ex.dpdu, ex.dpdv, rd);
                    m = material_resolve(S, si.mat, ex.uv, td);
                }
                const Rgb alb = gb_albedo(m);
                const V3 pc = m4_point(G.w2c, si.hit.p);
                r0 = make_float4(alb.r, alb.g, alb.b, 1.0f);
                r1 = make_float4(si.shading_n.x, si.shading_n.y, si.shading_n.z, pc.z);
                r2 = make_float4(si.hit.p.x, si.hit.p.y, si.hit.p.z, 0.0f);
            }
        }
        if (!push) { float4* R = G.rec + 3 * (size_t)p; R[0] = r0; R[1] = r1; R[2] = r2; }
    }
    const bool pred[1] = {push};
    const uint32_t val[1] = {p};
    uint32_t* const qs[1] = {q_out};
    uint32_t* const cs[1] = {count_out};
    block_push<1>(pred, val, qs, cs);
}

/* between two rounds: the trace kernels' queue heads and hand-back queues, and the count of the queue the next shading pass fills */
__global__ void k_gb_reset(WfBuffers W, uint32_t out_ctr) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    W.counters[CTR(WFC_DRY_WAVES)] = 0;
    static_assert(WFC_HEADS_END == WFC_EXC_FIRST, "the two ranges are cleared as one");
    for (int i = WFC_HEADS_FIRST; i < WFC_EXC_END; i++) W.counters[CTR(i)] = 0;
    W.counters[CTR(out_ctr)] = 0;
}

/* one sample's record into every pixel of its box-filter footprint (film_add): the own pixel in registers, others into the spill sums */
__device__ inline void gb_film_add(const GbParams& G, const FilmCtx& F, V2 p_film, float4 r0, float4 r1, float4 r2, int own_x, int own_y, float* acc, uint32_t* spill, uint32_t* bc_writes) {
    const FilmFootprint fp = film_footprint(F, p_film);
    const bool hit = r0.w != 0.0f;
    const float v[10] = {r0.x, r0.y, r0.z, r1.x, r1.y, r1.z, r2.x, r2.y, r2.z, r1.w};
    int touched = 0;
    for (int y = fp.y0; y < fp.y1; y++)
        for (int x = fp.x0; x < fp.x1; x++) {
            touched++;
            if (x == own_x && y == own_y) {
                if (hit) {
#pragma unroll
                    for (int k = 0; k < 10; k++) acc[k] += v[k] * 1.0f;       /* value * filter weight (box: 1.0) */
                    acc[10] += 1.0f;
                }
                acc[11] += 1.0f;
                continue;
            }
            const size_t i = film_idx(F, x, y);
            float* a = reinterpret_cast<float*>(G.spillA + i);
            float* b = reinterpret_cast<float*>(G.spillB + i);
            float* c = reinterpret_cast<float*>(G.spillC + i);
            if (hit) {
#pragma unroll
                for (int k = 0; k < 3; k++) { atomicAdd(a + k, v[k] * 1.0f); atomicAdd(b + k, v[3 + k] * 1.0f); atomicAdd(c + k, v[6 + k] * 1.0f); }
                atomicAdd(c + 3, v[9] * 1.0f);
                atomicAdd(a + 3, 1.0f);
            }
            atomicAdd(b + 3, 1.0f);
            (*bc_writes)++;
        }
    if (touched != 1) (*spill)++;
}

/* One thread per pixel slot adds its samples in sample order into the caller's buffer; the workgroup stages GB_ACC_CHUNK samples of its
 * 256 slots (48 bytes each, neighbours in memory) through LDS with coalesced loads, as k_wf_accumulate does. */
#define GB_ACC_CHUNK 4u
__global__ void __launch_bounds__(256) k_gb_accumulate(RenderParams P, WfBuffers W, GbParams G) {
    __shared__ float4 s_rec[256 * GB_ACC_CHUNK * 3];
    const uint32_t slot = blockIdx.x * 256u + threadIdx.x;
    uint32_t spill = 0, bc = 0;
    const FilmSlot fs = film_slot(P, W.n_slots, slot);
    const bool valid = fs.valid, in_crop = fs.in_crop; const int px = fs.px, py = fs.py; const size_t ai = fs.ai;
    float acc[12];
#pragma unroll
    for (int k = 0; k < 12; k++) acc[k] = in_crop ? G.out[12 * ai + k] : 0.0f;
    const size_t block_first = (size_t)blockIdx.x * 256u * W.samples;          /* first path of this workgroup's 256 slots */
    for (uint32_t s0 = 0; s0 < W.samples; s0 += GB_ACC_CHUNK) {
        const uint32_t n = W.samples - s0 < GB_ACC_CHUNK ? W.samples - s0 : GB_ACC_CHUNK;
        for (uint32_t e = threadIdx.x; e < 256u * 3u * n; e += 256u) {         /* the 3 n consecutive float4 of slot e / (3 n) */
            const uint32_t sl = e / (3u * n), k3 = e - sl * 3u * n;
            const size_t p = block_first + (size_t)sl * W.samples + s0 + k3 / 3u;
            if (p < W.n_paths) s_rec[sl * GB_ACC_CHUNK * 3u + k3] = G.rec[3 * p + k3 % 3u];
        }
        __syncthreads();
        if (valid) {
            for (uint32_t k = 0; k < n; k++) {
                const float4* r = &s_rec[(threadIdx.x * GB_ACC_CHUNK + k) * 3u];
                /* the sample's film position: the first two draws of its stream, exactly as k_wf_generate made them */
                Rng crng; crng.seed(indexed_key(P.seed, px, py, W.first_sample + s0 + k));
                const V2 j = crng.next2();
                gb_film_add(G, fs.F, V2((float)px + j.x, (float)py + j.y), r[0], r[1], r[2], in_crop ? px : FTN_OWN_NONE, py, acc, &spill, &bc);
            }
        }
        __syncthreads();
    }
    if (valid && in_crop) {
#pragma unroll
        for (int k = 0; k < 12; k++) G.out[12 * ai + k] = acc[k];
    }
    if (spill) atomicAdd(&P.stats->spill_samples, (unsigned long long)spill);       /* rare */
    if (bc) atomicAdd(&P.stats->bc_writes, (unsigned long long)bc);
}

/* after the last pass: the spill sums into the caller's buffer (nothing to do when no sample left its own pixel) */
__global__ void __launch_bounds__(256) k_gb_merge(GbParams G, size_t n, const DevStats* __restrict__ stats) {
    if (stats->bc_writes == 0) return;
    for (size_t i = (size_t)blockIdx.x * 256u + threadIdx.x; i < n; i += (size_t)gridDim.x * 256u) {
        const float4 a = G.spillA[i], b = G.spillB[i], c = G.spillC[i];
        if (b.w == 0.0f) continue;
        const float add[12] = {a.x, a.y, a.z, b.x, b.y, b.z, c.x, c.y, c.z, c.w, a.w, b.w};
#pragma unroll
        for (int k = 0; k < 12; k++) G.out[12 * i + k] += add[k];
    }
}

__global__ void __launch_bounds__(256) k_gb_resolve(const float* __restrict__ in, size_t n, float* __restrict__ out12) {
    for (size_t i = (size_t)blockIdx.x * 256u + threadIdx.x; i < n; i += (size_t)gridDim.x * 256u) gbuffer_resolve_pixel(in + 12 * i, out12 + 12 * i);
}
void launch_gbuffer_resolve(const float* in, size_t n, float* out12, hipStream_t stream) {
    if (n == 0) return;
    const unsigned grid = (unsigned)std::min<size_t>((n + 255) / 256, 4096);
    hipLaunchKernelGGL(k_gb_resolve, dim3(grid), dim3(256), 0, stream, in, n, out12);
}

int wavefront_gbuffer(WavefrontState** state, const RenderParams& P, const std::vector<DTile>& tiles, const float w2c[16], float* d_out,
                      float4* spill_a, float4* spill_b, float4* spill_c, hipStream_t stream, double* trace_ms_out) {
    knobs_begin();
    { int rc0 = wf_state_init(state); if (rc0) return rc0; }
    WavefrontState* st = *state;
    const uint32_t n_slots = (uint32_t)tiles.size() * 256u;
    const uint32_t total_samples = P.last_sample - P.first_sample;
    if (n_slots == 0 || total_samples == 0) return FTN_OK;
    /* the beauty's passes (wf_plan_passes) without the direct-lighting buffers: only camera rays are traced */
    WfPassPlan plan;
    int rc = wf_plan_passes(st, P, tiles.size() * 256u, total_samples, false, &plan);
    if (rc) return rc;
    const uint32_t S = plan.samples;
    if ((rc = trace4_prepare(st, P.S))) return rc;
    WfBuffers W = st->W;
    W.br = nullptr; W.pd = nullptr; W.pd_md = 0; W.pd_occ = 0; W.drain_sig = nullptr; W.drain_seq = 0; W.serial = 0; W.rng_replay = 0; W.mis_any = 0; W.late_finish = 0;
    W.gen_blocks = knob("FTN_GEN_BLOCKS", 1);
    uint32_t valid = 0; for (const DTile& t : tiles) valid += (uint32_t)((t.x1 - t.x0) * (t.y1 - t.y0));
    W.valid_per_sample = valid;
    GbParams G;
    memcpy(G.w2c, w2c, sizeof(G.w2c)); G.out = d_out; G.spillA = spill_a; G.spillB = spill_b; G.spillC = spill_c; G.rec = st->pd;         /* the path integrator's 64-byte records: 3 float4 per path used */
    const bool spheres = P.S.n_spheres != 0, tex = P.S.n_textures != 0;
    const size_t lds = wf_trace_lds(P.stack_entries);
    const unsigned trace_grid_max = wf_trace_grid_max(st, lds);
    double trace_ms = 0.0;
    for (uint32_t s0 = 0; s0 < total_samples; s0 += S) {
        const uint32_t Sp = std::min(S, total_samples - s0);
        W.n_slots = n_slots; W.samples = Sp; W.n_paths = Sp * n_slots; W.first_sample = P.first_sample + s0; W.seg_cap = (uint32_t)st->cap_paths;
        launch_wf_new_pass(W, P.stats, stream);
        launch_wf_generate(P, W, 0, stream);
        const unsigned tg = std::min<unsigned>(trace_grid_max, (2 * W.n_paths + 255) / 256);
        uint32_t n_q = Sp * valid;
        for (uint32_t r = 0;; r++) {
            /* round r traces the queue of round r - 1's pass-throughs; the two queues alternate between q_closest (count WFC_CLOSEST) and q_shadow (WFC_SHADOW) */
            const bool odd = (r & 1u) != 0;
            const uint32_t* q_in = odd ? W.q_shadow : W.q_closest;
            uint32_t* q_out = odd ? W.q_closest : W.q_shadow;
            const uint32_t c_in = odd ? WFC_SHADOW : WFC_CLOSEST, c_out = odd ? WFC_CLOSEST : WFC_SHADOW;
            if (r > 0) hipLaunchKernelGGL(k_gb_reset, dim3(1), dim3(64), 0, stream, W, c_out);
            WF_TRY(hipEventRecord(st->ev[0], stream));
            launch_trace(st, false, 0, spheres, tg, lds, stream, P, W, q_in, &W.counters[CTR(c_in)], &W.counters[CTR(WFC_HEAD_CLOSEST)], 2 * W.n_paths,
                         r == 0 && W.samples >= knob("FTN_T4_LOCKSTEP_MIN_SPP", 1) /* the camera rays: lockstep parameters, as the beauty's first launch */);
            WF_TRY(hipEventRecord(st->ev[1], stream));
            const dim3 sg(std::max<uint32_t>(1u, (n_q + 255) / 256));
            if (tex) hipLaunchKernelGGL(k_gb_shade<true>, sg, dim3(256), 0, stream, P, W, G, q_in, &W.counters[CTR(c_in)], q_out, &W.counters[CTR(c_out)]);
            else hipLaunchKernelGGL(k_gb_shade<false>, sg, dim3(256), 0, stream, P, W, G, q_in, &W.counters[CTR(c_in)], q_out, &W.counters[CTR(c_out)]);
            WF_TRY(hipMemcpyAsync(st->host_counters, W.counters, 16 * 32 * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
            WF_TRY(hipStreamSynchronize(stream));
            float ms = 0.0f; (void)hipEventElapsedTime(&ms, st->ev[0], st->ev[1]); trace_ms += ms;
            n_q = st->host_counters[CTR(c_out)];
            if (n_q == 0) break;
            if (r == GB_MAX_PASS_THROUGH) {
                wf_set_error("a camera ray passed through more than 4096 null-material surfaces: the G-buffer would be incomplete");
                return FTN_ERR_INTERNAL;
            }
        }
        hipLaunchKernelGGL(k_gb_accumulate, dim3((n_slots + 255) / 256), dim3(256), 0, stream, P, W, G);
    }
    const size_t npix = (size_t)std::max(0, P.crop[2] - P.crop[0]) * (size_t)std::max(0, P.crop[3] - P.crop[1]);
    if (npix) hipLaunchKernelGGL(k_gb_merge, dim3((unsigned)std::min<size_t>((npix + 255) / 256, 4096)), dim3(256), 0, stream, G, npix, (const DevStats*)P.stats);
    WF_TRY(hipGetLastError());
    if (trace_ms_out) *trace_ms_out = trace_ms;
    return FTN_OK;
}

}  // namespace ftn
