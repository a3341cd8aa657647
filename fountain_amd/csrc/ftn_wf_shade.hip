/*
 * ftn_wf_shade.hip -- the shading passes on the wavefront queues: the path integrator's (PathIntegrator::incident_radiance,
 * path.rs:25-95), and DirectLightingIntegrator's / WhittedIntegrator's:
 *
 *   k_wf_classify    groups the active paths by shading class (finished / missed / one per material type / null material)
 *   k_wf_shade<TEX, MT, ENV>  everything between two intersect calls of the Li loop: resolves the previous bounce's direct lighting
 *                    (shadow + MIS results), emission, termination, Material -> Bsdf, uniform_sample_one_light /
 *                    estimate_direct set-up, BSDF sampling, Russian roulette; emits shadow / MIS / continuation rays and
 *                    compacts the surviving paths into the next queue (one atomic per workgroup and queue).  One launch per
 *                    material type present, BSDF code specialised at compile time; ENV: the scene's only light is an
 *                    InfiniteAreaLight whose record travels in the kernel arguments.
 *   k_wf_shade_dl<WHITTED, TEX>  the same step of the other two integrators, all classes in one launch
 *   k_batch_finish   the hit records and surface interactions that a ray batch returns (wavefront_trace_batch, ftn_wf_trace.hip)
 *
 * launch_wf_classify, launch_wf_shade and launch_wf_shade_dl are what the two render drivers (ftn_wavefront.hip) call.  All per-path
 * arithmetic and the order of the RNG draws are those of the reference (and of the megakernel), so both pipelines produce identical radiance.
 *
 * Every kernel that builds a surface interaction or a run-time-typed BSDF is in this ONE unit on purpose.  Device helpers have internal
 * linkage, so the optimiser specialises make_interaction and make_bsdf<-1> for the arguments their callers OF THE UNIT pass (the
 * differentials pointer; allow_multiple_lobes, true in k_wf_shade and false in k_wf_shade_dl).  With k_wf_shade_dl or k_batch_finish in a
 * unit of their own, they and k_wf_shade<*, -1, *> compile to other instructions and registers (profiles/wf_split/README.md).
 */
#include "ftn_wf_internal.h"
#include "ftn_wf_path.h"
#include "ftn_texture.h"
#include <algorithm>

namespace ftn {

/* ------------------------------------------------------------------ material-sorted shading: group the active queue by shading class
 * class 0: finished paths that only need their pending direct term resolved; 1: alive, ray escaped or depth limit reached
 * (emission / environment only); 2..: alive hit, by material type (2 + FTN_MAT_*), 7: primitive without material.
 * Two passes (count, scatter) with block-level ballots; class segments start at multiples of 256 so that every shade
 * workgroup sees a single class and its branches on hit/material are wave-uniform. */
__device__ inline uint32_t wf_class_of(const RenderParams& P, const WfBuffers& W, uint32_t entry) {
    /* an active-queue entry says whether the path has ended / reached max_depth (WF_Q_*), hit_prim is a dense array, the primitive's
     * class is a byte (DScene::prim_class): nothing here gathers from the path state or the 32-byte prim_info records */
    if (entry & WF_Q_FIN) return 0u;
    const int prim = W.hit_prim[entry & WF_Q_ID_MASK];
    if (prim < 0 || (entry & WF_Q_DEPTH)) return 1u;
    return P.S.prim_class[prim];
}
/* Each class owns a segment of `seg_cap` slots in q_sorted (worst case: every path in one class).  A workgroup classifies all of
 * its rounds first (class codes and per-wave counts stay in LDS), reserves its slots with ONE global atomic per class -- with one
 * atomic per class and round the kernel ran at the rate of same-address atomics (65 k of them on the busiest counter) -- and
 * then writes its paths.  The shade kernel derives the 256-aligned virtual layout from the 8 counts itself. */
#define WF_CLS_ROUNDS 32
__global__ void __launch_bounds__(256) k_wf_classify(RenderParams P, WfBuffers W, int in_q, uint32_t drop /* classes whose entries leave the queues here (late finish) */) {
    __shared__ unsigned char s_cls[WF_CLS_ROUNDS][256];
    __shared__ uint32_t s_cnt[WF_CLS_ROUNDS][WF_NCLASS][4];        /* per round, class, wave */
    __shared__ uint32_t s_pre[WF_CLS_ROUNDS][WF_NCLASS];           /* slots of the class used by earlier rounds of this workgroup */
    __shared__ uint32_t s_base[WF_NCLASS];
    const uint32_t count = W.counters[CTR(in_q == 0 ? WFC_ACTIVE_A : WFC_ACTIVE_B)];
    const uint32_t stride = gridDim.x * 256u, rounds = (count + stride - 1) / stride;
    const uint32_t wave = threadIdx.x >> 6, lane = lane_id();
    for (uint32_t r0 = 0; r0 < rounds; r0 += WF_CLS_ROUNDS) {
        const uint32_t nr = rounds - r0 < WF_CLS_ROUNDS ? rounds - r0 : WF_CLS_ROUNDS;
        for (uint32_t r = 0; r < nr; r++) {                        /* 1: classify */
            const uint32_t qi = (r0 + r) * stride + blockIdx.x * 256u + threadIdx.x;
            uint32_t c = WF_NCLASS;
            if (qi < count) { c = wf_class_of(P, W, W.q_active[in_q][qi]); if ((drop >> c) & 1u) c = WF_NCLASS; }
            s_cls[r][threadIdx.x] = (unsigned char)c;
#pragma unroll
            for (int k = 0; k < WF_NCLASS; k++) {
                const unsigned long long m = __ballot(c == (uint32_t)k);
                if (lane == 0) s_cnt[r][k][wave] = (uint32_t)__popcll(m);
            }
        }
        __syncthreads();
        if (threadIdx.x < WF_NCLASS) {                             /* 2: reserve */
            const uint32_t k = threadIdx.x; uint32_t tot = 0;
            for (uint32_t r = 0; r < nr; r++) { s_pre[r][k] = tot; tot += s_cnt[r][k][0] + s_cnt[r][k][1] + s_cnt[r][k][2] + s_cnt[r][k][3]; }
            s_base[k] = tot ? atomicAdd(&W.cls[CTR(k)], tot) : 0u;
        }
        __syncthreads();
        for (uint32_t r = 0; r < nr; r++) {                        /* 3: write */
            const uint32_t qi = (r0 + r) * stride + blockIdx.x * 256u + threadIdx.x;
            const uint32_t c = s_cls[r][threadIdx.x];
            unsigned long long mine = 0;
#pragma unroll
            for (int k = 0; k < WF_NCLASS; k++) { const unsigned long long m = __ballot(c == (uint32_t)k); if (c == (uint32_t)k) mine = m; }
            if (c < WF_NCLASS) {
                uint32_t off = s_base[c] + s_pre[r][c];
                for (uint32_t w2 = 0; w2 < wave; w2++) off += s_cnt[r][c][w2];
                W.q_sorted[(size_t)c * W.seg_cap + off + (uint32_t)__popcll(mine & ((1ull << lane) - 1ull))] = W.q_active[in_q][qi] & WF_Q_ID_MASK;
            }
        }
        __syncthreads();
    }
}

/* ------------------------------------------------------------------ shade */
#ifndef FTN_SHADE_MIN_WAVES
#define FTN_SHADE_MIN_WAVES 1
#endif
#ifndef FTN_SHADE_WAVES_NOBSDF
#define FTN_SHADE_WAVES_NOBSDF 4      /* finished paths / misses (5 waves: 96 registers, no scratch -- measured equal: 99.3 against 99.5 ms of shading) */
#endif
#ifndef FTN_SHADE_WAVES_MATTE
#define FTN_SHADE_WAVES_MATTE 3
#endif
#ifndef FTN_SHADE_WAVES_OTHER
#define FTN_SHADE_WAVES_OTHER 3
#endif
/* MT: -1 = every class in `class_mask`, material type read at run time (textured scenes);  0..4 = ONE material class, its BSDF code
 * specialised at compile time (fewer registers: 3 waves/SIMD instead of 2, 4 for mirrors);  -2 = the classes without a BSDF
 * (finished paths, misses / depth limit, null materials), the material branch compiled out. */
/* ENV: the scene's only light is an InfiniteAreaLight (DScene::env_only).  Its record is read from the kernel arguments (scalar
 * loads instead of one gather per field and lane) and the point / distant / area-light code is compiled out; every value computed
 * is the one the generic kernel computes for such a scene. */
template <bool TEX, int MT, bool ENV>
__global__ void __launch_bounds__(256, (MT == -1 ? FTN_SHADE_MIN_WAVES : (MT == -2 ? FTN_SHADE_WAVES_NOBSDF : (MT == 0 ? FTN_SHADE_WAVES_MATTE : FTN_SHADE_WAVES_OTHER)))) k_wf_shade(RenderParams P, WfBuffers W, int in_q, uint32_t class_mask, uint32_t first /* 1: the pass right behind k_wf_generate -- every path is fresh */) {
    const DScene& S = P.S;
    /* virtual, 256-aligned concatenation of the selected class segments: a workgroup never straddles two classes */
    uint32_t cbase[WF_NCLASS + 1], ccnt[WF_NCLASS];
    cbase[0] = 0;
#pragma unroll
    for (int k = 0; k < WF_NCLASS; k++) { ccnt[k] = ((class_mask >> k) & 1u) ? W.cls[CTR(k)] : 0u; cbase[k + 1] = cbase[k] + ((ccnt[k] + 255u) & ~255u); }
    const uint32_t count = cbase[WF_NCLASS];
    uint32_t* out_q = W.q_active[in_q ^ 1];
    uint32_t* out_count = &W.counters[CTR(in_q == 0 ? WFC_ACTIVE_B : WFC_ACTIVE_A)];
    int err = 0;
    const uint32_t stride = gridDim.x * 256u;
    const uint32_t rounds = (count + stride - 1) / stride;
    for (uint32_t round = 0; round < rounds; round++) {
        const uint32_t qi = round * stride + blockIdx.x * 256u + threadIdx.x;
        bool have = false;
        uint32_t sorted_idx = 0;
        if (qi < count) {                                  /* which class segment does this slot belong to, and is it occupied? */
            uint32_t c = 0, cb = 0, cc = ccnt[0];
#pragma unroll
            for (int k = 1; k < WF_NCLASS; k++) if (qi >= cbase[k]) { c = (uint32_t)k; cb = cbase[k]; cc = ccnt[k]; }
            have = qi - cb < cc;
            sorted_idx = c * W.seg_cap + (qi - cb);
        }
        bool push_active = false, push_closest = false, push_mis = false, push_shadow = false, push_mis_any = false;
        uint32_t p = 0, active_entry = 0;
        if (have) {
            p = W.q_sorted[sorted_idx];
            float4 bq = make_float4(1.0f, 1.0f, 1.0f, __uint_as_float(PS_ALIVE)), lq = make_float4(0.0f, 0.0f, 0.0f, 0.0f);       /* a fresh path (k_wf_generate) */
            if (!first) { if (W.br) { bq = W.br[2 * (size_t)p]; lq = W.br[2 * (size_t)p + 1]; } else { bq = W.beta[p]; lq = W.rad[p]; } }
            Rgb beta(bq.x, bq.y, bq.z), L(lq.x, lq.y, lq.z);
            uint32_t ps = __float_as_uint(bq.w);
            /* ---- finish the previous bounce's estimate_direct (integrator/mod.rs:330-392) */
            if (ps & PS_DIRECT) {
                float4 q0, q1, q2, q3 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                if (W.pd) { const float4* Q = W.pd + 4 * (size_t)p; q0 = Q[0]; q1 = Q[1]; q2 = Q[2]; if (W.pd_md) q3 = Q[3]; } else { q0 = W.pend0[p]; q1 = W.pend1[p]; q2 = W.pend2[p]; }
                const uint32_t occ_word = __float_as_uint(q3.w);      /* pd_occ: the any-hit results of this path's two rays (store_occluded) */
                const bool shadow_lit = (ps & PS_SHADOW) && !(W.pd_occ ? (occ_word & 0xffu) != 0u : W.occluded[p] != 0);
                Rgb inc(0.0f);                                   /* what arrives along the MIS ray */
                if (ps & PS_MIS_ANY) {                           /* infinite light: the BSDF-sampled ray either escapes to it or contributes nothing (mod.rs:367-384) */
                    const int light_index = (int)__float_as_uint(lq.w);
                    const DLight& Lt = ENV ? S.env0 : S.lights[light_index];
                    const float4 md = W.pd_md ? q3 : W.ray[2 * (size_t)(p + W.n_paths) + 1];
                    if (!(W.pd_occ ? (occ_word & 0xff00u) != 0u : W.occluded[p + W.n_paths] != 0)) inc = light_Le_env(Lt, V3(md.x, md.y, md.z));
                } else if (ps & PS_MIS) {
                    const int light_index = (int)__float_as_uint(lq.w);
                    const DLight& Lt = ENV ? S.env0 : S.lights[light_index];
                    const DHit mh = load_hit(W, p + W.n_paths);
                    const float4 mo = W.ray[2 * (size_t)(p + W.n_paths)], md = W.ray[2 * (size_t)(p + W.n_paths) + 1];
                    if (mh.prim >= 0) {
                      if (!ENV) {                                /* ENV: no primitive carries an area light */
                        int h_mat, h_light; prim_mat_light(S, mh.prim, &h_mat, &h_light);
                        if (h_light >= 0 && h_light == light_index) {
                            DRay r0; r0.o = V3(mo.x, mo.y, mo.z); r0.d = V3(md.x, md.y, md.z); r0.t_max = FTN_INF; r0.time = 0.0f;
                            DSI s2; make_interaction(S, mh, r0, &s2);
                            inc = area_Le(Lt, s2.hit.n, -r0.d);
                        }
                      }
                    } else if (ENV || Lt.kind == LK_INFINITE) inc = light_Le_env(Lt, V3(md.x, md.y, md.z));
                }
                L = wf_add_direct(L, shadow_lit, q0, q1, q2, inc, S.n_lights);
                ps &= ~(PS_DIRECT | PS_SHADOW | PS_MIS | PS_MIS_ANY);
            }
            if (!(ps & PS_ALIVE)) {
                W.rad[p] = make_float4(L.r, L.g, L.b, 0.0f);     /* path finished: final radiance (the rest of its state is never read again) */
            } else {
                DRay ray0; ray0.o = V3(0.0f, 0.0f, 0.0f); ray0.d = V3(0.0f, 0.0f, 1.0f); ray0.t_max = FTN_INF; ray0.time = 0.0f;
                DHit h; h.t = FTN_INF; h.b0 = 0.0f; h.b1 = 0.0f; h.b2 = 0.0f; h.prim = -1;
                /* the light kernel of the classes without a BSDF mostly sees paths whose ray escaped: all such a path needs is that fact (hit_prim),
                 * unless it looks at the environment along the ray -- camera rays and specular bounces (path.rs:45-58).  Its ray and hit records are
                 * then not read at all */
                bool need_ray = true;
                if (MT == -2 && !first) { h.prim = W.hit_prim[p]; need_ray = h.prim >= 0 || (ps & PS_BOUNCE_MASK) == 0u || (ps & PS_SPECULAR) != 0u; }
                if (need_ray) {
                    const float4 ro = W.ray[2 * (size_t)(p)], rdv = W.ray[2 * (size_t)(p) + 1];
                    ray0.o = V3(ro.x, ro.y, ro.z); ray0.d = V3(rdv.x, rdv.y, rdv.z); ray0.t_max = rdv.w;
                    h = load_hit(W, p);
                }
                const bool hit = h.prim >= 0;
                uint32_t bounces = ps & PS_BOUNCE_MASK;
                const bool specular_bounce = (ps & PS_SPECULAR) != 0;
                DSI si;
                if (hit) make_interaction(S, h, ray0, &si);
                if (bounces == 0 || specular_bounce) {
                    if (hit) {
                        Rgb e(0.0f);
                        if (!ENV && si.light >= 0) e = area_Le(S.lights[si.light], si.hit.n, -ray0.d);
                        L = wf_add_seen(L, beta, e);
                    } else L = wf_add_seen(L, beta, wf_escaped_Le<ENV>(S, ray0.d));
                }
                bool alive = true;
                uint32_t light_word = 0;
                if (!hit || bounces >= P.max_depth) alive = false;
                else {
                    Rng rng;
                    if (first) {      /* the stream behind the camera sample's five draws (p_film 2, p_lens 2, time 1: sampler/mod.rs:43-51), as k_wf_generate left it */
                        const uint32_t slot = p / W.samples, sidx = p % W.samples;
                        const DTile tile = P.tiles[slot >> 8];
                        rng.seed(indexed_key(P.seed, tile.x0 + (int)(slot & 15u), tile.y0 + (int)((slot >> 4) & 15u), W.first_sample + sidx));
                        (void)rng.next2(); (void)rng.next2(); (void)rng.next();
                    } else if (W.rng_replay) {   /* the same stream, re-created: seed of the sample's key, then the draws the path has made so far */
                        const uint32_t slot = p / W.samples, sidx = p % W.samples;
                        const DTile tile = P.tiles[slot >> 8];
                        rng.seed(indexed_key(P.seed, tile.x0 + (int)(slot & 15u), tile.y0 + (int)((slot >> 4) & 15u), W.first_sample + sidx));
                        rng.skip(ps >> PS_DRAWS_SHIFT);
                    } else { ulonglong2 a = W.rng01[p], b = W.rng23[p]; rng.s0 = a.x; rng.s1 = a.y; rng.s2 = b.x; rng.s3 = b.y; }
                    uint32_t n_draws = first ? 5u : (ps >> PS_DRAWS_SHIFT);
                    const int mat = si.mat;
                    if (MT == -2 || mat < 0) {
                        DRay nr = spawn_ray(si.hit, ray0.d);                       /* null bsdf: path.rs:77-81 */
                        W.ray[2 * (size_t)(p)] = make_float4(nr.o.x, nr.o.y, nr.o.z, 0.0f); W.ray[2 * (size_t)(p) + 1] = make_float4(nr.d.x, nr.d.y, nr.d.z, nr.t_max);
                        push_closest = true;
                    } else {
                        DBsdf B;
                        ftn_material mloc; const ftn_material* mp = &S.materials[mat];
                        if (TEX && material_is_textured(S, mat)) {
                            /* Texture::evaluate(si).  The differentials are the CAMERA ray's, handed on unchanged by the path integrator
                             * (path.rs:73): rebuilt here from the path's sample key instead of being carried in the path state. */
                            DRayDiff rd;
                            if (W.serial) {                      /* (no sample key in the tile-serial stream: k_wf_serial_advance stored them) */
                                const float4 d0 = W.dfd[p], d1 = W.dfd[(size_t)W.n_paths + p], d2 = W.dfd[2 * (size_t)W.n_paths + p];
                                rd.has = true; rd.rxo = V3(d0.x, d0.y, d0.z); rd.ryo = V3(d1.x, d1.y, d1.z); rd.ryd = V3(d2.x, d2.y, d2.z); rd.rxd = V3(d0.w, d1.w, d2.w);
                            } else {
                                const uint32_t slot = p / W.samples, sidx = p % W.samples;
                                const DTile tile = P.tiles[slot >> 8];
                                const int px = tile.x0 + (int)(slot & 15u), py = tile.y0 + (int)((slot >> 4) & 15u);
                                Rng crng; crng.seed(indexed_key(P.seed, px, py, W.first_sample + sidx));
                                const V2 j = crng.next2(); const V2 p_film((float)px + j.x, (float)py + j.y); const V2 p_lens = crng.next2(); const float time_u = crng.next();
                                const DRay cam = camera_ray(P.C, p_film, p_lens, time_u);
                                rd = camera_ray_diff(P.C, p_film, p_lens, cam, 1.0f / sqrtf((float)P.spp));
                            }
                            DSIX ex; DSI s2; make_interaction(S, h, ray0, &s2, &ex);
                            const DTexDiffs td = compute_tex_diffs(si.hit.p, si.hit.n, ex.dpdu, ex.dpdv, rd);
                            mloc = material_resolve(S, mat, ex.uv, td); mp = &mloc;
                        }
                        if (!make_bsdf<(MT >= 0 ? MT : -1)>(*mp, si, true, &B)) { err = FTN_ERR_UNSUPPORTED; alive = false; }
                        else {
                            if (bsdf_num(B, T_ALL & ~T_SPECULAR) > 0 && S.n_lights > 0) {
                                /* uniform_sample_one_light + first half of estimate_direct (integrator/mod.rs:289-329) */
                                const uint32_t nl = S.n_lights;
                                const uint32_t ln = (uint32_t)f2usize(fmin_(rng.next() * (float)nl, (float)(nl - 1)));
                                const V2 ul = rng.next2(), us = rng.next2();
                                n_draws += 5u;
                                const DLight& Lt = ENV ? S.env0 : S.lights[ln];
                                const uint32_t flags = T_ALL & ~T_SPECULAR;
                                const bool delta = !ENV && (Lt.kind == LK_POINT || Lt.kind == LK_DISTANT);
                                ps |= PS_DIRECT; light_word = ln;
                                Rgb ld(0.0f); float mis_w = 0.0f, mis_pdf = 1.0f; Rgb mis_f(0.0f); V3 mis_d(0.0f, 0.0f, 0.0f);
                                DLiSample ls = ENV ? light_sample_env(Lt, si.hit, ul) : light_sample(S, Lt, si.hit, ul);
                                if (ls.pdf > 0.0f && !ls.radiance.is_black()) {
                                    Rgb f = bsdf_f(B, si.wo, ls.wi, flags) * abs_dot(ls.wi, si.shading_n);
                                    float sp = bsdf_pdf(B, si.wo, ls.wi, flags);
                                    if (!f.is_black()) {
                                        DRay sr = spawn_ray_to_hit(si.hit, ls.p1);
                                        W.sh[2 * (size_t)(p)] = make_float4(sr.o.x, sr.o.y, sr.o.z, 0.0f); W.sh[2 * (size_t)(p) + 1] = make_float4(sr.d.x, sr.d.y, sr.d.z, sr.t_max);
                                        ld = delta ? (f * ls.radiance / ls.pdf) : (f * ls.radiance * power_heuristic(ls.pdf, sp) / ls.pdf);
                                        ps |= PS_SHADOW; push_shadow = true;
                                    }
                                }
                                if (!delta) {
                                    DScatter sc;
                                    if (bsdf_sample(B, si.wo, us, flags, &sc)) {
                                        Rgb f = sc.f * abs_dot(sc.wi, si.shading_n);
                                        if (!f.is_black()) {
                                            bool go = true;
                                            if (sc.type & T_SPECULAR) mis_w = 1.0f;
                                            else {
                                                float lp = ENV ? light_pdf_env(Lt, sc.wi) : light_pdf(S, Lt, si.hit, sc.wi);
                                                if (lp == 0.0f) go = false; else mis_w = power_heuristic(sc.pdf, lp);
                                            }
                                            if (go) {
                                                DRay mr = spawn_ray(si.hit, sc.wi);
                                                W.ray[2 * (size_t)(p + W.n_paths)] = make_float4(mr.o.x, mr.o.y, mr.o.z, 0.0f);
                                                W.ray[2 * (size_t)(p + W.n_paths) + 1] = make_float4(mr.d.x, mr.d.y, mr.d.z, mr.t_max);
                                                mis_f = f; mis_pdf = sc.pdf; mis_d = mr.d;
                                                if (W.mis_any && (ENV || Lt.kind == LK_INFINITE)) { ps |= PS_MIS_ANY; push_mis_any = true; } else { ps |= PS_MIS; push_mis = true; }
                                            }
                                        }
                                    }
                                }
                                if (W.pd) {
                                    float4* Q = W.pd + 4 * (size_t)p;
                                    Q[0] = make_float4(ld.r, ld.g, ld.b, mis_w); Q[1] = make_float4(mis_f.r, mis_f.g, mis_f.b, mis_pdf); Q[2] = make_float4(beta.r, beta.g, beta.b, 0.0f);
                                    if (W.pd_md) Q[3] = make_float4(mis_d.x, mis_d.y, mis_d.z, 0.0f);      /* w: the any-hit kernels' result bytes */
                                } else {
                                    W.pend0[p] = make_float4(ld.r, ld.g, ld.b, mis_w);
                                    W.pend1[p] = make_float4(mis_f.r, mis_f.g, mis_f.b, mis_pdf);
                                    W.pend2[p] = make_float4(beta.r, beta.g, beta.b, 0.0f);
                                }
                            }
                            /* sample the BSDF for the next direction (path.rs:67-76) */
                            DScatter bs;
                            const V2 u = rng.next2();
                            n_draws += 2u;
                            const bool ok = bsdf_sample(B, -ray0.d, u, T_ALL, &bs);
                            if (ok && !bs.f.is_black()) {
                                beta = beta * (bs.f * abs_dot(bs.wi, si.shading_n) / bs.pdf);
                                ps = (bs.type & T_SPECULAR) ? (ps | PS_SPECULAR) : (ps & ~PS_SPECULAR);
                                DRay nr = spawn_ray(si.hit, bs.wi);
                                /* Russian roulette (path.rs:84-91) */
                                if (beta.max_component() < P.rr_threshold && bounces > 3) {
                                    float q = fmax_(0.05f, 1.0f - beta.max_component());
                                    n_draws += 1u;
                                    if (rng.next() < q) alive = false; else beta = beta / (1.0f - q);
                                }
                                if (alive) {
                                    W.ray[2 * (size_t)(p)] = make_float4(nr.o.x, nr.o.y, nr.o.z, 0.0f); W.ray[2 * (size_t)(p) + 1] = make_float4(nr.d.x, nr.d.y, nr.d.z, nr.t_max);
                                    bounces += 1; push_closest = true;
                                }
                            } else alive = false;
                        }
                    }
                    if (W.rng_replay) ps = (ps & ((1u << PS_DRAWS_SHIFT) - 1u)) | (n_draws << PS_DRAWS_SHIFT);
                    else if (alive || W.serial) { W.rng01[p] = make_ulonglong2(rng.s0, rng.s1); W.rng23[p] = make_ulonglong2(rng.s2, rng.s3); }      /* (an ended path draws nothing more; the tile-serial stream goes on behind it) */
                }
                ps = (ps & ~(PS_BOUNCE_MASK | PS_ALIVE)) | (bounces & PS_BOUNCE_MASK) | (alive ? PS_ALIVE : 0u);
                push_active = alive || (!W.late_finish && (ps & PS_DIRECT));        /* finished paths with a pending direct term come back once (late finish: k_wf_accumulate resolves it) */
                if (W.br) {
                    if (push_active || W.late_finish) {      /* (late finish: the record of an ended path is what k_wf_accumulate reads) */ W.br[2 * (size_t)p] = make_float4(beta.r, beta.g, beta.b, __uint_as_float(ps)); W.br[2 * (size_t)p + 1] = make_float4(L.r, L.g, L.b, __uint_as_float(light_word)); }
                    else W.rad[p] = make_float4(L.r, L.g, L.b, 0.0f);
                } else {
                    if (push_active) W.beta[p] = make_float4(beta.r, beta.g, beta.b, __uint_as_float(ps));        /* (a retired path's throughput is never read again) */
                    W.rad[p] = make_float4(L.r, L.g, L.b, __uint_as_float(light_word));
                }
                active_entry = p | (alive ? (bounces >= P.max_depth ? WF_Q_DEPTH : 0u) : WF_Q_FIN);
            }
            if (W.serial && !push_active) W.ser_retired[p] = 1;      /* nothing pending: k_wf_serial_advance takes it from here */
        }
        {
            const bool pred[6] = {push_active, push_closest, push_mis, push_shadow, push_mis_any, push_mis_any};
            const uint32_t val[6] = {active_entry, p, p | WF_MIS_BIT, p, p | WF_MIS_BIT, 0u};
            uint32_t* const qs[6] = {out_q, W.q_closest, W.q_closest, W.q_shadow, W.q_shadow, nullptr};        /* the last "queue" only counts (CTR(WFC_MIS_ANY)): MIS rays traced as any-hit */
            uint32_t* const cs[6] = {out_count, &W.counters[CTR(WFC_CLOSEST)], &W.counters[CTR(WFC_CLOSEST)], &W.counters[CTR(WFC_SHADOW)], &W.counters[CTR(WFC_SHADOW)], &W.counters[CTR(WFC_MIS_ANY)]};
            block_push<6>(pred, val, qs, cs);
        }
    }
    if (err) atomicCAS(&P.stats->error, 0, err);
}

/* resident workgroups of a shade kernel per CU (registers, LDS), asked once per variant */
template <bool TEX, int MT, bool ENV> static unsigned shade_wgs_per_cu() {
    static const unsigned nb = [] { int v = 0; return (hipOccupancyMaxActiveBlocksPerMultiprocessor(&v, k_wf_shade<TEX, MT, ENV>, 256, 0) == hipSuccess && v >= 1) ? (unsigned)(v > 8 ? 8 : v) : 3u; }();
    return nb;
}

/* ------------------------------------------------------------------ DirectLightingIntegrator / WhittedIntegrator through the queues
 * (direct_lighting.rs:50-110, whitted.rs:20-75, specular_reflect / specular_transmit integrator/mod.rs:39-178)
 *
 * Their radiance is a NESTED product: Li(depth d) = local_d + f_d * Li(depth d + 1) * |cos_d| / pdf_d, evaluated innermost first.
 * A wavefront walks the chain forwards, so every depth keeps its terms -- dlA[d] = {local_d.rgb, pdf_d}, dlB[d] = {f_d.rgb, |cos_d|},
 * level-major SoA -- and the path is folded from its deepest level when it ends (dl_unwind: the same expressions, in the same order,
 * as the megakernel's direct_li and as the recursion they restate).  Only chains are supported, as in the megakernel: a BSDF with
 * both specular lobes (specular glass) reports FTN_ERR_UNSUPPORTED like the reference's todo!(); so does a primitive without material
 * (unimplemented!() at direct_lighting.rs:103) and a chain longer than WF_DL_MAX levels.
 * Per level: `local` = emitted radiance (direct lighting only) + the direct term.  DirectLightingIntegrator: uniform_sample_one_light,
 * the same deferred shadow / MIS rays as the path integrator (resolved when the path comes back after the traces), but called for every
 * BSDF (no "has non-specular lobes" test) and not weighted by a throughput.  WhittedIntegrator: every light once, one 2D sample and one
 * shadow ray each (ray l of path p in slot p + l * n_paths), up to WF_WH_MAX_LIGHTS lights; no MIS ray, no emitted term.
 * TEX (scenes with textures): texture lookups need the ray differentials, which these integrators carry along the specular chain
 * (specular_reflect updates them, integrator/mod.rs:58-84): level 0 rebuilds the camera ray's from the path's sample key (as k_wf_shade
 * does at every bounce), deeper levels read what the level above stored in WfBuffers::dfd.
 * The 2D sample of specular_transmit is drawn after the reflect recursion returns and never used by a supported material: with one
 * stream per camera sample (the indexed sampler, the only one the wavefront runs) skipping it changes nothing. */
__device__ inline void dl_unwind(const RenderParams& P, const WfBuffers& W, uint32_t p, uint32_t depth, bool have_tail, Rgb tail) {
    Rgb li = have_tail ? tail : Rgb(0.0f);
    bool child = have_tail;
    for (int d = (int)depth - 1; d >= 0; d--) {
        const float4 a = W.dlA[(size_t)d * W.n_paths + p];
        Rgb r(a.x, a.y, a.z);
        if (child) { const float4 b = W.dlB[(size_t)d * W.n_paths + p]; r = r + Rgb(b.x, b.y, b.z) * li * b.w / a.w; }
        else if ((uint32_t)d + 1 < P.max_depth) r = r + Rgb(0.0f);                   /* radiance += specular_reflect (= 0) */
        if ((uint32_t)d + 1 < P.max_depth) r = r + Rgb(0.0f);                        /* radiance += specular_transmit (= 0) */
        li = r; child = true;
    }
    W.rad[p] = make_float4(li.r, li.g, li.b, 0.0f);
}

template <bool WHITTED, bool TEX>
__global__ void __launch_bounds__(256) k_wf_shade_dl(RenderParams P, WfBuffers W, int in_q) {
    const DScene& S = P.S;
    uint32_t cbase[WF_NCLASS + 1], ccnt[WF_NCLASS];
    cbase[0] = 0;
#pragma unroll
    for (int k = 0; k < WF_NCLASS; k++) { ccnt[k] = W.cls[CTR(k)]; cbase[k + 1] = cbase[k] + ((ccnt[k] + 255u) & ~255u); }
    const uint32_t count = cbase[WF_NCLASS];
    uint32_t* out_q = W.q_active[in_q ^ 1];
    uint32_t* out_count = &W.counters[CTR(in_q == 0 ? WFC_ACTIVE_B : WFC_ACTIVE_A)];
    int err = 0;
    const uint32_t stride = gridDim.x * 256u;
    const uint32_t rounds = (count + stride - 1) / stride;
    const uint32_t nl = S.n_lights;
    for (uint32_t round = 0; round < rounds; round++) {
        const uint32_t qi = round * stride + blockIdx.x * 256u + threadIdx.x;
        bool have = false; uint32_t sorted_idx = 0;
        if (qi < count) {
            uint32_t c = 0, cb = 0, cc = ccnt[0];
#pragma unroll
            for (int k = 1; k < WF_NCLASS; k++) if (qi >= cbase[k]) { c = (uint32_t)k; cb = cbase[k]; cc = ccnt[k]; }
            have = qi - cb < cc;
            sorted_idx = c * W.seg_cap + (qi - cb);
        }
        bool push_active = false, push_closest = false, push_mis = false, push_mis_any = false;
        uint32_t sh_mask = 0;                                    /* shadow rays this path emits: bit l = the ray in slot p + l * n_paths (Whitted: one per light) */
        uint32_t p = 0, active_entry = 0;
        if (have) {
            p = W.q_sorted[sorted_idx];
            const float4 bq = W.beta[p], lq = W.rad[p];
            uint32_t ps = __float_as_uint(bq.w);
            uint32_t depth = ps & PS_BOUNCE_MASK;                 /* levels stored so far = index of the level shaded now */
            /* ---- finish the direct term of level depth - 1 (its rays have been traced) */
            if (ps & PS_DIRECT) {
                const uint32_t lv = depth - 1u;
                float4 a = W.dlA[(size_t)lv * W.n_paths + p];
                Rgb rad(a.x, a.y, a.z);
                if (WHITTED) {                                   /* whitted.rs:42-58: radiance += f * Li * |cos| / pdf for every unoccluded light, in light order */
                    const uint32_t mask = __float_as_uint(lq.w);
                    for (uint32_t l = 0; l < nl; l++) if ((mask >> l) & 1u) {
                        const float4 t = W.whT[(size_t)l * W.n_paths + p];
                        if (!W.occluded[p + (size_t)l * W.n_paths]) rad = rad + Rgb(t.x, t.y, t.z);
                    }
                } else {                                         /* uniform_sample_one_light = n_lights * estimate_direct (integrator/mod.rs:289-395) */
                    const float4 q0 = W.pend0[p], q1 = W.pend1[p];
                    Rgb radiance(0.0f);
                    if ((ps & PS_SHADOW) && !W.occluded[p]) radiance = radiance + Rgb(q0.x, q0.y, q0.z);
                    const int light_index = (int)__float_as_uint(lq.w);
                    const DLight& Lt = S.lights[light_index];
                    if (ps & PS_MIS_ANY) {
                        const float4 md = W.ray[2 * (size_t)(p + W.n_paths) + 1];
                        Rgb inc(0.0f);
                        if (!W.occluded[p + W.n_paths]) inc = light_Le_env(Lt, V3(md.x, md.y, md.z));
                        if (!inc.is_black()) radiance = radiance + Rgb(q1.x, q1.y, q1.z) * inc * q0.w / q1.w;
                    } else if (ps & PS_MIS) {
                        const DHit mh = load_hit(W, p + W.n_paths);
                        const float4 mo = W.ray[2 * (size_t)(p + W.n_paths)], md = W.ray[2 * (size_t)(p + W.n_paths) + 1];
                        Rgb inc(0.0f);
                        if (mh.prim >= 0) {
                            int h_mat, h_light; prim_mat_light(S, mh.prim, &h_mat, &h_light);
                            if (h_light >= 0 && h_light == light_index) {
                                DRay r0; r0.o = V3(mo.x, mo.y, mo.z); r0.d = V3(md.x, md.y, md.z); r0.t_max = FTN_INF; r0.time = 0.0f;
                                DSI s2; make_interaction(S, mh, r0, &s2);
                                inc = area_Le(Lt, s2.hit.n, -r0.d);
                            }
                        } else if (Lt.kind == LK_INFINITE) inc = light_Le_env(Lt, V3(md.x, md.y, md.z));
                        if (!inc.is_black()) radiance = radiance + Rgb(q1.x, q1.y, q1.z) * inc * q0.w / q1.w;
                    }
                    rad = rad + (float)nl * radiance;
                }
                a.x = rad.r; a.y = rad.g; a.z = rad.b;
                W.dlA[(size_t)lv * W.n_paths + p] = a;
                ps &= ~(PS_DIRECT | PS_SHADOW | PS_MIS | PS_MIS_ANY);
            }
            if (!(ps & PS_ALIVE)) {
                dl_unwind(P, W, p, depth, false, Rgb(0.0f));       /* the chain ended at its last level: fold it */
                W.beta[p] = make_float4(0.0f, 0.0f, 0.0f, __uint_as_float(ps));
            } else {
                const float4 ro = W.ray[2 * (size_t)(p)], rdv = W.ray[2 * (size_t)(p) + 1];
                DRay ray0; ray0.o = V3(ro.x, ro.y, ro.z); ray0.d = V3(rdv.x, rdv.y, rdv.z); ray0.t_max = rdv.w; ray0.time = 0.0f;
                const DHit h = load_hit(W, p);
                bool alive = false; uint32_t light_word = 0; bool ended = false;
                if (h.prim < 0) { dl_unwind(P, W, p, depth, true, scene_env_Le(S, ray0.d)); ended = true; }      /* None => environment_emitted_radiance */
                else if (depth >= WF_DL_MAX) { err = FTN_ERR_UNSUPPORTED; ended = true; }
                else {
                    DSI si; make_interaction(S, h, ray0, &si);
                    DBsdf B;
                    ftn_material mloc; const ftn_material* mp = si.mat >= 0 ? &S.materials[si.mat] : nullptr;
                    DSIX ex; DTexDiffs td; float bsdf_eta = 1.0f; DRayDiff rd; rd.has = false;
                    if (TEX && mp) {                              /* as direct_li<TEX> (ftn_kernels.hip): differentials of this level, textured parameters resolved per hit */
                        if (depth == 0u) {
                            const uint32_t slot = p / W.samples, sidx = p % W.samples;
                            const DTile tile = P.tiles[slot >> 8];
                            const int px = tile.x0 + (int)(slot & 15u), py = tile.y0 + (int)((slot >> 4) & 15u);
                            Rng crng; crng.seed(indexed_key(P.seed, px, py, W.first_sample + sidx));
                            const V2 j = crng.next2(); const V2 p_film((float)px + j.x, (float)py + j.y); const V2 p_lens = crng.next2(); const float time_u = crng.next();
                            const DRay cam = camera_ray(P.C, p_film, p_lens, time_u);
                            rd = camera_ray_diff(P.C, p_film, p_lens, cam, 1.0f / sqrtf((float)P.spp));
                        } else {
                            const float4 d0 = W.dfd[p], d1 = W.dfd[(size_t)W.n_paths + p], d2 = W.dfd[2 * (size_t)W.n_paths + p];
                            rd.has = true; rd.rxo = V3(d0.x, d0.y, d0.z); rd.ryo = V3(d1.x, d1.y, d1.z); rd.ryd = V3(d2.x, d2.y, d2.z); rd.rxd = V3(d0.w, d1.w, d2.w);
                        }
                        DSI s2; make_interaction(S, h, ray0, &s2, &ex);
                        td = compute_tex_diffs(si.hit.p, si.hit.n, ex.dpdu, ex.dpdv, rd);
                        if (material_is_textured(S, si.mat)) { mloc = material_resolve(S, si.mat, ex.uv, td); mp = &mloc; }
                        if (mp->type == FTN_MAT_GLASS) bsdf_eta = mp->s0;
                    }
                    if (!mp || !make_bsdf<-1>(*mp, si, false, &B)) { err = FTN_ERR_UNSUPPORTED; ended = true; }
                    else {
                        Rng rng; { ulonglong2 a = W.rng01[p], b = W.rng23[p]; rng.s0 = a.x; rng.s1 = a.y; rng.s2 = b.x; rng.s3 = b.y; }
                        Rgb rad(0.0f);
                        if (WHITTED) {
                            uint32_t mask = 0;
                            if (nl > WF_WH_MAX_LIGHTS) err = FTN_ERR_UNSUPPORTED;
                            else for (uint32_t l = 0; l < nl; l++) {
                                const DLight& Lt = S.lights[l];
                                DLiSample ls = light_sample(S, Lt, si.hit, rng.next2());
                                if (ls.radiance.is_black() || ls.pdf == 0.0f) continue;
                                Rgb f = bsdf_f(B, si.wo, ls.wi, T_ALL);
                                if (!f.is_black()) {
                                    DRay sr = spawn_ray_to_hit(si.hit, ls.p1);
                                    const size_t slot = p + (size_t)l * W.n_paths;
                                    W.sh[2 * slot] = make_float4(sr.o.x, sr.o.y, sr.o.z, 0.0f); W.sh[2 * slot + 1] = make_float4(sr.d.x, sr.d.y, sr.d.z, sr.t_max);
                                    const Rgb term = f * ls.radiance * abs_dot(ls.wi, si.shading_n) / ls.pdf;
                                    W.whT[slot] = make_float4(term.r, term.g, term.b, 0.0f);
                                    mask |= 1u << l;
                                }
                            }
                            if (mask) { ps |= PS_DIRECT; light_word = mask; sh_mask = mask; }
                        } else {
                            if (si.light >= 0) rad = rad + area_Le(S.lights[si.light], si.hit.n, si.wo);      /* radiance += intersect.emitted_radiance(wo) */
                            else rad = rad + Rgb(0.0f);
                            if (nl > 0) {                                     /* uniform_sample_one_light + first half of estimate_direct */
                                const uint32_t ln = (uint32_t)f2usize(fmin_(rng.next() * (float)nl, (float)(nl - 1)));
                                const V2 ul = rng.next2(), us = rng.next2();
                                const DLight& Lt = S.lights[ln];
                                const uint32_t flags = T_ALL & ~T_SPECULAR;
                                const bool delta = Lt.kind == LK_POINT || Lt.kind == LK_DISTANT;
                                ps |= PS_DIRECT; light_word = ln;
                                Rgb ld(0.0f); float mis_w = 0.0f, mis_pdf = 1.0f; Rgb mis_f(0.0f);
                                DLiSample ls = light_sample(S, Lt, si.hit, ul);
                                if (ls.pdf > 0.0f && !ls.radiance.is_black()) {
                                    Rgb f = bsdf_f(B, si.wo, ls.wi, flags) * abs_dot(ls.wi, si.shading_n);
                                    float sp = bsdf_pdf(B, si.wo, ls.wi, flags);
                                    if (!f.is_black()) {
                                        DRay sr = spawn_ray_to_hit(si.hit, ls.p1);
                                        W.sh[2 * (size_t)(p)] = make_float4(sr.o.x, sr.o.y, sr.o.z, 0.0f); W.sh[2 * (size_t)(p) + 1] = make_float4(sr.d.x, sr.d.y, sr.d.z, sr.t_max);
                                        ld = delta ? (f * ls.radiance / ls.pdf) : (f * ls.radiance * power_heuristic(ls.pdf, sp) / ls.pdf);
                                        ps |= PS_SHADOW; sh_mask = 1u;
                                    }
                                }
                                if (!delta) {
                                    DScatter sc;
                                    if (bsdf_sample(B, si.wo, us, flags, &sc)) {
                                        Rgb f = sc.f * abs_dot(sc.wi, si.shading_n);
                                        if (!f.is_black()) {
                                            bool go = true;
                                            if (sc.type & T_SPECULAR) mis_w = 1.0f;
                                            else { float lp = light_pdf(S, Lt, si.hit, sc.wi); if (lp == 0.0f) go = false; else mis_w = power_heuristic(sc.pdf, lp); }
                                            if (go) {
                                                DRay mr = spawn_ray(si.hit, sc.wi);
                                                W.ray[2 * (size_t)(p + W.n_paths)] = make_float4(mr.o.x, mr.o.y, mr.o.z, 0.0f);
                                                W.ray[2 * (size_t)(p + W.n_paths) + 1] = make_float4(mr.d.x, mr.d.y, mr.d.z, mr.t_max);
                                                mis_f = f; mis_pdf = sc.pdf;
                                                if (W.mis_any && Lt.kind == LK_INFINITE) { ps |= PS_MIS_ANY; push_mis_any = true; } else { ps |= PS_MIS; push_mis = true; }
                                            }
                                        }
                                    }
                                }
                                W.pend0[p] = make_float4(ld.r, ld.g, ld.b, mis_w);
                                W.pend1[p] = make_float4(mis_f.r, mis_f.g, mis_f.b, mis_pdf);
                            }
                        }
                        float4 lvA = make_float4(rad.r, rad.g, rad.b, 1.0f), lvB = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                        if (depth + 1u < P.max_depth) {
                            /* specular_reflect: the 2D sample is drawn before the match (mod.rs:52) */
                            const V2 ur = rng.next2();
                            DScatter sr;
                            const bool has_r = bsdf_sample(B, si.wo, ur, T_REFL | T_SPECULAR, &sr) && !(abs_dot(sr.wi, si.shading_n) == 0.0f);
                            const bool has_t = bsdf_num(B, T_TRANS | T_SPECULAR) > 0;
                            if (has_t) err = FTN_ERR_UNSUPPORTED;              /* specular transmission: glass.rs:66 todo!() */
                            else if (has_r) {
                                lvA.w = sr.pdf; lvB = make_float4(sr.f.r, sr.f.g, sr.f.b, fabsf(dot(sr.wi, si.shading_n)));
                                if (TEX) {                            /* the reflected ray's differentials, for the next level's lookups (mod.rs:58-84) */
                                    rd = specular_diff(true, rd, si.hit.p, si.wo, sr.wi, si.shading_n, ex.dndu, ex.dndv, td, bsdf_eta);
                                    W.dfd[p] = make_float4(rd.rxo.x, rd.rxo.y, rd.rxo.z, rd.rxd.x); W.dfd[(size_t)W.n_paths + p] = make_float4(rd.ryo.x, rd.ryo.y, rd.ryo.z, rd.rxd.y);
                                    W.dfd[2 * (size_t)W.n_paths + p] = make_float4(rd.ryd.x, rd.ryd.y, rd.ryd.z, rd.rxd.z);
                                }
                                DRay nr = spawn_ray(si.hit, sr.wi);
                                W.ray[2 * (size_t)(p)] = make_float4(nr.o.x, nr.o.y, nr.o.z, 0.0f); W.ray[2 * (size_t)(p) + 1] = make_float4(nr.d.x, nr.d.y, nr.d.z, nr.t_max);
                                alive = true; push_closest = true;
                            }
                        }
                        W.dlA[(size_t)depth * W.n_paths + p] = lvA; W.dlB[(size_t)depth * W.n_paths + p] = lvB;
                        depth += 1u;
                        W.rng01[p] = make_ulonglong2(rng.s0, rng.s1); W.rng23[p] = make_ulonglong2(rng.s2, rng.s3);
                        if (!alive && !(ps & PS_DIRECT)) { dl_unwind(P, W, p, depth, false, Rgb(0.0f)); ended = true; }      /* nothing pending: fold now */
                    }
                }
                if (err && !ended) ended = true;
                if (ended) { alive = false; ps &= ~(PS_DIRECT | PS_SHADOW | PS_MIS | PS_MIS_ANY); sh_mask = 0; push_closest = push_mis = push_mis_any = false; if (err) W.rad[p] = make_float4(0.0f, 0.0f, 0.0f, 0.0f); }
                ps = (ps & ~(PS_BOUNCE_MASK | PS_ALIVE)) | (depth & PS_BOUNCE_MASK) | (alive ? PS_ALIVE : 0u);
                W.beta[p] = make_float4(0.0f, 0.0f, 0.0f, __uint_as_float(ps));
                if (!ended) W.rad[p] = make_float4(0.0f, 0.0f, 0.0f, __uint_as_float(light_word));
                push_active = alive || (ps & PS_DIRECT);
                active_entry = p | (alive ? 0u : WF_Q_FIN);
            }
        }
        {
            const bool pred[5] = {push_active, push_closest, push_mis, push_mis_any, push_mis_any};
            const uint32_t val[5] = {active_entry, p, p | WF_MIS_BIT, p | WF_MIS_BIT, 0u};
            uint32_t* const qs[5] = {out_q, W.q_closest, W.q_closest, W.q_shadow, nullptr};
            uint32_t* const cs[5] = {out_count, &W.counters[CTR(WFC_CLOSEST)], &W.counters[CTR(WFC_CLOSEST)], &W.counters[CTR(WFC_SHADOW)], &W.counters[CTR(WFC_MIS_ANY)]};
            block_push<5>(pred, val, qs, cs);
        }
        /* shadow rays: slot p + l * n_paths (direct lighting: l = 0 only) -- queue entries are slots; the any-hit kernels read W.sh[2 * slot] */
        for (uint32_t l = 0; l < (WHITTED ? nl : 1u); l++) {
            const bool on = ((sh_mask >> l) & 1u) != 0;
            const bool pred[1] = {on};
            const uint32_t val[1] = {p + l * W.n_paths};
            uint32_t* const qs[1] = {W.q_shadow};
            uint32_t* const cs[1] = {&W.counters[CTR(WFC_SHADOW)]};
            if (__syncthreads_or(on ? 1 : 0)) block_push<1>(pred, val, qs, cs);
        }
    }
    if (err) atomicCAS(&P.stats->error, 0, err);
}

/* ------------------------------------------------------------------ ray batches: the records ftn_intersect* return (wavefront_trace_batch,
 * ftn_wf_trace.hip), out24 the full SurfaceInteraction of every hit */
__global__ void __launch_bounds__(256) k_batch_finish(DScene S, const float* __restrict__ rays8, uint32_t n, const float4* __restrict__ hit, const int* __restrict__ hit_prim,
                                                      float* t_hit, int* prim, float* bary, float* out24) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const float4 h4 = hit[i]; const int hp = hit_prim[i];
    if (t_hit) t_hit[i] = hp >= 0 ? h4.x : FTN_INF;
    if (prim) prim[i] = hp;
    if (bary) { bary[3 * (size_t)i] = hp >= 0 ? h4.y : 0.0f; bary[3 * (size_t)i + 1] = hp >= 0 ? h4.z : 0.0f; bary[3 * (size_t)i + 2] = hp >= 0 ? h4.w : 0.0f; }
    if (out24) {                                                        /* the full SurfaceInteraction of the hit (ftn_intersect_full) */
        float* o = out24 + 24 * (size_t)i;
        if (hp < 0) { for (int k = 0; k < 24; k++) o[k] = 0.0f; o[23] = -1.0f; }
        else {
            const float* r = rays8 + 8 * (size_t)i;
            DRay ray0; ray0.o = V3(r[0], r[1], r[2]); ray0.d = V3(r[3], r[4], r[5]); ray0.t_max = r[6]; ray0.time = r[7];
            DHit h; h.t = h4.x; h.b0 = h4.y; h.b1 = h4.z; h.b2 = h4.w; h.prim = hp;
            DSI si; make_interaction(S, h, ray0, &si);
            o[0] = si.hit.p.x; o[1] = si.hit.p.y; o[2] = si.hit.p.z; o[3] = si.hit.p_err.x; o[4] = si.hit.p_err.y; o[5] = si.hit.p_err.z;
            o[6] = si.hit.n.x; o[7] = si.hit.n.y; o[8] = si.hit.n.z; o[9] = 0.0f; o[10] = 0.0f;
            o[11] = si.wo.x; o[12] = si.wo.y; o[13] = si.wo.z; o[14] = si.s_dpdu.x; o[15] = si.s_dpdu.y; o[16] = si.s_dpdu.z;
            o[17] = 0.0f; o[18] = 0.0f; o[19] = 0.0f; o[20] = si.shading_n.x; o[21] = si.shading_n.y; o[22] = si.shading_n.z; o[23] = h.t;
        }
    }
}

/* ------------------------------------------------------------------ launchers (ftn_wf_internal.h) */
void launch_wf_classify(const RenderParams& P, const WfBuffers& W, int in_q, uint32_t drop, unsigned grid, hipStream_t stream) {
    hipLaunchKernelGGL(k_wf_classify, dim3(grid), dim3(256), 0, stream, P, W, in_q, drop);
}

namespace {
struct ShadeLaunch {
    const WavefrontState* st; const RenderParams& P; const WfBuffers& W; int in_q; uint32_t first; unsigned fixed_grid; bool tex, env; hipStream_t stream;
    /* One variant over the classes in `mask`.  Workgroups per CU: what the kernel's registers let a CU hold at once (x 2 for the light kernel
     * of the classes without a BSDF) -- every workgroup loops over an equal share of its class, so a grid of 8 per CU against 3 resident ran
     * its last third at 2/3 of the machine (shading 83.2 -> 81.9 ms; 4 per CU: 97 ms); FTN_SHADE_GRID / FTN_SHADE_GRID_NOBSDF set it by
     * hand.  The unspecialised kernel takes 8 per CU. */
    template <bool TEX, int MT, bool ENV> void variant(uint32_t mask) const {
        unsigned grid = fixed_grid;
        if (!grid) {
            unsigned per_cu = 8u;
            if constexpr (MT != -1) {
                const unsigned by_hand = knob(MT == -2 ? "FTN_SHADE_GRID_NOBSDF" : "FTN_SHADE_GRID", 0);
                per_cu = by_hand ? by_hand : (MT == -2 ? 2u : 1u) * shade_wgs_per_cu<TEX, MT, ENV>();
            }
            grid = std::min<unsigned>((unsigned)st->n_cu * per_cu, (W.n_paths + 255) / 256);
        }
        hipLaunchKernelGGL((k_wf_shade<TEX, MT, ENV>), dim3(grid), dim3(256), 0, stream, P, W, in_q, mask, first);
    }
    template <int MT> void classes(uint32_t mask) const {
        if (tex) { if (env) variant<true, MT, true>(mask); else variant<true, MT, false>(mask); }
        else { if (env) variant<false, MT, true>(mask); else variant<false, MT, false>(mask); }
    }
};
}  // namespace

void launch_wf_shade(WavefrontState* st, const RenderParams& P, const WfBuffers& W, int in_q, uint32_t first, unsigned fixed_grid, hipStream_t stream) {
    const bool specialise = knob("FTN_SHADE_SPECIALISE", 1) != 0;
    /* lit by one InfiniteAreaLight: the variants specialised for it (the indexed driver's single unspecialised launch is the general kernel,
     * the tile-serial driver's is not) */
    const bool env = P.S.env_only && knob("FTN_SHADE_ENV", 1) && (specialise || W.serial);
    const ShadeLaunch L{st, P, W, in_q, first, fixed_grid, P.S.n_textures != 0, env, stream};
    if (!specialise) { L.classes<-1>(0xffu); return; }
    /* one launch per material type present in the scene + one for the classes without a BSDF (late finish: behind the first pass only the
     * primitives without a material are left of these classes) */
    if (!W.late_finish || first) L.classes<-2>(0x83u);
    else if (P.S.null_prims) L.classes<-2>(0x80u);
    if (P.S.material_types & 1u) L.classes<0>(1u << 2);
    if (P.S.material_types & 2u) L.classes<1>(1u << 3);
    if (P.S.material_types & 4u) L.classes<2>(1u << 4);
    if (P.S.material_types & 8u) L.classes<3>(1u << 5);
    if (P.S.material_types & 16u) L.classes<4>(1u << 6);
}

void launch_wf_shade_dl(bool whitted, bool tex, const RenderParams& P, const WfBuffers& W, int in_q, unsigned grid, hipStream_t stream) {
    if (whitted) { if (tex) hipLaunchKernelGGL((k_wf_shade_dl<true, true>), dim3(grid), dim3(256), 0, stream, P, W, in_q); else hipLaunchKernelGGL((k_wf_shade_dl<true, false>), dim3(grid), dim3(256), 0, stream, P, W, in_q); }
    else { if (tex) hipLaunchKernelGGL((k_wf_shade_dl<false, true>), dim3(grid), dim3(256), 0, stream, P, W, in_q); else hipLaunchKernelGGL((k_wf_shade_dl<false, false>), dim3(grid), dim3(256), 0, stream, P, W, in_q); }
}

void launch_batch_finish(const DScene& S, const float* d_rays8, uint32_t n, const float4* hit, const int* hit_prim, float* t_hit, int* prim, float* bary, float* out24, hipStream_t stream) {
    hipLaunchKernelGGL(k_batch_finish, dim3((n + 255) / 256), dim3(256), 0, stream, S, d_rays8, n, hit, hit_prim, t_hit, prim, bary, out24);
}

}  // namespace ftn
