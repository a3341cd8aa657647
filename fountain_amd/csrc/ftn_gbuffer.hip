/*
 * ftn_gbuffer.hip -- the first-hit G-buffer pass (include/fountain_hip_gbuffer.h) on the wavefront pipeline.
 *
 * A unit of its own: k_gb_shade is here and shares ftn_wf_common.h with the beauty's kernels; the passes and their pass-through rounds are
 * wf_first_hit_passes' (ftn_wf_internal.h, ftn_wavefront.hip), which wavefront_gbuffer hands the launches of k_gb_shade and of the
 * shared film's accumulate kernel (ftn_firsthit.h) for GbFilm.
 */
#include "ftn_firsthit.h"
#include "ftn_texture.h"
#include "ftn_gbuffer.h"
#include <cstring>

namespace ftn {

/* ================================================================== first-hit G-buffer (include/fountain_hip_gbuffer.h)
 * The camera samples of ftn_render for the same sampler, tiles and film: k_wf_generate makes the camera rays from the sample keys, the
 * production closest-hit kernels trace them, and k_gb_shade records the first surface that has a material.  A null-material hit spawns
 * the ray on along the same direction (path.rs:77-80) into the other queue and the round repeats (wf_first_hit_passes).
 * k_fh_accumulate<GbFilm> then adds the pass's samples of every pixel in sample order, as k_wf_accumulate adds the beauty's. */
struct GbParams {
    FhFilm film;          /* 12 floats per crop pixel (ftn_gbuffer_pixel); 3 float4 per path: {albedo, hit ? 1 : 0} {shading normal, camera-space z} {p, 0} */
    float w2c[16];        /* camera_to_world.inv: camera-space z of a hit (transform.rs:224) */
};
struct GbFilm {           /* sums: albedo, shading normal, p, camera-space z, hit weight, weight */
    static constexpr int OUT = 12, SUMS = 12;
    static constexpr uint32_t REC = 3, CHUNK = 4;
    __device__ static float4 load(const FhFilm& G, const WfBuffers&, size_t p, uint32_t j) { return G.rec[3 * p + j]; }
    __device__ static bool unpack(const float4* r, float* v, uint32_t* adds) {
        v[0] = r[0].x; v[1] = r[0].y; v[2] = r[0].z; v[3] = r[1].x; v[4] = r[1].y; v[5] = r[1].z; v[6] = r[2].x; v[7] = r[2].y; v[8] = r[2].z; v[9] = r[1].w;
        *adds = ~0u;
        return r[0].w != 0.0f;
    }
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
        DRay ray0; DHit h; DSI si;
        const FhHit found = fh_first_hit(S, W, p, &ray0, &h, &si);
        push = found == FH_THROUGH;
        float4 r0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), r1 = r0, r2 = r0;       /* a miss */
        if (found == FH_SURFACE) {
            ftn_material m = S.materials[si.mat];
            if (TEX && material_is_textured(S, si.mat)) {
                /* the camera ray's differentials, as the beauty's first shading pass rebuilds them (k_wf_shade): the path integrator hands
                 * them on unchanged through null-material pass-throughs */
                const FhSample cs = fh_sample(P, W, p);
                Rng crng; crng.seed(indexed_key(P.seed, cs.px, cs.py, cs.sample));
                const V2 j = crng.next2(); const V2 p_film((float)cs.px + j.x, (float)cs.py + j.y); const V2 p_lens = crng.next2(); const float time_u = crng.next();
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
        if (!push) { float4* R = G.film.rec + 3 * (size_t)p; R[0] = r0; R[1] = r1; R[2] = r2; }
    }
    const bool pred[1] = {push};
    const uint32_t val[1] = {p};
    uint32_t* const qs[1] = {q_out};
    uint32_t* const cs[1] = {count_out};
    block_push<1>(pred, val, qs, cs);
}

struct GbResolve {
    const float* in; float* out12;
    __device__ void operator()(size_t i) const { gbuffer_resolve_pixel(in + 12 * i, out12 + 12 * i); }
};
hipError_t launch_gbuffer_resolve(const float* in, size_t n, float* out12, hipStream_t stream) { return fh_per_pixel(n, stream, GbResolve{in, out12}); }

int wavefront_gbuffer(WavefrontState** state, const RenderParams& P, const std::vector<DTile>& tiles, const float w2c[16], float* d_out, hipStream_t stream,
                      double* trace_ms_out) {
    GbParams G;
    G.film = fh_film(P, d_out); memcpy(G.w2c, w2c, sizeof(G.w2c));
    const bool tex = P.S.n_textures != 0;
    WfFirstHitPass pass;
    pass.what = "the G-buffer";
    pass.setup = [&](WavefrontState* st, uint32_t) { G.film.rec = st->pd; return FTN_OK; };
    pass.shade = [&](const WfBuffers& W, const uint32_t* q_in, const uint32_t* count_in, uint32_t* q_out, uint32_t* count_out, dim3 grid, hipStream_t sm) {
        if (tex) hipLaunchKernelGGL(k_gb_shade<true>, grid, dim3(256), 0, sm, P, W, G, q_in, count_in, q_out, count_out);
        else hipLaunchKernelGGL(k_gb_shade<false>, grid, dim3(256), 0, sm, P, W, G, q_in, count_in, q_out, count_out);
    };
    pass.accumulate = [&](const WfBuffers& W, dim3 grid, hipStream_t sm) { hipLaunchKernelGGL(k_fh_accumulate<GbFilm>, grid, dim3(256), 0, sm, P, W, G.film); };
    return fh_merge<GbFilm>(wf_first_hit_passes(state, P, tiles, pass, stream, trace_ms_out), P, G.film, stream);
}

}  // namespace ftn
