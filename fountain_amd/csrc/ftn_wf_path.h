/*
 * ftn_wf_path.h -- the path integrator's terminal arithmetic, shared by k_wf_shade (ftn_wf_shade.hip) and k_wf_accumulate (ftn_wavefront.hip).
 */
#ifndef FTN_WF_PATH_H
#define FTN_WF_PATH_H
#include "ftn_wf_common.h"

namespace ftn {

/* ---- finishing a path: the terminal arithmetic of a shading event, values in and radiance out (no struct of floats goes through a
 * reference: DESIGN section 5, round 3 item 2).  k_wf_shade runs the two steps around its own work; wf_finish_path is the two in a row for
 * a path that nothing else happens to, which k_wf_accumulate runs under late finish (WfBuffers::late_finish): one source for every float
 * operation, and the order per path stays L + direct, then L + beta * Le. */
/* the pending estimate_direct of the previous bounce (integrator/mod.rs:330-392): q0 = {Ld_light, mis weight}, q1 = {f, pdf}, q2 = {beta_prev};
 * shadow_lit: a shadow ray was traced and found nothing; inc: what arrives along the MIS ray (black: no such ray, occluded, or no light there) */
__device__ inline Rgb wf_add_direct(Rgb L, bool shadow_lit, float4 q0, float4 q1, float4 q2, Rgb inc, uint32_t n_lights) {
    Rgb radiance(0.0f);
    if (shadow_lit) radiance = radiance + Rgb(q0.x, q0.y, q0.z);
    if (!inc.is_black()) radiance = radiance + Rgb(q1.x, q1.y, q1.z) * inc * q0.w / q1.w;
    Rgb direct = Rgb(q2.x, q2.y, q2.z) * ((float)n_lights * radiance);
    return L + direct;
}
/* what a camera ray or a specular bounce sees where it ends (path.rs:45-58): e = emitted radiance of the surface hit / of the environment */
__device__ inline Rgb wf_add_seen(Rgb L, Rgb beta, Rgb e) { return L + beta * e; }
template <bool ENV> __device__ inline Rgb wf_escaped_Le(const DScene& S, V3 d) { return ENV ? Rgb(0.0f) + light_Le_env(S.env0, d) : scene_env_Le(S, d); }
/* A path of an environment-only scene whose MIS rays went through the any-hit kernels (PS_MIS_ANY, results in q3.w: store_occluded), from its
 * br record {beta, ps} {L, -} and pd record q0..q3 once every ray of it has been traced.  Still PS_ALIVE: its last ray escaped (hit = false,
 * d = the ray's direction) or it reached max_depth (k_wf_classify's class 1), and nothing but what that ray sees is left to add. */
__device__ inline Rgb wf_finish_path(const DScene& S, Rgb beta, Rgb L, uint32_t ps, float4 q0, float4 q1, float4 q2, float4 q3, bool hit, V3 d) {
    if (ps & PS_DIRECT) {
        const uint32_t occ_word = __float_as_uint(q3.w);
        Rgb inc(0.0f);
        if ((ps & PS_MIS_ANY) && !((occ_word & 0xff00u) != 0u)) inc = light_Le_env(S.env0, V3(q3.x, q3.y, q3.z));
        L = wf_add_direct(L, (ps & PS_SHADOW) && !((occ_word & 0xffu) != 0u), q0, q1, q2, inc, S.n_lights);
    }
    if ((ps & PS_ALIVE) && ((ps & PS_BOUNCE_MASK) == 0u || (ps & PS_SPECULAR) != 0u)) L = wf_add_seen(L, beta, hit ? Rgb(0.0f) : wf_escaped_Le<true>(S, d));
    return L;
}

}  // namespace ftn
#endif
