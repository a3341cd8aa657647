/*
 * ftn_lightpass.h -- the light-group pass (ftn_lightpass.hip; C ABI: include/fountain_hip_lightpass.h): its host interface, and the
 * arithmetic its kernels and the host entries (ftn_lightpass_terms, ftn_lightpass_resolve, ftn_lightpass_compose) share, compiled for
 * both sides.
 */
#ifndef FTN_LIGHTPASS_H
#define FTN_LIGHTPASS_H
#include "ftn_wavefront.h"

namespace ftn {

/* uniform_sample_one_light's choice among n lights for the draw u (integrator/mod.rs:296-299); n > 0 */
FTN_HD uint32_t lp_select(float u, uint32_t n) { return (uint32_t)f2usize(fmin_(u * (float)n, (float)(n - 1u))); }

/* The term of one surface {geometric normal ng, shading normal ns, wo} and one light sample {radiance, wi, pdf} out of a group of n
 * lights: e = (radiance * (abs_dot(wi, ns) / pdf)) * n behind the tests of the header.  Returns whether a shadow ray is traced (e is
 * not black); *e is zero otherwise */
FTN_HD bool lp_term(V3 ng, V3 ns, V3 wo, Rgb radiance, V3 wi, float pdf, uint32_t n, Rgb* e) {
    *e = Rgb(0.0f);
    if (!(pdf > 0.0f) || radiance.is_black()) return false;
    if (!(dot(wi, ng) * dot(wo, ng) > 0.0f)) return false;            /* Bsdf::f's reflection test on the geometric normal */
    const float c = abs_dot(wi, ns) / pdf;
    const Rgb v = (radiance * c) * (float)n;
    if (v.is_black()) return false;
    *e = v;
    return true;
}

/* spawn_ray_to_hit (ftn_device.h, interaction.rs:22-58) for both sides: from the surface {p, p_err, n} to the point {tp, tp_err, tn}, both
 * ends offset off their surfaces, the direction not normalised and t_max = 1 - 0.0001 */
struct LpRay { V3 o, d; float t_max; };
FTN_HD LpRay lp_shadow_ray(V3 p, V3 p_err, V3 n, V3 tp, V3 tp_err, V3 tn) {
    const V3 origin = offset_ray_origin(p, p_err, n, tp - p);
    const V3 target = offset_ray_origin(tp, tp_err, tn, origin - tp);
    LpRay r; r.o = origin; r.d = target - origin; r.t_max = 1.0f - 0.0001f;
    return r;
}

/* ftn_lightpass_resolve for one pixel: sums {lit 3, unshadowed 3, H, W} -> {lit / H, unshadowed / H, Y(lit) / Y(unshadowed), H / W} */
FTN_HD void lp_resolve_pixel(const float* in, float* out) {
    const float h = in[6], w = in[7];
    if (w == 0.0f) { for (int k = 0; k < 8; k++) out[k] = 0.0f; return; }
    if (h == 0.0f) { for (int k = 0; k < 6; k++) out[k] = 0.0f; out[6] = 1.0f; }
    else {
        for (int k = 0; k < 6; k++) out[k] = in[k] / h;
        const float yl = Rgb(in[0], in[1], in[2]).luminance(), yu = Rgb(in[3], in[4], in[5]).luminance();
        out[6] = yu == 0.0f ? 1.0f : yl / yu;
    }
    out[7] = h / w;
}

/* ftn_lightpass_compose for one pixel: gb = its 12 resolved G-buffer floats, res8 + 8 (g n + i) = its resolved light pass of group g */
#define LP_MAX_GROUPS 16
struct LpGains { float v[3 * LP_MAX_GROUPS]; };
FTN_HD void lp_compose_pixel(const float* gb, const float* res8, size_t i, size_t n, uint32_t groups, const LpGains& gains, float* rgb) {
    float acc[3] = {0.0f, 0.0f, 0.0f};
    if (gb[10] != 0.0f) {
        for (uint32_t g = 0; g < groups; g++) {
            const float* lit = res8 + 8 * ((size_t)g * n + i);
            for (int c = 0; c < 3; c++) acc[c] = acc[c] + ((gb[c] * FTN_INV_PI) * lit[c]) * gains.v[3 * g + c];
        }
    }
    rgb[0] = acc[0]; rgb[1] = acc[1]; rgb[2] = acc[2];
}

/* the light-group pass over the camera samples wavefront_render traces for the same parameters (indexed sampler): d_lights = the group's
 * n_lights indices into S.lights in device memory, or NULL for all n_lights = S.n_lights of them; d_out = 8 floats per crop pixel
 * (ftn_lightpass_pixel), added into; P.accA / B = zero float4 per crop pixel (left non-zero where P.stats->bc_writes says so);
 * count_mode: launch_trace's, for the shadow rays (0: the production any-hit kernels, 1: the reference-order walk); times: any_ms and
 * any_launches of the shadow rays, the other fields untouched */
int wavefront_lightpass(WavefrontState** state, const RenderParams& P, const std::vector<DTile>& tiles, const uint32_t* d_lights, uint32_t n_lights, int count_mode,
                        float* d_out, hipStream_t stream, double* trace_ms, WavefrontTimes* times);
hipError_t launch_lp_resolve(const float* in, size_t n, float* out8, hipStream_t stream);
hipError_t launch_lp_compose(const float* gb12, const float* res8, uint32_t groups, const LpGains& gains, size_t n, float* rgb, hipStream_t stream);
}  // namespace ftn
#endif
