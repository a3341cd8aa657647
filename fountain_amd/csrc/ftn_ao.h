/*
 * ftn_ao.h -- the ambient-occlusion pass (ftn_ao.hip; C ABI: include/fountain_hip_ao.h): its host interface, and the arithmetic its
 * kernels and the host entries (ftn_ao_rays, ftn_ao_resolve) share, compiled for both sides.
 */
#ifndef FTN_AO_H
#define FTN_AO_H
#include "ftn_wavefront.h"

namespace ftn {

/* nf = faceforward(n, wo) (ftn_math.h), the geometric normal on wo's side that the hemisphere of the occlusion rays stands on, in two
 * halves: the kernels keep faceforward's condition as one bit of a path's record instead of wo */
FTN_HD bool ao_flipped(V3 n, V3 wo) { return dot(n, wo) < 0.0f; }
FTN_HD V3 ao_facing_normal(V3 n, bool flipped) { return flipped ? -n : n; }

/* The occlusion ray of a surface {p, p_err, n} for the draws u: a cosine-distributed direction about nf, in the
 * frame coordinate_system makes of nf, d = (s l.x + t l.y) + nf l.z per component and not renormalised; origin as spawn_ray offsets it
 * (interaction.rs:22-58, with the surface's own n) */
struct AoRay { V3 o, d; };
FTN_HD AoRay ao_ray(V3 p, V3 p_err, V3 n, V3 nf, V2 u) {
    V3 s, t; coordinate_system(nf, &s, &t);
    const V3 l = cosine_sample_hemisphere(u);
    AoRay r;
    r.d = V3((s.x * l.x + t.x * l.y) + nf.x * l.z, (s.y * l.x + t.y * l.y) + nf.y * l.z, (s.z * l.x + t.z * l.y) + nf.z * l.z);
    r.o = offset_ray_origin(p, p_err, n, r.d);
    return r;
}

/* ftn_ao_resolve for one pixel: sums {open, bent 3, H, W, -, -} -> {open / (rays H), normalize(bent), H / W, W} */
FTN_HD void ao_resolve_pixel(const float* in, uint32_t rays, float* out) {
    const float h = in[4], w = in[5];
    if (w == 0.0f) { for (int k = 0; k < 6; k++) out[k] = 0.0f; return; }
    if (h == 0.0f) { out[0] = 1.0f; out[1] = 0.0f; out[2] = 0.0f; out[3] = 0.0f; }
    else {
        const float den = (float)rays * h;
        out[0] = in[0] / den;
        const V3 b(in[1], in[2], in[3]);
        const float l = len(b);
        const V3 nb = l == 0.0f ? V3(0.0f, 0.0f, 0.0f) : normalize(b);
        out[1] = nb.x; out[2] = nb.y; out[3] = nb.z;
    }
    out[4] = h / w; out[5] = w;
}

/* ambient occlusion over the camera samples wavefront_render traces for the same parameters (indexed sampler): d_out = 8 floats per crop
 * pixel (ftn_ao_pixel), added into; P.accA / B = zero float4 per crop pixel (left non-zero where P.stats->bc_writes says so);
 * count_mode: launch_trace's, for the occlusion rays (0: the production any-hit kernels, 1: the reference-order walk); times: any_ms and
 * any_launches of the occlusion rays, the other fields untouched */
int wavefront_ao(WavefrontState** state, const RenderParams& P, const std::vector<DTile>& tiles, uint32_t rays, float radius, int count_mode, float* d_out,
                 hipStream_t stream, double* trace_ms, WavefrontTimes* times);
hipError_t launch_ao_resolve(const float* in, size_t n, uint32_t rays, float* out6, hipStream_t stream);
}  // namespace ftn
#endif
