/*
 * ftn_adaptive.h -- host interface and shared criterion of per-tile adaptive sampling (ftn_adaptive.hip; C ABI:
 * include/fountain_hip_adaptive.h).
 */
#ifndef FTN_ADAPTIVE_H
#define FTN_ADAPTIVE_H
#include "ftn_moments.h"

namespace ftn {
/* the header's criterion for one pixel: beauty {xyz, W} and moments {sq r, g, b, sq_y} as the call would return them now; t, a the
 * threshold and absolute floor.  Each step one f32 rounding (the library is built with -ffp-contract=off). */
FTN_HD bool adaptive_pixel_converged(const float* pix, const float* m, float t, float a) {
    float var[4];
    moments_resolve_pixel(pix, m, var);
    const float v = var[3];
    const float mean = pix[1] / pix[3];
    const float t2 = t * t, a2 = a * a;
    const float bound = t2 * (mean * mean + a2);
    return __builtin_isfinite(pix[1]) && __builtin_isfinite(pix[3]) && __builtin_isfinite(m[3]) && __builtin_isfinite(v) && __builtin_isfinite(bound) &&
           v <= bound;
}

/* k_film_resolve's and k_mo_merge's arithmetic for one pixel, into a zero pixel: A/B/C the beauty's accumulators, own/in/other the
 * moments'; `spilled` is DevStats::bc_writes != 0 (B, C, in and other are read only then, as those kernels do) */
FTN_HD void adaptive_pixel_sums(float4 a, float4 b, float4 c, float4 mo, float4 mi, float4 mt, bool spilled, float* pix, float* m) {
    const float4 zero = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (!spilled) { b = zero; c = zero; mi = zero; mt = zero; }
    float xyz[3];
    rgb_to_xyz(Rgb(a.x + b.x, a.y + b.y, a.z + b.z), xyz);
    pix[0] = 0.0f + xyz[0]; pix[1] = 0.0f + xyz[1]; pix[2] = 0.0f + xyz[2]; pix[3] = 0.0f + (a.w + b.w);
    if (c.w != 0.0f) {
        rgb_to_xyz(Rgb(c.x, c.y, c.z), xyz);
        pix[0] += xyz[0]; pix[1] += xyz[1]; pix[2] += xyz[2]; pix[3] += c.w;
    }
    m[0] = 0.0f + (mo.x + mi.x); m[1] = 0.0f + (mo.y + mi.y); m[2] = 0.0f + (mo.z + mi.z); m[3] = 0.0f + (mo.w + mi.w);
    if (spilled) { m[0] += mt.x; m[1] += mt.y; m[2] += mt.z; m[3] += mt.w; }
}

/* one workgroup per active tile (tiles[0 .. n)): flags[k] = 1 iff every pixel of tile k inside the crop has converged */
void launch_adaptive_decide(const RenderParams& P, const MomentAcc& M, const DTile* tiles, uint32_t n, float t, float a, uint8_t* flags, hipStream_t stream);
/* one workgroup per tile: out[pixel] = counts[k] for every pixel of tile k inside the crop */
void launch_adaptive_counts(const RenderParams& P, const DTile* tiles, const uint32_t* counts, uint32_t n, uint32_t* out, hipStream_t stream);
}  // namespace ftn
#endif
