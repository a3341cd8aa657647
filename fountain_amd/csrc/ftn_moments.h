/*
 * ftn_moments.h -- host interface of the per-pixel second moments (ftn_moments.hip; C ABI: include/fountain_hip_moments.h).
 */
#ifndef FTN_MOMENTS_H
#define FTN_MOMENTS_H
#include "ftn_wavefront.h"

namespace ftn {
/* the moments' own three accumulators, float4 {r^2, g^2, b^2, Y^2} per crop pixel: a pixel's own samples (zero at the start of a call),
 * other pixels' samples from the same tile and from other tiles (zero unless the last call's DevStats::bc_writes said otherwise) */
struct MomentAcc { float4 *own, *in_tile, *other_tile; };
/* ftn_render's wavefront passes with the moments of every pass's samples beside them: P as ftn_render_device sets it up (P.accA/B/C
 * zeroed by the caller), the samples [P.first_sample, P.last_sample) in wavefront_render's passes.  Then
 * launch_film_resolve (beauty) and launch_moments_merge (moments) finish the call. */
int wavefront_moments(WavefrontState** state, const RenderParams& P, const std::vector<DTile>& tiles, bool count, bool count_production,
                      const MomentAcc& M, hipStream_t stream, WavefrontTimes* times);
/* out (ftn_moment_pixel per crop pixel) += own + in-tile, then += other-tile (k_film_resolve's order; reads P.stats->bc_writes) */
void launch_moments_merge(const RenderParams& P, const MomentAcc& M, float4* out, hipStream_t stream);

/* ftn_moments_resolve for one pixel: beauty {xyz, W} and moments {sq r, g, b, sq_y} -> variance of the mean {r, g, b, Y} */
FTN_HD void moments_resolve_pixel(const float* pix, const float* m, float* out) {
    const float w = pix[3];
    if (w < 2.0f) { for (int k = 0; k < 4; k++) out[k] = FTN_INF; return; }
    float s[4];
    xyz_to_rgb(pix, s);
    s[3] = pix[1];
    for (int k = 0; k < 4; k++) {
        const float mean = s[k] / w;
        float v = m[k] / w - mean * mean;
        v = v < 0.0f ? 0.0f : v;
        out[k] = v / (w - 1.0f);
    }
}
void launch_moments_resolve(const float* pix, const float* m, size_t n, float* out4, hipStream_t stream);
}  // namespace ftn
#endif
