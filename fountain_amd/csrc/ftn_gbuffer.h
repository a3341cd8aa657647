/*
 * ftn_gbuffer.h -- host interface of the first-hit G-buffer pass (ftn_gbuffer.hip; C ABI: include/fountain_hip_gbuffer.h).
 */
#ifndef FTN_GBUFFER_H
#define FTN_GBUFFER_H
#include "ftn_wavefront.h"

namespace ftn {
/* first-hit G-buffer over the camera samples wavefront_render traces for the same parameters (indexed sampler): d_out = 12 floats per crop
 * pixel (ftn_gbuffer_pixel), added into; P.accA / B / C = zero float4 per crop pixel (left non-zero where P.stats->bc_writes says so) */
int wavefront_gbuffer(WavefrontState** state, const RenderParams& P, const std::vector<DTile>& tiles, const float w2c[16], float* d_out, hipStream_t stream,
                      double* trace_ms);
/* ftn_gbuffer_resolve for one pixel: sums {albedo 3, normal 3, position 3, depth, H, W} -> {albedo / W, normal / W, position / H, depth / H, H / W, W} */
FTN_HD void gbuffer_resolve_pixel(const float* in, float* out) {
    const float w = in[11], h = in[10];
    if (w == 0.0f) { for (int k = 0; k < 12; k++) out[k] = 0.0f; return; }
    for (int k = 0; k < 6; k++) out[k] = in[k] / w;
    if (h == 0.0f) { out[6] = 0.0f; out[7] = 0.0f; out[8] = 0.0f; out[9] = FTN_INF; }
    else { for (int k = 6; k < 10; k++) out[k] = in[k] / h; }
    out[10] = h / w; out[11] = w;
}
hipError_t launch_gbuffer_resolve(const float* in, size_t n, float* out12, hipStream_t stream);
}  // namespace ftn
#endif
