/*
 * ftn_motion.h -- host interface of the previous-position pass (ftn_motion.hip; C ABI: include/fountain_hip_motion.h), the per-pixel code
 * of its resolve and of the motion vectors, shared by the kernels and the host twins so that both give the same bits.  The motion-aware temporal
 * accumulation is ftn_temporal.h's code, reached through its entry points' shared bodies (tp_accumulate_*).
 */
#ifndef FTN_MOTION_H
#define FTN_MOTION_H
#include "ftn_wavefront.h"
#include "ftn_temporal.h"

#pragma GCC visibility push(hidden)
namespace ftn {

/* top bit of a remap entry: a sphere whose transforms are bit-equal in the two scenes -- p' and ns' are copies of p and ns */
#define MV_REMAP_COPY 0x80000000u

/* previous-position pass over the camera samples wavefront_gbuffer records for the same parameters: d_out = 8 floats per crop pixel
 * (ftn_motion_pixel), added into; P.accA / B = zero float4 per crop pixel (left non-zero where P.stats->bc_writes says so).  prev: the
 * previous scene's arrays; remap: per primitive of the current scene in BVH order, the previous scene's BVH index of the same primitive
 * (every entry validated by the caller against prev.n_prims and the primitive's kind), MV_REMAP_COPY or-ed in */
int wavefront_motion(WavefrontState** state, const RenderParams& P, const std::vector<DTile>& tiles, const DScene& prev, const uint32_t* remap,
                     float* d_out, hipStream_t stream, double* trace_ms);

/* ftn_motion_resolve for one pixel: sums {position 3, normal 3, H, W} -> {position / H, normal / W, H / W, W} */
FTN_HD void motion_resolve_pixel(const float* in, float* out) {
    const float h = in[6], w = in[7];
    if (w == 0.0f) { for (int k = 0; k < 8; k++) out[k] = 0.0f; return; }
    if (h == 0.0f) { out[0] = 0.0f; out[1] = 0.0f; out[2] = 0.0f; }
    else { for (int k = 0; k < 3; k++) out[k] = in[k] / h; }
    for (int k = 3; k < 6; k++) out[k] = in[k] / w;
    out[6] = h / w; out[7] = w;
}
hipError_t launch_motion_resolve(const float* in, size_t n, float* mv8, hipStream_t stream);

/* what the motion vectors need beside the buffers */
struct MvFrame { TpCamera cur, prev; int w, h, x0, y0; };

/* ftn_motion_vectors for crop pixel (x, y): r_prev - r_cur of tp_motion (ftn_temporal.h), NaN where the previous camera does not see the
 * point (q.z <= 0) or mv8 and gb12 disagree about the pixel's coverage class */
FTN_HD void motion_vector_pixel(const float* mv8, const float* gb12, const MvFrame& F, int x, int y, float* out2) {
    const size_t p = (size_t)y * (size_t)F.w + (size_t)x;
    const float* mv = mv8 + 8 * p;
    const float* gb = gb12 + 12 * p;
    const bool cov_p = gb[10] > 0.0f;
    V3 rc, rp;
    tp_motion(F.cur, F.prev, cov_p, V3(gb[6], gb[7], gb[8]), V3(mv[0], mv[1], mv[2]), x, y, F.x0, F.y0, &rc, &rp);
    const bool seen = rp.z > 0.0f && (mv[6] > 0.0f) == cov_p;
    const float nan = ftn_det::u2f(0x7fc00000u);
    out2[2 * p] = seen ? rp.x - rc.x : nan;
    out2[2 * p + 1] = seen ? rp.y - rc.y : nan;
}
hipError_t launch_motion_vectors(const float* mv8, const float* gb12, const MvFrame& frame, float* out2, hipStream_t stream);

}  // namespace ftn
#pragma GCC visibility pop
#endif
