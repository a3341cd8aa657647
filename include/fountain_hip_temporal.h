/*
 * fountain_hip_temporal.h -- extension of the C ABI (fountain_hip.h): temporal reprojection and accumulation for a sequence of frames of
 * one static scene under a moving camera (the temporal part of SVGF, Schied et al., HPG 2017).  It stands beside ftn_denoise_guided
 * (include/fountain_hip_denoise_guided.h) and in front of it: each frame's resolved beauty image (ftn_film_resolve), resolved first-hit
 * G-buffer (ftn_gbuffer_resolve, include/fountain_hip_gbuffer.h) and variance of each pixel's mean (ftn_moments_resolve,
 * include/fountain_hip_moments.h) are blended with the history of the frames before it, fetched where the pixel's surface was seen by the
 * previous camera.  The accumulated image and its variance go into ftn_denoise_guided unchanged, which widens or narrows by itself because
 * it reads that variance.
 *
 * The reference renders single frames, so these functions have no orc_* twin in the CPU oracle; FTN_ABI_VERSION and the other extension
 * versions are unchanged and the extension carries a version of its own.
 *
 * Inputs, row-major, w x h pixels (the film's crop): rgb = 3 floats per pixel; gb12 = the 12 resolved G-buffer floats per pixel: albedo a,
 * normal n, position x, depth z, coverage c = H / W, weight W; var4 = 4 floats per pixel, the variance of the pixel's mean in r, g, b and
 * Y.  The previous frame: its camera, its gb12 (n', x', c' below) and the history the call for it wrote.  History is one
 * ftn_temporal_pixel per pixel: u, the accumulated colour (demodulated when FTN_DENOISE_DEMODULATE is set); n, the history length in
 * frames (a real number: it is interpolated like the rest); nu, the accumulated variance of u in r, g, b and that of Y.  The caller owns
 * two history buffers and swaps them between frames.  prev_camera, prev_gb12 and prev_history are all null for the first frame.
 *
 * All arithmetic is binary32, one rounding per operation in the order written.  For pixel p = (x, y) of the crop:
 *
 *   1. prepare   u_cur as ftn_denoise's step 1: u_cur = rgb_p / d per channel, d = max(a_p, albedo_eps) when FTN_DENOISE_DEMODULATE is
 *                set and c_p > 0, else u_cur = rgb_p and d = 1.  nu_cur,c = var_c / (d_c d_c) for r, g, b (d d rounded, then the
 *                quotient; var_c itself when d = 1) and nu_cur,Y = var_Y: Y's variance is carried without demodulation.  When u_cur is
 *                not finite, or one of the four nu_cur is NaN or negative (which a NaN or negative var4 gives), the pixel passes through:
 *                out_rgb = rgb, out_var4 = var4, and its history is written as eight zeros: n = 0, so no later frame reads it.
 *   2. motion    project(camera, v, point) maps a world-space point or direction to raster coordinates: q = m4_point(camera_to_world.inv,
 *                v) for a point and m4_vector(camera_to_world.inv, v) for a direction, r = m4_point(raster_to_camera.inv, q); q.z is the
 *                camera-space depth.  m4_point and m4_vector are the library's (the reference's Transform applied to a point and a
 *                vector).  A covered pixel (c_p > 0) projects its G-buffer position x_p as a point.  An uncovered pixel projects its
 *                direction: D = m4_vector(cur.camera_to_world.m, m4_point(cur.raster_to_camera.m, (x + crop.x0 + 0.5, y + crop.y0 + 0.5,
 *                0))).  motion = r_prev - r_cur (x and y), both from the same function: equal cameras give a motion of exactly zero,
 *                although x_p is the mean over jittered samples and not the point under the pixel's centre.  q.z must be > 0 in the
 *                previous camera, else there is no history.  The lens radius is ignored: this is pinhole reprojection, and with depth of
 *                field the history of a defocused pixel is fetched where its in-focus surface point would be.
 *   3. taps      s = (x + motion.x, y + motion.y), ix = floor(s.x), tx = s.x - ix, likewise iy, ty.  A non-finite s, or one outside
 *                (-1, w) x (-1, h), means no history.  The four taps q = (ix + i, iy + j), j outer and i inner, carry the weights
 *                b = (i ? tx : 1 - tx) (j ? ty : 1 - ty).  A tap with b == 0 is skipped and never read.  A tap counts when it is inside
 *                the image; n_q > 0; (c'_q > 0) == (c_p > 0); its history is usable: u_q finite and no nu_q NaN, after the conversion
 *                below; and, for a covered p, |n_p - n'_q|^2 <= normal_tol and |n_p . (x_p - x'_q)| <= plane_tol max(z_p, 1e-6) -- Dn
 *                and Dp of ftn_denoise as thresholds, |.|^2 = (e0 e0 + e1 e1) + e2 e2 and the dot product summed the same way.
 *                Equal cameras (the four matrices of cur_camera and prev_camera agree element for element) make neither of these two
 *                tests: the only tap is the pixel itself, which sees the static scene as it did, while its n_p and x_p, means over a
 *                few jittered samples, jump between the surfaces a silhouette pixel covers and would refuse it its own history.
 *                Conversion, when p is demodulated, per channel c of r, g, b, with d'_q = max(a'_q, albedo_eps) from prev_gb12: when
 *                |d_p - d'_q| > albedo_tol max(d_p, d'_q) the tap is carried over by the radiance it stands for,
 *                  u_q <- (u_q d'_q) / d_p,   nu_q <- (nu_q (d'_q d'_q)) / (d_p d_p)
 *                and otherwise, equal divisors among them, it is read as it is.  u_q was divided by d'_q and u' is multiplied by
 *                d_p, and a pixel's albedo is the mean over its samples: a pixel on the edge of an emitter (albedo 0, radiance large)
 *                or between two materials changes its divisor from frame to frame by orders of magnitude even under a camera that
 *                stands still, and geometry cannot tell.  Within albedo_tol the demodulated colour is kept, which is what keeps a
 *                texture sharp under resampling; beyond it the tap blends as it would without demodulation.
 *                W = sum b, and u_prev, nu_prev
 *                and n_prev are (sum b v) / W, every sum starting at +0 and adding one term at a time.  When W is not > 0 there is no
 *                history.  The variance is interpolated linearly on purpose: reprojected neighbours are correlated, the weighted mean
 *                of variances bounds the variance of the weighted mean from above, and sum b^2 nu would understate it.
 *   4. blend     n' = n_prev + 1, alpha = max(1 / n', alpha_min), k = 1 - alpha:
 *                  u' = k u_prev + alpha u_cur,   nu' = (k k) nu_prev + (alpha alpha) nu_cur   (exact for independent frames)
 *                No history, or alpha >= 1: n' = 1, u' = u_cur, nu' = nu_cur, copied and not computed, so 0 inf never arises.
 *                var4 = +inf (fewer than 2 samples) stays +inf.
 *   5. write     out_history = {u', n', nu'}; out_rgb = u' d when FTN_DENOISE_DEMODULATE is set and c_p > 0, else u' (ftn_denoise's
 *                step 3); out_var4 = nu'_c (d_c d_c) for r, g, b (nu'_c itself when d = 1) and nu'_Y.
 *
 * The device path and ftn_temporal_accumulate_cpu share the per-pixel code and agree bit for bit.
 *
 * Exact properties.  First frame without demodulation: out_rgb = rgb and out_var4 = var4 bit for bit, n = 1.  Equal cameras: motion is
 * exactly zero, every pixel whose coverage class stays reads its own history with weight 1 whatever the tolerances, and K frames follow
 * the recurrence of step 4 bit for bit; with alpha_min = 0, n = K.  A tap of the other coverage class, or under cameras that differ a tap
 * of another surface by the two thresholds, never contributes.
 *
 * Refusals (FTN_ERR_INVALID_ARGUMENT, with ftn_last_error()): null pointers, apart from an all-null previous frame (any other mix of null
 * and non-null among prev_camera, prev_gb12 and prev_history is refused); w or h <= 0, or w h >= 2^31; a film whose crop is not w x h;
 * a tolerance (normal, plane, albedo) that is negative or not finite; alpha_min outside [0, 1]; an albedo_eps that is negative or not finite; flag bits other
 * than FTN_DENOISE_DEMODULATE; a non-zero reserved field; on the device path, an output overlapping an input or another output, a
 * history buffer not aligned to 16 bytes or an image not aligned to 4.
 */
#ifndef FOUNTAIN_HIP_TEMPORAL_H
#define FOUNTAIN_HIP_TEMPORAL_H

#include "fountain_hip_denoise.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ftn_temporal_pixel {     /* 32 bytes: two float4 */
    float u[3];                         /* accumulated colour (demodulated with FTN_DENOISE_DEMODULATE)         */
    float n;                            /* history length in frames; 0 = none                                   */
    float nu[4];                        /* accumulated variance of u in r, g, b, and that of Y                  */
} ftn_temporal_pixel;

typedef struct ftn_temporal_params {    /* 32 bytes */
    uint32_t flags;                     /* FTN_DENOISE_DEMODULATE only (default FTN_DENOISE_DEMODULATE)         */
    float alpha_min;                    /* floor of the blend weight of the current frame, 0..1 (default 0.4)   */
    float normal_tol;                   /* largest |n_p - n'_q|^2 of a counted tap (default 0.01)               */
    float plane_tol;                    /* largest plane distance of a counted tap, relative to depth (default 1e-3) */
    float albedo_eps;                   /* floor of the demodulation divisor (default 1e-3)                     */
    float albedo_tol;                   /* largest relative difference of divisors read as equal (default 0.01)  */
    uint32_t reserved[2];               /* must be 0                                                            */
} ftn_temporal_params;

void ftn_temporal_params_default(ftn_temporal_params* params);

/* HOST buffers in and out: uploads, accumulates on the GPU `device` (-1 = the current device) and downloads.  FTN_ERR_NO_DEVICE without a
 * GPU.  prev_camera, prev_gb12 and prev_history are all null for the first frame. */
int ftn_temporal_accumulate(const float* rgb, const float* gb12, const float* var4, const ftn_camera_desc* cur_camera, const ftn_film_desc* film,
                            int32_t w, int32_t h, const ftn_camera_desc* prev_camera, const float* prev_gb12, const ftn_temporal_pixel* prev_history,
                            const ftn_temporal_params* params, ftn_temporal_pixel* out_history, float* out_rgb, float* out_var4, int32_t device);

/* DEVICE buffers on `stream` (a hipStream_t; NULL = the default stream); the cameras, the film and the parameters are host structures, read
 * before the call returns.  Allocates nothing and does not synchronise, so it can be captured in a graph.  The outputs must not overlap
 * the inputs or each other. */
int ftn_temporal_accumulate_device(const void* rgb, const void* gb12, const void* var4, const ftn_camera_desc* cur_camera, const ftn_film_desc* film,
                                   int32_t w, int32_t h, const ftn_camera_desc* prev_camera, const void* prev_gb12, const void* prev_history,
                                   const ftn_temporal_params* params, void* out_history, void* out_rgb, void* out_var4, void* stream);

/* The host twin, bit-identical to the device path (it runs the same per-pixel code on the host's threads; the result does not depend on
 * their number).  It exists for tests and tools: rendering still has no CPU fallback. */
int ftn_temporal_accumulate_cpu(const float* rgb, const float* gb12, const float* var4, const ftn_camera_desc* cur_camera, const ftn_film_desc* film,
                                int32_t w, int32_t h, const ftn_camera_desc* prev_camera, const float* prev_gb12, const ftn_temporal_pixel* prev_history,
                                const ftn_temporal_params* params, ftn_temporal_pixel* out_history, float* out_rgb, float* out_var4);

#define FTN_TEMPORAL_ABI_VERSION 1
int ftn_temporal_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* FOUNTAIN_HIP_TEMPORAL_H */
