/*
 * fountain_hip_moments.h -- extension of the C ABI (fountain_hip.h): per-pixel second moments of the camera samples' radiance, rendered
 * beside the beauty in the same call, and the variance of each pixel's mean estimated from them.  Variance-guided denoising and
 * adaptive sampling read this buffer.
 *
 * The reference has no such output, so these functions have no orc_* twin in the CPU oracle; FTN_ABI_VERSION is unchanged and the
 * extension carries a version of its own.
 *
 * Beauty.  out_pixels receives the bits ftn_render writes for the same arguments, and the call returns the same statistics and the same
 * code, FTN_ERR_NAN_RADIANCE included (the pixels and moments are still written then).
 *
 * Sum order of the moments.  L is a camera sample's radiance as the film tile adds it (raw RGB), Y = the y of rgb_to_xyz(L) (ftn_math.h,
 * the conversion k_film_resolve applies).  Each sample adds fl(v * v) for each of its 4 values v = L.r, L.g, L.b, Y into every pixel of
 * its box-filter footprint (filter weight 1; the footprint rule of Film::add_sample_to_tile, the beauty's).  Per call, a pixel's own
 * samples are summed from +0 in increasing sample index; samples of other pixels are added by atomics into an in-tile and an other-tile
 * sum, as the beauty's are.  At the end out += (own + in-tile), then out += other-tile (k_film_resolve's order).  ftn_render_moments adds
 * the call's sum (from a zero buffer) once into the caller's host buffer, as ftn_render adds its film; ftn_render_moments_device adds in
 * that order straight into the caller's device buffer.  Only pixels reached by a sample of another pixel (never with the default box
 * filter of radius 0.5; counted in ftn_stats.spill_samples) may differ in the last bit from a serial sum in sample order.
 */
#ifndef FOUNTAIN_HIP_MOMENTS_H
#define FOUNTAIN_HIP_MOMENTS_H

#include "fountain_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ftn_moment_pixel {       /* 16 bytes; sums over the samples that touched the pixel (box filter: weight 1)                  */
    float sq[3];                        /* sum of L.r^2, L.g^2, L.b^2 (raw RGB radiance, as the film tile adds it)                        */
    float sq_y;                         /* sum of Y^2, Y = the y of rgb_to_xyz(L) (ftn_math.h, the conversion k_film_resolve applies)     */
} ftn_moment_pixel;

/* Arguments as ftn_render / ftn_render_device (same tile rules), on the wavefront pipeline (FTN_PIPELINE_AUTO means it) for the path,
 * direct-lighting and Whitted integrators.  Refusals, all before any device work: FTN_ERR_INVALID_ARGUMENT for null arguments;
 * FTN_ERR_UNSUPPORTED for FTN_SAMPLER_TILE_SERIAL, for FTN_PIPELINE_MEGAKERNEL and where the wavefront pipeline refuses the integrator
 * (Whitted with more than 32 lights); then FTN_ERR_NO_DEVICE without a GPU.
 * out_pixels, out_moments: HOST buffers of crop-width x crop-height pixels, both added into. */
int ftn_render_moments(const ftn_scene* scene, const ftn_camera_desc* camera, const ftn_film_desc* film,
                       const ftn_sampler_desc* sampler, const ftn_integrator_desc* integrator, const ftn_tile_range* tiles,
                       const ftn_render_options* options, ftn_pixel* out_pixels, ftn_moment_pixel* out_moments, ftn_stats* stats);
/* device_pixels (ftn_pixel), device_moments (ftn_moment_pixel): DEVICE buffers, added into on `stream` (a hipStream_t; NULL = the
 * default stream) */
int ftn_render_moments_device(const ftn_scene* scene, const ftn_camera_desc* camera, const ftn_film_desc* film,
                              const ftn_sampler_desc* sampler, const ftn_integrator_desc* integrator, const ftn_tile_range* tiles,
                              const ftn_render_options* options, void* device_pixels, void* device_moments, void* stream, ftn_stats* stats);

/* out4: 4 floats per pixel, r, g, b, Y: the unbiased estimate of the variance of the pixel's mean.  W = beauty.filter_weight_sum; the
 * sums S are xyz_to_rgb(beauty.xyz) for r, g, b (before any division) and beauty.xyz[1] for Y.  W < 2 -> +inf; otherwise, each step one
 * f32 rounding in this order: mean = S / W; v = sq / W - mean * mean; v = v < 0 ? 0 : v; out = v / (W - 1).  NaN propagates.  The host
 * and the _device variant share one code path and agree bit for bit.
 * Precision: the one-pass formula cancels.  When the variance is small against mean^2 (bright, nearly constant pixels at high sample
 * counts) sq / W and mean^2 agree in most of their bits, and a relative error e of the sums costs about 2 e mean^2 in v: a true variance
 * below that can come out as 0 (clamped) or as that size of noise.  e grows with the sample count (W float32 additions: up to about
 * W 2^-24); for r, g, b it also holds the round trip through the beauty's xyz (xyz_to_rgb's coefficients invert rgb_to_xyz's only to
 * about 1e-6 of the three channels' sum).  At 64 samples a Y variance of 2^-21 mean^2, and an r, g or b variance above 2^-17 mean^2 in a
 * channel small against the other two, can already come out as 0. */
int ftn_moments_resolve(const ftn_pixel* beauty, const ftn_moment_pixel* moments, size_t n, float* out4);
int ftn_moments_resolve_device(const void* beauty, const void* moments, size_t n, void* out4, void* stream);

#define FTN_MOMENTS_ABI_VERSION 1
int ftn_moments_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* FOUNTAIN_HIP_MOMENTS_H */
