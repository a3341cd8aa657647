/*
 * fountain_hip_adaptive.h -- extension of the C ABI (fountain_hip.h): per-tile adaptive sampling.  Every 16x16 film tile is rendered for
 * a few samples, the tiles whose pixels' estimated variance is already small enough stop, and the others get more samples, round by
 * round, up to samples_per_pixel.  The beauty and the second moments (include/fountain_hip_moments.h) of every tile are those of a
 * uniform render at that tile's final sample count.
 *
 * The reference has no adaptive sampling, so these functions have no orc_* twin in the CPU oracle; FTN_ABI_VERSION is unchanged and the
 * extension carries a version of its own.
 *
 * Schedule.  N = sampler.samples_per_pixel, n0 = min_samples.  Round 1 renders the samples [0, n0) of every tile of the tile range.
 * After each round every tile that is still active is tested (criterion below); a tile that passes drops out, the others render
 * [n_r, n_{r+1}) with n_{r+1} = min(N, n_r + (step_samples ? step_samples : n_r)).  The call ends when no tile is active or n_r = N.
 * Every tile's samples are drawn with samples_per_pixel = N (the camera ray differentials of textured scenes scale by 1/sqrt(N),
 * camera_ray_diff), so a tile that ends at n holds the bits of ftn_render_moments with samples_per_pixel = N and the sample range
 * [0, n), not those of a render with samples_per_pixel = n.
 *
 * Criterion.  For a pixel, take the ftn_pixel P and ftn_moment_pixel Q that the call would return into zero buffers if it ended now
 * (this call's own, in-tile and other-tile sums combined in k_film_resolve's order; no caller buffer content).  v = the Y component of
 * ftn_moments_resolve(P, Q) (so W = P.filter_weight_sum < 2 gives +inf); m = P.xyz[1] / W; t2 = t * t; a2 = a * a; the pixel has
 * converged iff v <= B = t2 * (m * m + a2).  Each step is one f32 rounding, in that order (no fused multiply-add).  NaN or inf in
 * what the criterion reads (P.xyz[1], W, Q.sq_y), in v or in B means not converged.  A tile has converged iff every pixel of the tile
 * inside the crop has; a tile with no pixel in the crop (an edge tile of the sample bounds when the filter radius is above 0.5)
 * converges after round 1.  The kernel and ftn_adaptive_converged share one code path and agree bit for bit.
 *
 * Limits.
 *   Bias: the decision to stop is made from estimates of the same samples that stay in the image, which biases the result slightly
 *   (tiles whose first samples happened to agree stop early).
 *   Spill pixels: a pixel reached by samples of another tile that ends at a different count is a mix of two counts, and its sums come
 *   from atomics, so at a threshold the decision can flip in the last bit from one call to the next.  This happens only where foreign
 *   samples land (ftn_stats.spill_samples; rare with the default box filter of radius 0.5: only samples on a pixel edge).
 */
#ifndef FOUNTAIN_HIP_ADAPTIVE_H
#define FOUNTAIN_HIP_ADAPTIVE_H

#include "fountain_hip.h"
#include "fountain_hip_moments.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ftn_adaptive_params {    /* 16 bytes                                                                                    */
    uint32_t min_samples;               /* n0, 2 <= n0 <= samples_per_pixel: every tile gets at least this many                       */
    uint32_t step_samples;              /* samples added per round; 0 = double: n_{r+1} = min(N, 2 n_r)                                */
    float    threshold;                 /* t >= 0, finite: target relative standard error of a pixel's mean luminance                 */
    float    abs_floor;                 /* a >= 0, finite: absolute floor added to the mean, so that dark pixels can converge         */
} ftn_adaptive_params;

typedef struct ftn_adaptive_info {      /* 24 bytes                                                                                    */
    uint32_t rounds;                    /* rounds run (1 ..; 0 when the tile range selects no tile)                                    */
    uint32_t tiles;                     /* tiles of the tile range                                                                     */
    uint32_t tiles_at_max;              /* tiles that ended at N                                                                       */
    uint32_t _pad;
    uint64_t pixel_samples;             /* sum over the tiles of final count * the tile's pixels inside the crop                      */
} ftn_adaptive_info;

/* n0 = 8, step = 0 (doubling), t = 0.05, a = 0.01 (DESIGN.md section 13 gives the measurements behind them) */
void ftn_adaptive_params_default(ftn_adaptive_params* params);

/* Arguments as ftn_render_moments (same tile rules, same pipelines and integrators), with the sampler's whole range: first_sample = 0
 * and sample_count 0 or samples_per_pixel.
 * Refusals, all before any device work, in this order: FTN_ERR_INVALID_ARGUMENT for null arguments (info and stats may be null), for
 * parameters outside the ranges above and for a partial sample range; FTN_ERR_UNSUPPORTED for FTN_SAMPLER_TILE_SERIAL, for
 * FTN_PIPELINE_MEGAKERNEL and for Whitted with more than 32 lights; then FTN_ERR_NO_DEVICE without a GPU.
 * out_pixels, out_moments: HOST buffers of crop-width x crop-height pixels, both added into (the sums of ftn_render_moments at each
 * tile's count).  out_samples: one uint32 per crop pixel, the final sample count of the pixel's tile; written for the pixels of the
 * tile range's tiles only and left untouched elsewhere, so that calls over disjoint tile ranges compose.  stats: the sum over all
 * rounds.  FTN_ERR_NAN_RADIANCE stops the schedule after the round that raised it; the buffers are still written and that code is
 * returned. */
int ftn_render_adaptive(const ftn_scene* scene, const ftn_camera_desc* camera, const ftn_film_desc* film,
                        const ftn_sampler_desc* sampler, const ftn_integrator_desc* integrator, const ftn_tile_range* tiles,
                        const ftn_render_options* options, const ftn_adaptive_params* params,
                        ftn_pixel* out_pixels, ftn_moment_pixel* out_moments, uint32_t* out_samples, ftn_adaptive_info* info, ftn_stats* stats);
/* device_pixels (ftn_pixel), device_moments (ftn_moment_pixel), device_samples (uint32): DEVICE buffers of crop pixels, the first two
 * added into, the last written as out_samples above, on `stream` (a hipStream_t; NULL = the default stream).  The call reads one byte
 * per active tile back to the host after every round and waits for it, so it cannot be captured in a graph. */
int ftn_render_adaptive_device(const ftn_scene* scene, const ftn_camera_desc* camera, const ftn_film_desc* film,
                               const ftn_sampler_desc* sampler, const ftn_integrator_desc* integrator, const ftn_tile_range* tiles,
                               const ftn_render_options* options, const ftn_adaptive_params* params,
                               void* device_pixels, void* device_moments, void* device_samples, void* stream, ftn_adaptive_info* info, ftn_stats* stats);

/* The criterion on the host (the twin of the device's decision): out[i] = 1 if pixel i (beauty P[i], moments Q[i]) has converged
 * under params, else 0.  Parameters are checked as above (min_samples is not used). */
int ftn_adaptive_converged(const ftn_pixel* beauty, const ftn_moment_pixel* moments, size_t n, const ftn_adaptive_params* params, uint8_t* out);

#define FTN_ADAPTIVE_ABI_VERSION 1
int ftn_adaptive_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* FOUNTAIN_HIP_ADAPTIVE_H */
