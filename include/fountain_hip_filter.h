/*
 * fountain_hip_filter.h -- extension of the C ABI (fountain_hip.h): films with a reconstruction filter (box, triangle, Gaussian,
 * Mitchell-Netravali, Lanczos-windowed sinc; the definitions of PBRT v3, the book the reference follows), rendered by a
 * deterministic gather beside ftn_render's passes.
 *
 * The reference's Film<F: Filter> is generic, but BoxFilter is its only filter and the scene file's PixelFilter statement is ignored
 * (film.rs:61-71, filter/mod.rs:15-18, loaders/pbrt.rs:528-529).  ftn_render reproduces exactly that and is unchanged; these functions
 * have no orc_* twin in the CPU oracle, FTN_ABI_VERSION is unchanged and the extension carries a version of its own.
 *
 * Samples.  The camera samples of a filtered call are those of ftn_render for the same sampler, tiles and film: the same p_film and
 * the same radiance L.  film->filter_radius must equal the filter's radius bit for bit (it decides the sample bounds and therefore the
 * tiles); anything else is FTN_ERR_INVALID_ARGUMENT.
 *
 * Footprint.  A sample at p_film, pd = p_film - 0.5, covers the pixels x in [ceil(pd.x - rx), floor(pd.x + rx)] and likewise in y
 * (Film::add_sample_to_tile, film.rs:137-139; every step one binary32 operation), clipped to the crop window ONLY.  The reference clips
 * to the sample tile's pixel bounds as well, and get_film_tile computes their upper y with "- radius" (film.rs:100): at radius 2 that
 * takes a tile's own last rows out of its bounds.  The slip is not reproduced here.  It has no effect at the box filter's radius 0.5,
 * where the two rules agree, so a box of radius 0.5 through this entry equals ftn_render wherever no sample left its own pixel.
 *
 * Weight.  w = table[iy][ix] with ix = min((int)floorf(fabsf((x - pd.x) * inv_rx * 16.0f)), 15), inv_rx = 1.0f / rx, in binary32 in
 * that operation order, iy likewise (film.rs:146-157).  The term of a covered pixel is c = (L * 1.0f) * w per channel, and it is added
 * whatever the value of w, zero and negative included.
 *
 * Order.  Per call and per crop pixel q the sum starts from +0.  The sample index s ascends over the call's range as the OUTER loop;
 * within one s the source pixels whose sample covers q are taken row-major, y then x (only pixels of selected tiles have samples).
 * acc.rgb += c; acc.w += w.  At the end of the call out.xyz += rgb_to_xyz(acc.rgb); out.filter_weight_sum += acc.w for every crop
 * pixel.  The order does not depend on how the samples are cut into passes, so the result is a pure function of the sample set: equal
 * from run to run, from pass plan to pass plan, and between the device and ftn_filter_accumulate_samples on the host.  There are no
 * atomics anywhere.  ftn_film_resolve(_device) divides by the weight sum and clamps at 0 as for any film, which matters for Mitchell
 * and sinc, whose lobes are negative.
 *
 * Statistics.  Ray and node counts, camera_samples and the times are the call's.  spill_samples is that of a box of radius 0.5 (the
 * beauty's own accumulate kernel runs behind every pass with that radius and its film is discarded) and means nothing for the filtered
 * film.
 */
#ifndef FOUNTAIN_HIP_FILTER_H
#define FOUNTAIN_HIP_FILTER_H

#include "fountain_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { FTN_FILTER_BOX = 0, FTN_FILTER_TRIANGLE = 1, FTN_FILTER_GAUSSIAN = 2, FTN_FILTER_MITCHELL = 3, FTN_FILTER_SINC = 4 };
#define FTN_FILTER_TABLE_WIDTH 16
#define FTN_FILTER_MAX_RADIUS 8.0f

typedef struct ftn_filter_desc {        /* 32 bytes                                                                                       */
    uint32_t kind;                      /* FTN_FILTER_*                                                                                   */
    float radius[2];                    /* x, y; finite, above 0, at most FTN_FILTER_MAX_RADIUS                                           */
    float param[2];                     /* Gaussian: alpha, -; Mitchell: B, C; sinc: tau, -; unused ones are ignored (finite)             */
    uint32_t reserved[3];               /* 0                                                                                              */
} ftn_filter_desc;

/* The defaults of a kind: box radius 0.5; triangle radius 2; Gaussian radius 2, alpha 2; Mitchell radius 2, B = C = 1/3; sinc radius 4,
 * tau 3.  FTN_ERR_INVALID_ARGUMENT for an unknown kind or a null pointer. */
int ftn_filter_init(uint32_t kind, ftn_filter_desc* out);

/* Film::new's table (film.rs:61-71): table[y * 16 + x] = evaluate((x + 0.5) * rx / 16, (y + 0.5) * ry / 16), each entry evaluated in
 * binary64 and rounded once to binary32 (host work; nothing on the device calls exp or sin).  evaluate(x, y):
 *   box        1
 *   triangle   max(0, rx - |x|) * max(0, ry - |y|)
 *   Gaussian   g(x, rx) * g(y, ry), g(v, r) = max(0, exp(-alpha v^2) - exp(-alpha r^2))
 *   Mitchell   m(x / rx) * m(y / ry); with t = |2 v|: t > 1: ((-B - 6C) t^3 + (6B + 30C) t^2 + (-12B - 48C) t + (8B + 24C)) / 6,
 *              else ((12 - 9B - 6C) t^3 + (-18 + 12B + 6C) t^2 + (6 - 2B)) / 6
 *   sinc       l(x, rx) * l(y, ry), l(v, r) = 0 for |v| > r, else sinc(v) * sinc(v / tau); sinc(v) = 1 for |v| < 1e-5, else
 *              sin(pi v) / (pi v)
 * Refused with FTN_ERR_INVALID_ARGUMENT, in this order: null pointers; an unknown kind; a radius that is not finite, not above 0 or
 * above FTN_FILTER_MAX_RADIUS; parameters that are not finite; a sinc with tau <= 0. */
int ftn_filter_table(const ftn_filter_desc* filter, float table[256]);

/* Arguments as ftn_render / ftn_render_device plus the filter, on the wavefront pipeline (FTN_PIPELINE_AUTO means it).  Refusals, all
 * before any device work and in this order: FTN_ERR_INVALID_ARGUMENT for null arguments; ftn_filter_table's refusals; a
 * film->filter_radius that differs from filter->radius; then those of ftn_render_moments (FTN_ERR_UNSUPPORTED for
 * FTN_SAMPLER_TILE_SERIAL, FTN_ERR_INVALID_ARGUMENT for a sample range outside [0, samples_per_pixel] or an unknown integrator,
 * FTN_ERR_UNSUPPORTED for FTN_PIPELINE_MEGAKERNEL and for Whitted with more than 32 lights); FTN_ERR_UNSUPPORTED for a film whose
 * coordinates are so large (beyond about 2^23) that binary32 rounding lets a sample reach more than 16 pixels from its own; then
 * FTN_ERR_NO_DEVICE without a GPU.
 * NaN radiance returns FTN_ERR_NAN_RADIANCE with the film written, as ftn_render does.
 * out_pixels: a HOST buffer of crop-width x crop-height pixels, added into (the call's film from a zero buffer, added once). */
int ftn_render_filtered(const ftn_scene* scene, const ftn_camera_desc* camera, const ftn_film_desc* film, const ftn_filter_desc* filter,
                        const ftn_sampler_desc* sampler, const ftn_integrator_desc* integrator, const ftn_tile_range* tiles,
                        const ftn_render_options* options, ftn_pixel* out_pixels, ftn_stats* stats);
/* device_pixels (ftn_pixel): a DEVICE buffer, added into on `stream` (a hipStream_t; NULL = the default stream) */
int ftn_render_filtered_device(const ftn_scene* scene, const ftn_camera_desc* camera, const ftn_film_desc* film, const ftn_filter_desc* filter,
                               const ftn_sampler_desc* sampler, const ftn_integrator_desc* integrator, const ftn_tile_range* tiles,
                               const ftn_render_options* options, void* device_pixels, void* stream, ftn_stats* stats);

/* The host twin of the filtered film: the rules above applied to a list of n camera samples given in any order -- source pixel
 * (px[i], py[i]), sample index sample[i], film position p_film[2 i .. 2 i + 1], radiance L[3 i .. 3 i + 2].  It orders them itself by
 * (sample, py, px); a duplicate key is FTN_ERR_INVALID_ARGUMENT, as are the refusals of ftn_filter_table and a film radius that differs
 * from the filter's.  out_pixels (crop-width x crop-height, HOST) is added into as ftn_render_filtered adds.  Runs on the host's
 * threads over output pixels; the result does not depend on their number.  Shares the per-term code with the device kernel. */
int ftn_filter_accumulate_samples(const ftn_film_desc* film, const ftn_filter_desc* filter, size_t n, const int32_t* px, const int32_t* py,
                                  const uint32_t* sample, const float* p_film, const float* L, ftn_pixel* out_pixels);

/* The PixelFilter statement of a parsed scene file ("box", "triangle", "gaussian", "mitchell", "sinc" with "float xwidth", "ywidth",
 * "alpha", "B", "C", "tau"; missing parameters take ftn_filter_init's defaults).  Returns 1 and fills *out when the file has one, 0
 * when it has none, FTN_ERR_INVALID_ARGUMENT for a filter name outside that list.  ftn_render of a parsed file still ignores the
 * statement, as the reference does, and ftn_pbrt_film's filter_radius stays 0.5. */
int ftn_pbrt_filter(const ftn_pbrt* p, ftn_filter_desc* out);

#define FTN_FILTER_ABI_VERSION 1
int ftn_filter_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* FOUNTAIN_HIP_FILTER_H */
