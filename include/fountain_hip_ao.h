/*
 * fountain_hip_ao.h -- extension of the C ABI (fountain_hip.h): ambient occlusion and bent normals over exactly the camera samples
 * ftn_render traces for the same sampler, tiles and film, filtered with the same box-filter footprint (the pass is the `ao`
 * integrator of PBRT v3 on this library's samples and film).
 *
 * The reference has no ambient-occlusion integrator, so these functions have no orc_* twin in the CPU oracle; FTN_ABI_VERSION is
 * unchanged and the extension carries a version of its own.
 *
 * Per camera sample (px, py, s) of ftn_render:
 *   surface   the first surface that HAS a material, as ftn_render_gbuffer takes it: null-material primitives are passed through along
 *             the same direction (src/integrator/path.rs:77-80), at most 4096 times per sample (beyond that: FTN_ERR_INTERNAL).
 *   miss      a sample that misses (also after pass-throughs) adds to `weight` only.
 *   hit       with the interaction's p, p_err, geometric normal n and wo = -d of the ray that found it (ftn_intersect_full slots 0-8
 *             and 11-13): nf = faceforward(n, wo) (geometry/mod.rs:64-70), coordinate_system(nf, &s, &t) (geometry/mod.rs:45-62).
 *             For k = 0 .. rays - 1:
 *               u    = (draw 5 + 2k, draw 6 + 2k) of the sample's own indexed stream, indexed_key(seed, px, py, s); draws 0-4 are the
 *                      camera sample, pass-throughs consume no draws
 *               l    = cosine_sample_hemisphere(u)                                     (sampling.rs)
 *               d    = (s * l.x + t * l.y) + nf * l.z  per component, in exactly this association, not renormalised
 *               ray  = spawn_ray({p, p_err, n}, d) with t_max = radius                  (interaction.rs:22-58; +inf is allowed)
 *               occluded = Scene::intersect_test(ray): every primitive occludes, null-material ones included; l.z == 0 is no
 *                      special case
 *               if not occluded: count += 1 and bent += d, component-wise, in increasing k
 * The sample then adds into every pixel of its box-filter footprint, with w = 1:  open += w * count, bent[3] += w * bent,
 * hit_weight += w, and for every sample, hit or not, weight += w.
 *
 * Film accumulation is the G-buffer's (Film::add_sample_to_tile, src/film.rs:133-172): a pixel receives its own samples one at a
 * time in increasing sample index, added into the value already in the caller's buffer; samples whose footprint leaves their own
 * pixel (counted in ftn_stats.spill_samples) are summed apart and added after the call's own samples.
 *
 * `open`, `hit_weight` and `weight` are sums of small integers in float32: they are exact, and therefore independent of the order of
 * the sums, of the pass plan and of how a sample range is split over calls, while they stay below 2^24.  `bent` is a float sum and
 * carries the order above in its last bits.
 */
#ifndef FOUNTAIN_HIP_AO_H
#define FOUNTAIN_HIP_AO_H

#include "fountain_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ftn_ao_options {
    uint32_t rays;                      /* occlusion rays per recorded surface, 1 .. 64                           */
    float radius;                       /* t_max of every occlusion ray, > 0; +inf: unbounded (the usual choice)  */
    uint32_t _pad[2];
} ftn_ao_options;

typedef struct ftn_ao_pixel {           /* 32 bytes; sums over the samples that touched the pixel, w = box filter weight */
    float open;                         /* sum of w * (occlusion rays of the sample that were not occluded)      */
    float bent[3];                      /* sum of w * (sum of the directions of those rays)                      */
    float hit_weight;                   /* sum of w over samples that recorded a surface                         */
    float weight;                       /* sum of w over all samples (= ftn_pixel.filter_weight_sum)             */
    float _pad[2];
} ftn_ao_pixel;

/* Arguments as ftn_render_gbuffer / ftn_render_gbuffer_device (same tile rules).  Refusals, all made on the host before any device
 * work, in this order: FTN_ERR_INVALID_ARGUMENT for null arguments (ao included), for ao->rays outside 1 .. 64 and for an ao->radius
 * that is NaN or <= 0; FTN_ERR_UNSUPPORTED for FTN_SAMPLER_TILE_SERIAL and for FTN_PIPELINE_MEGAKERNEL (AUTO and WAVEFRONT are
 * accepted); FTN_ERR_NO_DEVICE without a GPU.  Statistics: rays_closest (camera rays plus pass-through rays), rays_any (the
 * occlusion rays: recorded surfaces x ao->rays), camera_samples, spill_samples, kernel_ms, trace_ms, any_ms, any_launches.
 * Triangle-only scenes trace the occlusion rays over the quantised eight-box tree, scenes with spheres over the four-box records, as
 * the beauty's shadow rays; options->count_traffic = 1 sends them through the reference-order traversal instead (same answers, slower;
 * no tallies are reported).
 * out_pixels: HOST buffer of crop-width x crop-height pixels, added into. */
int ftn_render_ao(const ftn_scene* scene, const ftn_camera_desc* camera, const ftn_film_desc* film,
                  const ftn_sampler_desc* sampler, const ftn_tile_range* tiles, const ftn_render_options* options,
                  const ftn_ao_options* ao, ftn_ao_pixel* out_pixels, ftn_stats* stats);
/* device_pixels: DEVICE buffer of ftn_ao_pixel, added into on `stream` (a hipStream_t; NULL = the default stream) */
int ftn_render_ao_device(const ftn_scene* scene, const ftn_camera_desc* camera, const ftn_film_desc* film,
                         const ftn_sampler_desc* sampler, const ftn_tile_range* tiles, const ftn_render_options* options,
                         const ftn_ao_options* ao, void* device_pixels, void* stream, ftn_stats* stats);

/* out: 6 floats per pixel: ao, bent normal (3), coverage, weight.
 *   ao        open / (rays * hit_weight): one f32 multiply, then one f32 divide
 *   bent      bent * (1 / sqrt((x*x + y*y) + z*z)) in f32 (cgmath's normalize), or 0 when that length is 0
 *   coverage  hit_weight / weight, one f32 divide
 * hit_weight == 0: ao = 1, bent normal 0.  weight == 0: six zeros.  FTN_ERR_INVALID_ARGUMENT for rays outside 1 .. 64.
 * The _device variant reads and writes HBM on `stream`. */
int ftn_ao_resolve(const ftn_ao_pixel* in, size_t n, uint32_t rays, float* out6);
int ftn_ao_resolve_device(const void* in, size_t n, uint32_t rays, void* out6, void* stream);

/* Host only, no device needed: for n interaction records in ftn_intersect_full's layout (24 floats; p, p_err, n and wo are read) and n
 * pairs u, the occlusion ray {o.xyz, d.xyz, t_max = radius, 0} the pass builds for that surface and those two draws -- the same code
 * the kernel calls, compiled for the host.  With the scene's ftn_intersect_full and ftn_intersect_test it replays the pass ray by
 * ray. */
int ftn_ao_rays(const float* hit24, const float* u2, size_t n, float radius, float* rays8);

#define FTN_AO_ABI_VERSION 1
int ftn_ao_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* FOUNTAIN_HIP_AO_H */
