/*
 * fountain_hip_lightpass.h -- extension of the C ABI (fountain_hip.h): light-group AOVs.  Per group of lights, the direct light that
 * arrives at the first visible surface (`unshadowed`) and the part of it the scene lets through (`lit`), over exactly the camera samples
 * ftn_render traces for the same sampler, tiles and film, filtered with the same box-filter footprint.  One call renders one group; a
 * compositor scales and sums the groups afterwards (ftn_lightpass_compose) instead of rendering again with an edited scene.
 *
 * The reference has no light AOVs, so these functions have no orc_* twin in the CPU oracle; FTN_ABI_VERSION is unchanged and the
 * extension carries a version of its own.
 *
 * Light set.  M is a strictly increasing list of indices into Scene::lights, in the order ftn_scene_get_lights reports (the explicit
 * lights, then the area lights in BVH primitive order); n = |M|.  lights == NULL with n_lights == 0 means all lights.
 *
 * Per camera sample (px, py, s) of ftn_render with the indexed sampler:
 *   surface   the first surface that HAS a material, exactly as ftn_render_gbuffer takes it: null-material primitives are passed through
 *             along the same direction (src/integrator/path.rs:77-80), at most 4096 times per sample (beyond that: FTN_ERR_INTERNAL).
 *   miss      a sample that misses (also after pass-throughs) adds to `weight` only.
 *   draws     from the sample's own indexed stream, indexed_key(seed, px, py, s): draws 0-4 are the camera sample, draw 5 selects the
 *             light, draws 6 and 7 are u_light; pass-throughs consume no draws.  This is the order of uniform_sample_one_light at the
 *             path's first vertex (integrator/mod.rs:289-329): with M = all lights the pass picks the light and the light sample the
 *             beauty picks there.
 *   light     k = f2usize(min(u5 * (float)n, (float)(n - 1)))  (`as usize`: saturating, NaN -> 0; integrator/mod.rs:296-299); the
 *             chosen light is M[k].  n == 0 (a scene without lights, all-lights form): e = 0 and no ray.
 *   sample    ls = Light::sample_incident_radiance(S.lights[M[k]], hit, u_light): radiance, wi, pdf and the point p1 on the light
 *   term      with the interaction's geometric normal ng, shading normal ns and wo (ftn_intersect_full slots 6-8, 20-22 and 11-13):
 *               e = 0 and no ray unless ls.pdf > 0 and ls.radiance is not black;
 *               e = 0 and no ray unless dot(ls.wi, ng) * dot(wo, ng) > 0  (the reflection test of Bsdf::f, reflection/mod.rs);
 *               otherwise c = abs_dot(ls.wi, ns) / ls.pdf (one divide) and e = (ls.radiance * c) * (float)n per channel, in exactly
 *               this association; if e is black, no ray is traced.
 *   ray       spawn_ray_to(hit, p1) (interaction.rs:22-58: both ends offset, t_max = 1 - 0.0001), and
 *             occluded = Scene::intersect_test(ray): every primitive occludes, null-material ones included.
 * The sample then adds into every pixel of its box-filter footprint, with w = 1:  unshadowed += w * e;  lit += w * e when a ray was traced
 * and it was not occluded;  hit_weight += w for a recorded surface;  weight += w for every sample, hit or not.
 *
 * What it estimates.  There is no BSDF and no MIS in the term: it is the light-sampling estimator of n times one light's irradiance on the
 * shading normal, that is, of the group's irradiance.  For a matte surface (Lambert, sigma = 0) albedo / pi * lit is therefore the beauty's
 * direct term from light sampling at the first vertex; the BSDF-sampled half of estimate_direct, specular lobes and indirect light are not
 * in it.
 *
 * Film accumulation is the G-buffer's (Film::add_sample_to_tile, src/film.rs:133-172): a pixel receives its own samples one at a time in
 * increasing sample index, added into the value already in the caller's buffer; samples whose footprint leaves their own pixel (counted
 * in ftn_stats.spill_samples) are summed apart and added after the call's last pass.
 */
#ifndef FOUNTAIN_HIP_LIGHTPASS_H
#define FOUNTAIN_HIP_LIGHTPASS_H

#include "fountain_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ftn_lightpass_pixel {    /* 32 bytes; sums over the samples that touched the pixel, w = box filter weight */
    float lit[3];                       /* sum of w * e over samples whose shadow ray was not occluded          */
    float unshadowed[3];                /* sum of w * e                                                          */
    float hit_weight;                   /* sum of w over samples that recorded a surface                         */
    float weight;                       /* sum of w over all samples (= ftn_pixel.filter_weight_sum)             */
} ftn_lightpass_pixel;

/* Arguments as ftn_render_gbuffer / ftn_render_gbuffer_device (same tile rules), and the light set.  Refusals, all made on the host before
 * any device work, in this order: (1) FTN_ERR_INVALID_ARGUMENT for a null scene, camera, film, sampler or pixel buffer; (2)
 * FTN_ERR_INVALID_ARGUMENT for lights == NULL with n_lights != 0 and for a non-null lights with n_lights == 0; (3)
 * FTN_ERR_INVALID_ARGUMENT for indices that are not strictly increasing or not below the scene's light count; (4) FTN_ERR_UNSUPPORTED
 * for FTN_SAMPLER_TILE_SERIAL and for FTN_PIPELINE_MEGAKERNEL (AUTO and WAVEFRONT are accepted); (5) FTN_ERR_NO_DEVICE without a GPU.
 * The caller's buffer is untouched by a refused call.  A scene without lights, called with the all-lights form, adds the two weights and
 * traces no occlusion ray.
 * Statistics: rays_closest (camera rays plus pass-through rays), rays_any (the shadow rays), camera_samples, spill_samples, kernel_ms,
 * trace_ms, any_ms, any_launches.  Triangle-only scenes trace the shadow rays over the quantised eight-box tree, scenes with spheres
 * over the four-box records, as the beauty's shadow rays; options->count_traffic = 1 sends them through the reference-order traversal
 * instead (same answers, slower; no tallies are reported).
 * lights: HOST array of n_lights indices.  out_pixels: HOST buffer of crop-width x crop-height pixels, added into. */
int ftn_render_lightpass(const ftn_scene* scene, const ftn_camera_desc* camera, const ftn_film_desc* film,
                         const ftn_sampler_desc* sampler, const ftn_tile_range* tiles, const ftn_render_options* options,
                         const uint32_t* lights, uint32_t n_lights, ftn_lightpass_pixel* out_pixels, ftn_stats* stats);
/* device_pixels: DEVICE buffer of ftn_lightpass_pixel, added into on `stream` (a hipStream_t; NULL = the default stream); lights stays a
 * HOST array: it is uploaded for the call and freed on every way out */
int ftn_render_lightpass_device(const ftn_scene* scene, const ftn_camera_desc* camera, const ftn_film_desc* film,
                                const ftn_sampler_desc* sampler, const ftn_tile_range* tiles, const ftn_render_options* options,
                                const uint32_t* lights, uint32_t n_lights, void* device_pixels, void* stream, ftn_stats* stats);

/* out8: 8 floats per pixel, with H = hit_weight and W = weight: lit / H (3), unshadowed / H (3), visibility, H / W.
 *   visibility  Y(lit) / Y(unshadowed) of the sums, Y(c) = (c.r * 0.212671f + c.g * 0.715160f) + c.b * 0.072169f; 1 where
 *               Y(unshadowed) == 0
 * H == 0: zero irradiance and visibility 1.  W == 0: eight zeros.  Each quotient is one f32 divide.
 * ftn_lightpass_resolve runs on the host; the _device variant reads and writes HBM on `stream` (FTN_ERR_NO_DEVICE without a GPU).  Both
 * refuse null buffers with n != 0 (FTN_ERR_INVALID_ARGUMENT); n == 0 does nothing. */
int ftn_lightpass_resolve(const ftn_lightpass_pixel* in, size_t n, float* out8);
int ftn_lightpass_resolve_device(const void* in, size_t n, void* out8, void* stream);

/* The relighting step, an image-space stage: from the resolved G-buffer (ftn_gbuffer_resolve: 12 floats per pixel; albedo in 0-2,
 * coverage in 10) and `groups` resolved light passes (res8: `groups` planes of n x 8 floats, plane g = ftn_lightpass_resolve of group g),
 *   rgb[c] = sum over g, in increasing g from +0, of ((albedo[c] * INV_PI) * res8[g].lit[c]) * gains3[3 g + c]
 * per channel, in exactly this association (INV_PI = 0.31830987f); rgb = 0 where the G-buffer's coverage is 0.  rgb_out: n x 3 floats.
 * gains3: HOST array of 3 floats per group, for both entries.
 * Refusals, in this order: FTN_ERR_INVALID_ARGUMENT for a null argument (with n != 0; a null gains3 always), for groups outside 1 .. 16,
 * for n * groups >= 2^31, for gains that are not finite, for an output that overlaps an input, and (device entry) for a buffer that is
 * not aligned to 16 bytes; the device entry then FTN_ERR_NO_DEVICE without a GPU.  ftn_lightpass_compose is the host twin of the kernel
 * and needs no device: both give the same bits. */
#define FTN_LIGHTPASS_MAX_GROUPS 16
int ftn_lightpass_compose(const float* gb12, const float* res8, uint32_t groups, const float* gains3, size_t n, float* rgb_out);
int ftn_lightpass_compose_device(const void* gb12, const void* res8, uint32_t groups, const float* gains3, size_t n, void* rgb_out, void* stream);

/* Host only, no device needed: the term and the shadow ray of the pass for n surfaces and light samples -- the same code the kernel
 * calls, compiled for the host.  hit24: interaction records in ftn_intersect_full's layout (p, p_err, n, wo and the shading normal are
 * read); light24: output rows of ftn_test_light for those reference points (radiance, wi, pdf and p1's p, p_err, n are read);
 * group_size: n of the definition above.  e3: the term e per row; rays8: the shadow ray {o.xyz, d.xyz, t_max, 0}, or eight zeros for a
 * row that traces no ray.  With the scene's ftn_intersect_full, ftn_test_light and ftn_intersect_test it replays the pass sample by
 * sample. */
int ftn_lightpass_terms(const float* hit24, const float* light24, size_t n, uint32_t group_size, float* e3, float* rays8);

#define FTN_LIGHTPASS_ABI_VERSION 1
int ftn_lightpass_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* FOUNTAIN_HIP_LIGHTPASS_H */
