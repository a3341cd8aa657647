/*
 * fountain_hip_motion.h -- extension of the C ABI (fountain_hip.h): where the surface point each camera sample sees was in the previous
 * frame's scene, the screen-space motion it gives, and temporal accumulation (fountain_hip_temporal.h) that follows it.  With it the
 * temporal stage serves animation: objects that move through their transforms and meshes that deform, not only a moving camera.
 *
 * The reference renders single frames, so these functions have no orc_* twin in the CPU oracle; FTN_ABI_VERSION and the other extension
 * versions are unchanged and the extension carries a version of its own.
 *
 * CORRESPONDING SCENES.  Two scenes correspond when they have the same primitive count, every primitive in the order of the scene
 * description (insertion order) has the same kind, and every sphere's radius, z_min, z_max, phi_max and reverse_orientation are bit-equal:
 * a sphere moves through its transforms only, a triangle through its vertices.  The two scenes' BVHs differ; the pass maps a hit of the
 * current scene through both scenes' primitive orders (ftn_scene_get_nodes) to the same primitive of the previous scene.
 *
 * THE PASS.  Per camera sample (px, py, s) of ftn_render the surface is the one ftn_render_gbuffer records: the first surface that has
 * a material, null-material primitives passed through, at most 4096 times.  For a recorded hit on primitive `prim` with barycentrics
 * (b1, b2), prim' the corresponding primitive of prev_scene:
 *   triangle  p' and ns' are what the library's interaction code gives for prim' at the same barycentrics: slots 0-2 and 20-22 of
 *             ftn_intersect_full, the same expressions in the same association as for a real hit (neither depends on the ray).  A previous
 *             scene equal to the current one therefore gives p' == p and ns' == ns bit for bit.
 *   sphere    with the library's binary32 m4_point and normal transform (transform_normal with the transform's inverse):
 *               p_obj = point(world_to_object_cur, p)        p'  = point(object_to_world_prev, p_obj)
 *               n_obj = normal(world_to_object_cur, ns)      ns' = normalize(normal(object_to_world_prev, n_obj))
 *             The inverse of world_to_object the normal transform reads is object_to_world.m of the same sphere, which is what a scene keeps
 *             (Transform::inverse swaps the two matrices, so they are the same bits in every scene the library builds).  When
 *             object_to_world (m and inv) and world_to_object.m are bit-equal in the two scenes, p' and ns' are copies of p and ns.
 * The sample then adds into every pixel of its box-filter footprint, with w = 1: prev_position += w p', prev_normal += w ns',
 * hit_weight += w, and for every sample, hit or not, weight += w.  Film accumulation is the G-buffer's: a pixel's own samples one at a
 * time in increasing sample index into the value already in the caller's buffer, the samples whose footprint leaves their own pixel
 * (ftn_stats.spill_samples) summed apart and added after them.  hit_weight and weight equal ftn_gbuffer_pixel's for the same arguments
 * bit for bit.
 */
#ifndef FOUNTAIN_HIP_MOTION_H
#define FOUNTAIN_HIP_MOTION_H

#include "fountain_hip_temporal.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ftn_motion_pixel {       /* 32 bytes; sums over the samples that touched the pixel, w = box filter weight */
    float prev_position[3];             /* sum of w * p' over samples that recorded a surface                    */
    float prev_normal[3];               /* sum of w * ns' over the same samples                                  */
    float hit_weight;                   /* sum of w over samples that recorded a surface                         */
    float weight;                       /* sum of w over all samples (= ftn_pixel.filter_weight_sum)             */
} ftn_motion_pixel;

/* Arguments as ftn_render_gbuffer / ftn_render_gbuffer_device (same tile rules, sample ranges and statistics) plus prev_scene.
 * Refusals, all on the host before anything is launched, in this order: FTN_ERR_INVALID_ARGUMENT for null arguments; for scenes on
 * different devices, and for scenes that do not correspond, FTN_ERR_INVALID_ARGUMENT with a ftn_last_error() that names the first
 * offending primitive in insertion order; FTN_ERR_UNSUPPORTED for FTN_SAMPLER_TILE_SERIAL and for FTN_PIPELINE_MEGAKERNEL;
 * FTN_ERR_NO_DEVICE without a GPU.  (A scene exists only where a device does, so without one the handles are not looked behind and the
 * second refusal cannot arise.)  The kinds and sphere parameters of scenes with spheres are read back from the scenes' device arrays
 * with copies, without a launch; triangle-only scenes of equal count correspond by construction.
 * out_pixels: HOST buffer of crop-width x crop-height pixels, added into. */
int ftn_render_motion(const ftn_scene* scene, const ftn_scene* prev_scene, const ftn_camera_desc* camera, const ftn_film_desc* film,
                      const ftn_sampler_desc* sampler, const ftn_tile_range* tiles, const ftn_render_options* options,
                      ftn_motion_pixel* out_pixels, ftn_stats* stats);
/* device_pixels: DEVICE buffer of ftn_motion_pixel, added into on `stream` (a hipStream_t; NULL = the default stream) */
int ftn_render_motion_device(const ftn_scene* scene, const ftn_scene* prev_scene, const ftn_camera_desc* camera, const ftn_film_desc* film,
                             const ftn_sampler_desc* sampler, const ftn_tile_range* tiles, const ftn_render_options* options,
                             void* device_pixels, void* stream, ftn_stats* stats);

/* mv8, 8 floats per pixel: prev_position / H, prev_normal / W, H / W, W (H = hit_weight, W = weight), one f32 divide each -- the
 * G-buffer's convention for position, normal, coverage and weight.  W == 0: eight zeros.  H == 0: position 0.
 * The _device variant reads and writes HBM on `stream`. */
int ftn_motion_resolve(const ftn_motion_pixel* in, size_t n, float* mv8);
int ftn_motion_resolve_device(const void* in, size_t n, void* mv8, void* stream);

/* Screen-space motion, 2 floats per pixel of the w x h crop: r_prev - r_cur in raster pixels (x, y), project being step 2's function of
 * fountain_hip_temporal.h (the code is shared with it).  A covered pixel (gb12's coverage > 0): r_prev = project(prev_camera, x^prev_p)
 * with x^prev_p mv8's position, r_cur = project(cur_camera, x_p) with x_p gb12's position, both as points.  An uncovered pixel projects
 * its direction D into both cameras as step 2 does.  q.z <= 0 in the previous camera, or an mv8 whose coverage class differs from
 * gb12's, gives NaN in both components.  Refusals: null arguments, w or h <= 0 or w h >= 2^31, a film whose crop is not w x h.
 * ftn_motion_vectors takes HOST buffers and runs on the GPU `device` (-1 = current); _device takes DEVICE buffers on `stream`; _cpu is
 * the host twin, bit-identical. */
int ftn_motion_vectors(const float* mv8, const float* gb12, const ftn_camera_desc* cur_camera, const ftn_camera_desc* prev_camera,
                       const ftn_film_desc* film, int32_t w, int32_t h, float* out_motion2, int32_t device);
int ftn_motion_vectors_device(const void* mv8, const void* gb12, const ftn_camera_desc* cur_camera, const ftn_camera_desc* prev_camera,
                              const ftn_film_desc* film, int32_t w, int32_t h, void* out_motion2, void* stream);
int ftn_motion_vectors_cpu(const float* mv8, const float* gb12, const ftn_camera_desc* cur_camera, const ftn_camera_desc* prev_camera,
                           const ftn_film_desc* film, int32_t w, int32_t h, float* out_motion2);

/* ftn_temporal_accumulate, _device and _cpu (fountain_hip_temporal.h) with the current frame's mv8 (null: the existing call, bit for
 * bit).  The five steps of that header, with these changes for a covered pixel p, x^prev_p and n^prev_p being mv8's position and normal:
 *   2. motion    r_prev = project(prev_camera, x^prev_p), r_cur = project(cur_camera, x_p).
 *   3. taps      both thresholds use the pass's values: |n^prev_p - n'_q|^2 <= normal_tol and
 *                |n^prev_p . (x^prev_p - x'_q)| <= plane_tol max(z_p, 1e-6).  Under equal cameras a pixel is its own only tap and untested
 *                only when x^prev_p, n^prev_p equal x_p, n_p bit for bit; any other pixel makes both tests.
 *   A pixel whose mv8 coverage class (H / W > 0) differs from gb12's (c_p > 0) has no history.
 * Everything else is unchanged: prepare, albedo conversion, blend, the pass-through of bad pixels, the refusals; mv8 is an input like
 * gb12 for the overlap rule and needs 4-byte alignment.  An mv8 whose position and normal are copied from gb12 (and whose coverage
 * class is gb12's) gives the bits of the existing call.  The device path and the _cpu twin share the per-pixel code and agree bit for bit. */
int ftn_temporal_accumulate_motion(const float* rgb, const float* gb12, const float* var4, const float* mv8, const ftn_camera_desc* cur_camera,
                                   const ftn_film_desc* film, int32_t w, int32_t h, const ftn_camera_desc* prev_camera, const float* prev_gb12,
                                   const ftn_temporal_pixel* prev_history, const ftn_temporal_params* params, ftn_temporal_pixel* out_history,
                                   float* out_rgb, float* out_var4, int32_t device);
int ftn_temporal_accumulate_motion_device(const void* rgb, const void* gb12, const void* var4, const void* mv8, const ftn_camera_desc* cur_camera,
                                          const ftn_film_desc* film, int32_t w, int32_t h, const ftn_camera_desc* prev_camera, const void* prev_gb12,
                                          const void* prev_history, const ftn_temporal_params* params, void* out_history, void* out_rgb,
                                          void* out_var4, void* stream);
int ftn_temporal_accumulate_motion_cpu(const float* rgb, const float* gb12, const float* var4, const float* mv8, const ftn_camera_desc* cur_camera,
                                       const ftn_film_desc* film, int32_t w, int32_t h, const ftn_camera_desc* prev_camera, const float* prev_gb12,
                                       const ftn_temporal_pixel* prev_history, const ftn_temporal_params* params, ftn_temporal_pixel* out_history,
                                       float* out_rgb, float* out_var4);

#define FTN_MOTION_ABI_VERSION 1
int ftn_motion_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* FOUNTAIN_HIP_MOTION_H */
