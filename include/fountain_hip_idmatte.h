/*
 * fountain_hip_idmatte.h -- extension of the C ABI (fountain_hip.h): ID mattes.  Per pixel, a ranked list of (id, coverage) pairs over
 * exactly the camera samples ftn_render traces for the same sampler, tiles and film, with the same box-filter footprints; a resolve
 * that ranks the list; a matte extraction over a set of ids; and a multi-channel OpenEXR writer for the Cryptomatte encoding
 * (fountain_amd/idmatte.py).
 *
 * The reference renders no mattes, so these functions have no orc_* twin in the CPU oracle; FTN_ABI_VERSION is unchanged and the
 * extension carries a version of its own.
 *
 * What a sample records is the G-buffer's rule (fountain_hip_gbuffer.h): the first surface that HAS a material; null-material
 * primitives are passed through along the same direction, at most 4096 times per sample (beyond that the call fails with
 * FTN_ERR_INTERNAL).  The sample's id is the caller's id of that surface's primitive.  A sample that ends in a miss has no id.
 *
 * How a sample with id x and box-filter weight w (= 1) enters the table of a pixel of its footprint:
 *   a miss                         miss += w
 *   a used slot k holds x          weight[k] += w              (the first such slot)
 *   else n_used < FTN_IDMATTE_SLOTS   id[n_used] = x, weight[n_used] = w, n_used += 1
 *   else                           overflow += w
 *   always                         total += w
 * The caller's buffer is continued, not replaced: a second call goes on with the tables the first one left.
 *
 * Order (it decides the first-seen order of the slots and, once a table is full, which ids it holds): a pixel takes its OWN samples one
 * at a time in increasing sample index; the samples of OTHER pixels whose footprint reaches it come after all of the call's own samples,
 * ordered by sample index, then by the source pixel's offset from the destination (dy, dx) in row-major order.  Footprints are those of
 * Film::add_sample_to_tile (src/film.rs:133-172) inside the source tile's pixel bounds.  The result is a function of the arguments
 * alone.  Every weight is 1, so every sum is a small integer and exact in binary32.
 */
#ifndef FOUNTAIN_HIP_IDMATTE_H
#define FOUNTAIN_HIP_IDMATTE_H

#include "fountain_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FTN_IDMATTE_SLOTS 8
typedef struct ftn_idmatte_pixel {          /* 80 bytes */
    uint32_t id[FTN_IDMATTE_SLOTS];         /* in first-seen order; unused slots 0            */
    float    weight[FTN_IDMATTE_SLOTS];     /* sum of w over the samples that recorded id[k]  */
    float    overflow;                      /* sum of w over samples whose id found the table full */
    float    miss;                          /* sum of w over samples that recorded no surface */
    float    total;                         /* sum of w over all samples (= ftn_pixel.filter_weight_sum, = ftn_gbuffer_pixel.weight) */
    uint32_t n_used;
} ftn_idmatte_pixel;

/* Arguments, tile rules and sample ranges as ftn_render_gbuffer.  prim_ids: one id per primitive in the scene description's insertion
 * order (n_prim_ids must be the scene's primitive count).  FTN_ERR_UNSUPPORTED for FTN_SAMPLER_TILE_SERIAL, FTN_PIPELINE_MEGAKERNEL and
 * a filter radius above 1 in either axis (footprints of up to 3 x 3 pixels are supported); FTN_ERR_INVALID_ARGUMENT for null arguments
 * and a wrong n_prim_ids; FTN_ERR_NO_DEVICE without a GPU.  Every refusal comes before any device work.
 * Samples that reach other pixels are kept in a list until the call's own samples are in (16 bytes each, sorted on the device).  With
 * a radius of at most 0.5 only rounding produces them and the list is small; should it not hold them all, or should the list of a wider
 * radius not fit in device memory, the call fails with FTN_ERR_OUT_OF_MEMORY and a message (the host entry then leaves out_pixels as it
 * was, the device entry leaves device_pixels undefined); nothing is ever dropped.  Render such a film in several sample ranges.
 * Statistics: rays_closest, camera_samples, spill_samples, kernel_ms, trace_ms.
 * out_pixels: HOST buffer of crop-width x crop-height pixels, continued. */
int ftn_render_idmatte(const ftn_scene* scene, const ftn_camera_desc* camera, const ftn_film_desc* film,
                       const ftn_sampler_desc* sampler, const ftn_tile_range* tiles, const ftn_render_options* options,
                       const uint32_t* prim_ids, size_t n_prim_ids, ftn_idmatte_pixel* out_pixels, ftn_stats* stats);
/* device_pixels: DEVICE buffer of ftn_idmatte_pixel (4-byte aligned), continued on `stream` (a hipStream_t; NULL = the default stream) */
int ftn_render_idmatte_device(const ftn_scene* scene, const ftn_camera_desc* camera, const ftn_film_desc* film,
                              const ftn_sampler_desc* sampler, const ftn_tile_range* tiles, const ftn_render_options* options,
                              const uint32_t* prim_ids, size_t n_prim_ids, void* device_pixels, void* stream, ftn_stats* stats);

/* out20: 20 32-bit words per pixel.  The slots k < min(n_used, 8) are ranked by weight descending, ties by id ascending; unused slots
 * follow with id 0 and coverage 0.  Words 2r, 2r + 1: the id of rank r (its uint32 bits) and coverage = weight / total; then
 * overflow / total, miss / total, total, and n_used as a float.  One f32 divide each; total == 0 -> all twenty words zero.
 * The host version and the _device version (HBM, on `stream`) give the same bits. */
#define FTN_IDMATTE_RESOLVED_WORDS 20
int ftn_idmatte_resolve(const ftn_idmatte_pixel* in, size_t n, void* out20);
int ftn_idmatte_resolve_device(const void* in, size_t n, void* out20, void* stream);

/* mask_out[i] = the sum, in rank order from 0.0f, of the coverages of pixel i's ranks whose id is in ids[0, n_ids), then the overflow
 * share (FTN_IDMATTE_SELECT_OVERFLOW) and the miss share (FTN_IDMATTE_SELECT_MISS).  `resolved` is the output of ftn_idmatte_resolve.
 * ids is a HOST array in both variants, in any order, duplicates allowed.  Unknown flag bits: FTN_ERR_INVALID_ARGUMENT. */
#define FTN_IDMATTE_SELECT_OVERFLOW 1u
#define FTN_IDMATTE_SELECT_MISS 2u
int ftn_idmatte_select(const void* resolved, size_t n, const uint32_t* ids, size_t n_ids, uint32_t flags, float* mask_out);
int ftn_idmatte_select_device(const void* resolved, size_t n, const uint32_t* ids, size_t n_ids, uint32_t flags, void* mask_out, void* stream);

/* A scanline OpenEXR file (version 2, NO_COMPRESSION, increasing y) of n_channels FLOAT channels, planes[c] = width x height floats of
 * channel names[c], written bit for bit.  The header lists the channels sorted by name, as the format demands, whatever the caller's
 * order; the n_attrs extra attributes are written as type `string`.  FTN_ERR_INVALID_ARGUMENT, before the file is created, for null
 * pointers, zero sizes, duplicate or empty channel names and names (channels, attributes) of 256 bytes or more; as ftn_exr_write,
 * FTN_ERR_INVALID_ARGUMENT when the file cannot be created and FTN_ERR_INTERNAL on a short write.  ftn_exr_write / ftn_exr_read are
 * unchanged (the reader takes RGB files, not these). */
int ftn_exr_write_channels(const char* path, int32_t width, int32_t height, int32_t n_channels, const char* const* names,
                           const float* const* planes, int32_t n_attrs, const char* const* attr_names, const char* const* attr_values);

#define FTN_IDMATTE_ABI_VERSION 1
int ftn_idmatte_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* FOUNTAIN_HIP_IDMATTE_H */
