/*
 * fountain_hip_vectorblur.h -- extension of the C ABI (fountain_hip.h): a vector blur, the image-space stage that blurs a resolved image
 * along the per-pixel screen-space vectors of ftn_motion_vectors (fountain_hip_motion.h).  It is the reconstruction filter of McGuire,
 * Hennessy, Bukowski and Osman, "A Reconstruction Filter for Plausible Motion Blur" (I3D 2012), with a shutter centred on the frame's time
 * and tap offsets rounded to whole pixels: velocities per pixel, the longest velocity per 16 x 16 tile, the longest of a tile's 3 x 3
 * neighbourhood, and a gather along that direction whose weights compare each tap's depth and velocity with the pixel's.
 *
 * The reference renders single frames without a shutter, so these functions have no orc_* twin in the CPU oracle; FTN_ABI_VERSION and the
 * other extensions are unchanged and this one carries a version of its own.  ftn_render and every other entry point are untouched.
 *
 * Input and output.  All images are row-major w x h pixels, w, h > 0 and w * h < 2^31.  rgb, out_rgb: 3 binary32 floats per pixel, linear
 * light (ftn_film_resolve).  motion2: 2 floats per pixel, ftn_motion_vectors' output: where the pixel's surface was in the previous frame
 * minus where it is, in raster pixels; a NaN component means "unknown".  gb12: optional (NULL), the resolved G-buffer
 * (fountain_hip_gbuffer.h), 12 floats per pixel of which only the depth z (float 9) and the coverage c (float 10) are read.  A pixel's
 * depth z_p is 0 with a null gb12; otherwise +inf (background) when !(c > 0) or z is not finite, else z.
 *
 * All arithmetic is binary32 in the order written, no operation fused; sqrt and the divisions are correctly rounded; rint rounds to the
 * nearest integer, ties to even; (float)k converts an integer exactly.  "finite" means neither NaN nor an infinity.
 *
 * 1. Half velocity, per pixel p with m = motion2_p.  s = 0.5f * shutter.  If m.x or m.y is not finite, h = (0, 0); otherwise
 *    h = (s * m.x, s * m.y).  len2 = h.x * h.x + h.y * h.y, len = sqrt(len2).  If len > max_radius: k = max_radius / len,
 *    h = (h.x * k, h.y * k) and len = max_radius.  (A motion so long that len2 overflows has k = 0: h = (0, 0) with len = max_radius, which
 *    blurs nothing along itself.)  The pixel's record is {h.x, h.y, len, z_p}; its key is key_p = len * len.  key_p is never NaN.
 *
 * 2. Tile max.  The tiles are the film's 16 x 16 tiles, tile (tx, ty) covering columns 16 tx .. min(16 tx + 15, w - 1) and rows likewise;
 *    tiles_x = (w + 15) >> 4, tiles_y = (h + 15) >> 4.  A tile's record is {h.x, h.y, key, 0} of the pixel with the largest key among its
 *    pixels; among equal keys the smallest row-major pixel index y * w + x wins.  The rule is a total order, so it does not depend on the
 *    order in which the pixels are compared.
 *
 * 3. Neighbour max.  A tile's neighbour record n is the tile record with the largest key among the tiles (tx + i, ty + j), i, j in
 *    {-1, 0, 1}, that exist; among equal keys the smallest row-major tile index ty * tiles_x + tx wins.
 *
 * 4. Gather, per pixel p = (x, y) of a tile with neighbour record n; hp = the len of p's record, zp its z.
 *    Copies: if n.key <= 0.25f, or a channel of rgb_p is not finite, out_p = rgb_p, the same bits (sign bits and NaN payloads included).
 *    Otherwise, for i = 0 .. taps - 1 ascending:
 *        t = (float)(2 i + 1 - taps) / (float)taps;  ox = rint(t * n.x), oy = rint(t * n.y)       (|ox|, |oy| <= 16; one offset per tile)
 *        q = (x + ox, y + oy);  d = sqrt((float)(ox * ox + oy * oy))
 *    The tap is skipped when ox = oy = 0, when q lies outside the image, or when a channel of rgb_q is not finite.  Otherwise, with hq
 *    and zq from q's record,
 *        wt = (front(zq, zp) * cone(d, hq) + front(zp, zq) * cone(d, hp)) + (2.0f * cyl(d, hq)) * cyl(d, hp)
 *        cone(d, r)   = r > d ? 1.0f - d / r : 0.0f
 *        cyl(d, r)    = !(r > 0) ? 0.0f : 1.0f - (u * u) * (3.0f - 2.0f * u),  e0 = 0.95f * r, e1 = 1.05f * r,
 *                       u = (d - e0) / (e1 - e0) clamped: u < 0 gives 0, u > 1 gives 1 (an infinite u likewise)
 *        front(a, b)  = a <= b ? 1.0f : max(0.0f, 1.0f - (a - b) / (depth_extent * max(b, 1e-6f)))   (0 when a = +inf > b)
 *    wt is finite and >= 0.  The sums start from the centre, wc = (float)taps / (4.0f * max(hp, 0.5f)):
 *        W = wc, S_c = wc * rgb_p.c;   then per tap that is not skipped, in tap order:  W = W + wt, S_c = S_c + wt * rgb_q.c
 *    If no tap had wt > 0 (the sum of the tap weights is 0), out_p = rgb_p, the same bits; otherwise out_p.c = S_c / W.
 *
 * What the weights say.  cone(d, hq): the tap's surface, moving hq pixels in half a shutter, smears over p if it is in front of p (or at
 * p's depth); cone(d, hp): p's own surface smears over the tap's place if the tap is behind it; the cylinders blend two surfaces that both
 * move far enough to reach each other.  A static pixel nearer than every tap by more than depth_extent therefore keeps its bits: a sharp
 * foreground stays sharp over a moving background.  A non-finite colour stays what it was and reaches no other pixel.
 *
 * Why one offset per tile.  The direction of the blur is the neighbourhood's longest velocity, as in the paper; rounding t * n to whole
 * pixels once per tile makes every tap of a tile the tile itself shifted by (ox, oy): coalesced rows, no bilinear fetch, and no decision
 * that could differ between the GPU and the host twin.  The price is a blur sampled at whole pixels: taps beyond about twice the length
 * repeat offsets, and a half velocity below one pixel changes nothing (its nearest tap is a pixel away, where its cone and cylinder are 0).
 *
 * max_radius <= 16.  A blur longer than a tile would reach a tile outside the 3 x 3 neighbourhood of step 3, whose velocity step 3 did
 * not see; radii above 16 are refused rather than blurred wrongly.
 *
 * Workspace (ftn_vectorblur_device), with tiles = tiles_x * tiles_y:
 *     bytes = 16 * w * h + 2 * 16 * tiles
 * the per-pixel records of step 1 (4 floats each, row-major), then the tile records of step 2, then the neighbour records of step 3 (4
 * floats each, row-major over the tiles).  Every byte of it is written by every call.
 *
 * Refusals: FTN_ERR_INVALID_ARGUMENT with a message in ftn_last_error(), in this order, each reached only when everything before it is
 * in order: (1) null pointers (rgb, motion2, params, out_rgb, bytes); (2) w <= 0, h <= 0 or w * h >= 2^31; (3) taps outside 1..64; (4)
 * unknown flag bits; (5) reserved != 0; (6) shutter, max_radius or depth_extent not finite; (7) shutter outside [0, 1], max_radius outside
 * (0, 16], depth_extent <= 0; (8) on the device path a null workspace, then out_rgb overlapping rgb, motion2, gb12 or the workspace or the
 * workspace overlapping one of the inputs, then rgb, motion2, gb12, out_rgb or the workspace not 16-byte aligned; in ftn_vectorblur_cpu
 * out_rgb overlapping rgb.  Then the entries that run on the GPU return FTN_ERR_NO_DEVICE when there is none.
 * ftn_vectorblur_workspace_size stops after (2).
 */
#ifndef FOUNTAIN_HIP_VECTORBLUR_H
#define FOUNTAIN_HIP_VECTORBLUR_H

#include "fountain_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FTN_VECTORBLUR_MAX_TAPS 64
#define FTN_VECTORBLUR_MAX_RADIUS 16    /* the film tile's side                                                                           */

typedef struct ftn_vectorblur_params {  /* 32 bytes                                                                                       */
    int32_t taps;                       /* 1..64: taps per pixel along the blur direction                                                 */
    uint32_t flags;                     /* 0: no bit is defined yet                                                                       */
    float shutter;                      /* [0, 1]: the share of the frame interval the shutter is open, centred on the frame's time       */
    float max_radius;                   /* (0, 16]: the half length in pixels a pixel's blur is clamped to                                */
    float depth_extent;                 /* > 0: the soft depth comparison's width, relative to the nearer depth                           */
    uint32_t reserved[3];               /* 0                                                                                              */
} ftn_vectorblur_params;

/* taps 16, flags 0, shutter 0.5, max_radius 16, depth_extent 0.01.  A null pointer is ignored. */
void ftn_vectorblur_params_default(ftn_vectorblur_params* p);

/* rgb, motion2, gb12 (may be NULL) and out_rgb are HOST buffers; uploads, runs on GPU `device` (-1 = the current one) and downloads. */
int ftn_vectorblur(const float* rgb, const float* motion2, const float* gb12, int32_t w, int32_t h, const ftn_vectorblur_params* params, float* out_rgb, int32_t device);
/* bytes of device workspace ftn_vectorblur_device needs for a w x h image (the formula above). */
int ftn_vectorblur_workspace_size(int32_t w, int32_t h, size_t* bytes);
/* DEVICE buffers on `stream` (a hipStream_t; NULL = the default stream).  Allocates nothing, never synchronises and launches kernels
 * only, so it can be captured in a graph. */
int ftn_vectorblur_device(const void* rgb, const void* motion2, const void* gb12, int32_t w, int32_t h, const ftn_vectorblur_params* params, void* out_rgb, void* workspace, void* stream);
/* the host twin: the same bits, on the host's threads, whatever their number; shares the per-pixel code with the kernels.  out_rgb must
 * not overlap rgb. */
int ftn_vectorblur_cpu(const float* rgb, const float* motion2, const float* gb12, int32_t w, int32_t h, const ftn_vectorblur_params* params, float* out_rgb);
/* steps 1 to 3 of the host twin alone: `workspace` is a HOST buffer of ftn_vectorblur_workspace_size bytes, written in the layout above
 * with the bits ftn_vectorblur_device leaves in its workspace.  Refusals (1) to (7). */
int ftn_vectorblur_velocities_cpu(const float* motion2, const float* gb12, int32_t w, int32_t h, const ftn_vectorblur_params* params, void* workspace);

#define FTN_VECTORBLUR_ABI_VERSION 1
int ftn_vectorblur_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* FOUNTAIN_HIP_VECTORBLUR_H */
