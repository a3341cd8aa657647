/*
 * fountain_hip_denoise.h -- extension of the C ABI (fountain_hip.h): an edge-avoiding a-trous wavelet filter (after Dammertz et al.,
 * HPG 2010) over a resolved beauty image (ftn_film_resolve) and its resolved first-hit G-buffer (ftn_gbuffer_resolve,
 * include/fountain_hip_gbuffer.h), for images rendered with few samples per pixel.
 *
 * The reference has no denoiser, so these functions have no orc_* twin in the CPU oracle; FTN_ABI_VERSION and FTN_GBUFFER_ABI_VERSION are
 * unchanged and the extension carries a version of its own.
 *
 * Inputs, row-major, w x h pixels: rgb = 3 floats per pixel; gb12 = the 12 resolved G-buffer floats per pixel: albedo a, normal n,
 * position x, depth z, coverage c = H / W, weight W.
 *
 *   1. prepare     u_p = rgb_p / max(a_p, albedo_eps) per channel when FTN_DENOISE_DEMODULATE is set and c_p > 0, else u_p = rgb_p;
 *                  every level's colour carries m = (r + g + b) / 3 of its u
 *   2. level i     (i = 0 .. levels - 1, step s = 2^i)  u'_p = sum k(dx) k(dy) w(p,q) u_q / sum k(dx) k(dy) w(p,q),
 *                  q = p + s (dx, dy), dx, dy in -2..2, dy outer and dx inner, both ascending; taps outside the image are skipped;
 *                  k = {1/16, 1/4, 3/8, 1/4, 1/16}
 *                  w(p,q) = 0 when (c_p > 0) != (c_q > 0) (misses and surfaces stay apart) or when u_q has a non-finite component;
 *                  else exp(-(Dc + Dn + Dp)):
 *                    Dc = 2^i |u_p - u_q|^2 / (sigma_color^2 ((m_p^2 + m_q^2) / 2 + color_eps))
 *                    Dn = |n_p - n_q|^2 / sigma_normal^2
 *                    Dp = (n_p . (x_p - x_q))^2 / (sigma_plane^2 max(z_p, 1e-6)^2)
 *                  exp is ftn_det::kexp (binary64, rounded once to binary32).  A NaN exponent (only from non-finite features) counts as
 *                  w = 0.  A pixel whose own u_p is not finite is copied unchanged through every level.
 *   3. remodulate  out_p = u_p max(a_p, albedo_eps) when FTN_DENOISE_DEMODULATE is set and c_p > 0, else out_p = u_p.
 * levels = 0 is an exact copy of rgb.  The device path and ftn_denoise_cpu share the filter's code and agree bit for bit.
 *
 * Refusals (FTN_ERR_INVALID_ARGUMENT, with ftn_last_error()): null pointers; w or h <= 0, or w h >= 2^31; levels outside 0..10; a sigma
 * that is not finite or <= 0; an epsilon that is negative or not finite; a non-zero reserved field; unknown flag bits; on the device
 * path, out_rgb overlapping an input or the workspace, the workspace overlapping an input, or a workspace not aligned to 16 bytes.
 */
#ifndef FOUNTAIN_HIP_DENOISE_H
#define FOUNTAIN_HIP_DENOISE_H

#include "fountain_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FTN_DENOISE_DEMODULATE 1u       /* filter rgb / albedo on covered pixels and multiply the albedo back at the end */
#define FTN_DENOISE_MAX_LEVELS 10

typedef struct ftn_denoise_params {     /* 32 bytes */
    int32_t levels;                     /* a-trous levels, 0..10 (default 5)                                  */
    uint32_t flags;                     /* FTN_DENOISE_* (default FTN_DENOISE_DEMODULATE)                      */
    float sigma_color;                  /* colour edge-stopping width (default 2.0)                            */
    float sigma_normal;                 /* normal edge-stopping width (default 0.3)                            */
    float sigma_plane;                  /* plane-distance edge-stopping width, relative to depth (default 1e-4) */
    float albedo_eps;                   /* floor of the demodulation divisor (default 1e-3)                    */
    float color_eps;                    /* floor term of the colour distance (default 1e-4)                    */
    uint32_t reserved;                  /* must be 0                                                           */
} ftn_denoise_params;

void ftn_denoise_params_default(ftn_denoise_params* params);

/* HOST buffers in and out: uploads, filters on the GPU `device` (-1 = the current device) and downloads.  FTN_ERR_NO_DEVICE without
 * a GPU. */
int ftn_denoise(const float* rgb, const float* gb12, int32_t w, int32_t h, const ftn_denoise_params* params, float* out_rgb, int32_t device);

/* bytes of device workspace ftn_denoise_device needs for a w x h image: 64 per pixel (two float4 colour buffers, two float4 feature
 * buffers) */
int ftn_denoise_workspace_size(int32_t w, int32_t h, size_t* bytes);

/* DEVICE buffers on `stream` (a hipStream_t; NULL = the default stream).  Allocates nothing and does not synchronise, so it can be
 * captured in a graph.  out_rgb must not overlap the inputs or the workspace. */
int ftn_denoise_device(const void* rgb, const void* gb12, int32_t w, int32_t h, const ftn_denoise_params* params, void* out_rgb,
                       void* workspace, void* stream);

/* The host twin of the filter, bit-identical to the device path (it runs the same filter code on the host's threads; the result does
 * not depend on their number).  It exists for tests and tools: rendering still has no CPU fallback. */
int ftn_denoise_cpu(const float* rgb, const float* gb12, int32_t w, int32_t h, const ftn_denoise_params* params, float* out_rgb);

#define FTN_DENOISE_ABI_VERSION 1
int ftn_denoise_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* FOUNTAIN_HIP_DENOISE_H */
