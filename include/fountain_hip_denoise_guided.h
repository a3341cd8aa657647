/*
 * fountain_hip_denoise_guided.h -- extension of the C ABI (fountain_hip.h): a variance-guided edge-avoiding a-trous filter (the spatial
 * part of SVGF, Schied et al., HPG 2017) over a resolved beauty image (ftn_film_resolve), its resolved first-hit G-buffer
 * (ftn_gbuffer_resolve, include/fountain_hip_gbuffer.h) and the variance of each pixel's mean (ftn_moments_resolve,
 * include/fountain_hip_moments.h).  It stands beside ftn_denoise (include/fountain_hip_denoise.h), whose geometry terms, tap pattern
 * and coverage rules it shares; its colour term is normalised by the estimated noise of the centre pixel instead of its brightness.
 *
 * The reference has no denoiser, so these functions have no orc_* twin in the CPU oracle; FTN_ABI_VERSION and FTN_DENOISE_ABI_VERSION
 * are unchanged and the extension carries a version of its own.
 *
 * Inputs, row-major, w x h pixels: rgb = 3 floats per pixel; gb12 = the 12 resolved G-buffer floats per pixel: albedo a, normal n,
 * position x, depth z, coverage c = H / W, weight W; var4 = 4 floats per pixel, the variance of the pixel's mean in r, g, b and Y
 * (ftn_moments_resolve's output).  Only r, g and b of var4 are read.  All arithmetic is binary32 unless stated, one rounding per
 * operation in the order written.
 *
 *   1. prepare     u_p as ftn_denoise: u_p = rgb_p / d_p per channel, d_p = max(a_p, albedo_eps) when FTN_DENOISE_DEMODULATE is set
 *                  and c_p > 0, else u_p = rgb_p and d_p = 1.  The noise power of u_p:
 *                    nu_p = (var_r / (d_r d_r) + var_g / (d_g d_g)) + var_b / (d_b d_b)   (d d rounded, then the quotient)
 *                  nu_p = NaN when var_r, var_g or var_b is NaN or negative.  var = +inf (fewer than 2 samples) gives nu_p = +inf:
 *                  the noise is unknown.  Pixel p is usable when u_p has three finite components and nu_p is not NaN.
 *   2. level i     (i = 0 .. levels - 1, step s = 2^i), for a usable p (any other pixel keeps u_p and nu_p through every level):
 *                  a. centre variance  nuh_p = sum_q k3(dx) k3(dy) nu_q / sum_q k3(dx) k3(dy), q = p + (dx, dy), dx, dy in -1..1
 *                     (unit offsets at every level), dy outer and dx inner, both ascending; k3 = {1/4, 1/2, 1/4}; only q inside the
 *                     image, usable and of p's coverage class ((c_q > 0) == (c_p > 0)) count; both sums start at +0 and add one term
 *                     at a time.  It is recomputed from the current level's nu.
 *                  b. u'_p = sum k(dx) k(dy) w(p,q) u_q / sum k(dx) k(dy) w(p,q), q = p + s (dx, dy), dx, dy in -2..2, dy outer and dx
 *                     inner, both ascending; taps outside the image are skipped; k = {1/16, 1/4, 3/8, 1/4, 1/16}
 *                     w(p,q) = 0 when (c_p > 0) != (c_q > 0) or when q is not usable; else exp(-(Dc + Dn + Dp)), summed in that order:
 *                       Dc = |u_p - u_q|^2 / (kv nuh_p + rel_eps m_p^2),  kv = 2 sigma_variance^2 (sigma_variance^2 rounded, then
 *                            doubled), m_p = (u_p.r + u_p.g + u_p.b) / 3, |.|^2 = (dr dr + dg dg) + db db, m_p^2 = m_p m_p;
 *                            Dc = 0 when |u_p - u_q|^2 = 0 (equal colours are always compatible).  Otherwise a zero denominator
 *                            gives +inf (weight 0), and nuh_p = +inf gives 0 (unknown noise: geometry alone decides).  There is no
 *                            2^i factor: the propagated variance shrinks the width from level to level.
 *                       Dn = |n_p - n_q|^2 / sigma_normal^2            (as ftn_denoise)
 *                       Dp = (n_p . (x_p - x_q))^2 / (sigma_plane^2 max(z_p, 1e-6)^2)   (as ftn_denoise)
 *                     exp is ftn_det::kexp (binary64, rounded once to binary32); an exponent above 104 (exp rounds to binary32 zero)
 *                     or NaN weighs 0.  The tap's weight is wt = (k(dx) k(dy)) exp(-(Dc + Dn + Dp)).
 *                  c. nu'_p = sum wt (wt nu_q) / (W W), W = sum wt, over the taps of b with wt > 0 (a tap of weight 0 adds nothing,
 *                     so 0 inf never arises); an infinite nu_q with wt > 0 makes nu'_p infinite.
 *                  When W is not > 0 (only with non-finite features of p itself) u_p and nu_p are kept.
 *   3. remodulate  out_p = u_p d_p when FTN_DENOISE_DEMODULATE is set and c_p > 0, else out_p = u_p (ftn_denoise's step 3).
 * levels = 0 is an exact copy of rgb.  The device path and ftn_denoise_guided_cpu share the filter's code and agree bit for bit.
 *
 * Two exact properties follow.  Scale: out(2^k rgb, gb12, 4^k var4) = 2^k out(rgb, gb12, var4) bit for bit while nothing overflows or
 * becomes subnormal, since every term of Dc is homogeneous of degree 2 in the colour.  Noise-free pass-through: with var4 = 0 and
 * rel_eps = 0, two taps of different colour never mix.
 *
 * Refusals (FTN_ERR_INVALID_ARGUMENT, with ftn_last_error()): null pointers; w or h <= 0, or w h >= 2^31; levels outside 0..10; a sigma
 * that is not finite or <= 0; an epsilon that is negative or not finite; a non-zero reserved field; flag bits other than
 * FTN_DENOISE_DEMODULATE; on the device path, out_rgb overlapping an input or the workspace, the workspace overlapping an input, a
 * workspace not aligned to 16 bytes or an image not aligned to 4.
 */
#ifndef FOUNTAIN_HIP_DENOISE_GUIDED_H
#define FOUNTAIN_HIP_DENOISE_GUIDED_H

#include "fountain_hip_denoise.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ftn_denoise_guided_params {  /* 32 bytes */
    int32_t levels;                     /* a-trous levels, 0..10 (default 5)                                   */
    uint32_t flags;                     /* FTN_DENOISE_DEMODULATE only (default FTN_DENOISE_DEMODULATE)         */
    float sigma_variance;               /* colour edge-stopping width in standard deviations (default 2.0)      */
    float sigma_normal;                 /* normal edge-stopping width (default 0.3)                             */
    float sigma_plane;                  /* plane-distance edge-stopping width, relative to depth (default 0.1)  */
    float albedo_eps;                   /* floor of the demodulation divisor (default 1e-3)                     */
    float rel_eps;                      /* relative floor of the colour distance's denominator (default 1e-4)  */
    uint32_t reserved;                  /* must be 0                                                            */
} ftn_denoise_guided_params;

void ftn_denoise_guided_params_default(ftn_denoise_guided_params* params);

/* HOST buffers in and out: uploads, filters on the GPU `device` (-1 = the current device) and downloads.  FTN_ERR_NO_DEVICE without
 * a GPU. */
int ftn_denoise_guided(const float* rgb, const float* gb12, const float* var4, int32_t w, int32_t h, const ftn_denoise_guided_params* params,
                       float* out_rgb, int32_t device);

/* bytes of device workspace ftn_denoise_guided_device needs for a w x h image: 64 per pixel (two float4 colour buffers {u, nu}, two
 * float4 feature buffers) */
int ftn_denoise_guided_workspace_size(int32_t w, int32_t h, size_t* bytes);

/* DEVICE buffers on `stream` (a hipStream_t; NULL = the default stream).  Allocates nothing and does not synchronise, so it can be
 * captured in a graph.  out_rgb must not overlap the inputs or the workspace. */
int ftn_denoise_guided_device(const void* rgb, const void* gb12, const void* var4, int32_t w, int32_t h, const ftn_denoise_guided_params* params,
                              void* out_rgb, void* workspace, void* stream);

/* The host twin of the filter, bit-identical to the device path (it runs the same filter code on the host's threads; the result does
 * not depend on their number).  It exists for tests and tools: rendering still has no CPU fallback. */
int ftn_denoise_guided_cpu(const float* rgb, const float* gb12, const float* var4, int32_t w, int32_t h, const ftn_denoise_guided_params* params,
                           float* out_rgb);

#define FTN_DENOISE_GUIDED_ABI_VERSION 1
int ftn_denoise_guided_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* FOUNTAIN_HIP_DENOISE_GUIDED_H */
