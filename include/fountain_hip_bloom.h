/*
 * fountain_hip_bloom.h -- extension of the C ABI (fountain_hip.h): an HDR bloom (glare) operator in linear light, applied to a resolved
 * image before the display stage (fountain_hip_display.h): a prefilter, a chain of 2:1 down-samplings, a chain of 2:1 up-samplings that
 * blends the levels, and a composite that only moves energy.
 *
 * The reference writes linear OpenEXR files only, so these functions have no orc_* twin in the CPU oracle; FTN_ABI_VERSION and the other
 * extensions are unchanged and this one carries a version of its own.  ftn_render and every other entry point are untouched.
 *
 * Input and output.  rgb, out_rgb: row-major w x h pixels, 3 binary32 floats each, linear light (ftn_film_resolve).  w, h > 0 and
 * w * h < 2^31.  All arithmetic is binary32 in the order written, no operation fused.  Y(v) = v.r * 0.212671f + v.g * 0.715160f +
 * v.b * 0.072169f in that order (Spectrum::y, as in the display stage).
 *
 * 1. Prefilter, P = pre(in), per pixel.  Per channel s_c = !(c > 0) ? 0 : (c > clamp_max ? clamp_max : c): NaN, negatives, -0 and -inf
 *    become 0, +inf becomes clamp_max.  If threshold == 0, P = s.  Otherwise Y = Y(s), K = knee * threshold and
 *        g = Y - threshold                                       when Y >= threshold + K
 *        g = (t * t) / (4 * K), t = (Y - threshold) + K          when Y > threshold - K and K > 0
 *        g = 0                                                   otherwise
 *    and P = s * (g / Y) per channel, or 0 when g == 0.  P is always finite and >= 0: a NaN, an infinity or a negative number never
 *    enters the pyramid.
 *
 * 2. Down chain.  D_0 = P, w_0 = w, h_0 = h; w_{k+1} = (w_k + 1) >> 1, h_{k+1} = (h_k + 1) >> 1.  L = min(levels, the number of halvings
 *    after which both sides are 1).  With kappa = {1/8, 3/8, 3/8, 1/8},
 *        D_{k+1}(x, y) = sum_{j = 0..3} sum_{i = 0..3} (kappa_j * kappa_i) * D_k(clamp(2x - 1 + i, 0, w_k - 1), clamp(2y - 1 + j, 0, h_k - 1))
 *    per channel, j the outer loop and i the inner, both ascending, accumulated from +0; a tap's weight kappa_j * kappa_i is formed first
 *    (it is exact).  With FTN_BLOOM_KARIS the first step (D_0 -> D_1) only uses the weight q = (kappa_j * kappa_i) * (1 / (1 + Y(tap))),
 *    the quotient rounded before the product, accumulates the sum of the q's in the same loop and divides each channel's sum by it.  Every
 *    q is above 0 (Y(tap) <= 3e30), so the divisor is too.  This is the usual suppression of single-pixel fireflies; it deliberately gives
 *    up the conservation of energy below in that first step.
 *
 * 3. Up chain.  up(C)(x, y) for a coarse level C of wc x hc pixels is the 2 x 2 tent: coarse columns x0 = (x - 1) >> 1 (arithmetic
 *    shift: -1 for x = 0) and x0 + 1, both clamped to [0, wc - 1], with weights {1/4, 3/4} for even x and {3/4, 1/4} for odd x; rows
 *    likewise.  Rows are the outer loop and columns the inner, ascending, accumulated from +0; a tap's weight is the product of its row
 *    and column factors (exact).  U_L = D_L; for k = L - 1 ... 1, U_k = D_k * (1 - scatter) + up(U_{k+1}) * scatter per channel, with
 *    1 - scatter rounded once; B = up(U_1).
 *
 * 4. Composite, per channel c of `in`, with P recomputed from `in`: out = c + strength * (B - P) when c is finite and not below 0 (-0
 *    counts as 0); otherwise out = c, the same bits.  So a NaN, an infinity or a negative number stays what it was, and the prefilter
 *    keeps it out of every other pixel (what a +inf sends into the pyramid is clamp_max).  With strength == 0 or L == 0 (a 1 x 1 image
 *    or levels == 0) out is an exact copy of `in`, sign bits and NaN payloads included.
 *
 * Why this form.  The down step spreads each source pixel with total weight 1/4, the up step each coarse pixel with total weight 4, so
 * sum(B) = sum(P) away from the clamped borders and the composite only moves energy: sum(out) = sum(in), whatever the threshold.
 *
 * Exact properties, and where they end.  The weights of both steps are dyadic and sum to 1, so for a constant image whose value c has
 * at most 18 significant bits (every partial sum k * c / 64, k <= 64, is then representable) every D_k and every up() is c exactly.
 * The blend c * (1 - scatter) + c * scatter is exact as well for scatter 0, 0.5 and 1 (and for another dyadic scatter while its
 * products with c are representable): then the image comes back bit for bit at any strength.  With another scatter (the default 0.7)
 * each blend may miss c by about an ulp, B - P is then a few ulps of c (about 1 / (1 - scatter) at most), and the image comes back
 * bit for bit only while strength times that stays below half an ulp (the defaults give 0.04 * 3.3), which strength 1 does not.
 * Likewise the order of every sum is fixed above and a flip or a transpose of the image reverses it: the bloom of an image that is
 * symmetric under a flip or the transpose is symmetric bit for bit where every sum is exact (values that are powers of two, dyadic
 * scatter and strength, no threshold gain, no FTN_BLOOM_KARIS), and to within the rounding of the sums, a few ulps, otherwise.
 *
 * Workspace (ftn_bloom_device).  U_k overwrites D_k in place, so one buffer per level 1..L is enough:
 *     bytes = sum_{k = 1..L} 16 * ceil(12 * w_k * h_k / 16)
 * level k's buffer follows level k - 1's.  It is 0 when L == 0; then the workspace may be null.
 *
 * Refusals: FTN_ERR_INVALID_ARGUMENT with a message in ftn_last_error(), in this order, each reached only when everything before it is
 * in order: (1) null pointers (rgb, params, out_rgb, bytes); (2) w <= 0, h <= 0 or w * h >= 2^31; (3) levels outside 0..12; (4) unknown
 * flag bits; (5) reserved != 0; (6) strength, scatter, threshold, knee or clamp_max not finite; (7) strength, scatter or knee outside
 * [0, 1], threshold < 0, clamp_max outside (0, 1e30]; (8) on the device path a null workspace where the size is not 0, then out_rgb
 * overlapping rgb or the workspace or the workspace overlapping rgb, then rgb, out_rgb or the workspace not 16-byte aligned.  Then the
 * entries that run on the GPU return FTN_ERR_NO_DEVICE when there is none.  ftn_bloom_workspace_size stops after (3).
 */
#ifndef FOUNTAIN_HIP_BLOOM_H
#define FOUNTAIN_HIP_BLOOM_H

#include "fountain_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FTN_BLOOM_KARIS 1u              /* ftn_bloom_params.flags: the luminance-weighted first down step of 2.                            */
#define FTN_BLOOM_MAX_LEVELS 12

typedef struct ftn_bloom_params {       /* 32 bytes                                                                                       */
    int32_t levels;                     /* 0..12: the pyramid's depth, cut to what the image allows                                       */
    uint32_t flags;                     /* FTN_BLOOM_KARIS                                                                                */
    float strength;                     /* [0, 1]: how much of the image is replaced by its bloom                                         */
    float scatter;                      /* [0, 1]: how much of each level comes from the coarser ones                                     */
    float threshold;                    /* >= 0: luminance below which a pixel blooms nothing; 0 = everything blooms                      */
    float knee;                         /* [0, 1]: the soft knee's half width as a share of the threshold                                 */
    float clamp_max;                    /* (0, 1e30]: what enters the pyramid is clamped to this                                          */
    uint32_t reserved;                  /* 0                                                                                              */
} ftn_bloom_params;

/* levels 6, flags 0, strength 0.04, scatter 0.7, threshold 0, knee 0.5, clamp_max 65504.  A null pointer is ignored. */
void ftn_bloom_params_default(ftn_bloom_params* p);

/* rgb and out_rgb are HOST buffers (they may be the same); uploads, runs on GPU `device` (-1 = the current one) and downloads. */
int ftn_bloom(const float* rgb, int32_t w, int32_t h, const ftn_bloom_params* params, float* out_rgb, int32_t device);
/* bytes of device workspace ftn_bloom_device needs for a w x h image and `levels` (the formula above). */
int ftn_bloom_workspace_size(int32_t w, int32_t h, int32_t levels, size_t* bytes);
/* DEVICE buffers on `stream` (a hipStream_t; NULL = the default stream).  Allocates nothing, never synchronises and launches kernels
 * only (the exact copy included), so it can be captured in a graph. */
int ftn_bloom_device(const void* rgb, int32_t w, int32_t h, const ftn_bloom_params* params, void* out_rgb, void* workspace, void* stream);
/* the host twin: the same bits, on the host's threads, whatever their number; shares the per-pixel code with the kernels.  out_rgb must
 * not overlap rgb. */
int ftn_bloom_cpu(const float* rgb, int32_t w, int32_t h, const ftn_bloom_params* params, float* out_rgb);

#define FTN_BLOOM_ABI_VERSION 1
int ftn_bloom_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* FOUNTAIN_HIP_BLOOM_H */
