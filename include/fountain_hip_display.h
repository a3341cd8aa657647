/*
 * fountain_hip_display.h -- extension of the C ABI (fountain_hip.h): the display stage between a resolved linear-light image and pixels
 * on a screen -- a luminance histogram, an exposure (manual, or automatic from the histogram), a tone curve, a transfer function, 8-bit
 * quantisation with an optional ordered dither, and a PNG writer.
 *
 * The reference writes linear OpenEXR files only, so these functions have no orc_* twin in the CPU oracle; FTN_ABI_VERSION and the other
 * extensions are unchanged and this one carries a version of its own.  ftn_render and every other entry point are untouched.
 *
 * Input.  rgb: row-major w x h pixels, 3 binary32 floats each, linear light (ftn_film_resolve).  w, h > 0 and w * h < 2^31.
 *
 * Luminance histogram.  Y = r * 0.212671f + g * 0.715160f + b * 0.072169f in binary32 in that order (Spectrum::y).  The histogram is
 * FTN_DISPLAY_HIST_WORDS uint32_t words:
 *   [0, 384)   bins over [2^-24, 2^24), eight per octave, from the float's bits alone: bin = (bits(Y) >> 20) - 824, 824 being
 *              bits(2^-24) >> 20.  Bin i = 8 (o + 24) + m covers [2^o (1 + m / 8), 2^o (1 + (m + 1) / 8)).  Nothing computes a logarithm.
 *   [384]      FTN_DISPLAY_HIST_INVALID: pixels whose Y is NaN or negative, i.e. !(Y >= 0); -0 counts as 0
 *   [385]      FTN_DISPLAY_HIST_BELOW:   0 <= Y < 2^-24 (subnormals included)
 *   [386]      FTN_DISPLAY_HIST_ABOVE:   Y >= 2^24, +inf included
 *   [387]      0 (pads the array to a multiple of 16 bytes)
 * Every word is a full 32-bit count.  Counts are integers, so the histogram does not depend on the order in which pixels are counted:
 * the device, the host twin and any restatement agree bit for bit.
 *
 * Exposure (host only, binary64, from the histogram words).  Manual mode (no FTN_DISPLAY_AUTO_EXPOSURE): scale = 2^ev, rounded once to
 * binary32.  Automatic mode: t = the sum of the 384 bins; the window is [p_lo t, p_hi t]; with c_i the count of the bins below i, bin
 * i's weight is w_i = max(0, min(c_i + n_i, p_hi t) - max(c_i, p_lo t)) and its representative r_i = o + log2(1 + (m + 0.5) / 8), log2
 * of its arithmetic centre; avg_log2 = sum(w_i r_i) / sum(w_i), i ascending; scale = key / 2^avg_log2, clamped to
 * [2^min_ev, 2^max_ev], rounded once to binary32.  If t = 0: scale = 1, avg_log2 = 0 and FTN_DISPLAY_INFO_EMPTY is set in info.flags.
 *
 * Encode, per pixel (x, y), all in binary32, no operation fused.  clamp01(v) = !(v > 0) ? 0 : (v > 1 ? 1 : v), so a NaN becomes 0.
 *   1. c = rgb * scale per channel; c = !(c > 0) ? 0 : (c > 65504 ? 65504 : c).  NaN, negatives and -inf become 0, +inf 65504.
 *   2. the tone curve (params.tonemap), then clamp01:
 *        LINEAR    c
 *        REINHARD  L = c.r * 0.212671f + c.g * 0.715160f + c.b * 0.072169f; if L == 0, c; else with w2 = white * white,
 *                  Lp = (L * (1 + L / w2)) / (1 + L), s = Lp / L, c * s per channel
 *        ACES      per channel (x * (2.51f * x + 0.03f)) / (x * (2.43f * x + 0.59f) + 0.14f)   (Narkowicz's fit)
 *        HABLE     per channel f(x) / f(white), f(x) = (x * (A * x + C * B) + D * E) / (x * (A * x + B) + D * F) - (D * E) / (D * F)
 *                  with A..F = 0.15f, 0.50f, 0.10f, 0.20f, 0.02f, 0.30f; C * B, D * E and D * F are binary32 operations themselves.
 *                  The subtrahend is E / F written as (D * E) / (D * F), the first term's value at 0, so that f(0) is exactly 0:
 *                  with a rounded E / F it is 7e-9, which a gamma transfer lifts to 2e-4 and the dither then to code 1
 *   3. the transfer (params.transfer), then clamp01:
 *        SRGB      v <= 0.0031308f ? 12.92f * v : 1.055f * powf_det(v, (float)(1.0 / 2.4)) - 0.055f
 *        GAMMA     powf_det(v, 1.0f / gamma)
 *        LINEAR    v
 *      powf_det is the library's deterministic powf (binary64 exp(y ln x), rounded once), the same on the device and the host.
 *   4. out_rgb (optional) receives the three values of step 3.  out_rgba8 receives one uint32_t: R | G << 8 | B << 16 | 255 << 24, each
 *      code = min(max(floorf((v * 255.0f + 0.5f) + d), 0), 255) as an integer; d = 0, or with FTN_DISPLAY_DITHER
 *      d = ((float)B[y & 7][x & 7] + 0.5f) / 64.0f - 0.5f (exact) from the 8 x 8 Bayer matrix
 *            0 32  8 40  2 34 10 42
 *           48 16 56 24 50 18 58 26
 *           12 44  4 36 14 46  6 38
 *           60 28 52 20 62 30 54 22
 *            3 35 11 43  1 33  9 41
 *           51 19 59 27 49 17 57 25
 *           15 47  7 39 13 45  5 37
 *           63 31 55 23 61 29 53 21
 *      |d| < 0.5, so black stays 0 and white stays 255 under the dither.
 *
 * Refusals: FTN_ERR_INVALID_ARGUMENT with a message in ftn_last_error(), in this order, each reached only when everything before it is
 * in order: (1) null pointers (out_rgb may be null everywhere; the histogram may be null for ftn_display_exposure in manual mode);
 * (2) w <= 0, h <= 0 or w * h >= 2^31; (3) an unknown tonemap, an unknown transfer, unknown flag bits; (4) reserved != 0; (5) ev, key,
 * white or gamma not finite; (6) key, white or gamma <= 0; (7) percentiles outside 0 <= p_lo < p_hi <= 1; (8) !(min_ev <= max_ev);
 * (9) for the encode entries a scale that is not finite or is negative; (10) on the device path an output that overlaps the input or
 * the other output, then rgb, out_rgb, out_rgba8 or the histogram not 16-byte aligned.  Then the entries that run on the GPU return
 * FTN_ERR_NO_DEVICE when there is none.  The histogram entries take no parameters and skip (3) to (9).
 */
#ifndef FOUNTAIN_HIP_DISPLAY_H
#define FOUNTAIN_HIP_DISPLAY_H

#include "fountain_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { FTN_DISPLAY_TONEMAP_LINEAR = 0, FTN_DISPLAY_TONEMAP_REINHARD = 1, FTN_DISPLAY_TONEMAP_ACES = 2, FTN_DISPLAY_TONEMAP_HABLE = 3 };
enum { FTN_DISPLAY_TRANSFER_SRGB = 0, FTN_DISPLAY_TRANSFER_GAMMA = 1, FTN_DISPLAY_TRANSFER_LINEAR = 2 };
#define FTN_DISPLAY_DITHER 1u            /* ftn_display_params.flags: the ordered dither of step 4                                        */
#define FTN_DISPLAY_AUTO_EXPOSURE 2u     /* ftn_display_params.flags: automatic mode (ev is not read); without it manual mode             */
#define FTN_DISPLAY_INFO_EMPTY 1u        /* ftn_display_info.flags: automatic mode found no pixel in the 384 bins                         */

#define FTN_DISPLAY_HIST_BINS 384
#define FTN_DISPLAY_HIST_INVALID 384
#define FTN_DISPLAY_HIST_BELOW 385
#define FTN_DISPLAY_HIST_ABOVE 386
#define FTN_DISPLAY_HIST_WORDS 388

typedef struct ftn_display_params {     /* 48 bytes                                                                                       */
    uint32_t tonemap;                   /* FTN_DISPLAY_TONEMAP_*                                                                          */
    uint32_t transfer;                  /* FTN_DISPLAY_TRANSFER_*                                                                         */
    uint32_t flags;                     /* FTN_DISPLAY_DITHER | FTN_DISPLAY_AUTO_EXPOSURE                                                 */
    uint32_t reserved;                  /* 0                                                                                              */
    float ev;                           /* manual mode: scale = 2^ev                                                                      */
    float key;                          /* automatic mode: the value the window's log-average is mapped to                                */
    float white;                        /* REINHARD and HABLE: the scaled value that maps to 1                                            */
    float gamma;                        /* FTN_DISPLAY_TRANSFER_GAMMA                                                                     */
    float p_lo, p_hi;                   /* automatic mode: the window's percentiles                                                       */
    float min_ev, max_ev;               /* automatic mode: scale is clamped to [2^min_ev, 2^max_ev]                                       */
} ftn_display_params;

typedef struct ftn_display_info {       /* 32 bytes                                                                                       */
    float scale;                        /* what the encode entries take                                                                   */
    uint32_t flags;                     /* FTN_DISPLAY_INFO_EMPTY                                                                         */
    double avg_log2;                    /* automatic mode; 0 in manual mode or when empty                                                 */
    uint32_t count_bins;                /* t: pixels in the 384 bins (the counts are 0 when no histogram was given)                       */
    uint32_t count_invalid, count_below, count_above;
} ftn_display_info;

/* tonemap ACES, transfer SRGB, flags 0 (manual, no dither), ev 0, key 0.18, white 11.2, gamma 2.2, p_lo 0.10, p_hi 0.95, min_ev -16,
 * max_ev 16.  A null pointer is ignored. */
void ftn_display_params_default(ftn_display_params* p);

/* rgb and hist (FTN_DISPLAY_HIST_WORDS words, overwritten) are HOST buffers; counted on GPU `device` (-1 = the current one). */
int ftn_display_histogram(const float* rgb, int32_t w, int32_t h, uint32_t* hist, int32_t device);
/* DEVICE buffers on `stream` (a hipStream_t; NULL = the default stream).  Clears hist on that stream itself, allocates nothing and
 * does not synchronise, so it can be captured in a graph. */
int ftn_display_histogram_device(const void* rgb, int32_t w, int32_t h, void* hist, void* stream);
/* the host twin: the same words, on the host's threads, whatever their number */
int ftn_display_histogram_cpu(const float* rgb, int32_t w, int32_t h, uint32_t* hist);

/* Host only.  Refusals (1) and (3) to (8); fills every field of *info. */
int ftn_display_exposure(const uint32_t* hist, const ftn_display_params* params, ftn_display_info* info);

/* Steps 1 to 4 with the given scale (ftn_display_info.scale, so that a sequence of images can share one exposure); params->ev and the
 * automatic-mode fields are checked but not read.  Host buffers, encoded on GPU `device`. */
int ftn_display_encode(const float* rgb, int32_t w, int32_t h, const ftn_display_params* params, float scale, float* out_rgb,
                       uint32_t* out_rgba8, int32_t device);
/* DEVICE buffers on `stream`; allocates nothing and does not synchronise */
int ftn_display_encode_device(const void* rgb, int32_t w, int32_t h, const ftn_display_params* params, float scale, void* out_rgb,
                              void* out_rgba8, void* stream);
/* the host twin: the same bits, on the host's threads, whatever their number; shares the per-pixel code with the kernel */
int ftn_display_encode_cpu(const float* rgb, int32_t w, int32_t h, const ftn_display_params* params, float scale, float* out_rgb,
                           uint32_t* out_rgba8);

/* The whole chain on host buffers: the histogram (in automatic mode only), ftn_display_exposure, the encode.  info may be null.  An
 * exposure whose scale rounds to infinity (an ev of 128 or more) is refused as in (9). */
int ftn_display(const float* rgb, int32_t w, int32_t h, const ftn_display_params* params, float* out_rgb, uint32_t* out_rgba8,
                ftn_display_info* info, int32_t device);

/* An 8-bit RGB PNG file (colour type 2, no interlace) from w x h out_rgba8 words; alpha is dropped.  Filter type 0 on every scanline,
 * one zlib stream in one IDAT chunk.  Chunks: IHDR, then sRGB (rendering intent 0) or, with FTN_PNG_GAMA, gAMA holding flags >> 8 (the
 * file gamma times 100000, above 0: FTN_PNG_GAMA_OF(1 / 2.2) for a 2.2 display gamma, FTN_PNG_GAMA_OF(1) for linear codes), then IDAT,
 * then IEND.  FTN_ERR_INVALID_ARGUMENT, in this order: null pointers; w or h 0 or w * h >= 2^31; unknown flag bits, or a gAMA value
 * without FTN_PNG_GAMA or of 0 with it; a path that cannot be created (the code ftn_exr_write gives).  FTN_ERR_INTERNAL for a short
 * write. */
#define FTN_PNG_GAMA 1u
#define FTN_PNG_GAMA_OF(file_gamma) ((((uint32_t)((file_gamma) * 100000.0 + 0.5)) << 8) | FTN_PNG_GAMA)
int ftn_png_write(const char* path, const uint32_t* rgba8, uint32_t w, uint32_t h, uint32_t flags);

#define FTN_DISPLAY_ABI_VERSION 1
int ftn_display_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* FOUNTAIN_HIP_DISPLAY_H */
