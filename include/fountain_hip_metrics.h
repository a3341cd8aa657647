/*
 * fountain_hip_metrics.h -- extension of the C ABI (fountain_hip.h): the measuring stage of the image pipeline.  Two resolved images in,
 * the standard rendering error measures out: MSE, RMSE, MAE, relMSE, SMAPE, PSNR, the largest difference and, on request, SSIM; per image,
 * per 16 x 16 film tile and per pixel.
 *
 * The reference compares no images, so these functions have no orc_* twin in the CPU oracle; FTN_ABI_VERSION and the other extensions are
 * unchanged and this one carries a version of its own.  ftn_render and every other entry point are untouched.
 *
 * Inputs.  test, ref: row-major w x h pixels, 3 binary32 floats each (ftn_film_resolve).  w, h > 0 and w * h < 2^31.  They may be the
 * same buffer.  Pixel p = y * w + x.
 *
 * Arithmetic.  Everything below is binary64, in the order written, no operation fused.
 *
 * Bad pixels.  A pixel is bad when any of its six values is not finite.  Bad pixels are counted (n_nonfinite), add nothing to any sum,
 * and no SSIM window that holds one exists.
 *
 * Pointwise terms of a pixel that is not bad, per channel c = 0, 1, 2, with eps = (double)rel_eps:
 *     a = (double)test   b = (double)ref   d = a - b
 *     se_c = d * d   ae_c = |d|   rel_c = se_c / (b * b + eps)   sm_c = ae_c / ((|a| + |b|) + eps)
 * and per pixel SE_p = (se_0 + se_1) + se_2, likewise AE_p, REL_p, SM_p.  The three se_c are also summed on their own (the per-channel
 * MSE).  max_abs is the largest ae_c of the image, max_abs_index the smallest p that attains it (0 and 0 where every pixel is bad).
 * n_different counts the pixels of which any of the three binary32 bit patterns differ, bad pixels included; -0 against +0 differs.
 *
 * SSIM (Wang et al. 2004, an 11 x 11 Gaussian window of sigma 1.5, "valid" windows only), with FTN_METRICS_SSIM.
 *     weights   e_k = exp(-((k - 5)^2) / 4.5), k = 0..10 (the host's exp, binary64, once per call); s = the sum of the e_k, k ascending,
 *               from +0.0; g_k = e_k / s.  ftn_metrics_ssim_weights returns the g_k.
 *     planes    per channel, v in {a, b, a * a, b * b, a * b}
 *     passes    horizontal: H_v(x, y) = sum_k g_k * v(x + k - 5, y) as acc = acc + g_k * v, k ascending, from +0.0; vertical: the same
 *               expression over H_v, down the column.  They give mu_a, mu_b, E_aa, E_bb, E_ab.
 *     moments   va = E_aa - mu_a * mu_a   vb = E_bb - mu_b * mu_b   cab = E_ab - mu_a * mu_b
 *     constants k1 = 0.01 * (double)peak, C1 = k1 * k1, k2 = 0.03 * (double)peak, C2 = k2 * k2
 *     channel   ssim_c = (((2.0 * mu_a) * mu_b + C1) * (2.0 * cab + C2)) / (((mu_a * mu_a + mu_b * mu_b) + C1) * ((va + vb) + C2))
 *     pixel     SSIM_p = (ssim_0 + ssim_1) + ssim_2
 * A window exists at a pixel with 5 <= x < w - 5 and 5 <= y < h - 5 whose 11 x 11 neighbourhood holds no bad pixel; n_ssim_windows
 * counts them.  Every other pixel contributes +0.0.  For test == ref the parenthesisation gives ssim_c == 1.0 exactly: va == vb == cab
 * and mu_a == mu_b bit for bit, so numerator and denominator are the same two products.
 *
 * Order of the sums.  Pixels are grouped in 16 x 16 tiles over [0, w) x [0, h), row-major, the edge tiles clipped: the tile numbering of
 * ftn_film_tile_count for a film of that size, so tile t here is tile t of ftn_render_adaptive.  A tile's 256 slots are ly * 16 + lx; a
 * slot with no pixel or with a bad pixel (for SSIM: without a window) holds +0.0.  A tile's sum is the pairwise sum S[0, 256) with
 * S[lo, lo + n) = S[lo, lo + n / 2) + S[lo + n / 2, lo + n) and S of one slot the slot.  The image's sum is the same pairwise sum over
 * the tile sums, padded with +0.0 to the next power of two.  Eight quantities are summed this way, in this order wherever eight stand
 * together: SE, AE, REL, SM, SE_r, SE_g, SE_b, SSIM (the last +0.0 without the flag).  The counts are integers.  No floating-point
 * atomics: nothing depends on the launch geometry or on the host's thread count, and the device and the twin give the same bits.
 *
 * Results (ftn_metrics_resolve; the device path and the twin share it), with n = n_pixels - n_nonfinite and P = (double)peak:
 *     mse = SE / (3 n)   rmse = sqrt(mse)   mae = AE / (3 n)   rel_mse = REL / (3 n)   smape = SM / (3 n)   mse_rgb[c] = SE_c / n
 *     psnr = +inf when mse == 0, else 10 * log10(P * P / mse)          ssim = SSIM / (3 n_ssim_windows)
 * with 3 n formed as 3.0 * (double)n.  A mean over nothing is NaN: every mean and psnr and max_abs when n == 0, ssim without a window
 * (always without the flag).
 *
 * Optional outputs (a null pointer leaves one out): err_map[p] = (float)(SE_p / 3.0), NaN (0x7fc00000) at a bad pixel;
 * ssim_map[p] = (float)(SSIM_p / 3.0), NaN (0x7fc00000) where there is no window; tile_sums[8 t + q], the tile sums, n_tiles x 8 binary64
 * with n_tiles = ceil(w / 16) * ceil(h / 16).
 *
 * Workspace (ftn_metrics_device).  One 88-byte record per tile (the eight sums, the largest difference and its pixel, three counts), and
 * one per block of 256 records of each further level of the total's tree: with n_0 = n_tiles and n_{k+1} = ceil(n_k / 256) while
 * n_k > 256,  bytes = 16 * ceil(88 * (n_0 + n_1 + ...) / 16).  The flags do not change it.
 *
 * Refusals: FTN_ERR_INVALID_ARGUMENT with a message in ftn_last_error(), in this order, each reached only when everything before it is in
 * order: (1) a null test, ref, params or result (the totals for ftn_metrics_device; bytes for ftn_metrics_workspace_size; the totals or
 * the params for ftn_metrics_resolve); (2) w <= 0, h <= 0 or w * h >= 2^31; (3) unknown flag bits; (4) reserved != 0; (5) peak or rel_eps
 * not finite or not above 0; (6) FTN_METRICS_SSIM with w < 11 or h < 11; (7) an ssim_map without FTN_METRICS_SSIM; (8) on the device path
 * a null workspace (its size is never 0), then an output (totals, err_map, ssim_map, tile_sums, workspace) overlapping an input or
 * another output, then test, ref or an output not 16-byte aligned.  Then the entries that run on the GPU return FTN_ERR_NO_DEVICE when
 * there is none: there is no CPU fallback.  ftn_metrics_workspace_size stops after (3).  A refused call writes nothing.
 */
#ifndef FOUNTAIN_HIP_METRICS_H
#define FOUNTAIN_HIP_METRICS_H

#include "fountain_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FTN_METRICS_SSIM 1u             /* ftn_metrics_params.flags: compute SSIM as well                                                  */
#define FTN_METRICS_TILE 16             /* the side of a tile                                                                              */
#define FTN_METRICS_SUMS 8              /* SE, AE, REL, SM, SE_r, SE_g, SE_b, SSIM                                                         */
#define FTN_METRICS_SSIM_TAPS 11

typedef struct ftn_metrics_params {     /* 16 bytes                                                                                       */
    uint32_t flags;                     /* FTN_METRICS_SSIM                                                                               */
    float peak;                         /* > 0: the signal's peak, for PSNR and the SSIM constants                                        */
    float rel_eps;                      /* > 0: eps of rel_c and sm_c                                                                     */
    uint32_t reserved;                  /* 0                                                                                              */
} ftn_metrics_params;

typedef struct ftn_metrics_totals {     /* 112 bytes: what the device writes                                                              */
    double sum[FTN_METRICS_SUMS];       /* SE, AE, REL, SM, SE_r, SE_g, SE_b, SSIM                                                        */
    double max_abs;
    uint64_t max_abs_index;
    uint64_t n_pixels;                  /* w * h                                                                                          */
    uint64_t n_nonfinite;
    uint64_t n_different;
    uint64_t n_ssim_windows;
} ftn_metrics_totals;

typedef struct ftn_metrics_result {     /* 136 bytes                                                                                      */
    double mse, rmse, mae, rel_mse, smape, psnr, ssim;
    double mse_rgb[3];
    double max_abs;
    uint64_t max_abs_index;
    uint64_t n_pixels;
    uint64_t n;                         /* n_pixels - n_nonfinite                                                                         */
    uint64_t n_nonfinite;
    uint64_t n_different;
    uint64_t n_ssim_windows;
} ftn_metrics_result;

/* flags 0, peak 1, rel_eps 1e-2.  A null pointer is ignored. */
void ftn_metrics_params_default(ftn_metrics_params* p);

/* bytes of device workspace ftn_metrics_device needs for a w x h image (the formula above). */
int ftn_metrics_workspace_size(int32_t w, int32_t h, uint32_t flags, size_t* bytes);
/* the normalised weights g_0 .. g_10 of the SSIM window, as the kernels and the twin use them. */
int ftn_metrics_ssim_weights(double g[FTN_METRICS_SSIM_TAPS]);

/* HOST buffers; uploads, runs on GPU `device` (-1 = the current one), downloads and resolves.  totals, err_map, ssim_map and tile_sums
 * are optional. */
int ftn_metrics(const float* test, const float* ref, int32_t w, int32_t h, const ftn_metrics_params* params, ftn_metrics_result* result,
                ftn_metrics_totals* totals, float* err_map, float* ssim_map, double* tile_sums, int32_t device);
/* DEVICE buffers on `stream` (a hipStream_t; NULL = the default stream).  Allocates nothing, never synchronises and launches kernels
 * only, so it can be captured in a graph.  totals is an ftn_metrics_totals in device memory; err_map, ssim_map and tile_sums are optional. */
int ftn_metrics_device(const void* test, const void* ref, int32_t w, int32_t h, const ftn_metrics_params* params, void* totals,
                       void* err_map, void* ssim_map, void* tile_sums, void* workspace, void* stream);
/* host only: the results of the header from the totals.  peak is the only parameter read; refused: a null pointer, a peak that is not
 * finite or not above 0, totals that count more bad pixels than pixels. */
int ftn_metrics_resolve(const ftn_metrics_totals* totals, const ftn_metrics_params* params, ftn_metrics_result* result);
/* the host twin: the same bits, on the host's threads, whatever their number; shares the per-element code with the kernels. */
int ftn_metrics_cpu(const float* test, const float* ref, int32_t w, int32_t h, const ftn_metrics_params* params, ftn_metrics_result* result,
                    ftn_metrics_totals* totals, float* err_map, float* ssim_map, double* tile_sums);

#define FTN_METRICS_ABI_VERSION 1
int ftn_metrics_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* FOUNTAIN_HIP_METRICS_H */
