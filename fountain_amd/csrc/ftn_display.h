/*
 * ftn_display.h -- the display stage of include/fountain_hip_display.h: the per-pixel code (luminance bin, tone curve, transfer,
 * quantisation and dither), shared by the kernels (ftn_display.hip) and the host twin (ftn_display_host.cpp) so that both give the
 * same bits, and the device drivers' declarations.
 */
#ifndef FTN_DISPLAY_H
#define FTN_DISPLAY_H
#include <hip/hip_runtime.h>
#include "ftn_math.h"
#include "../../include/fountain_hip_display.h"

namespace ftn {

/* what a pixel's encode reads: the parameters and what follows from them once per call (each a binary32 operation of the header) */
struct DispEncode { float scale; uint32_t tonemap, transfer, flags; float white2, inv_gamma, hable_white; };

FTN_HD float disp_luminance(float r, float g, float b) { return Rgb(r, g, b).luminance(); }

/* the histogram word of a luminance: the float's bits alone, no logarithm */
FTN_HD uint32_t disp_bin(float Y) {
    if (!(Y >= 0.0f)) return FTN_DISPLAY_HIST_INVALID;
    if (Y < 0x1p-24f) return FTN_DISPLAY_HIST_BELOW;
    if (Y >= 0x1p24f) return FTN_DISPLAY_HIST_ABOVE;
    return (f2u(Y) >> 20) - 824u;
}

FTN_HD float disp_clamp01(float v) { return !(v > 0.0f) ? 0.0f : (v > 1.0f ? 1.0f : v); }
FTN_HD float disp_sanitise(float c) { return !(c > 0.0f) ? 0.0f : (c > 65504.0f ? 65504.0f : c); }

FTN_HD float disp_hable_f(float x) {
    const float A = 0.15f, B = 0.50f, C = 0.10f, D = 0.20f, E = 0.02f, F = 0.30f;
    return (x * (A * x + C * B) + D * E) / (x * (A * x + B) + D * F) - (D * E) / (D * F);
}
FTN_HD float disp_aces(float x) { return (x * (2.51f * x + 0.03f)) / (x * (2.43f * x + 0.59f) + 0.14f); }

FTN_HD DispEncode disp_make(const ftn_display_params& p, float scale) {
    DispEncode e;
    e.scale = scale; e.tonemap = p.tonemap; e.transfer = p.transfer; e.flags = p.flags;
    e.white2 = p.white * p.white;
    e.inv_gamma = 1.0f / p.gamma;
    e.hable_white = disp_hable_f(p.white);
    return e;
}

FTN_HD float disp_transfer(float v, DispEncode e) {
    if (e.transfer == FTN_DISPLAY_TRANSFER_SRGB) return v <= 0.0031308f ? 12.92f * v : 1.055f * ftn_det::powf_det(v, (float)(1.0 / 2.4)) - 0.055f;
    if (e.transfer == FTN_DISPLAY_TRANSFER_GAMMA) return ftn_det::powf_det(v, e.inv_gamma);
    return v;
}

/* B[y & 7][x & 7] of the header's matrix: the bits of y and x ^ y interleaved, most significant first into the lowest places */
FTN_HD uint32_t disp_bayer(uint32_t x, uint32_t y) {
    const uint32_t q = x ^ y;
    uint32_t v = 0;
    for (int p = 0; p < 3; p++) v |= (((y >> (2 - p)) & 1u) << (2 * p)) | (((q >> (2 - p)) & 1u) << (2 * p + 1));
    return v;
}

FTN_HD uint32_t disp_code(float v, float d) {
    const float c = floorf((v * 255.0f + 0.5f) + d);
    return c < 0.0f ? 0u : (c > 255.0f ? 255u : (uint32_t)c);
}

/* steps 1 to 4 of the header for pixel (x, y): the three display-referred values into o, the packed word returned */
FTN_HD uint32_t disp_pixel(float r, float g, float b, uint32_t x, uint32_t y, DispEncode e, float* o) {
    r = disp_sanitise(r * e.scale); g = disp_sanitise(g * e.scale); b = disp_sanitise(b * e.scale);
    if (e.tonemap == FTN_DISPLAY_TONEMAP_REINHARD) {
        const float L = disp_luminance(r, g, b);
        if (L != 0.0f) {
            const float Lp = (L * (1.0f + L / e.white2)) / (1.0f + L), s = Lp / L;
            r = r * s; g = g * s; b = b * s;
        }
    } else if (e.tonemap == FTN_DISPLAY_TONEMAP_ACES) {
        r = disp_aces(r); g = disp_aces(g); b = disp_aces(b);
    } else if (e.tonemap == FTN_DISPLAY_TONEMAP_HABLE) {
        r = disp_hable_f(r) / e.hable_white; g = disp_hable_f(g) / e.hable_white; b = disp_hable_f(b) / e.hable_white;
    }
    r = disp_clamp01(disp_transfer(disp_clamp01(r), e));
    g = disp_clamp01(disp_transfer(disp_clamp01(g), e));
    b = disp_clamp01(disp_transfer(disp_clamp01(b), e));
    o[0] = r; o[1] = g; o[2] = b;
    const float d = (e.flags & FTN_DISPLAY_DITHER) ? ((float)disp_bayer(x & 7u, y & 7u) + 0.5f) / 64.0f - 0.5f : 0.0f;
    return disp_code(r, d) | (disp_code(g, d) << 8) | (disp_code(b, d) << 16) | 0xff000000u;
}

/* the grids' caps, in 256-thread workgroups; every thread takes four pixels per trip of its grid-stride loop */
#define FTN_DISPLAY_ENCODE_MAX_BLOCKS 2048u
#define FTN_DISPLAY_HIST_MAX_BLOCKS 1024u

/* ftn_display.hip: n = w * h pixels; hist is cleared on the stream first */
hipError_t launch_display_histogram(const float* rgb, uint32_t n, uint32_t* hist, hipStream_t stream);
hipError_t launch_display_encode(const float* rgb, uint32_t w, uint32_t n, const DispEncode& e, float* out_rgb, uint32_t* out_rgba8, hipStream_t stream);

}  // namespace ftn
#endif
