/*
 * ftn_bloom.h -- the bloom stage of include/fountain_hip_bloom.h: the per-pixel code (prefilter, the 4 x 4 down-sampling sum, the 2 x 2
 * tent, the blend and the composite), shared by the kernels (ftn_bloom.hip) and the host twin (ftn_bloom_host.cpp) so that both give the
 * same bits, the pyramid's plan, and the device driver's declaration.  Small structs and floats go by value.
 */
#ifndef FTN_BLOOM_H
#define FTN_BLOOM_H
#include <hip/hip_runtime.h>
#include "ftn_math.h"
#include "../../include/fountain_hip_bloom.h"

namespace ftn {

struct Bloom3 { float r, g, b; };
/* a tap of the first down step: the prefiltered pixel and, with FTN_BLOOM_KARIS, k = 1 / (1 + Y) */
struct BloomTap { float r, g, b, k; };

/* what a pixel reads: the parameters and what follows from them once per call (each a binary32 operation of the header) */
struct BloomCall { float strength, scatter, keep, threshold, knee_k, clamp_max; uint32_t flags; };

FTN_HD BloomCall bloom_make(const ftn_bloom_params& p) {
    BloomCall e;
    e.strength = p.strength; e.scatter = p.scatter; e.keep = 1.0f - p.scatter;
    e.threshold = p.threshold; e.knee_k = p.knee * p.threshold; e.clamp_max = p.clamp_max; e.flags = p.flags;
    return e;
}

FTN_HD float bloom_luminance(float r, float g, float b) { return Rgb(r, g, b).luminance(); }
FTN_HD float bloom_sanitise(float c, float clamp_max) { return !(c > 0.0f) ? 0.0f : (c > clamp_max ? clamp_max : c); }

/* step 1 of the header */
FTN_HD Bloom3 bloom_pre(float r, float g, float b, BloomCall e) {
    Bloom3 s = {bloom_sanitise(r, e.clamp_max), bloom_sanitise(g, e.clamp_max), bloom_sanitise(b, e.clamp_max)};
    if (e.threshold == 0.0f) return s;
    const float Y = bloom_luminance(s.r, s.g, s.b), K = e.knee_k;
    float gain = 0.0f;
    if (Y >= e.threshold + K) gain = Y - e.threshold;
    else if (Y > e.threshold - K && K > 0.0f) { const float t = (Y - e.threshold) + K; gain = (t * t) / (4.0f * K); }
    if (gain == 0.0f) { s.r = 0.0f; s.g = 0.0f; s.b = 0.0f; return s; }
    const float q = gain / Y;
    s.r = s.r * q; s.g = s.g * q; s.b = s.b * q;
    return s;
}

FTN_HD float bloom_karis_k(float r, float g, float b) { return 1.0f / (1.0f + bloom_luminance(r, g, b)); }

/* step 2: tap(i, j) gives the BloomTap of column 2x - 1 + i and row 2y - 1 + j, clamped by the caller */
template <bool KARIS, class Tap> FTN_HD Bloom3 bloom_down_pixel(Tap tap) {
    float ar = 0.0f, ag = 0.0f, ab = 0.0f, aq = 0.0f;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const float kj = (j == 0 || j == 3) ? 0.125f : 0.375f;
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const float ki = (i == 0 || i == 3) ? 0.125f : 0.375f;
            const BloomTap t = tap(i, j);
            float q = kj * ki;
            if (KARIS) { q = q * t.k; aq += q; }
            ar += q * t.r; ag += q * t.g; ab += q * t.b;
        }
    }
    if (KARIS) { ar = ar / aq; ag = ag / aq; ab = ab / aq; }
    return Bloom3{ar, ag, ab};
}

FTN_HD int bloom_clampi(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

/* step 3: up(C)(x, y) of a coarse level of wc x hc pixels; tap(i, j, cx, cy) gives its pixel (cx, cy), the tent's column i and row j */
template <class Tap> FTN_HD Bloom3 bloom_up_pixel(int x, int y, int wc, int hc, Tap tap) {
    const int x0 = (x - 1) >> 1, y0 = (y - 1) >> 1;
    const int cx[2] = {bloom_clampi(x0, wc - 1), bloom_clampi(x0 + 1, wc - 1)}, cy[2] = {bloom_clampi(y0, hc - 1), bloom_clampi(y0 + 1, hc - 1)};
    const float fx[2] = {(x & 1) ? 0.75f : 0.25f, (x & 1) ? 0.25f : 0.75f}, fy[2] = {(y & 1) ? 0.75f : 0.25f, (y & 1) ? 0.25f : 0.75f};
    float ar = 0.0f, ag = 0.0f, ab = 0.0f;
#pragma unroll
    for (int j = 0; j < 2; j++) {
#pragma unroll
        for (int i = 0; i < 2; i++) {
            const Bloom3 t = tap(i, j, cx[i], cy[j]);
            const float q = fy[j] * fx[i];
            ar += q * t.r; ag += q * t.g; ab += q * t.b;
        }
    }
    return Bloom3{ar, ag, ab};
}

FTN_HD float bloom_blend(float d, float u, BloomCall e) { return d * e.keep + u * e.scatter; }

/* step 4, one channel */
FTN_HD float bloom_composite(float c, float B, float P, BloomCall e) {
    const bool finite = (f2u(c) & 0x7f800000u) != 0x7f800000u;
    return (finite && !(c < 0.0f)) ? c + e.strength * (B - P) : c;
}

/* the pyramid: L and the sizes and workspace offsets (in floats) of levels 0..L; level 0 has no buffer */
struct BloomPlan { int L; int w[FTN_BLOOM_MAX_LEVELS + 1], h[FTN_BLOOM_MAX_LEVELS + 1]; size_t off[FTN_BLOOM_MAX_LEVELS + 1]; size_t floats; };

inline BloomPlan bloom_plan(int w, int h, int levels) {
    BloomPlan p;
    p.L = 0; p.w[0] = w; p.h[0] = h; p.off[0] = 0; p.floats = 0;
    while (p.L < levels && (p.w[p.L] > 1 || p.h[p.L] > 1)) {
        const int k = ++p.L;
        p.w[k] = (p.w[k - 1] + 1) >> 1; p.h[k] = (p.h[k - 1] + 1) >> 1;
        p.off[k] = p.floats;
        p.floats += (3 * (size_t)p.w[k] * (size_t)p.h[k] + 3) / 4 * 4;          /* 16 bytes = 4 floats */
    }
    return p;
}

/* the down kernel's tile of outputs, one per thread */
#define FTN_BLOOM_TILE_X 32
#define FTN_BLOOM_TILE_Y 8

/* ftn_bloom.hip: the whole chain on `stream`; `copy` = the exact copy of the header's step 4 */
hipError_t launch_bloom(const float* rgb, const BloomPlan& plan, const BloomCall& e, bool copy, float* out_rgb, float* workspace, hipStream_t stream);

}  // namespace ftn
#endif
