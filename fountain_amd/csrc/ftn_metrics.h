/*
 * ftn_metrics.h -- the measuring stage of include/fountain_hip_metrics.h: the per-element code (the pointwise terms of a pixel, the two
 * passes of the SSIM window over the five planes, the SSIM of a channel), shared by the kernels (ftn_metrics.hip) and the host twin
 * (ftn_metrics_host.cpp) so that both give the same bits, the record a tile leaves, the workspace's plan and the device driver's
 * declaration.  All of it is binary64 and built with -ffp-contract=off: each line below is the header's expression, operation by operation.
 */
#ifndef FTN_METRICS_H
#define FTN_METRICS_H
#include <hip/hip_runtime.h>
#include "ftn_math.h"
#include "../../include/fountain_hip_metrics.h"

namespace ftn {

constexpr int kMetricsTile = FTN_METRICS_TILE, kMetricsTaps = FTN_METRICS_SSIM_TAPS, kMetricsRadius = kMetricsTaps / 2;
constexpr int kMetricsHalo = kMetricsTile + 2 * kMetricsRadius;            /* 26: a tile and the windows' reach around it */
constexpr int kMetricsSlots = kMetricsTile * kMetricsTile;                  /* 256 */

/* what an element reads: the parameters as binary64, what follows from them once per call, and the image's and the tiling's sizes */
struct MetricsCall { double eps, C1, C2, g[kMetricsTaps]; int32_t w, h; uint32_t tiles_x, n_tiles; };

/* what a tile, or a block of 256 records of the total's tree, leaves in the workspace: the eight sums, the largest |d| and the smallest
 * pixel that attains it (max_abs -1 where no pixel is good), the three counts */
struct MetricsRec { double sum[FTN_METRICS_SUMS]; double max_abs; uint32_t max_index, n_nonfinite, n_different, n_windows; };
static_assert(sizeof(MetricsRec) == 88, "the workspace formula of the header");

FTN_HD bool metrics_finite(float v) { return (f2u(v) & 0x7f800000u) != 0x7f800000u; }

/* the pointwise terms of one pixel */
struct MetricsPoint { double se[3], SE, AE, REL, SM, max_ae; bool bad, different; };

FTN_HD MetricsPoint metrics_point(float a0, float a1, float a2, float b0, float b1, float b2, double eps) {
    MetricsPoint o;
    const float ta[3] = {a0, a1, a2}, tb[3] = {b0, b1, b2};
    o.bad = false; o.different = false;
    double ae[3], rel[3], sm[3];
#pragma unroll
    for (int c = 0; c < 3; c++) {
        if (!metrics_finite(ta[c]) || !metrics_finite(tb[c])) o.bad = true;
        if (f2u(ta[c]) != f2u(tb[c])) o.different = true;
        const double a = (double)ta[c], b = (double)tb[c], d = a - b;
        o.se[c] = d * d;
        ae[c] = __builtin_fabs(d);
        rel[c] = o.se[c] / (b * b + eps);
        sm[c] = ae[c] / ((__builtin_fabs(a) + __builtin_fabs(b)) + eps);
    }
    o.SE = (o.se[0] + o.se[1]) + o.se[2];
    o.AE = (ae[0] + ae[1]) + ae[2];
    o.REL = (rel[0] + rel[1]) + rel[2];
    o.SM = (sm[0] + sm[1]) + sm[2];
    o.max_ae = ae[0] > ae[1] ? ae[0] : ae[1];
    o.max_ae = ae[2] > o.max_ae ? ae[2] : o.max_ae;
    return o;
}

/* the five planes of a channel at one place: a, b, a a, b b, a b, or their weighted sums */
struct Ssim5 { double a, b, aa, bb, ab; };

/* the horizontal pass: tap(k, &a, &b) gives the channel's two binary32 values at column x + k - 5 */
template <class Tap> FTN_HD Ssim5 metrics_hpass(const double (&g)[kMetricsTaps], Tap tap) {
    Ssim5 acc = {0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int k = 0; k < kMetricsTaps; k++) {
        float fa, fb;
        tap(k, &fa, &fb);
        const double a = (double)fa, b = (double)fb;
        acc.a = acc.a + g[k] * a;
        acc.b = acc.b + g[k] * b;
        acc.aa = acc.aa + g[k] * (a * a);
        acc.bb = acc.bb + g[k] * (b * b);
        acc.ab = acc.ab + g[k] * (a * b);
    }
    return acc;
}

/* the vertical pass: tap(k) gives the horizontal pass's result at row y + k - 5 */
template <class Tap> FTN_HD Ssim5 metrics_vpass(const double (&g)[kMetricsTaps], Tap tap) {
    Ssim5 acc = {0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int k = 0; k < kMetricsTaps; k++) {
        const Ssim5 v = tap(k);
        acc.a = acc.a + g[k] * v.a;
        acc.b = acc.b + g[k] * v.b;
        acc.aa = acc.aa + g[k] * v.aa;
        acc.bb = acc.bb + g[k] * v.bb;
        acc.ab = acc.ab + g[k] * v.ab;
    }
    return acc;
}

/* ssim_c from the window's five moments */
FTN_HD double metrics_ssim(Ssim5 m, double C1, double C2) {
    const double va = m.aa - m.a * m.a, vb = m.bb - m.b * m.b, cab = m.ab - m.a * m.b;
    return (((2.0 * m.a) * m.b + C1) * (2.0 * cab + C2)) / (((m.a * m.a + m.b * m.b) + C1) * ((va + vb) + C2));
}

/* does (om, oi) beat (m, i): the larger value, then the smaller pixel */
FTN_HD bool metrics_max_beats(double om, uint32_t oi, double m, uint32_t i) { return om > m || (om == m && oi < i); }

/* the records of the workspace: level 0 has one per tile; level k + 1 one per 256 of level k, while a level has more than 256 */
inline size_t metrics_records(size_t n_tiles) {
    size_t total = n_tiles;
    for (size_t n = n_tiles; n > 256;) { n = (n + 255) / 256; total += n; }
    return total;
}
inline size_t metrics_workspace_bytes(size_t n_tiles) { return (metrics_records(n_tiles) * sizeof(MetricsRec) + 15) / 16 * 16; }

/* ftn_metrics.hip: the tile kernel and the total's tree on `stream` */
hipError_t launch_metrics(const float* test, const float* ref, const MetricsCall& e, bool ssim, ftn_metrics_totals* totals, float* err_map, float* ssim_map,
                          double* tile_sums, MetricsRec* workspace, hipStream_t stream);

}  // namespace ftn
#endif
