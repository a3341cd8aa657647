/*
 * ftn_denoise.h -- the edge-avoiding a-trous filter of include/fountain_hip_denoise.h: the per-pixel math, shared by the kernels
 * (ftn_denoise.hip) and the host twin (ftn_denoise_host.cpp) so that both give the same bits, and the device driver's declaration.
 *
 * Buffers, one entry per pixel: colour float4 {u, m} (two, ping-pong), features float4 {n, c} and float4 {x, z}.  The variance-guided
 * filter of include/fountain_hip_denoise_guided.h keeps {u, nu} in the colour buffers instead, and its per-pixel code (dn_guided_*) sits
 * beside the unguided filter's, reusing its prepare, finish and tests.
 */
#ifndef FTN_DENOISE_H
#define FTN_DENOISE_H
#include <hip/hip_runtime.h>
#include "detmath.h"
#include "../../include/fountain_hip_denoise.h"
#include "../../include/fountain_hip_denoise_guided.h"

namespace ftn {

/* the constants of one level: step 2^i, Dc = kc |du|^2 / ((m_p^2 + m_q^2) / 2 + color_eps) with kc = 2^i / sigma_color^2,
 * Dn = kn |dn|^2 with kn = 1 / sigma_normal^2, Dp = (n_p . dx)^2 kp / max(z_p, 1e-6)^2 with kp = 1 / sigma_plane^2 */
struct DnLevel { int step; float kc, kn, kp, color_eps; };

FTN_HD DnLevel dn_level(const ftn_denoise_params& p, int i) {
    DnLevel L;
    L.step = 1 << i;
    L.kc = (float)L.step / (p.sigma_color * p.sigma_color);
    L.kn = 1.0f / (p.sigma_normal * p.sigma_normal);
    L.kp = 1.0f / (p.sigma_plane * p.sigma_plane);
    L.color_eps = p.color_eps;
    return L;
}

FTN_HD bool dn_finite(float v) { return (ftn_det::f2u(v) & 0x7f800000u) != 0x7f800000u; }
FTN_HD bool dn_finite3(float4 u) { return dn_finite(u.x) && dn_finite(u.y) && dn_finite(u.z); }
FTN_HD float dn_mean(float r, float g, float b) { return (r + g + b) / 3.0f; }
FTN_HD float dn_divisor(float a, float eps) { return a > eps ? a : eps; }

/* step 1 for one pixel: rgb (3 floats) and gb (12 floats) -> colour {u, m}, features {n, c}, {x, z} */
FTN_HD void dn_prepare_pixel(const float* rgb, const float* gb, uint32_t flags, float albedo_eps, float4* col, float4* fnc, float4* fxz) {
    float r = rgb[0], g = rgb[1], b = rgb[2];
    const float c = gb[10];
    if ((flags & FTN_DENOISE_DEMODULATE) && c > 0.0f) {
        r = r / dn_divisor(gb[0], albedo_eps); g = g / dn_divisor(gb[1], albedo_eps); b = b / dn_divisor(gb[2], albedo_eps);
    }
    *col = make_float4(r, g, b, dn_mean(r, g, b));
    *fnc = make_float4(gb[3], gb[4], gb[5], c);
    *fxz = make_float4(gb[6], gb[7], gb[8], gb[9]);
}

/* one level for pixel (x, y): the 25 taps in row-major order, one weight and one exp each; returns {u', m'} */
FTN_HD float4 dn_atrous_pixel(const float4* col, const float4* fnc, const float4* fxz, int w, int h, int x, int y, const DnLevel& L) {
    const int p = y * w + x;
    const float4 up = col[p];
    if (!dn_finite3(up)) return up;
    const float4 np = fnc[p], xp = fxz[p];
    const bool cov_p = np.w > 0.0f;
    const float mp2 = up.w * up.w;
    const float zc = xp.w > 1e-6f ? xp.w : 1e-6f;
    const float kpz = L.kp / (zc * zc);
    const float K[5] = {1.0f / 16.0f, 1.0f / 4.0f, 3.0f / 8.0f, 1.0f / 4.0f, 1.0f / 16.0f};
    float ws = 0.0f, sr = 0.0f, sg = 0.0f, sb = 0.0f;
#pragma unroll
    for (int j = 0; j < 5; j++) {
        const int qy = y + (j - 2) * L.step;
        if (qy < 0 || qy >= h) continue;
#pragma unroll
        for (int i = 0; i < 5; i++) {
            const int qx = x + (i - 2) * L.step;
            if (qx < 0 || qx >= w) continue;
            const int q = qy * w + qx;
            const float4 nq = fnc[q];
            if ((nq.w > 0.0f) != cov_p) continue;
            const float4 uq = col[q];
            if (!dn_finite3(uq)) continue;
            const float4 xq = fxz[q];
            const float dr = up.x - uq.x, dg = up.y - uq.y, db = up.z - uq.z;
            const float dc = L.kc * (dr * dr + dg * dg + db * db) / ((mp2 + uq.w * uq.w) * 0.5f + L.color_eps);
            const float e0 = np.x - nq.x, e1 = np.y - nq.y, e2 = np.z - nq.z;
            const float dn = L.kn * (e0 * e0 + e1 * e1 + e2 * e2);
            const float pd = np.x * (xp.x - xq.x) + np.y * (xp.y - xq.y) + np.z * (xp.z - xq.z);
            const float dp = pd * pd * kpz;
            const float t = dc + dn + dp;
            /* exp(-t) rounds to binary32 zero beyond 104 (it is below half the least subnormal); NaN (non-finite features) counts as 0 */
            if (!(t <= 104.0f)) continue;
            const float om = (float)ftn_det::kexp(-(double)t);
            const float wt = (K[j] * K[i]) * om;
            ws = ws + wt;
            sr = sr + wt * uq.x; sg = sg + wt * uq.y; sb = sb + wt * uq.z;
        }
    }
    if (!(ws > 0.0f)) return up;          /* only with non-finite features of p itself: the centre tap has weight 9/64 otherwise */
    const float r = sr / ws, g = sg / ws, b = sb / ws;
    return make_float4(r, g, b, dn_mean(r, g, b));
}

/* step 3 for one pixel: {u, m} -> 3 floats */
FTN_HD void dn_finish_pixel(float4 u, const float* gb, uint32_t flags, float albedo_eps, float* out) {
    if ((flags & FTN_DENOISE_DEMODULATE) && gb[10] > 0.0f) {
        out[0] = u.x * dn_divisor(gb[0], albedo_eps); out[1] = u.y * dn_divisor(gb[1], albedo_eps); out[2] = u.z * dn_divisor(gb[2], albedo_eps);
    } else {
        out[0] = u.x; out[1] = u.y; out[2] = u.z;
    }
}

/* ---- the variance-guided filter (include/fountain_hip_denoise_guided.h) ---- */

/* the constants of one guided level: step 2^i, Dc = |du|^2 / (kv nuh_p + rel_eps m_p^2) with kv = 2 sigma_variance^2, kn and kp as
 * DnLevel's */
struct DnGuidedLevel { int step; float kv, rel_eps, kn, kp; };

FTN_HD DnGuidedLevel dn_guided_level(const ftn_denoise_guided_params& p, int i) {
    DnGuidedLevel L;
    L.step = 1 << i;
    L.kv = 2.0f * (p.sigma_variance * p.sigma_variance);
    L.rel_eps = p.rel_eps;
    L.kn = 1.0f / (p.sigma_normal * p.sigma_normal);
    L.kp = 1.0f / (p.sigma_plane * p.sigma_plane);
    return L;
}

/* a colour {u, nu} the guided filter reads and changes: finite u and a variance that is not NaN (+inf, unknown, is usable) */
FTN_HD bool dn_guided_usable(float4 c) { return dn_finite3(c) && c.w == c.w; }

/* step 1 for one pixel: dn_prepare_pixel, then nu = sum var_c / d_c^2 (r, g, b in that order) in the place of m; NaN when a variance is
 * NaN or negative */
FTN_HD void dn_guided_prepare_pixel(const float* rgb, const float* gb, const float* var, uint32_t flags, float albedo_eps, float4* col, float4* fnc,
                                    float4* fxz) {
    float4 c;
    dn_prepare_pixel(rgb, gb, flags, albedo_eps, &c, fnc, fxz);
    float nu;
    if (!(var[0] >= 0.0f) || !(var[1] >= 0.0f) || !(var[2] >= 0.0f)) {
        nu = ftn_det::u2f(0x7fc00000u);
    } else if ((flags & FTN_DENOISE_DEMODULATE) && gb[10] > 0.0f) {
        const float dr = dn_divisor(gb[0], albedo_eps), dg = dn_divisor(gb[1], albedo_eps), db = dn_divisor(gb[2], albedo_eps);
        nu = (var[0] / (dr * dr) + var[1] / (dg * dg)) + var[2] / (db * db);
    } else {
        nu = (var[0] + var[1]) + var[2];
    }
    c.w = nu;
    *col = c;
}

/* one guided level for pixel (x, y): the 3 x 3 prefilter of nu, then the 25 taps in row-major order; returns {u', nu'} */
FTN_HD float4 dn_atrous_pixel(const float4* col, const float4* fnc, const float4* fxz, int w, int h, int x, int y, const DnGuidedLevel& L) {
    const int p = y * w + x;
    const float4 up = col[p];
    if (!dn_guided_usable(up)) return up;
    const float4 np = fnc[p], xp = fxz[p];
    const bool cov_p = np.w > 0.0f;
    const float K3[3] = {0.25f, 0.5f, 0.25f};
    float sv = 0.0f, sk = 0.0f;
#pragma unroll
    for (int j = 0; j < 3; j++) {
        const int qy = y + j - 1;
        if (qy < 0 || qy >= h) continue;
#pragma unroll
        for (int i = 0; i < 3; i++) {
            const int qx = x + i - 1;
            if (qx < 0 || qx >= w) continue;
            const int q = qy * w + qx;
            if ((fnc[q].w > 0.0f) != cov_p) continue;
            const float4 cq = col[q];
            if (!dn_guided_usable(cq)) continue;
            const float k = K3[j] * K3[i];
            sv = sv + k * cq.w;
            sk = sk + k;
        }
    }
    const float nuh = sv / sk;                       /* sk >= 1/4: p itself counts */
    const bool nuh_inf = !dn_finite(nuh);
    const float mp = dn_mean(up.x, up.y, up.z);
    const float den = L.kv * nuh + L.rel_eps * (mp * mp);
    const float zc = xp.w > 1e-6f ? xp.w : 1e-6f;
    const float kpz = L.kp / (zc * zc);
    const float K[5] = {1.0f / 16.0f, 1.0f / 4.0f, 3.0f / 8.0f, 1.0f / 4.0f, 1.0f / 16.0f};
    float ws = 0.0f, sr = 0.0f, sg = 0.0f, sb = 0.0f, snu = 0.0f;
#pragma unroll
    for (int j = 0; j < 5; j++) {
        const int qy = y + (j - 2) * L.step;
        if (qy < 0 || qy >= h) continue;
#pragma unroll
        for (int i = 0; i < 5; i++) {
            const int qx = x + (i - 2) * L.step;
            if (qx < 0 || qx >= w) continue;
            const int q = qy * w + qx;
            const float4 nq = fnc[q];
            if ((nq.w > 0.0f) != cov_p) continue;
            const float4 uq = col[q];
            if (!dn_guided_usable(uq)) continue;
            const float4 xq = fxz[q];
            const float dr = up.x - uq.x, dg = up.y - uq.y, db = up.z - uq.z;
            const float d2 = dr * dr + dg * dg + db * db;
            const float dc = (d2 == 0.0f || nuh_inf) ? 0.0f : d2 / den;
            const float e0 = np.x - nq.x, e1 = np.y - nq.y, e2 = np.z - nq.z;
            const float dn = L.kn * (e0 * e0 + e1 * e1 + e2 * e2);
            const float pd = np.x * (xp.x - xq.x) + np.y * (xp.y - xq.y) + np.z * (xp.z - xq.z);
            const float dp = pd * pd * kpz;
            const float t = dc + dn + dp;
            if (!(t <= 104.0f)) continue;
            const float om = (float)ftn_det::kexp(-(double)t);
            const float wt = (K[j] * K[i]) * om;
            if (!(wt > 0.0f)) continue;
            ws = ws + wt;
            sr = sr + wt * uq.x; sg = sg + wt * uq.y; sb = sb + wt * uq.z;
            snu = snu + wt * (wt * uq.w);
        }
    }
    if (!(ws > 0.0f)) return up;
    return make_float4(sr / ws, sg / ws, sb / ws, snu / (ws * ws));
}

/* the device path of ftn_denoise_device (arguments already checked): prepare, levels launches, the last one writing out_rgb; levels
 * == 0 copies rgb.  workspace = 4 float4 per pixel.  Returns the launch error, if any. */
hipError_t launch_denoise(const float* rgb, const float* gb12, int w, int h, const ftn_denoise_params& params, float* out_rgb,
                          float4* workspace, hipStream_t stream);

/* the same for ftn_denoise_guided_device: the colour buffers hold {u, nu} */
hipError_t launch_denoise_guided(const float* rgb, const float* gb12, const float* var4, int w, int h, const ftn_denoise_guided_params& params,
                                 float* out_rgb, float4* workspace, hipStream_t stream);

}  // namespace ftn
#endif
