/*
 * ftn_temporal.h -- temporal reprojection and accumulation (include/fountain_hip_temporal.h): the per-pixel code, shared by the kernel
 * (ftn_temporal.hip) and the host twin (ftn_temporal_host.cpp) so that both give the same bits, and the device driver's declaration.
 * Prepare, finish and the finiteness tests are ftn_denoise.h's.  The same per-pixel code serves include/fountain_hip_motion.h: with a frame's
 * mv8 (its resolved previous positions and normals) steps 2 and 3 follow what moved; tp_motion, step 2, is also the motion vectors'.
 *
 * Buffers, one entry per pixel: history, two float4 {u, n} and {nu_r, nu_g, nu_b, nu_Y} (an ftn_temporal_pixel), read through float4
 * pointers; everything else as the caller's float arrays.
 */
#ifndef FTN_TEMPORAL_H
#define FTN_TEMPORAL_H
#include "ftn_denoise.h"
#include "ftn_math.h"
#include "../../include/fountain_hip_temporal.h"

namespace ftn {

/* the four matrices of one camera the reprojection needs, column-major as ftn_transform's: a kernel argument */
struct TpCamera { float c2w[16], w2c[16], r2c[16], c2r[16]; };

inline TpCamera tp_camera(const ftn_camera_desc& c) {
    TpCamera t;
    for (int i = 0; i < 16; i++) {
        t.c2w[i] = c.camera_to_world.m[i]; t.w2c[i] = c.camera_to_world.inv[i];
        t.r2c[i] = c.raster_to_camera.m[i]; t.c2r[i] = c.raster_to_camera.inv[i];
    }
    return t;
}

/* equal cameras, matrix for matrix: the frame looks at the static scene as the previous one did */
inline bool tp_same_view(const TpCamera& a, const TpCamera& b) {
    for (int i = 0; i < 16; i++)
        if (!(a.c2w[i] == b.c2w[i] && a.w2c[i] == b.w2c[i] && a.r2c[i] == b.r2c[i] && a.c2r[i] == b.c2r[i])) return false;
    return true;
}

/* what a launch or a host pass needs beside the buffers (the previous camera is unused on the first frame) */
struct TpFrame {
    TpCamera cur, prev;
    int w, h, x0, y0;                   /* the crop's size and origin */
    uint32_t flags;
    int same_view;                      /* tp_same_view(cur, prev): a pixel's tap is the pixel itself, and the two geometry tests are not made */
    float alpha_min, normal_tol, plane_tol, albedo_eps, albedo_tol;
};

/* step 2's one function: a world-space point or direction -> raster x, y and camera-space depth z */
FTN_HD V3 tp_project(const TpCamera& c, V3 v, bool point) {
    const V3 q = point ? m4_point(c.w2c, v) : m4_vector(c.w2c, v);
    const V3 r = m4_point(c.c2r, q);
    return V3(r.x, r.y, q.z);
}

/* step 3's test of a tap's demodulation divisor against the pixel's: |a - b| <= tol max(a, b) */
FTN_HD bool tp_same_divisor(float a, float b, float tol) { return fabsf(a - b) <= tol * (a > b ? a : b); }

/* bit-equality of two floats (a NaN equals its copy, +0 differs from -0) */
FTN_HD bool tp_same_bits(float a, float b) { return ftn_det::f2u(a) == ftn_det::f2u(b); }

/* Step 2 for crop pixel (x, y) of a crop at (x0, y0): the two raster positions whose difference is the motion, rc in the current camera and
 * rp (with the camera-space depth in z) in the previous one.  A covered pixel projects x_cur into the current camera and x_prev into the
 * previous one as points -- the same point twice in a static scene, the previous-position pass's value (fountain_hip_motion.h) in a
 * moving one; an uncovered pixel projects its direction into both. */
FTN_HD void tp_motion(const TpCamera& cur, const TpCamera& prev, bool covered, V3 x_cur, V3 x_prev, int x, int y, int x0, int y0, V3* rc, V3* rp) {
    if (!covered) x_cur = x_prev = m4_vector(cur.c2w, m4_point(cur.r2c, V3((float)(x + x0) + 0.5f, (float)(y + y0) + 0.5f, 0.0f)));
    *rc = tp_project(cur, x_cur, covered); *rp = tp_project(prev, x_prev, covered);
}

/* steps 1 to 5 for pixel (x, y); prev_gb12 and prev_hist are null on the first frame.  Writes the pixel's history, rgb and var4.
 * mv8 (null: a static scene): the current frame's resolved previous positions and normals, fountain_hip_motion.h's changes to steps 2 and 3. */
FTN_HD void tp_accumulate_pixel(const float* rgb, const float* gb12, const float* var4, const float* prev_gb12, const float4* prev_hist,
                                const TpFrame& F, int x, int y, float4* out_hist, float* out_rgb, float* out_var4, const float* mv8 = nullptr) {
    const size_t p = (size_t)y * (size_t)F.w + (size_t)x;
    const float* gb = gb12 + 12 * p;
    const float* var = var4 + 4 * p;
    float4 ucur, np, xp;
    dn_prepare_pixel(rgb + 3 * p, gb, F.flags, F.albedo_eps, &ucur, &np, &xp);
    const bool cov_p = np.w > 0.0f;
    const bool demod = (F.flags & FTN_DENOISE_DEMODULATE) && cov_p;
    float dr = 1.0f, dg = 1.0f, db = 1.0f, d2r = 1.0f, d2g = 1.0f, d2b = 1.0f;
    float4 nucur = make_float4(var[0], var[1], var[2], var[3]);
    if (demod) {
        dr = dn_divisor(gb[0], F.albedo_eps); dg = dn_divisor(gb[1], F.albedo_eps); db = dn_divisor(gb[2], F.albedo_eps);
        d2r = dr * dr; d2g = dg * dg; d2b = db * db;
        nucur.x = var[0] / d2r; nucur.y = var[1] / d2g; nucur.z = var[2] / d2b;
    }
    if (!dn_finite3(ucur) || !(nucur.x >= 0.0f) || !(nucur.y >= 0.0f) || !(nucur.z >= 0.0f) || !(nucur.w >= 0.0f)) {
        out_hist[2 * p] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        out_hist[2 * p + 1] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        out_rgb[3 * p] = rgb[3 * p]; out_rgb[3 * p + 1] = rgb[3 * p + 1]; out_rgb[3 * p + 2] = rgb[3 * p + 2];
        out_var4[4 * p] = var[0]; out_var4[4 * p + 1] = var[1]; out_var4[4 * p + 2] = var[2]; out_var4[4 * p + 3] = var[3];
        return;
    }

    float W = 0.0f, sn = 0.0f;
    float su0 = 0.0f, su1 = 0.0f, su2 = 0.0f, sv0 = 0.0f, sv1 = 0.0f, sv2 = 0.0f, sv3 = 0.0f;
    /* the pixel's surface in the previous frame: where and how it stood (the pixel's own x_p, n_p without mv8), whether it stood still, and
     * whether mv8 speaks of the same coverage class as gb12 */
    V3 xq(xp.x, xp.y, xp.z), nq(np.x, np.y, np.z);
    bool still = true, same_class = true;
    if (mv8) {
        const float* mv = mv8 + 8 * p;
        same_class = (mv[6] > 0.0f) == cov_p;
        if (cov_p) {
            xq = V3(mv[0], mv[1], mv[2]); nq = V3(mv[3], mv[4], mv[5]);
            still = tp_same_bits(xq.x, xp.x) && tp_same_bits(xq.y, xp.y) && tp_same_bits(xq.z, xp.z) &&
                    tp_same_bits(nq.x, np.x) && tp_same_bits(nq.y, np.y) && tp_same_bits(nq.z, np.z);
        }
    }
    const bool untested = F.same_view && still;          /* equal cameras and a surface that did not move: the pixel is its own only tap */
    if (prev_hist && same_class) {
        V3 rc, rp;
        tp_motion(F.cur, F.prev, cov_p, V3(xp.x, xp.y, xp.z), xq, x, y, F.x0, F.y0, &rc, &rp);
        const float sx = (float)x + (rp.x - rc.x), sy = (float)y + (rp.y - rc.y);
        /* NaN fails every comparison; inside the bounds the conversions to int are exact */
        if (rp.z > 0.0f && sx > -1.0f && sx < (float)F.w && sy > -1.0f && sy < (float)F.h) {
            const float fx = floorf(sx), fy = floorf(sy);
            const int ix = (int)fx, iy = (int)fy;
            const float tx = sx - fx, ty = sy - fy;
            const float zc = xp.w > 1e-6f ? xp.w : 1e-6f;
            const float plane_max = F.plane_tol * zc;
#pragma unroll
            for (int j = 0; j < 2; j++) {
#pragma unroll
                for (int i = 0; i < 2; i++) {
                    const float b = (i ? tx : 1.0f - tx) * (j ? ty : 1.0f - ty);
                    const int qx = ix + i, qy = iy + j;
                    if (b == 0.0f || qx < 0 || qx >= F.w || qy < 0 || qy >= F.h) continue;
                    const size_t q = (size_t)qy * (size_t)F.w + (size_t)qx;
                    float4 hu = prev_hist[2 * q], hv = prev_hist[2 * q + 1];
                    if (!(hu.w > 0.0f)) continue;
                    const float* gq = prev_gb12 + 12 * q;
                    if ((gq[10] > 0.0f) != cov_p) continue;
                    if (demod) {                      /* a tap divided by another divisor is carried over by what it stands for, u d */
                        const float qr = dn_divisor(gq[0], F.albedo_eps), qg = dn_divisor(gq[1], F.albedo_eps), qb = dn_divisor(gq[2], F.albedo_eps);
                        if (!tp_same_divisor(dr, qr, F.albedo_tol)) { hu.x = (hu.x * qr) / dr; hv.x = (hv.x * (qr * qr)) / d2r; }
                        if (!tp_same_divisor(dg, qg, F.albedo_tol)) { hu.y = (hu.y * qg) / dg; hv.y = (hv.y * (qg * qg)) / d2g; }
                        if (!tp_same_divisor(db, qb, F.albedo_tol)) { hu.z = (hu.z * qb) / db; hv.z = (hv.z * (qb * qb)) / d2b; }
                    }
                    if (!dn_finite3(hu) || hv.x != hv.x || hv.y != hv.y || hv.z != hv.z || hv.w != hv.w) continue;
                    if (cov_p && !untested) {
                        const float e0 = nq.x - gq[3], e1 = nq.y - gq[4], e2 = nq.z - gq[5];
                        if (!((e0 * e0 + e1 * e1) + e2 * e2 <= F.normal_tol)) continue;
                        const float pd = (nq.x * (xq.x - gq[6]) + nq.y * (xq.y - gq[7])) + nq.z * (xq.z - gq[8]);
                        if (!(fabsf(pd) <= plane_max)) continue;
                    }
                    W = W + b;
                    sn = sn + b * hu.w;
                    su0 = su0 + b * hu.x; su1 = su1 + b * hu.y; su2 = su2 + b * hu.z;
                    sv0 = sv0 + b * hv.x; sv1 = sv1 + b * hv.y; sv2 = sv2 + b * hv.z; sv3 = sv3 + b * hv.w;
                }
            }
        }
    }

    float4 u = ucur, nu = nucur;
    float n = 1.0f;
    if (W > 0.0f) {
        const float n1 = sn / W + 1.0f;
        const float a0 = 1.0f / n1;
        const float alpha = a0 > F.alpha_min ? a0 : F.alpha_min;
        if (alpha < 1.0f) {
            const float k = 1.0f - alpha, kk = k * k, aa = alpha * alpha;
            n = n1;
            u.x = k * (su0 / W) + alpha * ucur.x; u.y = k * (su1 / W) + alpha * ucur.y; u.z = k * (su2 / W) + alpha * ucur.z;
            nu.x = kk * (sv0 / W) + aa * nucur.x; nu.y = kk * (sv1 / W) + aa * nucur.y;
            nu.z = kk * (sv2 / W) + aa * nucur.z; nu.w = kk * (sv3 / W) + aa * nucur.w;
        }
    }
    out_hist[2 * p] = make_float4(u.x, u.y, u.z, n);
    out_hist[2 * p + 1] = nu;
    dn_finish_pixel(u, gb, F.flags, F.albedo_eps, out_rgb + 3 * p);
    if (demod) { out_var4[4 * p] = nu.x * d2r; out_var4[4 * p + 1] = nu.y * d2g; out_var4[4 * p + 2] = nu.z * d2b; }
    else { out_var4[4 * p] = nu.x; out_var4[4 * p + 1] = nu.y; out_var4[4 * p + 2] = nu.z; }
    out_var4[4 * p + 3] = nu.w;
}

/* the device path of ftn_temporal_accumulate_device (arguments already checked): one launch.  Returns the launch error, if any.
 * mv8: the current frame's resolved previous positions (fountain_hip_motion.h), or null */
hipError_t launch_temporal(const float* rgb, const float* gb12, const float* var4, const float* prev_gb12, const float4* prev_hist,
                           const TpFrame& frame, float4* out_hist, float* out_rgb, float* out_var4, hipStream_t stream, const float* mv8 = nullptr);

#pragma GCC visibility push(hidden)
/* The bodies of ftn_temporal_accumulate_device, ftn_temporal_accumulate and ftn_temporal_accumulate_cpu (ftn_temporal_host.cpp), which those
 * entry points call with mv8 = null and fountain_hip_motion.h's ftn_temporal_accumulate_motion* with the caller's: refusals, buffers and
 * the per-pixel code are one. */
int tp_accumulate_device(const void* rgb, const void* gb12, const void* var4, const void* mv8, const ftn_camera_desc* cur_camera, const ftn_film_desc* film,
                         int32_t w, int32_t h, const ftn_camera_desc* prev_camera, const void* prev_gb12, const void* prev_history,
                         const ftn_temporal_params* params, void* out_history, void* out_rgb, void* out_var4, void* stream);
int tp_accumulate_host(const float* rgb, const float* gb12, const float* var4, const float* mv8, const ftn_camera_desc* cur_camera, const ftn_film_desc* film,
                       int32_t w, int32_t h, const ftn_camera_desc* prev_camera, const float* prev_gb12, const ftn_temporal_pixel* prev_history,
                       const ftn_temporal_params* params, ftn_temporal_pixel* out_history, float* out_rgb, float* out_var4, int32_t device);
int tp_accumulate_cpu(const float* rgb, const float* gb12, const float* var4, const float* mv8, const ftn_camera_desc* cur_camera, const ftn_film_desc* film,
                      int32_t w, int32_t h, const ftn_camera_desc* prev_camera, const float* prev_gb12, const ftn_temporal_pixel* prev_history,
                      const ftn_temporal_params* params, ftn_temporal_pixel* out_history, float* out_rgb, float* out_var4);
#pragma GCC visibility pop

}  // namespace ftn
#endif
