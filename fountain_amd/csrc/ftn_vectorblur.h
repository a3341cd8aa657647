/*
 * ftn_vectorblur.h -- the vector-blur stage of include/fountain_hip_vectorblur.h: the per-pixel code (a pixel's record, the order the
 * maxima are taken by, a tile's tap offsets, a tap's weight and the gather's sums), shared by the kernels (ftn_vectorblur.hip) and the
 * host twin (ftn_vectorblur_host.cpp) so that both give the same bits, the workspace's plan, and the device driver's declaration.  Small
 * structs and floats go by value.
 */
#ifndef FTN_VECTORBLUR_H
#define FTN_VECTORBLUR_H
#include <hip/hip_runtime.h>
#include "ftn_math.h"
#include "../../include/fountain_hip_vectorblur.h"

namespace ftn {

#define FTN_VB_TILE 16                              /* the film's tile; FTN_VECTORBLUR_MAX_RADIUS is its side */
static_assert(FTN_VB_TILE == FTN_VECTORBLUR_MAX_RADIUS, "a blur must stay inside the 3 x 3 tiles around its own");

/* a pixel's record of step 1 {h.x, h.y, len, z}; a tile's record of steps 2 and 3 {h.x, h.y, key, 0} */
struct VbRec { float x, y, l, z; };
struct Vb3 { float r, g, b; };

/* what a pixel reads: the parameters and what follows from them once per call */
struct VbCall { int taps; float half_shutter, max_radius, depth_extent; };

FTN_HD VbCall vb_make(const ftn_vectorblur_params& p) { return VbCall{p.taps, 0.5f * p.shutter, p.max_radius, p.depth_extent}; }

FTN_HD bool vb_finite(float v) { return (f2u(v) & 0x7f800000u) != 0x7f800000u; }
FTN_HD bool vb_finite3(float r, float g, float b) { return vb_finite(r) && vb_finite(g) && vb_finite(b); }

/* a pixel's depth from its G-buffer floats 9 and 10 */
FTN_HD float vb_depth(float z, float c) { return (c > 0.0f && vb_finite(z)) ? z : u2f(0x7f800000u); }

/* step 1 */
FTN_HD VbRec vb_velocity(float mx, float my, float z, VbCall e) {
    float hx = 0.0f, hy = 0.0f;
    if (vb_finite(mx) && vb_finite(my)) { hx = e.half_shutter * mx; hy = e.half_shutter * my; }
    const float len2 = hx * hx + hy * hy;
    float len = sqrtf(len2);
    if (len > e.max_radius) {
        const float k = e.max_radius / len;
        hx = hx * k; hy = hy * k; len = e.max_radius;
    }
    return VbRec{hx, hy, len, z};
}

FTN_HD float vb_key(VbRec r) { return r.l * r.l; }

/* steps 2 and 3: is (key a, index ia) before (key b, index ib) in the order the maxima are taken by?  Keys are never NaN. */
FTN_HD bool vb_before(float a, uint32_t ia, float b, uint32_t ib) { return a > b || (a == b && ia < ib); }

/* step 4: tap i's offset for a tile whose neighbour record is n, and its length */
struct VbOffset { int ox, oy; float d; };
FTN_HD VbOffset vb_offset(int i, int taps, VbRec n) {
    const float t = (float)(2 * i + 1 - taps) / (float)taps;
    VbOffset o;
    o.ox = (int)rintf(t * n.x); o.oy = (int)rintf(t * n.y);
    o.d = sqrtf((float)(o.ox * o.ox + o.oy * o.oy));
    return o;
}

FTN_HD float vb_cone(float d, float r) { return r > d ? 1.0f - d / r : 0.0f; }
FTN_HD float vb_cyl(float d, float r) {
    if (!(r > 0.0f)) return 0.0f;
    const float e0 = 0.95f * r, e1 = 1.05f * r;
    float u = (d - e0) / (e1 - e0);
    u = u < 0.0f ? 0.0f : (u > 1.0f ? 1.0f : u);
    return 1.0f - (u * u) * (3.0f - 2.0f * u);
}
FTN_HD float vb_front(float a, float b, float depth_extent) {
    if (a <= b) return 1.0f;
    const float f = 1.0f - (a - b) / (depth_extent * (b > 1e-6f ? b : 1e-6f));
    return f > 0.0f ? f : 0.0f;
}

/* a tap's weight: d its offset's length, (hq, zq) the tap's record, (hp, zp) the pixel's */
FTN_HD float vb_weight(float d, float hq, float zq, float hp, float zp, float depth_extent) {
    return (vb_front(zq, zp, depth_extent) * vb_cone(d, hq) + vb_front(zp, zq, depth_extent) * vb_cone(d, hp)) + (2.0f * vb_cyl(d, hq)) * vb_cyl(d, hp);
}

/* the gather's sums of one pixel, from the centre on */
struct VbSum {
    float W, r, g, b; bool any;
    FTN_HD void centre(Vb3 c, float hp, int taps) {
        W = (float)taps / (4.0f * (hp > 0.5f ? hp : 0.5f));
        r = W * c.r; g = W * c.g; b = W * c.b; any = false;
    }
    FTN_HD void tap(float wt, Vb3 c) {
        W = W + wt; r = r + wt * c.r; g = g + wt * c.g; b = b + wt * c.b;
        any = any || wt > 0.0f;
    }
    FTN_HD Vb3 result(Vb3 c) const { return any ? Vb3{r / W, g / W, b / W} : c; }
};

/* step 4 for pixel (x, y) of a tile whose neighbour record is n (n.l = the key) and whose taps' offsets are off[0 .. taps - 1]:
 * rgb(qx, qy) and rec(qx, qy) fetch a pixel inside the image */
template <class Rgb, class Rec> FTN_HD Vb3 vb_gather_pixel(int x, int y, int w, int h, VbRec n, const VbOffset* off, VbCall e, Rgb rgb, Rec rec) {
    const Vb3 c = rgb(x, y);
    if (n.l <= 0.25f || !vb_finite3(c.r, c.g, c.b)) return c;
    const VbRec p = rec(x, y);
    VbSum s;
    s.centre(c, p.l, e.taps);
    for (int i = 0; i < e.taps; i++) {
        const VbOffset o = off[i];
        const int qx = x + o.ox, qy = y + o.oy;
        if ((o.ox == 0 && o.oy == 0) || qx < 0 || qy < 0 || qx >= w || qy >= h) continue;
        const Vb3 cq = rgb(qx, qy);
        if (!vb_finite3(cq.r, cq.g, cq.b)) continue;
        const VbRec q = rec(qx, qy);
        s.tap(vb_weight(o.d, q.l, q.z, p.l, p.z, e.depth_extent), cq);
    }
    return s.result(c);
}

/* the workspace: the pixels' records, the tiles' records, the neighbour records (offsets in VbRec = 16 bytes) */
struct VbPlan { int w, h, tiles_x, tiles_y; size_t tile_off, nb_off, recs; };
inline VbPlan vb_plan(int w, int h) {
    VbPlan p;
    p.w = w; p.h = h; p.tiles_x = (w + FTN_VB_TILE - 1) / FTN_VB_TILE; p.tiles_y = (h + FTN_VB_TILE - 1) / FTN_VB_TILE;
    const size_t tiles = (size_t)p.tiles_x * (size_t)p.tiles_y;
    p.tile_off = (size_t)w * (size_t)h; p.nb_off = p.tile_off + tiles; p.recs = p.nb_off + tiles;
    return p;
}

/* ftn_vectorblur.hip: the four kernels on `stream`; gb12 may be null */
hipError_t launch_vectorblur(const float* rgb, const float* motion2, const float* gb12, const VbPlan& plan, const VbCall& e, float* out_rgb, VbRec* workspace,
                             hipStream_t stream);

}  // namespace ftn
#endif
