/*
 * ftn_subdiv.h -- Loop subdivision of include/fountain_hip_subdiv.h: the per-element code (the fan walk, the ring, the even, odd, limit
 * and normal rules, a face's children), shared by the kernels (ftn_subdiv.hip) and the host twin (ftn_subdiv_host.cpp) so that both give
 * the same bits, and the device driver's declaration.  Every walk is bounded by max(the control mesh's max_valence, 6); one that runs into
 * the bound reports it (SdFan::ok) and its vertex is written as zeros instead of being walked again.
 */
#ifndef FTN_SUBDIV_H
#define FTN_SUBDIV_H
#include <hip/hip_runtime.h>
#include "detmath.h"
#include "../../include/fountain_hip_subdiv.h"

namespace ftn {

/* one level of the mesh: positions, the faces' vertices and neighbours (3 per face), the vertices' start faces and boundary flags */
struct SdLevel { const float* P; const int32_t* idx; const int32_t* nb; const int32_t* sf; const uint8_t* bd; uint32_t V, F; int32_t max_valence; };
struct Sd3 { float x, y, z; };
/* a vertex's fan: n = the length of its ring; first = the face its ring starts at (sf[v], or the forward end of a boundary fan); the
 * ends r_0 and r_{n-1} of a boundary ring */
struct SdFan { int32_t first, n, r0, rl; bool ok; };

constexpr uint32_t kSdFlagWalk = 0, kSdFlagNormal = 1, kSdFlagWords = 2;      /* flag words: a walk hit its bound; the smallest vertex with a bad normal */
constexpr uint32_t kSdNoVertex = 0xffffffffu;

FTN_HD int sd_next(int k) { return k == 2 ? 0 : k + 1; }
FTN_HD int sd_prev(int k) { return k == 0 ? 2 : k - 1; }
FTN_HD int sd_vnum(const int32_t* idx, int32_t f, int32_t v) { const int32_t* t = idx + 3 * (size_t)f; return t[0] == v ? 0 : (t[1] == v ? 1 : 2); }
FTN_HD Sd3 sd_load(const float* P, int32_t v) { const float* p = P + 3 * (size_t)v; return Sd3{p[0], p[1], p[2]}; }
FTN_HD void sd_store(float* P, size_t v, Sd3 a) { float* p = P + 3 * v; p[0] = a.x; p[1] = a.y; p[2] = a.z; }
FTN_HD Sd3 sd_scale(float w, Sd3 a) { return Sd3{w * a.x, w * a.y, w * a.z}; }
FTN_HD Sd3 sd_add(Sd3 a, Sd3 b) { return Sd3{a.x + b.x, a.y + b.y, a.z + b.z}; }
FTN_HD Sd3 sd_sub(Sd3 a, Sd3 b) { return Sd3{a.x - b.x, a.y - b.y, a.z - b.z}; }
/* a + w * b */
FTN_HD Sd3 sd_madd(Sd3 a, float w, Sd3 b) { return Sd3{a.x + w * b.x, a.y + w * b.y, a.z + w * b.z}; }

FTN_HD float sd_beta(int32_t n) { return n == 3 ? 0.1875f : 3.0f / (8.0f * (float)n); }
FTN_HD float sd_gamma(int32_t n) { return 1.0f / ((float)n + 3.0f / (8.0f * sd_beta(n))); }

/* the first walk around v: the ring's length and, for a boundary vertex, where the ring starts and its two ends */
FTN_HD SdFan sd_fan(const SdLevel& L, int32_t v) {
    SdFan fan = {L.sf[v], 0, -1, -1, false};
    int32_t f = fan.first;
    if (!L.bd[v]) {
        /* `closed` is an integer each lane keeps from the step it leaves the loop at: hipcc (ROCm 7) took `ok = f == fan.first` after the
         * loop from the loop's own last comparison, which holds nothing for a lane that left in an earlier step than its wave */
        int32_t n = 0, closed = 0;
        do {
            f = L.nb[3 * (size_t)f + sd_vnum(L.idx, f, v)]; n++;
            if (f == fan.first) closed = n;
        } while (closed == 0 && f >= 0 && n < L.max_valence);
        fan.n = n; fan.ok = closed != 0;
        return fan;
    }
    int32_t steps = 0, g;
    while ((g = L.nb[3 * (size_t)f + sd_vnum(L.idx, f, v)]) >= 0 && steps < L.max_valence) { f = g; steps++; }
    if (g >= 0) return fan;
    fan.first = f;
    fan.r0 = L.idx[3 * (size_t)f + sd_next(sd_vnum(L.idx, f, v))];
    int32_t n = 1;
    for (;;) {
        const int k = sd_prev(sd_vnum(L.idx, f, v));
        n++;
        g = L.nb[3 * (size_t)f + k];
        if (g < 0) { fan.rl = L.idx[3 * (size_t)f + k]; break; }
        if (n >= L.max_valence) return fan;
        f = g;
    }
    fan.n = n; fan.ok = true;
    return fan;
}

/* r_j of the ring of v, for j = 0 .. n - 1 in turn, and the face to go on from; f starts as fan.first; `fan` is sd_fan's and ok */
struct SdStep { int32_t q, f; };
FTN_HD SdStep sd_ring_at(const SdLevel& L, int32_t v, const SdFan& fan, bool boundary, int32_t j, int32_t f) {
    if (boundary && j == 0) return SdStep{fan.r0, f};
    const int kv = sd_vnum(L.idx, f, v), k = boundary ? sd_prev(kv) : kv;
    return SdStep{L.idx[3 * (size_t)f + (boundary ? k : sd_next(kv))], L.nb[3 * (size_t)f + k]};
}

/* the one-ring rule with weight w (beta(n): an even interior vertex; gamma(n): its limit position), read from P */
FTN_HD Sd3 sd_interior_rule(const SdLevel& L, const float* P, int32_t v, const SdFan& fan, float w) {
    Sd3 p = sd_scale(1.0f - (float)fan.n * w, sd_load(P, v));
    int32_t f = fan.first;
    for (int32_t j = 0; j < fan.n; j++) { const SdStep s = sd_ring_at(L, v, fan, false, j, f); f = s.f; p = sd_madd(p, w, sd_load(P, s.q)); }
    return p;
}
/* the boundary rule with weight w (0.125f: an even boundary vertex; 0.2f: its limit position) */
FTN_HD Sd3 sd_boundary_rule(const float* P, int32_t v, const SdFan& fan, float w) {
    return sd_madd(sd_madd(sd_scale(1.0f - 2.0f * w, sd_load(P, v)), w, sd_load(P, fan.r0)), w, sd_load(P, fan.rl));
}
FTN_HD Sd3 sd_vertex_rule(const SdLevel& L, int32_t v, const SdFan& fan, bool limit) {
    if (L.bd[v]) return sd_boundary_rule(L.P, v, fan, limit ? 0.2f : 0.125f);
    return sd_interior_rule(L, L.P, v, fan, limit ? sd_gamma(fan.n) : sd_beta(fan.n));
}

/* does slot (f, k) own its edge? */
FTN_HD bool sd_owner(const SdLevel& L, int32_t f, int k) { const int32_t g = L.nb[3 * (size_t)f + k]; return g < 0 || f < g; }

/* the odd vertex of the edge slot (f, k) owns; *nslot is the neighbour's slot (3 g + vnum(g, b)) or -1 */
FTN_HD Sd3 sd_odd_rule(const SdLevel& L, int32_t f, int k, bool* boundary, int64_t* nslot) {
    const int32_t* t = L.idx + 3 * (size_t)f;
    const int32_t a = t[k], b = t[sd_next(k)], g = L.nb[3 * (size_t)f + k];
    const Sd3 pa = sd_load(L.P, a), pb = sd_load(L.P, b);
    *boundary = g < 0;
    if (g < 0) { *nslot = -1; return sd_add(sd_scale(0.5f, pa), sd_scale(0.5f, pb)); }
    const int kg = sd_vnum(L.idx, g, b);
    *nslot = 3 * (int64_t)g + kg;
    const Sd3 pc = sd_load(L.P, t[sd_prev(k)]), pd = sd_load(L.P, L.idx[3 * (size_t)g + sd_prev(kg)]);
    return sd_madd(sd_madd(sd_add(sd_scale(0.375f, pa), sd_scale(0.375f, pb)), 0.125f, pc), 0.125f, pd);
}

/* the four children of face f: their 12 vertices and 12 neighbours (child c's entry j at 3 c + j); e = the face's three odd vertices */
FTN_HD void sd_children(const SdLevel& L, int32_t f, const int32_t* e, int32_t* cidx, int32_t* cnb) {
    const int32_t* t = L.idx + 3 * (size_t)f;
    const int32_t* h = L.nb + 3 * (size_t)f;
    for (int j = 0; j < 3; j++) {
        const int nj = sd_next(j), pj = sd_prev(j);
        cnb[9 + j] = 4 * f + nj;
        cnb[3 * j + nj] = 4 * f + 3;
        const int32_t f2 = h[j], f3 = h[pj];
        cnb[3 * j + j] = f2 < 0 ? -1 : 4 * f2 + sd_vnum(L.idx, f2, t[j]);
        cnb[3 * j + pj] = f3 < 0 ? -1 : 4 * f3 + sd_vnum(L.idx, f3, t[j]);
        cidx[3 * j + j] = t[j];
        cidx[3 * j + nj] = e[j];
        cidx[3 * nj + j] = e[j];
        cidx[9 + j] = e[j];
    }
}

/* the limit normal of v from the limit positions Lim; false when its length is zero or not finite */
FTN_HD bool sd_normal(const SdLevel& L, const float* Lim, int32_t v, const SdFan& fan, Sd3* out) {
    const float pi_f = 3.14159265358979323846f;
    const int32_t n = fan.n;
    Sd3 S = {0.0f, 0.0f, 0.0f}, T = {0.0f, 0.0f, 0.0f};
    int32_t f = fan.first;
    if (!L.bd[v]) {
        for (int32_t j = 0; j < n; j++) {
            float s, c;
            ftn_det::sincosf_det(((2.0f * pi_f) * (float)j) / (float)n, &s, &c);
            const SdStep t = sd_ring_at(L, v, fan, false, j, f);
            f = t.f;
            const Sd3 r = sd_load(Lim, t.q);
            S = sd_madd(S, c, r); T = sd_madd(T, s, r);
        }
    } else {
        const Sd3 c = sd_load(Lim, v), r0 = sd_load(Lim, fan.r0), rl = sd_load(Lim, fan.rl);
        S = sd_sub(rl, r0);
        if (n == 2) T = sd_sub(sd_add(r0, rl), sd_scale(2.0f, c));
        else if (n == 3 || n == 4) {
            const SdStep t1 = sd_ring_at(L, v, fan, true, 1, f);
            const Sd3 r1 = sd_load(Lim, t1.q);
            if (n == 3) T = sd_sub(r1, c);
            else {
                const Sd3 r2 = sd_load(Lim, sd_ring_at(L, v, fan, true, 2, t1.f).q);
                T = sd_sub(sd_sub(sd_madd(sd_madd(Sd3{-r0.x, -r0.y, -r0.z}, 2.0f, r1), 2.0f, r2), rl), sd_scale(2.0f, c));
            }
        } else {
            const float theta = pi_f / (float)(n - 1);
            float st, ct;
            ftn_det::sincosf_det(theta, &st, &ct);
            const float w = 2.0f * ct - 2.0f;
            T = sd_scale(st, sd_add(r0, rl));
            for (int32_t k = 1; k <= n - 2; k++) {
                const SdStep t = sd_ring_at(L, v, fan, true, k, f);
                f = t.f;
                T = sd_madd(T, w * ftn_det::sinf_det((float)k * theta), sd_load(Lim, t.q));
            }
            T = Sd3{-T.x, -T.y, -T.z};
        }
    }
    Sd3 N = {T.y * S.z - T.z * S.y, T.z * S.x - T.x * S.z, T.x * S.y - T.y * S.x};
    const float len = sqrtf((N.x * N.x + N.y * N.y) + N.z * N.z);
    const bool good = len > 0.0f && len - len == 0.0f;
    *out = Sd3{N.x / len, N.y / len, N.z / len};
    return good;
}

/* device buffers of a run (ftn_subdiv_host.cpp allocates them): level l lives in set l & 1 */
struct SdDevice {
    float* P[2]; int32_t* idx[2]; int32_t* nb[2]; int32_t* sf[2]; uint8_t* bd[2];
    float* N;                         /* 3 V_L floats; the limit positions go to the P set the last level does not use */
    int32_t* eidx;                    /* 3 F_{levels-1}: the odd vertex of every slot */
    uint32_t* sums;                   /* one per 256 slots of the largest scanned level */
    uint32_t* flags;                  /* kSdFlagWords */
};
/* level 0 is in set 0; runs every level, the limit pass and the normal pass on `stream`; the results are in idx[levels & 1],
 * P[(levels + 1) & 1] (limit positions) and N.  Launches kernels and memsets only. */
hipError_t launch_subdivide(const SdDevice& d, const ftn_subdiv_info& info, hipStream_t stream);

}  // namespace ftn
#endif
