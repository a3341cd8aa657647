/*
 * ftn_idmatte.h -- what the ID-matte pass's device and host code share (ftn_idmatte.hip, ftn_idmatte_host.cpp; C ABI:
 * include/fountain_hip_idmatte.h): the per-pixel table and its update rule, the resolve and the matte extraction of one pixel.  Compiled
 * by hipcc for the kernels and by the host compiler for their bit-identical twins, as gbuffer_resolve_pixel is.
 *
 * Every loop over the eight slots has a constant trip count and indexes with the loop variable alone, so that it unrolls and the arrays
 * become registers: a slot chosen at run time is reached by a compare-and-select over all eight, never by a runtime index (which would
 * put the table into scratch memory).
 */
#ifndef FTN_IDMATTE_H
#define FTN_IDMATTE_H
#include "ftn_wavefront.h"

namespace ftn {
/* ID tables over the camera samples wavefront_render traces for the same parameters (indexed sampler): d_ids = the caller's id of every
 * primitive in BVH order; d_out = 20 words per crop pixel (ftn_idmatte_pixel), continued */
int wavefront_idmatte(WavefrontState** state, const RenderParams& P, const std::vector<DTile>& tiles, const uint32_t* d_ids, uint32_t* d_out,
                      hipStream_t stream, double* trace_ms);
hipError_t launch_idmatte_resolve(const uint32_t* in, size_t n, uint32_t* out20, hipStream_t stream);
/* ids: n_ids sorted ids on the device */
void launch_idmatte_select(const uint32_t* resolved, size_t n, const uint32_t* ids, size_t n_ids, uint32_t flags, float* mask, hipStream_t stream);

#define IM_SLOTS 8
#define IM_WORDS 20           /* 32-bit words of a ftn_idmatte_pixel, and of a resolved pixel */
#define IM_SAMPLE_BITS 28     /* a call's sample indices in the sort key of a sample that reaches another pixel */

struct ImTable { uint32_t id[IM_SLOTS]; float w[IM_SLOTS]; float overflow, miss, total; uint32_t n; };

/* ftn_idmatte_pixel as 20 words: id 8, weight 8, overflow, miss, total, n_used */
FTN_HD void im_load(const uint32_t* px, ImTable* t) {
#pragma unroll
    for (int k = 0; k < IM_SLOTS; k++) { t->id[k] = px[k]; t->w[k] = ftn_det::u2f(px[IM_SLOTS + k]); }
    t->overflow = ftn_det::u2f(px[16]); t->miss = ftn_det::u2f(px[17]); t->total = ftn_det::u2f(px[18]); t->n = px[19];
}
FTN_HD void im_store(const ImTable& t, uint32_t* px) {
#pragma unroll
    for (int k = 0; k < IM_SLOTS; k++) { px[k] = t.id[k]; px[IM_SLOTS + k] = ftn_det::f2u(t.w[k]); }
    px[16] = ftn_det::f2u(t.overflow); px[17] = ftn_det::f2u(t.miss); px[18] = ftn_det::f2u(t.total); px[19] = t.n;
}

/* one sample of box weight w into a pixel's table: a miss, or the id x (include/fountain_hip_idmatte.h) */
FTN_HD void im_add(ImTable* t, bool hit, uint32_t x, float w) {
    t->total += w;
    if (!hit) { t->miss += w; return; }
    bool found = false;
#pragma unroll
    for (int k = 0; k < IM_SLOTS; k++) {
        const bool here = !found && (uint32_t)k < t->n && t->id[k] == x;
        t->w[k] = here ? t->w[k] + w : t->w[k];
        found = found || here;
    }
    if (found) return;
    if (t->n >= (uint32_t)IM_SLOTS) { t->overflow += w; return; }
#pragma unroll
    for (int k = 0; k < IM_SLOTS; k++) {
        const bool here = (uint32_t)k == t->n;
        t->id[k] = here ? x : t->id[k];
        t->w[k] = here ? w : t->w[k];
    }
    t->n += 1;
}

/* a compare-exchange of the sorting network, on scalars.  Rank order of two slots: used before unused, then weight descending, then id
 * ascending */
FTN_HD void im_cswap(uint32_t& ia, float& wa, uint32_t& ua, uint32_t& ib, float& wb, uint32_t& ub) {
    const bool b_first = ua != ub ? ub > ua : (wa != wb ? wb > wa : ib < ia);
    const uint32_t i0 = b_first ? ib : ia, i1 = b_first ? ia : ib, u0 = b_first ? ub : ua, u1 = b_first ? ua : ub;
    const float w0 = b_first ? wb : wa, w1 = b_first ? wa : wb;
    ia = i0; ib = i1; ua = u0; ub = u1; wa = w0; wb = w1;
}
#define IM_CSWAP(a, b) im_cswap(id[a], w[a], used[a], id[b], w[b], used[b])

/* ftn_idmatte_resolve for one pixel: the nineteen compare-exchanges of the six-layer sorting network for eight elements */
FTN_HD void idmatte_resolve_pixel(const uint32_t* in, uint32_t* out) {
    const float total = ftn_det::u2f(in[18]);
    if (total == 0.0f) {
#pragma unroll
        for (int k = 0; k < IM_WORDS; k++) out[k] = 0u;
        return;
    }
    const uint32_t n = in[19];
    uint32_t id[IM_SLOTS], used[IM_SLOTS]; float w[IM_SLOTS];
#pragma unroll
    for (int k = 0; k < IM_SLOTS; k++) {
        used[k] = (uint32_t)k < n ? 1u : 0u;
        id[k] = used[k] ? in[k] : 0u; w[k] = used[k] ? ftn_det::u2f(in[IM_SLOTS + k]) : 0.0f;
    }
    IM_CSWAP(0, 2); IM_CSWAP(1, 3); IM_CSWAP(4, 6); IM_CSWAP(5, 7);
    IM_CSWAP(0, 4); IM_CSWAP(1, 5); IM_CSWAP(2, 6); IM_CSWAP(3, 7);
    IM_CSWAP(0, 1); IM_CSWAP(2, 3); IM_CSWAP(4, 5); IM_CSWAP(6, 7);
    IM_CSWAP(2, 4); IM_CSWAP(3, 5);
    IM_CSWAP(1, 4); IM_CSWAP(3, 6);
    IM_CSWAP(1, 2); IM_CSWAP(3, 4); IM_CSWAP(5, 6);
    const float overflow = ftn_det::u2f(in[16]), miss = ftn_det::u2f(in[17]);
#pragma unroll
    for (int k = 0; k < IM_SLOTS; k++) {
        out[2 * k] = id[k];
        out[2 * k + 1] = ftn_det::f2u(used[k] ? w[k] / total : 0.0f);
    }
    out[16] = ftn_det::f2u(overflow / total); out[17] = ftn_det::f2u(miss / total); out[18] = ftn_det::f2u(total);
    out[19] = ftn_det::f2u((float)n);
}
#undef IM_CSWAP

/* ftn_idmatte_select for one resolved pixel; ids: sorted ascending, n_ids of them */
FTN_HD float idmatte_select_pixel(const uint32_t* r, const uint32_t* ids, size_t n_ids, uint32_t flags) {
    float m = 0.0f;
#pragma unroll
    for (int k = 0; k < IM_SLOTS; k++) {
        const uint32_t x = r[2 * k];
        size_t lo = 0, hi = n_ids;                  /* first element >= x */
        while (lo < hi) { const size_t mid = lo + (hi - lo) / 2; if (ids[mid] < x) lo = mid + 1; else hi = mid; }
        if (lo < n_ids && ids[lo] == x) m += ftn_det::u2f(r[2 * k + 1]);
    }
    if (flags & 1u) m += ftn_det::u2f(r[16]);
    if (flags & 2u) m += ftn_det::u2f(r[17]);
    return m;
}

}  // namespace ftn
#endif
