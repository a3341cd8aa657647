/*
 * ftn_wf_trace.hip -- traversal for the wavefront pipeline in the reference's order (Scene::intersect / intersect_test, bvh.rs:160-266):
 *
 *   k_wf_trace<ANY>  Persistent 256-thread workgroups; each wave64 pulls rays from the queue in chunks (one atomic per chunk) and re-arms
 *                    idle lanes by __ballot / __popcll ranks: lanes whose ray finished get a new one while the others keep walking.
 *                    Per-lane node stack in LDS, [level][lane] interleaved.  The queue is cut into one slice per XCD.
 *   k_wf_trace_any2  any-hit walk (shadow rays, MIS rays toward infinite lights) over two boxes per step from 64-byte records, children in
 *                    the order that ends blocked rays soonest -- a boolean does not depend on the order
 *   k_wf_ray_keys + rocPRIM radix sort: orders a ray queue by Morton(origin cell) | direction octant (coherence); the only unit with hipcub
 *
 * launch_trace chooses between these and the production kernels over four-box records (ftn_trace4.hip), whose handed-back rays k_wf_trace
 * takes.  wavefront_trace_batch (ftn_intersect*) runs the same launches over a plain list of rays.
 */
#include "ftn_wf_internal.h"
#include <algorithm>
#include <cstring>
#include <string>
#include <hipcub/hipcub.hpp>

namespace ftn {

/* ------------------------------------------------------------------ trace
 * Per lane: mode 0 = needs a ray, 1 = at a BVH node, 2 = holds a leaf whose primitives are still to be tested.
 * A wave alternates between two cheap, convergent bodies instead of running the (long) triangle test for the two or three
 * lanes that happen to sit on a leaf at every step:
 *     node step   for all lanes in mode 1                         (~40 VALU instructions)
 *     leaf step   for all lanes in mode 2, once >= leaf_batch lanes wait there or no lane is left in mode 1
 * The visiting order of every single ray is exactly the reference's (bvh.rs:160-266): near child first, the far child is
 * re-tested against the shrunken t_max when popped, leaf primitives in order, `t == t_max` accepted.
 * Rays are taken from the queue in per-wave chunks (one global atomic per `chunk` rays) and lanes are re-armed from the chunk
 * with __ballot / __popcll prefix ranks as soon as `refill` of them are idle. */
enum : uint32_t { TM_IDLE = 0, TM_NODE = 1, TM_LEAF = 2 };

template <bool ANY, bool COUNT, bool SPHERES, int BURST /* 0: node_burst is a runtime value */>
__global__ void __launch_bounds__(256) k_wf_trace(DScene S, WfBuffers W, const uint32_t* __restrict__ queue, const uint32_t* count_ptr, uint32_t* head,
                                                  DevStats* stats, uint32_t refill, uint32_t leaf_batch, uint32_t chunk, uint32_t node_burst) {
    extern __shared__ uint32_t lds_stack[];
    uint32_t* const st_base = lds_stack + threadIdx.x;      /* [level][lane]; the stack pointer is kept as an LDS address */
    uint32_t* sptr = st_base;
    const uint32_t count = *count_ptr;
    const uint32_t lane = lane_id();
    const uint32_t np = W.n_paths;
    TravCount tc{0, 0};
    uint32_t w_idle_lanes = 0, w_leafwait_lanes = 0;
    uint32_t w_node_steps = 0, w_leaf_steps = 0;   /* COUNT only: wave-level step counts -> SIMD lane utilisation (FTN_WF_DEBUG) */
    uint32_t mode = TM_IDLE;
    uint32_t chunk_next = 0, chunk_end = 0; bool exhausted = count == 0;
    /* The queue is cut into 8 contiguous slices, one per XCD (workgroups b and b + 8 share an XCD and therefore an L2): with the
     * queue sorted by origin cell, an XCD's L2 only has to hold the part of the BVH its slice of space reaches.  A wave whose slice
     * has run dry moves on to the next one, so the partition costs no load balance. */
    uint32_t slice = blockIdx.x & 7u, slices_done = 0;
    /* per-wave chunk: few queue-head atomics, but small enough that the tail spreads over all waves */
    { uint32_t c = count / (gridDim.x * 4u * 16u); c &= ~63u; chunk = c < 64u ? 64u : (c > chunk ? chunk : c); }
    uint32_t rid = 0, cur = 0 /* byte offset of the node record */, neg16 = 0, lp = 0, lp_end = 0;
    V3 o, inv, dperm; float t_max = 0.0f, sx = 0.0f, sy = 0.0f, sz = 0.0f; int kz = 0;
    int hprim = -1; float hb0 = 0.0f, hb1 = 0.0f, hb2 = 0.0f; bool found = false;
    V3 dorig;   /* only the sphere path needs the unpermuted direction */
    for (;;) {
        /* ---- re-arm idle lanes */
        const unsigned long long idle = __ballot(mode == TM_IDLE);
        if (!exhausted && (uint32_t)__popcll(idle) >= refill) {
            const uint32_t need = (uint32_t)__popcll(idle);
            while (chunk_next == chunk_end && !exhausted) {      /* the wave's chunk is used up: take a new one from the current slice */
                const uint32_t s_lo = (uint32_t)(((unsigned long long)count * slice) >> 3) & ~63u, s_hi = slice == 7u ? count : ((uint32_t)(((unsigned long long)count * (slice + 1u)) >> 3) & ~63u);
                uint32_t base = 0;
                if (lane == 0) base = atomicAdd(head + CTR(slice), chunk);
                base = __shfl(base, 0, 64) + s_lo;
                if (base >= s_hi) {                                       /* this slice is empty: help the next XCD's */
                    slice = (slice + 1u) & 7u;
                    if (++slices_done == 8u) {
                        exhausted = true;
                        /* the launch starts to drain: let the stream that waits for it (the any-hit trace) go ahead */
                        if (!ANY && W.drain_sig && lane == 0 && atomicAdd(&W.counters[CTR(WFC_DRY_WAVES)], 1u) + 1u == W.drain_at)      /* the drain_at-th wave of this launch */
                            __hip_atomic_store(W.drain_sig, W.drain_seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);          /* a timing hint only: no data is handed over */
                    }
                }
                else { chunk_next = base; chunk_end = base + chunk < s_hi ? base + chunk : s_hi; }
            }
            const uint32_t avail = chunk_end - chunk_next;
            const uint32_t rank = (uint32_t)__popcll(idle & ((1ull << lane) - 1ull));
            if (mode == TM_IDLE && rank < avail) {
                float4 a, b;
                load_queued_ray<ANY>(W, queue[chunk_next + rank], &a, &b, &rid);      /* rid: the result slot of this ray from here on */
                o = V3(a.x, a.y, a.z); const V3 d(b.x, b.y, b.z); t_max = b.w;
                if (SPHERES) dorig = d;
                inv = V3(1.0f / d.x, 1.0f / d.y, 1.0f / d.z);
                neg16 = (d.x < 0.0f ? 0x10000u : 0u) | (d.y < 0.0f ? 0x20000u : 0u) | (d.z < 0.0f ? 0x40000u : 0u);   /* dir_is_neg, aligned with the node's one-hot axis */
                /* Triangle::intersect's per-ray constants (triangle.rs:189-205): permutation and shear depend on the ray only */
                kz = max_dimension(vabs(d));
                { const int kx = kz == 2 ? 0 : kz + 1, ky = kx == 2 ? 0 : kx + 1; dperm = V3(d.get(kx), d.get(ky), d.get(kz)); }
                sx = -dperm.x / dperm.z; sy = -dperm.y / dperm.z; sz = 1.0f / dperm.z;
                sptr = st_base; cur = 0; found = false; hprim = -1; hb0 = 0.0f; hb1 = 0.0f; hb2 = 0.0f;
                mode = TM_NODE;
                if (S.n_nodes == 0) {   /* empty scene: immediate miss */
                    if (ANY) store_occluded(W, rid, false); else { W.hit[rid] = make_float4(FTN_INF, 0.0f, 0.0f, 0.0f); W.hit_prim[rid] = -1; }
                    mode = TM_IDLE;
                }
            }
            chunk_next += (need < avail ? need : avail);
        }
        const unsigned long long m_node = __ballot(mode == TM_NODE), m_leaf = __ballot(mode == TM_LEAF);
        if ((m_node | m_leaf) == 0) { if (exhausted) break; else continue; }
        bool finish = false;
        if (m_node != 0 && (uint32_t)__popcll(m_leaf) < leaf_batch) {
            /* ---- node steps: `node_burst` of them per control round (lanes that reach a leaf or finish sit out the rest) */
#pragma unroll
            for (uint32_t burst = 0; burst < (BURST ? (uint32_t)BURST : node_burst); burst++) {
                if (COUNT && __ballot(mode == TM_NODE && !finish) != 0) { w_node_steps++; w_idle_lanes += (uint32_t)__popcll(__ballot(mode == TM_IDLE || finish)); w_leafwait_lanes += (uint32_t)__popcll(__ballot(mode == TM_LEAF)); }
                if (mode == TM_NODE && !finish) {
                    const float4* rec = reinterpret_cast<const float4*>(reinterpret_cast<const char*>(S.nodes) + cur);
                    float4 na = rec[0], nb = rec[1];
                    pin4(na); pin4(nb);
                    if (COUNT) tc.nodes++;
                    bool pop = true;
                    if (slab_test_node(na, nb, o, inv, t_max)) {
                        const uint32_t idx = __float_as_uint(nb.z), meta = __float_as_uint(nb.w);
                        if (meta >> 24) { lp = idx; lp_end = idx + (meta & 0xffffu); mode = TM_LEAF; pop = false; }
                        else {
                            if (meta & neg16) { *sptr = cur + 32u; cur = idx; }      /* dir_is_neg[axis]: second child first */
                            else { *sptr = idx; cur = cur + 32u; }
                            sptr += 256;
                            pop = false;
                        }
                    }
                    if (pop) { if (sptr == st_base) finish = true; else { sptr -= 256; cur = *sptr; } }
                }
            }
        } else {
            /* ---- leaf step: one primitive per lane */
            if (COUNT) w_leaf_steps++;
            if (mode == TM_LEAF) {
                const uint32_t prim = lp;
                float4 g0 = S.geom[S.geom_stride * prim], g1 = S.geom[S.geom_stride * prim + 1], g2 = S.geom[S.geom_stride * prim + 2];
                pin4(g0); pin4(g1); pin4(g2);
                if (COUNT) tc.prims++;
                float t = 0.0f, b0 = 0.0f, b1 = 0.0f, b2 = 0.0f;
                const bool hh = prim_hit<SPHERES>(S, prim, g0, g1, g2, o, dorig, t_max, kz, sx, sy, sz, &t, &b0, &b1, &b2);
                if (hh) { found = true; t_max = t; hprim = (int)prim; hb0 = b0; hb1 = b1; hb2 = b2; }
                lp++;
                if (ANY && hh) finish = true;
                else if (lp == lp_end) { if (sptr == st_base) finish = true; else { sptr -= 256; cur = *sptr; mode = TM_NODE; } }
            }
        }
        if (finish) {
            if (ANY) store_occluded(W, rid, found);
            else { W.hit[rid] = make_float4(found ? t_max : FTN_INF, hb0, hb1, hb2); W.hit_prim[rid] = hprim; }
            mode = TM_IDLE;
        }
    }
    if (COUNT) {
        unsigned long long n = tc.nodes, p = tc.prims;
        for (int off = 32; off > 0; off >>= 1) { n += __shfl_down(n, off, 64); p += __shfl_down(p, off, 64); }
        if (lane == 0) {
            if (n) atomicAdd(&stats->nodes_visited, n); if (p) atomicAdd(&stats->prims_tested, p);
            if (ANY) { if (n) atomicAdd(&stats->nodes_any, n); if (p) atomicAdd(&stats->prims_any, p); }
            atomicAdd(&W.counters[CTR(WFC_NODE_STEPS)], w_node_steps); atomicAdd(&W.counters[CTR(WFC_LEAF_STEPS)], w_leaf_steps);
            atomicAdd(&W.counters[CTR(WFC_IDLE_LANES)], w_idle_lanes >> 6); atomicAdd(&W.counters[CTR(WFC_LEAFWAIT_LANES)], w_leafwait_lanes >> 6);     /* in units of 64 lanes */
        }
    }
    if (stats && blockIdx.x == 0 && threadIdx.x == 0) { if (ANY) atomicAdd(&stats->rays_any, (unsigned long long)count); else atomicAdd(&stats->rays_closest, (unsigned long long)count); }   /* (NULL: the rays were counted by the kernel that handed them over) */
}

/* ------------------------------------------------------------------ any-hit traversal over two-box records
 *
 * Scene::intersect_test returns a boolean, and t_max never shrinks while it walks: whether a box or a triangle is reached does not
 * depend on the order of the walk.  So the any-hit kernel is free to test BOTH children of an interior node in one step from one
 * 64-byte record (DScene::fat: the two children's node records side by side) and to descend only into children whose box the ray
 * enters -- a node that fails its test is never fetched, and a step advances two levels' worth of box tests per memory round trip.
 * (For closest hits the far child must be re-tested against the shrunken t_max when it is popped; carrying its entry distance on
 * the stack doubles the LDS per lane and was measured slower, see DESIGN.md.)  The stack entry is one word: byte offset of an
 * interior child's record, or first primitive | bit 31 for a leaf child; leaf primitives are walked until GF_LEAF_END.
 * The counting build keeps k_wf_trace<ANY> (the reference's walk) so that node tallies equal the oracle's. */
template <bool SPHERES>
__global__ void __launch_bounds__(256) k_wf_trace_any2(DScene S, WfBuffers W, const uint32_t* __restrict__ queue, const uint32_t* count_ptr, uint32_t* head,
                                                       DevStats* stats, uint32_t refill, uint32_t leaf_batch, uint32_t chunk, uint32_t policy) {
    extern __shared__ uint32_t lds_stack[];
    uint32_t* const st_base = lds_stack + threadIdx.x;
    uint32_t* sptr = st_base;
    const uint32_t count = *count_ptr;
    const uint32_t lane = lane_id();
    uint32_t mode = TM_IDLE;
    uint32_t chunk_next = 0, chunk_end = 0; bool exhausted = count == 0;
    uint32_t slice = blockIdx.x & 7u, slices_done = 0;                     /* one queue slice per XCD, see k_wf_trace */
#ifdef FTN_DRAIN_PROBE      /* experiment build (tools/gpu_drain_probe.py): when does the first / last wave find the queue dry, when does the launch end */
    const uint32_t t_start = (uint32_t)wall_clock64(); uint32_t t_dry = t_start; bool seen_dry = false;
#endif
    { uint32_t c = count / (gridDim.x * 4u * 16u); c &= ~63u; chunk = c < 64u ? 64u : (c > chunk ? chunk : c); }
    uint32_t rid = 0, cur = 0, neg16 = 0, lp = 0;
    V3 o, inv, dperm; float t_max = 0.0f, sx = 0.0f, sy = 0.0f, sz = 0.0f; int kz = 0;
    bool found = false;
    V3 dorig;
    const float4 rlo = make_float4(S.root_lo[0], S.root_lo[1], S.root_lo[2], 0.0f), rhi = make_float4(S.root_hi[0], S.root_hi[1], S.root_hi[2], 0.0f);
    for (;;) {
        const unsigned long long idle = __ballot(mode == TM_IDLE);
        if (!exhausted && (uint32_t)__popcll(idle) >= refill) {
            const uint32_t need = (uint32_t)__popcll(idle);
            while (chunk_next == chunk_end && !exhausted) {
                const uint32_t s_lo = (uint32_t)(((unsigned long long)count * slice) >> 3) & ~63u, s_hi = slice == 7u ? count : ((uint32_t)(((unsigned long long)count * (slice + 1u)) >> 3) & ~63u);
                uint32_t base = 0;
                if (lane == 0) base = atomicAdd(head + CTR(slice), chunk);
                base = __shfl(base, 0, 64) + s_lo;
                if (base >= s_hi) { slice = (slice + 1u) & 7u; if (++slices_done == 8u) exhausted = true; }
                else { chunk_next = base; chunk_end = base + chunk < s_hi ? base + chunk : s_hi; }
            }
            const uint32_t avail = chunk_end - chunk_next;
            const uint32_t rank = (uint32_t)__popcll(idle & ((1ull << lane) - 1ull));
            if (mode == TM_IDLE && rank < avail) {
                float4 a, b;
                load_queued_ray<true>(W, queue[chunk_next + rank], &a, &b, &rid);
                o = V3(a.x, a.y, a.z); const V3 d(b.x, b.y, b.z); t_max = b.w;
                if (SPHERES) dorig = d;
                inv = V3(1.0f / d.x, 1.0f / d.y, 1.0f / d.z);
                neg16 = (d.x < 0.0f ? 0x10000u : 0u) | (d.y < 0.0f ? 0x20000u : 0u) | (d.z < 0.0f ? 0x40000u : 0u);
                kz = max_dimension(vabs(d));
                { const int kx = kz == 2 ? 0 : kz + 1, ky = kx == 2 ? 0 : kx + 1; dperm = V3(d.get(kx), d.get(ky), d.get(kz)); }
                sx = -dperm.x / dperm.z; sy = -dperm.y / dperm.z; sz = 1.0f / dperm.z;
                sptr = st_base; cur = 0; found = false;
                /* the root's own box test (bvh.rs:228-230) */
                if (S.n_nodes == 0 || !slab_test(rlo, rhi, o, inv, t_max)) { store_occluded(W, rid, false); mode = TM_IDLE; }
                else if (S.root_is_leaf) { lp = 0; mode = TM_LEAF; }
                else mode = TM_NODE;
            }
            chunk_next += (need < avail ? need : avail);
        }
        const unsigned long long m_node = __ballot(mode == TM_NODE), m_leaf = __ballot(mode == TM_LEAF);
#ifdef FTN_DRAIN_PROBE
        if (exhausted && !seen_dry) { seen_dry = true; t_dry = (uint32_t)wall_clock64(); }
#endif
        if ((m_node | m_leaf) == 0) { if (exhausted) break; else continue; }
        bool finish = false;
        if (m_node != 0 && (uint32_t)__popcll(m_leaf) < leaf_batch) {
#pragma unroll
            for (uint32_t burst = 0; burst < 8u; burst++) {
                if (mode == TM_NODE && !finish) {
                    const float4* rec = reinterpret_cast<const float4*>(reinterpret_cast<const char*>(S.fat) + cur);
                    float4 a0 = rec[0], b0 = rec[1], a1 = rec[2], b1 = rec[3];
                    pin4(a0); pin4(b0); pin4(a1); pin4(b1);
                    float i00, i01, i10, i11;
                    const bool h0 = slab_test_node_iv(a0, b0, o, inv, t_max, &i00, &i01), h1 = slab_test_node_iv(a1, b1, o, inv, t_max, &i10, &i11);
                    const uint32_t m0 = __float_as_uint(b0.w), m1 = __float_as_uint(b1.w);
                    /* stack / next entries: byte offset of the child's record, or first primitive | bit 31 for a leaf child */
                    const uint32_t e0 = __float_as_uint(b0.z) | ((m0 >> 24) ? 0x80000000u : 0u), e1 = __float_as_uint(b1.z) | ((m1 >> 24) ? 0x80000000u : 0u);
                    /* Which child first is a free choice here (the boolean does not depend on it) and it matters: a ray that is blocked at
                     * all ends at its first hit.  Measured on the config-5 scene, per step: reference order (near side of the split plane
                     * first, policy 0) 34.3 ms; far side first (1) 32.1 ms -- shadow and MIS rays start on a surface, what blocks them
                     * tends to lie ahead rather than around the origin; the child whose box the ray stays in longest first (2) 31.9 ms;
                     * leaf-child-first, interior-child-first, shortest stay, larger entry / exit distance first: slower or equal. */
                    const bool second_first = (policy & 0xffu) == 2u ? (i11 - i10) > (i01 - i00) : (((m0 & neg16) != 0) != ((policy & 0xffu) == 1u));
                    const uint32_t en = second_first ? e1 : e0, ef = second_first ? e0 : e1;
                    const bool hn = second_first ? h1 : h0, hf = second_first ? h0 : h1;
                    uint32_t next = 0; bool have = true;
                    if (hn) { next = en; if (hf) { *sptr = ef; sptr += 256; } }
                    else if (hf) next = ef;
                    else if (sptr == st_base) { finish = true; have = false; }
                    else { sptr -= 256; next = *sptr; }
                    if (have) { if (next >> 31) { lp = next & 0x7fffffffu; mode = TM_LEAF; } else cur = next; }
                }
            }
        } else {
            if (mode == TM_LEAF) {
                const uint32_t prim = lp;
                float4 g0 = S.geom[S.geom_stride * prim], g1 = S.geom[S.geom_stride * prim + 1], g2 = S.geom[S.geom_stride * prim + 2];
                pin4(g0); pin4(g1); pin4(g2);
                float t = 0.0f, b0 = 0.0f, b1 = 0.0f, b2 = 0.0f;
                const bool hh = prim_hit<SPHERES>(S, prim, g0, g1, g2, o, dorig, t_max, kz, sx, sy, sz, &t, &b0, &b1, &b2);
                if (hh) { found = true; finish = true; }
                else if (__float_as_uint(g0.w) & GF_LEAF_END) {
                    if (sptr == st_base) finish = true;
                    else { sptr -= 256; const uint32_t next = *sptr; if (next >> 31) lp = next & 0x7fffffffu; else { cur = next; mode = TM_NODE; } }
                } else lp++;
            }
        }
        if (finish) { store_occluded(W, rid, found); mode = TM_IDLE; }
    }
#ifdef FTN_DRAIN_PROBE
    if (lane == 0) {
        uint32_t* T = &W.counters[CTR(WFC_DRAIN_PROBE) + 4 * ((policy >> 8) & 7u)];             /* one slot of four words per bounce */
        atomicMax(&T[0], ~t_start); atomicMax(&T[1], ~t_dry); atomicMax(&T[2], t_dry); atomicMax(&T[3], (uint32_t)wall_clock64());
    }
#endif
    if (blockIdx.x == 0 && threadIdx.x == 0) atomicAdd(&stats->rays_any, (unsigned long long)count);
}

/* ------------------------------------------------------------------ coherence sort of the secondary-ray queues
 * After a bounce the queues hold rays in shading order: origins of neighbouring entries are still close, directions are not.
 * Sorting a queue by (Morton code of the origin's cell in the world box, direction octant) puts rays that walk the same part of
 * the BVH into the same wave, so a node record fetched by one lane is an L1 / L2 hit for its neighbours.  Measured on the config-5
 * scene: secondary closest-hit launches 18.1 -> 14.1 ms per step, shadow launches 8.4 -> 7.6 ms, for ~1.3 ms of sorting
 * (key kernel + rocPRIM radix sort of (key, ray id) pairs, 24 significant bits).  The order in which rays are traced does not
 * change any result (every ray writes its own hit record), so parity is untouched.  FTN_WF_SORT=0 disables it. */
__device__ inline uint32_t spread3(uint32_t v) {   /* 10 bits -> every third bit */
    v &= 0x3ffu; v = (v | (v << 16)) & 0x030000ffu; v = (v | (v << 8)) & 0x0300f00fu; v = (v | (v << 4)) & 0x030c30c3u; v = (v | (v << 2)) & 0x09249249u; return v;
}
template <bool ANY>
__global__ void __launch_bounds__(256) k_wf_ray_keys(DScene S, WfBuffers W, const uint32_t* __restrict__ queue, uint32_t count, uint32_t* __restrict__ keys, uint32_t bits) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= count) return;
    float4 a, b; uint32_t slot;
    load_queued_ray<ANY>(W, queue[i], &a, &b, &slot);
    const float ex = S.root_hi[0] - S.root_lo[0], ey = S.root_hi[1] - S.root_lo[1], ez = S.root_hi[2] - S.root_lo[2];
    const float sc = (float)(1u << bits);
    const float fx = fminf(fmaxf((a.x - S.root_lo[0]) / ex, 0.0f), 0.999f) * sc, fy = fminf(fmaxf((a.y - S.root_lo[1]) / ey, 0.0f), 0.999f) * sc, fz = fminf(fmaxf((a.z - S.root_lo[2]) / ez, 0.0f), 0.999f) * sc;
    const uint32_t m = spread3((uint32_t)fx) | (spread3((uint32_t)fy) << 1) | (spread3((uint32_t)fz) << 2);       /* NaN / inf -> cell 0: still a valid key */
    const uint32_t oct = (b.x < 0.0f ? 1u : 0u) | (b.y < 0.0f ? 2u : 0u) | (b.z < 0.0f ? 4u : 0u);
    keys[i] = (m << 3) | oct;
}

/* sorts queue[0, cnt) by the rays' coherence keys into `out`; *sorted_q = out (or the queue itself when it is too short to bother) */
int sort_ray_queue(WavefrontState* st, const RenderParams& P, const WfBuffers& W, bool any, uint32_t* queue, uint32_t cnt, uint32_t* out,
                   uint32_t* k_in, uint32_t* k_out, uint32_t bits, hipStream_t stream, const uint32_t** sorted_q) {
    *sorted_q = queue;
    if (cnt < knob("FTN_WF_SORT_MIN", 16384u)) return FTN_OK;             /* short queues: the launch overhead of the sort outweighs its gain */
    if (any) hipLaunchKernelGGL(k_wf_ray_keys<true>, dim3((cnt + 255) / 256), dim3(256), 0, stream, P.S, W, queue, cnt, k_in, bits);
    else hipLaunchKernelGGL(k_wf_ray_keys<false>, dim3((cnt + 255) / 256), dim3(256), 0, stream, P.S, W, queue, cnt, k_in, bits);
    const int end_bit = (int)(3 * bits + 3);
    size_t need = 0;
    hipcub::DoubleBuffer<uint32_t> keys(k_in, k_out), vals(queue, out);      /* both halves are scratch: the sort ping-pongs instead of copying */
    WF_TRY(hipcub::DeviceRadixSort::SortPairs(nullptr, need, keys, vals, (int)cnt, 0, end_bit, stream));
    { const int rc = wf_grow(&st->sort_tmp, &st->sort_tmp_bytes, need); if (rc) return rc; }
    WF_TRY(hipcub::DeviceRadixSort::SortPairs(st->sort_tmp, need, keys, vals, (int)cnt, 0, end_bit, stream));
    *sorted_q = vals.Current();
    return FTN_OK;
}

#ifdef FTN_DRAIN_PROBE
static uint32_t g_probe_bounce = 0;
void wf_set_probe_bounce(uint32_t bounce) { g_probe_bounce = bounce; }
#endif

/* Sizes the four-box kernels' launches for this call (LDS levels -> occupancy, persistent grid) and makes sure their spill areas exist.
 * FTN_TRACE4=0 or a scene without four-box records: the two-record kernels run. */
int trace4_prepare(WavefrontState* st, const DScene& S) {
    st->t4_on = S.quad != nullptr && knob("FTN_TRACE4", 1) != 0;
    if (!st->t4_on) return FTN_OK;
    st->t4 = trace4_plan(S, st->n_cu, knob("FTN_T4_ENTRIES", 0), knob("FTN_T4_ENTRIES_ANY", 0), knob("FTN_T4_WG", 0), knob("FTN_T4_WG_ANY", 0), knob("FTN_T8_WG", 0), knob("FTN_T8_ENTRIES", 0));
    /* 64-byte four-box records for the closest-hit rays of triangle-only scenes (FTN_QUAD64=0: the 128-byte records) */
    st->q64_on = st->t4.q64_ok && S.n_spheres == 0 && knob("FTN_QUAD64", 1) != 0;
    const size_t need_c = std::max<size_t>((size_t)st->t4.grid_closest * 256u * st->t4.spill_closest * sizeof(uint2),
                                           st->q64_on ? (size_t)st->t4.grid_q64 * 256u * st->t4.spill_q64 * sizeof(uint2) : 0);
    /* eight-box occlusion records for the any-hit rays of triangle-only scenes (FTN_T8=0: the four-box kernels trace them) */
    st->t8_on = st->t4.oct_ok && S.n_spheres == 0 && knob("FTN_T8", 1) != 0;
    const size_t need_a8 = st->t8_on ? (size_t)st->t4.grid_oct * 256u * st->t4.spill_oct * sizeof(uint32_t) : 0;
    const size_t need_a = std::max<size_t>(need_a8, (size_t)st->t4.grid_any * 256u * st->t4.spill_any * sizeof(uint32_t));
    int rc = wf_grow(&st->t4_spill_c, &st->t4_spill_c_bytes, need_c);
    if (!rc) rc = wf_grow(&st->t4_spill_a, &st->t4_spill_a_bytes, need_a);
    return rc;
}

/* count: 0 = production kernels, 1 = counting build of the REFERENCE walk (node / primitive tallies equal the oracle's), 2 = counting
 * build of the production kernels (what bench.py's byte model uses).  n_queue: upper bound of the queue's length (sizes the grid). */
void launch_trace(WavefrontState* st, bool any, int count, bool spheres, unsigned grid, size_t lds, hipStream_t stream, const RenderParams& P, const WfBuffers& W,
                  const uint32_t* queue, const uint32_t* count_ptr, uint32_t* head, uint32_t max_rays, bool camera_rays) {
    if (st->t4_on && count != 1) {     /* four-box records */
        const Trace4Plan& T = st->t4;
        const bool oct = any && st->t8_on, q64 = !any && st->q64_on;
        const unsigned g = std::min<unsigned>(oct ? T.grid_oct : (any ? T.grid_any : (q64 ? T.grid_q64 : T.grid_closest)), std::max<unsigned>(1u, (max_rays + 255u) / 256u));
        uint32_t chunk4 = knob("FTN_TRACE_CHUNK", 128);
        while (chunk4 > 64u && (uint64_t)chunk4 * g * 4u * 4u > (uint64_t)max_rays) chunk4 >>= 1;
        /* measured optima on the config-5 scene (profiles/r02_*, r03): lanes re-armed once 32 (closest, four-box any-hit) / 24 (eight-box any-hit)
         * are idle, leaf steps run once 16 lanes hold a leaf, 2 / 4 record steps per control round.
         * The camera rays' launch is the exception: its 64 rays per wave are four pixels' samples and walk the same records, so a wave that
         * re-arms only when ALL of its lanes are done keeps them in lockstep (every load of a step hits the same lines, the ray setup runs once
         * per 64 rays at full width): 46.2 -> 37.1 ms per step with FTN_T4_REFILL0 = 64, leaf steps as soon as 2 lanes hold a leaf, 3 record
         * steps per round (profiles/r03/n_*); at 60 instead of 64 the gain is gone, and the incoherent launches lose 50 % with it.  With
         * the pixels of a tile queued in 2 x 2 blocks (k_wf_generate) a pass of ONE sample per pixel gains too (a wave = an 8 x 8 block:
         * 25.5 -> 24.9 ms at 4096^2; with rows of 16 pixels it lost 2 %) */
        if (oct) launch_trace4(T4K_ANY_OCT, count == 2, false, g, T.lds_oct, T.entries_oct, st->t4_spill_a, stream, P.S, W, queue, count_ptr, head, P.stats,
                               camera_rays ? knob("FTN_T8_REFILL1", 16) : knob("FTN_T8_REFILL", 24), camera_rays ? knob("FTN_T8_LEAF_BATCH1", 16) : knob("FTN_T8_LEAF_BATCH", 16), chunk4, knob("FTN_T8_BURST", 2), knob("FTN_T8_POLICY", 1), T.spill_oct);
        else launch_trace4(any ? T4K_ANY : (q64 ? T4K_CLOSEST_Q64 : T4K_CLOSEST), count == 2, spheres, g, any ? T.lds_any : (q64 ? T.lds_q64 : T.lds_closest),
                      any ? T.entries_any : (q64 ? T.entries_q64 : T.entries_closest), any ? st->t4_spill_a : st->t4_spill_c, stream, P.S, W,
                      queue, count_ptr, head, P.stats,
                      any ? knob("FTN_T4_ANY_REFILL", 32) : (camera_rays ? knob("FTN_T4_REFILL0", 64) : knob("FTN_T4_REFILL", 32)),
                      any ? knob("FTN_T4_ANY_LEAF_BATCH", 16) : (camera_rays ? knob("FTN_T4_LEAF_BATCH0", 2) : knob("FTN_T4_LEAF_BATCH", 16)), chunk4,
                      any ? knob("FTN_T4_ANY_BURST", 4) : (camera_rays ? knob("FTN_T4_BURST0", 3) : knob("FTN_T4_BURST", 2)), knob("FTN_T4_ANY_POLICY", 1), any ? T.spill_any : (q64 ? T.spill_q64 : T.spill_closest));
        /* the rays it handed back (a zero direction component: ftn_trace4.hip, point 5) take the reference-order kernel.  The queue is
         * nearly always empty and the persistent workgroups leave at once; its rays are already in the statistics (stats = NULL) */
        const unsigned ge = std::min<unsigned>(grid, (unsigned)st->n_cu);
        uint32_t* ecount = &W.counters[CTR(any ? WFC_EXC_ANY : WFC_EXC_CLOSEST)]; uint32_t* ehead = &W.counters[CTR(any ? WFC_EXC_HEAD_ANY : WFC_EXC_HEAD_CLOSEST)];
        DevStats* none = nullptr;
#define FTN_TRE(A, Sp) hipLaunchKernelGGL((k_wf_trace<A, false, Sp, 8>), dim3(ge), dim3(256), lds, stream, P.S, W, any ? W.q_exc_any : W.q_exc_closest, ecount, ehead, none, 24u, 2u, 64u, 8u)
        if (any) { if (spheres) FTN_TRE(true, true); else FTN_TRE(true, false); } else { if (spheres) FTN_TRE(false, true); else FTN_TRE(false, false); }
#undef FTN_TRE
        return;
    }
    const bool count_b = count != 0;
    const uint32_t refill = knob("FTN_TRACE_REFILL", 24), leaf_batch = knob("FTN_TRACE_LEAF_BATCH", 2), chunk_knob = knob("FTN_TRACE_CHUNK", 128), node_burst = knob("FTN_TRACE_BURST", 8);
    /* per-wave chunk: large enough that queue-head atomics are rare, small enough that the tail spreads over all waves */
    uint32_t chunk = chunk_knob;
    const uint32_t waves = grid * 4u;
    while (chunk > 64u && (uint64_t)chunk * waves * 4u > (uint64_t)max_rays) chunk >>= 1;
    if (any && !count_b && knob("FTN_TRACE_ANY2", 1) && P.S.fat) {     /* any-hit rays: two boxes per step (k_wf_trace_any2) */
        const uint32_t refill2 = knob("FTN_ANY2_REFILL", 16), leaf_batch2 = knob("FTN_ANY2_LEAF_BATCH", leaf_batch);
        uint32_t policy2 = knob("FTN_ANY2_POLICY", 2);
#ifdef FTN_DRAIN_PROBE
        policy2 |= g_probe_bounce << 8;
#endif
        if (spheres) hipLaunchKernelGGL((k_wf_trace_any2<true>), dim3(grid), dim3(256), lds, stream, P.S, W, queue, count_ptr, head, P.stats, refill2, leaf_batch2, chunk, policy2);
        else hipLaunchKernelGGL((k_wf_trace_any2<false>), dim3(grid), dim3(256), lds, stream, P.S, W, queue, count_ptr, head, P.stats, refill2, leaf_batch2, chunk, policy2);
        return;
    }
    lds += knob("FTN_TRACE_LDS_PAD", 0);     /* experiment: lower the occupancy */
#define FTN_TR(A, C, Sp, B) hipLaunchKernelGGL((k_wf_trace<A, C, Sp, B>), dim3(grid), dim3(256), lds, stream, P.S, W, queue, count_ptr, head, P.stats, refill, leaf_batch, chunk, node_burst)
    const bool fixed = node_burst == 8 && !count_b && !knob("FTN_TRACE_NO_UNROLL", 0);      /* the default burst is compiled in (unrolled) */
    if (fixed) { if (any) { if (spheres) FTN_TR(true, false, true, 8); else FTN_TR(true, false, false, 8); } else { if (spheres) FTN_TR(false, false, true, 8); else FTN_TR(false, false, false, 8); } }
    else if (any) { if (count_b) { if (spheres) FTN_TR(true, true, true, 0); else FTN_TR(true, true, false, 0); } else { if (spheres) FTN_TR(true, false, true, 0); else FTN_TR(true, false, false, 0); } }
    else { if (count_b) { if (spheres) FTN_TR(false, true, true, 0); else FTN_TR(false, true, false, 0); } else { if (spheres) FTN_TR(false, false, true, 0); else FTN_TR(false, false, false, 0); } }
#undef FTN_TR
}

/* ------------------------------------------------------------------ Scene::intersect / intersect_test for arrays of rays (ftn_intersect*):
 * the same traversal kernel (and coherence sort) the renderer uses, over a queue that simply lists the rays */
__global__ void __launch_bounds__(256) k_batch_setup(const float* __restrict__ rays8, uint32_t n, float4* __restrict__ ray, uint32_t* __restrict__ queue) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const float* r = rays8 + 8 * (size_t)i;
    ray[2 * (size_t)i] = make_float4(r[0], r[1], r[2], r[7]);            /* o, time */
    ray[2 * (size_t)i + 1] = make_float4(r[3], r[4], r[5], r[6]);        /* d, t_max */
    queue[i] = i;
}
/* (k_batch_finish, which turns the hit records into what the caller gets, is in ftn_wf_shade.hip beside the other kernels that build
 * surface interactions) */
int wavefront_trace_batch(WavefrontState** state, const DScene& S, uint32_t stack_entries, const float* d_rays8, size_t n_rays, int mode, bool count,
                          float* t_hit, int* prim, float* bary, unsigned char* occluded, float* out24, DevStats* stats, hipStream_t stream) {
    if (n_rays == 0) return FTN_OK;
    if (n_rays >= (1ull << 31)) { wf_set_error("too many rays in one batch"); return FTN_ERR_INVALID_ARGUMENT; }
    knobs_begin();
    int rc = wf_state_init(state); if (rc) return rc;
    WavefrontState* st = *state;
    if ((rc = trace4_prepare(st, S))) return rc;
    const uint32_t n = (uint32_t)n_rays;
    const bool any = mode == 1;
    float4 *ray = nullptr, *hit = nullptr; int* hit_prim = nullptr; uint32_t *queue = nullptr, *scratch = nullptr, *counters = nullptr, *q_exc = nullptr;
    auto cleanup = [&]() { (void)hipFree(ray); (void)hipFree(hit); (void)hipFree(hit_prim); (void)hipFree(queue); (void)hipFree(scratch); (void)hipFree(counters); (void)hipFree(q_exc); };
#define WFB_TRY(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) { wf_set_error(std::string(#expr ": ") + hipGetErrorString(e_)); cleanup(); return e_ == hipErrorOutOfMemory ? FTN_ERR_OUT_OF_MEMORY : FTN_ERR_NO_DEVICE; } } while (0)
    WFB_TRY(hipMalloc((void**)&ray, (size_t)n * 32)); WFB_TRY(hipMalloc((void**)&queue, (size_t)n * 4)); WFB_TRY(hipMalloc((void**)&scratch, (size_t)n * 12));
    WFB_TRY(hipMalloc((void**)&counters, CTR(WFC_SLOTS) * 4)); WFB_TRY(hipMemsetAsync(counters, 0, CTR(WFC_SLOTS) * 4, stream));
    WFB_TRY(hipMalloc((void**)&q_exc, (size_t)n * 4));
    if (!any) { WFB_TRY(hipMalloc((void**)&hit, (size_t)n * 16)); WFB_TRY(hipMalloc((void**)&hit_prim, (size_t)n * 4)); }
    hipLaunchKernelGGL(k_batch_setup, dim3((n + 255) / 256), dim3(256), 0, stream, d_rays8, n, ray, queue);
    WFB_TRY(hipMemcpyAsync(&counters[CTR(any ? WFC_SHADOW : WFC_CLOSEST)], &n, 4, hipMemcpyHostToDevice, stream));
    WfBuffers W; memset(&W, 0, sizeof(W));
    W.n_paths = n; W.ray = ray; W.sh = ray; W.hit = hit; W.hit_prim = hit_prim; W.occluded = occluded; W.counters = counters; W.q_exc_closest = q_exc; W.q_exc_any = q_exc;
    RenderParams P; memset(&P, 0, sizeof(P)); P.S = S; P.stats = stats;
    const uint32_t* q = queue;
    if (knob("FTN_WF_SORT", 0)) { rc = sort_ray_queue(st, P, W, any, queue, n, scratch, scratch + n, scratch + 2 * (size_t)n, 7, stream, &q); if (rc) { cleanup(); return rc; } }
    const size_t lds = wf_trace_lds(stack_entries);
    const unsigned grid = std::min<unsigned>(wf_trace_grid_max(st, lds), (n + 255) / 256);
    launch_trace(st, any, count ? 1 : 0, S.n_spheres != 0, grid, lds, stream, P, W, q, &counters[CTR(any ? WFC_SHADOW : WFC_CLOSEST)], &counters[CTR(any ? WFC_HEAD_ANY : WFC_HEAD_CLOSEST)], n);
    if (!any) launch_batch_finish(S, d_rays8, n, hit, hit_prim, t_hit, prim, bary, out24, stream);
    WFB_TRY(hipStreamSynchronize(stream));
    WFB_TRY(hipGetLastError());
#undef WFB_TRY
    cleanup();
    return FTN_OK;
}

}  // namespace ftn
