/*
 * ftn_bvh_host.cpp -- BVH construction on the host (ftn_bvh_host.h): an exact restatement of the reference's BVH::build (src/bvh.rs:27-158),
 * serial and on host threads, the three record trees the traversal kernels walk (four-box, 64-byte four-box, eight-box), the host thread
 * budget, and the C entry points that hand the record trees of a flattened BVH to the tests.  Pure host code: nothing here needs a device.
 */
#include "ftn_bvh_host.h"

#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <limits>
#include <sched.h>

using namespace ftn;

/* ================================================================== BVH::build (bvh.rs:27-158), written directly in flattened DFS order */
namespace {

struct BvhBuilder {
    const std::vector<Aabb>& bounds;
    std::vector<float> own_centroid; std::vector<uint32_t> own_order;
    std::vector<float>& centroid;                                    /* 3 per prim */
    std::vector<uint32_t>& order;                                    /* permutation being partitioned */
    std::vector<ftn_bvh_node> nodes; std::vector<uint32_t> leaf_order; uint32_t max_depth = 0;
    size_t leaf_base = 0;                                            /* global position of this builder's first leaf primitive */
    /* sub-builder over a range of a parent's arrays (parallel build) */
    BvhBuilder(const std::vector<Aabb>& b, std::vector<float>& c, std::vector<uint32_t>& o, size_t base) : bounds(b), centroid(c), order(o), leaf_base(base) {}
    explicit BvhBuilder(const std::vector<Aabb>& b) : bounds(b), centroid(own_centroid), order(own_order) {
        size_t n = b.size(); centroid.resize(3 * n); order.resize(n);
        parallel_for(n, [&](size_t i0, size_t i1) { for (size_t i = i0; i < i1; i++) {
            order[i] = (uint32_t)i;
            for (int k = 0; k < 3; k++) centroid[3 * i + k] = b[i].lo[k] + ((b[i].hi[k] - b[i].lo[k]) / 2.0f);   /* Bounds3::centroid bounds.rs:160-162 */
        } });
    }
    void build(size_t lo, size_t hi, uint32_t depth) {               /* recursive_build :66-120 + flatten_tree :133-158 */
        if (depth > max_depth) max_depth = depth;
        Aabb nb = aabb_empty(), cb = aabb_empty();
        for (size_t i = lo; i < hi; i++) {
            const uint32_t p = order[i]; const Aabb& b = bounds[p];
            for (int k = 0; k < 3; k++) { nb.lo[k] = fmin_(nb.lo[k], b.lo[k]); nb.hi[k] = fmax_(nb.hi[k], b.hi[k]); cb.lo[k] = fmin_(cb.lo[k], centroid[3 * p + k]); cb.hi[k] = fmax_(cb.hi[k], centroid[3 * p + k]); }
        }
        ftn_bvh_node node; memset(&node, 0, sizeof(node));
        for (int k = 0; k < 3; k++) { node.bmin[k] = nb.lo[k]; node.bmax[k] = nb.hi[k]; }
        const size_t n = hi - lo;
        const bool is_point = cb.lo[0] == cb.hi[0] && cb.lo[1] == cb.hi[1] && cb.lo[2] == cb.hi[2];
        if (n == 1 || is_point) {
            node.is_leaf = 1; node.idx = (uint32_t)(leaf_base + leaf_order.size()); node.n_prims = (uint16_t)n;
            for (size_t i = lo; i < hi; i++) leaf_order.push_back(order[i]);
            nodes.push_back(node);
            return;
        }
        const float dx = cb.hi[0] - cb.lo[0], dy = cb.hi[1] - cb.lo[1], dz = cb.hi[2] - cb.lo[2];
        const int ax = (dx > dy && dx > dz) ? 0 : (dy > dz ? 1 : 2);                 /* maximum_extent bounds.rs:168-177 */
        const float mid = (cb.lo[ax] + cb.hi[ax]) / 2.0f;
        uint32_t* first = order.data() + lo; uint32_t* last = order.data() + hi;
        uint32_t* split = std::partition(first, last, [&](uint32_t p) { return centroid[3 * p + ax] < mid; });
        size_t m = (size_t)(split - first);
        if (m == 0 || m == n) {                                                    /* partition_equal_counts :122-131 */
            m = n / 2;
            std::nth_element(first, first + m, last, [&](uint32_t a, uint32_t b) { return centroid[3 * a + ax] < centroid[3 * b + ax]; });
        }
        node.is_leaf = 0; node.axis = (uint8_t)ax; node.idx = 0;
        const size_t my = nodes.size();
        nodes.push_back(node);
        build(lo, lo + m, depth + 1);
        nodes[my].idx = (uint32_t)nodes.size();                                    /* second_child_idx = my + first_subtree_len + 1 */
        build(lo + m, hi, depth + 1);
    }
};

/* Parallel driver for BvhBuilder: the top of the tree is split sequentially (same partitions as the serial build); every range
 * of at most `grain` primitives becomes a task that builds its subtree into a private BvhBuilder-style buffer; the buffers are then
 * stitched in DFS order with index fix-ups.  The result is identical to the serial build, node for node. */
struct ParallelBvh {
    BvhBuilder& B; size_t grain;
    struct Task { size_t lo, hi; uint32_t depth; std::vector<ftn_bvh_node> nodes; std::vector<uint32_t> leaf_order; uint32_t max_depth = 0; };
    struct Top { ftn_bvh_node node; int child[2]; bool is_task[2]; };
    std::vector<Task> tasks; std::vector<Top> tops;
    ParallelBvh(BvhBuilder& b, size_t g) : B(b), grain(g) {}
    /* returns (index, is_task) */
    std::pair<int, bool> split(size_t lo, size_t hi, uint32_t depth) {
        if (hi - lo <= grain) { Task t; t.lo = lo; t.hi = hi; t.depth = depth; tasks.push_back(std::move(t)); return {(int)tasks.size() - 1, true}; }
        Aabb nb = aabb_empty(), cb = aabb_empty();
        for (size_t i = lo; i < hi; i++) {
            const uint32_t p = B.order[i]; const Aabb& b = B.bounds[p];
            for (int k = 0; k < 3; k++) { nb.lo[k] = fmin_(nb.lo[k], b.lo[k]); nb.hi[k] = fmax_(nb.hi[k], b.hi[k]); cb.lo[k] = fmin_(cb.lo[k], B.centroid[3 * p + k]); cb.hi[k] = fmax_(cb.hi[k], B.centroid[3 * p + k]); }
        }
        const bool is_point = cb.lo[0] == cb.hi[0] && cb.lo[1] == cb.hi[1] && cb.lo[2] == cb.hi[2];
        if (is_point) { Task t; t.lo = lo; t.hi = hi; t.depth = depth; tasks.push_back(std::move(t)); return {(int)tasks.size() - 1, true}; }   /* becomes one leaf */
        Top tp; memset(&tp.node, 0, sizeof(tp.node));
        for (int k = 0; k < 3; k++) { tp.node.bmin[k] = nb.lo[k]; tp.node.bmax[k] = nb.hi[k]; }
        const float dx = cb.hi[0] - cb.lo[0], dy = cb.hi[1] - cb.lo[1], dz = cb.hi[2] - cb.lo[2];
        const int ax = (dx > dy && dx > dz) ? 0 : (dy > dz ? 1 : 2);
        const float mid = (cb.lo[ax] + cb.hi[ax]) / 2.0f;
        uint32_t* first = B.order.data() + lo; uint32_t* last = B.order.data() + hi;
        uint32_t* sp = std::partition(first, last, [&](uint32_t p) { return B.centroid[3 * p + ax] < mid; });
        size_t m = (size_t)(sp - first), n = hi - lo;
        if (m == 0 || m == n) { m = n / 2; std::nth_element(first, first + m, last, [&](uint32_t a, uint32_t b) { return B.centroid[3 * a + ax] < B.centroid[3 * b + ax]; }); }
        tp.node.is_leaf = 0; tp.node.axis = (uint8_t)ax;
        const int me = (int)tops.size();
        tops.push_back(tp);
        auto c0 = split(lo, lo + m, depth + 1);
        auto c1 = split(lo + m, hi, depth + 1);
        tops[me].child[0] = c0.first; tops[me].is_task[0] = c0.second; tops[me].child[1] = c1.first; tops[me].is_task[1] = c1.second;
        return {me, false};
    }
    void run_tasks(int n_threads) {
        std::atomic<size_t> next{0};
        auto worker = [&]() {
            for (;;) {
                size_t k = next.fetch_add(1); if (k >= tasks.size()) break;
                Task& t = tasks[k];
                BvhBuilder sub(B.bounds, B.centroid, B.order, t.lo);      /* shares bounds / centroids / the order array (disjoint ranges) */
                sub.build(t.lo, t.hi, t.depth);
                t.nodes.swap(sub.nodes); t.leaf_order.swap(sub.leaf_order); t.max_depth = sub.max_depth;
            }
        };
        std::vector<std::thread> th;
        for (int i = 0; i < n_threads; i++) th.emplace_back(worker);
        for (auto& t : th) t.join();
    }
    /* stitch: offsets by one sequential DFS over the (small) top tree, then the copies in parallel */
    std::vector<size_t> task_off;
    size_t assign(int idx, bool is_task, size_t off) {
        if (is_task) { task_off[idx] = off; return off + tasks[idx].nodes.size(); }
        ftn_bvh_node& n = tops[idx].node;
        const size_t my = off;
        off = assign(tops[idx].child[0], tops[idx].is_task[0], off + 1);
        n.idx = (uint32_t)off;                                   /* second_child_idx */
        off = assign(tops[idx].child[1], tops[idx].is_task[1], off);
        top_off[idx] = my;
        return off;
    }
    std::vector<size_t> top_off;
    void stitch(std::pair<int, bool> root, int n_threads) {
        task_off.assign(tasks.size(), 0); top_off.assign(tops.size(), 0);
        const size_t total = assign(root.first, root.second, 0);
        B.nodes.resize(total); B.leaf_order.resize(B.order.size());
        for (size_t i = 0; i < tops.size(); i++) B.nodes[top_off[i]] = tops[i].node;
        std::atomic<size_t> next{0};
        auto worker = [&]() {
            for (;;) {
                size_t k = next.fetch_add(1); if (k >= tasks.size()) break;
                Task& t = tasks[k];
                const uint32_t base = (uint32_t)task_off[k];
                ftn_bvh_node* dst = B.nodes.data() + task_off[k];
                for (size_t i = 0; i < t.nodes.size(); i++) { ftn_bvh_node n = t.nodes[i]; if (!n.is_leaf) n.idx += base; dst[i] = n; }
                memcpy(B.leaf_order.data() + t.lo, t.leaf_order.data(), t.leaf_order.size() * sizeof(uint32_t));
                std::vector<ftn_bvh_node>().swap(t.nodes); std::vector<uint32_t>().swap(t.leaf_order);
            }
        };
        std::vector<std::thread> th;
        for (int i = 0; i < n_threads; i++) th.emplace_back(worker);
        for (auto& t : th) t.join();
        for (const Task& t : tasks) if (t.max_depth > B.max_depth) B.max_depth = t.max_depth;
    }
};

}  // namespace

/* ------------------------------------------------------------------ four-box records (DScene::quad): the SAME tree, two levels per record
 * One 128-byte record (= one cache line) per interior node R reached on even collapsed levels: the node records of R's grandchildren
 * side by side, slots [A0, A1, B0, B1] with A = R's first child (bvh.rs: the next node) and B = its second child.  A child that is a
 * leaf takes its pair's first slot itself (the second one is empty).  The traversal kernels (ftn_trace4.hip) test the four boxes of a
 * record in one step and never test A's and B's own boxes:
 *   - Bounds3f::intersect_test (bounds.rs:214-233) is monotone in the box -- every operation in it is a correctly rounded, monotone f32
 *     operation -- so a ray whose plane distances are all numbers and that enters a child's box enters its parent's box, for the same
 *     or any larger t_max: skipping the parent's test changes nothing the reference would have visited.  A NaN (0 * inf: a zero direction
 *     component with the origin on a bounding plane) drops a constraint from ONE of the two tests, so for such rays the skip is not
 *     exact: the kernels hand every ray with a zero / non-finite 1/d component, or overflowing plane distances, to the reference-order
 *     kernel through the exception queue (ftn_trace4.hip, point 5; ray_is_exceptional);
 *   - the reference's visiting order (near child first by dir_is_neg[split_axis], bvh.rs:187-196) of the four grandchildren follows from
 *     the three split axes of R, A and B, which the record carries.
 * Slot layout = the 32-byte node record of ftn_device.h: {min.x, max.x, min.y, max.y} {min.z, max.z, bits(link), bits(meta)};
 * link = the traversal stack's entry for the child: byte offset of an interior child's own record, or first primitive | bit 31 for a
 * leaf (its primitives run to the one flagged GF_LEAF_END in `geom`).  Slot 0's meta carries the three one-hot split axes that order
 * the visit, one per byte: byte 0 A's (orders slots 0 / 1), byte 1 R's (orders the pairs), byte 2 B's (orders slots 2 / 3) -- tested
 * against the ray's dir_is_neg bits repeated in the same bytes.  An empty slot (bit 25 of its meta, for tools) holds the box
 * x = y = [0, 0], z = [+inf, +inf], which no ray that passes ray_is_exceptional enters: the kernels need no test for it.
 * Returns the records in DFS order (slot order) and an upper bound of the traversal stack (entries pending at any time). */
void build_quads(const std::vector<ftn_bvh_node>& nodes, QuadBvh* out) {
    out->rec.clear(); out->n_records = 0; out->stack_bound = 0; out->ok = false;
    if (nodes.empty() || nodes[0].is_leaf) { out->ok = true; return; }          /* no interior node: the kernels test the root's leaf directly */
    /* pass 1: which interior nodes own a record, in DFS slot order (explicit stack: the tree can be 64 deep, the record tree 32) */
    std::vector<uint32_t> owner_id(nodes.size(), 0xffffffffu), owners;
    {
        std::vector<uint32_t> todo{0u};
        while (!todo.empty()) {
            const uint32_t r = todo.back(); todo.pop_back();
            owner_id[r] = (uint32_t)owners.size(); owners.push_back(r);
            uint32_t gc[4]; int ng = 0;
            const uint32_t ch[2] = {r + 1u, nodes[r].idx};
            for (int k = 0; k < 2; k++) if (!nodes[ch[k]].is_leaf) { gc[ng++] = ch[k] + 1u; gc[ng++] = nodes[ch[k]].idx; }
            for (int k = ng - 1; k >= 0; k--) if (!nodes[gc[k]].is_leaf) todo.push_back(gc[k]);      /* reversed: slot 0's subtree is numbered first */
        }
    }
    if (owners.size() >= (1u << 24)) return;                                   /* links are 31-bit byte offsets: 2^24 records of 128 bytes */
    out->n_records = (uint32_t)owners.size();
    out->rec.assign((size_t)32 * owners.size(), 0.0f);
    std::vector<uint32_t> bound(owners.size(), 0);
    const float kInf = std::numeric_limits<float>::infinity();
    auto put = [&](float* slot, const ftn_bvh_node* c, uint32_t c_index, uint32_t axis_bits) {
        uint32_t link = 0, meta = axis_bits;
        if (!c) { slot[0] = 0.0f; slot[1] = 0.0f; slot[2] = 0.0f; slot[3] = 0.0f; slot[4] = kInf; slot[5] = kInf; link = 0xffffffffu; meta |= 1u << 25; }      /* empty: fails every slab test */
        else {
            slot[0] = c->bmin[0]; slot[1] = c->bmax[0]; slot[2] = c->bmin[1]; slot[3] = c->bmax[1]; slot[4] = c->bmin[2]; slot[5] = c->bmax[2];
            if (c->is_leaf) { link = c->idx | 0x80000000u; meta |= 1u << 24; }
            else link = owner_id[c_index] * 128u;
        }
        slot[6] = ftn_det::u2f(link); slot[7] = ftn_det::u2f(meta);
    };
    /* the records: each from the nodes alone (host threads) */
    parallel_for(owners.size(), [&](size_t q0, size_t q1) {
        for (size_t q = q0; q < q1; q++) {
            const uint32_t r = owners[q];
            const uint32_t ch[2] = {r + 1u, nodes[r].idx};
            float* R = &out->rec[(size_t)32 * q];
            for (int k = 0; k < 2; k++) {
                const ftn_bvh_node& c = nodes[ch[k]];
                /* slot 0's meta: one-hot axes of A (byte 0), R (byte 1), B (byte 2); a leaf child has no axis (its pair has one member) */
                const uint32_t axes = k == 0 ? ((c.is_leaf ? 0u : (1u << c.axis)) | ((1u << nodes[r].axis) << 8) | ((nodes[ch[1]].is_leaf ? 0u : (1u << nodes[ch[1]].axis)) << 16)) : 0u;
                if (c.is_leaf) { put(R + 16 * k, &c, ch[k], axes); put(R + 16 * k + 8, nullptr, 0, 0u); }
                else { const uint32_t g0 = ch[k] + 1u, g1 = c.idx; put(R + 16 * k, &nodes[g0], g0, axes); put(R + 16 * k + 8, &nodes[g1], g1, 0u); }
            }
        }
    });
    /* the stack bound, bottom up */
    for (size_t q = owners.size(); q-- > 0;) {                                  /* children have larger ids: their bounds are known */
        const uint32_t r = owners[q];
        const uint32_t ch[2] = {r + 1u, nodes[r].idx};
        uint32_t valid = 0, deepest = 0;
        for (int k = 0; k < 2; k++) {
            const ftn_bvh_node& c = nodes[ch[k]];
            if (c.is_leaf) valid += 1;
            else {
                const uint32_t g0 = ch[k] + 1u, g1 = c.idx; valid += 2;
                if (!nodes[g0].is_leaf) deepest = std::max(deepest, bound[owner_id[g0]]);
                if (!nodes[g1].is_leaf) deepest = std::max(deepest, bound[owner_id[g1]]);
            }
        }
        bound[q] = (valid - 1u) + deepest;
    }
    out->stack_bound = bound[0];
    out->ok = true;
}

/* ------------------------------------------------------------------ eight-box occlusion records (DScene::oct): a SECOND tree over the same leaves, for
 * Scene::intersect_test only (k_wf_trace8_any, ftn_trace8.hip).
 * intersect_test (bvh.rs:217-266) never shrinks t_max and returns a boolean: a ray is occluded iff SOME leaf's own box passes the slab test
 * and one of its primitives passes its test (the boxes of the leaf's ancestors pass whenever the leaf's does -- the monotonicity argument of
 * build_quads).  Which interior boxes are tested on the way is therefore free, as long as every leaf whose box the ray enters is reached:
 * interior boxes may be LARGER than the reference's.  A record holds up to eight children of a collapsed subtree (an interior node's
 * children, the largest one replaced by its own children until eight are there) with their boxes quantised to 8 bits per plane on a
 * per-record grid (origin = the subtree's min corner, a power-of-two step per axis), rounded outwards: 96 bytes decide up to three
 * levels -- a walk fetches ~40 % fewer records than four-box records and half the bytes.  Leaves are tested exactly in the kernel: a
 * single triangle's leaf box is the min / max of its vertices (checked here against the reference's node), any other leaf carries its
 * exact box in `xbox`.
 * Record (32 words): [0..2] origin, [3] step exponents (biased, one byte per axis), [4..11] child links -- byte offset of the child's
 * record | 0, leaf: bit 31 | first primitive, leaf with an explicit box: bit 31 | bit 30 | index into xbox, empty: 0xffffffff --,
 * [12..23] planes, one byte per child: lo.x[8] hi.x[8] lo.y[8] hi.y[8] lo.z[8] hi.z[8]; [24..31] unused (one 128-byte line per record). */
void build_octs(const std::vector<ftn_bvh_node>& nodes, const std::vector<float4>& geom, OctBvh* out) {
    out->rec.clear(); out->xbox.clear(); out->n_records = 0; out->stack_bound = 0; out->ok = false;
    if (nodes.empty() || nodes[0].is_leaf) return;                                /* (a single leaf: the four-box path handles it) */
    auto area = [&](uint32_t i) { const ftn_bvh_node& n = nodes[i]; const double dx = (double)n.bmax[0] - n.bmin[0], dy = (double)n.bmax[1] - n.bmin[1], dz = (double)n.bmax[2] - n.bmin[2]; return 2.0 * (dx * dy + dy * dz + dz * dx); };
    struct Rec { uint32_t root; uint32_t child[8]; int n; };
    std::vector<Rec> recs; std::vector<uint32_t> rec_of(nodes.size(), 0xffffffffu);
    {   /* pass 1: collapse, records numbered in DFS order */
        std::vector<uint32_t> todo{0u};
        while (!todo.empty()) {
            const uint32_t r = todo.back(); todo.pop_back();
            Rec R; R.root = r; R.n = 2; R.child[0] = r + 1u; R.child[1] = nodes[r].idx;
            for (;;) {
                if (R.n == 8) break;
                int best = -1; double ba = -1.0;
                for (int k = 0; k < R.n; k++) if (!nodes[R.child[k]].is_leaf) { const double a = area(R.child[k]); if (a > ba) { ba = a; best = k; } }
                if (best < 0) break;
                const uint32_t c = R.child[best];
                R.child[best] = c + 1u; R.child[R.n++] = nodes[c].idx;
            }
            rec_of[r] = (uint32_t)recs.size(); recs.push_back(R);
            for (int k = R.n - 1; k >= 0; k--) if (!nodes[R.child[k]].is_leaf) todo.push_back(R.child[k]);
        }
    }
    if (recs.size() >= (1u << 24)) return;                                       /* links are byte offsets below 2^31 */
    out->rec.assign((size_t)32 * recs.size(), 0u);
    std::vector<uint32_t> bound(recs.size(), 0);
    /* which leaf children carry an explicit box (bit k of xmask[q]): every leaf that is not a single triangle whose node box is the min / max
     * of its vertices.  Their xbox slots are numbered in the order records are finished (last record first, children in slot order) */
    auto leaf_is_implicit = [&](const ftn_bvh_node& c) {
        if (c.n_prims != 1 || geom.empty()) return false;
        const float4 g0 = geom[(size_t)FTN_GS * c.idx], g1 = geom[(size_t)FTN_GS * c.idx + 1], g2 = geom[(size_t)FTN_GS * c.idx + 2];
        if (ftn_det::f2u(g0.w) & GF_KIND_SPHERE) return false;
        const float lo[3] = {std::min(std::min(g0.x, g1.x), g2.x), std::min(std::min(g0.y, g1.y), g2.y), std::min(std::min(g0.z, g1.z), g2.z)};
        const float hi[3] = {std::max(std::max(g0.x, g1.x), g2.x), std::max(std::max(g0.y, g1.y), g2.y), std::max(std::max(g0.z, g1.z), g2.z)};
        for (int a = 0; a < 3; a++) if (ftn_det::f2u(lo[a]) != ftn_det::f2u(c.bmin[a]) || ftn_det::f2u(hi[a]) != ftn_det::f2u(c.bmax[a])) return false;
        return true;
    };
    std::vector<uint8_t> xmask(recs.size(), 0);
    parallel_for(recs.size(), [&](size_t q0, size_t q1) {
        for (size_t q = q0; q < q1; q++) {
            const Rec& R = recs[q]; uint8_t m = 0;
            for (int k = 0; k < R.n; k++) { const ftn_bvh_node& c = nodes[R.child[k]]; if (c.is_leaf && !leaf_is_implicit(c)) m |= (uint8_t)(1u << k); }
            xmask[q] = m;
        }
    });
    std::vector<uint32_t> xbase(recs.size(), 0);
    { uint32_t run = 0; for (size_t q = recs.size(); q-- > 0;) { xbase[q] = run; run += (uint32_t)__builtin_popcount(xmask[q]); } out->xbox.assign(2 * (size_t)run, make_float4(0.0f, 0.0f, 0.0f, 0.0f)); }
    /* the records: each from the nodes alone (host threads) */
    parallel_for(recs.size(), [&](size_t q0, size_t q1) {
    for (size_t q = q0; q < q1; q++) {
        const Rec& R = recs[q];
        const ftn_bvh_node& root = nodes[R.root];
        uint32_t* W = &out->rec[(size_t)32 * q];
        uint32_t ebits[3]; float step[3];
        for (int a = 0; a < 3; a++) {
            /* the smallest power-of-two step that covers the subtree's extent with 255 steps -- one more if the outward rounding of a child
             * plane would not fit */
            const double ext = (double)root.bmax[a] - (double)root.bmin[a];
            int e = ext > 0.0 ? (int)ceil(log2(ext / 255.0)) : -126;
            if (e < -126) e = -126;
            for (;; e++) {
                bool fits = true;
                const float st = ldexpf(1.0f, e);
                for (int k = 0; k < R.n && fits; k++) {
                    const ftn_bvh_node& c = nodes[R.child[k]];
                    const double qh = ceil(((double)c.bmax[a] - (double)root.bmin[a]) / (double)st);
                    if (qh > 254.0) fits = false;                                 /* (one step of slack for the adjustment below) */
                }
                if (fits || e >= 126) break;
            }
            step[a] = ldexpf(1.0f, e); ebits[a] = (uint32_t)(e + 127);
            memcpy(&W[a], &root.bmin[a], 4);
        }
        W[3] = ebits[0] | (ebits[1] << 8) | (ebits[2] << 16);
        uint32_t xi = xbase[q];
        for (int k = 0; k < 8; k++) {
            uint32_t link = 0xffffffffu; uint32_t qb[6] = {255u, 0u, 255u, 0u, 255u, 0u};
            if (k < R.n) {
                const uint32_t ci = R.child[k]; const ftn_bvh_node& c = nodes[ci];
                for (int a = 0; a < 3; a++) {
                    /* decoded plane = origin + q * step, exactly as the kernel's bounds (real-number inequality: lo_dec <= lo, hi_dec >= hi) */
                    const double o = (double)root.bmin[a], stp = (double)step[a];
                    double ql = floor(((double)c.bmin[a] - o) / stp), qh = ceil(((double)c.bmax[a] - o) / stp);
                    while (ql > 0.0 && o + ql * stp > (double)c.bmin[a]) ql -= 1.0;
                    while (o + qh * stp < (double)c.bmax[a]) qh += 1.0;
                    if (ql < 0.0) ql = 0.0;
                    if (qh > 255.0) qh = 255.0;                                   /* (cannot happen: the step was chosen with slack) */
                    qb[2 * a] = (uint32_t)ql; qb[2 * a + 1] = (uint32_t)qh;
                }
                if (!c.is_leaf) link = rec_of[ci] * 128u;
                else if (!((xmask[q] >> k) & 1u)) link = 0x80000000u | c.idx;         /* a single triangle whose node box is the min / max of its vertices */
                else {
                    link = 0xc0000000u | xi;
                    out->xbox[2 * (size_t)xi] = make_float4(c.bmin[0], c.bmin[1], c.bmin[2], ftn_det::u2f(c.idx));
                    out->xbox[2 * (size_t)xi + 1] = make_float4(c.bmax[0], c.bmax[1], c.bmax[2], 0.0f);
                    xi++;
                }
            }
            W[4 + k] = link;
            for (int j = 0; j < 6; j++) W[12 + 2 * j + (k >> 2)] |= qb[j] << (8 * (k & 3));
        }
    }
    });
    /* the stack bound, bottom up */
    for (size_t q = recs.size(); q-- > 0;) {
        const Rec& R = recs[q]; uint32_t deepest = 0;
        for (int k = 0; k < R.n; k++) if (!nodes[R.child[k]].is_leaf) deepest = std::max(deepest, bound[rec_of[R.child[k]]]);
        bound[q] = (uint32_t)(R.n - 1) + deepest;
    }
    if (out->xbox.size() / 2 >= (1u << 30) || nodes.size() >= (1u << 30)) return;
    out->n_records = (uint32_t)recs.size(); out->stack_bound = bound[0]; out->ok = true;
}

/* ------------------------------------------------------------------ 64-byte four-box records (DScene::quad64): the records of build_quads with
 * their boxes quantised as build_octs quantises its own, for Scene::intersect in triangle-only scenes (k_wf_trace4<.., Q64>, ftn_trace4.hip).
 * Same tree, same slots, same DFS order, same stack bound: record q of the 128-byte array is record q here (links are byte offsets / 2).
 * A record step then needs four dwordx4 loads instead of eight.  Exactness of the closest-hit walk over conservative boxes:
 *   - interior boxes may be larger than the reference's: a child the ray does not truly enter is visited at most in vain -- every leaf under
 *     it fails its exact test later (monotone in the box and in t_max, which only shrinks);
 *   - the reference's visiting order is kept (the split axes of build_quads' slot a meta word);
 *   - every leaf, whether entered from its record or popped, is tested exactly on its true box with the t_max of that moment (bvh.rs:173)
 *     before its primitives: a single triangle whose node box is the min / max of its vertices by those vertices, any other leaf by its
 *     explicit box in `xbox` (bit 30 of its link).
 * Record (16 words): [0..2] origin = the min corner of the four slot boxes, [3] step exponents (biased, one byte per axis), [4..9] planes,
 * one byte per slot: lo.x hi.x lo.y hi.y lo.z hi.z, [10..13] slot links (interior: byte offset of the child's record; leaf: bit 31 | first
 * primitive, or bit 31 | bit 30 | index into xbox; empty: 0xffffffff), [14] the three one-hot split axes (bytes 0 A, 1 R, 2 B), [15] 0.
 * `geom` empty: every leaf gets an explicit box (the C entry point for tests has no vertices). */
void build_quad64s(const QuadBvh& qb, const std::vector<float4>& geom, Quad64Bvh* out) {
    out->rec.clear(); out->xbox.clear(); out->n_records = 0; out->stack_bound = 0; out->ok = false;
    if (!qb.ok || qb.n_records == 0) return;
    const size_t n = qb.n_records;
    auto slot = [&](size_t q, int s) { return &qb.rec[(size_t)32 * q + 8 * s]; };
    auto meta = [&](const float* S) { return ftn_det::f2u(S[7]); };
    /* a leaf slot whose box is its single triangle's min / max (build_octs' test; the first primitive flagged GF_LEAF_END: one primitive) */
    auto leaf_is_implicit = [&](const float* S) {
        const uint32_t p = ftn_det::f2u(S[6]) & 0x7fffffffu;
        if (geom.empty() || (size_t)FTN_GS * p + 2 >= geom.size()) return false;
        const float4 g0 = geom[(size_t)FTN_GS * p], g1 = geom[(size_t)FTN_GS * p + 1], g2 = geom[(size_t)FTN_GS * p + 2];
        const uint32_t fl = ftn_det::f2u(g0.w);
        if ((fl & GF_KIND_SPHERE) || !(fl & GF_LEAF_END)) return false;
        const float lo[3] = {std::min(std::min(g0.x, g1.x), g2.x), std::min(std::min(g0.y, g1.y), g2.y), std::min(std::min(g0.z, g1.z), g2.z)};
        const float hi[3] = {std::max(std::max(g0.x, g1.x), g2.x), std::max(std::max(g0.y, g1.y), g2.y), std::max(std::max(g0.z, g1.z), g2.z)};
        for (int a = 0; a < 3; a++) if (ftn_det::f2u(lo[a]) != ftn_det::f2u(S[2 * a]) || ftn_det::f2u(hi[a]) != ftn_det::f2u(S[2 * a + 1])) return false;
        return true;
    };
    std::vector<uint8_t> xmask(n, 0);
    parallel_for(n, [&](size_t q0, size_t q1) {
        for (size_t q = q0; q < q1; q++) {
            uint8_t m = 0;
            for (int s = 0; s < 4; s++) { const float* S = slot(q, s); if ((meta(S) >> 24) == 1u && !leaf_is_implicit(S)) m |= (uint8_t)(1u << s); }
            xmask[q] = m;
        }
    });
    std::vector<uint32_t> xbase(n, 0);
    { uint32_t run = 0; for (size_t q = 0; q < n; q++) { xbase[q] = run; run += (uint32_t)__builtin_popcount(xmask[q]); } out->xbox.assign(2 * (size_t)run, make_float4(0.0f, 0.0f, 0.0f, 0.0f)); }
    if (out->xbox.size() / 2 >= (1u << 30)) return;
    out->rec.assign((size_t)16 * n, 0u);
    std::atomic<bool> bad{false};
    parallel_for(n, [&](size_t q0, size_t q1) {
    for (size_t q = q0; q < q1; q++) {
        uint32_t* W = &out->rec[(size_t)16 * q];
        bool used[4];
        for (int s = 0; s < 4; s++) used[s] = !((meta(slot(q, s)) >> 25) & 1u);
        for (int a = 0; a < 3; a++) {
            /* origin and extent of the four boxes; the step as build_octs chooses it (smallest power of two that leaves one step of slack) */
            float org = FTN_INF, top = -FTN_INF;
            for (int s = 0; s < 4; s++) if (used[s]) { org = std::min(org, slot(q, s)[2 * a]); top = std::max(top, slot(q, s)[2 * a + 1]); }
            if (!(std::fabs(org) < FTN_INF && std::fabs(top) < FTN_INF)) { bad = true; break; }
            const double ext = (double)top - (double)org;
            int e = ext > 0.0 ? (int)ceil(log2(ext / 255.0)) : -126;
            if (e < -126) e = -126;
            for (;; e++) {
                const double st = ldexp(1.0, e);
                if (ceil(((double)top - (double)org) / st) <= 254.0 || e >= 126) break;
            }
            const double stp = ldexp(1.0, e), o = (double)org;
            memcpy(&W[a], &org, 4);
            W[3] |= (uint32_t)(e + 127) << (8 * a);
            for (int s = 0; s < 4; s++) {
                uint32_t ql = 255u, qh = 0u;                                               /* empty: lo > hi (its link alone keeps it out) */
                if (used[s]) {
                    /* decoded plane = origin + q * step, exact in double: lo_dec <= lo and hi_dec >= hi as real numbers */
                    const double lo = slot(q, s)[2 * a], hi = slot(q, s)[2 * a + 1];
                    double l = floor((lo - o) / stp), h = ceil((hi - o) / stp);
                    while (l > 0.0 && o + l * stp > lo) l -= 1.0;
                    while (o + h * stp < hi) h += 1.0;
                    if (l < 0.0 || h > 255.0 || o + l * stp > lo || o + h * stp < hi) { bad = true; break; }
                    ql = (uint32_t)l; qh = (uint32_t)h;
                }
                W[4 + 2 * a] |= ql << (8 * s); W[5 + 2 * a] |= qh << (8 * s);
            }
        }
        uint32_t xi = xbase[q];
        for (int s = 0; s < 4; s++) {
            const float* S = slot(q, s);
            const uint32_t link = ftn_det::f2u(S[6]), m = meta(S);
            uint32_t l = 0xffffffffu;
            if (!used[s]) l = 0xffffffffu;
            else if (!((m >> 24) & 1u)) l = link >> 1;                                   /* 128-byte record q -> 64-byte record q */
            else if (link & 0x40000000u) bad = true;                                      /* (bit 30 marks an explicit box) */
            else if (!((xmask[q] >> s) & 1u)) l = link;
            else {
                l = 0xc0000000u | xi;
                out->xbox[2 * (size_t)xi] = make_float4(S[0], S[2], S[4], ftn_det::u2f(link & 0x7fffffffu));
                out->xbox[2 * (size_t)xi + 1] = make_float4(S[1], S[3], S[5], 0.0f);
                xi++;
            }
            W[10 + s] = l;
        }
        W[14] = meta(slot(q, 0)) & 0x00ffffffu;
    }
    });
    if (bad) { out->rec.clear(); out->xbox.clear(); return; }
    out->n_records = (uint32_t)n; out->stack_bound = qb.stack_bound; out->ok = true;
}

static int bvh_default_threads() {
    int cores = (int)std::thread::hardware_concurrency();
#ifdef __linux__
    cpu_set_t set; CPU_ZERO(&set);
    if (sched_getaffinity(0, sizeof(set), &set) == 0) { const int c = CPU_COUNT(&set); if (c > 0) cores = c; }
#endif
    int ranks = 1;
    if (const char* e = getenv("LOCAL_WORLD_SIZE")) { const int r = atoi(e); if (r > 1) ranks = r; }
    return std::max(1, cores / ranks);
}

/* host threads for the per-element passes (parallel_for): this process's share of the host (bvh_default_threads), FTN_BVH_THREADS overrides */
int host_threads() {
    int n = bvh_default_threads();
    if (const char* e = getenv("FTN_BVH_THREADS")) n = atoi(e);
    return std::max(1, std::min(n, 32));
}

void build_bvh(const std::vector<Aabb>& bounds, HostScene* hs) {
    const size_t n_prims = bounds.size();
    BvhBuilder b(bounds);
    /* build threads: this process's share of the host -- the cores it may run on (affinity mask), divided by the ranks a launcher
     * started on this node (LOCAL_WORLD_SIZE: an 8-rank job builds eight scenes side by side), at most 32; FTN_BVH_THREADS overrides */
    int n_threads = bvh_default_threads();
    if (const char* e = getenv("FTN_BVH_THREADS")) n_threads = atoi(e);
    if (n_threads > 32) n_threads = 32;
    if (n_threads > 1 && n_prims >= (1u << 16)) {
        const bool dbg = getenv("FTN_BVH_DEBUG") != nullptr;
        auto t0 = std::chrono::steady_clock::now();
        ParallelBvh pb2(b, std::max<size_t>(4096, n_prims / (size_t)(n_threads * 8)));
        auto root = pb2.split(0, n_prims, 0);
        auto t1 = std::chrono::steady_clock::now();
        pb2.run_tasks(n_threads);
        auto t2 = std::chrono::steady_clock::now();
        pb2.stitch(root, n_threads);
        auto t3 = std::chrono::steady_clock::now();
        if (dbg) fprintf(stderr, "[ftn bvh] %d threads, %zu tasks: top split %.2fs, subtrees %.2fs, stitch %.2fs\n", n_threads, pb2.tasks.size(),
                         std::chrono::duration<double>(t1 - t0).count(), std::chrono::duration<double>(t2 - t1).count(), std::chrono::duration<double>(t3 - t2).count());
        /* depth of the top part */
        std::function<void(int, bool, uint32_t)> walk = [&](int i, bool t, uint32_t dep) { if (t) return; if (dep > b.max_depth) b.max_depth = dep; walk(pb2.tops[i].child[0], pb2.tops[i].is_task[0], dep + 1); walk(pb2.tops[i].child[1], pb2.tops[i].is_task[1], dep + 1); };
        walk(root.first, root.second, 0);
    } else b.build(0, n_prims, 0);
    hs->nodes.swap(b.nodes); hs->order.swap(b.leaf_order); hs->max_depth = b.max_depth;
}

/* ------------------------------------------------------------------ the record trees of a caller's flattened BVH (tests) */
static int flattened_bvh(const ftn_bvh_node* nodes, uint32_t n_nodes, std::vector<ftn_bvh_node>* v) {
    if (!nodes && n_nodes) return fail(FTN_ERR_INVALID_ARGUMENT, "null nodes");
    v->assign(nodes, nodes + n_nodes);
    for (uint32_t i = 0; i < n_nodes; i++) if (!(*v)[i].is_leaf && ((*v)[i].idx <= i + 1 || (*v)[i].idx >= n_nodes || (*v)[i].axis > 2)) return fail(FTN_ERR_INVALID_ARGUMENT, "not a flattened BVH (bvh.rs:133-158)");
    return FTN_OK;
}
/* records, their count and stack bound, and the explicit leaf boxes with their count (two float4 each), each wherever the caller asks */
template <class T> static void records_out(const std::vector<T>& rec, uint32_t n_records, uint32_t stack_bound, T* rec_out, uint32_t* n_out, uint32_t* bound_out,
                                           const std::vector<float4>* xbox = nullptr, float* xbox_out = nullptr, uint32_t* n_xbox_out = nullptr) {
    if (rec_out) memcpy(rec_out, rec.data(), rec.size() * sizeof(T));
    if (n_out) *n_out = n_records;
    if (bound_out) *bound_out = stack_bound;
    if (xbox_out) memcpy(xbox_out, xbox->data(), xbox->size() * sizeof(float4));
    if (n_xbox_out) *n_xbox_out = (uint32_t)(xbox->size() / 2);
}

extern "C" {

int ftn_bvh_quads(const ftn_bvh_node* nodes, uint32_t n_nodes, float* records_out_, uint32_t* n_records_out, uint32_t* stack_bound_out) {
    std::vector<ftn_bvh_node> v; int rc = flattened_bvh(nodes, n_nodes, &v); if (rc) return rc;
    QuadBvh qb; build_quads(v, &qb);
    if (!qb.ok) return fail(FTN_ERR_UNSUPPORTED, "more than 2^24 four-box records");
    records_out(qb.rec, qb.n_records, qb.stack_bound, records_out_, n_records_out, stack_bound_out);
    return FTN_OK;
}

/* the 64-byte four-box records of a flattened BVH (build_quad64s), for tests/test_quad64_bvh.py.  Exported, but not declared in
 * include/fountain_hip.h, whose every function has a twin in the CPU oracle: this one has none (the oracle walks the reference's nodes) */
int ftn_bvh_quad64s(const ftn_bvh_node* nodes, uint32_t n_nodes, uint32_t* records_out_, uint32_t* n_records_out, uint32_t* stack_bound_out, float* xbox_out, uint32_t* n_xbox_out) {
    std::vector<ftn_bvh_node> v; int rc = flattened_bvh(nodes, n_nodes, &v); if (rc) return rc;
    QuadBvh qb; build_quads(v, &qb);
    Quad64Bvh q6; build_quad64s(qb, std::vector<float4>(), &q6);       /* (no vertex data here: every leaf gets an explicit box) */
    if (!q6.ok) return fail(FTN_ERR_UNSUPPORTED, "no interior node, a non-finite box, or more than 2^24 four-box records");
    records_out(q6.rec, q6.n_records, q6.stack_bound, records_out_, n_records_out, stack_bound_out, &q6.xbox, xbox_out, n_xbox_out);
    return FTN_OK;
}

int ftn_bvh_octs(const ftn_bvh_node* nodes, uint32_t n_nodes, uint32_t* records_out_, uint32_t* n_records_out, uint32_t* stack_bound_out, float* xbox_out, uint32_t* n_xbox_out) {
    std::vector<ftn_bvh_node> v; int rc = flattened_bvh(nodes, n_nodes, &v); if (rc) return rc;
    OctBvh ob; build_octs(v, std::vector<float4>(), &ob);       /* (no vertex data here: every leaf gets an explicit box) */
    if (!ob.ok) return fail(FTN_ERR_UNSUPPORTED, "no interior node, or more than 2^24 eight-box records");
    records_out(ob.rec, ob.n_records, ob.stack_bound, records_out_, n_records_out, stack_bound_out, &ob.xbox, xbox_out, n_xbox_out);
    return FTN_OK;
}

}  /* extern "C" */
