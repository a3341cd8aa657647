/*
 * ftn_subdiv_host.cpp -- C entry points of include/fountain_hip_subdiv.h: the refusals, the level-0 tables and the counts, the host twin
 * of the kernels and the host-buffer entry.
 *
 * The per-element code is ftn_subdiv.h's, shared with the kernels; error reporting, device selection and the host thread budget are the
 * host library's (ftn_host_internal.h).
 */
#include "ftn_stage_host.h"
#include "ftn_subdiv.h"

#include <atomic>
#include <cstring>

using namespace ftn;

namespace {

/* level 0: what the header's "Level 0" paragraph builds, and the counts that follow from it */
struct Cage {
    std::vector<int32_t> idx, nb, sf; std::vector<uint8_t> bd;
    ftn_subdiv_info info;
};

int bad(const char* what, size_t index) { return fail(FTN_ERR_INVALID_ARGUMENT, std::string("loopsubdiv: ") + what + " " + std::to_string(index)); }

/* refusals (2) to (11) of the header; fills `c` */
int build_cage(const uint32_t* indices, int32_t n_vertices, int32_t n_faces, int32_t levels, Cage* c) {
    if (n_vertices <= 0 || n_faces <= 0) return fail(FTN_ERR_INVALID_ARGUMENT, "loopsubdiv: n_vertices and n_faces must be positive");
    if (levels < 0 || levels > FTN_SUBDIV_MAX_LEVELS) return fail(FTN_ERR_INVALID_ARGUMENT, "loopsubdiv: levels must be 0..10");
    if (((uint64_t)n_faces << (2 * levels)) > (uint64_t)FTN_SUBDIV_MAX_FACES) return fail(FTN_ERR_INVALID_ARGUMENT, "loopsubdiv: n_faces * 4^levels must not exceed 2^26");
    const size_t V = (size_t)n_vertices, F = (size_t)n_faces;
    for (size_t f = 0; f < F; f++) for (int k = 0; k < 3; k++) if (indices[3 * f + k] >= (uint32_t)n_vertices) return bad("vertex index out of range in face", f);
    for (size_t f = 0; f < F; f++) {
        const uint32_t* t = indices + 3 * f;
        if (t[0] == t[1] || t[1] == t[2] || t[0] == t[2]) return bad("repeated vertex in face", f);
    }
    c->idx.assign(indices, indices + 3 * F);
    /* the edge map: slots sorted by their unordered vertex pair, each pair's slots in (face, k) order */
    struct Slot { uint64_t key; uint32_t slot; };
    std::vector<Slot> slots(3 * F);
    for (size_t s = 0; s < 3 * F; s++) {
        const uint32_t a = indices[s], b = indices[3 * (s / 3) + (s % 3 + 1) % 3];
        slots[s] = Slot{((uint64_t)std::min(a, b) << 32) | std::max(a, b), (uint32_t)s};
    }
    std::sort(slots.begin(), slots.end(), [](const Slot& x, const Slot& y) { return x.key != y.key ? x.key < y.key : x.slot < y.slot; });
    c->nb.assign(3 * F, -1);
    size_t third = SIZE_MAX, same_way = SIZE_MAX;
    uint64_t E = 0, Eb = 0;
    for (size_t i = 0; i < slots.size();) {
        size_t j = i + 1;
        while (j < slots.size() && slots[j].key == slots[i].key) j++;
        E++;
        if (j - i == 1) Eb++;
        if (j - i > 2) third = std::min<size_t>(third, slots[i + 2].slot / 3);
        else if (j - i == 2) {
            const uint32_t s0 = slots[i].slot, s1 = slots[i + 1].slot;
            if (indices[s0] == indices[s1]) same_way = std::min<size_t>(same_way, s1 / 3);
            c->nb[s0] = (int32_t)(s1 / 3); c->nb[s1] = (int32_t)(s0 / 3);
        }
        i = j;
    }
    if (third != SIZE_MAX) return bad("an edge is used by more than two faces, the third is face", third);
    if (same_way != SIZE_MAX) return bad("inconsistent winding: a shared edge is crossed in the same direction by face", same_way);
    std::vector<int32_t> uses(V, 0);
    c->sf.assign(V, -1);
    for (size_t f = 0; f < F; f++) for (int k = 0; k < 3; k++) { uses[indices[3 * f + k]]++; c->sf[indices[3 * f + k]] = (int32_t)f; }
    for (size_t v = 0; v < V; v++) if (c->sf[v] < 0) return bad("no face uses vertex", v);
    c->bd.assign(V, 0);
    int32_t max_valence = 0; uint64_t B = 0;
    const int32_t* idx = c->idx.data(); const int32_t* nb = c->nb.data();
    for (size_t v = 0; v < V; v++) {
        /* forward to the boundary or once round (a step is injective on the faces around v once (7) and (8) hold, so it ends) */
        int32_t f = c->sf[v], reached = 0;
        do { f = nb[3 * (size_t)f + sd_vnum(idx, f, (int32_t)v)]; reached++; } while (f >= 0 && f != c->sf[v] && reached <= uses[v]);
        if (f < 0) {
            /* boundary: count the fan from its forward end */
            c->bd[v] = 1; B++;
            f = c->sf[v];
            for (int32_t g; (g = nb[3 * (size_t)f + sd_vnum(idx, f, (int32_t)v)]) >= 0;) f = g;
            reached = 0;
            for (; f >= 0; f = nb[3 * (size_t)f + sd_prev(sd_vnum(idx, f, (int32_t)v))]) reached++;
        }
        if (reached < uses[v]) return bad("two fans are pinched at vertex", v);
        max_valence = std::max(max_valence, uses[v] + (c->bd[v] ? 1 : 0));
    }
    ftn_subdiv_info& in = c->info;
    memset(&in, 0, sizeof(in));
    in.levels = levels; in.max_valence = max_valence;
    uint64_t v = V, fc = F;
    for (int l = 0;; l++) {
        if (v >= ((uint64_t)1 << 31)) return fail(FTN_ERR_INVALID_ARGUMENT, "loopsubdiv: the refined mesh must have fewer than 2^31 vertices");
        in.n_vertices[l] = (uint32_t)v; in.n_faces[l] = (uint32_t)fc; in.n_edges[l] = (uint32_t)E; in.n_boundary[l] = (uint32_t)B;
        if (l == levels) break;
        v += E; E = 2 * E + 3 * fc; fc *= 4; B += Eb; Eb *= 2;
    }
    return FTN_OK;
}

/* parallel_for with a finer grain than the image passes': a vertex's walk is tens of dependent loads */
template <class Fn> void sd_parallel_for(size_t n, Fn f) {
    const int nt = (int)std::min<size_t>((size_t)host_threads(), n / 2048 + 1);
    if (nt <= 1) { f((size_t)0, n); return; }
    std::vector<std::thread> th;
    for (int t = 0; t < nt; t++) th.emplace_back([&, t]() { f(n * (size_t)t / (size_t)nt, n * (size_t)(t + 1) / (size_t)nt); });
    for (auto& x : th) x.join();
}

int normal_refusal(uint32_t v) { return bad("the limit normal has zero or non-finite length at vertex", v); }

}  // namespace

extern "C" {

static_assert(sizeof(ftn_subdiv_info) == 184, "ABI");
int ftn_subdiv_abi_version(void) { return FTN_SUBDIV_ABI_VERSION; }

int ftn_loop_subdivide_info(const uint32_t* indices, int32_t n_vertices, int32_t n_faces, int32_t levels, ftn_subdiv_info* info) {
    if (!indices || !info) return fail(FTN_ERR_INVALID_ARGUMENT, "null argument");
    Cage c;
    int rc = build_cage(indices, n_vertices, n_faces, levels, &c); if (rc) return rc;
    *info = c.info;
    return FTN_OK;
}

int ftn_loop_subdivide_cpu(const float* P, int32_t n_vertices, const uint32_t* indices, int32_t n_faces, int32_t levels, float* out_P, float* out_N,
                           uint32_t* out_indices) {
    if (!P || !indices || !out_P || !out_N || !out_indices) return fail(FTN_ERR_INVALID_ARGUMENT, "null argument");
    Cage c;
    int rc = build_cage(indices, n_vertices, n_faces, levels, &c); if (rc) return rc;
    const ftn_subdiv_info& in = c.info;
    const int32_t bound = std::max(in.max_valence, 6);
    std::vector<float> pos(P, P + 3 * (size_t)n_vertices);
    std::vector<int32_t> idx = std::move(c.idx), nb = std::move(c.nb), sf = std::move(c.sf); std::vector<uint8_t> bd = std::move(c.bd);
    std::atomic<bool> walk_failed(false);
    for (int l = 0; l < levels; l++) {
        const SdLevel L = {pos.data(), idx.data(), nb.data(), sf.data(), bd.data(), in.n_vertices[l], in.n_faces[l], bound};
        const size_t V = L.V, F = L.F, V2 = in.n_vertices[l + 1];
        std::vector<float> pos2(3 * V2); std::vector<int32_t> idx2(12 * F), nb2(12 * F), sf2(V2), eidx(3 * F), first(3 * F); std::vector<uint8_t> bd2(V2);
        sd_parallel_for(V, [&](size_t v0, size_t v1) {
            for (size_t v = v0; v < v1; v++) {
                const SdFan fan = sd_fan(L, (int32_t)v);
                Sd3 p = {0.0f, 0.0f, 0.0f};
                if (fan.ok) p = sd_vertex_rule(L, (int32_t)v, fan, false); else walk_failed = true;
                sd_store(pos2.data(), v, p);
                sf2[v] = 4 * sf[v] + sd_vnum(L.idx, sf[v], (int32_t)v);
                bd2[v] = bd[v];
            }
        });
        /* the exclusive prefix count of owning slots, serially: integers, one pass */
        uint32_t owners = 0;
        for (size_t s = 0; s < 3 * F; s++) { first[s] = (int32_t)owners; owners += sd_owner(L, (int32_t)(s / 3), (int)(s % 3)) ? 1u : 0u; }
        sd_parallel_for(3 * F, [&](size_t s0, size_t s1) {
            for (size_t s = s0; s < s1; s++) {
                const int32_t f = (int32_t)(s / 3); const int k = (int)(s % 3);
                if (!sd_owner(L, f, k)) continue;
                const size_t e = V + (size_t)first[s];
                bool boundary; int64_t nslot;
                sd_store(pos2.data(), e, sd_odd_rule(L, f, k, &boundary, &nslot));
                sf2[e] = 4 * f + 3; bd2[e] = boundary ? 1 : 0;
                eidx[s] = (int32_t)e;
                if (nslot >= 0) eidx[(size_t)nslot] = (int32_t)e;
            }
        });
        sd_parallel_for(F, [&](size_t f0, size_t f1) {
            for (size_t f = f0; f < f1; f++) sd_children(L, (int32_t)f, eidx.data() + 3 * f, idx2.data() + 12 * f, nb2.data() + 12 * f);
        });
        pos.swap(pos2); idx.swap(idx2); nb.swap(nb2); sf.swap(sf2); bd.swap(bd2);
    }
    if (walk_failed) return fail(FTN_ERR_INTERNAL, "loopsubdiv: a walk around a vertex did not end within the valence bound");
    const SdLevel L = {pos.data(), idx.data(), nb.data(), sf.data(), bd.data(), in.n_vertices[levels], in.n_faces[levels], bound};
    const size_t V = L.V;
    sd_parallel_for(V, [&](size_t v0, size_t v1) {
        for (size_t v = v0; v < v1; v++) {
            const SdFan fan = sd_fan(L, (int32_t)v);
            Sd3 p = {0.0f, 0.0f, 0.0f};
            if (fan.ok) p = sd_vertex_rule(L, (int32_t)v, fan, true); else walk_failed = true;
            sd_store(out_P, v, p);
        }
    });
    std::atomic<uint32_t> worst(kSdNoVertex);
    sd_parallel_for(V, [&](size_t v0, size_t v1) {
        uint32_t w = kSdNoVertex;
        for (size_t v = v0; v < v1; v++) {
            const SdFan fan = sd_fan(L, (int32_t)v);
            Sd3 n = {0.0f, 0.0f, 0.0f};
            if (!fan.ok) walk_failed = true;
            else if (!sd_normal(L, out_P, (int32_t)v, fan, &n)) w = std::min(w, (uint32_t)v);
            sd_store(out_N, v, n);
        }
        for (uint32_t have = worst.load(); w < have && !worst.compare_exchange_weak(have, w);) {}
    });
    for (size_t i = 0; i < 3 * (size_t)L.F; i++) out_indices[i] = (uint32_t)idx[i];
    if (walk_failed) return fail(FTN_ERR_INTERNAL, "loopsubdiv: a walk around a vertex did not end within the valence bound");
    if (worst.load() != kSdNoVertex) return normal_refusal(worst.load());
    return FTN_OK;
}

int ftn_loop_subdivide(const float* P, int32_t n_vertices, const uint32_t* indices, int32_t n_faces, int32_t levels, float* out_P, float* out_N,
                       uint32_t* out_indices, int32_t device) {
    if (!P || !indices || !out_P || !out_N || !out_indices) return fail(FTN_ERR_INVALID_ARGUMENT, "null argument");
    Cage c;
    int rc = build_cage(indices, n_vertices, n_faces, levels, &c); if (rc) return rc;
    if (int no = need_device()) return no;
    if ((rc = set_device(device))) return rc;
    const ftn_subdiv_info& in = c.info;
    /* set s holds the levels of parity s; the limit positions go to the P set the last level does not use */
    size_t nV[2] = {0, 0}, nF[2] = {0, 0};
    for (int l = 0; l <= levels; l++) { nV[l & 1] = std::max<size_t>(nV[l & 1], in.n_vertices[l]); nF[l & 1] = std::max<size_t>(nF[l & 1], in.n_faces[l]); }
    const size_t VL = in.n_vertices[levels], FL = in.n_faces[levels], Fscan = levels ? in.n_faces[levels - 1] : 0;
    struct Bufs {
        DevBuf<float> dP[2], dN; DevBuf<int32_t> dIdx[2], dNb[2], dSf[2], dE; DevBuf<uint8_t> dBd[2]; DevBuf<uint32_t> dSums, dFlags;
        ~Bufs() { for (int s = 0; s < 2; s++) { dP[s].release(); dIdx[s].release(); dNb[s].release(); dSf[s].release(); dBd[s].release(); } dN.release(); dE.release(); dSums.release(); dFlags.release(); }
    } B;
    DevBuf<float> (&dP)[2] = B.dP; DevBuf<float>& dN = B.dN; DevBuf<int32_t> (&dIdx)[2] = B.dIdx, (&dNb)[2] = B.dNb, (&dSf)[2] = B.dSf; DevBuf<int32_t>& dE = B.dE;
    DevBuf<uint8_t> (&dBd)[2] = B.dBd; DevBuf<uint32_t>& dSums = B.dSums; DevBuf<uint32_t>& dFlags = B.dFlags;
    auto alloc = [](auto& b, size_t count) -> int {
        typedef typename std::remove_reference<decltype(*b.p)>::type T;
        b.n = count;
        HIP_TRY(hipMalloc((void**)&b.p, std::max<size_t>(count, 4) * sizeof(T)));
        return FTN_OK;
    };
    for (int s = 0; s < 2; s++) {
        if ((rc = alloc(dP[s], 3 * VL)) || (rc = alloc(dIdx[s], 3 * nF[s])) || (rc = alloc(dNb[s], 3 * nF[s])) || (rc = alloc(dSf[s], nV[s])) || (rc = alloc(dBd[s], nV[s]))) return rc;
    }
    if ((rc = alloc(dN, 3 * VL)) || (rc = alloc(dE, 3 * Fscan)) || (rc = alloc(dSums, (3 * Fscan + 255) / 256 + 1)) || (rc = alloc(dFlags, kSdFlagWords))) return rc;
    HIP_TRY(hipMemcpy(dP[0].p, P, 3 * (size_t)n_vertices * sizeof(float), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(dIdx[0].p, c.idx.data(), c.idx.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(dNb[0].p, c.nb.data(), c.nb.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(dSf[0].p, c.sf.data(), c.sf.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(dBd[0].p, c.bd.data(), c.bd.size(), hipMemcpyHostToDevice));
    SdDevice d;
    for (int s = 0; s < 2; s++) { d.P[s] = dP[s].p; d.idx[s] = dIdx[s].p; d.nb[s] = dNb[s].p; d.sf[s] = dSf[s].p; d.bd[s] = dBd[s].p; }
    d.N = dN.p; d.eidx = dE.p; d.sums = dSums.p; d.flags = dFlags.p;
    const hipError_t e = launch_subdivide(d, in, nullptr);
    if (e != hipSuccess) return fail(FTN_ERR_INTERNAL, std::string("loopsubdiv launch: ") + hipGetErrorString(e));
    uint32_t flags[kSdFlagWords];
    HIP_TRY(hipMemcpy(flags, d.flags, sizeof(flags), hipMemcpyDeviceToHost));
    if (flags[kSdFlagWalk]) return fail(FTN_ERR_INTERNAL, "loopsubdiv: a walk around a vertex did not end within the valence bound");
    HIP_TRY(hipMemcpy(out_P, d.P[(levels + 1) & 1], 3 * VL * sizeof(float), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(out_N, d.N, 3 * VL * sizeof(float), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(out_indices, d.idx[levels & 1], 3 * FL * sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (flags[kSdFlagNormal] != kSdNoVertex) return normal_refusal(flags[kSdFlagNormal]);
    return FTN_OK;
}

}  /* extern "C" */
