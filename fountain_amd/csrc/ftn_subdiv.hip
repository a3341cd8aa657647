/*
 * ftn_subdiv.hip -- the kernels and the device driver of Loop subdivision (include/fountain_hip_subdiv.h).  The per-element code is
 * ftn_subdiv.h's, shared with the host twin; this file needs no scene internals and is its own translation unit.  Every kernel is a
 * gather: a thread writes the elements it owns from what it reads, with no float atomics, so nothing depends on the launch shape.  The
 * walks are chains of dependent loads (face -> neighbour -> face); what hides their latency is the number of vertices in flight, so the
 * kernels keep no LDS tile and few registers.  No grid is capped: a thread per element.
 *
 * Per level:
 *   k_sd_even         a thread per vertex: the even rule, the child's start face and boundary flag
 *   k_sd_owner_sums   a workgroup per 256 slots: how many of them own their edge
 *   k_sd_scan_sums    one workgroup: the exclusive scan of those counts, in place (a thread sums a contiguous run, the 256 run totals are
 *                     scanned in LDS, the thread writes its run back)
 *   k_sd_odd          a thread per slot: the owner's index = V + its workgroup's scanned count + its rank among the workgroup's owners
 *                     (wave ballots), the odd rule, the index recorded for both slots of the edge
 *   k_sd_topology     a thread per face: the four children's vertices and neighbours, 48 + 48 contiguous bytes as six 16-byte stores
 * After the last level:
 *   k_sd_limit        a thread per vertex: the limit position into a second array
 *   k_sd_normal       a thread per vertex: the normal from the ring's limit positions (a launch of its own: it reads what k_sd_limit wrote
 *                     for other vertices)
 * Flag words: a walk that hits its bound sets flags[0]; a vertex with a bad normal lowers flags[1] to its index (an integer atomicMin).
 */
#include "ftn_subdiv.h"
#include <algorithm>

namespace ftn {

constexpr uint32_t kSdBlock = 256;

__global__ void k_sd_init_flags(uint32_t* flags) { flags[kSdFlagWalk] = 0u; flags[kSdFlagNormal] = kSdNoVertex; }

__global__ void __launch_bounds__(kSdBlock) k_sd_even(SdLevel L, float* __restrict__ P, int32_t* __restrict__ sf, uint8_t* __restrict__ bd, uint32_t* flags) {
    const uint32_t v = blockIdx.x * kSdBlock + threadIdx.x;
    if (v >= L.V) return;
    const SdFan fan = sd_fan(L, (int32_t)v);
    Sd3 p = {0.0f, 0.0f, 0.0f};
    if (fan.ok) p = sd_vertex_rule(L, (int32_t)v, fan, false); else flags[kSdFlagWalk] = 1u;
    sd_store(P, v, p);
    const int32_t s = L.sf[v];
    sf[v] = 4 * s + sd_vnum(L.idx, s, (int32_t)v);
    bd[v] = L.bd[v];
}

/* is slot s (< 3 F) an owner; its rank among the owners of its wave and the wave's count */
__device__ __forceinline__ bool sd_slot_owner(const SdLevel& L, uint32_t s, uint32_t* wave_rank, uint32_t* wave_count) {
    bool own = false;
    if (s < 3u * L.F) own = sd_owner(L, (int32_t)(s / 3u), (int)(s % 3u));
    const unsigned long long m = __ballot(own);
    const uint32_t lane = threadIdx.x & 63u;
    *wave_rank = (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
    *wave_count = (uint32_t)__popcll(m);
    return own;
}

__global__ void __launch_bounds__(kSdBlock) k_sd_owner_sums(SdLevel L, uint32_t* __restrict__ sums) {
    __shared__ uint32_t s_wave[kSdBlock / 64];
    uint32_t rank, count;
    (void)sd_slot_owner(L, blockIdx.x * kSdBlock + threadIdx.x, &rank, &count);
    if ((threadIdx.x & 63u) == 0u) s_wave[threadIdx.x >> 6] = count;
    __syncthreads();
    if (threadIdx.x == 0) sums[blockIdx.x] = (s_wave[0] + s_wave[1]) + (s_wave[2] + s_wave[3]);
}

__global__ void __launch_bounds__(kSdBlock) k_sd_scan_sums(uint32_t* __restrict__ sums, uint32_t n) {
    __shared__ uint32_t s_run[kSdBlock];
    const uint32_t per = (n + kSdBlock - 1u) / kSdBlock, b = std::min(n, threadIdx.x * per), e = std::min(n, b + per);
    uint32_t t = 0;
    for (uint32_t i = b; i < e; i++) t += sums[i];
    s_run[threadIdx.x] = t;
    __syncthreads();
    if (threadIdx.x == 0) { uint32_t a = 0; for (uint32_t i = 0; i < kSdBlock; i++) { const uint32_t c = s_run[i]; s_run[i] = a; a += c; } }
    __syncthreads();
    uint32_t a = s_run[threadIdx.x];
    for (uint32_t i = b; i < e; i++) { const uint32_t c = sums[i]; sums[i] = a; a += c; }
}

__global__ void __launch_bounds__(kSdBlock) k_sd_odd(SdLevel L, const uint32_t* __restrict__ sums, float* __restrict__ P, int32_t* __restrict__ sf,
                                                     uint8_t* __restrict__ bd, int32_t* __restrict__ eidx) {
    __shared__ uint32_t s_wave[kSdBlock / 64];
    const uint32_t s = blockIdx.x * kSdBlock + threadIdx.x, w = threadIdx.x >> 6;
    uint32_t rank, count;
    const bool own = sd_slot_owner(L, s, &rank, &count);
    if ((threadIdx.x & 63u) == 0u) s_wave[w] = count;
    __syncthreads();
    if (!own) return;
    uint32_t before = sums[blockIdx.x] + rank;
    for (uint32_t i = 0; i < w; i++) before += s_wave[i];
    const uint32_t e = L.V + before;
    const int32_t f = (int32_t)(s / 3u);
    bool boundary; int64_t nslot;
    const Sd3 p = sd_odd_rule(L, f, (int)(s % 3u), &boundary, &nslot);
    sd_store(P, e, p);
    sf[e] = 4 * f + 3;
    bd[e] = boundary ? 1 : 0;
    eidx[s] = (int32_t)e;
    if (nslot >= 0) eidx[nslot] = (int32_t)e;
}

__global__ void __launch_bounds__(kSdBlock) k_sd_topology(SdLevel L, const int32_t* __restrict__ eidx, int32_t* __restrict__ idx, int32_t* __restrict__ nb) {
    const uint32_t f = blockIdx.x * kSdBlock + threadIdx.x;
    if (f >= L.F) return;
    const int32_t e[3] = {eidx[3 * (size_t)f], eidx[3 * (size_t)f + 1], eidx[3 * (size_t)f + 2]};
    int32_t ci[12], cn[12];
    sd_children(L, (int32_t)f, e, ci, cn);
    int4* const di = reinterpret_cast<int4*>(idx) + 3 * (size_t)f;       /* 12 ints per face: 48 bytes, 16-byte aligned */
    int4* const dn = reinterpret_cast<int4*>(nb) + 3 * (size_t)f;
    di[0] = make_int4(ci[0], ci[1], ci[2], ci[3]); di[1] = make_int4(ci[4], ci[5], ci[6], ci[7]); di[2] = make_int4(ci[8], ci[9], ci[10], ci[11]);
    dn[0] = make_int4(cn[0], cn[1], cn[2], cn[3]); dn[1] = make_int4(cn[4], cn[5], cn[6], cn[7]); dn[2] = make_int4(cn[8], cn[9], cn[10], cn[11]);
}

__global__ void __launch_bounds__(kSdBlock) k_sd_limit(SdLevel L, float* __restrict__ Lim, uint32_t* flags) {
    const uint32_t v = blockIdx.x * kSdBlock + threadIdx.x;
    if (v >= L.V) return;
    const SdFan fan = sd_fan(L, (int32_t)v);
    Sd3 p = {0.0f, 0.0f, 0.0f};
    if (fan.ok) p = sd_vertex_rule(L, (int32_t)v, fan, true); else flags[kSdFlagWalk] = 1u;
    sd_store(Lim, v, p);
}

__global__ void __launch_bounds__(kSdBlock) k_sd_normal(SdLevel L, const float* __restrict__ Lim, float* __restrict__ N, uint32_t* flags) {
    const uint32_t v = blockIdx.x * kSdBlock + threadIdx.x;
    if (v >= L.V) return;
    const SdFan fan = sd_fan(L, (int32_t)v);
    Sd3 n = {0.0f, 0.0f, 0.0f};
    if (!fan.ok) flags[kSdFlagWalk] = 1u;
    else if (!sd_normal(L, Lim, (int32_t)v, fan, &n)) atomicMin(flags + kSdFlagNormal, v);
    sd_store(N, v, n);
}

static unsigned sd_blocks(uint64_t n) { return (unsigned)std::max<uint64_t>(1, (n + kSdBlock - 1) / kSdBlock); }

hipError_t launch_subdivide(const SdDevice& d, const ftn_subdiv_info& info, hipStream_t stream) {
    const int32_t bound = std::max(info.max_valence, 6);
    auto level = [&](int l) {
        const int s = l & 1;
        return SdLevel{d.P[s], d.idx[s], d.nb[s], d.sf[s], d.bd[s], info.n_vertices[l], info.n_faces[l], bound};
    };
    hipLaunchKernelGGL(k_sd_init_flags, dim3(1), dim3(1), 0, stream, d.flags);
    for (int l = 0; l < info.levels; l++) {
        const SdLevel L = level(l);
        const int t = (l + 1) & 1;
        const uint64_t slots = 3ull * L.F;
        const unsigned slot_blocks = sd_blocks(slots);
        hipLaunchKernelGGL(k_sd_even, dim3(sd_blocks(L.V)), dim3(kSdBlock), 0, stream, L, d.P[t], d.sf[t], d.bd[t], d.flags);
        hipLaunchKernelGGL(k_sd_owner_sums, dim3(slot_blocks), dim3(kSdBlock), 0, stream, L, d.sums);
        hipLaunchKernelGGL(k_sd_scan_sums, dim3(1), dim3(kSdBlock), 0, stream, d.sums, (uint32_t)slot_blocks);
        hipLaunchKernelGGL(k_sd_odd, dim3(slot_blocks), dim3(kSdBlock), 0, stream, L, d.sums, d.P[t], d.sf[t], d.bd[t], d.eidx);
        hipLaunchKernelGGL(k_sd_topology, dim3(sd_blocks(L.F)), dim3(kSdBlock), 0, stream, L, d.eidx, d.idx[t], d.nb[t]);
    }
    const SdLevel L = level(info.levels);
    float* const Lim = d.P[(info.levels + 1) & 1];
    hipLaunchKernelGGL(k_sd_limit, dim3(sd_blocks(L.V)), dim3(kSdBlock), 0, stream, L, Lim, d.flags);
    hipLaunchKernelGGL(k_sd_normal, dim3(sd_blocks(L.V)), dim3(kSdBlock), 0, stream, L, Lim, d.N, d.flags);
    return hipGetLastError();
}

}  // namespace ftn
