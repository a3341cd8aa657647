/*
 * ftn_idmatte.hip -- the ID-matte pass (include/fountain_hip_idmatte.h) on the wavefront pipeline, with its resolve and matte extraction.
 *
 * A unit of its own, the second of the kind of ftn_gbuffer.hip: the kernels are here and share ftn_wf_common.h with the beauty's; the
 * passes and their pass-through rounds are wf_first_hit_passes' (ftn_wf_internal.h, ftn_wavefront.hip), which wavefront_idmatte hands the
 * launches of k_im_shade and k_im_accumulate.  The foreign list -- its allocation before the first pass, its sort and k_im_apply after the
 * last -- is this unit's.
 */
#include "ftn_firsthit.h"
#include "ftn_idmatte.h"
#include <hipcub/hipcub.hpp>
#include <cstring>

namespace ftn {

/* ================================================================== the pass
 * The camera samples of ftn_render for the same sampler, tiles and film: k_wf_generate makes the camera rays from the sample keys, the
 * production closest-hit kernels trace them, and k_im_shade records the id of the first surface that has a material.  A null-material
 * hit spawns the ray on along the same direction (path.rs:77-80) into the other queue and the round repeats
 * (wf_first_hit_passes).  k_im_accumulate then takes the pass's samples of every pixel into the pixel's table in sample order; what
 * a sample adds to OTHER pixels goes to the foreign list, which k_im_apply works off after the last pass, sorted. */
/* the foreign list: key = destination crop pixel << 32 | (sample - first sample of the call) << 4 | 3 (dy + 1) + (dx + 1), where (dx, dy)
 * is the source pixel's offset from the destination; value = id | hit << 32.  ctr[0]: entries asked for (beyond cap: not written),
 * ctr[1]: samples whose footprint reached further than one pixel (never with a radius of at most 1) */
struct ImParams {
    uint32_t* out;                  /* 20 words per crop pixel (ftn_idmatte_pixel), continued */
    const uint32_t* ids;            /* the caller's id of every primitive, in BVH order */
    uint2* rec;                     /* per path {id, hit ? 1 : 0} */
    unsigned long long *sp_key, *sp_val, *ctr;
    unsigned long long sp_cap;
};

/* one thread per queued ray: the hit it found is either recorded or passed through */
__global__ void __launch_bounds__(256) k_im_shade(RenderParams P, WfBuffers W, ImParams G, const uint32_t* __restrict__ q_in, const uint32_t* count_in,
                                                  uint32_t* q_out, uint32_t* count_out) {
    const DScene& S = P.S;
    const uint32_t qi = blockIdx.x * 256u + threadIdx.x;
    bool push = false;
    uint32_t p = 0;
    if (qi < *count_in) {
        p = q_in[qi];
        DRay ray0; DHit h; DSI si;
        const FhHit found = fh_first_hit(S, W, p, &ray0, &h, &si);
        push = found == FH_THROUGH;
        if (!push) G.rec[p] = found == FH_SURFACE ? make_uint2(G.ids[h.prim], 1u) : make_uint2(0u, 0u);          /* (a miss: zeros) */
    }
    const bool pred[1] = {push};
    const uint32_t val[1] = {p};
    uint32_t* const qs[1] = {q_out};
    uint32_t* const cs[1] = {count_out};
    block_push<1>(pred, val, qs, cs);
}

/* one sample into every pixel of its box-filter footprint: the own pixel's table in registers, the others as entries of the foreign list */
__device__ inline void im_film_add(const ImParams& G, const FilmCtx& F, V2 p_film, uint2 r, uint32_t s_rel, int px, int py, bool own, ImTable* t, uint32_t* spill) {
    const FilmFootprint fp = film_footprint(F, p_film);
    const int nx = fp.x1 - fp.x0, ny = fp.y1 - fp.y0;
    if (nx <= 0 || ny <= 0) { (*spill)++; return; }
    const bool own_in = own && px >= fp.x0 && px < fp.x1 && py >= fp.y0 && py < fp.y1;
    if (own_in) im_add(t, r.y != 0u, r.x, 1.0f);                                    /* filter weight (box: 1.0) */
    const uint32_t n_foreign = (uint32_t)nx * (uint32_t)ny - (own_in ? 1u : 0u);
    if (nx * ny != 1) (*spill)++;
    if (n_foreign == 0) return;
    if (fp.x0 < px - 1 || fp.x1 > px + 2 || fp.y0 < py - 1 || fp.y1 > py + 2) { atomicAdd(&G.ctr[1], 1ull); return; }
    unsigned long long at = atomicAdd(&G.ctr[0], (unsigned long long)n_foreign);
    if (at + n_foreign > G.sp_cap) return;                                          /* the host sees ctr[0] > cap and fails the call */
    for (int y = fp.y0; y < fp.y1; y++)
        for (int x = fp.x0; x < fp.x1; x++) {
            if (own_in && x == px && y == py) continue;
            const uint32_t off = (uint32_t)((py - y + 1) * 3 + (px - x + 1));
            G.sp_key[at] = ((unsigned long long)film_idx(F, x, y) << 32) | ((unsigned long long)s_rel << 4) | off;
            G.sp_val[at] = (unsigned long long)r.x | ((unsigned long long)(r.y != 0u) << 32);
            at++;
        }
}

/* One thread per pixel slot takes its samples in sample order into the pixel's table, which stays in registers from the load to the
 * store; the workgroup stages IM_ACC_CHUNK samples of its 256 slots (8 bytes each, neighbours in memory) through LDS with coalesced
 * loads, as k_fh_accumulate (ftn_firsthit.h) does for the passes whose film is float sums. */
#define IM_ACC_CHUNK 8u
__global__ void __launch_bounds__(256) k_im_accumulate(RenderParams P, WfBuffers W, ImParams G, uint32_t first_of_call) {
    __shared__ uint2 s_rec[IM_ACC_CHUNK * 256];
    const uint32_t slot = blockIdx.x * 256u + threadIdx.x;
    uint32_t spill = 0;
    const FilmSlot fs = film_slot(P, W.n_slots, slot);
    const bool valid = fs.valid, in_crop = fs.in_crop; const int px = fs.px, py = fs.py;
    uint32_t* const mine = G.out + (size_t)IM_WORDS * fs.ai;
    ImTable t;
    if (valid && in_crop) im_load(mine, &t);
    else {
#pragma unroll
        for (int k = 0; k < IM_SLOTS; k++) { t.id[k] = 0u; t.w[k] = 0.0f; }
        t.overflow = 0.0f; t.miss = 0.0f; t.total = 0.0f; t.n = 0u;
    }
    const size_t block_first = (size_t)blockIdx.x * 256u * W.samples;              /* first path of this workgroup's 256 slots */
    for (uint32_t s0 = 0; s0 < W.samples; s0 += IM_ACC_CHUNK) {
        const uint32_t n = W.samples - s0 < IM_ACC_CHUNK ? W.samples - s0 : IM_ACC_CHUNK;
        for (uint32_t e = threadIdx.x; e < 256u * n; e += 256u) {                   /* the n consecutive records of slot e / n */
            const uint32_t sl = e / n, k = e - sl * n;
            const size_t p = block_first + (size_t)sl * W.samples + s0 + k;
            if (p < (size_t)W.n_paths) s_rec[k * 256u + sl] = G.rec[p];
        }
        __syncthreads();
        if (valid) {
            for (uint32_t k = 0; k < n; k++) {
                /* the sample's film position: the first two draws of its stream, exactly as k_wf_generate made them */
                Rng crng; crng.seed(indexed_key(P.seed, px, py, W.first_sample + s0 + k));
                const V2 j = crng.next2();
                im_film_add(G, fs.F, V2((float)px + j.x, (float)py + j.y), s_rec[k * 256u + threadIdx.x], W.first_sample + s0 + k - first_of_call, px, py, in_crop, &t, &spill);
            }
        }
        __syncthreads();
    }
    if (valid && in_crop) im_store(t, mine);
    if (spill) atomicAdd(&P.stats->spill_samples, (unsigned long long)spill);       /* rare with a radius of 0.5 */
}

/* after the last pass, over the sorted foreign list: the thread at the head of a destination's run takes the run into that pixel's table */
__global__ void __launch_bounds__(256) k_im_apply(ImParams G, const unsigned long long* __restrict__ key, const unsigned long long* __restrict__ val, size_t n) {
    const size_t i = (size_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const uint32_t dest = (uint32_t)(key[i] >> 32);
    if (i > 0 && (uint32_t)(key[i - 1] >> 32) == dest) return;
    uint32_t* const px = G.out + (size_t)IM_WORDS * dest;
    ImTable t; im_load(px, &t);
    for (size_t j = i; j < n && (uint32_t)(key[j] >> 32) == dest; j++) {
        const unsigned long long v = val[j];
        im_add(&t, (v >> 32) != 0ull, (uint32_t)v, 1.0f);
    }
    im_store(t, px);
}

struct ImResolve {
    const uint32_t* in; uint32_t* out20;
    __device__ void operator()(size_t i) const { idmatte_resolve_pixel(in + IM_WORDS * i, out20 + IM_WORDS * i); }
};
hipError_t launch_idmatte_resolve(const uint32_t* in, size_t n, uint32_t* out20, hipStream_t stream) { return fh_per_pixel(n, stream, ImResolve{in, out20}); }

__global__ void __launch_bounds__(256) k_im_select(const uint32_t* __restrict__ resolved, size_t n, const uint32_t* __restrict__ ids, size_t n_ids, uint32_t flags, float* __restrict__ mask) {
    for (size_t i = (size_t)blockIdx.x * 256u + threadIdx.x; i < n; i += (size_t)gridDim.x * 256u) mask[i] = idmatte_select_pixel(resolved + IM_WORDS * i, ids, n_ids, flags);
}
void launch_idmatte_select(const uint32_t* resolved, size_t n, const uint32_t* ids, size_t n_ids, uint32_t flags, float* mask, hipStream_t stream) {
    if (n == 0) return;
    const unsigned grid = (unsigned)std::min<size_t>((n + 255) / 256, 4096);
    hipLaunchKernelGGL(k_im_select, dim3(grid), dim3(256), 0, stream, resolved, n, ids, n_ids, flags, mask);
}

namespace {
struct ImSpill {                                        /* the foreign list of one call in one allocation, freed on every way out */
    void* mem = nullptr;
    unsigned long long *key[2] = {nullptr, nullptr}, *val[2] = {nullptr, nullptr}, *ctr = nullptr;
    ~ImSpill() { if (mem) (void)hipFree(mem); }
};
}  // namespace

int wavefront_idmatte(WavefrontState** state, const RenderParams& P, const std::vector<DTile>& tiles, const uint32_t* d_ids, uint32_t* d_out,
                      hipStream_t stream, double* trace_ms_out) {
    ImSpill sp;
    unsigned long long cap = 0;
    ImParams G;
    G.out = d_out; G.ids = d_ids;
    WfFirstHitPass pass;
    pass.what = "the matte";
    pass.setup = [&](WavefrontState* st, uint32_t valid) -> int {
        /* the foreign list's capacity.  A footprint spans at most 2 pixels of an axis whose radius is at most 0.5 and 3 up to a radius of 1,
         * so a sample makes at most nx * ny - 1 entries.  A wider radius gets room for all of them; with at most 0.5 in both axes only
         * rounding makes a footprint leave its pixel (about one sample in 10^5), and one entry per 64 samples is room a thousandfold */
        const unsigned long long n_samples = (unsigned long long)valid * (P.last_sample - P.first_sample);
        const unsigned long long per_sample = (unsigned long long)((P.radius[0] <= 0.5f ? 2 : 3) * (P.radius[1] <= 0.5f ? 2 : 3) - 1);
        cap = n_samples * per_sample;
        if (P.radius[0] <= 0.5f && P.radius[1] <= 0.5f) cap = std::min(cap, std::max(4096ull, n_samples / 64ull));
        size_t free_b = 0, total_b = 0;
        WF_TRY(hipMemGetInfo(&free_b, &total_b));
        if (cap >= (1ull << 31) || cap * 40ull > (unsigned long long)free_b) {
            wf_set_error("the list of samples that reach other pixels would need " + std::to_string(cap) + " entries of 32 bytes and their sort's work space, which " +
                         (cap >= (1ull << 31) ? "is more than one sort takes" : "does not fit in the free device memory") + ": render the samples in several ranges");
            return FTN_ERR_OUT_OF_MEMORY;
        }
        WF_TRY(hipMalloc(&sp.mem, (size_t)(cap * 32ull + 16ull)));
        unsigned long long* const base = (unsigned long long*)sp.mem;
        for (int k = 0; k < 2; k++) { sp.key[k] = base + (size_t)cap * k; sp.val[k] = base + (size_t)cap * (2 + k); }
        sp.ctr = base + (size_t)cap * 4;
        WF_TRY(hipMemsetAsync(sp.ctr, 0, 16, stream));
        G.rec = reinterpret_cast<uint2*>(st->pd);        /* the path integrator's 64-byte records: 8 bytes per path used */
        G.sp_key = sp.key[0]; G.sp_val = sp.val[0]; G.ctr = sp.ctr; G.sp_cap = cap;
        return FTN_OK;
    };
    pass.shade = [&](const WfBuffers& W, const uint32_t* q_in, const uint32_t* count_in, uint32_t* q_out, uint32_t* count_out, dim3 grid, hipStream_t sm) {
        hipLaunchKernelGGL(k_im_shade, grid, dim3(256), 0, sm, P, W, G, q_in, count_in, q_out, count_out);
    };
    pass.accumulate = [&](const WfBuffers& W, dim3 grid, hipStream_t sm) { hipLaunchKernelGGL(k_im_accumulate, grid, dim3(256), 0, sm, P, W, G, P.first_sample); };
    const int rc = wf_first_hit_passes(state, P, tiles, pass, stream, trace_ms_out);
    if (rc || !sp.mem) return rc;          /* (no list: no tiles or no samples, nothing was launched) */
    WavefrontState* const st = *state;
    unsigned long long ctr[2] = {0, 0};
    WF_TRY(hipMemcpyAsync(ctr, sp.ctr, 16, hipMemcpyDeviceToHost, stream));
    WF_TRY(hipStreamSynchronize(stream));
    if (ctr[1]) {
        wf_set_error(std::to_string(ctr[1]) + " samples reached pixels more than one away from their own: the matte would be incomplete");
        return FTN_ERR_INTERNAL;
    }
    if (ctr[0] > cap) {
        wf_set_error(std::to_string(ctr[0]) + " samples reach other pixels, the list holds " + std::to_string(cap) + ": render the samples in several ranges");
        return FTN_ERR_OUT_OF_MEMORY;
    }
    if (ctr[0]) {
        const size_t npix = fh_crop_pixels(P);
        int end_bit = 33; while (end_bit < 64 && ((unsigned long long)npix >> (end_bit - 32)) != 0ull) end_bit++;
        hipcub::DoubleBuffer<unsigned long long> keys(sp.key[0], sp.key[1]), vals(sp.val[0], sp.val[1]);
        size_t need = 0;
        WF_TRY(hipcub::DeviceRadixSort::SortPairs(nullptr, need, keys, vals, (int)ctr[0], 0, end_bit, stream));
        { const int rc2 = wf_grow(&st->sort_tmp, &st->sort_tmp_bytes, need); if (rc2) return rc2; }
        WF_TRY(hipcub::DeviceRadixSort::SortPairs(st->sort_tmp, need, keys, vals, (int)ctr[0], 0, end_bit, stream));
        hipLaunchKernelGGL(k_im_apply, dim3((unsigned)((ctr[0] + 255) / 256)), dim3(256), 0, stream, G, keys.Current(), vals.Current(), (size_t)ctr[0]);
        WF_TRY(hipStreamSynchronize(stream));            /* the list is freed on return */
    }
    WF_TRY(hipGetLastError());
    return FTN_OK;
}

}  // namespace ftn
