/*
 * ftn_moments.hip -- per-pixel second moments of the camera samples' radiance (include/fountain_hip_moments.h), beside the beauty.
 *
 * The pass is part of the wavefront pipeline's translation unit: this file includes ftn_gbuffer.hip (which includes ftn_wavefront.hip)
 * and the Makefile compiles it in its place, so that the driver shares the pipeline's internals -- WavefrontState and its per-path
 * radiance, wf_reserve, the pass size rules, FilmCtxW -- without exporting them, and the sources of the beauty's kernels stay as they are.
 */
#include "ftn_gbuffer.hip"
#include "ftn_moments.h"

namespace ftn {

/* ================================================================== second moments (include/fountain_hip_moments.h)
 * wavefront_render leaves the radiance of its last pass's samples in WfBuffers::rad (path id = slot * samples + s).  wavefront_moments
 * therefore calls it over chunks of the sample range that it runs as one pass each, and after each chunk k_mo_accumulate adds the
 * squares of those samples.  The beauty's accumulators are not cleared between chunks, so its kernels run exactly as in one ftn_render
 * call with passes of that size. */

/* one sample's squares into every pixel of its box-filter footprint (wf_film_add's rule): the own pixel in registers, others into the
 * in-tile or other-tile sum by atomics */
__device__ inline void mo_film_add(const MomentAcc& M, const FilmCtxW& F, V2 p_film, float4 q, int own_x, int own_y, float4* acc) {
    const float pdx = p_film.x - 0.5f, pdy = p_film.y - 0.5f;
    int p0x = f2i_sat(ceilf(pdx - F.radius[0])), p0y = f2i_sat(ceilf(pdy - F.radius[1]));
    int p1x = f2i_sat(floorf(pdx + F.radius[0])) + 1, p1y = f2i_sat(floorf(pdy + F.radius[1])) + 1;
    p0x = max(p0x, F.tpb[0]); p0y = max(p0y, F.tpb[1]); p1x = min(p1x, F.tpb[2]); p1y = min(p1y, F.tpb[3]);
    const size_t width = (size_t)(F.crop[2] - F.crop[0]);
    for (int y = p0y; y < p1y; y++)
        for (int x = p0x; x < p1x; x++) {
            if (x == own_x && y == own_y) { acc->x += q.x; acc->y += q.y; acc->z += q.z; acc->w += q.w; continue; }
            const bool in_tile = x >= F.sb[0] && x < F.sb[2] && y >= F.sb[1] && y < F.sb[3];
            float* f = reinterpret_cast<float*>((in_tile ? M.in_tile : M.other_tile) + ((size_t)(y - F.crop[1]) * width + (size_t)(x - F.crop[0])));
            atomicAdd(f + 0, q.x); atomicAdd(f + 1, q.y); atomicAdd(f + 2, q.z); atomicAdd(f + 3, q.w);
        }
}

/* k_wf_accumulate's structure for the four squares: one thread per pixel slot adds its samples in sample order; the workgroup stages
 * MO_ACC_CHUNK samples of its 256 slots through LDS with coalesced loads.  The beauty's statistics (spill, bc_writes, NaN) are the
 * beauty kernel's: this one counts nothing. */
#define MO_ACC_CHUNK 8u
__global__ void __launch_bounds__(256) k_mo_accumulate(RenderParams P, WfBuffers W, MomentAcc M) {
    __shared__ float4 s_rad[256 * MO_ACC_CHUNK];
    const uint32_t slot = blockIdx.x * 256u + threadIdx.x;
    bool valid = false, in_crop = false; int px = 0, py = 0; size_t ai = 0;
    FilmCtxW F; float4 acc = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (slot < W.n_slots) {
        const DTile tile = P.tiles[slot >> 8];
        px = tile.x0 + (int)(slot & 15u); py = tile.y0 + (int)((slot >> 4) & 15u);
        if (px < tile.x1 && py < tile.y1) {
            valid = true;
            for (int i = 0; i < 4; i++) F.crop[i] = P.crop[i];
            F.sb[0] = tile.x0; F.sb[1] = tile.y0; F.sb[2] = tile.x1; F.sb[3] = tile.y1; F.radius[0] = P.radius[0]; F.radius[1] = P.radius[1];
            const int p0x = f2i_sat(ceilf((float)tile.x0 - 0.5f - P.radius[0])), p0y = f2i_sat(ceilf((float)tile.y0 - 0.5f - P.radius[1]));
            const int p1x = f2i_sat(ceilf((float)tile.x1 - 0.5f + P.radius[0] + 1.0f)), p1y = f2i_sat(ceilf((float)tile.y1 - 0.5f - P.radius[1] + 1.0f));
            F.tpb[0] = max(p0x, P.crop[0]); F.tpb[1] = max(p0y, P.crop[1]); F.tpb[2] = min(p1x, P.crop[2]); F.tpb[3] = min(p1y, P.crop[3]);
            in_crop = px >= P.crop[0] && px < P.crop[2] && py >= P.crop[1] && py < P.crop[3];
            ai = in_crop ? ((size_t)(py - P.crop[1]) * (size_t)(P.crop[2] - P.crop[0]) + (size_t)(px - P.crop[0])) : 0;
            if (in_crop) acc = M.own[ai];
        }
    }
    const size_t block_first = (size_t)blockIdx.x * 256u * W.samples;          /* first path of this workgroup's 256 slots */
    for (uint32_t s0 = 0; s0 < W.samples; s0 += MO_ACC_CHUNK) {
        const uint32_t n = W.samples - s0 < MO_ACC_CHUNK ? W.samples - s0 : MO_ACC_CHUNK;
        for (uint32_t e = threadIdx.x; e < 256u * n; e += 256u) {                /* n consecutive samples of slot e / n */
            const uint32_t sl = e / n, k = e - sl * n;
            const size_t p = block_first + (size_t)sl * W.samples + s0 + k;
            if (p < W.n_paths) s_rad[sl * MO_ACC_CHUNK + k] = W.rad[p];
        }
        __syncthreads();
        if (valid) {
            for (uint32_t k = 0; k < n; k++) {
                const float4 l = s_rad[threadIdx.x * MO_ACC_CHUNK + k];
                float xyz[3];
                rgb_to_xyz(Rgb(l.x, l.y, l.z), xyz);
                const float4 q = make_float4(l.x * l.x, l.y * l.y, l.z * l.z, xyz[1] * xyz[1]);
                /* the sample's film position: the first two draws of its stream, exactly as k_wf_generate made them */
                Rng crng; crng.seed(indexed_key(P.seed, px, py, W.first_sample + s0 + k));
                const V2 j = crng.next2();
                mo_film_add(M, F, V2((float)px + j.x, (float)py + j.y), q, in_crop ? px : (-2147483647), py, &acc);
            }
        }
        __syncthreads();
    }
    if (valid && in_crop) M.own[ai] = acc;
}

/* after the last chunk: out += own + in-tile, then out += other-tile (the spill sums are only read when a sample left its own pixel) */
__global__ void __launch_bounds__(256) k_mo_merge(MomentAcc M, float4* __restrict__ out, size_t n, const DevStats* __restrict__ stats) {
    const bool spilled = stats->bc_writes != 0;
    for (size_t i = (size_t)blockIdx.x * 256u + threadIdx.x; i < n; i += (size_t)gridDim.x * 256u) {
        const float4 a = M.own[i], zero = make_float4(0.0f, 0.0f, 0.0f, 0.0f), b = spilled ? M.in_tile[i] : zero;
        float4 o = out[i];
        o.x += a.x + b.x; o.y += a.y + b.y; o.z += a.z + b.z; o.w += a.w + b.w;
        if (spilled) { const float4 c = M.other_tile[i]; o.x += c.x; o.y += c.y; o.z += c.z; o.w += c.w; }
        out[i] = o;
    }
}
void launch_moments_merge(const RenderParams& P, const MomentAcc& M, float4* out, hipStream_t stream) {
    const size_t n = (size_t)std::max(0, P.crop[2] - P.crop[0]) * (size_t)std::max(0, P.crop[3] - P.crop[1]);
    if (n == 0) return;
    hipLaunchKernelGGL(k_mo_merge, dim3((unsigned)std::min<size_t>((n + 255) / 256, 4096)), dim3(256), 0, stream, M, out, n, (const DevStats*)P.stats);
}

__global__ void __launch_bounds__(256) k_mo_resolve(const float* __restrict__ pix, const float* __restrict__ m, size_t n, float* __restrict__ out4) {
    for (size_t i = (size_t)blockIdx.x * 256u + threadIdx.x; i < n; i += (size_t)gridDim.x * 256u) moments_resolve_pixel(pix + 4 * i, m + 4 * i, out4 + 4 * i);
}
void launch_moments_resolve(const float* pix, const float* m, size_t n, float* out4, hipStream_t stream) {
    if (n == 0) return;
    hipLaunchKernelGGL(k_mo_resolve, dim3((unsigned)std::min<size_t>((n + 255) / 256, 4096)), dim3(256), 0, stream, pix, m, n, out4);
}

int wavefront_moments(WavefrontState** state, const RenderParams& P, const std::vector<DTile>& tiles, bool count, bool count_production,
                      const MomentAcc& M, hipStream_t stream, WavefrontTimes* times) {
    knobs_begin();
    { int rc0 = wf_state_init(state); if (rc0) return rc0; }
    WavefrontState* st = *state;
    const uint32_t n_slots = (uint32_t)tiles.size() * 256u;
    const uint32_t total_samples = P.last_sample - P.first_sample;
    if (n_slots == 0 || total_samples == 0) return FTN_OK;
    if (tiles.size() > ((size_t)1 << 20)) { g_wf_err = "more than 2^20 tiles (2^28 pixel slots) in one call: render the film in several tile ranges"; return FTN_ERR_UNSUPPORTED; }
    /* the chunk: the pass size wavefront_render picks (FTN_WF_PATHS_M, at most 2^28 paths, the direct-lighting / Whitted slot cap), and
     * the wavefront reserved for it here, halved while it does not fit, so that wavefront_render finds it in place and runs one pass */
    uint32_t S = (uint32_t)std::max<size_t>(1, ((size_t)std::min<uint32_t>(knob("FTN_WF_PATHS_M", 256), 256u) << 20) / n_slots);
    S = std::min(S, total_samples);
    const bool dl_mode = P.integrator_kind != FTN_INTEGRATOR_PATH, whitted = P.integrator_kind == FTN_INTEGRATOR_WHITTED;
    uint32_t dl_levels = 0, dl_slots = 0;
    if (dl_mode) {
        if (whitted && P.S.n_lights > WF_WH_MAX_LIGHTS) { g_wf_err = "the wavefront pipeline runs WhittedIntegrator for up to 32 lights (one bit per light in a path's pending-light word)"; return FTN_ERR_UNSUPPORTED; }
        dl_levels = std::max<uint32_t>(1u, std::min<uint32_t>(P.max_depth, WF_DL_MAX)); dl_slots = whitted ? std::max<uint32_t>(P.S.n_lights, 1u) : 1u;
        const size_t cap = ((size_t)1 << 31) / std::max<uint32_t>(dl_slots, 2u) - 1u;
        if ((size_t)n_slots > cap) { g_wf_err = "too many pixel slots for this many lights in one call: render the film in several tile ranges"; return FTN_ERR_UNSUPPORTED; }
        S = (uint32_t)std::max<size_t>(1, std::min<size_t>(S, cap / n_slots));
    }
    auto reserve = [&](uint32_t samples) -> int {
        int r = wf_reserve(st, (size_t)samples * n_slots);
        if (!r && dl_mode) r = wf_reserve_dl(st, st->cap_paths, dl_levels, dl_slots, P.S.n_textures != 0);
        return r;
    };
    int rc = reserve(S);
    while (rc == FTN_ERR_OUT_OF_MEMORY && S > 1) {
        wf_free(st); wf_free_dl(st); (void)hipGetLastError();
        S = (S + 1) / 2;
        rc = reserve(S);
    }
    if (rc) { wf_free(st); wf_free_dl(st); return rc; }
    if (times) memset(times, 0, sizeof(*times));
    for (uint32_t s0 = 0; s0 < total_samples; s0 += S) {
        const uint32_t Sp = std::min(S, total_samples - s0);
        RenderParams Pc = P;
        Pc.first_sample = P.first_sample + s0; Pc.last_sample = Pc.first_sample + Sp;
        WavefrontTimes t; memset(&t, 0, sizeof(t));
        if ((rc = wavefront_render(state, Pc, tiles, count, stream, &t, count_production))) return rc;
        if (st->cap_paths < (size_t)Sp * n_slots) {        /* it had to shrink the wavefront: WfBuffers::rad holds only its last pass */
            g_wf_err = "the wavefront pipeline split a chunk of the moments pass into several passes";
            return FTN_ERR_INTERNAL;
        }
        WfBuffers W = st->W;
        W.n_slots = n_slots; W.samples = Sp; W.n_paths = Sp * n_slots; W.first_sample = Pc.first_sample;
        hipLaunchKernelGGL(k_mo_accumulate, dim3((n_slots + 255) / 256), dim3(256), 0, stream, Pc, W, M);
        if (times) {
            times->trace_ms += t.trace_ms; times->trace_launches += t.trace_launches; times->any_ms += t.any_ms; times->any_launches += t.any_launches;
            times->shade_ms += t.shade_ms; times->shade_launches += t.shade_launches; times->sort_ms += t.sort_ms; times->mis_any_rays += t.mis_any_rays;
        }
    }
    WF_TRY(hipGetLastError());
    return FTN_OK;
}

}  // namespace ftn
