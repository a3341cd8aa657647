/*
 * ftn_filter.hip -- the reconstruction-filtered film (include/fountain_hip_filter.h) as a deterministic gather beside the beauty.
 *
 * A unit of its own: the driver is a wavefront_render call (ftn_wavefront.h) with a per-pass hook, and k_ff_gather reads the layout of
 * a pass's buffers through ftn_wf_common.h.  Nothing here adds with atomics: every crop pixel has one writer.
 */
#include "ftn_wf_common.h"
#include "ftn_filter.h"
#include <algorithm>

namespace ftn {

/* ================================================================== the gather
 * wavefront_render leaves the radiance of a pass's samples in WfBuffers::rad (path id = slot * samples + s) until the next pass
 * overwrites it, and a pass always holds every selected tile, so all the samples that can reach a pixel are in the pass that holds the
 * pixel's own.
 *
 * One 256-thread workgroup per output tile, one thread per pixel.  Per chunk of sample indices the workgroup stages, for every pixel of
 * its tile grown by the margin (mx, my), the sample's radiance and its pd = p_film - 0.5 -- p_film redrawn from the sample's key exactly
 * as k_wf_generate and k_wf_accumulate draw it -- through LDS with coalesced loads (the samples of a slot are neighbours in memory, the
 * slots of a tile row are too).  Each thread then runs the header's loop for its pixel from LDS: s outermost, the window row-major.
 * Window pixels outside the sample bounds or in a tile the call does not render have slot -1 and contribute nothing.
 *
 * Dynamic LDS: float4 rad[chunk][npx], float2 pd[chunk][npx], int slot[npx], float table[256]; npx = (16 + 2 mx) (16 + 2 my). */
size_t filter_gather_lds(int mx, int my, uint32_t chunk) {
    const size_t npx = (size_t)(16 + 2 * mx) * (size_t)(16 + 2 * my);
    return (size_t)chunk * npx * (sizeof(float4) + sizeof(float2)) + npx * sizeof(int) + 256 * sizeof(float);
}

__global__ void __launch_bounds__(256) k_ff_gather(RenderParams P, WfBuffers W, FilterGather G) {
    extern __shared__ float4 s_ff[];
    const int ww = 16 + 2 * G.mx, wh = 16 + 2 * G.my;
    const uint32_t npx = (uint32_t)(ww * wh);
    float4* const s_rad = s_ff;
    float2* const s_pd = reinterpret_cast<float2*>(s_rad + (size_t)G.chunk * npx);
    int* const s_slot = reinterpret_cast<int*>(s_pd + (size_t)G.chunk * npx);
    float* const s_tab = reinterpret_cast<float*>(s_slot + npx);

    const FilterOutTile ot = G.out_tiles[blockIdx.x];
    const int ox0 = G.sb[0] + 16 * ot.gx, oy0 = G.sb[1] + 16 * ot.gy;
    const int wx0 = ox0 - G.mx, wy0 = oy0 - G.my;
    s_tab[threadIdx.x] = G.T.w[threadIdx.x];
    for (uint32_t w = threadIdx.x; w < npx; w += 256u) {
        const int x = wx0 + (int)(w % (uint32_t)ww), y = wy0 + (int)(w / (uint32_t)ww);
        int slot = -1;
        if (x >= G.sb[0] && x < G.sb[2] && y >= G.sb[1] && y < G.sb[3]) {
            const int lx = x - G.sb[0], ly = y - G.sb[1];
            const int k = G.grid_map[(ly >> 4) * G.grid_w + (lx >> 4)];
            if (k >= 0 && (uint32_t)k < P.n_tiles) slot = k * 256 + (ly & 15) * 16 + (lx & 15);
        }
        s_slot[w] = slot;
    }
    const int lx = (int)(threadIdx.x & 15u), ly = (int)(threadIdx.x >> 4);
    const int qx = ox0 + lx, qy = oy0 + ly;
    const bool in_crop = qx >= P.crop[0] && qx < P.crop[2] && qy >= P.crop[1] && qy < P.crop[3];
    const size_t ai = in_crop ? (size_t)(qy - P.crop[1]) * (size_t)(P.crop[2] - P.crop[0]) + (size_t)(qx - P.crop[0]) : 0;
    float4 acc = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (in_crop) acc = G.acc[ai];
    const float rx = G.T.radius[0], ry = G.T.radius[1], inv_rx = G.T.inv_radius[0], inv_ry = G.T.inv_radius[1];
    __syncthreads();
    for (uint32_t s0 = 0; s0 < W.samples; s0 += G.chunk) {
        const uint32_t n = W.samples - s0 < G.chunk ? W.samples - s0 : G.chunk;
        for (uint32_t e = threadIdx.x; e < npx * n; e += 256u) {                 /* n consecutive samples of window pixel e / n */
            const uint32_t w = e / n, k = e - w * n;
            const int slot = s_slot[w];
            if (slot < 0) continue;
            s_rad[k * npx + w] = W.rad[(size_t)slot * W.samples + s0 + k];
            const int x = wx0 + (int)(w % (uint32_t)ww), y = wy0 + (int)(w / (uint32_t)ww);
            /* the sample's film position: the first two draws of its stream (k_wf_accumulate) */
            Rng crng; crng.seed(indexed_key(P.seed, x, y, W.first_sample + s0 + k));
            const V2 j = crng.next2();
            const V2 p_film((float)x + j.x, (float)y + j.y);
            s_pd[k * npx + w] = make_float2(p_film.x - 0.5f, p_film.y - 0.5f);
        }
        __syncthreads();
        if (in_crop) {
            for (uint32_t k = 0; k < n; k++) {
                const float4* const rad = s_rad + k * npx; const float2* const pdk = s_pd + k * npx;
                for (int wy = ly; wy <= ly + 2 * G.my; wy++)
                    for (int wx = lx; wx <= lx + 2 * G.mx; wx++) {
                        const int w = wy * ww + wx;
                        if (s_slot[w] < 0) continue;
                        const float2 pd = pdk[w]; const float4 l = rad[w];
                        filter_add_term(s_tab, rx, ry, inv_rx, inv_ry, V2(pd.x, pd.y), qx, qy, l.x, l.y, l.z, &acc.x, &acc.y, &acc.z, &acc.w);
                    }
            }
        }
        __syncthreads();
    }
    if (in_crop) G.acc[ai] = acc;
}

/* after the last pass: out += {rgb_to_xyz(acc.rgb), acc.w} for every crop pixel */
__global__ void __launch_bounds__(256) k_ff_merge(const float4* __restrict__ acc, float4* __restrict__ out, size_t n) {
    for (size_t i = (size_t)blockIdx.x * 256u + threadIdx.x; i < n; i += (size_t)gridDim.x * 256u) {
        const float4 a = acc[i];
        float xyz[3];
        rgb_to_xyz(Rgb(a.x, a.y, a.z), xyz);
        float4 o = out[i];
        o.x += xyz[0]; o.y += xyz[1]; o.z += xyz[2]; o.w += a.w;
        out[i] = o;
    }
}
void launch_filter_merge(const RenderParams& P, const float4* acc, float4* out, hipStream_t stream) {
    const size_t n = (size_t)std::max(0, P.crop[2] - P.crop[0]) * (size_t)std::max(0, P.crop[3] - P.crop[1]);
    if (n == 0) return;
    hipLaunchKernelGGL(k_ff_merge, dim3((unsigned)std::min<size_t>((n + 255) / 256, 4096)), dim3(256), 0, stream, acc, out, n);
}

static void filtered_pass(void* ctx, const RenderParams& P, const WfBuffers& W, hipStream_t stream) {
    const FilterGather& G = *static_cast<const FilterGather*>(ctx);
    if (G.n_out_tiles == 0) return;
    hipLaunchKernelGGL(k_ff_gather, dim3(G.n_out_tiles), dim3(256), filter_gather_lds(G.mx, G.my, G.chunk), stream, P, W, G);
}
int wavefront_filtered(WavefrontState** state, const RenderParams& P, const std::vector<DTile>& tiles, bool count, bool count_production,
                       const FilterGather& G, hipStream_t stream, WavefrontTimes* times) {
    return wavefront_render(state, P, tiles, count, stream, times, count_production, filtered_pass, const_cast<FilterGather*>(&G));
}

}  // namespace ftn
