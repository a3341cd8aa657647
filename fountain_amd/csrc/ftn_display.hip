/*
 * ftn_display.hip -- the kernels and device drivers of the display stage (include/fountain_hip_display.h).  The per-pixel code is
 * ftn_display.h's, shared with the host twin; this file needs no scene internals and is its own translation unit.  Both kernels are
 * memory-bound streams: a thread takes four consecutive pixels per trip (three 16-byte loads), the last n mod 4 pixels go through a
 * scalar tail.
 *
 *   k_disp_hist_clear  97 16-byte stores: the histogram's clear on the call's stream
 *   k_disp_histogram   a private histogram per wave in LDS (4 x 388 words), cleared at the start; each lane keeps the bin and the
 *                      count of its current run of equal bins and adds to LDS only when the bin changes; at the end the four copies
 *                      are summed and every non-zero word goes to global memory with one integer atomic
 *   k_disp_encode      twelve floats in, four packed words out in one 16-byte store, the optional float image in three more
 */
#include "ftn_display.h"
#include <algorithm>

namespace ftn {

/* the histogram's clear, a kernel of its own rather than a memset so that a captured graph holds nothing but kernel nodes */
__global__ void __launch_bounds__(128) k_disp_hist_clear(uint4* __restrict__ hist) {
    if (threadIdx.x < FTN_DISPLAY_HIST_WORDS / 4) hist[threadIdx.x] = make_uint4(0u, 0u, 0u, 0u);
}

__global__ void __launch_bounds__(256) k_disp_histogram(const float* __restrict__ rgb, uint32_t n, uint32_t* __restrict__ hist) {
    __shared__ uint32_t s_hist[4 * FTN_DISPLAY_HIST_WORDS];
    for (uint32_t i = threadIdx.x; i < 4u * FTN_DISPLAY_HIST_WORDS; i += 256u) s_hist[i] = 0u;
    __syncthreads();
    uint32_t* const mine = s_hist + (threadIdx.x >> 6) * FTN_DISPLAY_HIST_WORDS;
    uint32_t run_bin = 0u, run = 0u;
    auto count = [&](float r, float g, float b) {
        const uint32_t bin = disp_bin(disp_luminance(r, g, b));
        if (bin != run_bin) {
            if (run) atomicAdd(&mine[run_bin], run);
            run_bin = bin; run = 0u;
        }
        run++;
    };
    const uint32_t n4 = n >> 2, t = blockIdx.x * 256u + threadIdx.x, stride = gridDim.x * 256u;
    for (uint32_t q = t; q < n4; q += stride) {
        const float4* const p = reinterpret_cast<const float4*>(rgb) + 3u * (size_t)q;
        const float4 a = p[0], b = p[1], c = p[2];
        count(a.x, a.y, a.z); count(a.w, b.x, b.y); count(b.z, b.w, c.x); count(c.y, c.z, c.w);
    }
    if (t < (n & 3u)) {
        const float* const p = rgb + 3u * (size_t)(4u * n4 + t);
        count(p[0], p[1], p[2]);
    }
    if (run) atomicAdd(&mine[run_bin], run);
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < FTN_DISPLAY_HIST_WORDS; i += 256u) {
        const uint32_t v = s_hist[i] + s_hist[FTN_DISPLAY_HIST_WORDS + i] + s_hist[2 * FTN_DISPLAY_HIST_WORDS + i] + s_hist[3 * FTN_DISPLAY_HIST_WORDS + i];
        if (v) atomicAdd(&hist[i], v);
    }
}

__global__ void __launch_bounds__(256) k_disp_encode(const float* __restrict__ rgb, uint32_t w, uint32_t n, DispEncode e, float* __restrict__ out_rgb,
                                                     uint32_t* __restrict__ out_rgba8) {
    const uint32_t n4 = n >> 2, t = blockIdx.x * 256u + threadIdx.x, stride = gridDim.x * 256u;
    for (uint32_t q = t; q < n4; q += stride) {
        const float4* const p = reinterpret_cast<const float4*>(rgb) + 3u * (size_t)q;
        const float4 a = p[0], b = p[1], c = p[2];
        /* each of the four pixels has its own (x, y): a group may straddle the end of a row */
        uint32_t y = (4u * q) / w, x = 4u * q - y * w;
        float o[12];
        uint4 code;
        code.x = disp_pixel(a.x, a.y, a.z, x, y, e, o);
        if (++x == w) { x = 0u; y++; }
        code.y = disp_pixel(a.w, b.x, b.y, x, y, e, o + 3);
        if (++x == w) { x = 0u; y++; }
        code.z = disp_pixel(b.z, b.w, c.x, x, y, e, o + 6);
        if (++x == w) { x = 0u; y++; }
        code.w = disp_pixel(c.y, c.z, c.w, x, y, e, o + 9);
        reinterpret_cast<uint4*>(out_rgba8)[q] = code;
        if (out_rgb) {
            float4* const d = reinterpret_cast<float4*>(out_rgb) + 3u * (size_t)q;
            d[0] = make_float4(o[0], o[1], o[2], o[3]); d[1] = make_float4(o[4], o[5], o[6], o[7]); d[2] = make_float4(o[8], o[9], o[10], o[11]);
        }
    }
    if (t < (n & 3u)) {
        const uint32_t i = 4u * n4 + t, y = i / w, x = i - y * w;
        const float* const p = rgb + 3u * (size_t)i;
        float o[3];
        out_rgba8[i] = disp_pixel(p[0], p[1], p[2], x, y, e, o);
        if (out_rgb) { float* const d = out_rgb + 3u * (size_t)i; d[0] = o[0]; d[1] = o[1]; d[2] = o[2]; }
    }
}

static unsigned display_grid(uint32_t n, unsigned cap) { return std::max(1u, std::min(((n >> 2) + 255u) / 256u, cap)); }

hipError_t launch_display_histogram(const float* rgb, uint32_t n, uint32_t* hist, hipStream_t stream) {
    static_assert(FTN_DISPLAY_HIST_WORDS / 4 <= 128, "one workgroup clears the histogram");
    hipLaunchKernelGGL(k_disp_hist_clear, dim3(1), dim3(128), 0, stream, reinterpret_cast<uint4*>(hist));
    hipLaunchKernelGGL(k_disp_histogram, dim3(display_grid(n, FTN_DISPLAY_HIST_MAX_BLOCKS)), dim3(256), 0, stream, rgb, n, hist);
    return hipGetLastError();
}

hipError_t launch_display_encode(const float* rgb, uint32_t w, uint32_t n, const DispEncode& e, float* out_rgb, uint32_t* out_rgba8, hipStream_t stream) {
    hipLaunchKernelGGL(k_disp_encode, dim3(display_grid(n, FTN_DISPLAY_ENCODE_MAX_BLOCKS)), dim3(256), 0, stream, rgb, w, n, e, out_rgb, out_rgba8);
    return hipGetLastError();
}

}  // namespace ftn
