/*
 * ftn_denoise_host.cpp -- C entry points of include/fountain_hip_denoise.h and include/fountain_hip_denoise_guided.h.
 *
 * The filter's math is ftn_denoise.h's, shared with the kernels; the refusals' shared parts and the device buffers of the host-buffer
 * entries are the stages' scaffold's (ftn_stage_host.h).  The plain and the guided filter are one set of entries over the params block.
 */
#include "ftn_stage_host.h"
#include "ftn_denoise.h"

#include <cstring>
#include <type_traits>

using namespace ftn;

namespace {

/* only the guided filter (P = ftn_denoise_guided_params) reads var4 */
template <class P> constexpr bool kGuided = std::is_same<P, ftn_denoise_guided_params>::value;

/* the refusals of a params block: `name` is the block's name in the messages */
template <class P> int params_check(const P* p, const std::string& name, std::initializer_list<float P::*> sigmas, std::initializer_list<float P::*> epsilons) {
    if (p->levels < 0 || p->levels > FTN_DENOISE_MAX_LEVELS) return fail(FTN_ERR_INVALID_ARGUMENT, name + ".levels must be in 0..10");
    if (p->flags & ~(uint32_t)FTN_DENOISE_DEMODULATE) return fail(FTN_ERR_INVALID_ARGUMENT, "unknown " + name + ".flags bits");
    if (p->reserved != 0) return fail(FTN_ERR_INVALID_ARGUMENT, name + ".reserved must be 0");
    for (float P::*s : sigmas)
        if (!(p->*s > 0.0f) || !is_finite(p->*s)) return fail(FTN_ERR_INVALID_ARGUMENT, "a sigma of " + name + " is not finite or not positive");
    for (float P::*e : epsilons)
        if (!(p->*e >= 0.0f) || !is_finite(p->*e)) return fail(FTN_ERR_INVALID_ARGUMENT, "an epsilon of " + name + " is negative or not finite");
    return FTN_OK;
}

/* the refusals every entry point shares */
template <class P> int check(const void* rgb, const void* gb12, const void* var4, int32_t w, int32_t h, const P* p, const void* out_rgb) {
    if (!rgb || !gb12 || (kGuided<P> && !var4) || !p || !out_rgb) return fail(FTN_ERR_INVALID_ARGUMENT, "null argument");
    if (int rc = image_check(w, h)) return rc;
    if constexpr (kGuided<P>)
        return params_check(p, "ftn_denoise_guided_params", {&P::sigma_variance, &P::sigma_normal, &P::sigma_plane}, {&P::albedo_eps, &P::rel_eps});
    else
        return params_check(p, "ftn_denoise_params", {&P::sigma_color, &P::sigma_normal, &P::sigma_plane}, {&P::albedo_eps, &P::color_eps});
}

template <class P> int denoise_device(const float* rgb, const float* gb12, const float* var4, int32_t w, int32_t h, const P* p, float* out_rgb,
                                      float4* workspace, hipStream_t stream) {
    if (!workspace) return fail(FTN_ERR_INVALID_ARGUMENT, "null argument");
    int rc = check(rgb, gb12, var4, w, h, p, out_rgb); if (rc) return rc;
    const size_t n = (size_t)w * (size_t)h;
    const Range r_rgb = {rgb, 12 * n, 4}, r_gb = {gb12, 48 * n, 4}, r_var = {kGuided<P> ? var4 : nullptr, 16 * n, 4}, r_out = {out_rgb, 12 * n, 4},
                r_ws = {workspace, 64 * n, 16};
    if ((rc = overlap_check({r_out}, {r_rgb, r_gb, r_var, r_ws}, "out_rgb overlaps an input or the workspace"))) return rc;
    if ((rc = overlap_check({r_ws}, {r_rgb, r_gb, r_var}, "the workspace overlaps an input"))) return rc;
    if ((rc = align_check({r_ws, r_rgb, r_gb, r_var, r_out}, "misaligned buffer: the workspace needs 16 bytes, the images 4"))) return rc;
    if ((rc = need_device())) return rc;
    if constexpr (kGuided<P>) return launched(launch_denoise_guided(rgb, gb12, var4, w, h, *p, out_rgb, workspace, stream), "guided denoise");
    else return launched(launch_denoise(rgb, gb12, w, h, *p, out_rgb, workspace, stream), "denoise");
}

template <class P> int denoise_host(const float* rgb, const float* gb12, const float* var4, int32_t w, int32_t h, const P* p, float* out_rgb, int32_t device) {
    int rc = check(rgb, gb12, var4, w, h, p, out_rgb); if (rc) return rc;
    if ((rc = need_device()) || (rc = set_device(device))) return rc;
    const size_t n = (size_t)w * (size_t)h;
    StageBufs bufs;
    float *d_rgb, *d_gb, *d_var, *d_out;
    float4* d_ws;
    if ((rc = bufs.upload(rgb, 3 * n, &d_rgb)) || (rc = bufs.upload(gb12, 12 * n, &d_gb)) || (rc = bufs.upload(kGuided<P> ? var4 : nullptr, 4 * n, &d_var)) ||
        (rc = bufs.alloc(3 * n, &d_out)) || (rc = bufs.alloc(4 * n, &d_ws))) return rc;
    if ((rc = denoise_device(d_rgb, d_gb, d_var, w, h, p, d_out, d_ws, nullptr))) return rc;
    return bufs.copy_back(out_rgb, d_out, 3 * n);
}

/* the host twin: the device path's buffers and steps, each pixel computed by the shared code from the previous step's buffers alone; the
 * last level writes out (3 floats per pixel) */
template <class P> int denoise_cpu(const float* rgb, const float* gb12, const float* var4, int32_t w, int32_t h, const P* p, float* out_rgb) {
    int rc = check(rgb, gb12, var4, w, h, p, out_rgb); if (rc) return rc;
    const size_t n = (size_t)w * (size_t)h;
    if (p->levels == 0) { memmove(out_rgb, rgb, 3 * n * sizeof(float)); return FTN_OK; }
    std::vector<float4> col0(n), col1(n), fnc(n), fxz(n);
    std::vector<float> out(3 * n);
    const uint32_t flags = p->flags;
    const float aeps = p->albedo_eps;
    parallel_for(n, [&](size_t i0, size_t i1) {
        for (size_t i = i0; i < i1; i++) {
            if constexpr (kGuided<P>) dn_guided_prepare_pixel(rgb + 3 * i, gb12 + 12 * i, var4 + 4 * i, flags, aeps, &col0[i], &fnc[i], &fxz[i]);
            else dn_prepare_pixel(rgb + 3 * i, gb12 + 12 * i, flags, aeps, &col0[i], &fnc[i], &fxz[i]);
        }
    });
    float4* col[2] = {col0.data(), col1.data()};
    for (int l = 0; l < p->levels; l++) {
        const auto L = [&] { if constexpr (kGuided<P>) return dn_guided_level(*p, l); else return dn_level(*p, l); }();
        const bool last = l == p->levels - 1;
        const float4* in = col[l & 1];
        float4* dst = col[(l + 1) & 1];
        parallel_for(n, [&](size_t i0, size_t i1) {
            for (size_t i = i0; i < i1; i++) {
                const int x = (int)(i % (size_t)w), y = (int)(i / (size_t)w);
                const float4 u = dn_atrous_pixel(in, fnc.data(), fxz.data(), w, h, x, y, L);
                if (last) dn_finish_pixel(u, gb12 + 12 * i, flags, aeps, &out[3 * i]);
                else dst[i] = u;
            }
        });
    }
    memcpy(out_rgb, out.data(), 3 * n * sizeof(float));          /* (out_rgb may alias the inputs on the host path) */
    return FTN_OK;
}

}  // namespace

extern "C" {

static_assert(sizeof(ftn_denoise_params) == 32 && sizeof(ftn_denoise_guided_params) == 32, "ABI");
int ftn_denoise_abi_version(void) { return FTN_DENOISE_ABI_VERSION; }
int ftn_denoise_guided_abi_version(void) { return FTN_DENOISE_GUIDED_ABI_VERSION; }

void ftn_denoise_params_default(ftn_denoise_params* p) {
    if (!p) return;
    p->levels = 5;
    p->flags = FTN_DENOISE_DEMODULATE;
    p->sigma_color = 2.0f;
    p->sigma_normal = 0.3f;
    p->sigma_plane = 1e-4f;
    p->albedo_eps = 1e-3f;
    p->color_eps = 1e-4f;
    p->reserved = 0;
}

void ftn_denoise_guided_params_default(ftn_denoise_guided_params* p) {
    if (!p) return;
    p->levels = 5;
    p->flags = FTN_DENOISE_DEMODULATE;
    p->sigma_variance = 2.0f;
    p->sigma_normal = 0.3f;
    p->sigma_plane = 0.1f;
    p->albedo_eps = 1e-3f;
    p->rel_eps = 1e-4f;
    p->reserved = 0;
}

int ftn_denoise_workspace_size(int32_t w, int32_t h, size_t* bytes) {
    if (!bytes) return fail(FTN_ERR_INVALID_ARGUMENT, "null argument");
    if (int rc = image_check(w, h)) return rc;
    *bytes = (size_t)w * (size_t)h * 4 * sizeof(float4);
    return FTN_OK;
}
int ftn_denoise_guided_workspace_size(int32_t w, int32_t h, size_t* bytes) { return ftn_denoise_workspace_size(w, h, bytes); }

int ftn_denoise_device(const void* rgb, const void* gb12, int32_t w, int32_t h, const ftn_denoise_params* p, void* out_rgb, void* workspace, void* stream) {
    return denoise_device((const float*)rgb, (const float*)gb12, nullptr, w, h, p, (float*)out_rgb, (float4*)workspace, (hipStream_t)stream);
}
int ftn_denoise(const float* rgb, const float* gb12, int32_t w, int32_t h, const ftn_denoise_params* p, float* out_rgb, int32_t device) {
    return denoise_host(rgb, gb12, nullptr, w, h, p, out_rgb, device);
}
int ftn_denoise_cpu(const float* rgb, const float* gb12, int32_t w, int32_t h, const ftn_denoise_params* p, float* out_rgb) {
    return denoise_cpu(rgb, gb12, nullptr, w, h, p, out_rgb);
}

int ftn_denoise_guided_device(const void* rgb, const void* gb12, const void* var4, int32_t w, int32_t h, const ftn_denoise_guided_params* p,
                              void* out_rgb, void* workspace, void* stream) {
    return denoise_device((const float*)rgb, (const float*)gb12, (const float*)var4, w, h, p, (float*)out_rgb, (float4*)workspace, (hipStream_t)stream);
}
int ftn_denoise_guided(const float* rgb, const float* gb12, const float* var4, int32_t w, int32_t h, const ftn_denoise_guided_params* p,
                       float* out_rgb, int32_t device) {
    return denoise_host(rgb, gb12, var4, w, h, p, out_rgb, device);
}
int ftn_denoise_guided_cpu(const float* rgb, const float* gb12, const float* var4, int32_t w, int32_t h, const ftn_denoise_guided_params* p,
                           float* out_rgb) {
    return denoise_cpu(rgb, gb12, var4, w, h, p, out_rgb);
}

}  /* extern "C" */
