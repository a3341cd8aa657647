/*
 * ftn_denoise_host.cpp -- C entry points of include/fountain_hip_denoise.h and include/fountain_hip_denoise_guided.h.
 *
 * The filter's math is ftn_denoise.h's, shared with the kernels; error reporting, device selection and the host thread budget are the host
 * library's (ftn_host_internal.h).
 */
#include "ftn_host_internal.h"
#include "ftn_denoise.h"

#include <cstring>

using namespace ftn;

extern "C" {

static_assert(sizeof(ftn_denoise_params) == 32, "ABI");
int ftn_denoise_abi_version(void) { return FTN_DENOISE_ABI_VERSION; }

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

}  /* extern "C" */

namespace {

static int image_check(int32_t w, int32_t h) {
    if (w <= 0 || h <= 0) return fail(FTN_ERR_INVALID_ARGUMENT, "image width and height must be positive");
    if ((int64_t)w * (int64_t)h >= ((int64_t)1 << 31)) return fail(FTN_ERR_INVALID_ARGUMENT, "w * h must be below 2^31 pixels");
    return FTN_OK;
}

/* the refusals every entry point shares (the pointers are checked by the callers) */
static int denoise_check(int32_t w, int32_t h, const ftn_denoise_params* p) {
    if (!p) return fail(FTN_ERR_INVALID_ARGUMENT, "null argument");
    if (int rc = image_check(w, h)) return rc;
    if (p->levels < 0 || p->levels > FTN_DENOISE_MAX_LEVELS) return fail(FTN_ERR_INVALID_ARGUMENT, "ftn_denoise_params.levels must be in 0..10");
    if (p->flags & ~(uint32_t)FTN_DENOISE_DEMODULATE) return fail(FTN_ERR_INVALID_ARGUMENT, "unknown ftn_denoise_params.flags bits");
    if (p->reserved != 0) return fail(FTN_ERR_INVALID_ARGUMENT, "ftn_denoise_params.reserved must be 0");
    for (float s : {p->sigma_color, p->sigma_normal, p->sigma_plane})
        if (!(s > 0.0f) || !dn_finite(s)) return fail(FTN_ERR_INVALID_ARGUMENT, "a sigma of ftn_denoise_params is not finite or not positive");
    for (float e : {p->albedo_eps, p->color_eps})
        if (!(e >= 0.0f) || !dn_finite(e)) return fail(FTN_ERR_INVALID_ARGUMENT, "an epsilon of ftn_denoise_params is negative or not finite");
    return FTN_OK;
}

static int denoise_guided_check(int32_t w, int32_t h, const ftn_denoise_guided_params* p) {
    if (!p) return fail(FTN_ERR_INVALID_ARGUMENT, "null argument");
    if (int rc = image_check(w, h)) return rc;
    if (p->levels < 0 || p->levels > FTN_DENOISE_MAX_LEVELS) return fail(FTN_ERR_INVALID_ARGUMENT, "ftn_denoise_guided_params.levels must be in 0..10");
    if (p->flags & ~(uint32_t)FTN_DENOISE_DEMODULATE) return fail(FTN_ERR_INVALID_ARGUMENT, "unknown ftn_denoise_guided_params.flags bits");
    if (p->reserved != 0) return fail(FTN_ERR_INVALID_ARGUMENT, "ftn_denoise_guided_params.reserved must be 0");
    for (float s : {p->sigma_variance, p->sigma_normal, p->sigma_plane})
        if (!(s > 0.0f) || !dn_finite(s)) return fail(FTN_ERR_INVALID_ARGUMENT, "a sigma of ftn_denoise_guided_params is not finite or not positive");
    for (float e : {p->albedo_eps, p->rel_eps})
        if (!(e >= 0.0f) || !dn_finite(e)) return fail(FTN_ERR_INVALID_ARGUMENT, "an epsilon of ftn_denoise_guided_params is negative or not finite");
    return FTN_OK;
}

static bool overlaps(const void* a, size_t na, const void* b, size_t nb) {
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a0 < b0 + nb && b0 < a0 + na;
}

/* the levels of either filter on the host, after col[0], fnc and fxz are prepared: the device path's buffers and steps, each pixel
 * computed by the shared code from the previous step's buffers alone; the last level writes out (3 floats per pixel) */
template <class Params, class MakeLevel>
static void host_levels(const float* gb12, int32_t w, int32_t h, const Params& p, MakeLevel make_level, std::vector<float4>& col0,
                        const std::vector<float4>& fnc, const std::vector<float4>& fxz, float* out) {
    const size_t n = (size_t)w * (size_t)h;
    std::vector<float4> col1(n);
    float4* col[2] = {col0.data(), col1.data()};
    const uint32_t flags = p.flags;
    const float aeps = p.albedo_eps;
    for (int l = 0; l < p.levels; l++) {
        const auto L = make_level(p, l);
        const bool last = l == p.levels - 1;
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
}

}  // namespace

extern "C" {

int ftn_denoise_workspace_size(int32_t w, int32_t h, size_t* bytes) {
    if (!bytes) return fail(FTN_ERR_INVALID_ARGUMENT, "null argument");
    if (int rc = image_check(w, h)) return rc;
    *bytes = (size_t)w * (size_t)h * 4 * sizeof(float4);
    return FTN_OK;
}

int ftn_denoise_device(const void* rgb, const void* gb12, int32_t w, int32_t h, const ftn_denoise_params* p, void* out_rgb, void* workspace, void* stream) {
    if (!rgb || !gb12 || !p || !out_rgb || !workspace) return fail(FTN_ERR_INVALID_ARGUMENT, "null argument");
    int rc = denoise_check(w, h, p); if (rc) return rc;
    const size_t n = (size_t)w * (size_t)h, n_rgb = 3 * n * sizeof(float), n_gb = 12 * n * sizeof(float), n_ws = n * 4 * sizeof(float4);
    if (overlaps(out_rgb, n_rgb, rgb, n_rgb) || overlaps(out_rgb, n_rgb, gb12, n_gb) || overlaps(out_rgb, n_rgb, workspace, n_ws))
        return fail(FTN_ERR_INVALID_ARGUMENT, "out_rgb overlaps an input or the workspace");
    if (overlaps(workspace, n_ws, rgb, n_rgb) || overlaps(workspace, n_ws, gb12, n_gb)) return fail(FTN_ERR_INVALID_ARGUMENT, "the workspace overlaps an input");
    if ((uintptr_t)workspace % 16 || (uintptr_t)rgb % 4 || (uintptr_t)gb12 % 4 || (uintptr_t)out_rgb % 4)
        return fail(FTN_ERR_INVALID_ARGUMENT, "misaligned buffer: the workspace needs 16 bytes, the images 4");
    if (ftn_device_count() <= 0) return fail(FTN_ERR_NO_DEVICE, "no HIP device available: the fountain HIP path needs an AMD GPU (there is no CPU fallback)");
    const hipError_t e = launch_denoise((const float*)rgb, (const float*)gb12, w, h, *p, (float*)out_rgb, (float4*)workspace, (hipStream_t)stream);
    if (e != hipSuccess) return fail(FTN_ERR_INTERNAL, std::string("denoise launch: ") + hipGetErrorString(e));
    return FTN_OK;
}

int ftn_denoise(const float* rgb, const float* gb12, int32_t w, int32_t h, const ftn_denoise_params* p, float* out_rgb, int32_t device) {
    if (!rgb || !gb12 || !p || !out_rgb) return fail(FTN_ERR_INVALID_ARGUMENT, "null argument");
    int rc = denoise_check(w, h, p); if (rc) return rc;
    if (ftn_device_count() <= 0) return fail(FTN_ERR_NO_DEVICE, "no HIP device available: the fountain HIP path needs an AMD GPU (there is no CPU fallback)");
    if ((rc = set_device(device))) return rc;
    const size_t n = (size_t)w * (size_t)h;
    DevBuf<float> d_rgb, d_gb, d_out;
    DevBuf<float4> d_ws;
    struct Release { DevBuf<float>* a; DevBuf<float>* b; DevBuf<float>* c; DevBuf<float4>* d;
                     ~Release() { a->release(); b->release(); c->release(); d->release(); } } keep{&d_rgb, &d_gb, &d_out, &d_ws};
    if ((rc = d_rgb.upload(rgb, 3 * n)) || (rc = d_gb.upload(gb12, 12 * n))) return rc;
    HIP_TRY(hipMalloc((void**)&d_out.p, 3 * n * sizeof(float)));
    HIP_TRY(hipMalloc((void**)&d_ws.p, 4 * n * sizeof(float4)));
    if ((rc = ftn_denoise_device(d_rgb.p, d_gb.p, w, h, p, d_out.p, d_ws.p, nullptr))) return rc;
    HIP_TRY(hipMemcpy(out_rgb, d_out.p, 3 * n * sizeof(float), hipMemcpyDeviceToHost));
    return FTN_OK;
}

int ftn_denoise_cpu(const float* rgb, const float* gb12, int32_t w, int32_t h, const ftn_denoise_params* p, float* out_rgb) {
    if (!rgb || !gb12 || !p || !out_rgb) return fail(FTN_ERR_INVALID_ARGUMENT, "null argument");
    int rc = denoise_check(w, h, p); if (rc) return rc;
    const size_t n = (size_t)w * (size_t)h;
    if (p->levels == 0) { memmove(out_rgb, rgb, 3 * n * sizeof(float)); return FTN_OK; }
    std::vector<float4> col0(n), fnc(n), fxz(n);
    std::vector<float> out(3 * n);
    const uint32_t flags = p->flags;
    const float aeps = p->albedo_eps;
    parallel_for(n, [&](size_t i0, size_t i1) {
        for (size_t i = i0; i < i1; i++) dn_prepare_pixel(rgb + 3 * i, gb12 + 12 * i, flags, aeps, &col0[i], &fnc[i], &fxz[i]);
    });
    host_levels(gb12, w, h, *p, dn_level, col0, fnc, fxz, out.data());
    memcpy(out_rgb, out.data(), 3 * n * sizeof(float));          /* (out_rgb may alias the inputs on the host path) */
    return FTN_OK;
}

}  /* extern "C" */

/* ---- include/fountain_hip_denoise_guided.h ---- */

extern "C" {

static_assert(sizeof(ftn_denoise_guided_params) == 32, "ABI");
int ftn_denoise_guided_abi_version(void) { return FTN_DENOISE_GUIDED_ABI_VERSION; }

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

int ftn_denoise_guided_workspace_size(int32_t w, int32_t h, size_t* bytes) { return ftn_denoise_workspace_size(w, h, bytes); }

int ftn_denoise_guided_device(const void* rgb, const void* gb12, const void* var4, int32_t w, int32_t h, const ftn_denoise_guided_params* p,
                              void* out_rgb, void* workspace, void* stream) {
    if (!rgb || !gb12 || !var4 || !p || !out_rgb || !workspace) return fail(FTN_ERR_INVALID_ARGUMENT, "null argument");
    int rc = denoise_guided_check(w, h, p); if (rc) return rc;
    const size_t n = (size_t)w * (size_t)h, n_rgb = 3 * n * sizeof(float), n_gb = 12 * n * sizeof(float), n_var = 4 * n * sizeof(float),
                 n_ws = n * 4 * sizeof(float4);
    if (overlaps(out_rgb, n_rgb, rgb, n_rgb) || overlaps(out_rgb, n_rgb, gb12, n_gb) || overlaps(out_rgb, n_rgb, var4, n_var) ||
        overlaps(out_rgb, n_rgb, workspace, n_ws))
        return fail(FTN_ERR_INVALID_ARGUMENT, "out_rgb overlaps an input or the workspace");
    if (overlaps(workspace, n_ws, rgb, n_rgb) || overlaps(workspace, n_ws, gb12, n_gb) || overlaps(workspace, n_ws, var4, n_var))
        return fail(FTN_ERR_INVALID_ARGUMENT, "the workspace overlaps an input");
    if ((uintptr_t)workspace % 16 || (uintptr_t)rgb % 4 || (uintptr_t)gb12 % 4 || (uintptr_t)var4 % 4 || (uintptr_t)out_rgb % 4)
        return fail(FTN_ERR_INVALID_ARGUMENT, "misaligned buffer: the workspace needs 16 bytes, the images 4");
    if (ftn_device_count() <= 0) return fail(FTN_ERR_NO_DEVICE, "no HIP device available: the fountain HIP path needs an AMD GPU (there is no CPU fallback)");
    const hipError_t e = launch_denoise_guided((const float*)rgb, (const float*)gb12, (const float*)var4, w, h, *p, (float*)out_rgb,
                                               (float4*)workspace, (hipStream_t)stream);
    if (e != hipSuccess) return fail(FTN_ERR_INTERNAL, std::string("guided denoise launch: ") + hipGetErrorString(e));
    return FTN_OK;
}

int ftn_denoise_guided(const float* rgb, const float* gb12, const float* var4, int32_t w, int32_t h, const ftn_denoise_guided_params* p,
                       float* out_rgb, int32_t device) {
    if (!rgb || !gb12 || !var4 || !p || !out_rgb) return fail(FTN_ERR_INVALID_ARGUMENT, "null argument");
    int rc = denoise_guided_check(w, h, p); if (rc) return rc;
    if (ftn_device_count() <= 0) return fail(FTN_ERR_NO_DEVICE, "no HIP device available: the fountain HIP path needs an AMD GPU (there is no CPU fallback)");
    if ((rc = set_device(device))) return rc;
    const size_t n = (size_t)w * (size_t)h;
    DevBuf<float> d_rgb, d_gb, d_var, d_out;
    DevBuf<float4> d_ws;
    struct Release { DevBuf<float>* a; DevBuf<float>* b; DevBuf<float>* c; DevBuf<float>* d; DevBuf<float4>* e;
                     ~Release() { a->release(); b->release(); c->release(); d->release(); e->release(); } } keep{&d_rgb, &d_gb, &d_var, &d_out, &d_ws};
    if ((rc = d_rgb.upload(rgb, 3 * n)) || (rc = d_gb.upload(gb12, 12 * n)) || (rc = d_var.upload(var4, 4 * n))) return rc;
    HIP_TRY(hipMalloc((void**)&d_out.p, 3 * n * sizeof(float)));
    HIP_TRY(hipMalloc((void**)&d_ws.p, 4 * n * sizeof(float4)));
    if ((rc = ftn_denoise_guided_device(d_rgb.p, d_gb.p, d_var.p, w, h, p, d_out.p, d_ws.p, nullptr))) return rc;
    HIP_TRY(hipMemcpy(out_rgb, d_out.p, 3 * n * sizeof(float), hipMemcpyDeviceToHost));
    return FTN_OK;
}

int ftn_denoise_guided_cpu(const float* rgb, const float* gb12, const float* var4, int32_t w, int32_t h, const ftn_denoise_guided_params* p,
                           float* out_rgb) {
    if (!rgb || !gb12 || !var4 || !p || !out_rgb) return fail(FTN_ERR_INVALID_ARGUMENT, "null argument");
    int rc = denoise_guided_check(w, h, p); if (rc) return rc;
    const size_t n = (size_t)w * (size_t)h;
    if (p->levels == 0) { memmove(out_rgb, rgb, 3 * n * sizeof(float)); return FTN_OK; }
    std::vector<float4> col0(n), fnc(n), fxz(n);
    std::vector<float> out(3 * n);
    const uint32_t flags = p->flags;
    const float aeps = p->albedo_eps;
    parallel_for(n, [&](size_t i0, size_t i1) {
        for (size_t i = i0; i < i1; i++) dn_guided_prepare_pixel(rgb + 3 * i, gb12 + 12 * i, var4 + 4 * i, flags, aeps, &col0[i], &fnc[i], &fxz[i]);
    });
    host_levels(gb12, w, h, *p, dn_guided_level, col0, fnc, fxz, out.data());
    memcpy(out_rgb, out.data(), 3 * n * sizeof(float));          /* (out_rgb may alias the inputs on the host path) */
    return FTN_OK;
}

}  /* extern "C" */
