/*
 * ftn_temporal_host.cpp -- C entry points of include/fountain_hip_temporal.h.
 *
 * The per-pixel code is ftn_temporal.h's, shared with the kernel; the refusals' shared parts and the device buffers of the host-buffer entry are
 * the stages' scaffold's (ftn_stage_host.h).
 */
#include "ftn_stage_host.h"
#include "ftn_temporal.h"

#include <cstring>

using namespace ftn;

namespace {

/* the refusals every entry point shares (the buffers' pointers are checked by the callers); fills the frame's constants */
static int temporal_check(const ftn_camera_desc* cur, const ftn_film_desc* film, int32_t w, int32_t h, const ftn_camera_desc* prev,
                          const void* prev_gb12, const void* prev_history, const ftn_temporal_params* p, TpFrame* F) {
    if (!cur || !film || !p) return fail(FTN_ERR_INVALID_ARGUMENT, "null argument");
    const int n_prev = (prev != nullptr) + (prev_gb12 != nullptr) + (prev_history != nullptr);
    if (n_prev != 0 && n_prev != 3)
        return fail(FTN_ERR_INVALID_ARGUMENT, "prev_camera, prev_gb12 and prev_history must be all null (the first frame) or all given");
    if (int rc = image_check(w, h)) return rc;
    if ((int64_t)film->crop[2] - (int64_t)film->crop[0] != w || (int64_t)film->crop[3] - (int64_t)film->crop[1] != h)
        return fail(FTN_ERR_INVALID_ARGUMENT, "the film's crop is not w x h pixels");
    if (p->flags & ~(uint32_t)FTN_DENOISE_DEMODULATE) return fail(FTN_ERR_INVALID_ARGUMENT, "unknown ftn_temporal_params.flags bits");
    if (p->reserved[0] != 0 || p->reserved[1] != 0) return fail(FTN_ERR_INVALID_ARGUMENT, "ftn_temporal_params.reserved must be 0");
    if (!(p->alpha_min >= 0.0f && p->alpha_min <= 1.0f)) return fail(FTN_ERR_INVALID_ARGUMENT, "ftn_temporal_params.alpha_min must be in 0..1");
    for (float t : {p->normal_tol, p->plane_tol, p->albedo_tol})
        if (!(t >= 0.0f) || !is_finite(t)) return fail(FTN_ERR_INVALID_ARGUMENT, "a tolerance of ftn_temporal_params is negative or not finite");
    if (!(p->albedo_eps >= 0.0f) || !is_finite(p->albedo_eps)) return fail(FTN_ERR_INVALID_ARGUMENT, "ftn_temporal_params.albedo_eps is negative or not finite");
    F->cur = tp_camera(*cur);
    F->prev = tp_camera(prev ? *prev : *cur);
    F->same_view = prev && tp_same_view(F->cur, F->prev);
    F->w = w; F->h = h; F->x0 = film->crop[0]; F->y0 = film->crop[1];
    F->flags = p->flags;
    F->alpha_min = p->alpha_min; F->normal_tol = p->normal_tol; F->plane_tol = p->plane_tol; F->albedo_eps = p->albedo_eps; F->albedo_tol = p->albedo_tol;
    return FTN_OK;
}

}  // namespace

extern "C" {

static_assert(sizeof(ftn_temporal_params) == 32 && sizeof(ftn_temporal_pixel) == 32, "ABI");
int ftn_temporal_abi_version(void) { return FTN_TEMPORAL_ABI_VERSION; }

void ftn_temporal_params_default(ftn_temporal_params* p) {
    if (!p) return;
    p->flags = FTN_DENOISE_DEMODULATE;
    p->alpha_min = 0.4f;
    p->normal_tol = 0.01f;
    p->plane_tol = 1e-3f;
    p->albedo_eps = 1e-3f;
    p->albedo_tol = 0.01f;
    p->reserved[0] = p->reserved[1] = 0;
}

int ftn_temporal_accumulate_device(const void* rgb, const void* gb12, const void* var4, const ftn_camera_desc* cur_camera, const ftn_film_desc* film,
                                   int32_t w, int32_t h, const ftn_camera_desc* prev_camera, const void* prev_gb12, const void* prev_history,
                                   const ftn_temporal_params* p, void* out_history, void* out_rgb, void* out_var4, void* stream) {
    return tp_accumulate_device(rgb, gb12, var4, nullptr, cur_camera, film, w, h, prev_camera, prev_gb12, prev_history, p, out_history, out_rgb, out_var4, stream);
}

int ftn_temporal_accumulate(const float* rgb, const float* gb12, const float* var4, const ftn_camera_desc* cur_camera, const ftn_film_desc* film,
                            int32_t w, int32_t h, const ftn_camera_desc* prev_camera, const float* prev_gb12, const ftn_temporal_pixel* prev_history,
                            const ftn_temporal_params* p, ftn_temporal_pixel* out_history, float* out_rgb, float* out_var4, int32_t device) {
    return tp_accumulate_host(rgb, gb12, var4, nullptr, cur_camera, film, w, h, prev_camera, prev_gb12, prev_history, p, out_history, out_rgb, out_var4, device);
}

int ftn_temporal_accumulate_cpu(const float* rgb, const float* gb12, const float* var4, const ftn_camera_desc* cur_camera, const ftn_film_desc* film,
                                int32_t w, int32_t h, const ftn_camera_desc* prev_camera, const float* prev_gb12, const ftn_temporal_pixel* prev_history,
                                const ftn_temporal_params* p, ftn_temporal_pixel* out_history, float* out_rgb, float* out_var4) {
    return tp_accumulate_cpu(rgb, gb12, var4, nullptr, cur_camera, film, w, h, prev_camera, prev_gb12, prev_history, p, out_history, out_rgb, out_var4);
}

}  /* extern "C" */

/* ------------------------------------------------------------------ the entry points' bodies (ftn_temporal.h); mv8 may be null */
namespace ftn {

int tp_accumulate_device(const void* rgb, const void* gb12, const void* var4, const void* mv8, const ftn_camera_desc* cur_camera, const ftn_film_desc* film,
                         int32_t w, int32_t h, const ftn_camera_desc* prev_camera, const void* prev_gb12, const void* prev_history,
                         const ftn_temporal_params* p, void* out_history, void* out_rgb, void* out_var4, void* stream) {
    if (!rgb || !gb12 || !var4 || !out_history || !out_rgb || !out_var4) return fail(FTN_ERR_INVALID_ARGUMENT, "null argument");
    TpFrame F;
    int rc = temporal_check(cur_camera, film, w, h, prev_camera, prev_gb12, prev_history, p, &F); if (rc) return rc;
    const size_t n = (size_t)w * (size_t)h;
    const Range r_rgb = {rgb, 12 * n, 4}, r_gb = {gb12, 48 * n, 4}, r_var = {var4, 16 * n, 4}, r_pgb = {prev_gb12, 48 * n, 4}, r_ph = {prev_history, 32 * n, 16},
                r_mv = {mv8, 32 * n, 4}, r_oh = {out_history, 32 * n, 16}, r_out = {out_rgb, 12 * n, 4}, r_ovar = {out_var4, 16 * n, 4};
    if ((rc = overlap_check({r_oh, r_out, r_ovar}, {r_rgb, r_gb, r_var, r_pgb, r_ph, r_mv}, "an output overlaps an input", "two outputs overlap"))) return rc;
    if ((rc = align_check({r_oh, r_ph, r_rgb, r_gb, r_var, r_pgb, r_out, r_ovar, r_mv}, "misaligned buffer: the histories need 16 bytes, the images 4"))) return rc;
    if ((rc = need_device())) return rc;
    return launched(launch_temporal((const float*)rgb, (const float*)gb12, (const float*)var4, (const float*)prev_gb12, (const float4*)prev_history, F,
                                    (float4*)out_history, (float*)out_rgb, (float*)out_var4, (hipStream_t)stream, (const float*)mv8), "temporal accumulation");
}

int tp_accumulate_host(const float* rgb, const float* gb12, const float* var4, const float* mv8, const ftn_camera_desc* cur_camera, const ftn_film_desc* film,
                       int32_t w, int32_t h, const ftn_camera_desc* prev_camera, const float* prev_gb12, const ftn_temporal_pixel* prev_history,
                       const ftn_temporal_params* p, ftn_temporal_pixel* out_history, float* out_rgb, float* out_var4, int32_t device) {
    if (!rgb || !gb12 || !var4 || !out_history || !out_rgb || !out_var4) return fail(FTN_ERR_INVALID_ARGUMENT, "null argument");
    TpFrame F;
    int rc = temporal_check(cur_camera, film, w, h, prev_camera, prev_gb12, prev_history, p, &F); if (rc) return rc;
    if ((rc = need_device()) || (rc = set_device(device))) return rc;
    const size_t n = (size_t)w * (size_t)h;
    StageBufs bufs;
    float *d_rgb, *d_gb, *d_var, *d_pgb, *d_out, *d_ovar, *d_mv;
    ftn_temporal_pixel *d_ph, *d_oh;
    if ((rc = bufs.upload(rgb, 3 * n, &d_rgb)) || (rc = bufs.upload(gb12, 12 * n, &d_gb)) || (rc = bufs.upload(var4, 4 * n, &d_var)) ||
        (rc = bufs.upload(prev_gb12, 12 * n, &d_pgb)) || (rc = bufs.upload(prev_history, n, &d_ph)) ||      /* (null on the first frame) */
        (rc = bufs.upload(mv8, 8 * n, &d_mv)) ||                                                            /* (null for a static scene) */
        (rc = bufs.alloc(n, &d_oh)) || (rc = bufs.alloc(3 * n, &d_out)) || (rc = bufs.alloc(4 * n, &d_ovar))) return rc;
    if ((rc = tp_accumulate_device(d_rgb, d_gb, d_var, d_mv, cur_camera, film, w, h, prev_camera, d_pgb, d_ph, p, d_oh, d_out, d_ovar, nullptr))) return rc;
    if ((rc = bufs.copy_back(out_history, d_oh, n)) || (rc = bufs.copy_back(out_rgb, d_out, 3 * n))) return rc;
    return bufs.copy_back(out_var4, d_ovar, 4 * n);
}

int tp_accumulate_cpu(const float* rgb, const float* gb12, const float* var4, const float* mv8, const ftn_camera_desc* cur_camera, const ftn_film_desc* film,
                      int32_t w, int32_t h, const ftn_camera_desc* prev_camera, const float* prev_gb12, const ftn_temporal_pixel* prev_history,
                      const ftn_temporal_params* p, ftn_temporal_pixel* out_history, float* out_rgb, float* out_var4) {
    if (!rgb || !gb12 || !var4 || !out_history || !out_rgb || !out_var4) return fail(FTN_ERR_INVALID_ARGUMENT, "null argument");
    TpFrame F;
    int rc = temporal_check(cur_camera, film, w, h, prev_camera, prev_gb12, prev_history, p, &F); if (rc) return rc;
    const size_t n = (size_t)w * (size_t)h;
    /* (the outputs may alias the inputs on the host path: every pixel is computed into buffers of the call's own first) */
    std::vector<float4> hist(2 * n), prev_copy;
    std::vector<float> out(3 * n), ovar(4 * n);
    const float4* prev = (const float4*)prev_history;
    if (prev_history && (uintptr_t)prev_history % 16) {           /* float4 loads want 16 bytes; a host caller need not give them */
        prev_copy.resize(2 * n);
        memcpy(prev_copy.data(), prev_history, n * sizeof(ftn_temporal_pixel));
        prev = prev_copy.data();
    }
    parallel_for(n, [&](size_t i0, size_t i1) {
        for (size_t i = i0; i < i1; i++)
            tp_accumulate_pixel(rgb, gb12, var4, prev_gb12, prev, F, (int)(i % (size_t)w), (int)(i / (size_t)w), hist.data(),
                                out.data(), ovar.data(), mv8);
    });
    memcpy(out_history, hist.data(), n * sizeof(ftn_temporal_pixel));
    memcpy(out_rgb, out.data(), 3 * n * sizeof(float));
    memcpy(out_var4, ovar.data(), 4 * n * sizeof(float));
    return FTN_OK;
}

}  // namespace ftn
