/*
 * ftn_idmatte_host.cpp -- C entry points of include/fountain_hip_idmatte.h (ftn_exr_write_channels is in ftn_imageio.cpp).
 *
 * The pass takes the steps of every render call (ftn_host_internal.h), as the G-buffer's does, with PathIntegrator of max_depth 0 in the
 * parameters; the caller's ids are permuted into the scene's BVH order here and uploaded for the call.
 */
#include "ftn_stage_host.h"
#include "../../include/fountain_hip_idmatte.h"
#include "ftn_idmatte.h"

#include <cstring>

using namespace ftn;

extern "C" {

static_assert(sizeof(ftn_idmatte_pixel) == 80 && sizeof(ftn_idmatte_pixel) == IM_WORDS * 4 && FTN_IDMATTE_SLOTS == IM_SLOTS && FTN_IDMATTE_RESOLVED_WORDS == IM_WORDS, "ABI");
int ftn_idmatte_abi_version(void) { return FTN_IDMATTE_ABI_VERSION; }

/* every refusal that needs no device, in the order of the header */
static int idmatte_refusals(const ftn_scene* cs, const ftn_camera_desc* cam, const ftn_film_desc* film, const ftn_sampler_desc* sd, const ftn_render_options* opt,
                            const uint32_t* prim_ids, size_t n_prim_ids, const void* out) {
    if (!cs || !cam || !film || !sd || !prim_ids || !out) return fail(FTN_ERR_INVALID_ARGUMENT, "null argument");
    if (int no = indexed_sampler_check(sd, "ID-matte")) return no;
    if (int no = wavefront_pipeline_check(opt, "ID-matte")) return no;
    if (!(film->filter_radius[0] <= 1.0f) || !(film->filter_radius[1] <= 1.0f))
        return fail(FTN_ERR_UNSUPPORTED, "the ID-matte pass takes footprints of up to 3 x 3 pixels: a filter radius of at most 1 in each axis");
    if (int no = sample_range_check(sd)) return no;
    if (sd->samples_per_pixel >= (1u << IM_SAMPLE_BITS)) return fail(FTN_ERR_UNSUPPORTED, "the ID-matte pass takes fewer than 2^28 samples per pixel");
    if (crop_pixels(film) >= ((size_t)1 << 31)) return fail(FTN_ERR_INVALID_ARGUMENT, "the crop window must be below 2^31 pixels");
    return FTN_OK;
}

int ftn_render_idmatte_device(const ftn_scene* cs, const ftn_camera_desc* cam, const ftn_film_desc* film, const ftn_sampler_desc* sd,
                              const ftn_tile_range* tr, const ftn_render_options* opt, const uint32_t* prim_ids, size_t n_prim_ids,
                              void* device_pixels, void* stream_v, ftn_stats* st) {
    if (int no = idmatte_refusals(cs, cam, film, sd, opt, prim_ids, n_prim_ids, device_pixels)) return no;
    if (int no = need_device()) return no;
    if (n_prim_ids != cs->host.order.size()) return fail(FTN_ERR_INVALID_ARGUMENT, "n_prim_ids must be the scene's primitive count (" + std::to_string(cs->host.order.size()) + ")");
    ftn_scene* s = const_cast<ftn_scene*>(cs);
    int rc = bind_scene_device(s, opt); if (rc) return rc;
    hipStream_t stream = (hipStream_t)stream_v;

    /* the caller's ids in insertion order -> BVH order, the order the traversal reports primitives in (ftn_scene_get_nodes) */
    std::vector<uint32_t> ids(n_prim_ids);
    for (size_t i = 0; i < n_prim_ids; i++) {
        const uint32_t o = s->host.order[i];
        if (o >= n_prim_ids) return fail(FTN_ERR_INTERNAL, "the scene's primitive order is corrupt");
        ids[i] = prim_ids[o];
    }
    StageBufs bufs;
    uint32_t* d_ids = nullptr;
    if ((rc = bufs.upload(ids.data(), ids.size(), &d_ids))) return rc;
    return first_hit_render(s, cam, film, sd, tr, stream, st, [&](const RenderParams& P, double* trace_ms) {        /* (it drains the stream before a failing return: d_ids is freed here) */
        return wavefront_idmatte(&s->wf, P, s->sel, d_ids, (uint32_t*)device_pixels, stream, trace_ms);
    });
}

int ftn_render_idmatte(const ftn_scene* cs, const ftn_camera_desc* cam, const ftn_film_desc* film, const ftn_sampler_desc* sd,
                       const ftn_tile_range* tr, const ftn_render_options* opt, const uint32_t* prim_ids, size_t n_prim_ids,
                       ftn_idmatte_pixel* out_pixels, ftn_stats* st) {
    if (int no = idmatte_refusals(cs, cam, film, sd, opt, prim_ids, n_prim_ids, out_pixels)) return no;
    if (int no = need_device()) return no;
    if (n_prim_ids != cs->host.order.size()) return fail(FTN_ERR_INVALID_ARGUMENT, "n_prim_ids must be the scene's primitive count (" + std::to_string(cs->host.order.size()) + ")");
    if (int rc = bind_scene_device(cs, opt)) return rc;
    /* the caller's tables go to the device and come back: the call continues them */
    return continue_on_device(out_pixels, crop_pixels(film), [&](void* d) { return ftn_render_idmatte_device(cs, cam, film, sd, tr, opt, prim_ids, n_prim_ids, d, nullptr, st); });
}

int ftn_idmatte_resolve(const ftn_idmatte_pixel* in, size_t n, void* out20) {
    if (n && (!in || !out20)) return fail(FTN_ERR_INVALID_ARGUMENT, "null argument");
    for (size_t i = 0; i < n; i++) idmatte_resolve_pixel(in[i].id, (uint32_t*)out20 + IM_WORDS * i);
    return FTN_OK;
}

int ftn_idmatte_resolve_device(const void* in, size_t n, void* out20, void* stream) {
    if (n && (!in || !out20)) return fail(FTN_ERR_INVALID_ARGUMENT, "null argument");
    if (int no = need_device()) return no;
    return launched(launch_idmatte_resolve((const uint32_t*)in, n, (uint32_t*)out20, (hipStream_t)stream), "ID-matte resolve");
}

static int select_refusals(const void* resolved, size_t n, const uint32_t* ids, size_t n_ids, uint32_t flags, const void* mask) {
    if ((n && (!resolved || !mask)) || (n_ids && !ids)) return fail(FTN_ERR_INVALID_ARGUMENT, "null argument");
    if (flags & ~(FTN_IDMATTE_SELECT_OVERFLOW | FTN_IDMATTE_SELECT_MISS)) return fail(FTN_ERR_INVALID_ARGUMENT, "unknown flag bits");
    return FTN_OK;
}

int ftn_idmatte_select(const void* resolved, size_t n, const uint32_t* ids, size_t n_ids, uint32_t flags, float* mask_out) {
    if (int no = select_refusals(resolved, n, ids, n_ids, flags, mask_out)) return no;
    std::vector<uint32_t> sorted(ids, ids + n_ids);
    std::sort(sorted.begin(), sorted.end());
    for (size_t i = 0; i < n; i++) mask_out[i] = idmatte_select_pixel((const uint32_t*)resolved + IM_WORDS * i, sorted.data(), n_ids, flags);
    return FTN_OK;
}

int ftn_idmatte_select_device(const void* resolved, size_t n, const uint32_t* ids, size_t n_ids, uint32_t flags, void* mask_out, void* stream_v) {
    if (int no = select_refusals(resolved, n, ids, n_ids, flags, mask_out)) return no;
    if (int no = need_device()) return no;
    if (n == 0) return FTN_OK;
    std::vector<uint32_t> sorted(ids, ids + n_ids);
    std::sort(sorted.begin(), sorted.end());
    StageBufs bufs;
    uint32_t* d_ids = nullptr;
    if (int rc = bufs.upload(sorted.data(), sorted.size(), &d_ids)) return rc;
    hipStream_t stream = (hipStream_t)stream_v;
    launch_idmatte_select((const uint32_t*)resolved, n, d_ids, n_ids, flags, (float*)mask_out, stream);
    const int rc = launched(hipGetLastError(), "ID-matte select");
    if (hipStreamSynchronize(stream) != hipSuccess && rc == FTN_OK) return fail(FTN_ERR_INTERNAL, "ID-matte select failed");      /* the sorted ids are freed on return */
    return rc;
}

}  /* extern "C" */
