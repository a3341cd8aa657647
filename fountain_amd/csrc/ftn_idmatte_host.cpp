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
    if (sd->kind == FTN_SAMPLER_TILE_SERIAL)
        return fail(FTN_ERR_UNSUPPORTED, "the ID-matte pass needs FTN_SAMPLER_INDEXED: with the tile-serial sampler a sample's camera ray depends on everything its tile drew before it");
    if (sd->kind != FTN_SAMPLER_INDEXED) return fail(FTN_ERR_INVALID_ARGUMENT, "unknown sampler kind");
    const uint32_t pipeline = opt ? opt->pipeline : FTN_PIPELINE_AUTO;
    if (pipeline == FTN_PIPELINE_MEGAKERNEL) return fail(FTN_ERR_UNSUPPORTED, "the ID-matte pass runs on the wavefront pipeline (FTN_PIPELINE_AUTO or FTN_PIPELINE_WAVEFRONT)");
    if (pipeline != FTN_PIPELINE_AUTO && pipeline != FTN_PIPELINE_WAVEFRONT) return fail(FTN_ERR_INVALID_ARGUMENT, "unknown pipeline");
    if (!(film->filter_radius[0] <= 1.0f) || !(film->filter_radius[1] <= 1.0f))
        return fail(FTN_ERR_UNSUPPORTED, "the ID-matte pass takes footprints of up to 3 x 3 pixels: a filter radius of at most 1 in each axis");
    if ((uint64_t)sd->first_sample > (uint64_t)sd->samples_per_pixel || (uint64_t)sd->first_sample + (uint64_t)sd->sample_count > (uint64_t)sd->samples_per_pixel)
        return fail(FTN_ERR_INVALID_ARGUMENT, "sample range outside [0, samples_per_pixel]");
    if (sd->samples_per_pixel >= (1u << IM_SAMPLE_BITS)) return fail(FTN_ERR_UNSUPPORTED, "the ID-matte pass takes fewer than 2^28 samples per pixel");
    const int64_t npix = (int64_t)std::max(0, film->crop[2] - film->crop[0]) * (int64_t)std::max(0, film->crop[3] - film->crop[1]);
    if (npix >= ((int64_t)1 << 31)) return fail(FTN_ERR_INVALID_ARGUMENT, "the crop window must be below 2^31 pixels");
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

    ftn_integrator_desc first_hit; memset(&first_hit, 0, sizeof(first_hit)); first_hit.kind = FTN_INTEGRATOR_PATH;
    RenderParams P = render_params(s, cam, film, sd, &first_hit);
    if ((rc = scene_tiles(s, film, tr, stream, &P)) || (rc = prepare_film(s, false, stream, &P))) return rc;
    EventPair ev; if ((rc = ev.start(stream))) return rc;
    double trace_ms = 0.0;
    if ((rc = wavefront_idmatte(&s->wf, P, s->sel, d_ids, (uint32_t*)device_pixels, stream, &trace_ms))) {
        (void)hipStreamSynchronize(stream);              /* d_ids is freed on return */
        return fail(rc, wavefront_error());
    }
    float ms; if ((rc = ev.stop(stream, &ms))) return rc;
    DevStats ds; if ((rc = read_stats(s, false, &ds))) return rc;
    if (st) {
        memset(st, 0, sizeof(*st));
        st->rays_closest = ds.rays_closest; st->camera_samples = ds.camera_samples; st->spill_samples = ds.spill_samples;
        st->kernel_ms = ms; st->trace_ms = trace_ms;
    }
    return FTN_OK;
}

int ftn_render_idmatte(const ftn_scene* cs, const ftn_camera_desc* cam, const ftn_film_desc* film, const ftn_sampler_desc* sd,
                       const ftn_tile_range* tr, const ftn_render_options* opt, const uint32_t* prim_ids, size_t n_prim_ids,
                       ftn_idmatte_pixel* out_pixels, ftn_stats* st) {
    if (int no = idmatte_refusals(cs, cam, film, sd, opt, prim_ids, n_prim_ids, out_pixels)) return no;
    if (int no = need_device()) return no;
    if (n_prim_ids != cs->host.order.size()) return fail(FTN_ERR_INVALID_ARGUMENT, "n_prim_ids must be the scene's primitive count (" + std::to_string(cs->host.order.size()) + ")");
    int rc = bind_scene_device(cs, opt); if (rc) return rc;
    const size_t npix = (size_t)std::max(0, film->crop[2] - film->crop[0]) * (size_t)std::max(0, film->crop[3] - film->crop[1]);
    /* the caller's tables go to the device and come back: the call continues them */
    DevBuf<ftn_idmatte_pixel> dev;
    if ((rc = dev.upload(out_pixels, npix))) { dev.release(); return rc; }
    rc = ftn_render_idmatte_device(cs, cam, film, sd, tr, opt, prim_ids, n_prim_ids, dev.p ? (void*)dev.p : (void*)out_pixels, nullptr, st);
    if (rc == FTN_OK && npix && hipMemcpy(out_pixels, dev.p, npix * sizeof(ftn_idmatte_pixel), hipMemcpyDeviceToHost) != hipSuccess) rc = fail(FTN_ERR_NO_DEVICE, "copy back failed");
    dev.release();
    return rc;
}

int ftn_idmatte_resolve(const ftn_idmatte_pixel* in, size_t n, void* out20) {
    if (n && (!in || !out20)) return fail(FTN_ERR_INVALID_ARGUMENT, "null argument");
    for (size_t i = 0; i < n; i++) idmatte_resolve_pixel(in[i].id, (uint32_t*)out20 + IM_WORDS * i);
    return FTN_OK;
}

int ftn_idmatte_resolve_device(const void* in, size_t n, void* out20, void* stream) {
    if (n && (!in || !out20)) return fail(FTN_ERR_INVALID_ARGUMENT, "null argument");
    if (int no = need_device()) return no;
    launch_idmatte_resolve((const uint32_t*)in, n, (uint32_t*)out20, (hipStream_t)stream);
    return launched(hipGetLastError(), "ID-matte resolve");
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
