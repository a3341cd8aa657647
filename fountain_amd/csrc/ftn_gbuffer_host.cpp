/*
 * ftn_gbuffer_host.cpp -- C entry points of include/fountain_hip_gbuffer.h.
 *
 * The pass takes the steps of every render call (ftn_host_internal.h): the scene's tile-list cache and film accumulators (the samples whose
 * footprint leaves their own pixel are summed there), with PathIntegrator of max_depth 0 in the parameters.
 */
#include "ftn_stage_host.h"
#include "../../include/fountain_hip_gbuffer.h"
#include "ftn_gbuffer.h"

#include <cstring>

using namespace ftn;

extern "C" {

static_assert(sizeof(ftn_gbuffer_pixel) == 48, "ABI");
int ftn_gbuffer_abi_version(void) { return FTN_GBUFFER_ABI_VERSION; }

int ftn_render_gbuffer_device(const ftn_scene* cs, const ftn_camera_desc* cam, const ftn_film_desc* film, const ftn_sampler_desc* sd,
                              const ftn_tile_range* tr, const ftn_render_options* opt, void* device_pixels, void* stream_v, ftn_stats* st) {
    if (!cs || !cam || !film || !sd || !device_pixels) return fail(FTN_ERR_INVALID_ARGUMENT, "null argument");
    if (sd->kind == FTN_SAMPLER_TILE_SERIAL)
        return fail(FTN_ERR_UNSUPPORTED, "the G-buffer pass needs FTN_SAMPLER_INDEXED: with the tile-serial sampler a sample's camera ray depends on everything its tile drew before it");
    if (sd->kind != FTN_SAMPLER_INDEXED) return fail(FTN_ERR_INVALID_ARGUMENT, "unknown sampler kind");
    const uint32_t pipeline = opt ? opt->pipeline : FTN_PIPELINE_AUTO;
    if (pipeline == FTN_PIPELINE_MEGAKERNEL) return fail(FTN_ERR_UNSUPPORTED, "the G-buffer pass runs on the wavefront pipeline (FTN_PIPELINE_AUTO or FTN_PIPELINE_WAVEFRONT)");
    if (pipeline != FTN_PIPELINE_AUTO && pipeline != FTN_PIPELINE_WAVEFRONT) return fail(FTN_ERR_INVALID_ARGUMENT, "unknown pipeline");
    if (int no = need_device()) return no;
    ftn_scene* s = const_cast<ftn_scene*>(cs);
    int rc = bind_scene_device(s, opt); if (rc) return rc;
    hipStream_t stream = (hipStream_t)stream_v;
    if ((uint64_t)sd->first_sample > (uint64_t)sd->samples_per_pixel || (uint64_t)sd->first_sample + (uint64_t)sd->sample_count > (uint64_t)sd->samples_per_pixel)
        return fail(FTN_ERR_INVALID_ARGUMENT, "sample range outside [0, samples_per_pixel]");

    ftn_integrator_desc first_hit; memset(&first_hit, 0, sizeof(first_hit)); first_hit.kind = FTN_INTEGRATOR_PATH;
    RenderParams P = render_params(s, cam, film, sd, &first_hit);
    if ((rc = scene_tiles(s, film, tr, stream, &P)) || (rc = prepare_film(s, false, stream, &P))) return rc;
    EventPair ev; if ((rc = ev.start(stream))) return rc;
    double trace_ms = 0.0;
    if ((rc = wavefront_gbuffer(&s->wf, P, s->sel, cam->camera_to_world.inv, (float*)device_pixels, P.accA, P.accB, P.accC, stream, &trace_ms))) return fail(rc, wavefront_error());
    float ms; if ((rc = ev.stop(stream, &ms))) return rc;
    DevStats ds; if ((rc = read_stats(s, false, &ds))) return rc;
    if (st) {
        memset(st, 0, sizeof(*st));
        st->rays_closest = ds.rays_closest; st->camera_samples = ds.camera_samples; st->spill_samples = ds.spill_samples;
        st->kernel_ms = ms; st->trace_ms = trace_ms;
    }
    return FTN_OK;
}

int ftn_render_gbuffer(const ftn_scene* cs, const ftn_camera_desc* cam, const ftn_film_desc* film, const ftn_sampler_desc* sd,
                       const ftn_tile_range* tr, const ftn_render_options* opt, ftn_gbuffer_pixel* out_pixels, ftn_stats* st) {
    if (!cs || !cam || !film || !sd || !out_pixels) return fail(FTN_ERR_INVALID_ARGUMENT, "null argument");
    if (sd->kind == FTN_SAMPLER_TILE_SERIAL || (opt && opt->pipeline == FTN_PIPELINE_MEGAKERNEL))          /* (the refusals come before any device work) */
        return ftn_render_gbuffer_device(cs, cam, film, sd, tr, opt, out_pixels, nullptr, st);
    if (int no = need_device()) return no;
    int rc = bind_scene_device(cs, opt); if (rc) return rc;
    const size_t npix = (size_t)std::max(0, film->crop[2] - film->crop[0]) * (size_t)std::max(0, film->crop[3] - film->crop[1]);
    /* the caller's sums go to the device and come back: every pixel's own samples are added to them one at a time (not summed apart and
     * added at the end), so splitting a sample range over calls gives the bits of one call */
    DevBuf<ftn_gbuffer_pixel> dev;
    if ((rc = dev.upload(out_pixels, npix))) { dev.release(); return rc; }
    rc = ftn_render_gbuffer_device(cs, cam, film, sd, tr, opt, dev.p ? (void*)dev.p : (void*)out_pixels, nullptr, st);
    if (rc == FTN_OK && npix && hipMemcpy(out_pixels, dev.p, npix * sizeof(ftn_gbuffer_pixel), hipMemcpyDeviceToHost) != hipSuccess) rc = fail(FTN_ERR_NO_DEVICE, "copy back failed");
    dev.release();
    return rc;
}

int ftn_gbuffer_resolve(const ftn_gbuffer_pixel* in, size_t n, float* out12) {
    if (n && (!in || !out12)) return fail(FTN_ERR_INVALID_ARGUMENT, "null argument");
    for (size_t i = 0; i < n; i++) gbuffer_resolve_pixel(in[i].albedo, out12 + 12 * i);
    return FTN_OK;
}

int ftn_gbuffer_resolve_device(const void* in, size_t n, void* out12, void* stream) {
    if (n && (!in || !out12)) return fail(FTN_ERR_INVALID_ARGUMENT, "null argument");
    if (ftn_device_count() <= 0) return fail(FTN_ERR_NO_DEVICE, "no HIP device");
    launch_gbuffer_resolve((const float*)in, n, (float*)out12, (hipStream_t)stream);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(FTN_ERR_INTERNAL, hipGetErrorString(e));
    return FTN_OK;
}

}  /* extern "C" */
