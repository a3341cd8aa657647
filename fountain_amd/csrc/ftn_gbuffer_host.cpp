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
    if (int no = indexed_sampler_check(sd, "G-buffer")) return no;
    if (int no = wavefront_pipeline_check(opt, "G-buffer")) return no;
    if (int no = need_device()) return no;
    ftn_scene* s = const_cast<ftn_scene*>(cs);
    if (int rc = bind_scene_device(s, opt)) return rc;
    hipStream_t stream = (hipStream_t)stream_v;
    if (int no = sample_range_check(sd)) return no;
    return first_hit_render(s, cam, film, sd, tr, stream, st, [&](const RenderParams& P, double* trace_ms) {
        return wavefront_gbuffer(&s->wf, P, s->sel, cam->camera_to_world.inv, (float*)device_pixels, stream, trace_ms);
    });
}

int ftn_render_gbuffer(const ftn_scene* cs, const ftn_camera_desc* cam, const ftn_film_desc* film, const ftn_sampler_desc* sd,
                       const ftn_tile_range* tr, const ftn_render_options* opt, ftn_gbuffer_pixel* out_pixels, ftn_stats* st) {
    if (!cs || !cam || !film || !sd || !out_pixels) return fail(FTN_ERR_INVALID_ARGUMENT, "null argument");
    if (sd->kind == FTN_SAMPLER_TILE_SERIAL || (opt && opt->pipeline == FTN_PIPELINE_MEGAKERNEL))          /* (the refusals come before any device work) */
        return ftn_render_gbuffer_device(cs, cam, film, sd, tr, opt, out_pixels, nullptr, st);
    if (int no = need_device()) return no;
    if (int rc = bind_scene_device(cs, opt)) return rc;
    return continue_on_device(out_pixels, crop_pixels(film), [&](void* d) { return ftn_render_gbuffer_device(cs, cam, film, sd, tr, opt, d, nullptr, st); });
}

int ftn_gbuffer_resolve(const ftn_gbuffer_pixel* in, size_t n, float* out12) {
    if (n && (!in || !out12)) return fail(FTN_ERR_INVALID_ARGUMENT, "null argument");
    for (size_t i = 0; i < n; i++) gbuffer_resolve_pixel(in[i].albedo, out12 + 12 * i);
    return FTN_OK;
}

int ftn_gbuffer_resolve_device(const void* in, size_t n, void* out12, void* stream) {
    if (n && (!in || !out12)) return fail(FTN_ERR_INVALID_ARGUMENT, "null argument");
    if (ftn_device_count() <= 0) return fail(FTN_ERR_NO_DEVICE, "no HIP device");          /* (not need_device(): this entry's refusal has words of its own) */
    return launched(launch_gbuffer_resolve((const float*)in, n, (float*)out12, (hipStream_t)stream), "G-buffer resolve");
}

}  /* extern "C" */
