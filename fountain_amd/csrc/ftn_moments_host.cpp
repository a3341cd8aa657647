/*
 * ftn_moments_host.cpp -- C entry points of include/fountain_hip_moments.h.
 *
 * The pass takes the steps of every render call (ftn_host_internal.h), with the scene's moments accumulators beside the film's: they are
 * grown on the first moments or adaptive call of a scene (ftn_render never allocates or clears them) and cleared under the same rule.
 */
#include "ftn_stage_host.h"
#include "../../include/fountain_hip_moments.h"
#include "ftn_moments.h"

#include <cstring>

using namespace ftn;

/* every refusal of the moments pass: host-side checks only, before any device work */
int moments_refusals(const ftn_scene* s, const ftn_sampler_desc* sd, const ftn_integrator_desc* id, const ftn_render_options* opt) {
    if (int no = indexed_sampler_check(sd, "moments", "it runs on the wavefront pipeline's sample-indexed passes")) return no;
    if (int no = sample_range_check(sd)) return no;
    if (id->kind != FTN_INTEGRATOR_PATH && id->kind != FTN_INTEGRATOR_DIRECT_LIGHTING && id->kind != FTN_INTEGRATOR_WHITTED) return fail(FTN_ERR_INVALID_ARGUMENT, "unknown integrator kind");
    if (id->max_depth > 65535u) return fail(FTN_ERR_INVALID_ARGUMENT, "max_depth is a u16 in the reference (integrator/path.rs:14)");
    if (int no = wavefront_pipeline_check(opt, "moments")) return no;
    if (id->kind == FTN_INTEGRATOR_WHITTED && s->d.n_lights > 32u)
        return fail(FTN_ERR_UNSUPPORTED, "the wavefront pipeline renders WhittedIntegrator with up to 32 lights (one bit per light in a path's pending-light word)");
    return FTN_OK;
}

extern "C" {

static_assert(sizeof(ftn_moment_pixel) == 16, "ABI");
int ftn_moments_abi_version(void) { return FTN_MOMENTS_ABI_VERSION; }

int ftn_render_moments_device(const ftn_scene* cs, const ftn_camera_desc* cam, const ftn_film_desc* film, const ftn_sampler_desc* sd, const ftn_integrator_desc* id,
                              const ftn_tile_range* tr, const ftn_render_options* opt, void* device_pixels, void* device_moments, void* stream_v, ftn_stats* st) {
    if (!cs || !cam || !film || !sd || !id || !device_pixels || !device_moments) return fail(FTN_ERR_INVALID_ARGUMENT, "null argument");
    int rc = moments_refusals(cs, sd, id, opt); if (rc) return rc;
    if (int no = need_device()) return no;
    ftn_scene* s = const_cast<ftn_scene*>(cs);
    if ((rc = bind_scene_device(s, opt))) return rc;
    hipStream_t stream = (hipStream_t)stream_v;
    const bool count = opt && opt->count_traffic, count_production = opt && opt->count_traffic == 2;

    RenderParams P = render_params(s, cam, film, sd, id);
    if ((rc = scene_tiles(s, film, tr, stream, &P)) || (rc = prepare_film(s, true, stream, &P))) return rc;
    const MomentAcc M{s->moments.own.p, s->moments.in_tile.p, s->moments.other_tile.p};
    EventPair ev; if ((rc = ev.start(stream))) return rc;
    WavefrontTimes wt; memset(&wt, 0, sizeof(wt));
    if ((rc = wavefront_moments(&s->wf, P, s->sel, count, count_production, M, stream, &wt))) return fail(rc, wavefront_error());
    launch_film_resolve(P, (ftn_pixel*)device_pixels, stream);
    launch_moments_merge(P, M, (float4*)device_moments, stream);
    float ms; if ((rc = ev.stop(stream, &ms))) return rc;
    DevStats ds; if ((rc = read_stats(s, true, &ds))) return rc;
    render_stats_out(ds, wt, ms, st);
    return render_error(ds.error);
}

int ftn_render_moments(const ftn_scene* cs, const ftn_camera_desc* cam, const ftn_film_desc* film, const ftn_sampler_desc* sd, const ftn_integrator_desc* id,
                       const ftn_tile_range* tr, const ftn_render_options* opt, ftn_pixel* out_pixels, ftn_moment_pixel* out_moments, ftn_stats* st) {
    if (!cs || !cam || !film || !sd || !id || !out_pixels || !out_moments) return fail(FTN_ERR_INVALID_ARGUMENT, "null argument");
    int rc = moments_refusals(cs, sd, id, opt); if (rc) return rc;
    if (int no = need_device()) return no;
    if ((rc = bind_scene_device(cs, opt))) return rc;
    const size_t npix = (size_t)std::max(0, film->crop[2] - film->crop[0]) * (size_t)std::max(0, film->crop[3] - film->crop[1]);
    /* as ftn_render: the call's sums from zero device buffers, added once into the caller's */
    return render_to_host(npix, {{out_pixels, sizeof(ftn_pixel), true}, {out_moments, sizeof(ftn_moment_pixel), true}},
                          [&](void* const* d) { return ftn_render_moments_device(cs, cam, film, sd, id, tr, opt, d[0], d[1], nullptr, st); });
}

int ftn_moments_resolve(const ftn_pixel* beauty, const ftn_moment_pixel* m, size_t n, float* out4) {
    if (n && (!beauty || !m || !out4)) return fail(FTN_ERR_INVALID_ARGUMENT, "null argument");
    for (size_t i = 0; i < n; i++) moments_resolve_pixel(reinterpret_cast<const float*>(beauty + i), m[i].sq, out4 + 4 * i);
    return FTN_OK;
}

int ftn_moments_resolve_device(const void* beauty, const void* m, size_t n, void* out4, void* stream) {
    if (n && (!beauty || !m || !out4)) return fail(FTN_ERR_INVALID_ARGUMENT, "null argument");
    if (ftn_device_count() <= 0) return fail(FTN_ERR_NO_DEVICE, "no HIP device");
    launch_moments_resolve((const float*)beauty, (const float*)m, n, (float*)out4, (hipStream_t)stream);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(FTN_ERR_INTERNAL, hipGetErrorString(e));
    return FTN_OK;
}

}  /* extern "C" */
