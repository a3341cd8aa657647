/*
 * ftn_ao_host.cpp -- C entry points of include/fountain_hip_ao.h.
 *
 * The pass takes the steps of every first-hit pass (first_hit_render, ftn_host_internal.h), as the G-buffer does; the resolve entry and
 * ftn_ao_rays run the arithmetic of ftn_ao.h on the host and need no device.
 */
#include "ftn_stage_host.h"
#include "../../include/fountain_hip_ao.h"
#include "ftn_ao.h"

#include <cstring>

using namespace ftn;

/* the options' refusals: rays 1 .. 64, a radius that is a number above zero (+inf included) */
static int ao_rays_check(uint32_t rays) {
    return (rays < 1u || rays > 64u) ? fail(FTN_ERR_INVALID_ARGUMENT, "ambient occlusion takes 1 to 64 rays per surface") : FTN_OK;
}
static int ao_options_check(const ftn_ao_options* ao) {
    if (int no = ao_rays_check(ao->rays)) return no;
    if (!(ao->radius > 0.0f)) return fail(FTN_ERR_INVALID_ARGUMENT, "the ambient-occlusion radius must be above zero (+inf: unbounded)");
    return FTN_OK;
}

extern "C" {

static_assert(sizeof(ftn_ao_pixel) == 32 && sizeof(ftn_ao_options) == 16, "ABI");
int ftn_ao_abi_version(void) { return FTN_AO_ABI_VERSION; }

int ftn_render_ao_device(const ftn_scene* cs, const ftn_camera_desc* cam, const ftn_film_desc* film, const ftn_sampler_desc* sd,
                         const ftn_tile_range* tr, const ftn_render_options* opt, const ftn_ao_options* ao, void* device_pixels, void* stream_v, ftn_stats* st) {
    if (!cs || !cam || !film || !sd || !ao || !device_pixels) return fail(FTN_ERR_INVALID_ARGUMENT, "null argument");
    if (int no = ao_options_check(ao)) return no;
    if (int no = indexed_sampler_check(sd, "ambient-occlusion")) return no;
    if (int no = wavefront_pipeline_check(opt, "ambient-occlusion")) return no;
    if (int no = need_device()) return no;
    ftn_scene* s = const_cast<ftn_scene*>(cs);
    if (int rc = bind_scene_device(s, opt)) return rc;
    hipStream_t stream = (hipStream_t)stream_v;
    if (int no = sample_range_check(sd)) return no;
    WavefrontTimes wt{};
    const int rc = first_hit_render(s, cam, film, sd, tr, stream, st, [&](const RenderParams& P, double* trace_ms) {
        return wavefront_ao(&s->wf, P, s->sel, ao->rays, ao->radius, count_mode(opt), (float*)device_pixels, stream, trace_ms, &wt);
    });
    return rc ? rc : any_hit_stats_out(s, wt, st);
}

int ftn_render_ao(const ftn_scene* cs, const ftn_camera_desc* cam, const ftn_film_desc* film, const ftn_sampler_desc* sd,
                  const ftn_tile_range* tr, const ftn_render_options* opt, const ftn_ao_options* ao, ftn_ao_pixel* out_pixels, ftn_stats* st) {
    if (!cs || !cam || !film || !sd || !ao || !out_pixels) return fail(FTN_ERR_INVALID_ARGUMENT, "null argument");
    if (int no = ao_options_check(ao)) return no;
    if (int no = indexed_sampler_check(sd, "ambient-occlusion")) return no;          /* (the refusals come before any device work) */
    if (int no = wavefront_pipeline_check(opt, "ambient-occlusion")) return no;
    if (int no = need_device()) return no;
    if (int rc = bind_scene_device(cs, opt)) return rc;
    return continue_on_device(out_pixels, crop_pixels(film), [&](void* d) { return ftn_render_ao_device(cs, cam, film, sd, tr, opt, ao, d, nullptr, st); });
}

int ftn_ao_resolve(const ftn_ao_pixel* in, size_t n, uint32_t rays, float* out6) {
    if (n && (!in || !out6)) return fail(FTN_ERR_INVALID_ARGUMENT, "null argument");
    if (int no = ao_rays_check(rays)) return no;
    for (size_t i = 0; i < n; i++) ao_resolve_pixel(&in[i].open, rays, out6 + 6 * i);
    return FTN_OK;
}

int ftn_ao_resolve_device(const void* in, size_t n, uint32_t rays, void* out6, void* stream) {
    if (n && (!in || !out6)) return fail(FTN_ERR_INVALID_ARGUMENT, "null argument");
    if (int no = ao_rays_check(rays)) return no;
    if (int no = need_device()) return no;
    return launched(launch_ao_resolve((const float*)in, n, rays, (float*)out6, (hipStream_t)stream), "ambient-occlusion resolve");
}

int ftn_ao_rays(const float* hit24, const float* u2, size_t n, float radius, float* rays8) {
    if (n && (!hit24 || !u2 || !rays8)) return fail(FTN_ERR_INVALID_ARGUMENT, "null argument");
    for (size_t i = 0; i < n; i++) {
        const float* h = hit24 + 24 * i;
        const V3 nrm(h[6], h[7], h[8]);
        const V3 nf = ao_facing_normal(nrm, ao_flipped(nrm, V3(h[11], h[12], h[13])));
        const AoRay r = ao_ray(V3(h[0], h[1], h[2]), V3(h[3], h[4], h[5]), nrm, nf, V2(u2[2 * i], u2[2 * i + 1]));
        float* o = rays8 + 8 * i;
        o[0] = r.o.x; o[1] = r.o.y; o[2] = r.o.z; o[3] = r.d.x; o[4] = r.d.y; o[5] = r.d.z; o[6] = radius; o[7] = 0.0f;
    }
    return FTN_OK;
}

}  /* extern "C" */
