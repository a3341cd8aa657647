/*
 * ftn_lightpass_host.cpp -- C entry points of include/fountain_hip_lightpass.h.
 *
 * The pass takes the steps of every first-hit pass (first_hit_render, ftn_host_internal.h), as the ambient-occlusion pass does; the
 * compose entries are an image-space stage on the stages' scaffold (ftn_stage_host.h); the resolve and compose twins and
 * ftn_lightpass_terms run the arithmetic of ftn_lightpass.h on the host and need no device.
 */
#include "ftn_stage_host.h"
#include "../../include/fountain_hip_lightpass.h"
#include "ftn_lightpass.h"

#include <cstring>

using namespace ftn;

namespace {

/* refusals (2) and (3) of the header.  The scene is only looked at for its host-side light list */
int light_set_check(const ftn_scene* s, const uint32_t* lights, uint32_t n_lights) {
    if ((lights == nullptr) != (n_lights == 0u))
        return fail(FTN_ERR_INVALID_ARGUMENT, "the light set is either lights == NULL with n_lights == 0 (all lights) or a list with its length");
    const size_t have = s->host.light_kind.size();
    for (uint32_t i = 0; i < n_lights; i++) {
        if (i > 0 && lights[i] <= lights[i - 1]) return fail(FTN_ERR_INVALID_ARGUMENT, "the light indices must be strictly increasing");
        if (lights[i] >= have) return fail(FTN_ERR_INVALID_ARGUMENT, "light index out of range: the scene has " + std::to_string(have) + " lights");
    }
    return FTN_OK;
}

/* the refusals of both render entries, in the header's order */
int render_refusals(const ftn_scene* cs, const ftn_camera_desc* cam, const ftn_film_desc* film, const ftn_sampler_desc* sd, const ftn_render_options* opt,
                    const uint32_t* lights, uint32_t n_lights, const void* pixels) {
    if (!cs || !cam || !film || !sd || !pixels) return fail(FTN_ERR_INVALID_ARGUMENT, "null argument");
    if (int no = light_set_check(cs, lights, n_lights)) return no;
    if (int no = indexed_sampler_check(sd, "light")) return no;
    if (int no = wavefront_pipeline_check(opt, "light")) return no;
    return need_device();
}

int compose_check(const void* gb12, const void* res8, uint32_t groups, const float* gains3, size_t n, const void* rgb_out, bool device) {
    if (!gains3 || (n && (!gb12 || !res8 || !rgb_out))) return fail(FTN_ERR_INVALID_ARGUMENT, "null argument");
    if (groups < 1u || groups > FTN_LIGHTPASS_MAX_GROUPS) return fail(FTN_ERR_INVALID_ARGUMENT, "the relighting step takes 1 to 16 light groups");
    if ((uint64_t)n * (uint64_t)groups >= ((uint64_t)1 << 31)) return fail(FTN_ERR_INVALID_ARGUMENT, "n * groups must be below 2^31 pixels");
    for (uint32_t k = 0; k < 3u * groups; k++)
        if (!is_finite(gains3[k])) return fail(FTN_ERR_INVALID_ARGUMENT, "the gains must be finite");
    const Range r_gb = {gb12, 12 * n * sizeof(float), 16}, r_res = {res8, 8 * n * (size_t)groups * sizeof(float), 16}, r_out = {rgb_out, 3 * n * sizeof(float), 16};
    if (int rc = overlap_check({r_out}, {r_gb, r_res}, "rgb_out overlaps an input")) return rc;
    if (device)
        if (int rc = align_check({r_gb, r_res, r_out}, "misaligned buffer: gb12, res8 and rgb_out need 16 bytes")) return rc;
    return FTN_OK;
}

LpGains gains_of(const float* gains3, uint32_t groups) {
    LpGains g; memset(&g, 0, sizeof(g));
    memcpy(g.v, gains3, 3 * (size_t)groups * sizeof(float));
    return g;
}

}  // namespace

extern "C" {

static_assert(sizeof(ftn_lightpass_pixel) == 32, "ABI");
static_assert(FTN_LIGHTPASS_MAX_GROUPS == LP_MAX_GROUPS, "ABI");
int ftn_lightpass_abi_version(void) { return FTN_LIGHTPASS_ABI_VERSION; }

int ftn_render_lightpass_device(const ftn_scene* cs, const ftn_camera_desc* cam, const ftn_film_desc* film, const ftn_sampler_desc* sd, const ftn_tile_range* tr,
                                const ftn_render_options* opt, const uint32_t* lights, uint32_t n_lights, void* device_pixels, void* stream_v, ftn_stats* st) {
    if (int no = render_refusals(cs, cam, film, sd, opt, lights, n_lights, device_pixels)) return no;
    ftn_scene* s = const_cast<ftn_scene*>(cs);
    if (int rc = bind_scene_device(s, opt)) return rc;
    hipStream_t stream = (hipStream_t)stream_v;
    if (int no = sample_range_check(sd)) return no;
    /* the group's list, uploaded for this call and freed on every way out (first_hit_render has drained the stream when it returns) */
    DevBuf<uint32_t> d_lights;
    struct Release { DevBuf<uint32_t>& b; ~Release() { b.release(); } } keep{d_lights};
    if (int rc = d_lights.upload(lights, n_lights)) return rc;
    const uint32_t n = lights ? n_lights : s->d.n_lights;
    WavefrontTimes wt{};
    const int rc = first_hit_render(s, cam, film, sd, tr, stream, st, [&](const RenderParams& P, double* trace_ms) {
        return wavefront_lightpass(&s->wf, P, s->sel, d_lights.p, n, count_mode(opt), (float*)device_pixels, stream, trace_ms, &wt);
    });
    return rc ? rc : any_hit_stats_out(s, wt, st);
}

int ftn_render_lightpass(const ftn_scene* cs, const ftn_camera_desc* cam, const ftn_film_desc* film, const ftn_sampler_desc* sd, const ftn_tile_range* tr,
                         const ftn_render_options* opt, const uint32_t* lights, uint32_t n_lights, ftn_lightpass_pixel* out_pixels, ftn_stats* st) {
    if (int no = render_refusals(cs, cam, film, sd, opt, lights, n_lights, out_pixels)) return no;          /* (before any device work) */
    if (int rc = bind_scene_device(cs, opt)) return rc;
    return continue_on_device(out_pixels, crop_pixels(film), [&](void* d) { return ftn_render_lightpass_device(cs, cam, film, sd, tr, opt, lights, n_lights, d, nullptr, st); });
}

int ftn_lightpass_resolve(const ftn_lightpass_pixel* in, size_t n, float* out8) {
    if (n && (!in || !out8)) return fail(FTN_ERR_INVALID_ARGUMENT, "null argument");
    for (size_t i = 0; i < n; i++) lp_resolve_pixel(in[i].lit, out8 + 8 * i);
    return FTN_OK;
}

int ftn_lightpass_resolve_device(const void* in, size_t n, void* out8, void* stream) {
    if (n && (!in || !out8)) return fail(FTN_ERR_INVALID_ARGUMENT, "null argument");
    if (int no = need_device()) return no;
    return launched(launch_lp_resolve((const float*)in, n, (float*)out8, (hipStream_t)stream), "light-pass resolve");
}

int ftn_lightpass_compose(const float* gb12, const float* res8, uint32_t groups, const float* gains3, size_t n, float* rgb_out) {
    if (int no = compose_check(gb12, res8, groups, gains3, n, rgb_out, false)) return no;
    const LpGains g = gains_of(gains3, groups);
    parallel_for(n, [&](size_t i0, size_t i1) {
        for (size_t i = i0; i < i1; i++) lp_compose_pixel(gb12 + 12 * i, res8, i, n, groups, g, rgb_out + 3 * i);
    });
    return FTN_OK;
}

int ftn_lightpass_compose_device(const void* gb12, const void* res8, uint32_t groups, const float* gains3, size_t n, void* rgb_out, void* stream) {
    if (int no = compose_check(gb12, res8, groups, gains3, n, rgb_out, true)) return no;
    if (int no = need_device()) return no;
    return launched(launch_lp_compose((const float*)gb12, (const float*)res8, groups, gains_of(gains3, groups), n, (float*)rgb_out, (hipStream_t)stream), "light-pass compose");
}

int ftn_lightpass_terms(const float* hit24, const float* light24, size_t n, uint32_t group_size, float* e3, float* rays8) {
    if (n && (!hit24 || !light24 || !e3 || !rays8)) return fail(FTN_ERR_INVALID_ARGUMENT, "null argument");
    for (size_t i = 0; i < n; i++) {
        const float* h = hit24 + 24 * i;
        const float* l = light24 + 24 * i;
        Rgb e;
        float* o = rays8 + 8 * i;
        for (int k = 0; k < 8; k++) o[k] = 0.0f;
        if (lp_term(V3(h[6], h[7], h[8]), V3(h[20], h[21], h[22]), V3(h[11], h[12], h[13]), Rgb(l[0], l[1], l[2]), V3(l[3], l[4], l[5]), l[6], group_size, &e)) {
            const LpRay r = lp_shadow_ray(V3(h[0], h[1], h[2]), V3(h[3], h[4], h[5]), V3(h[6], h[7], h[8]), V3(l[7], l[8], l[9]), V3(l[10], l[11], l[12]), V3(l[13], l[14], l[15]));
            o[0] = r.o.x; o[1] = r.o.y; o[2] = r.o.z; o[3] = r.d.x; o[4] = r.d.y; o[5] = r.d.z; o[6] = r.t_max;
        }
        e3[3 * i] = e.r; e3[3 * i + 1] = e.g; e3[3 * i + 2] = e.b;
    }
    return FTN_OK;
}

}  /* extern "C" */
