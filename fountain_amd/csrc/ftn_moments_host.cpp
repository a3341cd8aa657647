/*
 * ftn_moments_host.cpp -- C entry points of include/fountain_hip_moments.h.
 *
 * They are part of the host library's translation unit: this file includes ftn_denoise_host.cpp (which includes ftn_gbuffer_host.cpp and
 * ftn_host.cpp) and the Makefile compiles it in its place, so that the entry points share ftn_host.cpp's scene internals (device arrays,
 * tile-list cache, film accumulators, WavefrontState) and its tile and device rules without exporting them.
 *
 * The moments' three accumulators belong to the scene handle but are not members of ftn_scene, whose definition stays as it is: they live
 * in a table keyed by the handle, allocated on the handle's first moments call (ftn_render never pays for them) and released by
 * ftn_scene_destroy.  For that, ftn_host.cpp's ftn_scene_destroy is compiled under another name, with hidden visibility, and the exported
 * ftn_scene_destroy below releases the table's entry before it calls that.
 */
#define ftn_scene_destroy __attribute__((visibility("hidden"))) ftn_scene_destroy_core
#include "ftn_denoise_host.cpp"
#undef ftn_scene_destroy
#include "../../include/fountain_hip_moments.h"
#include "ftn_moments.h"
#include <mutex>
#include <unordered_map>

namespace {
struct SceneMoments {
    DevBuf<float4> own, in_tile, other_tile; size_t pixels = 0;
    bool spill_dirty = true;           /* in_tile / other_tile may hold something other than zeros (the rule of ftn_scene::spill_acc_dirty) */
    void release() { own.release(); in_tile.release(); other_tile.release(); pixels = 0; spill_dirty = true; }
};
std::mutex g_moments_mutex;                                        /* guards the table, not its entries: a handle is used by one call at a time */
std::unordered_map<const ftn_scene*, SceneMoments> g_moments;      /* (references to entries survive rehashing) */

SceneMoments& scene_moments(const ftn_scene* s) { std::lock_guard<std::mutex> lock(g_moments_mutex); return g_moments[s]; }

/* every refusal of the moments pass: host-side checks only, before any device work */
int moments_refusals(const ftn_scene* s, const ftn_sampler_desc* sd, const ftn_integrator_desc* id, const ftn_render_options* opt) {
    if (sd->kind == FTN_SAMPLER_TILE_SERIAL)
        return fail(FTN_ERR_UNSUPPORTED, "the moments pass needs FTN_SAMPLER_INDEXED: it runs on the wavefront pipeline's sample-indexed passes");
    if (sd->kind != FTN_SAMPLER_INDEXED) return fail(FTN_ERR_INVALID_ARGUMENT, "unknown sampler kind");
    if ((uint64_t)sd->first_sample > (uint64_t)sd->samples_per_pixel || (uint64_t)sd->first_sample + (uint64_t)sd->sample_count > (uint64_t)sd->samples_per_pixel)
        return fail(FTN_ERR_INVALID_ARGUMENT, "sample range outside [0, samples_per_pixel]");
    if (id->kind != FTN_INTEGRATOR_PATH && id->kind != FTN_INTEGRATOR_DIRECT_LIGHTING && id->kind != FTN_INTEGRATOR_WHITTED) return fail(FTN_ERR_INVALID_ARGUMENT, "unknown integrator kind");
    if (id->max_depth > 65535u) return fail(FTN_ERR_INVALID_ARGUMENT, "max_depth is a u16 in the reference (integrator/path.rs:14)");
    const uint32_t pipeline = opt ? opt->pipeline : FTN_PIPELINE_AUTO;
    if (pipeline == FTN_PIPELINE_MEGAKERNEL) return fail(FTN_ERR_UNSUPPORTED, "the moments pass runs on the wavefront pipeline (FTN_PIPELINE_AUTO or FTN_PIPELINE_WAVEFRONT)");
    if (pipeline != FTN_PIPELINE_AUTO && pipeline != FTN_PIPELINE_WAVEFRONT) return fail(FTN_ERR_INVALID_ARGUMENT, "unknown pipeline");
    if (id->kind == FTN_INTEGRATOR_WHITTED && s->d.n_lights > 32u)
        return fail(FTN_ERR_UNSUPPORTED, "the wavefront pipeline renders WhittedIntegrator with up to 32 lights (one bit per light in a path's pending-light word)");
    return FTN_OK;
}
}  // namespace

extern "C" {

static_assert(sizeof(ftn_moment_pixel) == 16, "ABI");
int ftn_moments_abi_version(void) { return FTN_MOMENTS_ABI_VERSION; }

void ftn_scene_destroy(ftn_scene* s) {
    {
        std::lock_guard<std::mutex> lock(g_moments_mutex);
        auto it = g_moments.find(s);
        if (it != g_moments.end()) {
            it->second.release();           /* (as the scene's own buffers are released: whatever device is current) */
            g_moments.erase(it);
        }
    }
    ftn_scene_destroy_core(s);
}

int ftn_render_moments_device(const ftn_scene* cs, const ftn_camera_desc* cam, const ftn_film_desc* film, const ftn_sampler_desc* sd, const ftn_integrator_desc* id,
                              const ftn_tile_range* tr, const ftn_render_options* opt, void* device_pixels, void* device_moments, void* stream_v, ftn_stats* st) {
    if (!cs || !cam || !film || !sd || !id || !device_pixels || !device_moments) return fail(FTN_ERR_INVALID_ARGUMENT, "null argument");
    int rc = moments_refusals(cs, sd, id, opt); if (rc) return rc;
    if (ftn_device_count() <= 0) return fail(FTN_ERR_NO_DEVICE, "no HIP device available: the fountain HIP path needs an AMD GPU (there is no CPU fallback)");
    ftn_scene* s = const_cast<ftn_scene*>(cs);
    if (opt && opt->device >= 0 && s->device >= 0 && opt->device != s->device) return fail(FTN_ERR_INVALID_ARGUMENT, "ftn_render_options.device differs from the device the scene was created on");
    if ((rc = set_device(opt && opt->device >= 0 ? opt->device : s->device))) return rc;
    hipStream_t stream = (hipStream_t)stream_v;
    const bool count = opt && opt->count_traffic, count_production = opt && opt->count_traffic == 2;

    /* from here to the events, ftn_render_device's setup: tile selection through the same cache, parameters, accumulators, statistics */
    const uint32_t stride = tr && tr->stride ? tr->stride : 1, first = tr ? tr->first : 0, cnt = tr ? tr->count : 0;
    int32_t key[10] = {film->crop[0], film->crop[1], film->crop[2], film->crop[3], (int32_t)ftn_det::f2u(film->filter_radius[0]), (int32_t)ftn_det::f2u(film->filter_radius[1]),
                       (int32_t)first, (int32_t)stride, (int32_t)cnt, 1};
    const bool tiles_cached = memcmp(key, s->tile_key, sizeof(key)) == 0;
    if (!tiles_cached) {
        memset(s->tile_key, 0, sizeof(s->tile_key));
        std::vector<DTile> all; list_tiles(film, &all);
        s->sel.clear();
        for (size_t i = first, k = 0; i < all.size() && (cnt == 0 || k < cnt); i += stride, k++) s->sel.push_back(all[i]);
        uint32_t off = 0; for (DTile& t : s->sel) { t.valid_off = off; t._pad = 0; off += (uint32_t)((t.x1 - t.x0) * (t.y1 - t.y0)); }
    }
    std::vector<DTile>& sel = s->sel;

    RenderParams P; memset(&P, 0, sizeof(P));
    P.S = s->d;
    memcpy(P.C.c2w, cam->camera_to_world.m, 64); memcpy(P.C.r2c, cam->raster_to_camera.m, 64);
    P.C.shutter_open = cam->shutter_open; P.C.shutter_close = cam->shutter_close; P.C.lens_radius = cam->lens_radius; P.C.focal_dist = cam->focal_dist;
    for (int k = 0; k < 3; k++) { P.C.dx_camera[k] = cam->dx_camera[k]; P.C.dy_camera[k] = cam->dy_camera[k]; }
    for (int i = 0; i < 4; i++) P.crop[i] = film->crop[i];
    P.radius[0] = film->filter_radius[0]; P.radius[1] = film->filter_radius[1]; P.inv_radius[0] = 1.0f / P.radius[0]; P.inv_radius[1] = 1.0f / P.radius[1];
    P.sampler_kind = sd->kind; P.spp = sd->samples_per_pixel; P.seed = sd->seed;
    P.first_sample = sd->first_sample;
    P.last_sample = sd->first_sample + (sd->sample_count ? sd->sample_count : (sd->samples_per_pixel - sd->first_sample));
    P.integrator_kind = id->kind; P.max_depth = id->max_depth; P.rr_threshold = id->rr_threshold;
    P.stack_entries = s->stack_entries;

    const size_t npix = (size_t)std::max(0, film->crop[2] - film->crop[0]) * (size_t)std::max(0, film->crop[3] - film->crop[1]);
    if (npix > s->acc_pixels) {
        s->accA.release(); s->accB.release(); s->accC.release(); s->acc_pixels = 0;
        HIP_TRY(hipMalloc((void**)&s->accA.p, npix * sizeof(float4))); HIP_TRY(hipMalloc((void**)&s->accB.p, npix * sizeof(float4))); HIP_TRY(hipMalloc((void**)&s->accC.p, npix * sizeof(float4)));
        s->acc_pixels = npix; s->spill_acc_dirty = true;
    }
    /* the moments' accumulators, grown like the beauty's and cleared under the same rule */
    SceneMoments& mo = scene_moments(s);
    if (npix > mo.pixels) {
        mo.release();
        HIP_TRY(hipMalloc((void**)&mo.own.p, npix * sizeof(float4))); HIP_TRY(hipMalloc((void**)&mo.in_tile.p, npix * sizeof(float4))); HIP_TRY(hipMalloc((void**)&mo.other_tile.p, npix * sizeof(float4)));
        mo.pixels = npix; mo.spill_dirty = true;
    }
    if (sel.size() > s->tiles.n) { s->tiles.release(); HIP_TRY(hipMalloc((void**)&s->tiles.p, sel.size() * sizeof(DTile))); s->tiles.n = sel.size(); }
    HIP_TRY(hipMemsetAsync(s->accA.p, 0, npix * sizeof(float4), stream));
    if (s->spill_acc_dirty) { HIP_TRY(hipMemsetAsync(s->accB.p, 0, npix * sizeof(float4), stream)); HIP_TRY(hipMemsetAsync(s->accC.p, 0, npix * sizeof(float4), stream)); }
    s->spill_acc_dirty = true;         /* until this call has finished and reported otherwise */
    HIP_TRY(hipMemsetAsync(mo.own.p, 0, npix * sizeof(float4), stream));
    if (mo.spill_dirty) { HIP_TRY(hipMemsetAsync(mo.in_tile.p, 0, npix * sizeof(float4), stream)); HIP_TRY(hipMemsetAsync(mo.other_tile.p, 0, npix * sizeof(float4), stream)); }
    mo.spill_dirty = true;
    HIP_TRY(hipMemsetAsync(s->stats.p, 0, sizeof(DevStats), stream));
    if (!tiles_cached) {
        if (!sel.empty()) HIP_TRY(hipMemcpyAsync(s->tiles.p, sel.data(), sel.size() * sizeof(DTile), hipMemcpyHostToDevice, stream));
        memcpy(s->tile_key, key, sizeof(key));
    }
    P.tiles = s->tiles.p; P.n_tiles = (uint32_t)sel.size();
    P.accA = s->accA.p; P.accB = s->accB.p; P.accC = s->accC.p; P.stats = s->stats.p;
    const MomentAcc M{mo.own.p, mo.in_tile.p, mo.other_tile.p};

    struct EventPair {
        hipEvent_t a = nullptr, b = nullptr;
        ~EventPair() { if (a) (void)hipEventDestroy(a); if (b) (void)hipEventDestroy(b); }
    } ev;
    HIP_TRY(hipEventCreate(&ev.a)); HIP_TRY(hipEventCreate(&ev.b));
    HIP_TRY(hipEventRecord(ev.a, stream));
    WavefrontTimes wt; memset(&wt, 0, sizeof(wt));
    if ((rc = wavefront_moments(&s->wf, P, sel, count, count_production, M, stream, &wt))) return fail(rc, wavefront_error());
    launch_film_resolve(P, (ftn_pixel*)device_pixels, stream);
    launch_moments_merge(P, M, (float4*)device_moments, stream);
    HIP_TRY(hipEventRecord(ev.b, stream));
    HIP_TRY(hipEventSynchronize(ev.b));
    HIP_TRY(hipGetLastError());
    float ms = 0.0f; (void)hipEventElapsedTime(&ms, ev.a, ev.b);
    DevStats ds; HIP_TRY(hipMemcpy(&ds, s->stats.p, sizeof(ds), hipMemcpyDeviceToHost));
    s->spill_acc_dirty = ds.bc_writes != 0;
    mo.spill_dirty = ds.bc_writes != 0;         /* the moments' footprints are the beauty's: they spilled exactly where it did */
    ds.rays_closest += wt.mis_any_rays; ds.rays_any -= wt.mis_any_rays;
    stats_out(ds, st, ms);
    if (st) {
        st->trace_ms = wt.trace_ms; st->trace_launches = wt.trace_launches; st->mis_rays_any_hit = wt.mis_any_rays;
        st->any_ms = wt.any_ms; st->any_launches = wt.any_launches; st->shade_ms = wt.shade_ms; st->shade_launches = wt.shade_launches; st->sort_ms = wt.sort_ms;
    }
    if (ds.error == FTN_ERR_NAN_RADIANCE) return fail(FTN_ERR_NAN_RADIANCE, "NaN radiance value (integrator/mod.rs:285-287)");
    if (ds.error) return fail(ds.error, "unsupported material / integrator combination (e.g. specular glass: material/glass.rs:66)");
    return FTN_OK;
}

int ftn_render_moments(const ftn_scene* cs, const ftn_camera_desc* cam, const ftn_film_desc* film, const ftn_sampler_desc* sd, const ftn_integrator_desc* id,
                       const ftn_tile_range* tr, const ftn_render_options* opt, ftn_pixel* out_pixels, ftn_moment_pixel* out_moments, ftn_stats* st) {
    if (!cs || !cam || !film || !sd || !id || !out_pixels || !out_moments) return fail(FTN_ERR_INVALID_ARGUMENT, "null argument");
    int rc = moments_refusals(cs, sd, id, opt); if (rc) return rc;
    if (ftn_device_count() <= 0) return fail(FTN_ERR_NO_DEVICE, "no HIP device available: the fountain HIP path needs an AMD GPU (there is no CPU fallback)");
    if (opt && opt->device >= 0 && cs->device >= 0 && opt->device != cs->device) return fail(FTN_ERR_INVALID_ARGUMENT, "ftn_render_options.device differs from the device the scene was created on");
    if ((rc = set_device(opt && opt->device >= 0 ? opt->device : cs->device))) return rc;
    const size_t npix = (size_t)std::max(0, film->crop[2] - film->crop[0]) * (size_t)std::max(0, film->crop[3] - film->crop[1]);
    /* as ftn_render: the call's sums from zero device buffers, added once into the caller's */
    DevBuf<ftn_pixel> dev; DevBuf<ftn_moment_pixel> dev_m;
    if ((rc = dev.alloc_zero(npix)) || (rc = dev_m.alloc_zero(npix))) { dev.release(); dev_m.release(); return rc; }
    rc = ftn_render_moments_device(cs, cam, film, sd, id, tr, opt, dev.p, dev_m.p, nullptr, st);
    if ((rc == FTN_OK || rc == FTN_ERR_NAN_RADIANCE) && npix) {
        std::vector<ftn_pixel> h(npix); std::vector<ftn_moment_pixel> hm(npix);
        if (hipMemcpy(h.data(), dev.p, npix * sizeof(ftn_pixel), hipMemcpyDeviceToHost) != hipSuccess ||
            hipMemcpy(hm.data(), dev_m.p, npix * sizeof(ftn_moment_pixel), hipMemcpyDeviceToHost) != hipSuccess) {
            dev.release(); dev_m.release(); return fail(FTN_ERR_NO_DEVICE, "copy back failed");
        }
        for (size_t i = 0; i < npix; i++) {
            out_pixels[i].xyz[0] += h[i].xyz[0]; out_pixels[i].xyz[1] += h[i].xyz[1]; out_pixels[i].xyz[2] += h[i].xyz[2];
            out_pixels[i].filter_weight_sum += h[i].filter_weight_sum;
            for (int k = 0; k < 3; k++) out_moments[i].sq[k] += hm[i].sq[k];
            out_moments[i].sq_y += hm[i].sq_y;
        }
    }
    dev.release(); dev_m.release();
    return rc;
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
