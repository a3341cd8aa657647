/*
 * ftn_host.cpp -- the render driver of libfountain_hip.so (the C ABI of include/fountain_hip.h): error reporting, device selection, the steps
 * of a render call (ftn_host_internal.h), batch intersection, and ftn_render / ftn_render_device (SamplerIntegrator::render_parallel,
 * src/integrator/mod.rs:218-227).  The rest of the ABI is in units of its own: transforms, spheres, cameras and films in
 * ftn_geometry_host.cpp, BVH construction in ftn_bvh_host.cpp, scene construction in ftn_scene_host.cpp, the test hooks in ftn_test_*.
 * There is no CPU fallback: every compute entry point needs a HIP device and fails with FTN_ERR_NO_DEVICE without one.
 */
#include "ftn_host_internal.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>

using namespace ftn;

/* the sizes of the ABI's structures, all in one place */
static_assert(sizeof(ftn_transform) == 128 && sizeof(ftn_pixel) == 16 && sizeof(ftn_bvh_node) == 32 && sizeof(ftn_prim) == 16, "ABI");
static_assert(sizeof(ftn_mesh) == 20 && sizeof(ftn_sphere) == 288 && sizeof(ftn_material) == 48 && sizeof(ftn_light) == 160, "ABI");
static_assert(sizeof(ftn_envmap) == 16 && sizeof(ftn_camera_desc) == 296 && sizeof(ftn_film_desc) == 32 && sizeof(ftn_sampler_desc) == 24, "ABI");
static_assert(sizeof(ftn_integrator_desc) == 16 && sizeof(ftn_tile_range) == 16 && sizeof(ftn_render_options) == 16 && sizeof(ftn_stats) == 152, "ABI");

static thread_local std::string g_err;
int fail(int code, const std::string& msg) { g_err = msg; return code; }

int set_device(int device) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n == 0) return fail(FTN_ERR_NO_DEVICE, kNoDevice);
    if (device >= 0) {
        hipError_t e = hipSetDevice(device);
        if (e != hipSuccess) { (void)hipGetLastError();      /* do not leave the error behind for the next call's hipGetLastError() */
                               return fail(FTN_ERR_NO_DEVICE, std::string("hipSetDevice(device): ") + hipGetErrorString(e)); }
    }
    return FTN_OK;
}

void stats_out(const DevStats& ds, ftn_stats* st, double ms) {
    if (!st) return;
    memset(st, 0, sizeof(*st));
    st->rays_closest = ds.rays_closest; st->rays_any = ds.rays_any; st->nodes_visited = ds.nodes_visited; st->prims_tested = ds.prims_tested;
    st->camera_samples = ds.camera_samples; st->spill_samples = ds.spill_samples; st->kernel_ms = ms;
    st->nodes_visited_any = ds.nodes_any; st->prims_tested_any = ds.prims_any;
    st->quad_records = ds.quad_records; st->quad_records_any = ds.quad_records_any;
}

/* ------------------------------------------------------------------ the steps of a render call (ftn_host_internal.h) */
int bind_scene_device(const ftn_scene* s, const ftn_render_options* opt) {
    if (opt && opt->device >= 0 && s->device >= 0 && opt->device != s->device) return fail(FTN_ERR_INVALID_ARGUMENT, "ftn_render_options.device differs from the device the scene was created on");
    return set_device(opt && opt->device >= 0 ? opt->device : s->device);
}

void select_tiles(const ftn_film_desc* film, const ftn_tile_range* tr, std::vector<DTile>* sel) {
    const uint32_t stride = tr && tr->stride ? tr->stride : 1, first = tr ? tr->first : 0, cnt = tr ? tr->count : 0;
    std::vector<DTile> all; list_tiles(film, &all);
    sel->clear();
    for (size_t i = first, k = 0; i < all.size() && (cnt == 0 || k < cnt); i += stride, k++) sel->push_back(all[i]);
    uint32_t off = 0; for (DTile& t : *sel) { t.valid_off = off; t._pad = 0; off += (uint32_t)((t.x1 - t.x0) * (t.y1 - t.y0)); }
}

int scene_tiles(ftn_scene* s, const ftn_film_desc* film, const ftn_tile_range* tr, hipStream_t stream, RenderParams* P) {
    /* the tile list only depends on the film and the tile range: keep it (and its device copy) between calls */
    const uint32_t stride = tr && tr->stride ? tr->stride : 1, first = tr ? tr->first : 0, cnt = tr ? tr->count : 0;
    const int32_t key[10] = {film->crop[0], film->crop[1], film->crop[2], film->crop[3], (int32_t)ftn_det::f2u(film->filter_radius[0]), (int32_t)ftn_det::f2u(film->filter_radius[1]),
                             (int32_t)first, (int32_t)stride, (int32_t)cnt, 1};
    if (memcmp(key, s->tile_key, sizeof(key)) != 0) {
        memset(s->tile_key, 0, sizeof(s->tile_key));      /* the host list is about to change: no key is valid until list AND device copy are in place */
        select_tiles(film, tr, &s->sel);
        if (s->sel.size() > s->tiles.n) { s->tiles.release(); HIP_TRY(hipMalloc((void**)&s->tiles.p, s->sel.size() * sizeof(DTile))); s->tiles.n = s->sel.size(); }
        if (!s->sel.empty()) HIP_TRY(hipMemcpyAsync(s->tiles.p, s->sel.data(), s->sel.size() * sizeof(DTile), hipMemcpyHostToDevice, stream));
        memcpy(s->tile_key, key, sizeof(key));            /* (an empty selection is a valid cached state too) */
    }
    P->tiles = s->tiles.p; P->n_tiles = (uint32_t)s->sel.size();
    return FTN_OK;
}

RenderParams render_params(const ftn_scene* s, const ftn_camera_desc* cam, const ftn_film_desc* film, const ftn_sampler_desc* sd, const ftn_integrator_desc* id) {
    RenderParams P; memset(&P, 0, sizeof(P));
    P.S = s->d;
    memcpy(P.C.c2w, cam->camera_to_world.m, 64); memcpy(P.C.r2c, cam->raster_to_camera.m, 64);
    P.C.shutter_open = cam->shutter_open; P.C.shutter_close = cam->shutter_close; P.C.lens_radius = cam->lens_radius; P.C.focal_dist = cam->focal_dist;
    for (int k = 0; k < 3; k++) { P.C.dx_camera[k] = cam->dx_camera[k]; P.C.dy_camera[k] = cam->dy_camera[k]; }
    for (int i = 0; i < 4; i++) P.crop[i] = film->crop[i];
    P.radius[0] = film->filter_radius[0]; P.radius[1] = film->filter_radius[1]; P.inv_radius[0] = 1.0f / P.radius[0]; P.inv_radius[1] = 1.0f / P.radius[1];
    const bool indexed = sd->kind == FTN_SAMPLER_INDEXED;
    P.sampler_kind = sd->kind; P.spp = sd->samples_per_pixel; P.seed = sd->seed;
    P.first_sample = indexed ? sd->first_sample : 0;
    P.last_sample = indexed ? sd->first_sample + (sd->sample_count ? sd->sample_count : (sd->samples_per_pixel - sd->first_sample)) : sd->samples_per_pixel;
    P.integrator_kind = id->kind; P.max_depth = id->max_depth; P.rr_threshold = id->rr_threshold;
    P.stack_entries = s->stack_entries;
    return P;
}

int FilmAcc::prepare(size_t npix, hipStream_t stream) {
    if (npix > pixels) {
        release();                     /* (pixels = 0 until all three exist again) */
        HIP_TRY(hipMalloc((void**)&own.p, npix * sizeof(float4))); HIP_TRY(hipMalloc((void**)&in_tile.p, npix * sizeof(float4))); HIP_TRY(hipMalloc((void**)&other_tile.p, npix * sizeof(float4)));
        pixels = npix;
    }
    if (npix) {
        HIP_TRY(hipMemsetAsync(own.p, 0, npix * sizeof(float4), stream));
        if (spill_dirty) {             /* else: still all zero from the last call (DevStats::bc_writes said nothing was added) */
            HIP_TRY(hipMemsetAsync(in_tile.p, 0, npix * sizeof(float4), stream));
            HIP_TRY(hipMemsetAsync(other_tile.p, 0, npix * sizeof(float4), stream));
        }
    }
    spill_dirty = true;                /* until this call has finished and reported otherwise */
    return FTN_OK;
}

int prepare_film(ftn_scene* s, bool moments, hipStream_t stream, RenderParams* P) {
    const size_t npix = (size_t)std::max(0, P->crop[2] - P->crop[0]) * (size_t)std::max(0, P->crop[3] - P->crop[1]);
    int rc = s->acc.prepare(npix, stream); if (rc) return rc;
    if (moments && (rc = s->moments.prepare(npix, stream))) return rc;
    HIP_TRY(hipMemsetAsync(s->stats.p, 0, sizeof(DevStats), stream));
    P->accA = s->acc.own.p; P->accB = s->acc.in_tile.p; P->accC = s->acc.other_tile.p; P->stats = s->stats.p;
    return FTN_OK;
}

int EventPair::start(hipStream_t stream) {
    HIP_TRY(hipEventCreate(&a)); HIP_TRY(hipEventCreate(&b));
    HIP_TRY(hipEventRecord(a, stream));
    return FTN_OK;
}
int EventPair::stop(hipStream_t stream, float* ms) {
    HIP_TRY(hipEventRecord(b, stream));
    HIP_TRY(hipEventSynchronize(b));
    HIP_TRY(hipGetLastError());
    *ms = 0.0f; (void)hipEventElapsedTime(ms, a, b);
    return FTN_OK;
}

int read_stats(ftn_scene* s, bool moments, DevStats* ds) {
    HIP_TRY(hipMemcpy(ds, s->stats.p, sizeof(*ds), hipMemcpyDeviceToHost));
    s->acc.spill_dirty = ds->bc_writes != 0;
    if (moments) s->moments.spill_dirty = ds->bc_writes != 0;     /* the moments' footprints are the beauty's: they spilled exactly where it did */
    return FTN_OK;
}

void render_stats_out(DevStats ds, const WavefrontTimes& wt, float ms, ftn_stats* st) {
    ds.rays_closest += wt.mis_any_rays; ds.rays_any -= wt.mis_any_rays;       /* they are Scene::intersect calls in the reference's accounting */
    stats_out(ds, st, ms);
    if (st) {
        st->trace_ms = wt.trace_ms; st->trace_launches = wt.trace_launches; st->mis_rays_any_hit = wt.mis_any_rays;
        st->any_ms = wt.any_ms; st->any_launches = wt.any_launches; st->shade_ms = wt.shade_ms; st->shade_launches = wt.shade_launches; st->sort_ms = wt.sort_ms;
    }
}

int render_error(int error) {
    if (error == FTN_ERR_NAN_RADIANCE) return fail(FTN_ERR_NAN_RADIANCE, "NaN radiance value (integrator/mod.rs:285-287)");
    if (error) return fail(error, "unsupported material / integrator combination (e.g. specular glass: material/glass.rs:66)");
    return FTN_OK;
}

int first_hit_render(ftn_scene* s, const ftn_camera_desc* cam, const ftn_film_desc* film, const ftn_sampler_desc* sd, const ftn_tile_range* tr, hipStream_t stream, ftn_stats* st,
                     const std::function<int(const RenderParams& P, double* trace_ms)>& run) {
    ftn_integrator_desc first_hit; memset(&first_hit, 0, sizeof(first_hit)); first_hit.kind = FTN_INTEGRATOR_PATH;
    RenderParams P = render_params(s, cam, film, sd, &first_hit);
    int rc;
    if ((rc = scene_tiles(s, film, tr, stream, &P)) || (rc = prepare_film(s, false, stream, &P))) return rc;
    EventPair ev; if ((rc = ev.start(stream))) return rc;
    double trace_ms = 0.0;
    if ((rc = run(P, &trace_ms))) {
        (void)hipStreamSynchronize(stream);              /* what the caller uploaded for the call is freed on return */
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

extern "C" {

const char* ftn_last_error(void) { return g_err.c_str(); }
const char* ftn_version(void) { return "fountain_hip 0.3 (gfx950)"; }
int ftn_abi_version(void) { return FTN_ABI_VERSION; }
int ftn_device_count(void) { int n = 0; if (hipGetDeviceCount(&n) != hipSuccess) return 0; return n; }

/* ------------------------------------------------------------------ batch intersection */
static int trace_batch(const ftn_scene* cs, const float* rays, size_t n, int mode, float* t_hit, int32_t* prim, float* bary, uint8_t* occ, float* out24, ftn_stats* st) {
    ftn_scene* s = const_cast<ftn_scene*>(cs);
    int rc = set_device(s->device); if (rc) return rc;
    DevBuf<float> d_rays, d_t, d_b, d_o; DevBuf<int> d_p; DevBuf<unsigned char> d_occ;
    struct Release {                                         /* frees the call's device buffers on every way out */
        DevBuf<float>&a, &b, &c, &d; DevBuf<int>& e; DevBuf<unsigned char>& f;
        ~Release() { a.release(); b.release(); c.release(); d.release(); e.release(); f.release(); }
    } keep{d_rays, d_t, d_b, d_o, d_p, d_occ};
    if ((rc = d_rays.upload(rays, 8 * n))) return rc;
    if (mode == 0) { if ((rc = d_t.alloc_zero(n)) || (rc = d_p.alloc_zero(n)) || (rc = d_b.alloc_zero(3 * n))) return rc; }
    else if (mode == 1) { if ((rc = d_occ.alloc_zero(n))) return rc; }
    else { if ((rc = d_o.alloc_zero(24 * n))) return rc; }
    HIP_TRY(hipMemset(s->stats.p, 0, sizeof(DevStats)));
    EventPair ev; if ((rc = ev.start(0))) return rc;
    if (getenv("FTN_BATCH_SIMPLE")) launch_trace_batch(s->d, d_rays.p, n, mode, d_t.p, d_p.p, d_b.p, d_occ.p, d_o.p, s->stats.p, s->stack_entries, st != nullptr, 0);   /* one lane per ray, plain loop */
    else if ((rc = wavefront_trace_batch(&s->wf, s->d, s->stack_entries, d_rays.p, n, mode, st != nullptr, d_t.p, d_p.p, d_b.p, d_occ.p, d_o.p, s->stats.p, 0))) return fail(rc, wavefront_error());
    float ms; if ((rc = ev.stop(0, &ms))) return rc;
    if (t_hit) HIP_TRY(hipMemcpy(t_hit, d_t.p, n * 4, hipMemcpyDeviceToHost));
    if (prim) HIP_TRY(hipMemcpy(prim, d_p.p, n * 4, hipMemcpyDeviceToHost));
    if (bary) HIP_TRY(hipMemcpy(bary, d_b.p, 3 * n * 4, hipMemcpyDeviceToHost));
    if (occ) HIP_TRY(hipMemcpy(occ, d_occ.p, n, hipMemcpyDeviceToHost));
    if (out24) HIP_TRY(hipMemcpy(out24, d_o.p, 24 * n * 4, hipMemcpyDeviceToHost));
    DevStats ds; HIP_TRY(hipMemcpy(&ds, s->stats.p, sizeof(ds), hipMemcpyDeviceToHost));
    stats_out(ds, st, ms);
    return FTN_OK;
}
int ftn_intersect(const ftn_scene* s, const float* rays, size_t n, float* t_hit, int32_t* prim, float* bary, ftn_stats* st) {
    return trace_batch(s, rays, n, 0, t_hit, prim, bary, nullptr, nullptr, st);
}
int ftn_intersect_test(const ftn_scene* s, const float* rays, size_t n, uint8_t* occluded, ftn_stats* st) {
    return trace_batch(s, rays, n, 1, nullptr, nullptr, nullptr, occluded, nullptr, st);
}
int ftn_intersect_full(const ftn_scene* s, const float* rays, size_t n, float* out24) {
    return trace_batch(s, rays, n, 2, nullptr, nullptr, nullptr, nullptr, out24, nullptr);
}

/* ------------------------------------------------------------------ render */
int ftn_render_device(const ftn_scene* cs, const ftn_camera_desc* cam, const ftn_film_desc* film, const ftn_sampler_desc* sd, const ftn_integrator_desc* id,
                      const ftn_tile_range* tr, const ftn_render_options* opt, void* device_pixels, void* stream_v, ftn_stats* st) {
    if (!cs || !cam || !film || !sd || !id || !device_pixels) return fail(FTN_ERR_INVALID_ARGUMENT, "null argument");
    ftn_scene* s = const_cast<ftn_scene*>(cs);
    int rc = bind_scene_device(s, opt); if (rc) return rc;
    hipStream_t stream = (hipStream_t)stream_v;
    const bool indexed = sd->kind == FTN_SAMPLER_INDEXED;
    /* sample range [first_sample, first_sample + sample_count) must lie inside [0, samples_per_pixel] (64-bit: no wrap-around) */
    if (indexed && ((uint64_t)sd->first_sample > (uint64_t)sd->samples_per_pixel || (uint64_t)sd->first_sample + (uint64_t)sd->sample_count > (uint64_t)sd->samples_per_pixel))
        return fail(FTN_ERR_INVALID_ARGUMENT, "sample range outside [0, samples_per_pixel]");
    if (!indexed && sd->kind != FTN_SAMPLER_TILE_SERIAL) return fail(FTN_ERR_INVALID_ARGUMENT, "unknown sampler kind");
    if (!indexed && (sd->first_sample != 0 || (sd->sample_count != 0 && sd->sample_count != sd->samples_per_pixel)))
        return fail(FTN_ERR_INVALID_ARGUMENT, "sample ranges need FTN_SAMPLER_INDEXED");
    if (id->kind != FTN_INTEGRATOR_PATH && id->kind != FTN_INTEGRATOR_DIRECT_LIGHTING && id->kind != FTN_INTEGRATOR_WHITTED) return fail(FTN_ERR_INVALID_ARGUMENT, "unknown integrator kind");
    if (id->max_depth > 65535u) return fail(FTN_ERR_INVALID_ARGUMENT, "max_depth is a u16 in the reference (integrator/path.rs:14)");
    uint32_t pipeline = opt ? opt->pipeline : FTN_PIPELINE_AUTO;
    /* the wavefront pipeline renders the indexed sampler for PathIntegrator, DirectLightingIntegrator and WhittedIntegrator (the latter with at
     * most 32 lights: one bit per light in a path's pending-light word), and the reference's tile-serial sampler for PathIntegrator (one
     * path per tile in flight: wavefront_render_serial).  AUTO takes it for the tile-serial sampler once the call has enough tiles to fill
     * the queues (below, when the tile list is known); everything else is the megakernel's */
    const bool wf_ok = indexed ? (id->kind != FTN_INTEGRATOR_WHITTED || s->d.n_lights <= 32u) : id->kind == FTN_INTEGRATOR_PATH;
    const bool auto_pipeline = pipeline == FTN_PIPELINE_AUTO;
    if (auto_pipeline) pipeline = wf_ok ? FTN_PIPELINE_WAVEFRONT : FTN_PIPELINE_MEGAKERNEL;
    if (pipeline == FTN_PIPELINE_WAVEFRONT && !wf_ok)
        return fail(FTN_ERR_UNSUPPORTED, "the wavefront pipeline renders PathIntegrator with either sampler, DirectLightingIntegrator / WhittedIntegrator (up to 32 lights) with FTN_SAMPLER_INDEXED");
    const bool count = opt && opt->count_traffic;
    const bool count_production = opt && opt->count_traffic == 2;      /* tally the production configuration instead of the reference's walk */

    RenderParams P = render_params(s, cam, film, sd, id);
    if ((rc = scene_tiles(s, film, tr, stream, &P))) return rc;
    /* tile-serial: a round of the queue pipeline costs ~0.3 ms whatever it holds, a megakernel lane per tile diverges from its 63 neighbours:
     * the queues win once a call has a few thousand tiles (measured: profiles/r03), a handful of tiles is the megakernel's */
    if (auto_pipeline && !indexed && pipeline == FTN_PIPELINE_WAVEFRONT && P.n_tiles < 2048) pipeline = FTN_PIPELINE_MEGAKERNEL;
    if ((rc = prepare_film(s, false, stream, &P))) return rc;

    EventPair ev; if ((rc = ev.start(stream))) return rc;
    WavefrontTimes wt; memset(&wt, 0, sizeof(wt));
    if (pipeline == FTN_PIPELINE_WAVEFRONT) { rc = wavefront_render(&s->wf, P, s->sel, count, stream, &wt, count_production); if (rc) return fail(rc, wavefront_error()); }
    else launch_render_mega(P, count, stream);
    launch_film_resolve(P, (ftn_pixel*)device_pixels, stream);
    float ms; if ((rc = ev.stop(stream, &ms))) return rc;
    DevStats ds; if ((rc = read_stats(s, false, &ds))) return rc;
    if (ds.t4_occ[0] | ds.t4_occ[7]) { const char* dbg = getenv("FTN_WF_DEBUG"); if (dbg && atoi(dbg)) {     /* lane occupancy of the counting builds (experiments) */
        for (int k = 0; k < 2; k++) { const unsigned long long* o = &ds.t4_occ[7 * k]; if (!o[0]) continue;
            fprintf(stderr, "[wf] %s four-box trace: %llu control rounds; %llu record steps with %.1f of 64 lanes; %llu leaf steps with %.1f lanes; %llu refills of %.1f lanes\n", k ? "any-hit" : "closest-hit",
                    o[0], o[1], o[1] ? (double)o[2] / (double)o[1] : 0.0, o[3], o[3] ? (double)o[4] / (double)o[3] : 0.0, o[5], o[5] ? (double)o[6] / (double)o[5] : 0.0); } } }
    render_stats_out(ds, wt, ms, st);
    return render_error(ds.error);
}

int ftn_film_resolve_device(const void* device_pixels, size_t n, void* device_rgb_out, void* stream) {   /* film.rs:195-210 in HBM */
    if (!device_pixels || !device_rgb_out) return fail(FTN_ERR_INVALID_ARGUMENT, "null argument");
    if (ftn_device_count() <= 0) return fail(FTN_ERR_NO_DEVICE, "no HIP device");
    launch_spectrum_buffer((const ftn_pixel*)device_pixels, n, (float*)device_rgb_out, (hipStream_t)stream);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(FTN_ERR_INTERNAL, hipGetErrorString(e));
    return FTN_OK;
}

int ftn_render(const ftn_scene* cs, const ftn_camera_desc* cam, const ftn_film_desc* film, const ftn_sampler_desc* sd, const ftn_integrator_desc* id,
               const ftn_tile_range* tr, const ftn_render_options* opt, ftn_pixel* out_pixels, ftn_stats* st) {
    if (!cs || !film || !out_pixels) return fail(FTN_ERR_INVALID_ARGUMENT, "null argument");
    int rc = bind_scene_device(cs, opt); if (rc) return rc;
    const size_t npix = (size_t)std::max(0, film->crop[2] - film->crop[0]) * (size_t)std::max(0, film->crop[3] - film->crop[1]);
    /* merge_pixel.xyz[i] += xyz[i] (film.rs:127-130) */
    return render_to_host(npix, {{out_pixels, sizeof(ftn_pixel), true}},
                          [&](void* const* d) { return ftn_render_device(cs, cam, film, sd, id, tr, opt, d[0], nullptr, st); });
}

}  /* extern "C" */
