/*
 * ftn_adaptive_host.cpp -- C entry points of include/fountain_hip_adaptive.h.
 *
 * They are part of the host library's translation unit: this file includes ftn_moments_host.cpp (which includes the denoiser's,
 * the G-buffer's and ftn_host.cpp) and the Makefile compiles it in its place, so that the driver shares the scene internals, the moments'
 * accumulator table and the tile rules without exporting them.
 *
 * The driver repeats ftn_render_moments_device's setup (accumulators cleared once per call), then runs rounds: the active tiles (film
 * tile order, valid_off recomputed) go to a per-call device tile list, wavefront_moments renders [n_r, n_{r+1}) for them, and
 * k_ad_tile_converged writes one byte per active tile, which is read back.  Nothing is cleared between rounds: every pixel's own sums grow
 * in sample order however the range is cut, and indexed_key makes each sample's stream independent of its neighbours' counts.  The
 * scene's cached tile list (ftn_scene::sel, tiles, tile_key) is not used.
 */
#include "ftn_moments_host.cpp"
#include "../../include/fountain_hip_adaptive.h"
#include "ftn_adaptive.h"

namespace {
int adaptive_param_refusals(const ftn_adaptive_params* p) {
    if (!(p->threshold >= 0.0f) || !std::isfinite(p->threshold)) return fail(FTN_ERR_INVALID_ARGUMENT, "ftn_adaptive_params.threshold must be finite and >= 0");
    if (!(p->abs_floor >= 0.0f) || !std::isfinite(p->abs_floor)) return fail(FTN_ERR_INVALID_ARGUMENT, "ftn_adaptive_params.abs_floor must be finite and >= 0");
    return FTN_OK;
}

/* every refusal of the adaptive call, in the header's order; host-side checks only, before any device work */
int adaptive_refusals(const ftn_scene* s, const ftn_sampler_desc* sd, const ftn_integrator_desc* id, const ftn_render_options* opt,
                      const ftn_adaptive_params* p) {
    int rc = adaptive_param_refusals(p); if (rc) return rc;
    if (p->min_samples < 2u || p->min_samples > sd->samples_per_pixel)
        return fail(FTN_ERR_INVALID_ARGUMENT, "ftn_adaptive_params.min_samples must lie in [2, samples_per_pixel]");
    if (sd->first_sample != 0 || (sd->sample_count != 0 && sd->sample_count != sd->samples_per_pixel))
        return fail(FTN_ERR_INVALID_ARGUMENT, "adaptive sampling renders the sampler's whole range: first_sample = 0, sample_count 0 or samples_per_pixel");
    return moments_refusals(s, sd, id, opt);
}

/* the tiles of the tile range, in film tile order (ftn_render_device's selection rule) */
void adaptive_tiles(const ftn_film_desc* film, const ftn_tile_range* tr, std::vector<DTile>* sel) {
    const uint32_t stride = tr && tr->stride ? tr->stride : 1, first = tr ? tr->first : 0, cnt = tr ? tr->count : 0;
    std::vector<DTile> all; list_tiles(film, &all);
    sel->clear();
    for (size_t i = first, k = 0; i < all.size() && (cnt == 0 || k < cnt); i += stride, k++) sel->push_back(all[i]);
}

/* the pixels of a tile inside the crop */
uint64_t tile_crop_pixels(const DTile& t, const int32_t* crop) {
    const int w = std::min(t.x1, crop[2]) - std::max(t.x0, crop[0]), h = std::min(t.y1, crop[3]) - std::max(t.y0, crop[1]);
    return w > 0 && h > 0 ? (uint64_t)w * (uint64_t)h : 0;
}

template <class T> struct CallBuf {             /* a device buffer that lives for one call */
    T* p = nullptr;
    ~CallBuf() { if (p) (void)hipFree(p); }
};
}  // namespace

extern "C" {

static_assert(sizeof(ftn_adaptive_params) == 16, "ABI");
static_assert(sizeof(ftn_adaptive_info) == 24, "ABI");
int ftn_adaptive_abi_version(void) { return FTN_ADAPTIVE_ABI_VERSION; }

void ftn_adaptive_params_default(ftn_adaptive_params* p) {
    if (!p) return;
    p->min_samples = 8; p->step_samples = 0; p->threshold = 0.05f; p->abs_floor = 0.01f;
}

int ftn_adaptive_converged(const ftn_pixel* beauty, const ftn_moment_pixel* m, size_t n, const ftn_adaptive_params* p, uint8_t* out) {
    if (!p || (n && (!beauty || !m || !out))) return fail(FTN_ERR_INVALID_ARGUMENT, "null argument");
    int rc = adaptive_param_refusals(p); if (rc) return rc;
    for (size_t i = 0; i < n; i++)
        out[i] = adaptive_pixel_converged(reinterpret_cast<const float*>(beauty + i), m[i].sq, p->threshold, p->abs_floor) ? 1 : 0;
    return FTN_OK;
}

int ftn_render_adaptive_device(const ftn_scene* cs, const ftn_camera_desc* cam, const ftn_film_desc* film, const ftn_sampler_desc* sd,
                               const ftn_integrator_desc* id, const ftn_tile_range* tr, const ftn_render_options* opt, const ftn_adaptive_params* ap,
                               void* device_pixels, void* device_moments, void* device_samples, void* stream_v, ftn_adaptive_info* info, ftn_stats* st) {
    if (!cs || !cam || !film || !sd || !id || !ap || !device_pixels || !device_moments || !device_samples) return fail(FTN_ERR_INVALID_ARGUMENT, "null argument");
    int rc = adaptive_refusals(cs, sd, id, opt, ap); if (rc) return rc;
    if (ftn_device_count() <= 0) return fail(FTN_ERR_NO_DEVICE, "no HIP device available: the fountain HIP path needs an AMD GPU (there is no CPU fallback)");
    ftn_scene* s = const_cast<ftn_scene*>(cs);
    if (opt && opt->device >= 0 && s->device >= 0 && opt->device != s->device) return fail(FTN_ERR_INVALID_ARGUMENT, "ftn_render_options.device differs from the device the scene was created on");
    if ((rc = set_device(opt && opt->device >= 0 ? opt->device : s->device))) return rc;
    hipStream_t stream = (hipStream_t)stream_v;
    const bool count = opt && opt->count_traffic, count_production = opt && opt->count_traffic == 2;
    const uint32_t N = sd->samples_per_pixel;

    std::vector<DTile> sel; adaptive_tiles(film, tr, &sel);
    const uint32_t n_sel = (uint32_t)sel.size();

    /* ftn_render_moments_device's parameters, accumulators and statistics */
    RenderParams P; memset(&P, 0, sizeof(P));
    P.S = s->d;
    memcpy(P.C.c2w, cam->camera_to_world.m, 64); memcpy(P.C.r2c, cam->raster_to_camera.m, 64);
    P.C.shutter_open = cam->shutter_open; P.C.shutter_close = cam->shutter_close; P.C.lens_radius = cam->lens_radius; P.C.focal_dist = cam->focal_dist;
    for (int k = 0; k < 3; k++) { P.C.dx_camera[k] = cam->dx_camera[k]; P.C.dy_camera[k] = cam->dy_camera[k]; }
    for (int i = 0; i < 4; i++) P.crop[i] = film->crop[i];
    P.radius[0] = film->filter_radius[0]; P.radius[1] = film->filter_radius[1]; P.inv_radius[0] = 1.0f / P.radius[0]; P.inv_radius[1] = 1.0f / P.radius[1];
    P.sampler_kind = sd->kind; P.spp = N; P.seed = sd->seed;
    P.integrator_kind = id->kind; P.max_depth = id->max_depth; P.rr_threshold = id->rr_threshold;
    P.stack_entries = s->stack_entries;

    const size_t npix = (size_t)std::max(0, film->crop[2] - film->crop[0]) * (size_t)std::max(0, film->crop[3] - film->crop[1]);
    if (npix > s->acc_pixels) {
        s->accA.release(); s->accB.release(); s->accC.release(); s->acc_pixels = 0;
        HIP_TRY(hipMalloc((void**)&s->accA.p, npix * sizeof(float4))); HIP_TRY(hipMalloc((void**)&s->accB.p, npix * sizeof(float4))); HIP_TRY(hipMalloc((void**)&s->accC.p, npix * sizeof(float4)));
        s->acc_pixels = npix; s->spill_acc_dirty = true;
    }
    SceneMoments& mo = scene_moments(s);
    if (npix > mo.pixels) {
        mo.release();
        HIP_TRY(hipMalloc((void**)&mo.own.p, npix * sizeof(float4))); HIP_TRY(hipMalloc((void**)&mo.in_tile.p, npix * sizeof(float4))); HIP_TRY(hipMalloc((void**)&mo.other_tile.p, npix * sizeof(float4)));
        mo.pixels = npix; mo.spill_dirty = true;
    }
    /* per call: the active tile list (reused by the counts at the end), one flag and one count per tile */
    CallBuf<DTile> d_tiles; CallBuf<uint8_t> d_flags; CallBuf<uint32_t> d_counts;
    if (n_sel) {
        HIP_TRY(hipMalloc((void**)&d_tiles.p, n_sel * sizeof(DTile))); HIP_TRY(hipMalloc((void**)&d_flags.p, n_sel)); HIP_TRY(hipMalloc((void**)&d_counts.p, n_sel * sizeof(uint32_t)));
    }
    HIP_TRY(hipMemsetAsync(s->accA.p, 0, npix * sizeof(float4), stream));
    if (s->spill_acc_dirty) { HIP_TRY(hipMemsetAsync(s->accB.p, 0, npix * sizeof(float4), stream)); HIP_TRY(hipMemsetAsync(s->accC.p, 0, npix * sizeof(float4), stream)); }
    s->spill_acc_dirty = true;
    HIP_TRY(hipMemsetAsync(mo.own.p, 0, npix * sizeof(float4), stream));
    if (mo.spill_dirty) { HIP_TRY(hipMemsetAsync(mo.in_tile.p, 0, npix * sizeof(float4), stream)); HIP_TRY(hipMemsetAsync(mo.other_tile.p, 0, npix * sizeof(float4), stream)); }
    mo.spill_dirty = true;
    HIP_TRY(hipMemsetAsync(s->stats.p, 0, sizeof(DevStats), stream));
    P.accA = s->accA.p; P.accB = s->accB.p; P.accC = s->accC.p; P.stats = s->stats.p; P.tiles = d_tiles.p;
    const MomentAcc M{mo.own.p, mo.in_tile.p, mo.other_tile.p};

    struct EventPair {
        hipEvent_t a = nullptr, b = nullptr;
        ~EventPair() { if (a) (void)hipEventDestroy(a); if (b) (void)hipEventDestroy(b); }
    } ev;
    HIP_TRY(hipEventCreate(&ev.a)); HIP_TRY(hipEventCreate(&ev.b));
    HIP_TRY(hipEventRecord(ev.a, stream));
    WavefrontTimes wt; memset(&wt, 0, sizeof(wt));

    std::vector<uint32_t> final_count(n_sel, 0);          /* per selected tile: its count once it has stopped */
    std::vector<uint32_t> active(n_sel);                  /* indices into sel of the active tiles, film tile order */
    for (uint32_t k = 0; k < n_sel; k++) active[k] = k;
    std::vector<DTile> act; std::vector<uint8_t> flags;
    uint32_t n_lo = 0, n_hi = ap->min_samples, rounds = 0;
    int dev_error = 0;
    while (!active.empty()) {
        rounds++;
        act.clear();
        uint32_t off = 0;
        for (uint32_t k : active) { DTile t = sel[k]; t.valid_off = off; t._pad = 0; off += (uint32_t)((t.x1 - t.x0) * (t.y1 - t.y0)); act.push_back(t); }
        HIP_TRY(hipMemcpyAsync(d_tiles.p, act.data(), act.size() * sizeof(DTile), hipMemcpyHostToDevice, stream));
        RenderParams Pr = P;
        Pr.n_tiles = (uint32_t)act.size(); Pr.first_sample = n_lo; Pr.last_sample = n_hi;
        WavefrontTimes t; memset(&t, 0, sizeof(t));
        if ((rc = wavefront_moments(&s->wf, Pr, act, count, count_production, M, stream, &t))) return fail(rc, wavefront_error());
        wt.trace_ms += t.trace_ms; wt.trace_launches += t.trace_launches; wt.any_ms += t.any_ms; wt.any_launches += t.any_launches;
        wt.shade_ms += t.shade_ms; wt.shade_launches += t.shade_launches; wt.sort_ms += t.sort_ms; wt.mis_any_rays += t.mis_any_rays;
        const bool last = n_hi >= N;
        if (!last) launch_adaptive_decide(Pr, M, d_tiles.p, (uint32_t)act.size(), ap->threshold, ap->abs_floor, d_flags.p, stream);
        HIP_TRY(hipGetLastError());
        flags.assign(act.size(), 0);
        if (!last) HIP_TRY(hipMemcpyAsync(flags.data(), d_flags.p, act.size(), hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipMemcpyAsync(&dev_error, &s->stats.p->error, sizeof(int), hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        /* a tile stops when it passed, at N, or when the round raised an error (the schedule ends there) */
        std::vector<uint32_t> next;
        for (size_t j = 0; j < active.size(); j++) {
            if (last || flags[j] || dev_error) final_count[active[j]] = n_hi;
            else next.push_back(active[j]);
        }
        active.swap(next);
        n_lo = n_hi;
        n_hi = (uint32_t)std::min<uint64_t>(N, (uint64_t)n_hi + (ap->step_samples ? ap->step_samples : n_hi));
    }
    launch_film_resolve(P, (ftn_pixel*)device_pixels, stream);
    launch_moments_merge(P, M, (float4*)device_moments, stream);
    if (n_sel) {
        HIP_TRY(hipMemcpyAsync(d_tiles.p, sel.data(), n_sel * sizeof(DTile), hipMemcpyHostToDevice, stream));
        HIP_TRY(hipMemcpyAsync(d_counts.p, final_count.data(), n_sel * sizeof(uint32_t), hipMemcpyHostToDevice, stream));
        launch_adaptive_counts(P, d_tiles.p, d_counts.p, n_sel, (uint32_t*)device_samples, stream);
    }
    HIP_TRY(hipEventRecord(ev.b, stream));
    HIP_TRY(hipEventSynchronize(ev.b));
    HIP_TRY(hipGetLastError());
    float ms = 0.0f; (void)hipEventElapsedTime(&ms, ev.a, ev.b);
    DevStats ds; HIP_TRY(hipMemcpy(&ds, s->stats.p, sizeof(ds), hipMemcpyDeviceToHost));
    s->spill_acc_dirty = ds.bc_writes != 0;
    mo.spill_dirty = ds.bc_writes != 0;
    ds.rays_closest += wt.mis_any_rays; ds.rays_any -= wt.mis_any_rays;
    stats_out(ds, st, ms);
    if (st) {
        st->trace_ms = wt.trace_ms; st->trace_launches = wt.trace_launches; st->mis_rays_any_hit = wt.mis_any_rays;
        st->any_ms = wt.any_ms; st->any_launches = wt.any_launches; st->shade_ms = wt.shade_ms; st->shade_launches = wt.shade_launches; st->sort_ms = wt.sort_ms;
    }
    if (info) {
        memset(info, 0, sizeof(*info));
        info->rounds = rounds; info->tiles = n_sel;
        for (uint32_t k = 0; k < n_sel; k++) {
            if (final_count[k] == N) info->tiles_at_max++;
            info->pixel_samples += (uint64_t)final_count[k] * tile_crop_pixels(sel[k], film->crop);
        }
    }
    if (ds.error == FTN_ERR_NAN_RADIANCE) return fail(FTN_ERR_NAN_RADIANCE, "NaN radiance value (integrator/mod.rs:285-287)");
    if (ds.error) return fail(ds.error, "unsupported material / integrator combination (e.g. specular glass: material/glass.rs:66)");
    return FTN_OK;
}

int ftn_render_adaptive(const ftn_scene* cs, const ftn_camera_desc* cam, const ftn_film_desc* film, const ftn_sampler_desc* sd, const ftn_integrator_desc* id,
                        const ftn_tile_range* tr, const ftn_render_options* opt, const ftn_adaptive_params* ap,
                        ftn_pixel* out_pixels, ftn_moment_pixel* out_moments, uint32_t* out_samples, ftn_adaptive_info* info, ftn_stats* st) {
    if (!cs || !cam || !film || !sd || !id || !ap || !out_pixels || !out_moments || !out_samples) return fail(FTN_ERR_INVALID_ARGUMENT, "null argument");
    int rc = adaptive_refusals(cs, sd, id, opt, ap); if (rc) return rc;
    if (ftn_device_count() <= 0) return fail(FTN_ERR_NO_DEVICE, "no HIP device available: the fountain HIP path needs an AMD GPU (there is no CPU fallback)");
    if (opt && opt->device >= 0 && cs->device >= 0 && opt->device != cs->device) return fail(FTN_ERR_INVALID_ARGUMENT, "ftn_render_options.device differs from the device the scene was created on");
    if ((rc = set_device(opt && opt->device >= 0 ? opt->device : cs->device))) return rc;
    const size_t npix = (size_t)std::max(0, film->crop[2] - film->crop[0]) * (size_t)std::max(0, film->crop[3] - film->crop[1]);
    /* as ftn_render_moments: the call's sums from zero device buffers, added once into the caller's */
    DevBuf<ftn_pixel> dev; DevBuf<ftn_moment_pixel> dev_m; DevBuf<uint32_t> dev_n;
    if ((rc = dev.alloc_zero(npix)) || (rc = dev_m.alloc_zero(npix)) || (rc = dev_n.alloc_zero(npix))) { dev.release(); dev_m.release(); dev_n.release(); return rc; }
    rc = ftn_render_adaptive_device(cs, cam, film, sd, id, tr, opt, ap, dev.p, dev_m.p, dev_n.p, nullptr, info, st);
    if ((rc == FTN_OK || rc == FTN_ERR_NAN_RADIANCE) && npix) {
        std::vector<ftn_pixel> h(npix); std::vector<ftn_moment_pixel> hm(npix); std::vector<uint32_t> hn(npix);
        if (hipMemcpy(h.data(), dev.p, npix * sizeof(ftn_pixel), hipMemcpyDeviceToHost) != hipSuccess ||
            hipMemcpy(hm.data(), dev_m.p, npix * sizeof(ftn_moment_pixel), hipMemcpyDeviceToHost) != hipSuccess ||
            hipMemcpy(hn.data(), dev_n.p, npix * sizeof(uint32_t), hipMemcpyDeviceToHost) != hipSuccess) {
            dev.release(); dev_m.release(); dev_n.release(); return fail(FTN_ERR_NO_DEVICE, "copy back failed");
        }
        for (size_t i = 0; i < npix; i++) {
            out_pixels[i].xyz[0] += h[i].xyz[0]; out_pixels[i].xyz[1] += h[i].xyz[1]; out_pixels[i].xyz[2] += h[i].xyz[2];
            out_pixels[i].filter_weight_sum += h[i].filter_weight_sum;
            for (int k = 0; k < 3; k++) out_moments[i].sq[k] += hm[i].sq[k];
            out_moments[i].sq_y += hm[i].sq_y;
        }
        /* the counts only for the tile range's pixels inside the crop */
        std::vector<DTile> sel; adaptive_tiles(film, tr, &sel);
        const size_t width = (size_t)(film->crop[2] - film->crop[0]);
        for (const DTile& t : sel)
            for (int y = std::max(t.y0, film->crop[1]); y < std::min(t.y1, film->crop[3]); y++)
                for (int x = std::max(t.x0, film->crop[0]); x < std::min(t.x1, film->crop[2]); x++) {
                    const size_t i = (size_t)(y - film->crop[1]) * width + (size_t)(x - film->crop[0]);
                    out_samples[i] = hn[i];
                }
    }
    dev.release(); dev_m.release(); dev_n.release();
    return rc;
}

}  /* extern "C" */
