/*
 * ftn_adaptive_host.cpp -- C entry points of include/fountain_hip_adaptive.h.
 *
 * The driver takes the steps of ftn_render_moments_device (ftn_host_internal.h; accumulators cleared once per call), then runs rounds: the
 * active tiles (film tile order, valid_off recomputed) go to a per-call device tile list, wavefront_moments renders [n_r, n_{r+1}) for them,
 * and k_ad_tile_converged writes one byte per active tile, which is read back.  Nothing is cleared between rounds: every pixel's own sums
 * grow in sample order however the range is cut, and indexed_key makes each sample's stream independent of its neighbours' counts.  The
 * scene's cached tile list (ftn_scene::sel, tiles, tile_key) is not used.
 */
#include "ftn_stage_host.h"
#include "../../include/fountain_hip_adaptive.h"
#include "ftn_adaptive.h"

#include <cmath>
#include <cstring>

using namespace ftn;

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
    if (int no = need_device()) return no;
    ftn_scene* s = const_cast<ftn_scene*>(cs);
    if ((rc = bind_scene_device(s, opt))) return rc;
    hipStream_t stream = (hipStream_t)stream_v;
    const bool count = opt && opt->count_traffic, count_production = opt && opt->count_traffic == 2;
    const uint32_t N = sd->samples_per_pixel;

    std::vector<DTile> sel; select_tiles(film, tr, &sel);
    const uint32_t n_sel = (uint32_t)sel.size();
    RenderParams P = render_params(s, cam, film, sd, id);          /* (each round sets its tiles and sample range) */
    if ((rc = prepare_film(s, true, stream, &P))) return rc;
    /* per call: the active tile list (reused by the counts at the end), one flag and one count per tile */
    CallBuf<DTile> d_tiles; CallBuf<uint8_t> d_flags; CallBuf<uint32_t> d_counts;
    if (n_sel) {
        HIP_TRY(hipMalloc((void**)&d_tiles.p, n_sel * sizeof(DTile))); HIP_TRY(hipMalloc((void**)&d_flags.p, n_sel)); HIP_TRY(hipMalloc((void**)&d_counts.p, n_sel * sizeof(uint32_t)));
    }
    P.tiles = d_tiles.p;
    const MomentAcc M{s->moments.own.p, s->moments.in_tile.p, s->moments.other_tile.p};
    EventPair ev; if ((rc = ev.start(stream))) return rc;
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
    float ms; if ((rc = ev.stop(stream, &ms))) return rc;
    DevStats ds; if ((rc = read_stats(s, true, &ds))) return rc;
    render_stats_out(ds, wt, ms, st);
    if (info) {
        memset(info, 0, sizeof(*info));
        info->rounds = rounds; info->tiles = n_sel;
        for (uint32_t k = 0; k < n_sel; k++) {
            if (final_count[k] == N) info->tiles_at_max++;
            info->pixel_samples += (uint64_t)final_count[k] * tile_crop_pixels(sel[k], film->crop);
        }
    }
    return render_error(ds.error);
}

int ftn_render_adaptive(const ftn_scene* cs, const ftn_camera_desc* cam, const ftn_film_desc* film, const ftn_sampler_desc* sd, const ftn_integrator_desc* id,
                        const ftn_tile_range* tr, const ftn_render_options* opt, const ftn_adaptive_params* ap,
                        ftn_pixel* out_pixels, ftn_moment_pixel* out_moments, uint32_t* out_samples, ftn_adaptive_info* info, ftn_stats* st) {
    if (!cs || !cam || !film || !sd || !id || !ap || !out_pixels || !out_moments || !out_samples) return fail(FTN_ERR_INVALID_ARGUMENT, "null argument");
    int rc = adaptive_refusals(cs, sd, id, opt, ap); if (rc) return rc;
    if (int no = need_device()) return no;
    if ((rc = bind_scene_device(cs, opt))) return rc;
    const size_t npix = (size_t)std::max(0, film->crop[2] - film->crop[0]) * (size_t)std::max(0, film->crop[3] - film->crop[1]);
    /* as ftn_render_moments: the call's sums from zero device buffers, added once into the caller's; the counts only for the tile range's
     * pixels inside the crop */
    std::vector<uint32_t> counts(npix);
    rc = render_to_host(npix, {{out_pixels, sizeof(ftn_pixel), true}, {out_moments, sizeof(ftn_moment_pixel), true}, {counts.data(), sizeof(uint32_t), false}},
                        [&](void* const* d) { return ftn_render_adaptive_device(cs, cam, film, sd, id, tr, opt, ap, d[0], d[1], d[2], nullptr, info, st); });
    if ((rc == FTN_OK || rc == FTN_ERR_NAN_RADIANCE) && npix) {
        std::vector<DTile> sel; select_tiles(film, tr, &sel);
        const size_t width = (size_t)(film->crop[2] - film->crop[0]);
        for (const DTile& t : sel)
            for (int y = std::max(t.y0, film->crop[1]); y < std::min(t.y1, film->crop[3]); y++)
                for (int x = std::max(t.x0, film->crop[0]); x < std::min(t.x1, film->crop[2]); x++) {
                    const size_t i = (size_t)(y - film->crop[1]) * width + (size_t)(x - film->crop[0]);
                    out_samples[i] = counts[i];
                }
    }
    return rc;
}

}  /* extern "C" */
