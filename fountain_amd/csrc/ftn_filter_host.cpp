/*
 * ftn_filter_host.cpp -- C entry points of include/fountain_hip_filter.h: the filters and Film::new's table, the filtered render on
 * the steps of every render call (ftn_host_internal.h), and the host twin of the gather.
 *
 * Device memory.  The scene handle's moments accumulators (ftn_scene::moments: three grow-only arrays of one float4 per crop pixel,
 * grown by moments, adaptive and filtered calls only, freed with the scene, never touched by ftn_render) serve a filtered call, which
 * renders no moments: `own` holds the gather's running sums, `in_tile` the call's grid map followed by its output-tile list.  They are
 * left marked dirty, so the next moments call clears them as after any call that spilled.
 */
#include "ftn_stage_host.h"
#include "../../include/fountain_hip_filter.h"
#include "ftn_filter.h"

#include <cmath>
#include <cstring>

using namespace ftn;

namespace {

const double kPi = 3.14159265358979323846;

double mitchell_1d(double v, double B, double C) {
    const double t = std::fabs(2.0 * v);
    if (t > 1.0) return ((-B - 6.0 * C) * t * t * t + (6.0 * B + 30.0 * C) * t * t + (-12.0 * B - 48.0 * C) * t + (8.0 * B + 24.0 * C)) * (1.0 / 6.0);
    return ((12.0 - 9.0 * B - 6.0 * C) * t * t * t + (-18.0 + 12.0 * B + 6.0 * C) * t * t + (6.0 - 2.0 * B)) * (1.0 / 6.0);
}
double sinc(double v) { v = std::fabs(v); return v < 1e-5 ? 1.0 : std::sin(kPi * v) / (kPi * v); }
double windowed_sinc(double v, double r, double tau) { v = std::fabs(v); return v > r ? 0.0 : sinc(v) * sinc(v / tau); }
double gaussian_1d(double v, double r, double alpha) { return std::max(0.0, std::exp(-alpha * v * v) - std::exp(-alpha * r * r)); }

/* the filter's evaluate (PBRT v3's definitions, include/fountain_hip_filter.h) in binary64 */
double filter_evaluate(const ftn_filter_desc& f, double x, double y) {
    const double rx = f.radius[0], ry = f.radius[1], a = f.param[0], b = f.param[1];
    switch (f.kind) {
        case FTN_FILTER_BOX: return 1.0;
        case FTN_FILTER_TRIANGLE: return std::max(0.0, rx - std::fabs(x)) * std::max(0.0, ry - std::fabs(y));
        case FTN_FILTER_GAUSSIAN: return gaussian_1d(x, rx, a) * gaussian_1d(y, ry, a);
        case FTN_FILTER_MITCHELL: return mitchell_1d(x / rx, a, b) * mitchell_1d(y / ry, a, b);
        default: return windowed_sinc(x, rx, a) * windowed_sinc(y, ry, a);
    }
}

int filter_refusals(const ftn_filter_desc* f) {
    if (f->kind > FTN_FILTER_SINC) return fail(FTN_ERR_INVALID_ARGUMENT, "unknown filter kind");
    for (int k = 0; k < 2; k++)
        if (!std::isfinite(f->radius[k]) || !(f->radius[k] > 0.0f) || f->radius[k] > FTN_FILTER_MAX_RADIUS)
            return fail(FTN_ERR_INVALID_ARGUMENT, "a filter radius must be finite, above 0 and at most 8");
    if (!std::isfinite(f->param[0]) || !std::isfinite(f->param[1])) return fail(FTN_ERR_INVALID_ARGUMENT, "filter parameters must be finite");
    if (f->kind == FTN_FILTER_SINC && !(f->param[0] > 0.0f)) return fail(FTN_ERR_INVALID_ARGUMENT, "the sinc filter's tau must be above 0");
    return FTN_OK;
}

int filter_table(const ftn_filter_desc* f, FilterTable* T) {
    int rc = filter_refusals(f); if (rc) return rc;
    for (int k = 0; k < 2; k++) { T->radius[k] = f->radius[k]; T->inv_radius[k] = 1.0f / f->radius[k]; }
    for (int y = 0; y < 16; y++)
        for (int x = 0; x < 16; x++)
            T->w[y * 16 + x] = (float)filter_evaluate(*f, (x + 0.5) * (double)f->radius[0] / 16.0, (y + 0.5) * (double)f->radius[1] / 16.0);
    return FTN_OK;
}

int radius_refusal(const ftn_film_desc* film, const ftn_filter_desc* f) {
    if (memcmp(film->filter_radius, f->radius, sizeof(f->radius)) != 0)
        return fail(FTN_ERR_INVALID_ARGUMENT, "film->filter_radius must equal the filter's radius bit for bit: it decides the sample bounds and the tiles");
    return FTN_OK;
}

/* f(begin, end) over [0, n) in contiguous blocks on the host's threads (each element is written from its own inputs alone) */
template <class F> void filter_parallel_for(size_t n, F f) {
    const int nt = (int)std::min<size_t>((size_t)host_threads(), n / 64 + 1);
    if (nt <= 1) { f((size_t)0, n); return; }
    std::vector<std::thread> th;
    for (int t = 0; t < nt; t++) th.emplace_back([&, t]() { f(n * (size_t)t / (size_t)nt, n * (size_t)(t + 1) / (size_t)nt); });
    for (auto& x : th) x.join();
}

}  // namespace

extern "C" {

static_assert(sizeof(ftn_filter_desc) == 32, "ABI");
int ftn_filter_abi_version(void) { return FTN_FILTER_ABI_VERSION; }

int ftn_filter_init(uint32_t kind, ftn_filter_desc* out) {
    if (!out) return fail(FTN_ERR_INVALID_ARGUMENT, "null argument");
    if (kind > FTN_FILTER_SINC) return fail(FTN_ERR_INVALID_ARGUMENT, "unknown filter kind");
    memset(out, 0, sizeof(*out));
    out->kind = kind;
    const float r = kind == FTN_FILTER_BOX ? 0.5f : (kind == FTN_FILTER_SINC ? 4.0f : 2.0f);
    out->radius[0] = r; out->radius[1] = r;
    if (kind == FTN_FILTER_GAUSSIAN) out->param[0] = 2.0f;
    if (kind == FTN_FILTER_MITCHELL) { out->param[0] = 1.0f / 3.0f; out->param[1] = 1.0f / 3.0f; }
    if (kind == FTN_FILTER_SINC) out->param[0] = 3.0f;
    return FTN_OK;
}

int ftn_filter_table(const ftn_filter_desc* f, float table[256]) {
    if (!f || !table) return fail(FTN_ERR_INVALID_ARGUMENT, "null argument");
    FilterTable T; int rc = filter_table(f, &T); if (rc) return rc;
    memcpy(table, T.w, sizeof(T.w));
    return FTN_OK;
}

int ftn_render_filtered_device(const ftn_scene* cs, const ftn_camera_desc* cam, const ftn_film_desc* film, const ftn_filter_desc* filter, const ftn_sampler_desc* sd,
                               const ftn_integrator_desc* id, const ftn_tile_range* tr, const ftn_render_options* opt, void* device_pixels, void* stream_v, ftn_stats* st) {
    if (!cs || !cam || !film || !filter || !sd || !id || !device_pixels) return fail(FTN_ERR_INVALID_ARGUMENT, "null argument");
    FilterGather G; memset(&G, 0, sizeof(G));
    int rc;
    if ((rc = filter_table(filter, &G.T)) || (rc = radius_refusal(film, filter)) || (rc = moments_refusals(cs, sd, id, opt))) return rc;
    int32_t sb[4]; ftn_film_sample_bounds(film, sb);
    G.mx = filter_margin(filter->radius[0], sb[0], sb[2]); G.my = filter_margin(filter->radius[1], sb[1], sb[3]);
    if (G.mx > 16 || G.my > 16) return fail(FTN_ERR_UNSUPPORTED, "film coordinates too large for the filter's footprint to stay within one tile of its pixel");
    if (int no = need_device()) return no;
    ftn_scene* s = const_cast<ftn_scene*>(cs);
    if ((rc = bind_scene_device(s, opt))) return rc;
    hipStream_t stream = (hipStream_t)stream_v;
    const bool count = opt && opt->count_traffic, count_production = opt && opt->count_traffic == 2;

    /* the tiles come from the true radius; the beauty's own accumulate kernel, which runs behind every pass and whose film is discarded,
     * gets the box's 0.5 and so stays on its one-pixel-per-sample path instead of (2 r)^2 atomic adds per sample.  Its NaN flag and
     * the ray statistics are the call's. */
    RenderParams P = render_params(s, cam, film, sd, id);
    if ((rc = scene_tiles(s, film, tr, stream, &P))) return rc;
    P.radius[0] = P.radius[1] = 0.5f; P.inv_radius[0] = P.inv_radius[1] = 2.0f;

    /* the grid map and the output tiles: the 16 x 16 tiles of the sample-bounds grid that meet the crop and have a selected tile in
     * their 3 x 3 ring (the margin is at most 16, so every source lies inside that ring) */
    for (int k = 0; k < 4; k++) G.sb[k] = sb[k];
    G.grid_w = std::max(0, (sb[2] - sb[0] + 15) / 16); G.grid_h = std::max(0, (sb[3] - sb[1] + 15) / 16);
    const size_t n_grid = (size_t)G.grid_w * (size_t)G.grid_h;
    std::vector<int> grid_map(n_grid, -1);
    for (size_t k = 0; k < s->sel.size(); k++) grid_map[(size_t)((s->sel[k].y0 - sb[1]) / 16) * (size_t)G.grid_w + (size_t)((s->sel[k].x0 - sb[0]) / 16)] = (int)k;
    std::vector<FilterOutTile> out_tiles;
    for (int gy = 0; gy < G.grid_h; gy++)
        for (int gx = 0; gx < G.grid_w; gx++) {
            const int x0 = sb[0] + 16 * gx, y0 = sb[1] + 16 * gy, x1 = std::min(x0 + 16, sb[2]), y1 = std::min(y0 + 16, sb[3]);
            if (std::max(x0, film->crop[0]) >= std::min(x1, film->crop[2]) || std::max(y0, film->crop[1]) >= std::min(y1, film->crop[3])) continue;
            bool any = false;
            for (int ny = std::max(gy - 1, 0); ny <= std::min(gy + 1, G.grid_h - 1); ny++)
                for (int nx = std::max(gx - 1, 0); nx <= std::min(gx + 1, G.grid_w - 1); nx++) any = any || grid_map[(size_t)ny * (size_t)G.grid_w + (size_t)nx] >= 0;
            if (any) out_tiles.push_back(FilterOutTile{gx, gy});
        }
    G.n_out_tiles = (uint32_t)out_tiles.size();
    const size_t npx = (size_t)(16 + 2 * G.mx) * (size_t)(16 + 2 * G.my);
    G.chunk = (uint32_t)std::max<size_t>(1, std::min<size_t>(8, (40 * 1024 - npx * sizeof(int) - 256 * sizeof(float)) / (npx * (sizeof(float4) + sizeof(float2)))));

    /* the film's accumulators (discarded) and the gather's: `own` cleared, `in_tile` large enough for the map and the list */
    if ((rc = prepare_film(s, false, stream, &P))) return rc;
    const size_t map_bytes = (n_grid * sizeof(int) + 7) / 8 * 8, list_bytes = out_tiles.size() * sizeof(FilterOutTile);
    if ((rc = s->moments.prepare(std::max(crop_pixels(film), (map_bytes + list_bytes + sizeof(float4) - 1) / sizeof(float4)), stream))) return rc;
    char* const side = reinterpret_cast<char*>(s->moments.in_tile.p);
    if (n_grid) HIP_TRY(hipMemcpyAsync(side, grid_map.data(), n_grid * sizeof(int), hipMemcpyHostToDevice, stream));
    if (list_bytes) HIP_TRY(hipMemcpyAsync(side + map_bytes, out_tiles.data(), list_bytes, hipMemcpyHostToDevice, stream));
    G.grid_map = reinterpret_cast<const int*>(side); G.out_tiles = reinterpret_cast<const FilterOutTile*>(side + map_bytes);
    G.acc = s->moments.own.p;

    EventPair ev; if ((rc = ev.start(stream))) return rc;
    WavefrontTimes wt; memset(&wt, 0, sizeof(wt));
    if ((rc = wavefront_filtered(&s->wf, P, s->sel, count, count_production, G, stream, &wt))) return fail(rc, wavefront_error());
    launch_filter_merge(P, G.acc, (float4*)device_pixels, stream);
    float ms; if ((rc = ev.stop(stream, &ms))) return rc;          /* (waits: grid_map and out_tiles outlive their copies) */
    DevStats ds; if ((rc = read_stats(s, false, &ds))) return rc;
    render_stats_out(ds, wt, ms, st);
    return render_error(ds.error);
}

int ftn_render_filtered(const ftn_scene* cs, const ftn_camera_desc* cam, const ftn_film_desc* film, const ftn_filter_desc* filter, const ftn_sampler_desc* sd,
                        const ftn_integrator_desc* id, const ftn_tile_range* tr, const ftn_render_options* opt, ftn_pixel* out_pixels, ftn_stats* st) {
    if (!cs || !cam || !film || !filter || !sd || !id || !out_pixels) return fail(FTN_ERR_INVALID_ARGUMENT, "null argument");
    int rc;
    if ((rc = filter_refusals(filter)) || (rc = radius_refusal(film, filter)) || (rc = moments_refusals(cs, sd, id, opt))) return rc;
    { int32_t sb[4]; ftn_film_sample_bounds(film, sb);
      if (filter_margin(filter->radius[0], sb[0], sb[2]) > 16 || filter_margin(filter->radius[1], sb[1], sb[3]) > 16)
          return fail(FTN_ERR_UNSUPPORTED, "film coordinates too large for the filter's footprint to stay within one tile of its pixel"); }
    if (int no = need_device()) return no;
    if ((rc = bind_scene_device(cs, opt))) return rc;
    /* as ftn_render: the call's film from a zero device buffer, added once into the caller's */
    return render_to_host(crop_pixels(film), {{out_pixels, sizeof(ftn_pixel), true}},
                          [&](void* const* d) { return ftn_render_filtered_device(cs, cam, film, filter, sd, id, tr, opt, d[0], nullptr, st); });
}

int ftn_filter_accumulate_samples(const ftn_film_desc* film, const ftn_filter_desc* filter, size_t n, const int32_t* px, const int32_t* py, const uint32_t* sample,
                                  const float* p_film, const float* L, ftn_pixel* out_pixels) {
    if (!film || !filter || !out_pixels || (n && (!px || !py || !sample || !p_film || !L))) return fail(FTN_ERR_INVALID_ARGUMENT, "null argument");
    FilterTable T; int rc;
    if ((rc = filter_table(filter, &T)) || (rc = radius_refusal(film, filter))) return rc;
    /* the order of the sum: (sample, py, px) */
    std::vector<size_t> order(n);
    for (size_t i = 0; i < n; i++) order[i] = i;
    auto less = [&](size_t a, size_t b) { return sample[a] != sample[b] ? sample[a] < sample[b] : (py[a] != py[b] ? py[a] < py[b] : px[a] < px[b]); };
    std::sort(order.begin(), order.end(), less);
    for (size_t i = 1; i < n; i++) if (!less(order[i - 1], order[i])) return fail(FTN_ERR_INVALID_ARGUMENT, "two samples share (sample, py, px)");
    const int* c = film->crop;
    const size_t W = (size_t)std::max(0, c[2] - c[0]), npix = crop_pixels(film);
    if (npix == 0) return FTN_OK;
    /* per crop pixel the samples that cover it, in that order: count, then fill, walking the ordered list */
    auto footprint = [&](size_t i, int* b) {
        const float pdx = p_film[2 * i] - 0.5f, pdy = p_film[2 * i + 1] - 0.5f;
        b[0] = std::max(f2i_sat(ceilf(pdx - T.radius[0])), c[0]); b[1] = std::max(f2i_sat(ceilf(pdy - T.radius[1])), c[1]);
        b[2] = std::min(f2i_sat(floorf(pdx + T.radius[0])), c[2] - 1); b[3] = std::min(f2i_sat(floorf(pdy + T.radius[1])), c[3] - 1);
    };
    std::vector<size_t> first(npix + 1, 0);
    for (size_t i = 0; i < n; i++) { int b[4]; footprint(i, b); for (int y = b[1]; y <= b[3]; y++) for (int x = b[0]; x <= b[2]; x++) first[(size_t)(y - c[1]) * W + (size_t)(x - c[0]) + 1]++; }
    for (size_t q = 0; q < npix; q++) first[q + 1] += first[q];
    std::vector<size_t> terms(first[npix]), fill(first.begin(), first.end() - 1);
    for (size_t k = 0; k < n; k++) { const size_t i = order[k]; int b[4]; footprint(i, b); for (int y = b[1]; y <= b[3]; y++) for (int x = b[0]; x <= b[2]; x++) terms[fill[(size_t)(y - c[1]) * W + (size_t)(x - c[0])]++] = i; }
    filter_parallel_for(npix, [&](size_t q0, size_t q1) {
        for (size_t q = q0; q < q1; q++) {
            const int qx = c[0] + (int)(q % W), qy = c[1] + (int)(q / W);
            float a[4] = {0.0f, 0.0f, 0.0f, 0.0f};
            for (size_t t = first[q]; t < first[q + 1]; t++) {
                const size_t i = terms[t];
                filter_add_term(T.w, T.radius[0], T.radius[1], T.inv_radius[0], T.inv_radius[1], V2(p_film[2 * i] - 0.5f, p_film[2 * i + 1] - 0.5f), qx, qy,
                                L[3 * i], L[3 * i + 1], L[3 * i + 2], &a[0], &a[1], &a[2], &a[3]);
            }
            float xyz[3];
            rgb_to_xyz(Rgb(a[0], a[1], a[2]), xyz);
            /* as ftn_render_filtered: the call's film from a zero buffer, added once into the caller's */
            for (int k = 0; k < 3; k++) out_pixels[q].xyz[k] += 0.0f + xyz[k];
            out_pixels[q].filter_weight_sum += 0.0f + a[3];
        }
    });
    return FTN_OK;
}

}  /* extern "C" */
