// ORACLE -- TEST INFRASTRUCTURE ONLY.  C entry points (orc_*) of the CPU restatement; twins of the ftn_*
// functions declared in include/fountain_hip.h, plus orc_kat_* hooks for the reference's known-answer tests.
// Only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg may load this library.
#include "orc_render.hpp"
#include <thread>
#include <mutex>
#include <chrono>
#include <string>
#include <functional>

using namespace orc;

struct orc_scene { SceneData data; };

static thread_local std::string g_err;
static int fail(int code, const char* msg) { g_err = msg; return code; }

static Transform from_abi(const ftn_transform* t) { return Transform::make(Mat4::from_flat(t->m), Mat4::from_flat(t->inv)); }
static void to_abi(const Transform& t, ftn_transform* o) { memcpy(o->m, t.t.a, 64); memcpy(o->inv, t.invt.a, 64); }

extern "C" {

const char* orc_last_error(void) { return g_err.c_str(); }
int orc_uses_detmath(void) {
#ifdef ORC_DETMATH
    return 1;
#else
    return 0;
#endif
}

// ---------------------------------------------------------------- host constructors
int orc_transform_identity(ftn_transform* out) { to_abi(Transform::identity(), out); return 0; }
int orc_transform_translate(const float d[3], ftn_transform* out) { to_abi(tf_translate(Vec3(d[0], d[1], d[2])), out); return 0; }
int orc_transform_scale(float sx, float sy, float sz, ftn_transform* out) { to_abi(tf_scale(sx, sy, sz), out); return 0; }
int orc_transform_rotate(float deg, const float a[3], ftn_transform* out) {
    Transform t; if (!tf_rotate(deg, Vec3(a[0], a[1], a[2]), &t)) return fail(FTN_ERR_INVALID_ARGUMENT, "singular"); to_abi(t, out); return 0; }
int orc_transform_look_at(const float p[3], const float l[3], const float u[3], ftn_transform* out) {
    Transform t; if (!tf_look_at(Vec3(p[0], p[1], p[2]), Vec3(l[0], l[1], l[2]), Vec3(u[0], u[1], u[2]), &t)) return fail(FTN_ERR_INVALID_ARGUMENT, "singular"); to_abi(t, out); return 0; }
int orc_transform_from_flat(const float m[16], ftn_transform* out) {
    Transform t; if (!Transform::from_mat(Mat4::from_flat(m), &t)) return fail(FTN_ERR_INVALID_ARGUMENT, "singular"); to_abi(t, out); return 0; }
int orc_transform_mul(const ftn_transform* a, const ftn_transform* b, ftn_transform* out) { to_abi(from_abi(a) * from_abi(b), out); return 0; }
int orc_transform_inverse(const ftn_transform* a, ftn_transform* out) { to_abi(from_abi(a).inverse(), out); return 0; }
int orc_transform_perspective(float fov, float n, float f, ftn_transform* out) {
    Transform t; if (!tf_perspective(fov, n, f, &t)) return fail(FTN_ERR_INVALID_ARGUMENT, "singular"); to_abi(t, out); return 0; }
int orc_transform_point(const ftn_transform* t, const float p[3], float o[3]) { Vec3 r = tf_point(from_abi(t), Vec3(p[0], p[1], p[2])); o[0] = r.x; o[1] = r.y; o[2] = r.z; return 0; }
int orc_transform_vector(const ftn_transform* t, const float p[3], float o[3]) { Vec3 r = tf_vector(from_abi(t), Vec3(p[0], p[1], p[2])); o[0] = r.x; o[1] = r.y; o[2] = r.z; return 0; }
int orc_transform_normal(const ftn_transform* t, const float p[3], float o[3]) { Vec3 r = tf_normal(from_abi(t), Vec3(p[0], p[1], p[2])); o[0] = r.x; o[1] = r.y; o[2] = r.z; return 0; }
int orc_transform_points(const ftn_transform* t, size_t n, const float* in, float* out) { Transform T = from_abi(t); for (size_t i = 0; i < n; i++) { Vec3 r = tf_point(T, Vec3(in[3*i], in[3*i+1], in[3*i+2])); out[3*i] = r.x; out[3*i+1] = r.y; out[3*i+2] = r.z; } return 0; }
int orc_transform_normals(const ftn_transform* t, size_t n, const float* in, float* out) { Transform T = from_abi(t); for (size_t i = 0; i < n; i++) { Vec3 r = tf_normal(T, Vec3(in[3*i], in[3*i+1], in[3*i+2])); out[3*i] = r.x; out[3*i+1] = r.y; out[3*i+2] = r.z; } return 0; }
int orc_transform_swaps_handedness(const ftn_transform* t) { return from_abi(t).swaps_handedness() ? 1 : 0; }

int orc_sphere_init(const ftn_transform* o2w, const ftn_transform* w2o, int rev, float radius, float z_min, float z_max, float phi_max_deg, ftn_sphere* out) {
    Sphere s = Sphere::make(from_abi(o2w), from_abi(w2o), rev != 0, radius, z_min, z_max, phi_max_deg);
    memset(out, 0, sizeof(*out));
    out->object_to_world = *o2w; out->world_to_object = *w2o;
    out->radius = s.radius; out->z_min = s.z_min; out->z_max = s.z_max; out->theta_min = s.theta_min; out->theta_max = s.theta_max; out->phi_max = s.phi_max;
    out->reverse_orientation = rev ? 1 : 0;
    return 0;
}
int orc_camera_perspective(const ftn_transform* c2w, const int32_t res[2], const float sw[4], const float sh[2], float lens_radius, float focal_dist, float fov, ftn_camera_desc* out) {
    memset(out, 0, sizeof(*out));
    if (!make_perspective_camera(from_abi(c2w), res[0], res[1], sw, sh[0], sh[1], lens_radius, focal_dist, fov, out)) return fail(FTN_ERR_INVALID_ARGUMENT, "singular");
    return 0;
}
int orc_film_init(const int32_t res[2], const float cw[4], ftn_film_desc* out) { make_film(res, cw, out); return 0; }
int orc_film_sample_bounds(const ftn_film_desc* f, int32_t out[4]) { Film film; film.init(f); Bounds2i b = film.sample_bounds(); out[0] = b.x0; out[1] = b.y0; out[2] = b.x1; out[3] = b.y1; return 0; }
static void iter_tiles(Bounds2i b, int tile_size, std::vector<Bounds2i>* tiles) {            // Bounds2i::iter_tiles, bounds.rs:85-97
    for (int y = b.y0; y < b.y1; y += tile_size) for (int x = b.x0; x < b.x1; x += tile_size)
        tiles->push_back(Bounds2i{x, y, std::min(x + tile_size, b.x1), std::min(y + tile_size, b.y1)});
}
static void list_tiles(const Film& film, std::vector<Bounds2i>* tiles, Bounds2i* sb_out) {   // render_parallel: sample_bounds.iter_tiles(16), integrator/mod.rs:218-227
    Bounds2i sb = film.sample_bounds(); *sb_out = sb;
    iter_tiles(sb, 16, tiles);
}
int orc_film_tile_count(const ftn_film_desc* f, uint32_t* out) { Film film; film.init(f); std::vector<Bounds2i> t; Bounds2i sb; list_tiles(film, &t, &sb); *out = (uint32_t)t.size(); return 0; }
int orc_film_resolve(const ftn_pixel* p, size_t n, float* rgb) { film_resolve(p, n, rgb); return 0; }

// ---------------------------------------------------------------- scene
int orc_scene_create(const ftn_scene_desc* d, orc_scene** out) {
    orc_scene* s = new orc_scene();
    int rc = build_scene(d, &s->data);
    if (rc != 0) { delete s; return fail(rc, "invalid scene description"); }
    *out = s; return 0;
}
void orc_scene_destroy(orc_scene* s) { delete s; }
int orc_scene_info(const orc_scene* s, uint32_t* n_nodes, uint32_t* n_prims, uint32_t* n_lights, uint32_t* max_depth, float wb[6]) {
    const BVH& b = s->data.bvh;
    if (n_nodes) *n_nodes = (uint32_t)b.nodes.size();
    if (n_prims) *n_prims = (uint32_t)b.prims.size();
    if (n_lights) *n_lights = (uint32_t)s->data.lights.size();
    if (max_depth) *max_depth = b.max_depth;
    if (wb) for (int i = 0; i < 3; i++) { wb[i] = b.bounds.min[i]; wb[3 + i] = b.bounds.max[i]; }
    return 0;
}
int orc_scene_get_nodes(const orc_scene* s, ftn_bvh_node* nodes, uint32_t* order) {
    const BVH& b = s->data.bvh;
    if (nodes) memcpy(nodes, b.nodes.data(), b.nodes.size() * sizeof(ftn_bvh_node));
    if (order) for (size_t i = 0; i < b.prims.size(); i++) order[i] = b.prims[i].original_index;
    return 0;
}
// area-light table in Scene::lights order: per light {kind, prim (BVH order) or -1}
int orc_scene_get_lights(const orc_scene* s, int32_t* kind, int32_t* prim) {
    const SceneData& d = s->data;
    for (size_t i = 0; i < d.lights.size(); i++) { kind[i] = (int)d.lights[i].kind; prim[i] = -1; }
    for (size_t i = 0; i < d.bvh.prims.size(); i++) if (d.bvh.prims[i].light >= 0) prim[d.bvh.prims[i].light] = (int)i;
    return 0;
}

static Ray ray_from(const float* r) { Ray ray; ray.origin = Vec3(r[0], r[1], r[2]); ray.dir = Vec3(r[3], r[4], r[5]); ray.t_max = r[6]; ray.time = r[7]; return ray; }

static void parallel_for(size_t n, int n_threads, const std::function<void(size_t, size_t)>& fn) {
    if (n_threads <= 1 || n < 1024) { fn(0, n); return; }
    std::vector<std::thread> th; size_t chunk = (n + n_threads - 1) / n_threads;
    for (int t = 0; t < n_threads; t++) { size_t a = t * chunk, b = std::min(n, a + chunk); if (a < b) th.emplace_back(fn, a, b); }
    for (auto& t : th) t.join();
}

int orc_intersect(const orc_scene* s, const float* rays, size_t n, float* t_hit, int32_t* prim, float* bary, ftn_stats* stats, int n_threads) {
    const SceneData& d = s->data;
    std::atomic<uint64_t> nodes{0}, prims{0};
    parallel_for(n, n_threads, [&](size_t a, size_t b) {
        TraversalCounters c;
        for (size_t i = a; i < b; i++) {
            Ray ray = ray_from(rays + 8 * i); SurfaceInteraction si; bool deep = false;
            bool hit = d.bvh.intersect(ray, &si, &c, &deep);
            if (t_hit) t_hit[i] = hit ? ray.t_max : INF;
            if (prim) prim[i] = hit ? si.prim : -1;
            (void)bary;
        }
        nodes += c.nodes_visited; prims += c.prims_tested;
    });
    if (stats) { memset(stats, 0, sizeof(*stats)); stats->rays_closest = n; stats->nodes_visited = nodes; stats->prims_tested = prims; }
    return 0;
}
int orc_intersect_test(const orc_scene* s, const float* rays, size_t n, uint8_t* occluded, ftn_stats* stats, int n_threads) {
    const SceneData& d = s->data;
    std::atomic<uint64_t> nodes{0}, prims{0};
    parallel_for(n, n_threads, [&](size_t a, size_t b) {
        TraversalCounters c;
        for (size_t i = a; i < b; i++) { Ray ray = ray_from(rays + 8 * i); bool deep = false; occluded[i] = d.bvh.intersect_test(ray, &c, &deep) ? 1 : 0; }
        nodes += c.nodes_visited; prims += c.prims_tested;
    });
    if (stats) { memset(stats, 0, sizeof(*stats)); stats->rays_any = n; stats->nodes_visited = nodes; stats->prims_tested = prims; }
    return 0;
}
// p[3] p_err[3] n[3] uv[2] wo[3] dpdu[3] dpdv[3] shading_n[3] t
int orc_intersect_full(const orc_scene* s, const float* rays, size_t n, float* out24, int n_threads) {
    const SceneData& d = s->data;
    parallel_for(n, n_threads, [&](size_t a, size_t b) {
        for (size_t i = a; i < b; i++) {
            Ray ray = ray_from(rays + 8 * i); SurfaceInteraction si; bool deep = false; float* o = out24 + 24 * i;
            if (!d.bvh.intersect(ray, &si, nullptr, &deep)) { for (int k = 0; k < 24; k++) o[k] = 0.0f; o[23] = -1.0f; continue; }
            Vec3 v[] = {si.hit.p, si.hit.p_err, si.hit.n};
            for (int k = 0; k < 3; k++) for (int c = 0; c < 3; c++) o[3 * k + c] = v[k][c];
            o[9] = si.uv.x; o[10] = si.uv.y;
            Vec3 w[] = {si.wo, si.shading_geom.dpdu /* what Bsdf::new builds its frame from (bsdf.rs:24-26) */, si.geom.dpdv, si.shading_n};
            for (int k = 0; k < 4; k++) for (int c = 0; c < 3; c++) o[11 + 3 * k + c] = w[k][c];
            o[23] = ray.t_max;
        }
    });
    return 0;
}

// ---------------------------------------------------------------- render
}  // extern "C"

// orc_render's tile loop; with `records`, every camera sample is also written there (orc_render_sample_log's order)
static int render_tiles(const orc_scene* s, const ftn_camera_desc* cam, const ftn_film_desc* fd, const ftn_sampler_desc* sd,
                        const ftn_integrator_desc* id, const ftn_tile_range* tr, int n_threads, int count_traffic,
                        ftn_pixel* out_pixels, ftn_stats* stats, SampleRecord* records, size_t capacity, size_t* n_records) {
    SceneData& scene = const_cast<SceneData&>(s->data);
    scene.count_traffic = count_traffic != 0;
    scene.rays_closest = 0; scene.rays_any = 0; scene.nodes_visited = 0; scene.prims_tested = 0; scene.nodes_any = 0; scene.prims_any = 0; scene.error = 0;
    Camera camera;
    camera.camera_to_world = from_abi(&cam->camera_to_world); camera.raster_to_camera = from_abi(&cam->raster_to_camera);
    camera.shutter_open = cam->shutter_open; camera.shutter_close = cam->shutter_close;
    camera.lens_radius = cam->lens_radius; camera.focal_dist = cam->focal_dist;
    camera.dx_camera = Vec3(cam->dx_camera[0], cam->dx_camera[1], cam->dx_camera[2]);
    camera.dy_camera = Vec3(cam->dy_camera[0], cam->dy_camera[1], cam->dy_camera[2]);
    Film film; film.init(fd);
    Integrator it{id->kind, id->max_depth, id->rr_threshold};
    Sampler base; base.kind = sd->kind; base.base_seed = sd->seed; base.samples_per_pixel = sd->samples_per_pixel;
    base.rng = Xoshiro256Plus::seed_from_u64(sd->seed);
    if (sd->kind == FTN_SAMPLER_INDEXED && ((uint64_t)sd->first_sample > (uint64_t)sd->samples_per_pixel || (uint64_t)sd->first_sample + (uint64_t)sd->sample_count > (uint64_t)sd->samples_per_pixel))
        return fail(FTN_ERR_INVALID_ARGUMENT, "sample range outside [0, samples_per_pixel]");     /* same contract as ftn_render_device */
    base.first_sample = sd->first_sample;
    base.last_sample = sd->first_sample + (sd->sample_count ? sd->sample_count : (sd->samples_per_pixel - sd->first_sample));
    if (sd->kind == FTN_SAMPLER_TILE_SERIAL && (sd->first_sample != 0 || (sd->sample_count != 0 && sd->sample_count != sd->samples_per_pixel)))
        return fail(FTN_ERR_INVALID_ARGUMENT, "sample ranges need FTN_SAMPLER_INDEXED");

    std::vector<Bounds2i> all_tiles; Bounds2i sb; list_tiles(film, &all_tiles, &sb);
    std::vector<size_t> sel;
    uint32_t stride = tr && tr->stride ? tr->stride : 1, first = tr ? tr->first : 0, count = tr ? tr->count : 0;
    for (size_t i = first, k = 0; i < all_tiles.size() && (count == 0 || k < count); i += stride, k++) sel.push_back(i);
    // each selected tile's records start where the previous tile's end
    std::vector<size_t> rec_off(sel.size() + 1, 0);
    for (size_t k = 0; k < sel.size(); k++)
        rec_off[k + 1] = rec_off[k] + (size_t)std::max(all_tiles[sel[k]].area(), 0) * (size_t)(base.last_sample - base.first_sample);
    if (n_records) *n_records = rec_off.back();
    if (n_records && !records) return 0;
    if (records && capacity < rec_off.back()) return fail(FTN_ERR_INVALID_ARGUMENT, "record buffer too small");

    std::vector<FilmTile> done(sel.size());
    std::vector<TileStats> tstats(sel.size());
    std::atomic<size_t> next{0};
    auto t0 = std::chrono::steady_clock::now();
    auto worker = [&]() {
        for (;;) {
            size_t k = next.fetch_add(1); if (k >= sel.size()) break;
            Bounds2i tile = all_tiles[sel[k]];
            uint64_t tile_id = (uint64_t)(int64_t)(tile.y0 * sb.x1 + tile.x0);   // tile_id: integrator/mod.rs:182-185
            render_tile(scene, camera, film, it, base.clone_with_seed(tile_id), tile, &done[k], &tstats[k], records ? records + rec_off[k] : nullptr, (uint32_t)k);
        }
    };
    if (n_threads <= 0) n_threads = (int)std::thread::hardware_concurrency();
    if (n_threads <= 1) worker();
    else { std::vector<std::thread> th; for (int t = 0; t < n_threads; t++) th.emplace_back(worker); for (auto& t : th) t.join(); }
    auto t1 = std::chrono::steady_clock::now();
    // merge in tile order (Film::render's order; render_parallel's order is scheduling dependent)
    uint64_t cs = 0, spill = 0;
    for (size_t k = 0; k < sel.size(); k++) { if (out_pixels) film.merge_film_tile(done[k], out_pixels); cs += tstats[k].camera_samples; spill += tstats[k].spill_samples; }
    if (stats) {
        memset(stats, 0, sizeof(*stats));
        stats->rays_closest = scene.rays_closest; stats->rays_any = scene.rays_any;
        stats->nodes_visited = scene.nodes_visited; stats->prims_tested = scene.prims_tested;
        stats->nodes_visited_any = scene.nodes_any; stats->prims_tested_any = scene.prims_any;
        stats->camera_samples = cs; stats->spill_samples = spill;
        stats->kernel_ms = std::chrono::duration<double, std::milli>(t1 - t0).count();
    }
    int err = scene.error.load();
    if (err) return fail(err, err == FTN_ERR_NAN_RADIANCE ? "NaN radiance" : (err == FTN_ERR_BVH_TOO_DEEP ? "BVH deeper than 64" : "unsupported material configuration"));
    return 0;
}

extern "C" {

int orc_render(const orc_scene* s, const ftn_camera_desc* cam, const ftn_film_desc* fd, const ftn_sampler_desc* sd,
               const ftn_integrator_desc* id, const ftn_tile_range* tr, int n_threads, int count_traffic,
               ftn_pixel* out_pixels, ftn_stats* stats) {
    return render_tiles(s, cam, fd, sd, id, tr, n_threads, count_traffic, out_pixels, stats, nullptr, 0, nullptr);
}

// Not a twin of an ftn_* function: orc_render's tile loop (the indexed sampler only), which writes one orc_sample_record per camera
// sample -- selected-tile order, then row-major pixels within a tile, then increasing sample index (render_tile's order) -- and, when
// out_pixels is not null, also adds the film as orc_render does.  With records null it only stores the record count in *n_records.
struct orc_sample_record { int32_t px, py; uint32_t sample, tile; float p_film[2]; float L[3]; float ray_weight; };
static_assert(sizeof(orc_sample_record) == sizeof(SampleRecord) && sizeof(orc_sample_record) == 40, "record layout");
int orc_render_sample_log(const orc_scene* s, const ftn_camera_desc* cam, const ftn_film_desc* fd, const ftn_sampler_desc* sd,
                          const ftn_integrator_desc* id, const ftn_tile_range* tr, int n_threads,
                          orc_sample_record* records, size_t capacity, size_t* n_records, ftn_pixel* out_pixels, ftn_stats* stats) {
    if (!s || !cam || !fd || !sd || !id || !n_records) return fail(FTN_ERR_INVALID_ARGUMENT, "null argument");
    if (sd->kind != FTN_SAMPLER_INDEXED) return fail(FTN_ERR_UNSUPPORTED, "the sample log needs FTN_SAMPLER_INDEXED");
    return render_tiles(s, cam, fd, sd, id, tr, n_threads, 0, out_pixels, stats, reinterpret_cast<SampleRecord*>(records), capacity, n_records);
}

// ---------------------------------------------------------------- known-answer hooks (reference unit tests)
float orc_kat_fresnel_dielectric(float cos_i, float eta_i, float eta_t) { return fresnel_dielectric(cos_i, eta_i, eta_t); }   // fresnel.rs:110-116
void orc_kat_fresnel_conductor(float cos_i, const float eta[3], const float k[3], float out[3]) {
    Spectrum r = fresnel_conductor(fabsf(cos_i), Spectrum(1.0f), Spectrum(eta[0], eta[1], eta[2]), Spectrum(k[0], k[1], k[2]));
    out[0] = r[0]; out[1] = r[1]; out[2] = r[2]; }
int orc_kat_bounds_intersect(const float bmin[3], const float bmax[3], const float ray8[8], float out[2]) {   // bounds.rs:292-323
    Bounds3 b; b.min = Vec3(bmin[0], bmin[1], bmin[2]); b.max = Vec3(bmax[0], bmax[1], bmax[2]);
    return b.intersect_test(ray_from(ray8), &out[0], &out[1]) ? 1 : 0; }
int orc_kat_solve_2x2(const float a[4], const float b[2], float x[2]) { return solve_linear_system_2x2(a[0], a[1], a[2], a[3], b[0], b[1], &x[0], &x[1]) ? 1 : 0; }   // math.rs:88-102 (Matrix2::new(c0r0,c0r1,c1r0,c1r1))
int orc_kat_sign_differs(float a, float b, float c) { return sign_differs(a, b, c) ? 1 : 0; }                     // triangle.rs:441-450
void orc_kat_distribution1d(const float* f, size_t n, float u, float out[3]) {                                    // sampling.rs:188-198
    Distribution1D d; d.init(f, n); Float x, pdf; size_t idx; d.sample_continuous(u, &x, &pdf, &idx); out[0] = x; out[1] = pdf; out[2] = (float)idx; }
void orc_kat_concentric_disk(float u0, float u1, float out[2]) { Vec2 d = concentric_sample_disk(Vec2(u0, u1)); out[0] = d.x; out[1] = d.y; }   // sampling.rs:200-208
void orc_kat_cosine_hemisphere(float u0, float u1, float out[3]) { Vec3 d = cosine_sample_hemisphere(Vec2(u0, u1)); out[0] = d.x; out[1] = d.y; out[2] = d.z; }
void orc_kat_xoshiro(const uint64_t s[4], uint64_t* out, size_t n) { Xoshiro256Plus r; for (int i = 0; i < 4; i++) r.s[i] = s[i]; for (size_t i = 0; i < n; i++) out[i] = r.next_u64(); }
void orc_kat_splitmix(uint64_t seed, uint64_t* out, size_t n) { SplitMix64 r{seed}; for (size_t i = 0; i < n; i++) out[i] = r.next_u64(); }
void orc_kat_sampler_f32(uint64_t seed, float* out, size_t n) { Xoshiro256Plus r = Xoshiro256Plus::seed_from_u64(seed); for (size_t i = 0; i < n; i++) out[i] = r.gen_f32(); }
void orc_kat_indexed_f32(uint64_t seed, int32_t px, int32_t py, uint32_t sample, float* out, size_t n) {
    Xoshiro256Plus r = Xoshiro256Plus::seed_from_u64(indexed_sample_key(seed, px, py, sample)); for (size_t i = 0; i < n; i++) out[i] = r.gen_f32(); }
void orc_kat_permutation(int64_t* items, const int64_t* perm, size_t n) { std::vector<int64_t> o(n); for (size_t i = 0; i < n; i++) o[i] = items[perm[i]]; memcpy(items, o.data(), n * 8); }   // bvh.rs:391-398
float orc_kat_next_float_up(float v) { return next_float_up(v); }
float orc_kat_next_float_down(float v) { return next_float_down(v); }
float orc_kat_gamma(int n) { return gamma(n); }
// camera ray for the camera tests (camera/mod.rs:220-366): out = o[3] d[3]
void orc_kat_camera_ray(const ftn_camera_desc* cam, const float sample5[5], float out[6]) {
    Camera c; c.camera_to_world = from_abi(&cam->camera_to_world); c.raster_to_camera = from_abi(&cam->raster_to_camera);
    c.shutter_open = cam->shutter_open; c.shutter_close = cam->shutter_close; c.lens_radius = cam->lens_radius; c.focal_dist = cam->focal_dist;
    c.dx_camera = Vec3(cam->dx_camera[0], cam->dx_camera[1], cam->dx_camera[2]); c.dy_camera = Vec3(cam->dy_camera[0], cam->dy_camera[1], cam->dy_camera[2]);
    CameraSample cs; cs.p_film = Vec2(sample5[0], sample5[1]); cs.p_lens = Vec2(sample5[2], sample5[3]); cs.time = sample5[4];
    Float w; RayDifferential rd = c.generate_ray_differential(cs, &w);
    out[0] = rd.ray.origin.x; out[1] = rd.ray.origin.y; out[2] = rd.ray.origin.z; out[3] = rd.ray.dir.x; out[4] = rd.ray.dir.y; out[5] = rd.ray.dir.z;
}
// the camera ray of a sample as render_tile hands it to the integrator (mod.rs:252-254: generate_ray_differential, then
// scale_differentials(1 / sqrt(spp))) and, with hit12 = {p, n, dpdu, dpdv} of a surface, compute_tex_differentials there
// (interaction.rs:124-173).  out = o[3] d[3] rx_origin[3] rx_dir[3] ry_origin[3] ry_dir[3] dudx dvdx dudy dvdy (zeros without hit12)
void orc_kat_camera_ray_differential(const ftn_camera_desc* cam, const float sample5[5], uint32_t spp, const float* hit12, float out[22]) {
    Camera c; c.camera_to_world = from_abi(&cam->camera_to_world); c.raster_to_camera = from_abi(&cam->raster_to_camera);
    c.shutter_open = cam->shutter_open; c.shutter_close = cam->shutter_close; c.lens_radius = cam->lens_radius; c.focal_dist = cam->focal_dist;
    c.dx_camera = Vec3(cam->dx_camera[0], cam->dx_camera[1], cam->dx_camera[2]); c.dy_camera = Vec3(cam->dy_camera[0], cam->dy_camera[1], cam->dy_camera[2]);
    CameraSample cs; cs.p_film = Vec2(sample5[0], sample5[1]); cs.p_lens = Vec2(sample5[2], sample5[3]); cs.time = sample5[4];
    Float w; RayDifferential rd = c.generate_ray_differential(cs, &w);
    rd.scale_differentials(1.0f / sqrtf((Float)spp));
    Vec3 v[] = {rd.ray.origin, rd.ray.dir, rd.diff.rx_origin, rd.diff.rx_dir, rd.diff.ry_origin, rd.diff.ry_dir};
    for (int k = 0; k < 6; k++) for (int i = 0; i < 3; i++) out[3 * k + i] = v[k][i];
    SurfaceInteraction si;
    if (hit12) {
        si.hit.p = Vec3(hit12[0], hit12[1], hit12[2]); si.hit.n = Vec3(hit12[3], hit12[4], hit12[5]);
        si.geom.dpdu = Vec3(hit12[6], hit12[7], hit12[8]); si.geom.dpdv = Vec3(hit12[9], hit12[10], hit12[11]);
        si.compute_tex_differentials(rd);
    }
    out[18] = si.tex_diffs.dudx; out[19] = si.tex_diffs.dvdx; out[20] = si.tex_diffs.dudy; out[21] = si.tex_diffs.dvdy;
}
// t_max and time of the same ray (Ray::transform shifts t_max, transform.rs:307-322): out = t_max, time
void orc_kat_camera_ray_full(const ftn_camera_desc* cam, const float sample5[5], float out[2]) {
    Camera c; c.camera_to_world = from_abi(&cam->camera_to_world); c.raster_to_camera = from_abi(&cam->raster_to_camera);
    c.shutter_open = cam->shutter_open; c.shutter_close = cam->shutter_close; c.lens_radius = cam->lens_radius; c.focal_dist = cam->focal_dist;
    c.dx_camera = Vec3(cam->dx_camera[0], cam->dx_camera[1], cam->dx_camera[2]); c.dy_camera = Vec3(cam->dy_camera[0], cam->dy_camera[1], cam->dy_camera[2]);
    CameraSample cs; cs.p_film = Vec2(sample5[0], sample5[1]); cs.p_lens = Vec2(sample5[2], sample5[3]); cs.time = sample5[4];
    Float w; RayDifferential rd = c.generate_ray_differential(cs, &w);
    out[0] = rd.ray.t_max; out[1] = rd.ray.time;
}
// SurfaceHit::spawn_ray (interaction.rs:22-30) from p, p_err, n along d: out = the ray's 8 floats (o, d, t_max, time 0)
void orc_kat_spawn_ray(const float p[3], const float p_err[3], const float n[3], const float d[3], float out8[8]) {
    SurfaceHit h; h.p = Vec3(p[0], p[1], p[2]); h.p_err = Vec3(p_err[0], p_err[1], p_err[2]); h.n = Vec3(n[0], n[1], n[2]); h.time = 0.0f;
    Ray r = h.spawn_ray(Vec3(d[0], d[1], d[2]));
    out8[0] = r.origin.x; out8[1] = r.origin.y; out8[2] = r.origin.z; out8[3] = r.dir.x; out8[4] = r.dir.y; out8[5] = r.dir.z; out8[6] = r.t_max; out8[7] = r.time;
}
// Transform::tf_err_to_err for points / vectors (transform.rs:411-437): out = t[3] err[3]
void orc_kat_tf_err(const ftn_transform* t, const float p[3], const float e[3], int is_point, float out[6]) {
    Vec3 err; Vec3 r = is_point ? tf_point_err_to_err(from_abi(t), Vec3(p[0], p[1], p[2]), Vec3(e[0], e[1], e[2]), &err)
                                : tf_vector_err_to_err(from_abi(t), Vec3(p[0], p[1], p[2]), Vec3(e[0], e[1], e[2]), &err);
    out[0] = r.x; out[1] = r.y; out[2] = r.z; out[3] = err.x; out[4] = err.y; out[5] = err.z;
}
// Ray::transform (transform.rs:307-322): in/out 8 floats
void orc_kat_tf_ray(const ftn_transform* t, const float in8[8], float out8[8]) {
    Ray r = tf_ray(from_abi(t), ray_from(in8));
    out8[0] = r.origin.x; out8[1] = r.origin.y; out8[2] = r.origin.z; out8[3] = r.dir.x; out8[4] = r.dir.y; out8[5] = r.dir.z; out8[6] = r.t_max; out8[7] = r.time;
}
// single-shape sphere intersect (sphere.rs:241-273): returns hit; out = t, p_err[3], p[3]
int orc_kat_sphere_intersect(const ftn_sphere* sp, const float ray8[8], float out[7]) {
    Sphere s; s.object_to_world = from_abi(&sp->object_to_world); s.world_to_object = from_abi(&sp->world_to_object);
    s.reverse_orientation = sp->reverse_orientation; s.radius = sp->radius; s.z_min = sp->z_min; s.z_max = sp->z_max;
    s.theta_min = sp->theta_min; s.theta_max = sp->theta_max; s.phi_max = sp->phi_max;
    Float t; SurfaceInteraction si;
    if (!s.intersect(ray_from(ray8), &t, &si)) return 0;
    out[0] = t; out[1] = si.hit.p_err.x; out[2] = si.hit.p_err.y; out[3] = si.hit.p_err.z; out[4] = si.hit.p.x; out[5] = si.hit.p.y; out[6] = si.hit.p.z;
    return 1;
}
float orc_kat_math(int which, float x, float y) {
    switch (which) { case 0: return m_sin(x); case 1: return m_cos(x); case 2: return m_tan(x); case 3: return m_acos(x);
                     case 4: return m_atan(x); case 5: return m_atan2(x, y); case 6: return m_ln(x); case 7: return m_log2(x); case 13: return m_pow(x, y); default: return 0.0f; }
}
float orc_kat_roughness_to_alpha(float r) { return roughness_to_alpha(r); }
// imageio/mod.rs:169-175 inverse_gamma_correct, applied by load_mipmap (imageio/mod.rs:101-107) to every channel of a gamma-encoded map
static inline Float inverse_gamma_correct(Float v) { return v <= 0.04045f ? v * 1.0f / 12.92f : m_pow((v + 0.055f) * 1.0f / 1.055f, 2.4f); }
int orc_image_inverse_gamma(float* texels, size_t n) { if (!texels && n) return FTN_ERR_INVALID_ARGUMENT; for (size_t i = 0; i < n; i++) texels[i] = inverse_gamma_correct(texels[i]); return FTN_OK; }
// Bounds2i::iter_points / iter_tiles (bounds.rs:76-97): out holds 2 ints per point / 4 per tile; returns the count
size_t orc_kat_iter_points(const int32_t b[4], int32_t* out, size_t cap) {
    size_t n = 0;
    for (int y = b[1]; y < b[3]; y++) for (int x = b[0]; x < b[2]; x++) { if (n < cap) { out[2 * n] = x; out[2 * n + 1] = y; } n++; }
    return n;
}
size_t orc_kat_iter_tiles(const int32_t b[4], int32_t tile_size, int32_t* out, size_t cap) {
    std::vector<Bounds2i> t; iter_tiles(Bounds2i{b[0], b[1], b[2], b[3]}, tile_size, &t);
    for (size_t i = 0; i < t.size() && i < cap; i++) { out[4 * i] = t[i].x0; out[4 * i + 1] = t[i].y0; out[4 * i + 2] = t[i].x1; out[4 * i + 3] = t[i].y1; }
    return t.size();
}
// ---- textures (orc_texture.hpp)
// a level of the pyramid MIPMap::new builds (mipmap.rs:78-145)
int orc_test_mipmap_level(uint32_t w, uint32_t h, const float* texels, uint32_t level, uint32_t* lw, uint32_t* lh, float* rgb_out) {
    MIPMap m = MIPMap::make((int)w, (int)h, texels, FTN_WRAP_REPEAT);
    if ((int)level >= m.levels()) return FTN_ERR_INVALID_ARGUMENT;
    const MipLevel& L = m.pyramid[level];
    if (lw) *lw = (uint32_t)L.w;
    if (lh) *lh = (uint32_t)L.h;
    if (rgb_out) for (size_t i = 0; i < L.data.size(); i++) for (int c = 0; c < 3; c++) rgb_out[3 * i + c] = L.data[i][c];
    return FTN_OK;
}
// Texture::evaluate for rows of {u, v, dudx, dvdx, dudy, dvdy}
int orc_test_texture_eval(const orc_scene* s, int32_t texture, const float* in6, size_t n, float* out3) {
    if (texture < 0 || (size_t)texture >= s->data.tex.textures.size()) return FTN_ERR_INVALID_ARGUMENT;
    for (size_t i = 0; i < n; i++) {
        SurfaceInteraction si; si.uv = Vec2(in6[6 * i], in6[6 * i + 1]);
        si.tex_diffs.dudx = in6[6 * i + 2]; si.tex_diffs.dvdx = in6[6 * i + 3]; si.tex_diffs.dudy = in6[6 * i + 4]; si.tex_diffs.dvdy = in6[6 * i + 5];
        Spectrum c = s->data.tex.evaluate(texture, si);
        out3[3 * i] = c[0]; out3[3 * i + 1] = c[1]; out3[3 * i + 2] = c[2];
    }
    return FTN_OK;
}
// the constant-per-material part of compute_scattering_functions (orc_reflection.hpp: matte.rs:39-50 + OrenNayar::new, the remap of
// metal.rs:40-44, plastic.rs:35-38, glass.rs:57-61), written back into the record the way the device keeps it
static void finalize_material(ftn_material& m) {
    if (m.type == FTN_MAT_MATTE) {
        m.s0 = clampf(m.s0, 0.0f, 90.0f);
        if (m.s0 != 0.0f) { Float sg = deg_to_rad_cgmath(m.s0); Float sigma2 = sg * sg; m.s1 = 1.0f - (sigma2 / (2.0f * (sigma2 + 0.33f))); m.s2 = 0.45f * sigma2 / (sigma2 + 0.09f); }
    } else if (m.type == FTN_MAT_METAL || m.type == FTN_MAT_GLASS) {
        if (m.remap_roughness) { m.s1 = roughness_to_alpha(m.s1); m.s2 = roughness_to_alpha(m.s2); m.remap_roughness = 0; }
    } else if (m.type == FTN_MAT_PLASTIC) {
        if (m.remap_roughness) { m.s1 = roughness_to_alpha(m.s1); m.remap_roughness = 0; }
    }
}
// ---- textured materials: the twin of ftn_test_material (fountain_hip.h has the row layouts): TextureSet::resolve, then the step above
int orc_test_material(const orc_scene* s, int32_t material, const float* in6, size_t n, float* out16) {
    if (!s || !in6 || !out16) return fail(FTN_ERR_INVALID_ARGUMENT, "null argument");
    if (material < 0 || (size_t)material >= s->data.materials.size()) return fail(FTN_ERR_INVALID_ARGUMENT, "material index out of range");
    const ftn_material_textures* mt = s->data.mtex.empty() ? nullptr : &s->data.mtex[material];
    const bool textured = mt && (mt->a & mt->b & mt->s0 & mt->s1 & mt->s2) >= 0;
    for (size_t i = 0; i < n; i++) {
        const float* r = in6 + 6 * i; float* o = out16 + 16 * i;
        SurfaceInteraction si; si.uv = Vec2(r[0], r[1]);
        si.tex_diffs.dudx = r[2]; si.tex_diffs.dvdx = r[3]; si.tex_diffs.dudy = r[4]; si.tex_diffs.dvdy = r[5];
        ftn_material m = s->data.tex.resolve(s->data.materials[material], textured ? mt : nullptr, si);
        finalize_material(m);
        const uint32_t type = m.type, remap = m.remap_roughness;
        o[0] = textured ? 1.0f : 0.0f; memcpy(o + 1, &type, 4); memcpy(o + 2, &remap, 4);
        for (int k = 0; k < 3; k++) { o[3 + k] = m.a[k]; o[6 + k] = m.b[k]; }
        o[9] = m.s0; o[10] = m.s1; o[11] = m.s2; o[12] = o[13] = o[14] = o[15] = 0.0f;
    }
    return FTN_OK;
}
// ---- BSDFs (orc_reflection.hpp): the twin of ftn_test_bsdf (fountain_hip.h has the row layouts); `specialised` has no meaning here
int orc_test_bsdf(const orc_scene* s, int32_t material, uint32_t flags, int allow_multiple_lobes, int /*specialised*/, const float* in17, size_t n, float* out16) {
    if (!s || !in17 || !out16) return fail(FTN_ERR_INVALID_ARGUMENT, "null argument");
    if (material < 0 || (size_t)material >= s->data.materials.size()) return fail(FTN_ERR_INVALID_ARGUMENT, "material index out of range");
    if (flags > 31u) return fail(FTN_ERR_INVALID_ARGUMENT, "flags hold bits outside BxDFType");
    if (!s->data.mtex.empty()) { const ftn_material_textures& mt = s->data.mtex[material];
        if ((mt.a & mt.b & mt.s0 & mt.s1 & mt.s2) >= 0) return fail(FTN_ERR_UNSUPPORTED, "orc_test_bsdf takes materials with constant parameters only"); }
    const ftn_material& m = s->data.materials[material];
    for (size_t i = 0; i < n; i++) {
        const float* r = in17 + 17 * i; float* o = out16 + 16 * i;
        for (int k = 0; k < 16; k++) o[k] = 0.0f;
        SurfaceInteraction si;
        si.hit.n = Vec3(r[0], r[1], r[2]); si.shading_n = Vec3(r[3], r[4], r[5]); si.shading_geom.dpdu = Vec3(r[6], r[7], r[8]);
        const Vec3 wo(r[9], r[10], r[11]), wi(r[12], r[13], r[14]); const Vec2 u(r[15], r[16]);
        si.wo = wo;
        Bsdf bsdf;
        if (compute_scattering_functions(m, si, allow_multiple_lobes != 0, &bsdf) != MAT_OK) continue;
        const Spectrum f = bsdf.f(wo, wi, (uint8_t)flags);
        o[0] = 1.0f; o[1] = (float)bsdf.num_components((uint8_t)flags); o[2] = f[0]; o[3] = f[1]; o[4] = f[2]; o[5] = bsdf.pdf(wo, wi, (uint8_t)flags);
        ScatterSample sc;
        if (bsdf.sample_f(wo, u, (uint8_t)flags, &sc)) {
            o[6] = 1.0f; o[7] = sc.f[0]; o[8] = sc.f[1]; o[9] = sc.f[2]; o[10] = sc.wi.x; o[11] = sc.wi.y; o[12] = sc.wi.z; o[13] = sc.pdf; o[14] = (float)sc.sampled_type;
        }
    }
    return FTN_OK;
}
// ---- lights (orc_scene.hpp, orc_shapes.hpp): the twin of ftn_test_light (fountain_hip.h has the row layouts); `via_env0` has no meaning here
int orc_test_light(const orc_scene* s, int32_t light, int /*via_env0*/, const float* in15, size_t n, float* out24) {
    if (!s || !in15 || !out24) return fail(FTN_ERR_INVALID_ARGUMENT, "null argument");
    if (light < 0 || (size_t)light >= s->data.lights.size()) return fail(FTN_ERR_INVALID_ARGUMENT, "light index out of range");
    const Light& L = s->data.lights[light];
    for (size_t i = 0; i < n; i++) {
        const float* r = in15 + 15 * i; float* o = out24 + 24 * i;
        SurfaceHit ref; ref.p = Vec3(r[0], r[1], r[2]); ref.p_err = Vec3(r[3], r[4], r[5]); ref.n = Vec3(r[6], r[7], r[8]); ref.time = r[9];
        const Vec3 wi(r[10], r[11], r[12]); const Vec2 u(r[13], r[14]);
        const LiSample ls = L.sample_incident_radiance(ref, u);
        Spectrum le(0.0f);
        if (L.kind == Light::INFINITE) { Ray ray; ray.origin = ref.p; ray.dir = wi; le = L.environment_emitted_radiance(ray); }
        else if (L.kind == Light::AREA) le = L.area_emitted_radiance(ls.p1, -ls.wi);
        o[0] = ls.radiance[0]; o[1] = ls.radiance[1]; o[2] = ls.radiance[2]; o[3] = ls.wi.x; o[4] = ls.wi.y; o[5] = ls.wi.z; o[6] = ls.pdf;
        o[7] = ls.p1.p.x; o[8] = ls.p1.p.y; o[9] = ls.p1.p.z; o[10] = ls.p1.p_err.x; o[11] = ls.p1.p_err.y; o[12] = ls.p1.p_err.z;
        o[13] = ls.p1.n.x; o[14] = ls.p1.n.y; o[15] = ls.p1.n.z; o[16] = ls.p1.time;
        o[17] = L.pdf_incident_radiance(ref, wi); o[18] = L.pdf_incident_radiance(ref, ls.wi);
        o[19] = le[0]; o[20] = le[1]; o[21] = le[2]; o[22] = 0.0f; o[23] = 0.0f;
    }
    return FTN_OK;
}
// ---- surface interactions and cameras: the twins of ftn_test_interaction / ftn_test_camera (fountain_hip.h has the row layouts)
int orc_test_interaction(const orc_scene* s, const float* in32, size_t n, float* out68) {
    if (!s || !in32 || !out68) return fail(FTN_ERR_INVALID_ARGUMENT, "null argument");
    const std::vector<Primitive>& prims = s->data.bvh.prims;
    for (size_t i = 0; i < n; i++) { uint32_t prim; memcpy(&prim, in32 + 32 * i + 8, 4); if (prim >= prims.size()) return fail(FTN_ERR_INVALID_ARGUMENT, "primitive index out of range"); }
    for (size_t i = 0; i < n; i++) {
        const float* r = in32 + 32 * i; float* o = out68 + 68 * i;
        for (int k = 0; k < 68; k++) o[k] = 0.0f;
        uint32_t prim; memcpy(&prim, r + 8, 4);
        RayDifferential rd; rd.ray = ray_from(r); rd.has_diff = r[9] != 0.0f;
        rd.diff.rx_origin = Vec3(r[10], r[11], r[12]); rd.diff.ry_origin = Vec3(r[13], r[14], r[15]);
        rd.diff.rx_dir = Vec3(r[16], r[17], r[18]); rd.diff.ry_dir = Vec3(r[19], r[20], r[21]);
        const Vec3 wi(r[22], r[23], r[24]); const Float eta = r[25]; const bool reflect = r[26] != 0.0f;
        Float t; SurfaceInteraction si;
        if (!prims[prim].shape->intersect(rd.ray, &t, &si)) continue;
        si.compute_tex_differentials(rd);
        const Ray out = si.hit.spawn_ray(wi);
        const int32_t mat = prims[prim].material, light = prims[prim].light;
        o[0] = 1.0f; o[1] = t; o[2] = si.bary.x; o[3] = si.bary.y; o[4] = si.bary.z;
        const Vec3 a[] = {si.hit.p, si.hit.p_err, si.hit.n};
        for (int k = 0; k < 3; k++) for (int c = 0; c < 3; c++) o[5 + 3 * k + c] = a[k][c];
        o[14] = si.hit.time;
        const Vec3 b[] = {si.wo, si.shading_n, si.shading_geom.dpdu};
        for (int k = 0; k < 3; k++) for (int c = 0; c < 3; c++) o[15 + 3 * k + c] = b[k][c];
        memcpy(o + 24, &mat, 4); memcpy(o + 25, &light, 4);
        o[26] = si.uv.x; o[27] = si.uv.y;
        const Vec3 e[] = {si.geom.dpdu, si.geom.dpdv, si.shading_geom.dndu, si.shading_geom.dndv, si.tex_diffs.dpdx, si.tex_diffs.dpdy};
        for (int k = 0; k < 6; k++) for (int c = 0; c < 3; c++) o[28 + 3 * k + c] = e[k][c];
        o[46] = si.tex_diffs.dudx; o[47] = si.tex_diffs.dvdx; o[48] = si.tex_diffs.dudy; o[49] = si.tex_diffs.dvdy;
        o[50] = out.origin.x; o[51] = out.origin.y; o[52] = out.origin.z; o[53] = out.t_max;
        if (rd.has_diff) {
            const Differential d = specular_differential(reflect, rd.diff, si, wi, eta);
            const Vec3 v[] = {d.rx_origin, d.ry_origin, d.rx_dir, d.ry_dir};
            for (int k = 0; k < 4; k++) for (int c = 0; c < 3; c++) o[54 + 3 * k + c] = v[k][c];
        }
    }
    return FTN_OK;
}
int orc_test_camera(const ftn_camera_desc* cam, uint32_t spp, const float* in8, size_t n, float* out20) {
    if (!cam || !in8 || !out20) return fail(FTN_ERR_INVALID_ARGUMENT, "null argument");
    if (spp == 0) return fail(FTN_ERR_INVALID_ARGUMENT, "samples per pixel must be positive");
    for (size_t i = 0; i < n; i++) {
        float o22[22], t8[2];
        orc_kat_camera_ray_differential(cam, in8 + 8 * i, spp, nullptr, o22);
        orc_kat_camera_ray_full(cam, in8 + 8 * i, t8);
        float* o = out20 + 20 * i;
        for (int k = 0; k < 6; k++) o[k] = o22[k];
        o[6] = t8[0]; o[7] = t8[1];
        // rx_origin rx_dir ry_origin ry_dir -> rx_origin ry_origin rx_dir ry_dir
        for (int c = 0; c < 3; c++) { o[8 + c] = o22[6 + c]; o[11 + c] = o22[12 + c]; o[14 + c] = o22[9 + c]; o[17 + c] = o22[15 + c]; }
    }
    return FTN_OK;
}
// MIPMap::lookup_trilinear_width on an image built by MIPMap::new (custom = 0) or new_custom (custom = 1): rows of {s, t, width}
void orc_kat_mipmap_lookup(uint32_t w, uint32_t h, const float* texels, int wrap, int custom, const float* st_width3, size_t n, float* out3) {
    MIPMap m;
    if (custom) { std::vector<Spectrum> img((size_t)w * h); for (size_t i = 0; i < img.size(); i++) img[i] = Spectrum(texels[3 * i], texels[3 * i + 1], texels[3 * i + 2]); m = MIPMap::make_custom((int)w, (int)h, img, wrap); }
    else m = MIPMap::make((int)w, (int)h, texels, wrap);
    for (size_t i = 0; i < n; i++) { Spectrum c = m.lookup_trilinear_width(Vec2(st_width3[3 * i], st_width3[3 * i + 1]), st_width3[3 * i + 2]); out3[3 * i] = c[0]; out3[3 * i + 1] = c[1]; out3[3 * i + 2] = c[2]; }
}

}  // extern "C"
