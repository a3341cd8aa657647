/*
 * ftn_scene_host.cpp -- scene construction (ftn_scene_create and the entry points around a ftn_scene): validation of the descriptor, the
 * host scene (primitive bounds, the reference's BVH through ftn_bvh_host.h, Scene::new's light list, src/scene/mod.rs:32-49), Distribution2D
 * for environment lights, MIP pyramids, and the flattening of all of it into the HBM layout of ftn_device.h, one step per table family.
 * What a scene keeps resident under which build knob is decided here (SceneKnobs) and pinned by tests/test_scene_residency.py.
 */
#include "ftn_bvh_host.h"
#include "ftn_texture.h"

#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>

using namespace ftn;

static Aabb prim_bounds(const ftn_scene_desc* d, const ftn_prim& p) {
    Aabb b = aabb_empty();
    if (p.shape_kind == FTN_SHAPE_TRIANGLE) {                                      /* Triangle::world_bound triangle.rs:152-158 */
        for (int k = 0; k < 3; k++) { uint32_t v = d->tri_indices[3 * (size_t)p.shape_index + k]; aabb_join_point(b, V3(d->P[3 * v], d->P[3 * v + 1], d->P[3 * v + 2])); }
    } else {                                                                       /* Shape::world_bound default + Bounds3f::transform, shapes/mod.rs:13-15 */
        const ftn_sphere& s = d->spheres[p.shape_index];
        const float lo[3] = {-s.radius, -s.radius, s.z_min}, hi[3] = {s.radius, s.radius, s.z_max};
        for (int c = 0; c < 8; c++) {                                              /* iter_corners order bounds.rs:183-194 */
            V3 q((c & 4) ? hi[0] : lo[0], (c & 2) ? hi[1] : lo[1], (c & 1) ? hi[2] : lo[2]);
            aabb_join_point(b, m4_point(s.object_to_world.m, q));
        }
    }
    return b;
}
static int validate_desc(const ftn_scene_desc* d) {
    if (!d) return fail(FTN_ERR_INVALID_ARGUMENT, "null scene description");
    if ((d->n_prims && !d->prims) || (d->n_triangles && (!d->tri_indices || !d->tri_mesh)) || (d->n_vertices && !d->P) || (d->n_meshes && !d->meshes) ||
        (d->n_spheres && !d->spheres) || (d->n_materials && !d->materials) || (d->n_area_emit && !d->area_emit) || (d->n_lights && !d->lights) || (d->n_envmaps && !d->envmaps))
        return fail(FTN_ERR_INVALID_ARGUMENT, "a count is non-zero but its array is NULL");
    for (uint32_t i = 0; i < d->n_materials; i++) if (d->materials[i].type > FTN_MAT_GLASS) return fail(FTN_ERR_INVALID_ARGUMENT, "unknown material type");
    for (uint32_t i = 0; i < d->n_meshes; i++) {
        if (d->meshes[i].has_normals && !d->N) return fail(FTN_ERR_INVALID_ARGUMENT, "a mesh has normals but N is NULL");
        if (d->meshes[i].has_uvs && !d->UV) return fail(FTN_ERR_INVALID_ARGUMENT, "a mesh has uvs but UV is NULL");
        if (d->meshes[i].has_tangents && !d->S) return fail(FTN_ERR_INVALID_ARGUMENT, "a mesh has tangents but S is NULL");
    }
    for (uint32_t i = 0; i < d->n_envmaps; i++) if (!d->envmaps[i].texels) return fail(FTN_ERR_INVALID_ARGUMENT, "environment map without texels");
    if (d->n_textures && d->textures) {                        /* textures */
        const int nt = (int)d->n_textures, ni = d->images ? (int)d->n_images : 0;
        for (int i = 0; i < nt; i++) {
            const ftn_texture& t = d->textures[i];
            if (t.kind > FTN_TEX_IMAGE) return fail(FTN_ERR_INVALID_ARGUMENT, "unknown texture kind");
            if (t.kind == FTN_TEX_CHECKERBOARD && (t.tex1 < 0 || t.tex1 >= nt || t.tex2 < 0 || t.tex2 >= nt)) return fail(FTN_ERR_INVALID_ARGUMENT, "checkerboard child texture out of range");
            if (t.kind == FTN_TEX_IMAGE && (t.image < 0 || t.image >= ni)) return fail(FTN_ERR_INVALID_ARGUMENT, "image index out of range");
        }
        for (int i = 0; i < ni; i++) { const ftn_image& im = d->images[i]; if (im.width == 0 || im.height == 0 || !im.texels || im.wrap > FTN_WRAP_CLAMP) return fail(FTN_ERR_INVALID_ARGUMENT, "bad image"); }
        if (d->material_textures) for (uint32_t i = 0; i < d->n_materials; i++) { const ftn_material_textures& mt = d->material_textures[i];
            for (int32_t id : {mt.a, mt.b, mt.s0, mt.s1, mt.s2}) if (id >= nt) return fail(FTN_ERR_INVALID_ARGUMENT, "material texture index out of range"); }
    }
    for (uint32_t i = 0; i < d->n_triangles; i++) {
        if (d->tri_mesh[i] >= d->n_meshes) return fail(FTN_ERR_INVALID_ARGUMENT, "triangle mesh id out of range");
        for (int k = 0; k < 3; k++) if (d->tri_indices[3 * (size_t)i + k] >= d->n_vertices) return fail(FTN_ERR_INVALID_ARGUMENT, "vertex index out of range");
    }
    for (uint32_t i = 0; i < d->n_prims; i++) {
        const ftn_prim& p = d->prims[i];
        if (p.shape_kind == FTN_SHAPE_TRIANGLE) { if (p.shape_index >= d->n_triangles) return fail(FTN_ERR_INVALID_ARGUMENT, "triangle index out of range"); }
        else if (p.shape_kind == FTN_SHAPE_SPHERE) { if (p.shape_index >= d->n_spheres) return fail(FTN_ERR_INVALID_ARGUMENT, "sphere index out of range"); }
        else return fail(FTN_ERR_INVALID_ARGUMENT, "unknown shape kind");
        if (p.material >= (int)d->n_materials || p.area_emit >= (int)d->n_area_emit) return fail(FTN_ERR_INVALID_ARGUMENT, "material / area light index out of range");
    }
    for (uint32_t i = 0; i < d->n_envmaps; i++) {
        uint32_t w = d->envmaps[i].width, h = d->envmaps[i].height;
        /* any size: compute_distribution's filter width 1 / max(w, h) puts the lookup at pyramid level floor(log2 max) - log2 max, which is
         * 0 for a power of two (lerp with weight exactly 0 on level 1) and negative otherwise (level 0 alone, mipmap.rs:247-249) -- level 1
         * never contributes, so no pyramid is needed for environment maps (infinite.rs:63-77) */
        if (w == 0 || h == 0) return fail(FTN_ERR_INVALID_ARGUMENT, "environment map without texels");
    }
    for (uint32_t i = 0; i < d->n_lights; i++) {
        if (d->lights[i].type > FTN_LIGHT_INFINITE) return fail(FTN_ERR_INVALID_ARGUMENT, "unknown light type");
        if (d->lights[i].type == FTN_LIGHT_INFINITE && (d->lights[i].envmap < 0 || d->lights[i].envmap >= (int)d->n_envmaps)) return fail(FTN_ERR_INVALID_ARGUMENT, "envmap index out of range");
    }
    return FTN_OK;
}
static int build_host_scene(const ftn_scene_desc* d, HostScene* hs) {
    int rc = validate_desc(d); if (rc) return rc;
    std::vector<Aabb> pb(d->n_prims);
    parallel_for(d->n_prims, [&](size_t i0, size_t i1) { for (size_t i = i0; i < i1; i++) pb[i] = prim_bounds(d, d->prims[i]); });
    hs->world = aabb_empty();
    if (d->n_prims) {
        build_bvh(pb, hs);
        for (int k = 0; k < 3; k++) { hs->world.lo[k] = hs->nodes[0].bmin[k]; hs->world.hi[k] = hs->nodes[0].bmax[k]; }
    }
    /* Scene::new (scene/mod.rs:32-49): explicit lights first, then one area light per emissive primitive in BVH order */
    for (uint32_t i = 0; i < d->n_lights; i++) { hs->light_kind.push_back((int)d->lights[i].type); hs->light_prim.push_back(-1); }
    for (size_t i = 0; i < hs->order.size(); i++) if (d->prims[hs->order[i]].area_emit >= 0) { hs->light_kind.push_back((int)LK_AREA); hs->light_prim.push_back((int)i); }
    return FTN_OK;
}

/* Distribution1D::new (sampling.rs:84-107) into flat arrays */
static float dist1d_build(const float* f, size_t n, float* cdf) {
    cdf[0] = 0.0f;
    for (size_t i = 1; i < n + 1; i++) cdf[i] = cdf[i - 1] + (f[i - 1] / (float)n);
    float integral = cdf[n];
    if (integral == 0.0f) { for (size_t i = 1; i < n + 1; i++) cdf[i] = (float)i / (float)n; }
    else { for (size_t i = 1; i < n + 1; i++) cdf[i] /= integral; }
    return integral;
}

/* ------------------------------------------------------------------ MIPMap::<Spectrum>::new (mipmap.rs:78-145): level 0 = the image, every further
 * level = the previous one shrunk to max(1, w/2) x max(1, h/2) by the `resize` crate's Triangle filter (resize 0.4.3, un-vendored:
 * its published algorithm restated -- DESIGN.md "parity unpinned" note).  Separable: per output sample a coefficient line
 * (support 1.0 scaled by the shrink ratio, taps clamped to the image, normalised); rows first (H1 -> H2, into a transposed f32
 * buffer), then columns (W1 -> W2); plain f32 multiply-adds in tap order. */
namespace {
struct MipLevelHost { uint32_t w, h; std::vector<float> rgb; };
struct TapLine { size_t first; std::vector<float> w; };
static std::vector<TapLine> triangle_taps(size_t n_src, size_t n_dst) {
    const float ratio = (float)n_src / (float)n_dst;
    const float scale = ratio > 1.0f ? ratio : 1.0f;
    const float radius = ceilf(scale);                                        /* support (1.0) * scale */
    std::vector<TapLine> lines(n_dst);
    for (size_t j = 0; j < n_dst; j++) {
        const float centre = ((float)j + 0.5f) * ratio - 0.5f;
        long lo = (long)ceilf(centre - radius), hi = (long)floorf(centre + radius);
        lo = std::min<long>(std::max<long>(lo, 0), (long)n_src - 1); hi = std::min<long>(std::max<long>(hi, 0), (long)n_src - 1);
        float total = 0.0f;
        for (long k = lo; k <= hi; k++) total += fmaxf(1.0f - fabsf(((float)k - centre) / scale), 0.0f);
        lines[j].first = (size_t)lo;
        for (long k = lo; k <= hi; k++) lines[j].w.push_back(fmaxf(1.0f - fabsf(((float)k - centre) / scale), 0.0f) / total);
    }
    return lines;
}
static void shrink_triangle(uint32_t w1, uint32_t h1, uint32_t w2, uint32_t h2, const std::vector<float>& src, std::vector<float>* dst) {
    const std::vector<TapLine> across = triangle_taps(w1, w2), down = triangle_taps(h1, h2);
    std::vector<float> mid((size_t)w1 * h2 * 3);                              /* [x1][y2] */
    for (size_t x = 0; x < w1; x++)
        for (size_t y = 0; y < h2; y++) {
            float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f; const TapLine& L = down[y];
            for (size_t k = 0; k < L.w.size(); k++) { const float* q = &src[((L.first + k) * w1 + x) * 3]; a0 += q[0] * L.w[k]; a1 += q[1] * L.w[k]; a2 += q[2] * L.w[k]; }
            float* o = &mid[(x * h2 + y) * 3]; o[0] = a0; o[1] = a1; o[2] = a2;
        }
    dst->assign((size_t)w2 * h2 * 3, 0.0f);
    for (size_t y = 0; y < h2; y++)
        for (size_t x = 0; x < w2; x++) {
            float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f; const TapLine& L = across[x];
            for (size_t k = 0; k < L.w.size(); k++) { const float* q = &mid[((L.first + k) * h2 + y) * 3]; a0 += q[0] * L.w[k]; a1 += q[1] * L.w[k]; a2 += q[2] * L.w[k]; }
            float* o = &(*dst)[(y * w2 + x) * 3]; o[0] = a0; o[1] = a1; o[2] = a2;
        }
}
static void build_mip_pyramid(uint32_t w, uint32_t h, const float* rgb, std::vector<MipLevelHost>* out) {
    out->clear();
    MipLevelHost l0; l0.w = w; l0.h = h; l0.rgb.assign(rgb, rgb + (size_t)w * h * 3); out->push_back(l0);
    uint32_t big = std::max(w, h); int n_levels = 1; while (big >>= 1) n_levels++;          /* 1 + log2_usize(max(w, h)) */
    for (int l = 1; l < n_levels; l++) {
        const MipLevelHost& prev = out->back();
        MipLevelHost nx; nx.w = std::max<uint32_t>(1, prev.w / 2); nx.h = std::max<uint32_t>(1, prev.h / 2);
        shrink_triangle(prev.w, prev.h, nx.w, nx.h, prev.rgb, &nx.rgb);
        out->push_back(std::move(nx));
    }
}
}  // namespace

/* FTN_SCENE_DEBUG: wall time of the phases of ftn_scene_create on stderr */
struct PhaseClock {
    bool on; std::chrono::steady_clock::time_point t;
    PhaseClock() : on(getenv("FTN_SCENE_DEBUG") != nullptr), t(std::chrono::steady_clock::now()) {}
    void mark(const char* what) {
        if (!on) return;
        const auto n = std::chrono::steady_clock::now();
        fprintf(stderr, "[ftn scene] %-44s %.3f s\n", what, std::chrono::duration<double>(n - t).count()); t = n;
    }
};

namespace {          /* (to the end of upload_scene: the structures below are this unit's alone) */

/* ------------------------------------------------------------------ the build knobs of a scene, read once when it is created.
 * env_is(name, value): the variable is set and its integer value is `value`; an unset variable never matches */
static bool env_is(const char* name, int value) { const char* v = getenv(name); return v && atoi(v) == value; }
struct SceneKnobs {
    /* two-box records (DScene::fat): only the legacy any-hit kernel (k_wf_trace_any2: FTN_TRACE4=0, or a scene without four-box records)
     * reads them: 639 MB at 10 M triangles that a default scene does not allocate.  A scene created without them still renders under
     * FTN_TRACE4=0 (plain node walk).  Built under FTN_TRACE4=0, FTN_QUAD=0 or FTN_FAT=1 */
    bool trace4_off = env_is("FTN_TRACE4", 0), fat_on = env_is("FTN_FAT", 1);
    /* FTN_QUAD=0: no four-box records (DScene::quad; the two-record kernels run), and none of the trees made from them */
    bool quad_off = env_is("FTN_QUAD", 0);
    /* FTN_QUAD64=0: no 64-byte four-box records (DScene::quad64) */
    bool quad64_off = env_is("FTN_QUAD64", 0);
    /* FTN_OCT=0: no eight-box occlusion records (DScene::oct; the four-box any-hit kernel traces the shadow rays) */
    bool oct_off = env_is("FTN_OCT", 0);
    /* FTN_SREC=0: no shading records (DScene::srec) */
    bool srec_off = env_is("FTN_SREC", 0);
    /* FTN_GEOM=1: the dense leaf-test array stays resident beside the shading records */
    bool geom_on = env_is("FTN_GEOM", 1);
    /* FTN_LEGACY_ARRAYS=1: prim_info and the per-vertex normals / uvs stay resident beside the shading records */
    bool legacy_arrays_on = env_is("FTN_LEGACY_ARRAYS", 1);
    /* FTN_ENV_CELLS=0: no cell records for square environment maps (DLight::cells) */
    bool env_cells_off = env_is("FTN_ENV_CELLS", 0);
    /* FTN_NO_COARSE_CDF, set to anything: no coarse CDF tables (DLight::cond_coarse / marg_coarse) */
    bool no_coarse_cdf = getenv("FTN_NO_COARSE_CDF") != nullptr;
    bool want_fat() const { return trace4_off || quad_off || fat_on; }
};

/* what the steps of upload_scene share: the descriptor, the scene with its host BVH, the knobs, the host tables later steps read again,
 * and the counts the DScene reports */
struct Upload {
    const ftn_scene_desc* d; ftn_scene* sc; const HostScene& hs; const SceneKnobs& knobs; size_t np;
    std::vector<float4> geom; std::vector<uint4> info; std::vector<uint8_t> leaf_end;     /* per primitive in BVH order: leaf-test records, prim_info, last of its leaf */
    std::vector<ftn_material> mats; std::vector<DLight> lights; std::vector<uint32_t> inf;
    uint32_t n_fat = 0, n_quads = 0, quad_bound = 0, n_quad64 = 0, quad64_bound = 0, n_octs = 0, oct_bound = 0;
    bool geom_in_srec = false, has_tex = false, null_prims = false;      /* null_prims: some primitive has shading class 7 (prim_classes) */
    Upload(const ftn_scene_desc* d_, ftn_scene* sc_, const SceneKnobs& k) : d(d_), sc(sc_), hs(sc_->host), knobs(k), np(sc_->host.order.size()) {}
};

/* a table of the scene's that has no member of its own (the tables of an environment light): it belongs to the scene from the moment it is
 * allocated, so a scene that fails later frees it */
template <class T> static int held_table(std::vector<DevBuf<T>>& held, const T* src, size_t n, const T** p) {
    held.emplace_back();
    const int rc = held.back().upload(src, n);
    *p = held.back().p;
    return rc;
}

static int node_records(const Upload& U, std::vector<float4>* out) {
    const HostScene& hs = U.hs;
    std::vector<float4>& nodes = *out;
    nodes.resize(2 * hs.nodes.size());
    parallel_for(hs.nodes.size(), [&](size_t i0, size_t i1) { for (size_t i = i0; i < i1; i++) {
        const ftn_bvh_node& n = hs.nodes[i];
        /* slab pairs first: the x and y (min, max) pairs, then the z pair with the two index words (see ftn_device.h) */
        nodes[2 * i] = make_float4(n.bmin[0], n.bmax[0], n.bmin[1], n.bmax[1]);
        /* interior: byte offset of the second child (the first child is the next record: +32); leaf: first primitive.
         * meta: n_prims | one-hot split axis << 16 (matches the ray's dir_is_neg bits) | leaf << 24 */
        const uint32_t link = n.is_leaf ? n.idx : n.idx * 32u;
        nodes[2 * i + 1] = make_float4(n.bmin[2], n.bmax[2], ftn_det::u2f(link), ftn_det::u2f((uint32_t)n.n_prims | ((1u << n.axis) << 16) | ((uint32_t)n.is_leaf << 24)));
    } });
    if (hs.nodes.size() >= (1u << 27)) return fail(FTN_ERR_UNSUPPORTED, "more than 2^27 BVH nodes (node links are 32-bit byte offsets)");
    return FTN_OK;
}

/* two-box records (see DScene::fat): one per interior node, numbered in DFS order -- and, on the same walk, which primitive ends its leaf */
static void two_box_records(Upload& U, std::vector<float4>* out) {
    const HostScene& hs = U.hs;
    const bool want_fat = U.knobs.want_fat();
    std::vector<uint32_t> fat_id(want_fat ? hs.nodes.size() : 0, 0xffffffffu);
    uint32_t n_fat = 0;
    if (want_fat) for (size_t i = 0; i < hs.nodes.size(); i++) if (!hs.nodes[i].is_leaf) fat_id[i] = n_fat++;
    std::vector<float4>& fat = *out;
    fat.resize(4 * (size_t)n_fat);
    U.leaf_end.assign(U.np, 0);
    for (size_t i = 0; i < hs.nodes.size(); i++) {
        const ftn_bvh_node& n = hs.nodes[i];
        if (n.is_leaf) { if (n.n_prims) U.leaf_end[n.idx + n.n_prims - 1] = 1; continue; }
        if (!want_fat) continue;
        const size_t ch[2] = {i + 1, (size_t)n.idx};
        for (int k = 0; k < 2; k++) {                            /* the two children's node records side by side (same layout as `nodes`) */
            const ftn_bvh_node& c = hs.nodes[ch[k]];
            const uint32_t link = c.is_leaf ? c.idx : fat_id[ch[k]] * 64u;            /* byte offset of the child's own two-box record, or first primitive */
            const uint32_t meta = (uint32_t)c.n_prims | (k == 0 ? ((1u << n.axis) << 16) : 0u) | ((uint32_t)c.is_leaf << 24);   /* record 0 carries THIS node's split axis */
            fat[4 * (size_t)fat_id[i] + 2 * k] = make_float4(c.bmin[0], c.bmax[0], c.bmin[1], c.bmax[1]);
            fat[4 * (size_t)fat_id[i] + 2 * k + 1] = make_float4(c.bmin[2], c.bmax[2], ftn_det::u2f(link), ftn_det::u2f(meta));
        }
    }
    U.n_fat = n_fat;
}

/* leaf-test records (DScene::geom) and prim_info, per primitive in BVH order */
static void leaf_test_records(Upload& U) {
    const ftn_scene_desc* d = U.d; const HostScene& hs = U.hs; const size_t np = U.np;
    const std::vector<uint8_t>& leaf_end = U.leaf_end;
    std::vector<int> prim_light(np, -1);
    for (size_t l = 0; l < hs.light_prim.size(); l++) if (hs.light_prim[l] >= 0) prim_light[hs.light_prim[l]] = (int)l;
    std::vector<float4>& geom = U.geom; std::vector<uint4>& info = U.info;
    geom.resize((size_t)FTN_GS * np); info.resize(2 * np);
    parallel_for(np, [&](size_t i0, size_t i1) { for (size_t i = i0; i < i1; i++) {
        const ftn_prim& p = d->prims[hs.order[i]];
        uint32_t fl = 0;
        if (p.shape_kind == FTN_SHAPE_SPHERE) {
            fl = GF_KIND_SPHERE | (leaf_end[i] ? GF_LEAF_END : 0u);
            geom[FTN_GS * i] = make_float4(0, 0, 0, ftn_det::u2f(fl)); geom[FTN_GS * i + 1] = make_float4(0, 0, 0, ftn_det::u2f(p.shape_index)); geom[FTN_GS * i + 2] = make_float4(0, 0, 0, 0);
            info[2 * i + 1] = make_uint4(0, 0, 0, p.shape_index);
        } else {
            const ftn_mesh& m = d->meshes[d->tri_mesh[p.shape_index]];
            if (m.has_normals && d->N) fl |= GF_HAS_NORMALS;
            if (m.has_uvs && d->UV) fl |= GF_HAS_UVS;
            if (m.has_tangents && d->S) fl |= GF_HAS_TANGENTS;
            if (m.flip_normals) fl |= GF_FLIP;
            if (leaf_end[i]) fl |= GF_LEAF_END;
            const uint32_t* vi = d->tri_indices + 3 * (size_t)p.shape_index;
            const float* P = d->P;
            geom[FTN_GS * i] = make_float4(P[3 * vi[0]], P[3 * vi[0] + 1], P[3 * vi[0] + 2], ftn_det::u2f(fl));
            geom[FTN_GS * i + 1] = make_float4(P[3 * vi[1]], P[3 * vi[1] + 1], P[3 * vi[1] + 2], ftn_det::u2f(p.shape_index));
            geom[FTN_GS * i + 2] = make_float4(P[3 * vi[2]], P[3 * vi[2] + 1], P[3 * vi[2] + 2], 0.0f);
            info[2 * i + 1] = make_uint4(vi[0], vi[1], vi[2], p.shape_index);
        }
        info[2 * i] = make_uint4((uint32_t)p.material, (uint32_t)prim_light[i], fl, 0);
    } });
}

/* the record trees over the same nodes, each built and uploaded before the next one is built */
static int record_trees(Upload& U, PhaseClock& clk) {
    const ftn_scene_desc* d = U.d; ftn_scene* sc = U.sc; const HostScene& hs = U.hs;
    int rc;
    /* four-box records (DScene::quad): what the production traversal kernels walk */
    QuadBvh qb;
    if (!U.knobs.quad_off) {
        build_quads(hs.nodes, &qb);
        if (qb.ok && qb.n_records) {
            if ((rc = sc->quad.upload(reinterpret_cast<const float4*>(qb.rec.data()), (size_t)8 * qb.n_records))) return rc;
            U.n_quads = qb.n_records; U.quad_bound = qb.stack_bound;
        }
    }
    clk.mark("four-box records (host + upload)");
    /* 64-byte four-box records (DScene::quad64): the closest-hit walk of triangle-only scenes.  The 128-byte records stay resident: the
     * any-hit kernels of FTN_T8=0, scenes with spheres and the FTN_QUAD64=0 A/B at render time walk them */
    if (!U.knobs.quad64_off && U.n_quads != 0 && d->n_spheres == 0) {
        Quad64Bvh q6; build_quad64s(qb, U.geom, &q6);
        if (q6.ok && q6.n_records) {
            if ((rc = sc->quad64.upload(reinterpret_cast<const uint4*>(q6.rec.data()), (size_t)4 * q6.n_records))) return rc;
            if (!q6.xbox.empty() && (rc = sc->quad64_xbox.upload(q6.xbox.data(), q6.xbox.size()))) return rc;
            U.n_quad64 = q6.n_records; U.quad64_bound = q6.stack_bound;
        }
    }
    qb = QuadBvh();
    clk.mark("64-byte four-box records (host + upload)");
    /* eight-box occlusion records (DScene::oct): triangle-only scenes with four-box records (the kernel hands its exceptional rays to the
     * same fallback) */
    if (!U.knobs.oct_off && U.n_quads != 0 && d->n_spheres == 0) {
        OctBvh ob; build_octs(hs.nodes, U.geom, &ob);
        if (ob.ok && ob.n_records) {
            if ((rc = sc->oct.upload(reinterpret_cast<const uint4*>(ob.rec.data()), (size_t)8 * ob.n_records))) return rc;
            if (!ob.xbox.empty() && (rc = sc->oct_xbox.upload(ob.xbox.data(), ob.xbox.size()))) return rc;
            U.n_octs = ob.n_records; U.oct_bound = ob.stack_bound;
        }
    }
    clk.mark("eight-box records (host + upload)");
    return FTN_OK;
}

/* shading records (DScene::srec): one 128-byte line per primitive with everything make_interaction reads.
 * (Building these three arrays on a worker while this thread uploads the previous one was measured: no faster -- the pageable
 * host-to-device copies and the builders want the same memory bandwidth.) */
static int shading_records(Upload& U) {
    const ftn_scene_desc* d = U.d; const size_t np = U.np;
    const std::vector<float4>& geom = U.geom; const std::vector<uint4>& info = U.info;
    if (U.knobs.srec_off || np == 0 || (uint64_t)np * 128u > (16ull << 30)) return FTN_OK;
    std::unique_ptr<float4[]> rec(new float4[8 * np]);          /* (not value-initialised: every word is written below) */
    parallel_for(np, [&](size_t i0, size_t i1) { for (size_t i = i0; i < i1; i++) {
        float4* R = &rec[8 * i];
        for (int k = 3; k < 8; k++) R[k] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        const uint4 pi = info[2 * i], vi = info[2 * i + 1];
        R[0] = geom[FTN_GS * i]; R[1] = geom[FTN_GS * i + 1]; R[2] = geom[FTN_GS * i + 2];
        R[1].w = ftn_det::u2f(pi.x); R[2].w = ftn_det::u2f(pi.y); R[6].w = ftn_det::u2f(vi.w);
        const uint32_t fl = ftn_det::f2u(R[0].w);
        if (fl & GF_KIND_SPHERE) continue;
        const uint32_t v[3] = {vi.x, vi.y, vi.z};
        if (fl & GF_HAS_NORMALS) for (int k = 0; k < 3; k++) { R[3 + k].x = d->N[3 * (size_t)v[k]]; R[3 + k].y = d->N[3 * (size_t)v[k] + 1]; R[3 + k].z = d->N[3 * (size_t)v[k] + 2]; }
        if (fl & GF_HAS_UVS) {
            R[3].w = d->UV[2 * (size_t)v[0]]; R[4].w = d->UV[2 * (size_t)v[0] + 1]; R[5].w = d->UV[2 * (size_t)v[1]];
            R[6].x = d->UV[2 * (size_t)v[1] + 1]; R[6].y = d->UV[2 * (size_t)v[2]]; R[6].z = d->UV[2 * (size_t)v[2] + 1];
        }
    } });
    return U.sc->srec.upload(rec.get(), 8 * np);
}

/* the dense leaf-test array, prim_info and the per-vertex arrays: what the shading records replace */
static int attribute_arrays(Upload& U) {
    const ftn_scene_desc* d = U.d; ftn_scene* sc = U.sc;
    int rc;
    /* leaf-test records: the shading records' first 48 bytes in triangle-only scenes (DScene::geom_stride = 8), the dense array otherwise */
    U.geom_in_srec = sc->srec.p != nullptr && d->n_spheres == 0 && !U.knobs.geom_on;
    if (!U.geom_in_srec && (rc = sc->geom.upload(U.geom.data(), U.geom.size()))) return rc;
    /* prim_info and the per-vertex normals / uvs: what the shading records replace (ftn_device.h: prim_mat_light / prim_normals / prim_uvs).
     * Resident only without records, or when a mesh has shading tangents (gathered through prim_info's vertex indices) */
    bool any_tangents = false;
    for (uint32_t i = 0; i < d->n_meshes; i++) if (d->meshes[i].has_tangents && d->S) any_tangents = true;
    if (!sc->srec.p || any_tangents || U.knobs.legacy_arrays_on) {
        if ((rc = sc->prim_info.upload(U.info.data(), U.info.size()))) return rc;
        if (d->N && (rc = sc->N.upload(d->N, 3 * (size_t)d->n_vertices))) return rc;
        if (d->UV && (rc = sc->UV.upload(d->UV, 2 * (size_t)d->n_vertices))) return rc;
    }
    if (any_tangents && (rc = sc->T.upload(d->S, 3 * (size_t)d->n_vertices))) return rc;
    return FTN_OK;
}

static int spheres_and_materials(Upload& U) {
    const ftn_scene_desc* d = U.d; ftn_scene* sc = U.sc;
    int rc;
    std::vector<DSphere> sph(d->n_spheres);
    for (uint32_t i = 0; i < d->n_spheres; i++) {
        const ftn_sphere& s = d->spheres[i]; DSphere& o = sph[i];
        memcpy(o.o2w, s.object_to_world.m, 64); memcpy(o.o2w_inv, s.object_to_world.inv, 64); memcpy(o.w2o, s.world_to_object.m, 64);
        o.radius = s.radius; o.z_min = s.z_min; o.z_max = s.z_max; o.theta_min = s.theta_min; o.theta_max = s.theta_max; o.phi_max = s.phi_max;
        o.reverse_orientation = s.reverse_orientation; o._pad = 0;
    }
    if ((rc = sc->spheres.upload(sph.data(), sph.size()))) return rc;
    /* materials: evaluate the constant-per-material parts of compute_scattering_functions once (textured materials stay raw and are
     * finalized per hit by material_resolve, ftn_texture.h) */
    U.mats.assign(d->materials, d->materials + d->n_materials);
    U.has_tex = d->n_textures != 0 && d->textures != nullptr;
    for (size_t i = 0; i < U.mats.size(); i++) {
        bool textured = false;
        if (U.has_tex && d->material_textures) { const ftn_material_textures& mt = d->material_textures[i]; textured = (mt.a & mt.b & mt.s0 & mt.s1 & mt.s2) >= 0; }
        if (!textured) material_finalize(U.mats[i]);
    }
    return sc->materials.upload(U.mats.data(), U.mats.size());
}

/* shading class per primitive (DScene::prim_class) */
static int prim_classes(Upload& U) {
    std::vector<unsigned char> cls(U.np);
    for (size_t i = 0; i < U.np; i++) { const int m = (int)U.info[2 * i].x; cls[i] = (unsigned char)(m < 0 || (size_t)m >= U.mats.size() ? 7u : std::min<uint32_t>(2u + U.mats[(size_t)m].type, 7u)); }
    U.null_prims = false;
    for (const unsigned char c : cls) if (c == 7u) U.null_prims = true;
    return U.sc->prim_class.upload(cls.data(), cls.size());
}

/* the tables of one infinite light: texels, Distribution2D (compute_distribution, infinite.rs:63-78), cell records, coarse CDFs */
struct EnvTables { std::vector<float4> tex4; std::vector<float> img, ccdf, cint, mcdf; uint32_t nu = 0, nv = 0; };

static void env_distribution(const ftn_envmap& e, DLight& L, EnvTables* T) {
    /* compute_distribution infinite.rs:63-78: (height, width) = resolution() name swap (the distribution of a w x h map has h columns and
     * w rows, its rows filled from texture rows as if the map were h wide: reproduced as written); only pyramid level 0 is ever read */
    const uint32_t height = e.width, width = e.height;
    T->tex4.resize((size_t)e.width * e.height);
    for (size_t k = 0; k < T->tex4.size(); k++) T->tex4[k] = make_float4(e.texels[3 * k], e.texels[3 * k + 1], e.texels[3 * k + 2], 0.0f);
    DLight hostL = L; hostL.texels = T->tex4.data();
    std::vector<float>& img = T->img;
    img.resize((size_t)width * height);
    for (uint32_t j = 0; j < height; j++) {
        float v = (float)j / (float)height;
        float sin_theta = ftn_det::sinf_det(FTN_PI * ((float)j + 0.5f) / (float)height);
        for (uint32_t i = 0; i < width; i++) {
            float u = (float)i / (float)width;
            Rgb tex = (e.width == 1 && e.height == 1) ? env_texel(hostL, 0, 0) : env_lookup(hostL, V2(u, v));
            img[i + (size_t)j * width] = tex.luminance() * sin_theta;
        }
    }
    const uint32_t nu = width, nv = height;
    T->ccdf.resize((size_t)nv * (nu + 1)); T->cint.resize(nv); T->mcdf.resize(nv + 1);
    for (uint32_t v2 = 0; v2 < nv; v2++) T->cint[v2] = dist1d_build(&img[(size_t)v2 * nu], nu, &T->ccdf[(size_t)v2 * (nu + 1)]);
    float mint = dist1d_build(T->cint.data(), nv, T->mcdf.data());
    T->nu = nu; T->nv = nv;
    L.nu = nu; L.nv = nv; L.marg_integral = mint;
}

/* cell records (DLight::cells): square maps only -- compute_distribution's (height, width) swap makes the distribution's cell
 * (u, v) the texel (u, v) only then */
static int env_cells(Upload& U, const ftn_envmap& e, const EnvTables& T, DLight& L) {
    if (!(e.width == e.height && (uint64_t)e.width * e.height * 128u <= (2ull << 30) && !U.knobs.env_cells_off)) return FTN_OK;
    const int w = (int)e.width, h = (int)e.height;
    const uint32_t width = e.height;
    std::unique_ptr<float4[]> cells(new float4[8 * (size_t)w * h]);
    parallel_for((size_t)h, [&](size_t y0, size_t y1) { for (size_t cy = y0; cy < y1; cy++) for (int cx = 0; cx < w; cx++) {
        float* c = reinterpret_cast<float*>(&cells[8 * (cy * (size_t)w + (size_t)cx)]);
        for (int dy = -1; dy <= 1; dy++) for (int dx = -1; dx <= 1; dx++) {
            const int sx = ((cx + dx) % w + w) % w, sy = (((int)cy + dy) % h + h) % h;        /* env_texel's wrap */
            const float4 t = T.tex4[(size_t)sy * w + sx];
            float* o = c + 3 * ((dy + 1) * 3 + dx + 1);
            o[0] = t.x; o[1] = t.y; o[2] = t.z;
        }
        c[27] = T.img[(size_t)cx + cy * (size_t)width];
        c[28] = c[29] = c[30] = c[31] = 0.0f;
    } });
    return held_table<float4>(U.sc->misc4, cells.get(), 8 * (size_t)w * h, &L.cells);
}

/* every 32nd CDF entry (DLight::cond_coarse / marg_coarse); only for CDFs that really are non-decreasing */
static int env_coarse_cdfs(Upload& U, const EnvTables& T, DLight& L) {
    const uint32_t nu = T.nu, nv = T.nv;
    bool monotone = true;
    auto check = [&](const float* c, uint32_t n) { for (uint32_t k = 0; k < n; k++) if (!(c[k] <= c[k + 1])) monotone = false; };
    for (uint32_t v2 = 0; v2 < nv; v2++) check(&T.ccdf[(size_t)v2 * (nu + 1)], nu);
    check(T.mcdf.data(), nv);
    if (!monotone || U.knobs.no_coarse_cdf) return FTN_OK;
    const uint32_t nbu = (nu + 31u) / 32u, nbv = (nv + 31u) / 32u;
    std::vector<float> cc((size_t)nv * (nbu + 1)), mc(nbv + 1);
    for (uint32_t v2 = 0; v2 < nv; v2++) for (uint32_t k = 0; k <= nbu; k++) cc[(size_t)v2 * (nbu + 1) + k] = T.ccdf[(size_t)v2 * (nu + 1) + std::min(k * 32u, nu)];
    for (uint32_t k = 0; k <= nbv; k++) mc[k] = T.mcdf[std::min(k * 32u, nv)];
    int rc;
    if ((rc = held_table(U.sc->misc, cc.data(), cc.size(), &L.cond_coarse))) return rc;
    return held_table(U.sc->misc, mc.data(), mc.size(), &L.marg_coarse);
}

static int env_light_tables(Upload& U, const ftn_light& src, DLight& L) {
    const ftn_envmap& e = U.d->envmaps[src.envmap];
    memcpy(L.l2w, src.light_to_world.m, 64); memcpy(L.w2l, src.light_to_world.inv, 64);
    L.env_w = e.width; L.env_h = e.height;
    EnvTables T; env_distribution(e, L, &T);
    std::vector<DevBuf<float>>& misc = U.sc->misc;
    int rc;
    if ((rc = held_table<float4>(U.sc->misc4, T.tex4.data(), T.tex4.size(), &L.texels))) return rc;
    if ((rc = held_table(misc, T.img.data(), T.img.size(), &L.cond_func))) return rc;
    if ((rc = held_table(misc, T.ccdf.data(), T.ccdf.size(), &L.cond_cdf))) return rc;
    if ((rc = held_table(misc, T.cint.data(), T.cint.size(), &L.cond_integral))) return rc;
    if ((rc = held_table(misc, T.cint.data(), T.cint.size(), &L.marg_func))) return rc;            /* marginal func == conditional integrals */
    if ((rc = held_table(misc, T.mcdf.data(), T.mcdf.size(), &L.marg_cdf))) return rc;
    if ((rc = env_cells(U, e, T, L))) return rc;
    return env_coarse_cdfs(U, T, L);
}

static int light_records(Upload& U) {
    const ftn_scene_desc* d = U.d; const HostScene& hs = U.hs;
    std::vector<DLight>& lights = U.lights;
    lights.resize(hs.light_kind.size());
    V3 wc((hs.world.lo[0] + hs.world.hi[0]) / 2.0f, (hs.world.lo[1] + hs.world.hi[1]) / 2.0f, (hs.world.lo[2] + hs.world.hi[2]) / 2.0f);   /* bounding_sphere bounds.rs:208-212 */
    wc = V3(0.0f, 0.0f, 0.0f) + wc;
    float wr = len(wc - V3(hs.world.hi[0], hs.world.hi[1], hs.world.hi[2]));
    int rc;
    for (size_t l = 0; l < lights.size(); l++) {
        DLight& L = lights[l]; memset(&L, 0, sizeof(L));
        L.kind = (uint32_t)hs.light_kind[l]; L.prim = hs.light_prim[l];
        if (L.kind == LK_AREA) {
            const ftn_prim& p = d->prims[hs.order[L.prim]];
            for (int k = 0; k < 3; k++) L.rgb[k] = d->area_emit[3 * p.area_emit + k];
            if (p.shape_kind == FTN_SHAPE_SPHERE) { const ftn_sphere& s = d->spheres[p.shape_index]; L.area = s.phi_max * s.radius * (s.z_max - s.z_min); }   /* sphere.rs:77-79 */
            else {                                                                /* triangle.rs:171-174 */
                const uint32_t* vi = d->tri_indices + 3 * (size_t)p.shape_index; const float* P = d->P;
                V3 p0(P[3 * vi[0]], P[3 * vi[0] + 1], P[3 * vi[0] + 2]), p1(P[3 * vi[1]], P[3 * vi[1] + 1], P[3 * vi[1] + 2]), p2(P[3 * vi[2]], P[3 * vi[2] + 1], P[3 * vi[2] + 2]);
                L.area = 0.5f * len(cross(p1 - p0, p2 - p0));
            }
            continue;
        }
        const ftn_light& src = d->lights[l];
        for (int k = 0; k < 3; k++) { L.rgb[k] = src.rgb[k]; L.v[k] = src.v[k]; }
        if (L.kind == LK_DISTANT || L.kind == LK_INFINITE) { L.world_center[0] = wc.x; L.world_center[1] = wc.y; L.world_center[2] = wc.z; L.world_radius = wr; }   /* preprocess */
        if (L.kind == LK_INFINITE) {
            U.inf.push_back((uint32_t)l);
            if ((rc = env_light_tables(U, src, L))) return rc;
        }
    }
    if ((rc = U.sc->lights.upload(lights.data(), lights.size()))) return rc;
    return U.sc->inf_lights.upload(U.inf.data(), U.inf.size());
}

static void fill_dscene(Upload& U) {
    ftn_scene* sc = U.sc; const HostScene& hs = U.hs;
    DScene& D = sc->d; memset(&D, 0, sizeof(D));
    D.nodes = sc->nodes.p; D.geom = U.geom_in_srec ? sc->srec.p : sc->geom.p; D.geom_stride = U.geom_in_srec ? 8u : (uint32_t)FTN_GS; D.prim_info = sc->prim_info.p; D.N = sc->N.p; D.UV = sc->UV.p; D.T = sc->T.p; D.spheres = sc->spheres.p;
    D.materials = sc->materials.p; D.lights = sc->lights.p; D.inf_lights = sc->inf_lights.p;
    D.n_nodes = (uint32_t)hs.nodes.size(); D.n_prims = (uint32_t)U.np; D.n_lights = (uint32_t)U.lights.size(); D.n_inf_lights = (uint32_t)U.inf.size(); D.n_spheres = U.d->n_spheres;
    D.srec = sc->srec.p; D.prim_class = sc->prim_class.p; D.null_prims = U.null_prims ? 1u : 0u;
    D.quad = sc->quad.p; D.n_quads = U.n_quads; D.quad_stack_bound = U.quad_bound;
    D.oct = sc->oct.p; D.oct_xbox = sc->oct_xbox.p; D.n_octs = U.n_octs; D.oct_stack_bound = U.oct_bound;
    D.quad64 = sc->quad64.p; D.quad64_xbox = sc->quad64_xbox.p; D.n_quad64 = U.n_quad64; D.quad64_stack_bound = U.quad64_bound;
    D.fat = sc->fat.p; D.n_fat = U.n_fat; D.root_is_leaf = (!hs.nodes.empty() && hs.nodes[0].is_leaf) ? 1u : 0u;
    for (int k = 0; k < 3; k++) { D.root_lo[k] = hs.nodes.empty() ? 0.0f : hs.nodes[0].bmin[k]; D.root_hi[k] = hs.nodes.empty() ? 0.0f : hs.nodes[0].bmax[k]; }
    if (U.lights.size() == 1 && U.lights[0].kind == LK_INFINITE) { D.env_only = 1; D.env0 = U.lights[0]; }
    sc->stack_entries = std::max<uint32_t>(hs.max_depth, 1u);
    for (const ftn_material& m : U.mats) if (m.type < 32u) D.material_types |= 1u << m.type;
}

/* textures + MIP pyramids; validate_desc has checked every index */
static int textures_and_pyramids(Upload& U) {
    const ftn_scene_desc* d = U.d; ftn_scene* sc = U.sc;
    if (!U.has_tex) return FTN_OK;
    const int nt = (int)d->n_textures, ni = d->images ? (int)d->n_images : 0;
    std::vector<ftn_material_textures> mt(d->n_materials);
    for (uint32_t i = 0; i < d->n_materials; i++) {
        if (d->material_textures) mt[i] = d->material_textures[i]; else { mt[i].a = mt[i].b = mt[i].s0 = mt[i].s1 = mt[i].s2 = -1; }
    }
    std::vector<DImage> imgs((size_t)ni); std::vector<float4> texels;
    for (int i = 0; i < ni; i++) {
        const ftn_image& im = d->images[i];
        std::vector<MipLevelHost> pyr; build_mip_pyramid(im.width, im.height, im.texels, &pyr);
        if (pyr.size() > 16) return fail(FTN_ERR_UNSUPPORTED, "image larger than 32768 texels on a side");
        DImage& D2 = imgs[(size_t)i]; memset(&D2, 0, sizeof(D2));
        D2.w = im.width; D2.h = im.height; D2.wrap = im.wrap; D2.n_levels = (uint32_t)pyr.size();
        for (size_t l = 0; l < pyr.size(); l++) {
            D2.off[l] = (uint32_t)texels.size(); D2.lw[l] = pyr[l].w; D2.lh[l] = pyr[l].h;
            for (size_t k = 0; k < (size_t)pyr[l].w * pyr[l].h; k++) texels.push_back(make_float4(pyr[l].rgb[3 * k], pyr[l].rgb[3 * k + 1], pyr[l].rgb[3 * k + 2], 0.0f));
        }
    }
    int rc;
    if ((rc = sc->textures.upload(d->textures, (size_t)nt)) || (rc = sc->mtex.upload(mt.data(), mt.size())) || (rc = sc->images.upload(imgs.data(), imgs.size())) ||
        (rc = sc->texels.upload(texels.data(), texels.size()))) return rc;
    DScene& D = sc->d;
    D.textures = sc->textures.p; D.mtex = sc->mtex.p; D.images = sc->images.p; D.texels = sc->texels.p; D.n_textures = (uint32_t)nt;
    return FTN_OK;
}

/* the scene's tables, each family built on the host and uploaded before the next is built: at 10 M triangles the host copies of the
 * record trees and of the shading records are freed again before the next one is made */
static int upload_scene(const ftn_scene_desc* d, const SceneKnobs& knobs, ftn_scene* sc) {
    Upload U(d, sc, knobs);
    PhaseClock clk;
    int rc;
    std::vector<float4> nodes, fat;
    if ((rc = node_records(U, &nodes))) return rc;
    two_box_records(U, &fat);
    leaf_test_records(U);
    clk.mark("node records, leaf-test records (host)");
    if ((rc = sc->nodes.upload(nodes.data(), nodes.size()))) return rc;
    clk.mark("upload nodes");
    /* two-box record links are 31-bit byte offsets: beyond 2^25 interior nodes the any-hit kernel falls back to the plain node walk */
    if (U.n_fat && U.n_fat < (1u << 25)) { if ((rc = sc->fat.upload(fat.data(), fat.size()))) return rc; }
    if ((rc = record_trees(U, clk))) return rc;
    if ((rc = shading_records(U))) return rc;
    clk.mark("shading records (host + upload)");
    if ((rc = attribute_arrays(U))) return rc;
    if ((rc = spheres_and_materials(U))) return rc;
    clk.mark("leaf-test / attribute arrays, spheres, materials");
    if ((rc = prim_classes(U))) return rc;
    if ((rc = light_records(U))) return rc;
    clk.mark("classes, lights, environment tables, textures");
    fill_dscene(U);
    if ((rc = sc->stats.alloc_zero(1))) return rc;
    return textures_and_pyramids(U);
}

}  // namespace

extern "C" {

int ftn_bvh_build(const ftn_scene_desc* d, ftn_bvh_node* nodes_out, uint32_t* order_out, uint32_t* n_nodes_out, uint32_t* max_depth_out) {
    HostScene hs; int rc = build_host_scene(d, &hs); if (rc) return rc;
    if (nodes_out) memcpy(nodes_out, hs.nodes.data(), hs.nodes.size() * sizeof(ftn_bvh_node));
    if (order_out) memcpy(order_out, hs.order.data(), hs.order.size() * sizeof(uint32_t));
    if (n_nodes_out) *n_nodes_out = (uint32_t)hs.nodes.size();
    if (max_depth_out) *max_depth_out = hs.max_depth;
    return FTN_OK;
}

int ftn_scene_create(const ftn_scene_desc* d, int device, ftn_scene** out) {
    if (!out) return fail(FTN_ERR_INVALID_ARGUMENT, "null output");
    int rc = set_device(device); if (rc) return rc;
    ftn_scene* sc = new ftn_scene();
    sc->device = device;
    const SceneKnobs knobs;
    PhaseClock clk;
    rc = build_host_scene(d, &sc->host);
    clk.mark("host scene: bounds, BVH, lights");
    if (!rc && sc->host.max_depth > 64) rc = fail(FTN_ERR_BVH_TOO_DEEP, "BVH deeper than the reference's 64-entry traversal stack (bvh.rs:168)");
    if (!rc) rc = upload_scene(d, knobs, sc);
    if (rc) { delete sc; return rc; }
    *out = sc; return FTN_OK;
}
void ftn_scene_destroy(ftn_scene* s) { delete s; }
int ftn_scene_info(const ftn_scene* s, uint32_t* n_nodes, uint32_t* n_prims, uint32_t* n_lights, uint32_t* max_depth, float wb[6]) {
    if (n_nodes) *n_nodes = (uint32_t)s->host.nodes.size();
    if (n_prims) *n_prims = (uint32_t)s->host.order.size();
    if (n_lights) *n_lights = (uint32_t)s->host.light_kind.size();
    if (max_depth) *max_depth = s->host.max_depth;
    if (wb) for (int i = 0; i < 3; i++) { wb[i] = s->host.world.lo[i]; wb[3 + i] = s->host.world.hi[i]; }
    return FTN_OK;
}
int ftn_scene_memory_info(const ftn_scene* s, ftn_scene_memory* m) {
    if (!s || !m) return fail(FTN_ERR_INVALID_ARGUMENT, "null scene / output");
    memset(m, 0, sizeof(*m));
    m->oct = s->oct.n * sizeof(uint4) + s->oct_xbox.n * sizeof(float4);
    m->nodes = s->nodes.n * sizeof(float4); m->quad = s->quad.n * sizeof(float4) + s->quad64.n * sizeof(uint4) + s->quad64_xbox.n * sizeof(float4); m->fat = s->fat.n * sizeof(float4); m->geom = s->geom.n * sizeof(float4);
    m->srec = s->srec.n * sizeof(float4); m->indexed_attributes = s->prim_info.n * sizeof(uint4) + (s->N.n + s->UV.n + s->T.n) * sizeof(float);
    m->prim_class = s->prim_class.n;
    m->lights = s->lights.n * sizeof(DLight) + s->inf_lights.n * sizeof(uint32_t);
    for (const auto& b : s->misc) m->lights += b.n * sizeof(float);
    for (const auto& b : s->misc4) m->lights += b.n * sizeof(float4);
    m->textures = s->textures.n * sizeof(ftn_texture) + s->mtex.n * sizeof(ftn_material_textures) + s->images.n * sizeof(DImage) + s->texels.n * sizeof(float4);
    m->other = s->spheres.n * sizeof(DSphere) + s->materials.n * sizeof(ftn_material) + s->stats.n * sizeof(DevStats);
    m->total = m->oct + m->nodes + m->quad + m->fat + m->geom + m->srec + m->indexed_attributes + m->prim_class + m->lights + m->textures + m->other;
    return FTN_OK;
}
int ftn_scene_get_nodes(const ftn_scene* s, ftn_bvh_node* nodes, uint32_t* order) {
    if (nodes) memcpy(nodes, s->host.nodes.data(), s->host.nodes.size() * sizeof(ftn_bvh_node));
    if (order) memcpy(order, s->host.order.data(), s->host.order.size() * sizeof(uint32_t));
    return FTN_OK;
}
int ftn_scene_get_lights(const ftn_scene* s, int32_t* kind, int32_t* prim) {
    for (size_t i = 0; i < s->host.light_kind.size(); i++) { kind[i] = s->host.light_kind[i]; prim[i] = s->host.light_prim[i]; }
    return FTN_OK;
}

/* test hook for the texture path: a pyramid level as built on the host */
int ftn_test_mipmap_level(uint32_t width, uint32_t height, const float* texels, uint32_t level, uint32_t* level_w, uint32_t* level_h, float* rgb_out) {
    if (!texels || width == 0 || height == 0) return fail(FTN_ERR_INVALID_ARGUMENT, "bad image");
    std::vector<MipLevelHost> pyr; build_mip_pyramid(width, height, texels, &pyr);
    if (level >= pyr.size()) return fail(FTN_ERR_INVALID_ARGUMENT, "no such level");
    if (level_w) *level_w = pyr[level].w;
    if (level_h) *level_h = pyr[level].h;
    if (rgb_out) memcpy(rgb_out, pyr[level].rgb.data(), pyr[level].rgb.size() * sizeof(float));
    return FTN_OK;
}

}  /* extern "C" */
