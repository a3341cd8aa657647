/*
 * host_split_check.cpp -- a stand-alone caller of the pure-host units of the library (ftn_geometry_host.cpp, ftn_bvh_host.cpp, the host half of
 * ftn_scene_host.cpp), for a sanitizer run on a machine without a GPU: the transform, sphere, camera and film entries; ftn_bvh_build serial
 * and on four host threads (a 70 000-triangle mesh, above the threshold of ParallelBvh and of parallel_for) with the same result; the three
 * record trees of each BVH; every level of a few MIP pyramids; the refusals of these entries; ftn_scene_create up to its no-device refusal.
 *
 *   make -C fountain_amd/csrc SUFFIX=_asan EXTRA="-Xarch_host -fsanitize=address,undefined"
 *   hipcc -Xarch_host -fsanitize=address,undefined -x c++ -Iinclude tools/host_split_check.cpp -o host_split_check \
 *         -Lfountain_amd -lfountain_hip_asan -Wl,-rpath,$PWD/fountain_amd && ./host_split_check
 *
 * Without a device ftn_scene_create stops at set_device, so the table steps of upload_scene run only on a GPU (tests/test_scene_residency.py
 * and the parity tests).  Never run it on a GPU machine: sanitizers are for host code.
 */
#include "fountain_hip.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

extern "C" int ftn_bvh_quad64s(const ftn_bvh_node*, uint32_t, uint32_t*, uint32_t*, uint32_t*, float*, uint32_t*);

static int failures = 0;
static void expect(int got, int want, const char* what) {
    if (got != want) { printf("FAIL %s: status %d, expected %d (%s)\n", what, got, want, ftn_last_error()); failures++; }
}

struct Bvh { std::vector<ftn_bvh_node> nodes; std::vector<uint32_t> order; uint32_t depth = 0; };

/* a bumpy n x n grid of quads (2 n^2 triangles) plus, when asked, one sphere */
struct Mesh {
    std::vector<float> P; std::vector<uint32_t> idx, tri_mesh; std::vector<ftn_prim> prims; ftn_mesh mesh; ftn_sphere sphere; ftn_material mat; ftn_scene_desc d;
    Mesh(int n, bool with_sphere) {
        for (int j = 0; j <= n; j++) for (int i = 0; i <= n; i++) { P.push_back(0.5f * (float)i); P.push_back(0.25f * (float)j); P.push_back(0.125f * (float)((i * 7 + j * 3) % 5)); }
        for (int j = 0; j < n; j++) for (int i = 0; i < n; i++) {
            const uint32_t v = (uint32_t)(j * (n + 1) + i);
            const uint32_t q[6] = {v, v + 1, v + (uint32_t)n + 2, v, v + (uint32_t)n + 2, v + (uint32_t)n + 1};
            idx.insert(idx.end(), q, q + 6);
        }
        const uint32_t nt = (uint32_t)idx.size() / 3;
        tri_mesh.assign(nt, 0);
        for (uint32_t t = 0; t < nt; t++) prims.push_back(ftn_prim{FTN_SHAPE_TRIANGLE, t, 0, -1});
        memset(&mesh, 0, sizeof(mesh)); memset(&mat, 0, sizeof(mat)); memset(&d, 0, sizeof(d));
        if (with_sphere) {
            ftn_transform o2w, w2o; const float at[3] = {3.0f, 2.0f, 5.0f};
            expect(ftn_transform_translate(at, &o2w), FTN_OK, "translate"); expect(ftn_transform_inverse(&o2w, &w2o), FTN_OK, "inverse");
            expect(ftn_sphere_init(&o2w, &w2o, 0, 1.5f, -1.0f, 1.25f, 300.0f, &sphere), FTN_OK, "sphere_init");
            prims.push_back(ftn_prim{FTN_SHAPE_SPHERE, 0, 0, -1});
            d.n_spheres = 1; d.spheres = &sphere;
        }
        d.n_prims = (uint32_t)prims.size(); d.prims = prims.data();
        d.n_triangles = nt; d.tri_indices = idx.data(); d.tri_mesh = tri_mesh.data();
        d.n_vertices = (uint32_t)P.size() / 3; d.P = P.data();
        d.n_meshes = 1; d.meshes = &mesh; d.n_materials = 1; d.materials = &mat;
    }
};

static Bvh build(const ftn_scene_desc& d, const char* threads) {
    setenv("FTN_BVH_THREADS", threads, 1);
    Bvh b; b.nodes.resize(2 * (size_t)d.n_prims); b.order.resize(d.n_prims);
    uint32_t n = 0;
    expect(ftn_bvh_build(&d, b.nodes.data(), b.order.data(), &n, &b.depth), FTN_OK, "ftn_bvh_build");
    b.nodes.resize(n);
    return b;
}

static void record_trees(const Bvh& b) {
    const uint32_t n = (uint32_t)b.nodes.size();
    uint32_t nq = 0, bound = 0, nx = 0;
    expect(ftn_bvh_quads(b.nodes.data(), n, nullptr, &nq, &bound), FTN_OK, "ftn_bvh_quads count");
    std::vector<float> quad(32 * (size_t)nq);
    expect(ftn_bvh_quads(b.nodes.data(), n, quad.data(), &nq, &bound), FTN_OK, "ftn_bvh_quads");
    expect(ftn_bvh_quad64s(b.nodes.data(), n, nullptr, &nq, &bound, nullptr, &nx), FTN_OK, "ftn_bvh_quad64s count");
    std::vector<uint32_t> q64(16 * (size_t)nq); std::vector<float> xbox(8 * (size_t)nx);
    expect(ftn_bvh_quad64s(b.nodes.data(), n, q64.data(), &nq, &bound, xbox.data(), &nx), FTN_OK, "ftn_bvh_quad64s");
    expect(ftn_bvh_octs(b.nodes.data(), n, nullptr, &nq, &bound, nullptr, &nx), FTN_OK, "ftn_bvh_octs count");
    std::vector<uint32_t> oct(32 * (size_t)nq); xbox.assign(8 * (size_t)nx, 0.0f);
    expect(ftn_bvh_octs(b.nodes.data(), n, oct.data(), &nq, &bound, xbox.data(), &nx), FTN_OK, "ftn_bvh_octs");
    std::vector<ftn_bvh_node> bad(b.nodes);
    bad[0].idx = 0;                                                                  /* no flattened BVH: the second child before the first */
    expect(ftn_bvh_quads(bad.data(), n, nullptr, &nq, &bound), FTN_ERR_INVALID_ARGUMENT, "ftn_bvh_quads, broken tree");
    expect(ftn_bvh_quad64s(bad.data(), n, nullptr, &nq, &bound, nullptr, &nx), FTN_ERR_INVALID_ARGUMENT, "ftn_bvh_quad64s, broken tree");
    expect(ftn_bvh_octs(bad.data(), n, nullptr, &nq, &bound, nullptr, &nx), FTN_ERR_INVALID_ARGUMENT, "ftn_bvh_octs, broken tree");
    expect(ftn_bvh_quads(nullptr, 3, nullptr, &nq, &bound), FTN_ERR_INVALID_ARGUMENT, "ftn_bvh_quads, null nodes");
}

static void geometry() {
    ftn_transform t[6], m, inv;
    const float d[3] = {1.5f, -2.0f, 0.25f}, axis[3] = {1.0f, 2.0f, 3.0f}, eye[3] = {1.0f, 2.0f, 3.0f}, look[3] = {0.0f, 0.5f, -1.0f}, up[3] = {0.0f, 1.0f, 0.0f};
    expect(ftn_transform_identity(&t[0]), FTN_OK, "identity"); expect(ftn_transform_translate(d, &t[1]), FTN_OK, "translate");
    expect(ftn_transform_scale(2.0f, 0.5f, -3.0f, &t[2]), FTN_OK, "scale"); expect(ftn_transform_rotate(37.0f, axis, &t[3]), FTN_OK, "rotate");
    expect(ftn_transform_look_at(eye, look, up, &t[4]), FTN_OK, "look_at"); expect(ftn_transform_perspective(40.0f, 0.01f, 1000.0f, &t[5]), FTN_OK, "perspective");
    const float singular[16] = {0};
    expect(ftn_transform_from_flat(singular, &m), FTN_ERR_INVALID_ARGUMENT, "from_flat, singular");
    std::vector<float> pts(3 * 257), out(3 * 257);
    for (size_t i = 0; i < pts.size(); i++) pts[i] = 0.01f * (float)(i % 211) - 1.0f;
    for (int i = 0; i < 6; i++) {
        expect(ftn_transform_mul(&t[i], &t[(i + 1) % 6], &m), FTN_OK, "mul"); expect(ftn_transform_inverse(&m, &inv), FTN_OK, "inverse");
        expect(ftn_transform_points(&m, 257, pts.data(), out.data()), FTN_OK, "points"); expect(ftn_transform_normals(&m, 257, pts.data(), out.data()), FTN_OK, "normals");
        float o[3];
        expect(ftn_transform_point(&m, pts.data(), o), FTN_OK, "point"); expect(ftn_transform_vector(&m, pts.data(), o), FTN_OK, "vector");
        expect(ftn_transform_normal(&m, pts.data(), o), FTN_OK, "normal"); (void)ftn_transform_swaps_handedness(&m);
    }
    const int32_t sizes[4][2] = {{64, 48}, {1920, 1080}, {1, 1}, {37, 53}};
    const float crops[4][4] = {{0.0f, 0.0f, 1.0f, 1.0f}, {0.25f, 0.1f, 0.8f, 0.95f}, {0.0f, 0.0f, 1.0f, 1.0f}, {0.3f, 0.3f, 0.31f, 0.9f}};
    for (int k = 0; k < 4; k++) {
        const float sw[4] = {-1.5f, -1.0f, 1.5f, 1.0f}, sh[2] = {0.0f, 1.0f};
        ftn_camera_desc cam; ftn_film_desc film; int32_t sb[4]; uint32_t tiles = 0;
        expect(ftn_camera_perspective(&inv, sizes[k], sw, sh, 0.1f, 4.0f, 35.0f, &cam), FTN_OK, "camera_perspective");
        expect(ftn_film_init(sizes[k], crops[k], &film), FTN_OK, "film_init"); expect(ftn_film_sample_bounds(&film, sb), FTN_OK, "film_sample_bounds");
        expect(ftn_film_tile_count(&film, &tiles), FTN_OK, "film_tile_count");
        std::vector<ftn_pixel> px(9); std::vector<float> rgb(27);
        for (size_t i = 0; i < px.size(); i++) { px[i].xyz[0] = 0.1f * (float)i; px[i].xyz[1] = 0.2f; px[i].xyz[2] = 0.3f; px[i].filter_weight_sum = (float)(i % 3); }
        expect(ftn_film_resolve(px.data(), px.size(), rgb.data()), FTN_OK, "film_resolve");
    }
}

static void pyramids() {
    const uint32_t shapes[6][2] = {{1, 1}, {7, 1}, {1, 7}, {5, 4}, {33, 17}, {32768, 1}};
    for (const auto& s : shapes) {
        std::vector<float> img(3 * (size_t)s[0] * s[1]);
        for (size_t i = 0; i < img.size(); i++) img[i] = 0.05f + 0.001f * (float)(i % 900);
        uint32_t lw = 0, lh = 0, level = 0;
        while (ftn_test_mipmap_level(s[0], s[1], img.data(), level, &lw, &lh, nullptr) == FTN_OK) {
            std::vector<float> lev(3 * (size_t)lw * lh);
            expect(ftn_test_mipmap_level(s[0], s[1], img.data(), level, nullptr, nullptr, lev.data()), FTN_OK, "mipmap level");
            level++;
        }
        uint32_t want = 1; for (uint32_t big = s[0] > s[1] ? s[0] : s[1]; big >>= 1;) want++;
        expect((int)level, (int)want, "mipmap level count");
    }
    expect(ftn_test_mipmap_level(0, 4, nullptr, 0, nullptr, nullptr, nullptr), FTN_ERR_INVALID_ARGUMENT, "mipmap, bad image");
}

int main() {
    geometry();
    pyramids();
    Mesh small(5, true), large(187, false);                                         /* 50 triangles and a sphere; 69 938 triangles */
    const Bvh a = build(small.d, "1");
    record_trees(a);
    const Bvh s1 = build(large.d, "1"), s4 = build(large.d, "4");
    if (large.d.n_prims < 65536) { printf("FAIL the large mesh is below the threshold for host threads\n"); failures++; }
    if (s1.nodes.size() != s4.nodes.size() || s1.depth != s4.depth || memcmp(s1.nodes.data(), s4.nodes.data(), s1.nodes.size() * sizeof(ftn_bvh_node)) != 0 ||
        memcmp(s1.order.data(), s4.order.data(), s1.order.size() * sizeof(uint32_t)) != 0) { printf("FAIL the BVH depends on the thread count\n"); failures++; }
    record_trees(s4);
    ftn_scene_desc bad = small.d; bad.prims = nullptr;
    expect(ftn_bvh_build(&bad, nullptr, nullptr, nullptr, nullptr), FTN_ERR_INVALID_ARGUMENT, "ftn_bvh_build, null array");
    expect(ftn_bvh_build(nullptr, nullptr, nullptr, nullptr, nullptr), FTN_ERR_INVALID_ARGUMENT, "ftn_bvh_build, null description");
    ftn_scene* sc = nullptr;
    expect(ftn_scene_create(&small.d, 0, &sc), FTN_ERR_NO_DEVICE, "ftn_scene_create without a device");
    expect(ftn_scene_create(&small.d, 0, nullptr), FTN_ERR_INVALID_ARGUMENT, "ftn_scene_create, null output");
    printf(failures ? "%d failures\n" : "host_split_check: ok\n", failures);
    return failures ? 1 : 0;
}
