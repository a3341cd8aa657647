/*
 * idmatte_host_check.cpp -- a stand-alone program over the host code of the ID-matte extension, for sanitizer builds: it calls
 * ftn_idmatte_resolve, ftn_idmatte_select and ftn_exr_write_channels on their edge inputs (empty, 1 x 1, the longest names, many
 * attributes, every refusal) and the render entries' refusals.  It needs no GPU: what ftn_idmatte_host.cpp asks of the other units is
 * stubbed below, and there is no device, so nothing behind the stubs is reached.
 *
 *   cd fountain_amd/csrc
 *   hipcc -std=c++17 -O1 -g -x hip --cuda-host-only -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
 *         ../../tools/idmatte_host_check.cpp ftn_idmatte_host.cpp ftn_imageio.cpp -I. -fsanitize=address,undefined -lz -o /tmp/idmatte_host_check
 *   /tmp/idmatte_host_check /tmp
 */
#include "ftn_stage_host.h"
#include "../../include/fountain_hip_idmatte.h"
#include "ftn_idmatte.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>

/* ------------------------------------------------------------------ what the other units provide */
static std::string g_err;
int fail(int code, const std::string& msg) { g_err = msg; return code; }
extern "C" int ftn_device_count(void) { return 0; }
int bind_scene_device(const ftn_scene*, const ftn_render_options*) { abort(); }
int first_hit_render(ftn_scene*, const ftn_camera_desc*, const ftn_film_desc*, const ftn_sampler_desc*, const ftn_tile_range*, hipStream_t, ftn_stats*,
                     const std::function<int(const ftn::RenderParams&, double*)>&) { abort(); }
namespace ftn {
int wavefront_idmatte(WavefrontState**, const RenderParams&, const std::vector<DTile>&, const uint32_t*, uint32_t*, hipStream_t, double*) { abort(); }
hipError_t launch_idmatte_resolve(const uint32_t*, size_t, uint32_t*, hipStream_t) { abort(); }
void launch_idmatte_select(const uint32_t*, size_t, const uint32_t*, size_t, uint32_t, float*, hipStream_t) { abort(); }
void wavefront_destroy(WavefrontState*) {}
}  // namespace ftn

#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "%s:%d: %s failed (%s)\n", __FILE__, __LINE__, #cond, g_err.c_str()); return 1; } } while (0)

int main(int argc, char** argv) {
    const std::string dir = argc > 1 ? argv[1] : ".";
    /* resolve and select: empty, one pixel, a full table with ties, n_used beyond the table, ids at both ends */
    CHECK(ftn_idmatte_resolve(nullptr, 0, nullptr) == FTN_OK);
    CHECK(ftn_idmatte_resolve(nullptr, 1, nullptr) == FTN_ERR_INVALID_ARGUMENT);
    std::vector<ftn_idmatte_pixel> px(5);
    memset(px.data(), 0, px.size() * sizeof(px[0]));
    for (int k = 0; k < 8; k++) { px[1].id[k] = k % 2 ? 0xffffffffu - (uint32_t)k : (uint32_t)k; px[1].weight[k] = (float)(k / 3 + 1); }
    px[1].n_used = 8; px[1].overflow = 2.0f; px[1].miss = 1.0f; px[1].total = 20.0f;
    px[2] = px[1]; px[2].n_used = 0xffffffffu;
    px[3].miss = 4.0f; px[3].total = 4.0f;
    px[4] = px[1]; px[4].n_used = 3; px[4].total = 0.0f;
    std::vector<uint32_t> out(20 * px.size(), 0xdeadbeefu);
    CHECK(ftn_idmatte_resolve(px.data(), px.size(), out.data()) == FTN_OK);
    for (int k = 0; k < 20; k++) CHECK(out[k] == 0u && out[80 + k] == 0u);
    for (int k = 1; k < 8; k++) {                          /* ranked: coverage never rises, ties by id */
        float a, b; memcpy(&a, &out[20 + 2 * k - 1], 4); memcpy(&b, &out[20 + 2 * k + 1], 4);
        CHECK(a > b || (a == b && out[20 + 2 * k - 2] < out[20 + 2 * k]));
    }
    std::vector<float> mask(px.size(), -1.0f);
    const uint32_t ids[4] = {0xfffffffeu, 0u, 4u, 4u};
    CHECK(ftn_idmatte_select(out.data(), px.size(), ids, 4, 3u, mask.data()) == FTN_OK);
    CHECK(mask[0] == 0.0f && mask[3] == 1.0f && mask[1] > 0.0f && mask[1] < 1.0f);
    CHECK(ftn_idmatte_select(out.data(), px.size(), nullptr, 0, 0u, mask.data()) == FTN_OK && mask[1] == 0.0f);
    CHECK(ftn_idmatte_select(nullptr, 0, nullptr, 0, 0u, nullptr) == FTN_OK);
    CHECK(ftn_idmatte_select(out.data(), 1, ids, 4, 4u, mask.data()) == FTN_ERR_INVALID_ARGUMENT);
    CHECK(ftn_idmatte_select(out.data(), 1, nullptr, 4, 0u, mask.data()) == FTN_ERR_INVALID_ARGUMENT);
    CHECK(ftn_idmatte_resolve_device(px.data(), 1, out.data(), nullptr) == FTN_ERR_NO_DEVICE);
    CHECK(ftn_idmatte_select_device(out.data(), 1, ids, 4, 0u, mask.data(), nullptr) == FTN_ERR_NO_DEVICE);

    /* the render entries: refusals, then no device */
    ftn_camera_desc cam; memset(&cam, 0, sizeof(cam));
    ftn_film_desc film; memset(&film, 0, sizeof(film)); film.crop[2] = 4; film.crop[3] = 4; film.filter_radius[0] = film.filter_radius[1] = 0.5f;
    ftn_sampler_desc sd; memset(&sd, 0, sizeof(sd)); sd.kind = FTN_SAMPLER_INDEXED; sd.samples_per_pixel = 2;
    const ftn_scene* scene = reinterpret_cast<const ftn_scene*>(&cam);          /* never looked behind without a device */
    std::vector<ftn_idmatte_pixel> tables(16);
    CHECK(ftn_render_idmatte(nullptr, &cam, &film, &sd, nullptr, nullptr, ids, 4, tables.data(), nullptr) == FTN_ERR_INVALID_ARGUMENT);
    CHECK(ftn_render_idmatte(scene, &cam, &film, &sd, nullptr, nullptr, ids, 4, tables.data(), nullptr) == FTN_ERR_NO_DEVICE);
    CHECK(ftn_render_idmatte_device(scene, &cam, &film, &sd, nullptr, nullptr, ids, 4, tables.data(), nullptr, nullptr) == FTN_ERR_NO_DEVICE);
    film.filter_radius[1] = 1.5f;
    CHECK(ftn_render_idmatte(scene, &cam, &film, &sd, nullptr, nullptr, ids, 4, tables.data(), nullptr) == FTN_ERR_UNSUPPORTED);
    film.filter_radius[1] = 1.0f; sd.kind = FTN_SAMPLER_TILE_SERIAL;
    CHECK(ftn_render_idmatte_device(scene, &cam, &film, &sd, nullptr, nullptr, ids, 4, tables.data(), nullptr, nullptr) == FTN_ERR_UNSUPPORTED);

    /* the file: 1 x 1; 33 x 7 with the longest names and many long attributes; every refusal */
    const std::string path = dir + "/idmatte_host_check.exr";
    const float one = 1.5f;
    const char* n1[1] = {"Y"}; const float* p1[1] = {&one};
    CHECK(ftn_exr_write_channels(path.c_str(), 1, 1, 1, n1, p1, 0, nullptr, nullptr) == FTN_OK);
    const int W = 33, H = 7, NC = 40, NA = 200;
    std::vector<std::vector<float>> planes(NC, std::vector<float>((size_t)W * H, 0.25f));
    std::vector<std::string> names(NC), an(NA), av(NA);
    std::vector<const char*> np(NC), anp(NA), avp(NA);
    std::vector<const float*> pp(NC);
    for (int c = 0; c < NC; c++) { names[c] = std::string(255 - 2, 'a' + c % 26) + std::to_string(10 + c); pp[c] = planes[c].data(); }
    for (int c = 0; c < NC; c++) np[c] = names[NC - 1 - c].c_str();
    for (int a = 0; a < NA; a++) { an[a] = std::string(255 - 3, 'k') + std::to_string(100 + a); av[a] = std::string((size_t)a * 37, 'v'); anp[a] = an[a].c_str(); avp[a] = av[a].c_str(); }
    CHECK(ftn_exr_write_channels(path.c_str(), W, H, NC, np.data(), pp.data(), NA, anp.data(), avp.data()) == FTN_OK);
    remove(path.c_str());
    const std::string long_name(256, 'x');
    const char* dup[2] = {"a", "a"}; const char* empty[2] = {"a", ""}; const char* too_long[2] = {"a", long_name.c_str()}; const char* with_null[2] = {"a", nullptr};
    const float* p2[2] = {&one, &one}; const float* p2n[2] = {&one, nullptr};
    const char* ok2[2] = {"a", "b"};
    const char* bad_attr[1] = {long_name.c_str()}; const char* attr[1] = {"k"};
    CHECK(ftn_exr_write_channels(nullptr, 1, 1, 2, ok2, p2, 0, nullptr, nullptr) == FTN_ERR_INVALID_ARGUMENT);
    CHECK(ftn_exr_write_channels(path.c_str(), 0, 1, 2, ok2, p2, 0, nullptr, nullptr) == FTN_ERR_INVALID_ARGUMENT);
    CHECK(ftn_exr_write_channels(path.c_str(), 1, -3, 2, ok2, p2, 0, nullptr, nullptr) == FTN_ERR_INVALID_ARGUMENT);
    CHECK(ftn_exr_write_channels(path.c_str(), 1, 1, 0, ok2, p2, 0, nullptr, nullptr) == FTN_ERR_INVALID_ARGUMENT);
    CHECK(ftn_exr_write_channels(path.c_str(), 1, 1, 2, nullptr, p2, 0, nullptr, nullptr) == FTN_ERR_INVALID_ARGUMENT);
    CHECK(ftn_exr_write_channels(path.c_str(), 1, 1, 2, ok2, nullptr, 0, nullptr, nullptr) == FTN_ERR_INVALID_ARGUMENT);
    CHECK(ftn_exr_write_channels(path.c_str(), 1, 1, 2, ok2, p2n, 0, nullptr, nullptr) == FTN_ERR_INVALID_ARGUMENT);
    CHECK(ftn_exr_write_channels(path.c_str(), 1, 1, 2, dup, p2, 0, nullptr, nullptr) == FTN_ERR_INVALID_ARGUMENT);
    CHECK(ftn_exr_write_channels(path.c_str(), 1, 1, 2, empty, p2, 0, nullptr, nullptr) == FTN_ERR_INVALID_ARGUMENT);
    CHECK(ftn_exr_write_channels(path.c_str(), 1, 1, 2, too_long, p2, 0, nullptr, nullptr) == FTN_ERR_INVALID_ARGUMENT);
    CHECK(ftn_exr_write_channels(path.c_str(), 1, 1, 2, with_null, p2, 0, nullptr, nullptr) == FTN_ERR_INVALID_ARGUMENT);
    CHECK(ftn_exr_write_channels(path.c_str(), 1, 1, 2, ok2, p2, 1, nullptr, attr) == FTN_ERR_INVALID_ARGUMENT);
    CHECK(ftn_exr_write_channels(path.c_str(), 1, 1, 2, ok2, p2, 1, bad_attr, attr) == FTN_ERR_INVALID_ARGUMENT);
    CHECK(ftn_exr_write_channels(path.c_str(), 1, 1, 2, ok2, p2, -1, attr, attr) == FTN_ERR_INVALID_ARGUMENT);
    FILE* f = fopen(path.c_str(), "rb");
    CHECK(f == nullptr);                                   /* no refusal created the file */
    printf("idmatte_host_check: ok\n");
    return 0;
}
