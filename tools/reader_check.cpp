/*
 * reader_check.cpp -- a stand-alone program over the library's three file readers, for sanitizer builds: it calls ftn_exr_read,
 * ftn_ply_load or ftn_pbrt_load on every file of a corpus of corrupt files, the way a caller does: the sizing call, then the filling
 * call into heap buffers of exactly the size the sizing call reported, so that one element written too many is a heap overflow the
 * sanitizer sees.  Every scene file that is accepted goes on to ftn_bvh_build (bounds, the BVH and its record trees, the light tables: the
 * host half of ftn_scene_host.cpp with ftn_bvh_host.cpp), which must return, whatever numbers the file delivered.  It needs no GPU: what
 * these units ask of the others is stubbed below (there is no device, and no case of the corpus reaches a subdivision).
 *
 *   python tests/_corrupt_files.py --write /tmp/corpus          # every case of the catalogue and /tmp/corpus/manifest.txt
 *   cd fountain_amd/csrc
 *   hipcc -std=c++17 -O1 -g -x hip --cuda-host-only -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
 *         ../../tools/reader_check.cpp ftn_pbrt.cpp ftn_imageio.cpp ftn_geometry_host.cpp ftn_scene_host.cpp ftn_bvh_host.cpp -I. -fsanitize=address,undefined -lz -o /tmp/reader_check
 *   /tmp/reader_check /tmp/corpus /tmp/corpus/manifest.txt
 *
 * A manifest line is  reader <TAB> must_refuse <TAB> path relative to the directory <TAB> name of the case.  Per file: every call returns
 * FTN_OK, FTN_ERR_INVALID_ARGUMENT, FTN_ERR_UNSUPPORTED or FTN_ERR_OUT_OF_MEMORY; a refusal leaves a message; a case marked must_refuse
 * is refused; the two calls agree on the size; an accepted PLY has no index at or above its vertex count; ftn_bvh_build returns on every
 * accepted scene (any status).  Prints `reader_check: ok`.
 */
#include "../include/fountain_hip.h"
#include "../include/fountain_hip_filter.h"
#include "../include/fountain_hip_subdiv.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <memory>
#include <sstream>
#include <string>

/* ------------------------------------------------------------------ what the other units provide */
static std::string g_err;
int fail(int code, const std::string& msg) { g_err = msg; return code; }
extern "C" int ftn_device_count(void) { return 0; }
extern "C" const char* ftn_last_error(void) { return g_err.c_str(); }
extern "C" int ftn_filter_init(uint32_t, ftn_filter_desc*) { return fail(FTN_ERR_UNSUPPORTED, "reader_check: no filters"); }
extern "C" int ftn_loop_subdivide_info(const uint32_t*, int32_t, int32_t, int32_t, ftn_subdiv_info*) { return fail(FTN_ERR_UNSUPPORTED, "reader_check: no subdivision"); }
extern "C" int ftn_loop_subdivide(const float*, int32_t, const uint32_t*, int32_t, int32_t, float*, float*, uint32_t*, int) { abort(); }
extern "C" int ftn_loop_subdivide_cpu(const float*, int32_t, const uint32_t*, int32_t, int32_t, float*, float*, uint32_t*) { abort(); }
int set_device(int) { return fail(FTN_ERR_NO_DEVICE, "reader_check: no device"); }
namespace ftn { struct WavefrontState; void wavefront_destroy(WavefrontState*) {} }

static int g_bad = 0;
static void bad(const std::string& file, const std::string& name, const std::string& what) {
    if (g_bad++ < 40) fprintf(stderr, "reader_check: %s [%s]: %s\n", file.c_str(), name.c_str(), what.c_str());
}
static bool allowed(int rc) { return rc == FTN_OK || rc == FTN_ERR_INVALID_ARGUMENT || rc == FTN_ERR_UNSUPPORTED || rc == FTN_ERR_OUT_OF_MEMORY; }
static long file_size(const std::string& p) { std::ifstream f(p, std::ios::binary | std::ios::ate); return f ? (long)f.tellg() : 0; }

/* -> true when the file was accepted by both calls */
static bool check_exr(const std::string& path, const std::string& name) {
    uint32_t w = 0, h = 0, w2 = 0, h2 = 0;
    int rc = ftn_exr_read(path.c_str(), &w, &h, nullptr);
    if (!allowed(rc)) bad(path, name, "sizing call returned " + std::to_string(rc));
    if (rc) { if (!*ftn_imageio_last_error()) bad(path, name, "refused without a message"); return false; }
    const size_t n = (size_t)w * h * 3;
    if (n * 4 > (size_t)file_size(path) * 2048 + (1u << 20)) { bad(path, name, "the sizing call reports more pixels than a file of this size packs"); return true; }
    std::unique_ptr<float[]> px(new float[n]);                  /* exactly sized: the sanitizer guards its end */
    rc = ftn_exr_read(path.c_str(), &w2, &h2, px.get());
    if (!allowed(rc)) bad(path, name, "filling call returned " + std::to_string(rc));
    if (rc) { if (!*ftn_imageio_last_error()) bad(path, name, "refused without a message"); return false; }
    if (w2 != w || h2 != h) bad(path, name, "the two calls disagree on the size");
    return true;
}
static bool check_ply(const std::string& path, const std::string& name) {
    uint32_t nv = 0, nt = 0, nv2 = 0, nt2 = 0; int hn = 0, hu = 0;
    int rc = ftn_ply_load(path.c_str(), &nv, &nt, nullptr, nullptr, nullptr, nullptr, &hn, &hu);
    if (!allowed(rc)) bad(path, name, "sizing call returned " + std::to_string(rc));
    if (rc) { if (!*ftn_pbrt_last_error()) bad(path, name, "refused without a message"); return false; }
    if (((size_t)nv + nt) * 4 > (size_t)file_size(path) + 64) { bad(path, name, "the sizing call reports more elements than the file holds"); return true; }
    /* exactly sized: the sanitizer guards each end */
    std::unique_ptr<float[]> P(new float[3 * (size_t)nv]), N(new float[3 * (size_t)nv]), UV(new float[2 * (size_t)nv]);
    std::unique_ptr<uint32_t[]> idx(new uint32_t[3 * (size_t)nt]);
    rc = ftn_ply_load(path.c_str(), &nv2, &nt2, P.get(), N.get(), UV.get(), idx.get(), &hn, &hu);
    if (!allowed(rc)) bad(path, name, "filling call returned " + std::to_string(rc));
    if (rc) { if (!*ftn_pbrt_last_error()) bad(path, name, "refused without a message"); return false; }
    if (nv2 != nv || nt2 != nt) bad(path, name, "the two calls disagree on the counts");
    for (size_t k = 0; k < 3 * (size_t)nt; k++) if (idx[k] >= nv) { bad(path, name, "accepted a vertex index at or above the vertex count"); break; }
    return true;
}
static bool check_pbrt(const std::string& path, const std::string& name) {
    ftn_pbrt* s = nullptr;
    int rc = ftn_pbrt_load(path.c_str(), &s);
    if (!allowed(rc)) bad(path, name, "returned " + std::to_string(rc));
    if (rc) { if (!*ftn_pbrt_last_error()) bad(path, name, "refused without a message"); if (s) bad(path, name, "a refusal left a handle"); return false; }
    const ftn_scene_desc* d = ftn_pbrt_scene(s);
    for (uint32_t k = 0; k < 3 * d->n_triangles; k++) if (d->tri_indices[k] >= d->n_vertices) { bad(path, name, "accepted a vertex index at or above the vertex count"); break; }
    for (uint32_t k = 0; k < d->n_prims; k++) if (d->prims[k].material < 0 || (uint32_t)d->prims[k].material >= d->n_materials) { bad(path, name, "a primitive without a material"); break; }
    uint32_t n_nodes = 0;
    (void)ftn_bvh_build(d, nullptr, nullptr, &n_nodes, nullptr);        /* refused or built: it returns, and the sanitizers watch it */
    ftn_pbrt_destroy(s);
    return true;
}

int main(int argc, char** argv) {
    if (argc < 3) { fprintf(stderr, "usage: reader_check DIR MANIFEST\n"); return 2; }
    const std::string dir = argv[1];
    std::ifstream man(argv[2]);
    if (!man) { fprintf(stderr, "reader_check: cannot open %s\n", argv[2]); return 2; }
    std::string line; long n = 0, n_ok = 0;
    while (std::getline(man, line)) {
        std::istringstream ss(line); std::string reader, refuse, rel, name;
        if (!std::getline(ss, reader, '\t') || !std::getline(ss, refuse, '\t') || !std::getline(ss, rel, '\t')) { fprintf(stderr, "reader_check: malformed manifest line %ld\n", n + 1); return 2; }
        std::getline(ss, name);
        const std::string path = dir + "/" + rel;
        bool ok;
        if (reader == "exr") ok = check_exr(path, name); else if (reader == "ply") ok = check_ply(path, name); else if (reader == "pbrt") ok = check_pbrt(path, name);
        else { fprintf(stderr, "reader_check: unknown reader %s\n", reader.c_str()); return 2; }
        if (ok && refuse == "1") bad(path, name, "accepted, must be refused");
        n++; n_ok += ok;
    }
    if (g_bad) { fprintf(stderr, "reader_check: %d checks failed over %ld files\n", g_bad, n); return 1; }
    printf("reader_check: ok (%ld files, %ld accepted)\n", n, n_ok);
    return 0;
}
