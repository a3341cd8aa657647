/*
 * ftn_host_internal.h -- what the host files of libfountain_hip.so share (ftn_host.cpp, ftn_scene_host.cpp, ftn_bvh_host.cpp,
 * ftn_geometry_host.cpp, ftn_gbuffer_host.cpp, ftn_denoise_host.cpp, ftn_moments_host.cpp, ftn_adaptive_host.cpp, the test hooks): the scene
 * behind a ftn_scene handle, error reporting, device selection, the host thread budget, and the steps every render call takes (device,
 * tiles, parameters, accumulators, timing, statistics).  What scene construction asks of the BVH unit is in ftn_bvh_host.h.
 *
 * Everything declared here has hidden visibility: splitting the host library into files exports nothing beyond the C ABI.
 */
#ifndef FTN_HOST_INTERNAL_H
#define FTN_HOST_INTERNAL_H
#include "ftn_kernels.h"
#include "ftn_wavefront.h"

#include <algorithm>
#include <functional>
#include <string>
#include <thread>
#include <vector>

#pragma GCC visibility push(hidden)

/* the message of the calling thread's last failure (ftn_last_error); returns `code` */
int fail(int code, const std::string& msg);
#define HIP_TRY(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) return fail(e_ == hipErrorOutOfMemory ? FTN_ERR_OUT_OF_MEMORY : FTN_ERR_NO_DEVICE, std::string(#expr ": ") + hipGetErrorString(e_)); } while (0)

/* hipSetDevice(device) unless device < 0; FTN_ERR_NO_DEVICE (kNoDevice) without a HIP device */
inline const char* const kNoDevice = "no HIP device available: the fountain HIP path needs an AMD GPU (there is no CPU fallback)";
int set_device(int device);

/* host threads for per-element passes (this process's share of the host; FTN_BVH_THREADS overrides; at most 32).  f(begin, end) over
 * [0, n) in contiguous blocks: every pass that uses it writes each element from that element's inputs alone, so the result does not depend
 * on the number of threads. */
int host_threads();
template <class F> void parallel_for(size_t n, F f) {
    const int nt = (int)std::min<size_t>((size_t)host_threads(), n / 65536 + 1);
    if (nt <= 1) { f((size_t)0, n); return; }
    std::vector<std::thread> th;
    for (int t = 0; t < nt; t++) th.emplace_back([&, t]() { f(n * (size_t)t / (size_t)nt, n * (size_t)(t + 1) / (size_t)nt); });
    for (auto& x : th) x.join();
}

template <class T> struct DevBuf {
    T* p = nullptr; size_t n = 0;
    int upload(const T* src, size_t count) {
        n = count; if (!count) return FTN_OK;
        HIP_TRY(hipMalloc((void**)&p, count * sizeof(T)));
        HIP_TRY(hipMemcpy(p, src, count * sizeof(T), hipMemcpyHostToDevice));
        return FTN_OK;
    }
    int alloc_zero(size_t count) {
        n = count; if (!count) return FTN_OK;
        HIP_TRY(hipMalloc((void**)&p, count * sizeof(T)));
        HIP_TRY(hipMemset(p, 0, count * sizeof(T)));
        return FTN_OK;
    }
    void release() { if (p) (void)hipFree(p); p = nullptr; n = 0; }
};

/* three per-crop-pixel sums of a render call (grow-only, reused across calls): a pixel's own samples, cleared on every call, and the samples
 * that spill into it from inside / outside their tile, cleared only while spill_dirty says they may be non-zero (DevStats::bc_writes) */
struct FilmAcc {
    DevBuf<float4> own, in_tile, other_tile; size_t pixels = 0;
    bool spill_dirty = true;
    void release() { own.release(); in_tile.release(); other_tile.release(); pixels = 0; spill_dirty = true; }
    int prepare(size_t npix, hipStream_t stream);      /* grow to npix pixels and clear; spill_dirty until the call reports otherwise */
};

struct Aabb { float lo[3], hi[3]; };
struct HostScene {
    std::vector<ftn_bvh_node> nodes; std::vector<uint32_t> order; uint32_t max_depth = 0; Aabb world;
    std::vector<int32_t> light_kind, light_prim;
};

struct ftn_scene {
    int device = 0;
    HostScene host;
    ftn::DScene d; uint32_t stack_entries = 1;
    DevBuf<float4> nodes, geom, fat, srec, quad, oct_xbox, quad64_xbox; DevBuf<uint4> prim_info, oct, quad64; DevBuf<float> N, UV, T; DevBuf<ftn::DSphere> spheres; DevBuf<ftn_material> materials; DevBuf<ftn::DLight> lights;
    DevBuf<uint32_t> inf_lights; DevBuf<unsigned char> prim_class; std::vector<DevBuf<float>> misc; std::vector<DevBuf<float4>> misc4;
    DevBuf<ftn_texture> textures; DevBuf<ftn_material_textures> mtex; DevBuf<ftn::DImage> images; DevBuf<float4> texels;
    /* render work buffers (grow-only, reused across calls; not counted by ftn_scene_memory_info): the film's accumulators, the moments'
     * (grown by moments and adaptive calls only), the cached tile selection (tile_key: the film and tile range it was made for) */
    FilmAcc acc, moments; DevBuf<ftn::DTile> tiles; DevBuf<ftn::DevStats> stats;
    ftn::WavefrontState* wf = nullptr;
    std::vector<ftn::DTile> sel; int32_t tile_key[10] = {0};
    ~ftn_scene() {
        nodes.release(); geom.release(); fat.release(); srec.release(); quad.release(); quad64.release(); quad64_xbox.release(); oct.release(); oct_xbox.release(); prim_info.release(); N.release(); UV.release(); T.release(); spheres.release(); materials.release(); lights.release(); inf_lights.release(); prim_class.release();
        for (auto& b : misc) b.release();
        for (auto& b : misc4) b.release();
        textures.release(); mtex.release(); images.release(); texels.release();
        acc.release(); moments.release(); tiles.release(); stats.release();
        ftn::wavefront_destroy(wf);
    }
};

/* the film's sample-space tiles in film tile order (bounds.rs:85-97, integrator/mod.rs:182-185) */
void list_tiles(const ftn_film_desc* f, std::vector<ftn::DTile>* tiles);
/* ftn_stats from the device tallies and the call's time */
void stats_out(const ftn::DevStats& ds, ftn_stats* st, double ms);

/* ------------------------------------------------------------------ the steps of a render call, in call order */
/* the options' device if one is given (it must be the scene's: the scene's arrays live there), else the scene's */
int bind_scene_device(const ftn_scene* s, const ftn_render_options* opt);
/* the tiles of the tile range, in film tile order, valid_off = exclusive prefix sum of their pixel counts */
void select_tiles(const ftn_film_desc* film, const ftn_tile_range* tr, std::vector<ftn::DTile>* sel);
/* select_tiles through the scene's cache (s->sel and its device copy s->tiles); sets P->tiles / n_tiles */
int scene_tiles(ftn_scene* s, const ftn_film_desc* film, const ftn_tile_range* tr, hipStream_t stream, ftn::RenderParams* P);
/* camera, film, sampler (sample range [first_sample, first_sample + sample_count) of the indexed sampler, all samples of the tile-serial
 * one) and integrator */
ftn::RenderParams render_params(const ftn_scene* s, const ftn_camera_desc* cam, const ftn_film_desc* film, const ftn_sampler_desc* sd, const ftn_integrator_desc* id);
/* grows and clears the film's accumulators for P's crop (and the moments' when `moments`), clears the call's DevStats; sets P's pointers */
int prepare_film(ftn_scene* s, bool moments, hipStream_t stream, ftn::RenderParams* P);

struct EventPair {                                       /* a call's start and stop events, destroyed on every way out */
    hipEvent_t a = nullptr, b = nullptr;
    ~EventPair() { if (a) (void)hipEventDestroy(a); if (b) (void)hipEventDestroy(b); }
    int start(hipStream_t stream);
    int stop(hipStream_t stream, float* ms);             /* waits for the call's last launch */
};

/* the call's DevStats; whether the spill accumulators (and the moments' when `moments`) still hold zeros follows from them */
int read_stats(ftn_scene* s, bool moments, ftn::DevStats* ds);
/* ftn_stats of a wavefront or megakernel render: stats_out, the estimate_direct rays the any-hit kernel answered counted as Scene::intersect
 * calls (the reference's accounting), the kernel groups' times */
void render_stats_out(ftn::DevStats ds, const ftn::WavefrontTimes& wt, float ms, ftn_stats* st);
/* the call's device-side error (DevStats::error) as a status */
int render_error(int error);

/* host-buffer twins (ftn_render, ftn_render_moments, ftn_render_adaptive): run(device pointers) renders into zeroed device buffers of npix
 * pixels, one per output; when it returns its film (FTN_OK or FTN_ERR_NAN_RADIANCE) they are copied back and added float by float into the
 * caller's arrays -- or, for an output with add = false, copied into it */
struct HostOut { void* host; size_t pixel_bytes; bool add; };
template <class Run> int render_to_host(size_t npix, std::initializer_list<HostOut> outs, Run run) {
    std::vector<DevBuf<unsigned char>> dev(outs.size());
    struct Release { std::vector<DevBuf<unsigned char>>& d; ~Release() { for (auto& b : d) b.release(); } } keep{dev};
    std::vector<void*> dp;
    size_t k = 0;
    for (const HostOut& o : outs) { int rc = dev[k].alloc_zero(npix * o.pixel_bytes); if (rc) return rc; dp.push_back(dev[k++].p); }
    const int rc = run(dp.data());
    if ((rc != FTN_OK && rc != FTN_ERR_NAN_RADIANCE) || npix == 0) return rc;
    std::vector<std::vector<float>> back;
    k = 0;
    for (const HostOut& o : outs) {
        back.emplace_back(o.add ? npix * o.pixel_bytes / sizeof(float) : 0);
        if (hipMemcpy(o.add ? (void*)back.back().data() : o.host, dev[k++].p, npix * o.pixel_bytes, hipMemcpyDeviceToHost) != hipSuccess)
            return fail(FTN_ERR_NO_DEVICE, "copy back failed");
    }
    k = 0;
    for (const HostOut& o : outs) {
        const std::vector<float>& b = back[k++];
        float* h = (float*)o.host;
        for (size_t i = 0; i < b.size(); i++) h[i] += b[i];
    }
    return rc;
}

/* The device entry of a first-hit pass (G-buffer, ID mattes) behind its refusals and bind_scene_device: the steps above with PathIntegrator
 * of max_depth 0 in the parameters, around run(P, &trace_ms), the pass's wavefront call.  When run fails the stream is drained before the
 * return (the caller may free what it uploaded for the call) and the status comes with wavefront_error().  st: rays_closest,
 * camera_samples, spill_samples, kernel_ms, trace_ms; the rest zero. */
int first_hit_render(ftn_scene* s, const ftn_camera_desc* cam, const ftn_film_desc* film, const ftn_sampler_desc* sd, const ftn_tile_range* tr, hipStream_t stream, ftn_stats* st,
                     const std::function<int(const ftn::RenderParams& P, double* trace_ms)>& run);

/* host-buffer twins of the first-hit passes: the caller's npix pixels go to the device, run(device pixels) continues them there, and they
 * come back -- every pixel's own samples are added to the caller's sums one at a time (not summed apart and added at the end), so
 * splitting a sample range over calls gives the bits of one call */
template <class T, class Run> int continue_on_device(T* host_pixels, size_t npix, Run run) {
    DevBuf<T> dev;
    int rc = dev.upload(host_pixels, npix);
    if (rc == FTN_OK) rc = run(dev.p ? (void*)dev.p : (void*)host_pixels);
    if (rc == FTN_OK && npix && hipMemcpy(host_pixels, dev.p, npix * sizeof(T), hipMemcpyDeviceToHost) != hipSuccess) rc = fail(FTN_ERR_NO_DEVICE, "copy back failed");
    dev.release();
    return rc;
}

/* the moments pass's refusals (ftn_moments_host.cpp): host-side checks only, before any device work */
int moments_refusals(const ftn_scene* s, const ftn_sampler_desc* sd, const ftn_integrator_desc* id, const ftn_render_options* opt);

#pragma GCC visibility pop
#endif
