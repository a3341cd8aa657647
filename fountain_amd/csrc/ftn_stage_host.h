/*
 * ftn_stage_host.h -- what the host files of the image-space stages share (ftn_denoise_host.cpp, ftn_temporal_host.cpp,
 * ftn_display_host.cpp, ftn_bloom_host.cpp, ftn_vectorblur_host.cpp, ftn_metrics_host.cpp): the refusals every stage makes in the same words, the overlap and alignment rules over byte
 * ranges, the launch result, and the device buffers of a host-buffer entry.  need_device() also serves the other host files, and the sampler,
 * pipeline and sample-range refusals are those of the passes on the wavefront pipeline (ftn_gbuffer_host.cpp, ftn_idmatte_host.cpp,
 * ftn_moments_host.cpp), as are the crop's pixel count, count_mode and the any-hit statistics of the first-hit passes.
 *
 * Like ftn_host_internal.h, which it builds on, everything here has hidden visibility and exports nothing.
 */
#ifndef FTN_STAGE_HOST_H
#define FTN_STAGE_HOST_H
#include "ftn_host_internal.h"

#pragma GCC visibility push(hidden)

inline int need_device() { return ftn_device_count() <= 0 ? fail(FTN_ERR_NO_DEVICE, kNoDevice) : FTN_OK; }

/* The refusals the passes on the wavefront pipeline's sample-indexed passes make in the same words (G-buffer, ID mattes, moments): one
 * check each, so that every entry keeps the order of its own.  pass: "G-buffer", "ID-matte", "moments" */
inline int indexed_sampler_check(const ftn_sampler_desc* sd, const char* pass,
                                 const char* why = "with the tile-serial sampler a sample's camera ray depends on everything its tile drew before it") {
    if (sd->kind == FTN_SAMPLER_TILE_SERIAL) return fail(FTN_ERR_UNSUPPORTED, std::string("the ") + pass + " pass needs FTN_SAMPLER_INDEXED: " + why);
    if (sd->kind != FTN_SAMPLER_INDEXED) return fail(FTN_ERR_INVALID_ARGUMENT, "unknown sampler kind");
    return FTN_OK;
}
inline int wavefront_pipeline_check(const ftn_render_options* opt, const char* pass) {
    const uint32_t pipeline = opt ? opt->pipeline : FTN_PIPELINE_AUTO;
    if (pipeline == FTN_PIPELINE_MEGAKERNEL)
        return fail(FTN_ERR_UNSUPPORTED, std::string("the ") + pass + " pass runs on the wavefront pipeline (FTN_PIPELINE_AUTO or FTN_PIPELINE_WAVEFRONT)");
    if (pipeline != FTN_PIPELINE_AUTO && pipeline != FTN_PIPELINE_WAVEFRONT) return fail(FTN_ERR_INVALID_ARGUMENT, "unknown pipeline");
    return FTN_OK;
}
inline int sample_range_check(const ftn_sampler_desc* sd) {
    if ((uint64_t)sd->first_sample > (uint64_t)sd->samples_per_pixel || (uint64_t)sd->first_sample + (uint64_t)sd->sample_count > (uint64_t)sd->samples_per_pixel)
        return fail(FTN_ERR_INVALID_ARGUMENT, "sample range outside [0, samples_per_pixel]");
    return FTN_OK;
}

/* the crop window's pixel count (ftn_firsthit.h has the pass units' twin over RenderParams) */
inline size_t crop_pixels(const ftn_film_desc* film) { return (size_t)std::max(0, film->crop[2] - film->crop[0]) * (size_t)std::max(0, film->crop[3] - film->crop[1]); }
/* launch_trace's count argument for the options' count_traffic: 0 the production kernels, 1 the reference-order walk, 2 the counting build
 * of the production kernels */
inline int count_mode(const ftn_render_options* opt) { return opt ? (opt->count_traffic == 2 ? 2 : (opt->count_traffic ? 1 : 0)) : 0; }
/* The any-hit statistics of a first-hit pass that traces rays of its own (ambient occlusion, light groups), behind a first_hit_render that
 * returned FTN_OK: it has waited for the call and filled the first-hit statistics */
inline int any_hit_stats_out(const ftn_scene* s, const ftn::WavefrontTimes& wt, ftn_stats* st) {
    if (!st) return FTN_OK;
    ftn::DevStats ds; HIP_TRY(hipMemcpy(&ds, s->stats.p, sizeof(ds), hipMemcpyDeviceToHost));
    st->rays_any = ds.rays_any; st->any_ms = wt.any_ms; st->any_launches = wt.any_launches;
    return FTN_OK;
}

inline int image_check(int32_t w, int32_t h) {
    if (w <= 0 || h <= 0) return fail(FTN_ERR_INVALID_ARGUMENT, "image width and height must be positive");
    if ((int64_t)w * (int64_t)h >= ((int64_t)1 << 31)) return fail(FTN_ERR_INVALID_ARGUMENT, "w * h must be below 2^31 pixels");
    return FTN_OK;
}

inline bool is_finite(float v) { return (ftn_det::f2u(v) & 0x7f800000u) != 0x7f800000u; }

/* a buffer argument: where it starts, how many bytes the call touches, the alignment it needs.  A null or zero-length range (an optional
 * buffer that is absent, a workspace of no bytes) overlaps nothing */
struct Range { const void* p; size_t bytes; size_t align; };
inline bool overlaps(const Range& a, const Range& b) {
    const uintptr_t a0 = (uintptr_t)a.p, b0 = (uintptr_t)b.p;
    return a.p && b.p && a.bytes && b.bytes && a0 < b0 + b.bytes && b0 < a0 + a.bytes;
}

/* every output against every input (msg), then against the outputs after it (msg_out, where that refusal has words of its own), in the
 * order given */
inline int overlap_check(std::initializer_list<Range> outs, std::initializer_list<Range> ins, const char* msg, const char* msg_out = nullptr) {
    for (const Range* o = outs.begin(); o != outs.end(); o++) {
        for (const Range& i : ins)
            if (overlaps(*o, i)) return fail(FTN_ERR_INVALID_ARGUMENT, msg);
        for (const Range* o2 = o + 1; o2 != outs.end(); o2++)
            if (overlaps(*o, *o2)) return fail(FTN_ERR_INVALID_ARGUMENT, msg_out ? msg_out : msg);
    }
    return FTN_OK;
}

inline int align_check(std::initializer_list<Range> ranges, const char* msg) {
    for (const Range& r : ranges)
        if ((uintptr_t)r.p % r.align) return fail(FTN_ERR_INVALID_ARGUMENT, msg);
    return FTN_OK;
}

inline int launched(hipError_t e, const char* what) {
    return e == hipSuccess ? FTN_OK : fail(FTN_ERR_INTERNAL, std::string(what) + " launch: " + hipGetErrorString(e));
}

/* the device buffers of one host-buffer entry, freed on every way out.  Each call hands out one buffer of `count` elements in *p, or null
 * for none: count == 0, or an upload from a null host pointer (an optional input the caller left out) */
struct StageBufs {
    std::vector<DevBuf<unsigned char>> held;
    StageBufs() = default;
    StageBufs(const StageBufs&) = delete;
    ~StageBufs() { for (auto& b : held) b.release(); }
    template <class T> int upload(const T* src, size_t count, T** p) {
        held.emplace_back();
        const int rc = src ? held.back().upload((const unsigned char*)src, count * sizeof(T)) : FTN_OK;
        *p = (T*)held.back().p;
        return rc;
    }
    template <class T> int alloc_zero(size_t count, T** p) {
        held.emplace_back();
        const int rc = held.back().alloc_zero(count * sizeof(T));
        *p = (T*)held.back().p;
        return rc;
    }
    template <class T> int alloc(size_t count, T** p) {
        held.emplace_back();
        *p = nullptr;
        if (!(held.back().n = count * sizeof(T))) return FTN_OK;
        HIP_TRY(hipMalloc((void**)&held.back().p, held.back().n));
        *p = (T*)held.back().p;
        return FTN_OK;
    }
    /* copy_back(dst, src, count): a null dst (an optional output the caller left out) copies nothing */
    template <class T> int copy_back(T* dst, const T* src, size_t count) {
        if (dst) HIP_TRY(hipMemcpy(dst, src, count * sizeof(T), hipMemcpyDeviceToHost));
        return FTN_OK;
    }
};

#pragma GCC visibility pop
#endif
