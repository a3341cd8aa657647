/*
 * ftn_motion_host.cpp -- C entry points of include/fountain_hip_motion.h.
 *
 * The pass takes the steps of every first-hit pass (first_hit_render, ftn_host_internal.h), as the G-buffer does, behind the correspondence
 * check of the two scenes and with the table that carries a primitive of the current scene's BVH order to the previous scene's; the
 * resolve and the motion vectors run the arithmetic of ftn_motion.h on the host or in its kernels; the three temporal entries are the
 * temporal stage's own bodies (ftn_temporal.h) with the caller's mv8.
 */
#include "ftn_stage_host.h"
#include "../../include/fountain_hip_motion.h"
#include "ftn_motion.h"

#include <cstring>

using namespace ftn;

namespace {

/* what the correspondence check reads of one scene: per primitive in INSERTION order its kind and, for a sphere, its record */
struct SceneKinds {
    std::vector<uint32_t> inv;          /* insertion index -> BVH index */
    std::vector<uint8_t> sphere;        /* per insertion index: 1 = sphere */
    std::vector<uint32_t> shape;        /* per insertion index: sphere index (spheres only) */
    std::vector<DSphere> spheres;
};

/* the scene's primitive order inverted (it must be a permutation), and for a scene with spheres the kinds and sphere indices of its
 * leaf-test records and its sphere records, read back from the device arrays with copies: a scene keeps no host copy of them */
static int scene_kinds(const ftn_scene* s, const char* which, SceneKinds* K) {
    const std::vector<uint32_t>& order = s->host.order;
    const size_t np = order.size();
    K->inv.assign(np, 0xffffffffu);
    for (size_t i = 0; i < np; i++) {
        if (order[i] >= np || K->inv[order[i]] != 0xffffffffu) return fail(FTN_ERR_INTERNAL, std::string("the ") + which + " scene's primitive order is corrupt");
        K->inv[order[i]] = (uint32_t)i;
    }
    K->sphere.assign(np, 0); K->shape.assign(np, 0);
    if (s->d.n_spheres == 0 || np == 0) return FTN_OK;
    if (int rc = set_device(s->device)) return rc;
    const size_t stride = s->d.geom_stride;
    std::vector<float4> g(stride * np);
    HIP_TRY(hipMemcpy(g.data(), s->d.geom, g.size() * sizeof(float4), hipMemcpyDeviceToHost));
    K->spheres.resize(s->spheres.n);
    if (s->spheres.n) HIP_TRY(hipMemcpy(K->spheres.data(), s->spheres.p, s->spheres.n * sizeof(DSphere), hipMemcpyDeviceToHost));
    for (size_t i = 0; i < np; i++) {
        if (!(ftn_det::f2u(g[stride * i].w) & GF_KIND_SPHERE)) continue;
        const uint32_t si = ftn_det::f2u(g[stride * i + 1].w);
        if (si >= K->spheres.size()) return fail(FTN_ERR_INTERNAL, std::string("the ") + which + " scene's sphere indices are corrupt");
        K->sphere[order[i]] = 1; K->shape[order[i]] = si;
    }
    return FTN_OK;
}

static bool same_bits(const void* a, const void* b, size_t n) { return memcmp(a, b, n) == 0; }

/* Refusal 2 of the header and the remap table: entry i, for primitive i of `cur` in BVH order, is the BVH index in `prev` of the same
 * insertion-order primitive (below prev's primitive count by construction: inv is a permutation's inverse), MV_REMAP_COPY or-ed in for a
 * sphere whose transforms are the same bits in both scenes.  The kernel reads prev's arrays through these entries and nothing else. */
static int correspondence(const ftn_scene* cur, const ftn_scene* prev, std::vector<uint32_t>* remap) {
    if (cur->device >= 0 && prev->device >= 0 && cur->device != prev->device)
        return fail(FTN_ERR_INVALID_ARGUMENT, "the two scenes live on different devices (" + std::to_string(cur->device) + " and " + std::to_string(prev->device) + ")");
    const size_t np = cur->host.order.size(), np_prev = prev->host.order.size();
    if (np != np_prev)
        return fail(FTN_ERR_INVALID_ARGUMENT, "the scenes do not correspond: " + std::to_string(np) + " primitives against " + std::to_string(np_prev) +
                                                  " in the previous scene; primitive " + std::to_string(std::min(np, np_prev)) + " has no counterpart");
    if (np >= (size_t)MV_REMAP_COPY) return fail(FTN_ERR_UNSUPPORTED, "the previous-position pass takes fewer than 2^31 primitives");
    SceneKinds kc, kp;
    int rc;
    if ((rc = scene_kinds(cur, "current", &kc)) || (rc = scene_kinds(prev, "previous", &kp))) return rc;
    std::vector<uint8_t> copy(np, 0);
    for (size_t i = 0; i < np; i++) {                     /* insertion order: the first offending primitive is named */
        if (kc.sphere[i] != kp.sphere[i])
            return fail(FTN_ERR_INVALID_ARGUMENT, "the scenes do not correspond: primitive " + std::to_string(i) + " is a " + (kc.sphere[i] ? "sphere" : "triangle") +
                                                      " here and a " + (kp.sphere[i] ? "sphere" : "triangle") + " in the previous scene");
        if (!kc.sphere[i]) continue;
        const DSphere& a = kc.spheres[kc.shape[i]]; const DSphere& b = kp.spheres[kp.shape[i]];
        if (!same_bits(&a.radius, &b.radius, 4) || !same_bits(&a.z_min, &b.z_min, 4) || !same_bits(&a.z_max, &b.z_max, 4) || !same_bits(&a.phi_max, &b.phi_max, 4) ||
            a.reverse_orientation != b.reverse_orientation)
            return fail(FTN_ERR_INVALID_ARGUMENT, "the scenes do not correspond: primitive " + std::to_string(i) +
                                                      ", a sphere, changed its radius, z range, phi_max or orientation (a sphere moves through its transforms only)");
        copy[i] = same_bits(a.o2w, b.o2w, 64) && same_bits(a.o2w_inv, b.o2w_inv, 64) && same_bits(a.w2o, b.w2o, 64);
    }
    remap->resize(np);
    for (size_t i = 0; i < np; i++) {
        const uint32_t ins = cur->host.order[i];
        (*remap)[i] = kp.inv[ins] | (copy[ins] ? MV_REMAP_COPY : 0u);
    }
    return FTN_OK;
}

/* every refusal of the pass in the header's order; with a device, the remap table.  A scene handle is looked behind only where a device
 * exists: without one no scene can have been created */
static int motion_refusals(const ftn_scene* cs, const ftn_scene* prev, const ftn_camera_desc* cam, const ftn_film_desc* film, const ftn_sampler_desc* sd,
                           const ftn_render_options* opt, const void* out, std::vector<uint32_t>* remap) {
    if (!cs || !prev || !cam || !film || !sd || !out) return fail(FTN_ERR_INVALID_ARGUMENT, "null argument");
    const bool device = ftn_device_count() > 0;
    if (device) { if (int no = correspondence(cs, prev, remap)) return no; }
    if (int no = indexed_sampler_check(sd, "previous-position")) return no;
    if (int no = wavefront_pipeline_check(opt, "previous-position")) return no;
    return need_device();
}

static int render_motion_device(const ftn_scene* cs, const ftn_scene* prev, const std::vector<uint32_t>& remap, const ftn_camera_desc* cam, const ftn_film_desc* film,
                                const ftn_sampler_desc* sd, const ftn_tile_range* tr, const ftn_render_options* opt, void* device_pixels, void* stream_v, ftn_stats* st) {
    ftn_scene* s = const_cast<ftn_scene*>(cs);
    int rc = bind_scene_device(s, opt); if (rc) return rc;
    hipStream_t stream = (hipStream_t)stream_v;
    if (int no = sample_range_check(sd)) return no;
    StageBufs bufs;
    uint32_t* d_remap = nullptr;
    if ((rc = bufs.upload(remap.data(), remap.size(), &d_remap))) return rc;
    return first_hit_render(s, cam, film, sd, tr, stream, st, [&](const RenderParams& P, double* trace_ms) {        /* (it drains the stream before a failing return: d_remap is freed here) */
        return wavefront_motion(&s->wf, P, s->sel, prev->d, d_remap, (float*)device_pixels, stream, trace_ms);
    });
}

static int vectors_check(const void* mv8, const void* gb12, const ftn_camera_desc* cur, const ftn_camera_desc* prev, const ftn_film_desc* film, int32_t w, int32_t h,
                         const void* out, MvFrame* F) {
    if (!mv8 || !gb12 || !cur || !prev || !film || !out) return fail(FTN_ERR_INVALID_ARGUMENT, "null argument");
    if (int rc = image_check(w, h)) return rc;
    if ((int64_t)film->crop[2] - (int64_t)film->crop[0] != w || (int64_t)film->crop[3] - (int64_t)film->crop[1] != h)
        return fail(FTN_ERR_INVALID_ARGUMENT, "the film's crop is not w x h pixels");
    F->cur = tp_camera(*cur); F->prev = tp_camera(*prev);
    F->w = w; F->h = h; F->x0 = film->crop[0]; F->y0 = film->crop[1];
    return FTN_OK;
}

}  // namespace

extern "C" {

static_assert(sizeof(ftn_motion_pixel) == 32, "ABI");
int ftn_motion_abi_version(void) { return FTN_MOTION_ABI_VERSION; }

int ftn_render_motion_device(const ftn_scene* cs, const ftn_scene* prev, const ftn_camera_desc* cam, const ftn_film_desc* film, const ftn_sampler_desc* sd,
                             const ftn_tile_range* tr, const ftn_render_options* opt, void* device_pixels, void* stream, ftn_stats* st) {
    std::vector<uint32_t> remap;
    if (int no = motion_refusals(cs, prev, cam, film, sd, opt, device_pixels, &remap)) return no;
    return render_motion_device(cs, prev, remap, cam, film, sd, tr, opt, device_pixels, stream, st);
}

int ftn_render_motion(const ftn_scene* cs, const ftn_scene* prev, const ftn_camera_desc* cam, const ftn_film_desc* film, const ftn_sampler_desc* sd,
                      const ftn_tile_range* tr, const ftn_render_options* opt, ftn_motion_pixel* out_pixels, ftn_stats* st) {
    std::vector<uint32_t> remap;
    if (int no = motion_refusals(cs, prev, cam, film, sd, opt, out_pixels, &remap)) return no;
    if (int rc = bind_scene_device(cs, opt)) return rc;
    return continue_on_device(out_pixels, crop_pixels(film), [&](void* d) { return render_motion_device(cs, prev, remap, cam, film, sd, tr, opt, d, nullptr, st); });
}

int ftn_motion_resolve(const ftn_motion_pixel* in, size_t n, float* mv8) {
    if (n && (!in || !mv8)) return fail(FTN_ERR_INVALID_ARGUMENT, "null argument");
    for (size_t i = 0; i < n; i++) motion_resolve_pixel(in[i].prev_position, mv8 + 8 * i);
    return FTN_OK;
}

int ftn_motion_resolve_device(const void* in, size_t n, void* mv8, void* stream) {
    if (n && (!in || !mv8)) return fail(FTN_ERR_INVALID_ARGUMENT, "null argument");
    if (int no = need_device()) return no;
    return launched(launch_motion_resolve((const float*)in, n, (float*)mv8, (hipStream_t)stream), "motion resolve");
}

int ftn_motion_vectors_device(const void* mv8, const void* gb12, const ftn_camera_desc* cur, const ftn_camera_desc* prev, const ftn_film_desc* film,
                              int32_t w, int32_t h, void* out2, void* stream) {
    MvFrame F;
    if (int rc = vectors_check(mv8, gb12, cur, prev, film, w, h, out2, &F)) return rc;
    if (int no = need_device()) return no;
    return launched(launch_motion_vectors((const float*)mv8, (const float*)gb12, F, (float*)out2, (hipStream_t)stream), "motion vectors");
}

int ftn_motion_vectors(const float* mv8, const float* gb12, const ftn_camera_desc* cur, const ftn_camera_desc* prev, const ftn_film_desc* film,
                       int32_t w, int32_t h, float* out2, int32_t device) {
    MvFrame F;
    int rc = vectors_check(mv8, gb12, cur, prev, film, w, h, out2, &F); if (rc) return rc;
    if ((rc = need_device()) || (rc = set_device(device))) return rc;
    const size_t n = (size_t)w * (size_t)h;
    StageBufs bufs;
    float *d_mv, *d_gb, *d_out;
    if ((rc = bufs.upload(mv8, 8 * n, &d_mv)) || (rc = bufs.upload(gb12, 12 * n, &d_gb)) || (rc = bufs.alloc(2 * n, &d_out))) return rc;
    if ((rc = ftn_motion_vectors_device(d_mv, d_gb, cur, prev, film, w, h, d_out, nullptr))) return rc;
    return bufs.copy_back(out2, d_out, 2 * n);
}

int ftn_motion_vectors_cpu(const float* mv8, const float* gb12, const ftn_camera_desc* cur, const ftn_camera_desc* prev, const ftn_film_desc* film,
                           int32_t w, int32_t h, float* out2) {
    MvFrame F;
    if (int rc = vectors_check(mv8, gb12, cur, prev, film, w, h, out2, &F)) return rc;
    const size_t n = (size_t)w * (size_t)h;
    parallel_for(n, [&](size_t i0, size_t i1) {
        for (size_t i = i0; i < i1; i++) motion_vector_pixel(mv8, gb12, F, (int)(i % (size_t)w), (int)(i / (size_t)w), out2);
    });
    return FTN_OK;
}

int ftn_temporal_accumulate_motion_device(const void* rgb, const void* gb12, const void* var4, const void* mv8, const ftn_camera_desc* cur_camera,
                                          const ftn_film_desc* film, int32_t w, int32_t h, const ftn_camera_desc* prev_camera, const void* prev_gb12,
                                          const void* prev_history, const ftn_temporal_params* p, void* out_history, void* out_rgb, void* out_var4, void* stream) {
    return tp_accumulate_device(rgb, gb12, var4, mv8, cur_camera, film, w, h, prev_camera, prev_gb12, prev_history, p, out_history, out_rgb, out_var4, stream);
}

int ftn_temporal_accumulate_motion(const float* rgb, const float* gb12, const float* var4, const float* mv8, const ftn_camera_desc* cur_camera,
                                   const ftn_film_desc* film, int32_t w, int32_t h, const ftn_camera_desc* prev_camera, const float* prev_gb12,
                                   const ftn_temporal_pixel* prev_history, const ftn_temporal_params* p, ftn_temporal_pixel* out_history, float* out_rgb,
                                   float* out_var4, int32_t device) {
    return tp_accumulate_host(rgb, gb12, var4, mv8, cur_camera, film, w, h, prev_camera, prev_gb12, prev_history, p, out_history, out_rgb, out_var4, device);
}

int ftn_temporal_accumulate_motion_cpu(const float* rgb, const float* gb12, const float* var4, const float* mv8, const ftn_camera_desc* cur_camera,
                                       const ftn_film_desc* film, int32_t w, int32_t h, const ftn_camera_desc* prev_camera, const float* prev_gb12,
                                       const ftn_temporal_pixel* prev_history, const ftn_temporal_params* p, ftn_temporal_pixel* out_history, float* out_rgb,
                                       float* out_var4) {
    return tp_accumulate_cpu(rgb, gb12, var4, mv8, cur_camera, film, w, h, prev_camera, prev_gb12, prev_history, p, out_history, out_rgb, out_var4);
}

}  /* extern "C" */
