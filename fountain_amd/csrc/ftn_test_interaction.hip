/*
 * ftn_test_interaction.hip -- the surface-interaction and camera test hooks (include/fountain_hip.h, ftn_test_interaction, ftn_test_camera):
 * kernels, launches and C entry points in a unit of their own, as ftn_test_bsdf.hip and ftn_test_light.hip, so that the sources of the render
 * kernels stay as they were profiled.
 * k_test_interaction intersects ONE primitive per row as shape_pdf_from_ref does (tri_hit + tri_uv_degenerate_reject, or sphere_intersect), then
 * calls make_interaction, compute_tex_diffs, spawn_ray and specular_diff of ftn_device.h / ftn_texture.h as the shade kernels do.
 * k_test_camera calls camera_ray and camera_ray_diff on a DCamera built by render_params, the host code of ftn_render.
 *
 * Why no row can leave a table (the host entry point refuses a primitive index outside [0, n_prims) before the launch):
 *   geom[geom_stride * prim + 0..2]  geom is the dense array of 3 * n_prims float4 (stride 3) or the shading records themselves (stride 8,
 *                                    8 * n_prims float4): ftn_scene_create uploads one or the other for every scene with primitives;
 *   srec[8 * prim + 0..6]            8 * n_prims float4 whenever the pointer is not null;
 *   spheres[bits(g1.w)]              g1.w of a sphere's record is ftn_prim::shape_index, which ftn_scene_create refuses unless < n_spheres;
 *   prim_info[2 * prim + 0..1]       read without shading records, or for a primitive with GF_HAS_TANGENTS: resident (2 * n_prims uint4) in
 *                                    exactly those scenes (no records, or some mesh has tangents);
 *   N / UV / T[3 | 2 * vertex]       vertex indices are refused at scene creation unless < n_vertices; N and UV are read only under the flag
 *                                    that says the scene has them and only without records (then resident, n_vertices entries); T only
 *                                    under GF_HAS_TANGENTS, which is set only when the scene has tangents, and then T holds n_vertices entries.
 * Rows are read and written at 32 * i and 68 * i floats of buffers of 32 * n and 68 * n floats, i < n.
 */
#include "ftn_test_rows.h"
#include "ftn_texture.h"

#include <cstring>

namespace ftn {

__device__ inline void put3(float* o, V3 v) { o[0] = v.x; o[1] = v.y; o[2] = v.z; }

__global__ void __launch_bounds__(256) k_test_interaction(DScene S, const float* __restrict__ in32, size_t n, float* __restrict__ out68) {
    const size_t stride = (size_t)gridDim.x * 256;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
        const float* r = in32 + FTN_TEST_INTERACTION_IN * i;
        float* o = out68 + FTN_TEST_INTERACTION_OUT * i;
        for (int k = 0; k < FTN_TEST_INTERACTION_OUT; k++) o[k] = 0.0f;
        DRay ray; ray.o = V3(r[0], r[1], r[2]); ray.d = V3(r[3], r[4], r[5]); ray.t_max = r[6]; ray.time = r[7];
        const int prim = (int)__float_as_uint(r[8]);
        DRayDiff rd; rd.has = r[9] != 0.0f;
        rd.rxo = V3(r[10], r[11], r[12]); rd.ryo = V3(r[13], r[14], r[15]); rd.rxd = V3(r[16], r[17], r[18]); rd.ryd = V3(r[19], r[20], r[21]);
        const V3 wi(r[22], r[23], r[24]); const float bsdf_eta = r[25]; const bool reflect = r[26] != 0.0f;

        const float4 g0 = S.geom[S.geom_stride * prim];
        DHit h; h.prim = prim; h.t = 0.0f; h.b0 = h.b1 = h.b2 = 0.0f;
        if (__float_as_uint(g0.w) & GF_KIND_SPHERE) {
            const float4 g1 = S.geom[S.geom_stride * prim + 1];
            if (!sphere_intersect<false>(S.spheres[__float_as_uint(g1.w)], ray, &h.t, nullptr)) continue;
        } else {
            V3 p0, p1, p2; uint32_t fl; load_tri(S, prim, &p0, &p1, &p2, &fl);
            if (!tri_hit(ray.o, ray.d, ray.t_max, p0, p1, p2, &h.t, &h.b0, &h.b1, &h.b2)) continue;
            if ((fl & GF_HAS_UVS) && tri_uv_degenerate_reject(S, prim, p0, p1, p2)) continue;
        }
        DSI si; DSIX ex;
        if (!make_interaction(S, h, ray, &si, &ex)) continue;
        const DTexDiffs td = compute_tex_diffs(si.hit.p, si.hit.n, ex.dpdu, ex.dpdv, rd);
        const DRay out_ray = spawn_ray(si.hit, wi);
        const DRayDiff bd = specular_diff(reflect, rd, si.hit.p, si.wo, wi, si.shading_n, ex.dndu, ex.dndv, td, bsdf_eta);
        o[0] = 1.0f; o[1] = h.t; o[2] = h.b0; o[3] = h.b1; o[4] = h.b2;
        put3(o + 5, si.hit.p); put3(o + 8, si.hit.p_err); put3(o + 11, si.hit.n); o[14] = si.hit.time;
        put3(o + 15, si.wo); put3(o + 18, si.shading_n); put3(o + 21, si.s_dpdu);
        o[24] = __uint_as_float((uint32_t)si.mat); o[25] = __uint_as_float((uint32_t)si.light);
        o[26] = ex.uv.x; o[27] = ex.uv.y; put3(o + 28, ex.dpdu); put3(o + 31, ex.dpdv); put3(o + 34, ex.dndu); put3(o + 37, ex.dndv);
        put3(o + 40, td.dpdx); put3(o + 43, td.dpdy); o[46] = td.dudx; o[47] = td.dvdx; o[48] = td.dudy; o[49] = td.dvdy;
        put3(o + 50, out_ray.o); o[53] = out_ray.t_max;
        if (bd.has) { put3(o + 54, bd.rxo); put3(o + 57, bd.ryo); put3(o + 60, bd.rxd); put3(o + 63, bd.ryd); }
    }
}

__global__ void __launch_bounds__(256) k_test_camera(DCamera C, float spp_scale, const float* __restrict__ in8, size_t n, float* __restrict__ out20) {
    const size_t stride = (size_t)gridDim.x * 256;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
        const float* r = in8 + FTN_TEST_CAMERA_IN * i;
        float* o = out20 + FTN_TEST_CAMERA_OUT * i;
        const V2 p_film(r[0], r[1]), p_lens(r[2], r[3]);
        const DRay ray = camera_ray(C, p_film, p_lens, r[4]);
        const DRayDiff rd = camera_ray_diff(C, p_film, p_lens, ray, spp_scale);
        put3(o, ray.o); put3(o + 3, ray.d); o[6] = ray.t_max; o[7] = ray.time;
        put3(o + 8, rd.rxo); put3(o + 11, rd.ryo); put3(o + 14, rd.rxd); put3(o + 17, rd.ryd);
    }
}

}  // namespace ftn

using namespace ftn;

extern "C" int ftn_test_interaction(const ftn_scene* cs, const float* rows_in, size_t n, float* rows_out) {
    if (!cs || !rows_in || !rows_out) return fail(FTN_ERR_INVALID_ARGUMENT, "null argument");
    for (size_t i = 0; i < n; i++) {
        uint32_t prim; memcpy(&prim, rows_in + FTN_TEST_INTERACTION_IN * i + 8, 4);
        if (prim >= cs->d.n_prims) return fail(FTN_ERR_INVALID_ARGUMENT, "primitive index out of range");
    }
    return test_rows(cs->device, n, {{rows_in, FTN_TEST_INTERACTION_IN}}, rows_out, FTN_TEST_INTERACTION_OUT,
                     [&](const float* const* in, float* dout) { hipLaunchKernelGGL(k_test_interaction, dim3(blocks_for(n)), dim3(256), 0, 0, cs->d, in[0], n, dout); });
}

extern "C" int ftn_test_camera(const ftn_camera_desc* cam, uint32_t spp, const float* rows_in, size_t n, float* rows_out) {
    if (!cam || !rows_in || !rows_out) return fail(FTN_ERR_INVALID_ARGUMENT, "null argument");
    if (spp == 0) return fail(FTN_ERR_INVALID_ARGUMENT, "samples per pixel must be positive");
    if (n == 0) return FTN_OK;
    /* render_params wants a scene, a film, a sampler and an integrator beside the camera: empty ones, only its DCamera is used */
    ftn_scene none; memset(&none.d, 0, sizeof(none.d));
    ftn_film_desc film; memset(&film, 0, sizeof(film));
    ftn_sampler_desc sd; memset(&sd, 0, sizeof(sd)); sd.samples_per_pixel = spp;
    ftn_integrator_desc id; memset(&id, 0, sizeof(id));
    const RenderParams P = render_params(&none, cam, &film, &sd, &id);
    return test_rows(-1, n, {{rows_in, FTN_TEST_CAMERA_IN}}, rows_out, FTN_TEST_CAMERA_OUT,
                     [&](const float* const* in, float* dout) { hipLaunchKernelGGL(k_test_camera, dim3(blocks_for(n)), dim3(256), 0, 0, P.C, 1.0f / sqrtf((float)P.spp), in[0], n, dout); });
}
