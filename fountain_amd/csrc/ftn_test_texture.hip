/*
 * ftn_test_texture.hip -- the textured-material test hook (include/fountain_hip.h, ftn_test_material): kernel, launch and C entry point in a
 * unit of their own, as ftn_test_bsdf.hip, ftn_test_light.hip and ftn_test_interaction.hip, so that the sources of the render kernels stay
 * as they were profiled.
 * k_test_material does per row what the shade kernels do per hit: material_is_textured(S, mat) ? material_resolve(S, mat, uv, td) :
 * S.materials[mat] (ftn_texture.h).  A row is six floats in (u, v, dudx, dvdx, dudy, dvdy, as ftn_test_texture_eval takes them), 16 floats out.
 *
 * Why no row can leave a table (the host entry point refuses a material index outside [0, n_materials) before the launch; a row carries
 * floats only, no index):
 *   materials[mat]           n_materials records, uploaded by ftn_scene_create for every scene;
 *   mtex[mat]                read only when the pointer is not null, and then it holds n_materials records: ftn_scene_create fills a record
 *                            of five -1 for every material when the descriptor brings none;
 *   textures[id]             id is a slot of mtex[mat] that is >= 0 (a negative slot is never followed), or tex1 / tex2 of a checkerboard:
 *                            ftn_scene_create refuses a slot >= n_textures and a checkerboard child outside [0, n_textures); tex_eval follows
 *                            at most 64 children and then returns black, so a cycle of checkerboards ends as well;
 *   images[t.image]          read for FTN_TEX_IMAGE only, whose image index is refused at scene creation unless in [0, n_images);
 *   im.off / lw / lh[level]  16 entries each; ftn_scene_create refuses an image with more than 16 levels, mip_triangle clamps its level to
 *                            [0, n_levels - 1] and the top-texel read uses n_levels - 1 itself;
 *   texels[off + t * w + s]  mip_texel wraps, clamps or rejects (s, t) into [0, w) x [0, h) of the level (f2i_sat saturates the float to int
 *                            conversion, NaN -> 0, and whatever int s0 + 1 is, each of the three wrap modes brings it
 *                            inside or rejects it); a level holds w * h texels from off[level] on, and the levels lie back to back.
 * Rows are read and written at 6 * i and 16 * i floats of buffers of 6 * n and 16 * n floats, i < n.
 */
#include "ftn_test_rows.h"
#include "ftn_texture.h"

namespace ftn {

__global__ void __launch_bounds__(256) k_test_material(DScene S, int mat, const float* __restrict__ in6, size_t n, float* __restrict__ out16) {
    const size_t stride = (size_t)gridDim.x * 256;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
        const float* r = in6 + FTN_TEST_MATERIAL_IN * i;
        float* o = out16 + FTN_TEST_MATERIAL_OUT * i;
        DTexDiffs td; td.dpdx = V3(0.0f, 0.0f, 0.0f); td.dpdy = td.dpdx; td.dudx = r[2]; td.dvdx = r[3]; td.dudy = r[4]; td.dvdy = r[5];
        const bool textured = material_is_textured(S, mat);
        const ftn_material m = textured ? material_resolve(S, mat, V2(r[0], r[1]), td) : S.materials[mat];
        o[0] = textured ? 1.0f : 0.0f; o[1] = __uint_as_float((uint32_t)m.type); o[2] = __uint_as_float((uint32_t)m.remap_roughness);
        for (int k = 0; k < 3; k++) { o[3 + k] = m.a[k]; o[6 + k] = m.b[k]; }
        o[9] = m.s0; o[10] = m.s1; o[11] = m.s2;
        o[12] = o[13] = o[14] = o[15] = 0.0f;
    }
}
static void launch_test_material(const DScene& S, int mat, const float* rows_in, size_t n, float* rows_out, hipStream_t stream) {
    hipLaunchKernelGGL(k_test_material, dim3(blocks_for(n)), dim3(256), 0, stream, S, mat, rows_in, n, rows_out);
}

}  // namespace ftn

using namespace ftn;

extern "C" int ftn_test_material(const ftn_scene* cs, int32_t material, const float* rows_in, size_t n, float* rows_out) {
    if (!cs || !rows_in || !rows_out) return fail(FTN_ERR_INVALID_ARGUMENT, "null argument");
    if (material < 0 || (size_t)material >= cs->materials.n) return fail(FTN_ERR_INVALID_ARGUMENT, "material index out of range");
    return test_rows(cs->device, n, {{rows_in, FTN_TEST_MATERIAL_IN}}, rows_out, FTN_TEST_MATERIAL_OUT,
                     [&](const float* const* in, float* dout) { launch_test_material(cs->d, material, in[0], n, dout, 0); });
}
