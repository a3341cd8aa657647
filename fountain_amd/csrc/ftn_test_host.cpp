/*
 * ftn_test_host.cpp -- the C entry points of the two test hooks whose kernels live beside the render kernels (ftn_kernels.hip):
 * ftn_test_math (the deterministic math functions on the device) and ftn_test_texture_eval (Texture::evaluate on the device for rows of
 * (u, v, dudx, dvdx, dudy, dvdy)).  Both report a missing device even when they are given no rows.
 */
#include "ftn_test_rows.h"

using namespace ftn;

extern "C" {

int ftn_test_math(int which, const float* x, const float* y, size_t n, float* out) {
    int rc = set_device(-1); if (rc) return rc;
    return test_rows(-1, n, {{x, 1}, {y, 1}}, out, 1, [&](const float* const* in, float* dout) { launch_test_math(which, in[0], in[1], n, dout, 0); });
}

int ftn_test_texture_eval(const ftn_scene* cs, int32_t texture, const float* uv_diffs6, size_t n, float* rgb_out) {
    if (!cs || !uv_diffs6 || !rgb_out) return fail(FTN_ERR_INVALID_ARGUMENT, "null argument");
    if (texture < 0 || (uint32_t)texture >= cs->d.n_textures) return fail(FTN_ERR_INVALID_ARGUMENT, "texture index out of range");
    int rc = set_device(cs->device); if (rc) return rc;
    return test_rows(cs->device, n, {{uv_diffs6, 6}}, rgb_out, 3, [&](const float* const* in, float* dout) { launch_test_texture_eval(cs->d, texture, in[0], n, dout, 0); });
}

}  /* extern "C" */
