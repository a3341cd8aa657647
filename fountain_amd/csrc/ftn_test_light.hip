/*
 * ftn_test_light.hip -- the light test hook (include/fountain_hip.h, ftn_test_light): kernel, launch and C entry point in a unit of their
 * own, as ftn_test_bsdf.hip, so that the sources of the render kernels stay as they were profiled.
 * Calls light_sample / light_pdf / light_Le_env / area_Le of ftn_device.h as the shade kernels do -- through S.lights[light], or through
 * the copy of the one infinite light in the kernel arguments (S.env0, light_sample_env / light_pdf_env) as k_wf_shade<.., ENV> does.
 * A row is 15 floats in, six float4 out.
 */
#include "ftn_test_rows.h"

namespace ftn {

__global__ void __launch_bounds__(256) k_test_light(DScene S, int light, int via_env0, const float* __restrict__ in15, size_t n, float4* __restrict__ out4) {
    const size_t stride = (size_t)gridDim.x * 256;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
        const float* r = in15 + 15 * i;
        DSurfHit ref;
        ref.p = V3(r[0], r[1], r[2]); ref.p_err = V3(r[3], r[4], r[5]); ref.n = V3(r[6], r[7], r[8]); ref.time = r[9];
        const V3 wi(r[10], r[11], r[12]); const V2 u(r[13], r[14]);
        DLiSample s; float pdf_in, pdf_s; Rgb le(0.0f);
        if (via_env0) {
            s = light_sample_env(S.env0, ref, u);
            pdf_in = light_pdf_env(S.env0, wi); pdf_s = light_pdf_env(S.env0, s.wi);
            le = light_Le_env(S.env0, wi);
        } else {
            const DLight& L = S.lights[light];
            s = light_sample(S, L, ref, u);
            pdf_in = light_pdf(S, L, ref, wi); pdf_s = light_pdf(S, L, ref, s.wi);
            if (L.kind == LK_INFINITE) le = light_Le_env(L, wi);
            else if (L.kind == LK_AREA) le = area_Le(L, s.p1.n, -s.wi);
        }
        out4[6 * i] = make_float4(s.radiance.r, s.radiance.g, s.radiance.b, s.wi.x);
        out4[6 * i + 1] = make_float4(s.wi.y, s.wi.z, s.pdf, s.p1.p.x);
        out4[6 * i + 2] = make_float4(s.p1.p.y, s.p1.p.z, s.p1.p_err.x, s.p1.p_err.y);
        out4[6 * i + 3] = make_float4(s.p1.p_err.z, s.p1.n.x, s.p1.n.y, s.p1.n.z);
        out4[6 * i + 4] = make_float4(s.p1.time, pdf_in, pdf_s, le.r);
        out4[6 * i + 5] = make_float4(le.g, le.b, 0.0f, 0.0f);
    }
}
static void launch_test_light(const DScene& S, int light, int via_env0, const float* rows_in, size_t n, float* rows_out, hipStream_t stream) {
    hipLaunchKernelGGL(k_test_light, dim3(blocks_for(n)), dim3(256), 0, stream, S, light, via_env0, rows_in, n, reinterpret_cast<float4*>(rows_out));
}

}  // namespace ftn

using namespace ftn;

extern "C" int ftn_test_light(const ftn_scene* cs, int32_t light, int via_env0, const float* rows_in, size_t n, float* rows_out) {
    if (!cs || !rows_in || !rows_out) return fail(FTN_ERR_INVALID_ARGUMENT, "null argument");
    if (light < 0 || (uint32_t)light >= cs->d.n_lights) return fail(FTN_ERR_INVALID_ARGUMENT, "light index out of range");
    if (via_env0 && !cs->d.env_only) return fail(FTN_ERR_INVALID_ARGUMENT, "via_env0 needs a scene lit by one infinite light alone");
    return test_rows(cs->device, n, {{rows_in, FTN_TEST_LIGHT_IN}}, rows_out, FTN_TEST_LIGHT_OUT,
                     [&](const float* const* in, float* dout) { launch_test_light(cs->d, light, via_env0 != 0, in[0], n, dout, 0); });
}
