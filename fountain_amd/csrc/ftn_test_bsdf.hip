/*
 * ftn_test_bsdf.hip -- the BSDF test hook (include/fountain_hip.h, ftn_test_bsdf): kernel, launch and C entry point in a unit of their
 * own, so that the sources of the render kernels stay as they were profiled (profiles/r03/traffic.json hashes them).
 * Calls make_bsdf / bsdf_f / bsdf_pdf / bsdf_sample of ftn_device.h as the shade kernels do; a row is 17 floats in, four float4 out.
 */
#include "ftn_test_rows.h"

namespace ftn {

__global__ void __launch_bounds__(256) k_test_bsdf(DScene S, int material, uint32_t flags, int allow_multiple_lobes, int specialised,
                                                   const float* __restrict__ in17, size_t n, float4* __restrict__ out4) {
    const ftn_material& m = S.materials[material];
    const size_t stride = (size_t)gridDim.x * 256;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
        const float* r = in17 + 17 * i;
        DSI si;
        si.hit.p = V3(0.0f, 0.0f, 0.0f); si.hit.p_err = si.hit.p; si.hit.time = 0.0f; si.prim = -1; si.mat = material; si.light = -1;
        si.hit.n = V3(r[0], r[1], r[2]); si.shading_n = V3(r[3], r[4], r[5]); si.s_dpdu = V3(r[6], r[7], r[8]);
        const V3 wo(r[9], r[10], r[11]), wi(r[12], r[13], r[14]); const V2 u(r[15], r[16]);
        si.wo = wo;
        DBsdf B; bool ok;
        const bool aml = allow_multiple_lobes != 0;
        if (specialised) {
            switch (m.type) {
                case FTN_MAT_MATTE: ok = make_bsdf<FTN_MAT_MATTE>(m, si, aml, &B); break;
                case FTN_MAT_METAL: ok = make_bsdf<FTN_MAT_METAL>(m, si, aml, &B); break;
                case FTN_MAT_MIRROR: ok = make_bsdf<FTN_MAT_MIRROR>(m, si, aml, &B); break;
                case FTN_MAT_PLASTIC: ok = make_bsdf<FTN_MAT_PLASTIC>(m, si, aml, &B); break;
                default: ok = make_bsdf<FTN_MAT_GLASS>(m, si, aml, &B); break;
            }
        } else ok = make_bsdf<-1>(m, si, aml, &B);
        float4 o0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), o1 = o0, o2 = o0, o3 = o0;
        if (ok) {
            const Rgb f = bsdf_f(B, wo, wi, flags);
            const float pdf = bsdf_pdf(B, wo, wi, flags);
            o0 = make_float4(1.0f, (float)bsdf_num(B, flags), f.r, f.g); o1.x = f.b; o1.y = pdf;
            DScatter s;
            if (bsdf_sample(B, wo, u, flags, &s)) {
                o1.z = 1.0f; o1.w = s.f.r;
                o2 = make_float4(s.f.g, s.f.b, s.wi.x, s.wi.y);
                o3 = make_float4(s.wi.z, s.pdf, (float)s.type, 0.0f);
            }
        }
        out4[4 * i] = o0; out4[4 * i + 1] = o1; out4[4 * i + 2] = o2; out4[4 * i + 3] = o3;
    }
}
static void launch_test_bsdf(const DScene& S, int material, uint32_t flags, int allow_multiple_lobes, int specialised, const float* rows_in, size_t n,
                             float* rows_out, hipStream_t stream) {
    hipLaunchKernelGGL(k_test_bsdf, dim3(blocks_for(n)), dim3(256), 0, stream, S, material, flags, allow_multiple_lobes, specialised, rows_in, n,
                       reinterpret_cast<float4*>(rows_out));
}

}  // namespace ftn

using namespace ftn;

extern "C" int ftn_test_bsdf(const ftn_scene* cs, int32_t material, uint32_t flags, int allow_multiple_lobes, int specialised, const float* rows_in, size_t n, float* rows_out) {
    if (!cs || !rows_in || !rows_out) return fail(FTN_ERR_INVALID_ARGUMENT, "null argument");
    if (material < 0 || (size_t)material >= cs->materials.n) return fail(FTN_ERR_INVALID_ARGUMENT, "material index out of range");
    if (flags > 31u) return fail(FTN_ERR_INVALID_ARGUMENT, "flags hold bits outside BxDFType");
    int rc = set_device(cs->device); if (rc) return rc;
    if (cs->mtex.n) {                                  /* a textured material is stored raw and resolved per hit: not this hook's business */
        ftn_material_textures mt;
        hipError_t e = hipMemcpy(&mt, cs->mtex.p + material, sizeof(mt), hipMemcpyDeviceToHost);
        if (e != hipSuccess) return fail(FTN_ERR_NO_DEVICE, hipGetErrorString(e));
        if ((mt.a & mt.b & mt.s0 & mt.s1 & mt.s2) >= 0) return fail(FTN_ERR_UNSUPPORTED, "ftn_test_bsdf takes materials with constant parameters only");
    }
    return test_rows(cs->device, n, {{rows_in, FTN_TEST_BSDF_IN}}, rows_out, FTN_TEST_BSDF_OUT,
                     [&](const float* const* in, float* dout) { launch_test_bsdf(cs->d, material, flags, allow_multiple_lobes, specialised, in[0], n, dout, 0); });
}
