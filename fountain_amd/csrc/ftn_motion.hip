/*
 * ftn_motion.hip -- the previous-position pass (include/fountain_hip_motion.h) on the wavefront pipeline, its resolve and the motion
 * vectors (the motion-aware temporal kernel is ftn_temporal.hip's, instantiated with mv8).
 *
 * A unit of its own, like ftn_gbuffer.hip: k_mv_shade is here and shares ftn_wf_common.h with the beauty's kernels; the passes and their
 * pass-through rounds are wf_first_hit_passes' (ftn_wf_internal.h, ftn_wavefront.hip), which wavefront_motion hands the launches of
 * k_mv_shade and of the shared film's accumulate kernel (ftn_firsthit.h) for MvFilm.  The image-space kernels at the end need no scene
 * internals: their per-pixel code is ftn_motion.h's, shared with the host twins.
 */
#include "ftn_firsthit.h"
#include "ftn_motion.h"
#include <cstring>

namespace ftn {

/* ================================================================== previous positions (include/fountain_hip_motion.h)
 * The camera samples and the recorded surface are the G-buffer's (ftn_gbuffer.hip): k_mv_shade is k_gb_shade with another record.  For
 * the surface it records it builds the interaction of the corresponding primitive of the previous scene at the hit's barycentrics
 * (tri_interaction on the previous DScene: the expressions of a real hit) or carries a sphere's point and normal through the two
 * scenes' transforms.  k_fh_accumulate<MvFilm> then adds the pass's samples of every pixel in sample order. */
struct MvParams {
    FhFilm film;          /* 8 floats per crop pixel (ftn_motion_pixel); 2 float4 per path: {p', hit ? 1 : 0} {ns', 0} */
    DScene prev;          /* the previous scene's arrays */
    const uint32_t* remap;   /* per primitive of P.S in BVH order: prev's BVH index of the same primitive | MV_REMAP_COPY (validated on the host) */
};
struct MvFilm {           /* sums: p', ns', hit weight, weight */
    static constexpr int OUT = 8, SUMS = 8;
    static constexpr uint32_t REC = 2, CHUNK = 4;
    __device__ static float4 load(const FhFilm& G, const WfBuffers&, size_t p, uint32_t j) { return G.rec[2 * p + j]; }
    __device__ static bool unpack(const float4* r, float* v, uint32_t* adds) {
        v[0] = r[0].x; v[1] = r[0].y; v[2] = r[0].z; v[3] = r[1].x; v[4] = r[1].y; v[5] = r[1].z;
        *adds = ~0u;
        return r[0].w != 0.0f;
    }
};
static_assert(sizeof(RenderParams) + sizeof(WfBuffers) + sizeof(MvParams) + 64 <= 4096, "the kernel arguments of k_mv_shade");

/* a sphere's point and shading normal in the previous scene: to object space through the current sphere's transforms, back to the world
 * through the previous sphere's (the normal with transform_normal's inverse matrices: object_to_world.m stands for world_to_object's) */
__device__ inline void mv_sphere_prev(const DSphere& cur, const DSphere& prev, V3 p, V3 ns, V3* p_prev, V3* ns_prev) {
    const V3 p_obj = m4_point(cur.w2o, p);
    *p_prev = m4_point(prev.o2w, p_obj);
    const V3 n_obj = m4_normal(cur.o2w, ns);
    *ns_prev = normalize(m4_normal(prev.o2w_inv, n_obj));
}

/* one thread per queued ray: the hit it found is either recorded or passed through */
__global__ void __launch_bounds__(256) k_mv_shade(RenderParams P, WfBuffers W, MvParams G, const uint32_t* __restrict__ q_in, const uint32_t* count_in,
                                                  uint32_t* q_out, uint32_t* count_out) {
    const DScene& S = P.S;
    const uint32_t qi = blockIdx.x * 256u + threadIdx.x;
    bool push = false;
    uint32_t p = 0;
    if (qi < *count_in) {
        p = q_in[qi];
        DRay ray0; DHit h; DSI si;
        const FhHit found = fh_first_hit(S, W, p, &ray0, &h, &si);
        push = found == FH_THROUGH;
        float4 r0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), r1 = r0;       /* a miss */
        if (found == FH_SURFACE) {
            const uint32_t rm = G.remap[h.prim];
            V3 pp = si.hit.p, nn = si.shading_n;                     /* MV_REMAP_COPY: a sphere that stands as it stood */
            if (!(rm & MV_REMAP_COPY)) {
                DHit hp = h; hp.prim = (int)rm;
                const float4 g0 = S.srec ? S.srec[8 * (size_t)h.prim] : S.geom[S.geom_stride * h.prim];
                if (__float_as_uint(g0.w) & GF_KIND_SPHERE) {
                    const uint32_t ic = __float_as_uint(S.geom[S.geom_stride * h.prim + 1].w), ip = __float_as_uint(G.prev.geom[G.prev.geom_stride * hp.prim + 1].w);
                    mv_sphere_prev(S.spheres[ic], G.prev.spheres[ip], si.hit.p, si.shading_n, &pp, &nn);
                } else {
                    DSI sp; tri_interaction(G.prev, hp, ray0.d, ray0.time, &sp);
                    pp = sp.hit.p; nn = sp.shading_n;
                }
            }
            r0 = make_float4(pp.x, pp.y, pp.z, 1.0f);
            r1 = make_float4(nn.x, nn.y, nn.z, 0.0f);
        }
        if (!push) { float4* R = G.film.rec + 2 * (size_t)p; R[0] = r0; R[1] = r1; }
    }
    const bool pred[1] = {push};
    const uint32_t val[1] = {p};
    uint32_t* const qs[1] = {q_out};
    uint32_t* const cs[1] = {count_out};
    block_push<1>(pred, val, qs, cs);
}

int wavefront_motion(WavefrontState** state, const RenderParams& P, const std::vector<DTile>& tiles, const DScene& prev, const uint32_t* remap,
                     float* d_out, hipStream_t stream, double* trace_ms_out) {
    MvParams G;
    G.film = fh_film(P, d_out); G.prev = prev; G.remap = remap;
    WfFirstHitPass pass;
    pass.what = "the previous positions";
    pass.setup = [&](WavefrontState* st, uint32_t) { G.film.rec = st->pd; return FTN_OK; };
    pass.shade = [&](const WfBuffers& W, const uint32_t* q_in, const uint32_t* count_in, uint32_t* q_out, uint32_t* count_out, dim3 grid, hipStream_t sm) {
        hipLaunchKernelGGL(k_mv_shade, grid, dim3(256), 0, sm, P, W, G, q_in, count_in, q_out, count_out);
    };
    pass.accumulate = [&](const WfBuffers& W, dim3 grid, hipStream_t sm) { hipLaunchKernelGGL(k_fh_accumulate<MvFilm>, grid, dim3(256), 0, sm, P, W, G.film); };
    return fh_merge<MvFilm>(wf_first_hit_passes(state, P, tiles, pass, stream, trace_ms_out), P, G.film, stream);
}

/* ================================================================== resolve and motion vectors */
struct MvResolve {
    const float* in; float* mv8;
    __device__ void operator()(size_t i) const { motion_resolve_pixel(in + 8 * i, mv8 + 8 * i); }
};
hipError_t launch_motion_resolve(const float* in, size_t n, float* mv8, hipStream_t stream) { return fh_per_pixel(n, stream, MvResolve{in, mv8}); }

/* one thread per pixel over a grid-stride loop; the frame's constants, both cameras' matrices among them, are one kernel argument */
__global__ void __launch_bounds__(256) k_mv_vectors(const float* __restrict__ mv8, const float* __restrict__ gb12, MvFrame F, float* __restrict__ out2) {
    const size_t n = (size_t)F.w * (size_t)F.h;
    for (size_t i = (size_t)blockIdx.x * 256u + threadIdx.x; i < n; i += (size_t)gridDim.x * 256u)
        motion_vector_pixel(mv8, gb12, F, (int)(i % (size_t)F.w), (int)(i / (size_t)F.w), out2);
}
hipError_t launch_motion_vectors(const float* mv8, const float* gb12, const MvFrame& frame, float* out2, hipStream_t stream) {
    const size_t n = (size_t)frame.w * (size_t)frame.h;
    const unsigned grid = (unsigned)std::min<size_t>((n + 255) / 256, 4096);
    hipLaunchKernelGGL(k_mv_vectors, dim3(grid), dim3(256), 0, stream, mv8, gb12, frame, out2);
    return hipGetLastError();
}

}  // namespace ftn
