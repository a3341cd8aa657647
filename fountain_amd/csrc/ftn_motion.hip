/*
 * ftn_motion.hip -- the previous-position pass (include/fountain_hip_motion.h) on the wavefront pipeline, its resolve and the motion
 * vectors (the motion-aware temporal kernel is ftn_temporal.hip's, instantiated with mv8).
 *
 * A unit of its own, like ftn_gbuffer.hip: the kernels are here and share ftn_wf_common.h with the beauty's; the passes and their
 * pass-through rounds are wf_first_hit_passes' (ftn_wf_internal.h, ftn_wavefront.hip), which wavefront_motion hands the launches of
 * k_mv_shade and k_mv_accumulate.  The image-space kernels at the end need no scene internals: their per-pixel code is ftn_motion.h's, shared with the host twins.
 */
#include "ftn_wf_internal.h"
#include "ftn_motion.h"
#include <algorithm>
#include <cstring>

namespace ftn {

/* ================================================================== previous positions (include/fountain_hip_motion.h)
 * The camera samples and the recorded surface are the G-buffer's (ftn_gbuffer.hip): k_mv_shade is k_gb_shade with another record.  For
 * the surface it records it builds the interaction of the corresponding primitive of the previous scene at the hit's barycentrics
 * (tri_interaction on the previous DScene: the expressions of a real hit) or carries a sphere's point and normal through the two
 * scenes' transforms.  k_mv_accumulate then adds the pass's samples of every pixel in sample order, as k_gb_accumulate does. */
struct MvParams {
    DScene prev;          /* the previous scene's arrays */
    const uint32_t* remap;   /* per primitive of P.S in BVH order: prev's BVH index of the same primitive | MV_REMAP_COPY (validated on the host) */
    float* out;           /* 8 floats per crop pixel (ftn_motion_pixel), added into */
    float4 *spillA, *spillB;   /* per crop pixel, the samples whose footprint leaves their own pixel (the film rule's atomics; added into out at
                                * the end): {p', hit weight} {ns', weight} */
    float4* rec;          /* 2 float4 per path: {p', hit ? 1 : 0} {ns', 0} */
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
        const float4 ro = W.ray[2 * (size_t)p], rdv = W.ray[2 * (size_t)p + 1];
        DRay ray0; ray0.o = V3(ro.x, ro.y, ro.z); ray0.d = V3(rdv.x, rdv.y, rdv.z); ray0.t_max = rdv.w; ray0.time = 0.0f;
        const DHit h = load_hit(W, p);
        float4 r0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), r1 = r0;       /* a miss */
        if (h.prim >= 0) {
            DSI si; make_interaction(S, h, ray0, &si);
            if (si.mat < 0) {
                const DRay nr = spawn_ray(si.hit, ray0.d);
                W.ray[2 * (size_t)p] = make_float4(nr.o.x, nr.o.y, nr.o.z, 0.0f); W.ray[2 * (size_t)p + 1] = make_float4(nr.d.x, nr.d.y, nr.d.z, nr.t_max);
                push = true;
            } else {
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
        }
        if (!push) { float4* R = G.rec + 2 * (size_t)p; R[0] = r0; R[1] = r1; }
    }
    const bool pred[1] = {push};
    const uint32_t val[1] = {p};
    uint32_t* const qs[1] = {q_out};
    uint32_t* const cs[1] = {count_out};
    block_push<1>(pred, val, qs, cs);
}

/* one sample's record into every pixel of its box-filter footprint (film_add): the own pixel in registers, others into the spill sums */
__device__ inline void mv_film_add(const MvParams& G, const FilmCtx& F, V2 p_film, float4 r0, float4 r1, int own_x, int own_y, float* acc, uint32_t* spill, uint32_t* bc_writes) {
    const FilmFootprint fp = film_footprint(F, p_film);
    const bool hit = r0.w != 0.0f;
    const float v[6] = {r0.x, r0.y, r0.z, r1.x, r1.y, r1.z};
    int touched = 0;
    for (int y = fp.y0; y < fp.y1; y++)
        for (int x = fp.x0; x < fp.x1; x++) {
            touched++;
            if (x == own_x && y == own_y) {
                if (hit) {
#pragma unroll
                    for (int k = 0; k < 6; k++) acc[k] += v[k] * 1.0f;        /* value * filter weight (box: 1.0) */
                    acc[6] += 1.0f;
                }
                acc[7] += 1.0f;
                continue;
            }
            const size_t i = film_idx(F, x, y);
            float* a = reinterpret_cast<float*>(G.spillA + i);
            float* b = reinterpret_cast<float*>(G.spillB + i);
            if (hit) {
#pragma unroll
                for (int k = 0; k < 3; k++) { atomicAdd(a + k, v[k] * 1.0f); atomicAdd(b + k, v[3 + k] * 1.0f); }
                atomicAdd(a + 3, 1.0f);
            }
            atomicAdd(b + 3, 1.0f);
            (*bc_writes)++;
        }
    if (touched != 1) (*spill)++;
}

/* One thread per pixel slot adds its samples in sample order into the caller's buffer; the workgroup stages MV_ACC_CHUNK samples of its
 * 256 slots (32 bytes each, neighbours in memory) through LDS with coalesced loads, as k_gb_accumulate does. */
#define MV_ACC_CHUNK 4u
__global__ void __launch_bounds__(256) k_mv_accumulate(RenderParams P, WfBuffers W, MvParams G) {
    __shared__ float4 s_rec[256 * MV_ACC_CHUNK * 2];
    const uint32_t slot = blockIdx.x * 256u + threadIdx.x;
    uint32_t spill = 0, bc = 0;
    const FilmSlot fs = film_slot(P, W.n_slots, slot);
    const bool valid = fs.valid, in_crop = fs.in_crop; const int px = fs.px, py = fs.py; const size_t ai = fs.ai;
    float acc[8];
#pragma unroll
    for (int k = 0; k < 8; k++) acc[k] = in_crop ? G.out[8 * ai + k] : 0.0f;
    const size_t block_first = (size_t)blockIdx.x * 256u * W.samples;          /* first path of this workgroup's 256 slots */
    for (uint32_t s0 = 0; s0 < W.samples; s0 += MV_ACC_CHUNK) {
        const uint32_t n = W.samples - s0 < MV_ACC_CHUNK ? W.samples - s0 : MV_ACC_CHUNK;
        for (uint32_t e = threadIdx.x; e < 256u * 2u * n; e += 256u) {         /* the 2 n consecutive float4 of slot e / (2 n) */
            const uint32_t sl = e / (2u * n), k2 = e - sl * 2u * n;
            const size_t p = block_first + (size_t)sl * W.samples + s0 + k2 / 2u;
            if (p < W.n_paths) s_rec[sl * MV_ACC_CHUNK * 2u + k2] = G.rec[2 * p + k2 % 2u];
        }
        __syncthreads();
        if (valid) {
            for (uint32_t k = 0; k < n; k++) {
                const float4* r = &s_rec[(threadIdx.x * MV_ACC_CHUNK + k) * 2u];
                /* the sample's film position: the first two draws of its stream, exactly as k_wf_generate made them */
                Rng crng; crng.seed(indexed_key(P.seed, px, py, W.first_sample + s0 + k));
                const V2 j = crng.next2();
                mv_film_add(G, fs.F, V2((float)px + j.x, (float)py + j.y), r[0], r[1], in_crop ? px : FTN_OWN_NONE, py, acc, &spill, &bc);
            }
        }
        __syncthreads();
    }
    if (valid && in_crop) {
#pragma unroll
        for (int k = 0; k < 8; k++) G.out[8 * ai + k] = acc[k];
    }
    if (spill) atomicAdd(&P.stats->spill_samples, (unsigned long long)spill);       /* rare */
    if (bc) atomicAdd(&P.stats->bc_writes, (unsigned long long)bc);
}

/* after the last pass: the spill sums into the caller's buffer (nothing to do when no sample left its own pixel) */
__global__ void __launch_bounds__(256) k_mv_merge(MvParams G, size_t n, const DevStats* __restrict__ stats) {
    if (stats->bc_writes == 0) return;
    for (size_t i = (size_t)blockIdx.x * 256u + threadIdx.x; i < n; i += (size_t)gridDim.x * 256u) {
        const float4 a = G.spillA[i], b = G.spillB[i];
        if (b.w == 0.0f) continue;
        const float add[8] = {a.x, a.y, a.z, b.x, b.y, b.z, a.w, b.w};
#pragma unroll
        for (int k = 0; k < 8; k++) G.out[8 * i + k] += add[k];
    }
}

int wavefront_motion(WavefrontState** state, const RenderParams& P, const std::vector<DTile>& tiles, const DScene& prev, const uint32_t* remap,
                     float* d_out, float4* spill_a, float4* spill_b, hipStream_t stream, double* trace_ms_out) {
    MvParams G;
    G.prev = prev; G.remap = remap; G.out = d_out; G.spillA = spill_a; G.spillB = spill_b; G.rec = nullptr;
    WfFirstHitPass pass;
    pass.what = "the previous positions";
    pass.setup = [&](WavefrontState* st, uint32_t) { G.rec = st->pd; return FTN_OK; };          /* the path integrator's 64-byte records: 2 float4 per path used */
    pass.shade = [&](const WfBuffers& W, const uint32_t* q_in, const uint32_t* count_in, uint32_t* q_out, uint32_t* count_out, dim3 grid, hipStream_t sm) {
        hipLaunchKernelGGL(k_mv_shade, grid, dim3(256), 0, sm, P, W, G, q_in, count_in, q_out, count_out);
    };
    pass.accumulate = [&](const WfBuffers& W, dim3 grid, hipStream_t sm) { hipLaunchKernelGGL(k_mv_accumulate, grid, dim3(256), 0, sm, P, W, G); };
    const int rc = wf_first_hit_passes(state, P, tiles, pass, stream, trace_ms_out);
    if (rc || !G.rec) return rc;          /* (no record buffer: no tiles or no samples, nothing was launched) */
    const size_t npix = (size_t)std::max(0, P.crop[2] - P.crop[0]) * (size_t)std::max(0, P.crop[3] - P.crop[1]);
    if (npix) hipLaunchKernelGGL(k_mv_merge, dim3((unsigned)std::min<size_t>((npix + 255) / 256, 4096)), dim3(256), 0, stream, G, npix, (const DevStats*)P.stats);
    WF_TRY(hipGetLastError());
    return FTN_OK;
}

/* ================================================================== resolve and motion vectors */
__global__ void __launch_bounds__(256) k_mv_resolve(const float* __restrict__ in, size_t n, float* __restrict__ mv8) {
    for (size_t i = (size_t)blockIdx.x * 256u + threadIdx.x; i < n; i += (size_t)gridDim.x * 256u) motion_resolve_pixel(in + 8 * i, mv8 + 8 * i);
}
void launch_motion_resolve(const float* in, size_t n, float* mv8, hipStream_t stream) {
    if (n == 0) return;
    const unsigned grid = (unsigned)std::min<size_t>((n + 255) / 256, 4096);
    hipLaunchKernelGGL(k_mv_resolve, dim3(grid), dim3(256), 0, stream, in, n, mv8);
}

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
