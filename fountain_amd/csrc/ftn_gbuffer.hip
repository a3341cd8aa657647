/*
 * ftn_gbuffer.hip -- the first-hit G-buffer pass (include/fountain_hip_gbuffer.h) on the wavefront pipeline.
 *
 * A unit of its own: the kernels are here and share ftn_wf_common.h with the beauty's; the passes and their pass-through rounds are
 * wf_first_hit_passes' (ftn_wf_internal.h, ftn_wavefront.hip), which wavefront_gbuffer hands the launches of k_gb_shade and k_gb_accumulate.
 */
#include "ftn_wf_internal.h"
#include "ftn_texture.h"
#include "ftn_gbuffer.h"
#include <algorithm>
#include <cstring>

namespace ftn {

/* ================================================================== first-hit G-buffer (include/fountain_hip_gbuffer.h)
 * The camera samples of ftn_render for the same sampler, tiles and film: k_wf_generate makes the camera rays from the sample keys, the
 * production closest-hit kernels trace them, and k_gb_shade records the first surface that has a material.  A null-material hit spawns
 * the ray on along the same direction (path.rs:77-80) into the other queue and the round repeats (wf_first_hit_passes).
 * k_gb_accumulate then adds the pass's samples of every pixel in sample order, as k_wf_accumulate adds the beauty's. */
struct GbParams {
    float w2c[16];        /* camera_to_world.inv: camera-space z of a hit (transform.rs:224) */
    float* out;           /* 12 floats per crop pixel (ftn_gbuffer_pixel), added into */
    float4 *spillA, *spillB, *spillC;   /* per crop pixel, the samples whose footprint leaves their own pixel (atomics; added into out at the end):
                                         * {albedo, hit weight} {shading normal, weight} {p, camera-space z} */
    float4* rec;          /* 3 float4 per path: {albedo, hit ? 1 : 0} {shading normal, camera-space z} {p, 0} */
};

/* the albedo the first BSDF of the beauty is built from: each parameter clamped as compute_scattering_functions clamps it */
__device__ inline Rgb gb_albedo(const ftn_material& m) {
    const Rgb a(m.a[0], m.a[1], m.a[2]), b(m.b[0], m.b[1], m.b[2]);
    switch (m.type) {
        case FTN_MAT_MATTE: return clamp_positive(a);                              /* matte.rs:39 */
        case FTN_MAT_MIRROR: return clamp_positive(a);                             /* mirror.rs:24 */
        case FTN_MAT_METAL: return fresnel_conductor(1.0f, Rgb(1.0f), a, b);       /* FresnelConductor{1, eta, k} at normal incidence */
        case FTN_MAT_PLASTIC: return a + b;                                        /* plastic.rs:27-32: not clamped */
        default: return clamp_positive(a) + clamp_positive(b);                     /* glass.rs:54-55 */
    }
}

/* one thread per queued ray: the hit it found is either recorded or passed through */
template <bool TEX>
__global__ void __launch_bounds__(256) k_gb_shade(RenderParams P, WfBuffers W, GbParams G, const uint32_t* __restrict__ q_in, const uint32_t* count_in,
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
        float4 r0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), r1 = r0, r2 = r0;       /* a miss */
        if (h.prim >= 0) {
            DSI si; make_interaction(S, h, ray0, &si);
            if (si.mat < 0) {
                const DRay nr = spawn_ray(si.hit, ray0.d);
                W.ray[2 * (size_t)p] = make_float4(nr.o.x, nr.o.y, nr.o.z, 0.0f); W.ray[2 * (size_t)p + 1] = make_float4(nr.d.x, nr.d.y, nr.d.z, nr.t_max);
                push = true;
            } else {
                ftn_material m = S.materials[si.mat];
                if (TEX && material_is_textured(S, si.mat)) {
                    /* the camera ray's differentials, as the beauty's first shading pass rebuilds them (k_wf_shade): the path integrator hands
                     * them on unchanged through null-material pass-throughs */
                    const uint32_t slot = p / W.samples, sidx = p % W.samples;
                    const DTile tile = P.tiles[slot >> 8];
                    const int px = tile.x0 + (int)(slot & 15u), py = tile.y0 + (int)((slot >> 4) & 15u);
                    Rng crng; crng.seed(indexed_key(P.seed, px, py, W.first_sample + sidx));
                    const V2 j = crng.next2(); const V2 p_film((float)px + j.x, (float)py + j.y); const V2 p_lens = crng.next2(); const float time_u = crng.next();
                    const DRay cam = camera_ray(P.C, p_film, p_lens, time_u);
                    const DRayDiff rd = camera_ray_diff(P.C, p_film, p_lens, cam, 1.0f / sqrtf((float)P.spp));
                    DSIX ex; DSI s2; make_interaction(S, h, ray0, &s2, &ex);
                    const DTexDiffs td = compute_tex_diffs(si.hit.p, si.hit.n, ex.dpdu, ex.dpdv, rd);
                    m = material_resolve(S, si.mat, ex.uv, td);
                }
                const Rgb alb = gb_albedo(m);
                const V3 pc = m4_point(G.w2c, si.hit.p);
                r0 = make_float4(alb.r, alb.g, alb.b, 1.0f);
                r1 = make_float4(si.shading_n.x, si.shading_n.y, si.shading_n.z, pc.z);
                r2 = make_float4(si.hit.p.x, si.hit.p.y, si.hit.p.z, 0.0f);
            }
        }
        if (!push) { float4* R = G.rec + 3 * (size_t)p; R[0] = r0; R[1] = r1; R[2] = r2; }
    }
    const bool pred[1] = {push};
    const uint32_t val[1] = {p};
    uint32_t* const qs[1] = {q_out};
    uint32_t* const cs[1] = {count_out};
    block_push<1>(pred, val, qs, cs);
}

/* one sample's record into every pixel of its box-filter footprint (film_add): the own pixel in registers, others into the spill sums */
__device__ inline void gb_film_add(const GbParams& G, const FilmCtx& F, V2 p_film, float4 r0, float4 r1, float4 r2, int own_x, int own_y, float* acc, uint32_t* spill, uint32_t* bc_writes) {
    const FilmFootprint fp = film_footprint(F, p_film);
    const bool hit = r0.w != 0.0f;
    const float v[10] = {r0.x, r0.y, r0.z, r1.x, r1.y, r1.z, r2.x, r2.y, r2.z, r1.w};
    int touched = 0;
    for (int y = fp.y0; y < fp.y1; y++)
        for (int x = fp.x0; x < fp.x1; x++) {
            touched++;
            if (x == own_x && y == own_y) {
                if (hit) {
#pragma unroll
                    for (int k = 0; k < 10; k++) acc[k] += v[k] * 1.0f;       /* value * filter weight (box: 1.0) */
                    acc[10] += 1.0f;
                }
                acc[11] += 1.0f;
                continue;
            }
            const size_t i = film_idx(F, x, y);
            float* a = reinterpret_cast<float*>(G.spillA + i);
            float* b = reinterpret_cast<float*>(G.spillB + i);
            float* c = reinterpret_cast<float*>(G.spillC + i);
            if (hit) {
#pragma unroll
                for (int k = 0; k < 3; k++) { atomicAdd(a + k, v[k] * 1.0f); atomicAdd(b + k, v[3 + k] * 1.0f); atomicAdd(c + k, v[6 + k] * 1.0f); }
                atomicAdd(c + 3, v[9] * 1.0f);
                atomicAdd(a + 3, 1.0f);
            }
            atomicAdd(b + 3, 1.0f);
            (*bc_writes)++;
        }
    if (touched != 1) (*spill)++;
}

/* One thread per pixel slot adds its samples in sample order into the caller's buffer; the workgroup stages GB_ACC_CHUNK samples of its
 * 256 slots (48 bytes each, neighbours in memory) through LDS with coalesced loads, as k_wf_accumulate does. */
#define GB_ACC_CHUNK 4u
__global__ void __launch_bounds__(256) k_gb_accumulate(RenderParams P, WfBuffers W, GbParams G) {
    __shared__ float4 s_rec[256 * GB_ACC_CHUNK * 3];
    const uint32_t slot = blockIdx.x * 256u + threadIdx.x;
    uint32_t spill = 0, bc = 0;
    const FilmSlot fs = film_slot(P, W.n_slots, slot);
    const bool valid = fs.valid, in_crop = fs.in_crop; const int px = fs.px, py = fs.py; const size_t ai = fs.ai;
    float acc[12];
#pragma unroll
    for (int k = 0; k < 12; k++) acc[k] = in_crop ? G.out[12 * ai + k] : 0.0f;
    const size_t block_first = (size_t)blockIdx.x * 256u * W.samples;          /* first path of this workgroup's 256 slots */
    for (uint32_t s0 = 0; s0 < W.samples; s0 += GB_ACC_CHUNK) {
        const uint32_t n = W.samples - s0 < GB_ACC_CHUNK ? W.samples - s0 : GB_ACC_CHUNK;
        for (uint32_t e = threadIdx.x; e < 256u * 3u * n; e += 256u) {         /* the 3 n consecutive float4 of slot e / (3 n) */
            const uint32_t sl = e / (3u * n), k3 = e - sl * 3u * n;
            const size_t p = block_first + (size_t)sl * W.samples + s0 + k3 / 3u;
            if (p < W.n_paths) s_rec[sl * GB_ACC_CHUNK * 3u + k3] = G.rec[3 * p + k3 % 3u];
        }
        __syncthreads();
        if (valid) {
            for (uint32_t k = 0; k < n; k++) {
                const float4* r = &s_rec[(threadIdx.x * GB_ACC_CHUNK + k) * 3u];
                /* the sample's film position: the first two draws of its stream, exactly as k_wf_generate made them */
                Rng crng; crng.seed(indexed_key(P.seed, px, py, W.first_sample + s0 + k));
                const V2 j = crng.next2();
                gb_film_add(G, fs.F, V2((float)px + j.x, (float)py + j.y), r[0], r[1], r[2], in_crop ? px : FTN_OWN_NONE, py, acc, &spill, &bc);
            }
        }
        __syncthreads();
    }
    if (valid && in_crop) {
#pragma unroll
        for (int k = 0; k < 12; k++) G.out[12 * ai + k] = acc[k];
    }
    if (spill) atomicAdd(&P.stats->spill_samples, (unsigned long long)spill);       /* rare */
    if (bc) atomicAdd(&P.stats->bc_writes, (unsigned long long)bc);
}

/* after the last pass: the spill sums into the caller's buffer (nothing to do when no sample left its own pixel) */
__global__ void __launch_bounds__(256) k_gb_merge(GbParams G, size_t n, const DevStats* __restrict__ stats) {
    if (stats->bc_writes == 0) return;
    for (size_t i = (size_t)blockIdx.x * 256u + threadIdx.x; i < n; i += (size_t)gridDim.x * 256u) {
        const float4 a = G.spillA[i], b = G.spillB[i], c = G.spillC[i];
        if (b.w == 0.0f) continue;
        const float add[12] = {a.x, a.y, a.z, b.x, b.y, b.z, c.x, c.y, c.z, c.w, a.w, b.w};
#pragma unroll
        for (int k = 0; k < 12; k++) G.out[12 * i + k] += add[k];
    }
}

__global__ void __launch_bounds__(256) k_gb_resolve(const float* __restrict__ in, size_t n, float* __restrict__ out12) {
    for (size_t i = (size_t)blockIdx.x * 256u + threadIdx.x; i < n; i += (size_t)gridDim.x * 256u) gbuffer_resolve_pixel(in + 12 * i, out12 + 12 * i);
}
void launch_gbuffer_resolve(const float* in, size_t n, float* out12, hipStream_t stream) {
    if (n == 0) return;
    const unsigned grid = (unsigned)std::min<size_t>((n + 255) / 256, 4096);
    hipLaunchKernelGGL(k_gb_resolve, dim3(grid), dim3(256), 0, stream, in, n, out12);
}

int wavefront_gbuffer(WavefrontState** state, const RenderParams& P, const std::vector<DTile>& tiles, const float w2c[16], float* d_out,
                      float4* spill_a, float4* spill_b, float4* spill_c, hipStream_t stream, double* trace_ms_out) {
    GbParams G;
    memcpy(G.w2c, w2c, sizeof(G.w2c)); G.out = d_out; G.spillA = spill_a; G.spillB = spill_b; G.spillC = spill_c; G.rec = nullptr;
    const bool tex = P.S.n_textures != 0;
    WfFirstHitPass pass;
    pass.what = "the G-buffer";
    pass.setup = [&](WavefrontState* st, uint32_t) { G.rec = st->pd; return FTN_OK; };          /* the path integrator's 64-byte records: 3 float4 per path used */
    pass.shade = [&](const WfBuffers& W, const uint32_t* q_in, const uint32_t* count_in, uint32_t* q_out, uint32_t* count_out, dim3 grid, hipStream_t sm) {
        if (tex) hipLaunchKernelGGL(k_gb_shade<true>, grid, dim3(256), 0, sm, P, W, G, q_in, count_in, q_out, count_out);
        else hipLaunchKernelGGL(k_gb_shade<false>, grid, dim3(256), 0, sm, P, W, G, q_in, count_in, q_out, count_out);
    };
    pass.accumulate = [&](const WfBuffers& W, dim3 grid, hipStream_t sm) { hipLaunchKernelGGL(k_gb_accumulate, grid, dim3(256), 0, sm, P, W, G); };
    const int rc = wf_first_hit_passes(state, P, tiles, pass, stream, trace_ms_out);
    if (rc || !G.rec) return rc;          /* (no record buffer: no tiles or no samples, nothing was launched) */
    const size_t npix = (size_t)std::max(0, P.crop[2] - P.crop[0]) * (size_t)std::max(0, P.crop[3] - P.crop[1]);
    if (npix) hipLaunchKernelGGL(k_gb_merge, dim3((unsigned)std::min<size_t>((npix + 255) / 256, 4096)), dim3(256), 0, stream, G, npix, (const DevStats*)P.stats);
    WF_TRY(hipGetLastError());
    return FTN_OK;
}

}  // namespace ftn
