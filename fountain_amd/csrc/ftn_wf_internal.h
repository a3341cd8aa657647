/*
 * ftn_wf_internal.h -- what the units of the wavefront pipeline share on the host side, beyond the public ftn_wavefront.h:
 *
 *   ftn_wf_state.cpp      error text, knobs, WavefrontState and its buffers, the pass plan, the traversal grid
 *   ftn_wf_trace.hip      the reference-order traversal kernels, the coherence sort, launch_trace, the ray-batch entry point
 *   ftn_wf_shade.hip      k_wf_classify, k_wf_shade (path integrator), k_wf_shade_dl (direct lighting / Whitted) and k_batch_finish with
 *                         their launchers
 *   ftn_wavefront.hip     generate / reset / accumulate / serial-advance, the two render drivers and the first-hit passes' driver
 *   ftn_gbuffer.hip       the G-buffer pass: its kernels, and what it hands wf_first_hit_passes
 *   ftn_idmatte.hip       the ID-matte pass, likewise, with its foreign list, resolve and matte extraction
 *   ftn_ao.hip            the ambient-occlusion pass, likewise, with the any-hit steps between its first hits and its film sums
 *
 * The passes beside the beauty need nothing declared here: ftn_moments.hip hooks its kernel behind every pass of the public
 * wavefront_render (ftn_wavefront.h, ftn_wf_common.h), and ftn_adaptive.hip decides between rounds that are such calls.
 *
 * A kernel is launched from the unit that defines it; what another unit needs of it is a launcher declared here.  Declarations only,
 * all of hidden visibility: the library exports the C ABI alone.
 */
#ifndef FTN_WF_INTERNAL_H
#define FTN_WF_INTERNAL_H
#include "ftn_wf_common.h"
#include <functional>
#include <string>
#include <vector>

#pragma GCC visibility push(hidden)
namespace ftn {

struct WavefrontState {
    void* sort_tmp = nullptr; size_t sort_tmp_bytes = 0;
    size_t cap_paths = 0;
    void* mem[40]; int n_mem = 0;
    WfBuffers W;
    float4* br = nullptr; float4* pd = nullptr;          /* WfBuffers::br, WfBuffers::pd */
    hipEvent_t ev[64]; int n_ev = 0;
    hipStream_t side = nullptr; hipEvent_t ev_ready = nullptr, ev_side = nullptr;     /* the any-hit launches run beside the closest-hit ones */
    uint32_t* drain_sig = nullptr; uint32_t drain_seq = 0;                              /* signal memory for hipStreamWaitValue32 (NULL: not supported) */
    uint32_t* host_counters = nullptr;    /* pinned */
    int n_cu = 256;
    /* buffers of the direct-lighting / Whitted mode (grow-only): level terms, and shadow-ray records / results / queue sized for one ray per light */
    void* dl_mem[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr}; size_t dl_paths = 0; uint32_t dl_levels = 0, dl_slots = 0; bool dl_tex = false;
    /* four-box traversal (ftn_trace4.hip): launch plan of the current call and the global spill areas behind the LDS stacks */
    Trace4Plan t4; bool t4_on = false, t8_on = false, q64_on = false;
    void* ser_mem[4] = {nullptr, nullptr, nullptr, nullptr}; size_t ser_paths = 0; bool ser_tex = false; uint32_t* ser_host = nullptr;      /* tile-serial sampler on the queues: cursor, film position, retired flag, differentials */
    void* t4_spill_c = nullptr; void* t4_spill_a = nullptr; size_t t4_spill_c_bytes = 0, t4_spill_a_bytes = 0;
};

/* limits of k_wf_shade_dl that the pass plan reads: chain levels kept per path; lights under WhittedIntegrator */
#define WF_DL_MAX 8u
#define WF_WH_MAX_LIGHTS 32u     /* one bit per light in the path's pending-light word */

/* ------------------------------------------------------------------ ftn_wf_state.cpp */
/* the text wavefront_error() returns on this thread */
void wf_set_error(const std::string& msg);
#define WF_TRY(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) { wf_set_error(std::string(#expr ": ") + hipGetErrorString(e_)); return e_ == hipErrorOutOfMemory ? FTN_ERR_OUT_OF_MEMORY : FTN_ERR_NO_DEVICE; } } while (0)

/* tuning knobs (environment overrides, for experiments only): the environment is read once per entry-point call (knobs_begin), not
 * once per launch of the bounce loop */
void knobs_begin();
uint32_t knob(const char* name, uint32_t def);

int wf_state_init(WavefrontState** state);
int wf_reserve(WavefrontState* st, size_t n_paths);
void wf_free(WavefrontState* st);
/* buffers of k_wf_shade_dl for n paths, `levels` chain levels and `slots` shadow rays per path; tex: the differentials of textured scenes */
int wf_reserve_dl(WavefrontState* st, size_t n, uint32_t levels, uint32_t slots, bool tex);
void wf_free_dl(WavefrontState* st);
/* buffers of the tile-serial sampler for n_tiles tiles (WavefrontState::ser_mem); tex: the differentials of textured scenes */
int wf_reserve_serial(WavefrontState* st, uint32_t n_tiles, bool tex);
/* a grow-only device buffer: at least `need` bytes behind *p.  When the allocation fails, *p and *bytes are left zero */
int wf_grow(void** p, size_t* bytes, size_t need);

/* refuses more than 2^28 pixel slots in one call */
int wf_refuse_slots(size_t n_slots);
/* The pass plan of a call over n_slots pixel slots and total_samples samples of each: how many samples one pass takes (FTN_WF_PATHS_M,
 * at most 2^28 paths; with dl, the direct-lighting / Whitted cap on slots x paths), halved while the buffers do not fit, and those
 * buffers reserved (dl: wf_reserve_dl's too).  Refuses more than 2^28 slots and, with dl, more than 32 lights under WhittedIntegrator
 * and more slots than the lights leave room for. */
struct WfPassPlan { uint32_t samples, dl_levels, dl_slots; };
int wf_plan_passes(WavefrontState* st, const RenderParams& P, size_t n_slots, uint32_t total_samples, bool dl, WfPassPlan* plan);

/* the persistent traversal launches: dynamic LDS of a 256-thread workgroup whose lanes keep stack_entries node-stack levels each, and the
 * largest grid worth launching with it (CUs x the workgroups, at most 8, that 160 KiB of LDS hold) */
size_t wf_trace_lds(uint32_t stack_entries);
unsigned wf_trace_grid_max(const WavefrontState* st, size_t lds);

/* ------------------------------------------------------------------ ftn_wf_trace.hip */
/* Sizes the four-box kernels' launches for this call and makes sure their spill areas exist */
int trace4_prepare(WavefrontState* st, const DScene& S);
/* count: 0 = production kernels, 1 = counting build of the REFERENCE walk (node / primitive tallies equal the oracle's), 2 = counting
 * build of the production kernels (what bench.py's byte model uses).  max_rays: upper bound of the queue's length (sizes the grid). */
void launch_trace(WavefrontState* st, bool any, int count, bool spheres, unsigned grid, size_t lds, hipStream_t stream, const RenderParams& P, const WfBuffers& W,
                  const uint32_t* queue, const uint32_t* count_ptr, uint32_t* head, uint32_t max_rays, bool camera_rays = false);
/* sorts queue[0, cnt) by the rays' coherence keys into `out`; *sorted_q = out (or the queue itself when it is too short to bother) */
int sort_ray_queue(WavefrontState* st, const RenderParams& P, const WfBuffers& W, bool any, uint32_t* queue, uint32_t cnt, uint32_t* out,
                   uint32_t* k_in, uint32_t* k_out, uint32_t bits, hipStream_t stream, const uint32_t** sorted_q);
#ifdef FTN_DRAIN_PROBE
/* experiment build (tools/gpu_drain_probe.py): the bounce whose any-hit launch reports next */
void wf_set_probe_bounce(uint32_t bounce);
#endif

/* ------------------------------------------------------------------ ftn_wf_shade.hip */
/* groups the active queue in_q by shading class; drop: classes whose entries leave the queues here (late finish) */
void launch_wf_classify(const RenderParams& P, const WfBuffers& W, int in_q, uint32_t drop, unsigned grid, hipStream_t stream);
/* The path integrator's shading pass over the classified queue: one launch per material type present in the scene and one for the classes
 * without a BSDF (FTN_SHADE_SPECIALISE=0: one launch for everything).  first: the pass right behind k_wf_generate.  fixed_grid = 0: every
 * variant takes the grid its registers let the CUs hold (FTN_SHADE_GRID, FTN_SHADE_GRID_NOBSDF); != 0 (the tile-serial driver): every
 * variant launches at this grid */
void launch_wf_shade(WavefrontState* st, const RenderParams& P, const WfBuffers& W, int in_q, uint32_t first, unsigned fixed_grid, hipStream_t stream);
void launch_wf_shade_dl(bool whitted, bool tex, const RenderParams& P, const WfBuffers& W, int in_q, unsigned grid, hipStream_t stream);
/* what a batch of n closest-hit rays returns (wavefront_trace_batch): t, primitive, barycentrics, and in out24 the surface interaction */
void launch_batch_finish(const DScene& S, const float* d_rays8, uint32_t n, const float4* hit, const int* hit_prim, float* t_hit, int* prim, float* bary, float* out24, hipStream_t stream);

/* ------------------------------------------------------------------ ftn_wavefront.hip */
/* the first two launches of a pass: k_wf_reset in mode 0 (counters, queue lengths of the camera rays, camera_samples) and k_wf_generate
 * with their launch parameters */
void launch_wf_new_pass(const WfBuffers& W, DevStats* stats, hipStream_t stream);
void launch_wf_generate(const RenderParams& P, const WfBuffers& W, int write_state, hipStream_t stream);

/* What a first-hit pass (G-buffer, ID mattes) hands the driver below.  The kernels stay in the pass's unit; these launch them. */
struct WfFirstHitPass {
    const char* what;          /* "the G-buffer", "the matte": what would be incomplete after 4096 pass-through rounds */
    /* once per call, behind the pass plan: the per-path record buffer is st->pd (64 bytes per path), valid_per_sample the tiles' pixel count */
    std::function<int(WavefrontState* st, uint32_t valid_per_sample)> setup;
    /* one round's shade kernel over q_in[0, *count_in): records first hits, pushes null-material pass-throughs to q_out / *count_out */
    std::function<void(const WfBuffers& W, const uint32_t* q_in, const uint32_t* count_in, uint32_t* q_out, uint32_t* count_out, dim3 grid, hipStream_t stream)> shade;
    /* one pass's accumulate kernel: one thread per pixel slot */
    std::function<void(const WfBuffers& W, dim3 grid, hipStream_t stream)> accumulate;
    /* optional (empty for the G-buffer and the mattes, which launch nothing here): once per pass, between the last pass-through round and
     * accumulate, what the pass traces from the surfaces it recorded (ambient occlusion: its any-hit rays).  It gets what launch_trace
     * needs -- the state, the pass's buffers, the traversal's dynamic LDS and its largest grid -- and keeps its own times and counts */
    std::function<int(WavefrontState* st, const WfBuffers& W, size_t lds, unsigned trace_grid_max, hipStream_t stream)> secondary;
};
/* Renders P's sample range of the tiles' camera samples through `pass`, in the beauty's passes (wf_plan_passes without direct lighting):
 * per pass k_wf_reset, k_wf_generate, then rounds of closest-hit trace and pass.shade until no ray passed through a null material
 * (k_wf_round_reset between them; more than 4096 rounds: FTN_ERR_INTERNAL), then pass.secondary if there is one, then pass.accumulate.  Without tiles or samples it returns
 * FTN_OK before pass.setup.  *trace_ms_out: the trace launches' time.  The caller runs what follows the last pass. */
int wf_first_hit_passes(WavefrontState** state, const RenderParams& P, const std::vector<DTile>& tiles, const WfFirstHitPass& pass, hipStream_t stream, double* trace_ms_out);

}  // namespace ftn
#pragma GCC visibility pop
#endif
