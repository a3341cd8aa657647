/*
 * ftn_wf_state.cpp -- host-side state of the wavefront pipeline, shared by its units through ftn_wf_internal.h: the error text, the
 * knob cache, WavefrontState and the buffers it owns, the pass plan and the grid of the persistent traversal launches.  No kernels.
 */
#include "ftn_wf_internal.h"
#include <algorithm>
#include <cstdlib>
#include <string>
#include <unordered_map>

namespace ftn {

static thread_local std::string g_wf_err;
const char* wavefront_error() { return g_wf_err.c_str(); }
void wf_set_error(const std::string& msg) { g_wf_err = msg; }

/* a grow-only device buffer: the old one is released first, and a failed allocation leaves pointer and size zero */
int wf_grow(void** p, size_t* bytes, size_t need) {
    if (need <= *bytes) return FTN_OK;
    if (*p) (void)hipFree(*p);
    *p = nullptr; *bytes = 0;
    WF_TRY(hipMalloc(p, need));
    *bytes = need;
    return FTN_OK;
}

size_t wf_trace_lds(uint32_t stack_entries) { return (size_t)stack_entries * 256 * sizeof(uint32_t); }
unsigned wf_trace_grid_max(const WavefrontState* st, size_t lds) {
    const unsigned blocks_per_cu = (unsigned)std::max<size_t>(1, std::min<size_t>(8, (size_t)(160 * 1024) / std::max<size_t>(lds, 1)));
    return (unsigned)st->n_cu * blocks_per_cu;
}

void wf_free(WavefrontState* st) { for (int i = 0; i < st->n_mem; i++) (void)hipFree(st->mem[i]); st->n_mem = 0; st->cap_paths = 0; }
void wavefront_destroy(WavefrontState* st) {
    if (!st) return;
    wf_free(st);
    if (st->sort_tmp) (void)hipFree(st->sort_tmp);
    for (int i = 0; i < st->n_ev; i++) (void)hipEventDestroy(st->ev[i]);
    if (st->ev_ready) (void)hipEventDestroy(st->ev_ready);
    if (st->ev_side) (void)hipEventDestroy(st->ev_side);
    if (st->side) (void)hipStreamDestroy(st->side);
    if (st->drain_sig) (void)hipFree(st->drain_sig);
    for (void* m : st->dl_mem) if (m) (void)hipFree(m);
    for (void* m : st->ser_mem) if (m) (void)hipFree(m);
    if (st->t4_spill_c) (void)hipFree(st->t4_spill_c);
    if (st->t4_spill_a) (void)hipFree(st->t4_spill_a);
    if (st->host_counters) (void)hipHostFree(st->host_counters);
    if (st->ser_host) (void)hipHostFree(st->ser_host);
    delete st;
}
template <class T> static int wf_alloc(WavefrontState* st, T** p, size_t n) {
    WF_TRY(hipMalloc((void**)p, n * sizeof(T)));
    st->mem[st->n_mem++] = (void*)*p;
    return FTN_OK;
}
int wf_reserve(WavefrontState* st, size_t n) {
    if (n <= st->cap_paths) return FTN_OK;
    wf_free(st);
    WfBuffers& W = st->W; int rc;
    if ((rc = wf_alloc(st, &W.ray, 4 * n)) || (rc = wf_alloc(st, &W.hit, 2 * n)) || (rc = wf_alloc(st, &W.hit_prim, 2 * n)) ||
        (rc = wf_alloc(st, &W.sh, 2 * n)) || (rc = wf_alloc(st, &W.occluded, 2 * n)) || (rc = wf_alloc(st, &W.beta, n)) || (rc = wf_alloc(st, &W.rad, n)) ||
        (rc = wf_alloc(st, &W.rng01, n)) || (rc = wf_alloc(st, &W.rng23, n)) || (rc = wf_alloc(st, &W.pend0, n)) || (rc = wf_alloc(st, &W.pend1, n)) || (rc = wf_alloc(st, &W.pend2, n)) ||
        (rc = wf_alloc(st, &W.q_active[0], n)) || (rc = wf_alloc(st, &W.q_active[1], n)) || (rc = wf_alloc(st, &W.q_closest, 2 * n)) || (rc = wf_alloc(st, &W.q_shadow, 2 * n)) || (rc = wf_alloc(st, &W.q_sorted, 8 * n)) || (rc = wf_alloc(st, &W.cls, CTR(WF_NCLASS))) ||
        (rc = wf_alloc(st, &W.q_exc_closest, 2 * n)) || (rc = wf_alloc(st, &W.q_exc_any, 2 * n)) || (rc = wf_alloc(st, &W.counters, CTR(WFC_SLOTS))) || (rc = wf_alloc(st, &st->br, 2 * n)) || (rc = wf_alloc(st, &st->pd, 4 * n))) return rc;
    st->cap_paths = n;
    return FTN_OK;
}

/* tuning knobs (environment overrides, for experiments only): the environment is read once per entry-point call (knobs_begin), not
 * once per launch of the bounce loop */
static thread_local std::unordered_map<std::string, std::pair<bool, uint32_t>> g_knobs;
void knobs_begin() { g_knobs.clear(); }
uint32_t knob(const char* name, uint32_t def) {
    auto it = g_knobs.find(name);
    if (it == g_knobs.end()) { const char* v = getenv(name); it = g_knobs.emplace(name, std::make_pair(v != nullptr, v ? (uint32_t)atoi(v) : 0u)).first; }
    return it->second.first ? it->second.second : def;
}

/* buffers of k_wf_shade_dl for n paths, `levels` chain levels and `slots` shadow rays per path; tex: the differentials of textured scenes */
void wf_free_dl(WavefrontState* st) { for (void*& m : st->dl_mem) { if (m) (void)hipFree(m); m = nullptr; } st->dl_paths = 0; st->dl_levels = 0; st->dl_slots = 0; st->dl_tex = false; }
int wf_reserve_dl(WavefrontState* st, size_t n, uint32_t levels, uint32_t slots, bool tex) {
    if (n <= st->dl_paths && levels <= st->dl_levels && slots <= st->dl_slots && (!tex || st->dl_tex)) return FTN_OK;
    wf_free_dl(st);
    const size_t sl = std::max<uint32_t>(slots, 2u);                       /* (direct lighting: shadow results at [0, n), MIS-any results at [n, 2n)) */
    WF_TRY(hipMalloc(&st->dl_mem[0], (size_t)levels * n * sizeof(float4)));          /* dlA */
    WF_TRY(hipMalloc(&st->dl_mem[1], (size_t)levels * n * sizeof(float4)));          /* dlB */
    WF_TRY(hipMalloc(&st->dl_mem[2], (size_t)slots * n * sizeof(float4)));           /* whT */
    WF_TRY(hipMalloc(&st->dl_mem[3], 2 * (size_t)slots * n * sizeof(float4)));       /* shadow-ray records */
    WF_TRY(hipMalloc(&st->dl_mem[4], sl * n));                                       /* occluded */
    WF_TRY(hipMalloc(&st->dl_mem[5], sl * n * sizeof(uint32_t)));                    /* any-hit queue */
    WF_TRY(hipMalloc(&st->dl_mem[6], sl * n * sizeof(uint32_t)));                    /* ... and the queue of the rays the four-box kernel hands back */
    if (tex) WF_TRY(hipMalloc(&st->dl_mem[7], 3 * n * sizeof(float4)));              /* dfd */
    st->dl_paths = n; st->dl_levels = levels; st->dl_slots = slots; st->dl_tex = tex;
    return FTN_OK;
}

/* the tile-serial sampler on the queues: one path per tile (the wavefront's buffers for at least one workgroup of them), and per tile the
 * cursor, the film position, the retired flag and, in textured scenes, the differentials; the pinned copies of the polled counters */
int wf_reserve_serial(WavefrontState* st, uint32_t n_tiles, bool tex) {
    int rc = wf_reserve(st, (size_t)std::max<uint32_t>(n_tiles, 256u));
    if (rc) { wf_free(st); return rc; }
    if (n_tiles > st->ser_paths || (tex && !st->ser_tex)) {
        for (void*& m : st->ser_mem) { if (m) (void)hipFree(m); m = nullptr; }
        st->ser_paths = 0;
        WF_TRY(hipMalloc(&st->ser_mem[0], (size_t)n_tiles * sizeof(uint2)));
        WF_TRY(hipMalloc(&st->ser_mem[1], (size_t)n_tiles * sizeof(float2)));
        WF_TRY(hipMalloc(&st->ser_mem[2], (size_t)n_tiles));
        if (tex) WF_TRY(hipMalloc(&st->ser_mem[3], 3 * (size_t)n_tiles * sizeof(float4)));
        st->ser_paths = n_tiles; st->ser_tex = tex;
    }
    if (!st->ser_host) WF_TRY(hipHostMalloc((void**)&st->ser_host, 2 * 16 * 32 * sizeof(uint32_t)));
    return FTN_OK;
}

int wf_state_init(WavefrontState** state) {
    if (*state) return FTN_OK;
    *state = new WavefrontState();
    for (int i = 0; i < 64; i++) { WF_TRY(hipEventCreate(&(*state)->ev[i])); (*state)->n_ev = i + 1; }
    {   /* lowest priority: its workgroups should only take what the main stream's kernels leave free */
        int least = 0, greatest = 0;
        WF_TRY(hipDeviceGetStreamPriorityRange(&least, &greatest));
        WF_TRY(hipStreamCreateWithPriority(&(*state)->side, hipStreamNonBlocking, knob("FTN_WF_SIDE_PRIO", 1) ? least : 0));
    }
    WF_TRY(hipEventCreateWithFlags(&(*state)->ev_ready, hipEventDisableTiming));
    WF_TRY(hipEventCreateWithFlags(&(*state)->ev_side, hipEventDisableTiming));
    {   /* stream memory operations: the side stream can wait for a value a running kernel stores */
        int dev = 0, can = 0;
        WF_TRY(hipGetDevice(&dev));
        if (hipDeviceGetAttribute(&can, hipDeviceAttributeCanUseStreamWaitValue, dev) == hipSuccess && can) {
            if (hipExtMallocWithFlags((void**)&(*state)->drain_sig, 8, hipMallocSignalMemory) != hipSuccess) { (void)hipGetLastError(); (*state)->drain_sig = nullptr; }
            else WF_TRY(hipMemset((*state)->drain_sig, 0, 8));
        }
    }
    WF_TRY(hipHostMalloc((void**)&(*state)->host_counters, 16 * 32 * sizeof(uint32_t)));
    hipDeviceProp_t prop; int dev = 0; WF_TRY(hipGetDevice(&dev)); WF_TRY(hipGetDeviceProperties(&prop, dev));
    (*state)->n_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    return FTN_OK;
}

/* ------------------------------------------------------------------ the pass plan (ftn_wf_internal.h)
 * Samples per pass: up to 256 Mi paths in flight (~88 GB of path state and queues out of 288 GB; the ids, queue indices and sort
 * counts are 32-bit: 2^28 paths is also their limit).  Bigger wavefronts are faster per ray: the sorted queues hold more rays per
 * cell of space (more lanes of a wave share node records) and every launch's drain -- about 0.5 ms whatever its size -- is paid
 * once for more work.  Measured on the config-5 scene, per sample per pixel: 16 Mi paths 29.7 ms, 32 Mi 27.8, 64 Mi 26.7,
 * 128 Mi 25.1, 256 Mi 24.5 (FTN_WF_PATHS_M, in Mi paths).  If the GPU has less to give, the pass is halved. */
int wf_refuse_slots(size_t n_slots) {
    if (n_slots <= ((size_t)1 << 28)) return FTN_OK;
    g_wf_err = "more than 2^20 tiles (2^28 pixel slots) in one call: render the film in several tile ranges";
    return FTN_ERR_UNSUPPORTED;
}
int wf_plan_passes(WavefrontState* st, const RenderParams& P, size_t n_slots, uint32_t total_samples, bool dl, WfPassPlan* plan) {
    int rc = wf_refuse_slots(n_slots);
    if (rc) return rc;
    uint32_t S = (uint32_t)std::max<size_t>(1, ((size_t)std::min<uint32_t>(knob("FTN_WF_PATHS_M", 256), 256u) << 20) / n_slots);
    S = std::min(S, total_samples);
    const bool whitted = P.integrator_kind == FTN_INTEGRATOR_WHITTED;
    uint32_t dl_levels = 0, dl_slots = 0;
    if (dl) {
        if (whitted && P.S.n_lights > WF_WH_MAX_LIGHTS) { g_wf_err = "the wavefront pipeline runs WhittedIntegrator for up to 32 lights (one bit per light in a path's pending-light word)"; return FTN_ERR_UNSUPPORTED; }
        dl_levels = std::max<uint32_t>(1u, std::min<uint32_t>(P.max_depth, WF_DL_MAX)); dl_slots = whitted ? std::max<uint32_t>(P.S.n_lights, 1u) : 1u;
        /* a shadow ray's queue entry is its slot p + l * n_paths, and bit 31 marks MIS rays: slots * paths stays below 2^31 */
        const size_t cap = ((size_t)1 << 31) / std::max<uint32_t>(dl_slots, 2u) - 1u;
        S = (uint32_t)std::max<size_t>(1, std::min<size_t>(S, cap / n_slots));
        if (n_slots > cap) { g_wf_err = "too many pixel slots for this many lights in one call: render the film in several tile ranges"; return FTN_ERR_UNSUPPORTED; }
    }
    auto reserve = [&](uint32_t samples) -> int {
        int r = wf_reserve(st, (size_t)samples * n_slots);
        if (!r && dl) r = wf_reserve_dl(st, st->cap_paths, dl_levels, dl_slots, P.S.n_textures != 0);
        return r;
    };
    rc = reserve(S);
    while (rc == FTN_ERR_OUT_OF_MEMORY && S > 1) {            /* the wavefront does not fit next to what else lives on this GPU: smaller passes */
        wf_free(st); wf_free_dl(st); (void)hipGetLastError();
        S = (S + 1) / 2;
        rc = reserve(S);
    }
    if (rc) { wf_free(st); wf_free_dl(st); return rc; }
    plan->samples = S; plan->dl_levels = dl_levels; plan->dl_slots = dl_slots;
    return FTN_OK;
}

}  // namespace ftn
