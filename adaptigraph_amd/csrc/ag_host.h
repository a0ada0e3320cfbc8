// Private to the host files of the C-ABI (ag_api.hip, ag_api_edges.hip, ag_api_rollout.hip, ag_api_train.hip, ...): the context, its
// call slots, the workspace slab and the helpers they share.  Everything declared here is defined once, in ag_api.hip.
#pragma once
#include "../../include/adaptigraph_amd.h"
#include "ag_edges.h"
#include "ag_model.h"
#include "ag_options.h"
#include "ag_rollout.h"

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

namespace ag {
#ifdef AG_DIAG   // diagnostic build only (ag_diag.hip)
void* diag_create();
void diag_destroy(void* diag);
int diag_fail_at_chunk(void* diag);
int diag_timing_skip(void* diag);
void diag_chunk_dump(void* diag, const EdgeArgs& ea, int n_tools, hipStream_t st);
#endif

// A call's workspace: buffers are taken in order, each 256-byte aligned.  Without a base the slab only MEASURES: take() advances
// `used` and returns null, so a call sizes its workspace by running the very carve it then runs for real (carve_slab).
struct Slab {
    char* base = nullptr;
    size_t cap = 0, used = 0;
    template <typename T> T* take(size_t n) {
        used = (used + 255) & ~size_t(255);
        T* p = base ? reinterpret_cast<T*>(base + used) : nullptr;
        used += n * sizeof(T);
        return p;
    }
};
struct ProfEvent { int fam; hipEvent_t e0, e1; };

// what a kept base rollout of the prefix sharing (and a census verdict) is valid for; compared with memcmp, so always memset +
// field-wise filled + memcpy'd
struct BaseKey { int N_o, M, topk, cta, max_nR, n_his, precision, pstep, grip_on; float thr, grip, phys, clamp; const float* phys_vec;
                 unsigned long long weights_version; };

// Everything a call writes while it is in flight: workspace, launch plans, pinned read-back buffers, the events and streams of
// its fork / join.  A context keeps up to kMaxSlots of them, one per CALLER STREAM: calls issued on different streams then run
// side by side on the GPU (the planner's chunk loop, plan.py:241-247, is 40 independent calls on one start state;
// adaptigraph_amd/planner.py deals them to a few streams), calls on one stream stay ordered by the stream.  A stream that finds no
// free slot takes over the least recently used one after making itself wait for that slot's last call (an event recorded at the
// end of every call).  Created on first use, kept until ag_ctx_destroy: a call of a shape the slot has seen allocates nothing.
struct CallSlot {
    hipStream_t stream = nullptr; bool bound = false; unsigned long long tick = 0;
    Slab slab;
    int* d_repeat = nullptr; size_t repeat_cap = 0;   // device: [repeat (B*H) | launch order (H*B)]
    std::vector<int> h_repeat;   // slot-owned copy so the caller's array may die right after the call; same layout
    char* d_plan = nullptr; size_t plan_cap = 0;      // device-planned rollouts (ag_rollout_actions): decoded tool keypoints,
                                                      // repeats, launch order and per-step live counts
    int* h_rep_pin = nullptr; size_t rep_pin_cap = 0;     // pinned: [forwards left | action_repeat | flag, census x4] of a prefix-sharing call
    int* h_plan_max = nullptr; size_t plan_max_cap = 0;   // pinned host copy of RollPlan::maxrep of the call being enqueued
    int* h_census = nullptr;                            // pinned (8 ints): result of a census nobody waited for (see Decision)
    hipEvent_t ev_plan = nullptr;                       // fires when a read-back of this call has landed
    hipEvent_t ev_census = nullptr; bool census_pending = false;   // a census went out on this slot's stream that nobody waited for
    BaseKey census_key{}; int census_B = 0, census_H = 0, census_R = 0;
    hipEvent_t ev_done = nullptr; bool have_done = false;   // end of the slot's last call
    float* d_work = nullptr; size_t work_cap = 0;   // ag_rollout_work: scratch for the plan kernel's other outputs
    int* d_words = nullptr;      // 64 ints: [0] overflow word of the synchronous entry points, [8..11] census counters
    unsigned long long* d_share_stats = nullptr;      // shared first forward: [0] slots served by the base table, [1] slots encoded per candidate
    static constexpr int kMaxStreams = 4;
    hipStream_t aux_stream[kMaxStreams] = {nullptr, nullptr, nullptr, nullptr};   // [0] unused: the caller's stream
    hipEvent_t ev_fork = nullptr, ev_join[kMaxStreams] = {nullptr, nullptr, nullptr, nullptr};
};
}  // namespace ag

struct ag_ctx {
    int device = 0;
    ag_dims dims{};
    std::string err;
    float* d_w = nullptr;
    float* d_wb3 = nullptr;      // bf16x3 weight image (58 phases of 30,720 B)
    float* d_wlat = nullptr;     // weight image of the latency-mode chains (ag_lat.hip), n_his = 4 models only
    int precision = 0;           // 0: exact fp32 MFMA (default), 1: bf16x3 split on the bf16 matrix pipe
    bool have_w = false;
    bool w_finite = false;       // the packed weights were seen on the host and are all finite: zero skip (Options::zero_skip) may run
    int chunk = 0;
    ag::Options opt;             // per-context switches: environment defaults read once at create, ag_ctx_set_option afterwards
    void* diag = nullptr;        // diagnostic build only: probe state of this context (ag_diag.hip)
    static constexpr int kMaxSlots = 8;
    static constexpr int kMaxStreams = ag::CallSlot::kMaxStreams;
    ag::CallSlot slots[kMaxSlots];
    unsigned long long slot_tick = 0;
    int last_slot = 0;           // slot of the last rollout call (the diagnostics below refer to it)
    long long n_allocs = 0;      // hipMalloc / hipHostMalloc / hipFree / hipHostFree / event and stream creations so far (ag_ctx_alloc_counts)
    long long fwd_executed = 0, fwd_needed = 0;       // candidate-forwards of the last rollout call (ag_ctx_rollout_counts)
    int* d_plan_sums = nullptr; int plan_sums_n = 0;  // device-planned call: sums pending a read-back
    // base rollout of the prefix sharing, kept across calls: the reference's planner calls dynamics() 40 times per planner call
    // with one start state (plan.py:241-247).  Valid for (start state bit-equal, same model / task scalars); [states | heights].
    // Shared by all slots: host-side validity (base_cache_R) is set only after the producing call has waited for its contact plan,
    // i.e. with the contents complete; a call that overwrites it first makes its stream wait for every other slot's last call.
    float* d_base_cache = nullptr; size_t base_cache_cap = 0; int base_cache_R = -1, base_cache_capR = 0;
    ag::BaseKey base_key{};
    // the automatic mode's last census verdict "not worth a base rollout" (bench-like batches: every push starts on the object),
    // for batches of the same key and shape: such a call skips the blocking census, enqueues one that nobody waits for, and the
    // verdict is revisited when that one has landed (see rollout_impl).  A stale verdict costs time, never a result.
    struct Decision { bool decline = false; ag::BaseKey key{}; int B = 0, H = 0; } decision;
    unsigned long long weights_version = 0;
    long long steps_enqueued = 0, steps_bound = 0;      // model forwards (per chunk) enqueued by the last rollout call / what the bound alone gives
    const int* d_share_nns = nullptr;                 // edges the base encode ran over (workspace of the last rollout call), or null
    float* d_cself = nullptr;    // (256, NFP): rows 0/1 = C of an object / tool self-loop edge (see GraphBufs)
    char* d_self_mini = nullptr; // the constant 2-particle graph those rows are computed on (enqueue_self_rows)
    // in-library streams of a call: alternate chunks run on them so that the HBM-bound kernels of one chunk overlap the
    // MFMA-bound chains of the other (fork/join with events around every rollout call)
    int n_streams = 2;
    // profiling
    unsigned prof_mask = 0;
    std::vector<ag::ProfEvent> prof_live;
    std::vector<hipEvent_t> prof_pool;
    double prof_ms[ag::FAM_COUNT] = {0};
    long long prof_n[ag::FAM_COUNT] = {0};
    hipStream_t prof_stream = nullptr;
};

namespace ag {

int fail(ag_ctx* c, int code, const char* fmt, ...);
#define HIPCHK(c, expr)                                                                                   \
    do {                                                                                                  \
        hipError_t _e = (expr);                                                                           \
        if (_e != hipSuccess) return fail(c, AG_ERR_HIP, "%s failed: %s", #expr, hipGetErrorString(_e)); \
    } while (0)

// every allocation / creation the library makes is counted (ag_ctx_alloc_counts): a steady-state call makes none
inline hipError_t dev_alloc(ag_ctx* c, void** p, size_t bytes) { ++c->n_allocs; return hipMalloc(p, bytes); }
inline hipError_t dev_free(ag_ctx* c, void* p) { ++c->n_allocs; return hipFree(p); }
inline hipError_t pin_alloc(ag_ctx* c, void** p, size_t bytes) { ++c->n_allocs; return hipHostMalloc(p, bytes, hipHostMallocDefault); }
inline hipError_t pin_free(ag_ctx* c, void* p) { ++c->n_allocs; return hipHostFree(p); }
inline hipError_t event_new(ag_ctx* c, hipEvent_t* e) { ++c->n_allocs; return hipEventCreateWithFlags(e, hipEventDisableTiming); }
inline hipError_t stream_new(ag_ctx* c, hipStream_t* s) { ++c->n_allocs; return hipStreamCreateWithFlags(s, hipStreamNonBlocking); }
// grow-on-demand buffer of `cap` T's, device or pinned: below `need` it is replaced by one of `want` (the site's own slack)
template <typename T>
int grow(ag_ctx* c, bool pinned, T*& buf, size_t& cap, size_t need, size_t want) {
    if (cap >= need) return AG_OK;
    if (buf) HIPCHK(c, pinned ? pin_free(c, buf) : dev_free(c, buf));
    buf = nullptr; cap = 0;
    void** q = reinterpret_cast<void**>(&buf);
    HIPCHK(c, pinned ? pin_alloc(c, q, want * sizeof(T)) : dev_alloc(c, q, want * sizeof(T)));
    cap = want;
    return AG_OK;
}

// ---------------------------------------------------------------------------------------------- call slots
// The slot of caller stream `st` (see CallSlot).  capturing: the call is being recorded into a hipGraph - it may neither wait for
// nor record an event that lives outside the graph.
int slot_acquire(ag_ctx* c, hipStream_t st, bool capturing, CallSlot** out);
// end of a call that used the slot: later calls on OTHER streams that take the slot over wait for this point
void slot_release(CallSlot* s, hipStream_t st, bool capturing);
// is a call of another slot still running on the GPU?  (then this caller is pipelining calls over streams)
bool other_slot_busy(ag_ctx* c, const CallSlot* me);
// Records the slot's end-of-call event on EVERY exit of the call that acquired it (r06): an early `return rc` after work was
// enqueued used to leave ev_done marking an EARLIER call, so a later take-over of the slot by another stream (slot_acquire's LRU
// path, the wait-for-all-slots before d_base_cache is replaced) would not have waited for what the failed call had enqueued.
// Filled by begin_call; an entry point reads its stream and slot from it.
struct SlotGuard {
    hipStream_t st = nullptr; CallSlot* sl = nullptr; bool capturing = false;
    SlotGuard() = default;
    SlotGuard(const SlotGuard&) = delete; SlotGuard& operator=(const SlotGuard&) = delete;
    ~SlotGuard() { slot_release(sl, st, capturing); }
};
// The opening of every entry point that works on a slot: the context's device, the caller's stream (the profiling marks of the
// call go there), its slot, the guard.  watch_capture (the rollout): find out whether the caller is capturing the stream.
int begin_call(ag_ctx* c, void* stream, SlotGuard& call, bool watch_capture = false);

void prof_mark(void* vc, int fam, int phase);
struct Scoped {
    ag_ctx* c; int fam;
    Scoped(ag_ctx* c_, int f) : c(c_), fam(f) { prof_mark(c, fam, 0); }
    ~Scoped() { prof_mark(c, fam, 1); }
};

// ---------------------------------------------------------------------------------------------- workspace
struct Work {
    GraphBufs g{};
    RollBufs r{};
    int* ell; int* deg; int* slice_tot; int* cta_flag;
    int* recv; int* send; int* row_ptr; int* n_edges;
    int* ns_edge; int* n_ns; int* n_oo;
    unsigned long long* ck_bits; int* ck_off; unsigned* ck_list;   // chunk list (EdgeArgs::ck_list), slot-indexed rollout graphs only
    int* send_pk;                // first forward of a dynamics() call (GraphBufs::send_pk)
    int* rowlist; int* n_rows;   // ragged batches (GraphBufs::rowlist)
};

inline size_t round_up(size_t v, size_t m) { return (v + m - 1) / m * m; }
// the slot's slab, emptied, with room for `bytes` (grown with one eighth of slack, rounded to 1 MiB)
inline int ensure_slab(ag_ctx* c, CallSlot& sl, size_t bytes) {
    sl.slab.used = 0;
    return grow(c, false, sl.slab.base, sl.slab.cap, bytes, round_up(bytes + (bytes >> 3), 1 << 20));
}
// A call's workspace, described ONCE by carve(Slab&): run on a measuring slab for its size, then - the slot's slab grown to that -
// for real.  carve only takes buffers and keeps the pointers; it runs twice, the second run's pointers stand.
template <typename Carve>
int carve_slab(ag_ctx* c, CallSlot& sl, Carve&& carve) {
    Slab measure;
    carve(measure);
    int rc = ensure_slab(c, sl, measure.used);
    if (rc) return rc;
    carve(sl.slab);
    if (sl.slab.used > sl.slab.cap) return fail(c, AG_ERR_INVALID, "internal: workspace carve overflow");   // the two runs differed
    return AG_OK;
}
// one workspace for Bc candidates.  own_edges: edge index arrays + builder scratch; roll: rollout state
void carve_work(const ag_ctx* c, Slab& s, Work& w, int Bc, int N, int n_inst, int edge_cap, int c_cap, int slices, bool own_edges,
                bool roll, bool own_group, int N_o, int ell_stride);

int pick_slices(const ag_ctx* c, int B, int N);
int clamp_chunk_for_offsets(int Bc, int N, int c_cap);
int check_graph_rows(ag_ctx* c, const char* me, int N, int edge_cap);   // one graph within the 32-bit activation offsets, or AG_ERR_UNSUPPORTED
int auto_chunk(const ag_ctx* c, int B, int N);
bool lat_node_for(const ag_ctx* c, const GraphBufs& g);
bool lat_edge_for(const ag_ctx* c, const GraphBufs& g);
hipError_t node_enc_for(const ag_ctx* c, const GraphBufs& g, long row0, long nrows, hipStream_t st);
int run_edge_chain(ag_ctx* c, const GraphBufs& g, hipStream_t st);
int run_model(ag_ctx* c, const GraphBufs& g, float* pred_pos, float* pred_motion, hipStream_t st);
int enqueue_self_rows(ag_ctx* c, hipStream_t st);
int check_topk(ag_ctx* c, int N, int topk);

// DynamicsPredictor.forward over caller-built graphs (ag_forward, every step of ag_train_step, ag_ppm_grad_step): the launch chunk
// and the workspace carved for it, so that all three choose the same kernels.  n_guard: guarded edge counts (launch_edge_guard)
// carved behind the workspace - B of them, or none where the caller keeps its own per step.
struct ForwardFrame {
    int B, N, n_inst, edge_cap, n_p, n_guard, c_cap, Bc;
    Work w{}; int* n_eff = nullptr;
    ForwardFrame(const ag_ctx* c, int B, int N, int n_inst, int edge_cap, int n_p, int n_guard);
    void carve(const ag_ctx* c, Slab& s);
};
// the forward over the batch in launch chunks of f.Bc; n_eff: the guarded per-graph edge counts
int enqueue_forward(ag_ctx* c, const ForwardFrame& f, const float* d_state, const float* d_attrs, const float* d_action,
                    const float* d_phys, const float* d_group, const int32_t* d_recv, const int32_t* d_send,
                    const int32_t* d_row_ptr, const int* n_eff, int B, float* d_pred_pos, float* d_pred_motion, hipStream_t st);

}  // namespace ag
