// C-ABI of the MI355X-native GNN-dynamics rollout engine (see include/adaptigraph_amd.h).
// Host orchestration only: context, workspace, weight repacking, launch sequences.  No CPU compute fallback.
#include "../../include/adaptigraph_amd.h"
#include "ag_common.h"

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

namespace ag {
size_t edge_build_max_particles();
int edge_ell_stride(int N, int topk);
size_t lat_weights_floats();
size_t lat_weights_offset(int which);
hipError_t launch_edge_enc_lat(const float* wl, const GraphBufs& g, hipStream_t st);
hipError_t launch_node_enc_lat(const float* wl, const GraphBufs& g, long row0, long nrows, hipStream_t st);
hipError_t launch_node_prop_lat(const float* wl, const GraphBufs& g, int round, bool last, float clamp, float* pred_pos,
                                float* pred_motion, hipStream_t st);
#ifdef AG_DIAG   // diagnostic build only (ag_diag.hip)
void* diag_create();
void diag_destroy(void* diag);
int diag_fail_at_chunk(void* diag);
int diag_timing_skip(void* diag);
#endif
}
using namespace ag;

namespace {

const char* kFamilyNames[FAM_COUNT] = {"edge_count", "edge_emit", "prep", "node_enc", "edge_enc",
                                       "mp", "node_prop", "node_final", "roll_init", "roll_update", "cost"};

struct Slab {
    char* base = nullptr;
    size_t cap = 0, used = 0;
    template <typename T> T* take(size_t n) {
        used = (used + 255) & ~size_t(255);
        T* p = reinterpret_cast<T*>(base + used);
        used += n * sizeof(T);
        return p;
    }
};

struct ProfEvent { int fam; hipEvent_t e0, e1; };

}  // namespace

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

struct ag_ctx {
    int device = 0;
    ag_dims dims{};
    std::string err;
    float* d_w = nullptr;
    float* d_wb3 = nullptr;      // bf16x3 weight image (58 phases of 30,720 B)
    float* d_wlat = nullptr;     // weight image of the latency-mode chains (ag_lat.hip), n_his = 4 models only
    int precision = 0;           // 0: exact fp32 MFMA (default), 1: bf16x3 split on the bf16 matrix pipe
    bool have_w = false;
    int chunk = 0;
    Options opt;                 // per-context switches: environment defaults read once at create, ag_ctx_set_option afterwards
    void* diag = nullptr;        // diagnostic build only: probe state of this context (ag_diag.hip)
    static constexpr int kMaxSlots = 8;
    static constexpr int kMaxStreams = CallSlot::kMaxStreams;
    CallSlot slots[kMaxSlots];
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
    BaseKey base_key{};
    // the automatic mode's last census verdict "not worth a base rollout" (bench-like batches: every push starts on the object),
    // for batches of the same key and shape: such a call skips the blocking census, enqueues one that nobody waits for, and the
    // verdict is revisited when that one has landed (see rollout_impl).  A stale verdict costs time, never a result.
    struct Decision { bool decline = false; BaseKey key{}; int B = 0, H = 0; } decision;
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
    std::vector<ProfEvent> prof_live;
    std::vector<hipEvent_t> prof_pool;
    double prof_ms[FAM_COUNT] = {0};
    long long prof_n[FAM_COUNT] = {0};
    hipStream_t prof_stream = nullptr;
};

namespace {

struct OptName { const char* name; const char* env; int Options::* field; bool env_negates; int lo, hi; };
const OptName kOptions[] = {
    {"streams", "AG_STREAMS", &Options::streams, false, 0, ag_ctx::kMaxStreams},
    {"chunk", "AG_CHUNK", &Options::chunk, false, 0, 1 << 20},
    {"latency", "AG_LATENCY", &Options::latency, false, -1, 1},
    {"ragged", "AG_NO_RAGGED", &Options::ragged, true, 0, 1},
    {"ell_graph", "AG_NO_ELL_GRAPH", &Options::ell_graph, true, 0, 1},
    {"self_dedupe", "AG_NO_SELF_DEDUPE", &Options::self_dedupe, true, 0, 1},
    {"repeat_sort", "AG_NO_REPEAT_SORT", &Options::repeat_sort, true, 0, 1},
    {"edge_wgs", "AG_EDGE_WGS", &Options::edge_wgs, false, 1, 1 << 16},
    {"edge_block_min", "AG_EDGE_BLOCK_MIN", &Options::edge_block_min, false, -1, 0x7fffffff},
    {"enc_persist", "AG_ENC_PERSIST", &Options::enc_persist, false, 0, 1 << 20},
    {"stagger_us", "AG_STAGGER_US", &Options::stagger_us, false, 0, 1000},
    {"device_decode", "AG_DEVICE_DECODE", &Options::device_decode, false, -1, 1},
    {"zigzag", "AG_ZIGZAG", &Options::zigzag, false, 0, 1},
    {"share_first", "AG_SHARE_FIRST", &Options::share_first, false, -1, 1},
    {"share_prefix", "AG_SHARE_PREFIX", &Options::share_prefix, false, -1, 1},
    {"stream_min_rows", "AG_STREAM_MIN_ROWS", &Options::stream_min_rows, false, 0, 0x7fffffff},
    {"pipeline_fork", "AG_PIPELINE_FORK", &Options::pipeline_fork, false, 0, 1},
};
void options_from_env(Options& o) {   // values from the environment are clamped into the option's range
    for (const OptName& n : kOptions)
        if (const char* e = getenv(n.env)) o.*(n.field) = n.env_negates ? (atoi(e) ? 0 : 1) : std::min(n.hi, std::max(n.lo, atoi(e)));
}

int fail(ag_ctx* c, int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (c) c->err = buf;
    return code;
}
#define HIPCHK(c, expr)                                                                                   \
    do {                                                                                                  \
        hipError_t _e = (expr);                                                                           \
        if (_e != hipSuccess) return fail(c, AG_ERR_HIP, "%s failed: %s", #expr, hipGetErrorString(_e)); \
    } while (0)

// every allocation / creation the library makes is counted (ag_ctx_alloc_counts): a steady-state call makes none
hipError_t dev_alloc(ag_ctx* c, void** p, size_t bytes) { ++c->n_allocs; return hipMalloc(p, bytes); }
hipError_t dev_free(ag_ctx* c, void* p) { ++c->n_allocs; return hipFree(p); }
hipError_t pin_alloc(ag_ctx* c, void** p, size_t bytes) { ++c->n_allocs; return hipHostMalloc(p, bytes, hipHostMallocDefault); }
hipError_t pin_free(ag_ctx* c, void* p) { ++c->n_allocs; return hipHostFree(p); }
hipError_t event_new(ag_ctx* c, hipEvent_t* e) { ++c->n_allocs; return hipEventCreateWithFlags(e, hipEventDisableTiming); }
hipError_t stream_new(ag_ctx* c, hipStream_t* s) { ++c->n_allocs; return hipStreamCreateWithFlags(s, hipStreamNonBlocking); }
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

// The slot of caller stream `st` (see CallSlot).  capturing: the call is being recorded into a hipGraph - it may neither wait for
// nor record an event that lives outside the graph.
int slot_acquire(ag_ctx* c, hipStream_t st, bool capturing, CallSlot** out) {
    CallSlot* s = nullptr;
    for (CallSlot& k : c->slots) if (k.bound && k.stream == st) { s = &k; break; }
    if (!s) for (CallSlot& k : c->slots) if (!k.bound) { s = &k; break; }
    if (!s) {   // every slot belongs to another stream: take the least recently used one, after its last call
        s = &c->slots[0];
        for (CallSlot& k : c->slots) if (k.tick < s->tick) s = &k;
        if (!capturing && s->have_done) HIPCHK(c, hipStreamWaitEvent(st, s->ev_done, 0));
        s->census_pending = false;
    }
    if (!s->ev_done) {   // first use: everything whose size does not depend on the call
        HIPCHK(c, event_new(c, &s->ev_done));
        HIPCHK(c, event_new(c, &s->ev_plan));
        HIPCHK(c, event_new(c, &s->ev_census));
        HIPCHK(c, event_new(c, &s->ev_fork));
        HIPCHK(c, dev_alloc(c, reinterpret_cast<void**>(&s->d_words), 256));
        HIPCHK(c, dev_alloc(c, reinterpret_cast<void**>(&s->d_share_stats), 256));
        HIPCHK(c, hipMemset(s->d_share_stats, 0, 256));
        HIPCHK(c, pin_alloc(c, reinterpret_cast<void**>(&s->h_census), 64));
    }
    s->bound = true; s->stream = st; s->tick = ++c->slot_tick;
    *out = s;
    return AG_OK;
}
// end of a call that used the slot: later calls on OTHER streams that take the slot over wait for this point
void slot_release(CallSlot* s, hipStream_t st, bool capturing) {
    if (capturing || !s || !s->ev_done) return;
    if (hipEventRecord(s->ev_done, st) == hipSuccess) s->have_done = true;
}
// Records the slot's end-of-call event on EVERY exit of the call that acquired it (r06): an early `return rc` after work was
// enqueued used to leave ev_done marking an EARLIER call, so a later take-over of the slot by another stream (slot_acquire's LRU
// path, the wait-for-all-slots before d_base_cache is replaced) would not have waited for what the failed call had enqueued.
struct SlotGuard {
    CallSlot* s; hipStream_t st; bool capturing;
    SlotGuard(CallSlot* s_, hipStream_t st_, bool cap_) : s(s_), st(st_), capturing(cap_) {}
    SlotGuard(const SlotGuard&) = delete;
    SlotGuard& operator=(const SlotGuard&) = delete;
    ~SlotGuard() { slot_release(s, st, capturing); }
};
// is a call of another slot still running on the GPU?  (then this caller is pipelining calls over streams)
bool other_slot_busy(ag_ctx* c, const CallSlot* me) {
    bool busy = false;
    for (CallSlot& k : c->slots)
        if (&k != me && k.bound && k.have_done) {
            if (hipEventQuery(k.ev_done) == hipErrorNotReady) busy = true;
            (void)hipGetLastError();
        }
    return busy;
}
void slot_destroy(ag_ctx* c, CallSlot& s) {
    for (hipEvent_t e : {s.ev_plan, s.ev_census, s.ev_done, s.ev_fork}) if (e) (void)hipEventDestroy(e);
    for (int i = 1; i < CallSlot::kMaxStreams; ++i) {
        if (s.ev_join[i]) (void)hipEventDestroy(s.ev_join[i]);
        if (s.aux_stream[i]) (void)hipStreamDestroy(s.aux_stream[i]);
    }
    if (s.h_plan_max) (void)hipHostFree(s.h_plan_max);
    if (s.h_rep_pin) (void)hipHostFree(s.h_rep_pin);
    if (s.h_census) (void)hipHostFree(s.h_census);
    if (s.d_words) (void)hipFree(s.d_words);
    if (s.d_share_stats) (void)hipFree(s.d_share_stats);
    if (s.d_repeat) (void)hipFree(s.d_repeat);
    if (s.d_plan) (void)hipFree(s.d_plan);
    if (s.d_work) (void)hipFree(s.d_work);
    if (s.slab.base) (void)hipFree(s.slab.base);
    s = CallSlot();
}

void prof_mark(void* vc, int fam, int phase) {
    ag_ctx* c = static_cast<ag_ctx*>(vc);
    if (!(c->prof_mask & (1u << fam))) return;
    auto get = [&]() {
        hipEvent_t e;
        if (!c->prof_pool.empty()) { e = c->prof_pool.back(); c->prof_pool.pop_back(); }
        else (void)hipEventCreate(&e);
        return e;
    };
    if (phase == 0) {
        ProfEvent p{fam, get(), get()};
        (void)hipEventRecord(p.e0, c->prof_stream);
        c->prof_live.push_back(p);
    } else {
        for (auto it = c->prof_live.rbegin(); it != c->prof_live.rend(); ++it)
            if (it->fam == fam) { (void)hipEventRecord(it->e1, c->prof_stream); break; }
    }
}
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
    int* ns_edge; int* n_ns;
    int* send_pk;                // first forward of a dynamics() call (GraphBufs::send_pk)
    int* rowlist; int* n_rows;   // ragged batches (GraphBufs::rowlist)
};

size_t round_up(size_t v, size_t m) { return (v + m - 1) / m * m; }

int ensure_slab(ag_ctx* c, CallSlot& sl, size_t bytes) {
    sl.slab.used = 0;
    return grow(c, false, sl.slab.base, sl.slab.cap, bytes, round_up(bytes + (bytes >> 3), 1 << 20));
}

// bytes of one workspace for Bc candidates.  own_edges: edge index arrays + builder scratch; roll: rollout state
size_t work_bytes(int Bc, int N, int n_inst, int edge_cap, int c_cap, int slices, bool own_edges, bool roll,
                  bool own_group, int N_o, int ell_stride) {
    const size_t rows = (size_t)Bc * N;
    size_t bytes = 16 * 256;
    bytes += rows * (NODE_IN + F15_PITCH + (own_group ? n_inst : 0)) * 4 + 6 * rows * NFP * 4 + ((size_t)Bc * c_cap + 256) * NFP * 4;
    if (own_edges) bytes += rows * (size_t)(ell_stride + 1) * 4 + (size_t)Bc * (slices + 3) * 4 + 3 * (size_t)Bc * edge_cap * 4 + (size_t)Bc * (N + 1) * 4;
    if (roll) bytes += (size_t)Bc * edge_cap * 4 + rows * 4 + 1024 + (size_t)Bc * 4 + (size_t)Bc * N_HIS_MAX * N * 3 * 4 + 2 * (size_t)Bc * N_o * 3 * 4 + 2 * rows +
                       (size_t)cls_rows(N_o, N - N_o, Bc) * (NODE_IN + 4 * NFP) * 4;
    return bytes + 64 * 256;
}

// carve one workspace from the slab (which must already be large enough; see work_bytes)
int carve_work(ag_ctx* c, Slab& s, Work& w, int Bc, int N, int n_inst, int edge_cap, int c_cap, int slices, bool own_edges,
               bool roll, bool own_group, int N_o, int ell_stride) {
    const size_t rows = (size_t)Bc * N;
    w.g.node_in = s.take<float>(rows * NODE_IN);
    w.g.feat12 = s.take<float>(rows * F15_PITCH);            // pitch 12 (n_his 4) or 16 (n_his 5, forward path)
    w.g.group = own_group ? s.take<float>(rows * n_inst) : nullptr;
    w.g.eff = s.take<float>(rows * NFP);
    w.g.P = s.take<float>(rows * NFP);
    for (int par = 0; par < 2; ++par)
        for (int k = 0; k < 2; ++k) w.g.UV[par][k] = s.take<float>(rows * NFP);
    w.g.C = s.take<float>(((size_t)Bc * c_cap + 256) * NFP);   // + room for the two self-loop constant rows
    w.g.B = Bc; w.g.N = N; w.g.n_inst = n_inst; w.g.edge_cap = edge_cap; w.g.c_cap = c_cap; w.g.n_p = N_o;
    w.g.enc_persist = c->opt.enc_persist; w.g.stagger_us = c->opt.stagger_us; w.g.zigzag = c->opt.zigzag; w.g.diag = c->diag;
    if (own_edges) {
        w.ell = s.take<int>(rows * (size_t)std::max(1, ell_stride));
        w.deg = s.take<int>(rows);
        w.slice_tot = s.take<int>((size_t)Bc * slices);
        w.cta_flag = s.take<int>(Bc);
        w.recv = s.take<int>((size_t)Bc * edge_cap);
        w.send = s.take<int>((size_t)Bc * edge_cap);
        w.row_ptr = s.take<int>((size_t)Bc * (N + 1));
        w.n_edges = s.take<int>(Bc);
        w.ns_edge = s.take<int>((size_t)Bc * edge_cap);
        w.n_ns = s.take<int>(Bc);
        w.g.recv = w.recv; w.g.send = w.send; w.g.row_ptr = w.row_ptr; w.g.n_edges = w.n_edges;
    }
    if (roll) {
        w.send_pk = s.take<int>((size_t)Bc * edge_cap);
        w.rowlist = s.take<int>(rows);
        w.n_rows = s.take<int>((size_t)Bc + 64);            // ragged batches: row count per number of live slots (k_build_rowlist)
        w.r.hist = s.take<float>((size_t)Bc * N_HIS_MAX * N * 3);   // (Bc, n_his, N, 3) with the model's n_his (4 or 5)
        w.r.pred = s.take<float>((size_t)Bc * N_o * 3);
        w.r.motion = s.take<float>((size_t)Bc * N_o * 3);
        w.r.mask = s.take<uint8_t>(rows);
        w.r.tool = s.take<uint8_t>(rows);
        const size_t cr = (size_t)cls_rows(N_o, N - N_o, Bc);
        w.g.cls_on = 1; w.g.N_o = N_o; w.g.M = N - N_o; w.g.vmask = w.r.mask;
        w.g.c_node_in = s.take<float>(cr * NODE_IN);
        w.g.c_eff = s.take<float>(cr * NFP);
        w.g.c_P = s.take<float>(cr * NFP);
        w.g.c_U = s.take<float>(cr * NFP);
        w.g.c_V = s.take<float>(cr * NFP);
    }
    if (s.used > s.cap) return fail(c, AG_ERR_INVALID, "internal: workspace carve overflow");
    return AG_OK;
}

int pick_slices(const ag_ctx* c, int B, int N) {
    // one sixteen-wave workgroup per CU: every workgroup re-reads its candidate's positions and re-derives the chunk
    // boxes, so fewer, longer row slices win (cloth, 128 candidates: 128 workgroups 56.8 ms per rollout, 256: 31.0,
    // 384: 43.1, 512: 35.2, 1024: 41.9)
    const int target = std::max(1, c->opt.edge_wgs);
    int s = (target + B - 1) / B;
    // a slice is at least 16 rows (one per wavefront of the workgroup): small batches are latency-bound, so a single
    // graph is spread over as many workgroups as that allows (one rope graph: 4 -> 18 workgroups, 43 -> 13 us per launch)
    s = std::min(s, std::max(1, N / 16));
    // (r06: up to 128 slices - one cloth-sized graph alone was cut into 64 slices of 32 rows, two rows per wavefront on a quarter
    // of the chip; 127 slices of 16 rows give every wavefront one row.  Which rows share a workgroup never changes a row's result.)
    return std::max(1, std::min(s, 128));
}

// the gather (ag_mlp.hip: gather_agg) addresses C, U and V with 32-bit element offsets: a launch chunk must keep every buffer below 2^32 floats
int clamp_chunk_for_offsets(int Bc, int N, int c_cap) {
    const long max_rows = ((1L << 32) / NFP) - 512;          // rows of NFP floats addressable with a 32-bit element offset
    const long by_c = max_rows / std::max(1, c_cap);
    const long by_n = max_rows / std::max(1, N);
    return (int)std::max(1L, std::min<long>(Bc, std::min(by_c, by_n)));
}

int auto_chunk(const ag_ctx* c, int B, int N) {
    if (c->chunk > 0) return std::min(c->chunk, B);
    if (c->opt.chunk > 0) return std::min(c->opt.chunk, B);
    // Node chains run 128-row workgroups, two per CU: the largest chunk whose workgroup count is <= 4 rounds of 512.
    // (Measured on the 1024 x 2026 cloth batch: 64 candidates/launch 574 ms, 96: 564, 128: 559, 192: 561, 256: 558 -
    // more rounds per launch dilute the lockstep store bursts and the launch tails; the workspace grows with it.)
    const long max_rows = 4L * 256 * 256;
    long bc = max_rows / N;
    return (int)std::max(1L, std::min<long>(bc, B));
}

// Small launches are latency-bound: below one chip-filling round of 128-row workgroups the latency-mode chains take over
// (ag_lat.hip: 32-row workgroups, every layer split over the four wavefronts; bit-identical results).  Options::latency:
// 0 never, 1 always, -1 = by size.  (Thresholds in 128-row workgroups of the throughput kernels: a latency workgroup reads
// its weight fragments from L2 itself - 200 KB per layer - so beyond about one latency workgroup per CU the L2 traffic eats
// the gain: rope 64 x 301 rows = 151 workgroups runs the same 71 us either way, one rope graph 66 -> 31 us.)
bool lat_available(const ag_ctx* c, const GraphBufs& g) { return c->d_wlat && !g.wb3 && g.n_his != 5; }
bool lat_edge_for(const ag_ctx* c, const GraphBufs& g) {
    const long edge_wgs = (long)g.B * g.c_cap / 128;
    return lat_available(c, g) && (c->opt.latency >= 0 ? c->opt.latency == 1 : edge_wgs <= 128);
}
// particle-encoder chain (class table: 2 N_o + B M rows per look-ahead step): the latency-mode kernel while its grid of 32-row
// workgroups fits one round of the chip (two per CU); beyond that the 128-row throughput kernel
hipError_t node_enc_for(const ag_ctx* c, const GraphBufs& g, long row0, long nrows, hipStream_t st) {
    const long rows = g.cls_on ? nrows : (long)g.B * g.N;
    const bool lat = lat_available(c, g) && (c->opt.latency >= 0 ? c->opt.latency == 1 : rows <= 512L * 32);
    return lat ? launch_node_enc_lat(c->d_wlat, g, row0, nrows, st) : launch_node_enc(c->d_w, g, row0, nrows, st);
}
bool lat_node_for(const ag_ctx* c, const GraphBufs& g) {
    const long node_wgs = ((long)g.B * g.N + 127) / 128;
    return lat_available(c, g) && (c->opt.latency >= 0 ? c->opt.latency == 1 : node_wgs <= 64);
}
// relation encoder + W1 over the graph's (non-self-loop) edges -> C
int run_edge_chain(ag_ctx* c, const GraphBufs& g, hipStream_t st) {
    Scoped p(c, FAM_EDGE_ENC);
    if (lat_edge_for(c, g)) HIPCHK(c, launch_edge_enc_lat(c->d_wlat, g, st));
    else HIPCHK(c, launch_edge_enc(c->d_w, g, st));
    return AG_OK;
}

// one model forward on a prepared workspace (node_in, feat12, group, edges all set).  With g.cls_on the particle
// encoder outputs already sit in the class table (encoded at look-ahead-step start) and k_node_enc is skipped.
int run_model(ag_ctx* c, const GraphBufs& g, float* pred_pos, float* pred_motion, hipStream_t st) {
    if (!g.cls_on) { Scoped p(c, FAM_NODE_ENC); HIPCHK(c, node_enc_for(c, g, 0, (long)g.B * g.N, st)); }
    const bool lat_node = lat_node_for(c, g);
    if (g.send_pk && lat_node) return fail(c, AG_ERR_INVALID, "internal: shared first forward on the latency-mode chains");
    int rc = run_edge_chain(c, g, st);
    if (rc) return rc;
    for (int ps = 0; ps < c->dims.pstep; ++ps) {
        const bool last = ps + 1 == c->dims.pstep;
        Scoped p(c, last ? FAM_NODE_FINAL : FAM_NODE_PROP);
        if (lat_node) HIPCHK(c, launch_node_prop_lat(c->d_wlat, g, ps, last, c->dims.motion_clamp, pred_pos, pred_motion, st));
        else if (!last) HIPCHK(c, launch_node_prop(c->d_w, g, ps, st));
        else HIPCHK(c, launch_node_final(c->d_w, g, ps, c->dims.motion_clamp, pred_pos, pred_motion, st));
    }
    return AG_OK;
}

// C rows of the two kinds of self-loop edge (object: attrs 1,0; tool: attrs 0,1), through the real edge chain of the
// ACTIVE precision mode on a 2-particle, 2-edge graph {(0,0),(1,1)} - bitwise what k_edge_enc produces for such edges.
// The 2-graph's inputs are constants: uploaded once per context (d_self_mini); enqueue_self_rows only launches the edge chain on
// `st`, so ag_ctx_load_weights_device / ag_adam_step refresh the rows without a wait.
struct SelfMini { float node_in[2 * NODE_IN]; float feat12[2 * F15_PITCH]; float group[2]; int recv[2]; int send[2]; int n_edges; int pad; };
int enqueue_self_rows(ag_ctx* c, hipStream_t st) {
    HIPCHK(c, hipSetDevice(c->device));
    if (!c->d_cself) HIPCHK(c, dev_alloc(c, reinterpret_cast<void**>(&c->d_cself), 256 * NFP * 4));
    if (!c->d_self_mini) {
        SelfMini h{};
        h.node_in[0] = 1.f; h.node_in[6] = 1.f;                         // object particle
        h.node_in[NODE_IN + 1] = 1.f; h.node_in[NODE_IN + 6] = 1.f;     // tool particle
        h.group[0] = 1.f;
        h.recv[0] = 0; h.recv[1] = 1; h.send[0] = 0; h.send[1] = 1; h.n_edges = 2;
        HIPCHK(c, dev_alloc(c, reinterpret_cast<void**>(&c->d_self_mini), sizeof(SelfMini)));
        HIPCHK(c, hipMemcpy(c->d_self_mini, &h, sizeof(SelfMini), hipMemcpyHostToDevice));
    }
    char* d = c->d_self_mini;
    GraphBufs g{};
    g.n_his = c->dims.n_his;
    g.node_in = reinterpret_cast<float*>(d + offsetof(SelfMini, node_in));
    g.feat12 = reinterpret_cast<float*>(d + offsetof(SelfMini, feat12));
    g.group = reinterpret_cast<float*>(d + offsetof(SelfMini, group));
    g.recv = reinterpret_cast<int*>(d + offsetof(SelfMini, recv));
    g.send = reinterpret_cast<int*>(d + offsetof(SelfMini, send));
    g.n_edges = reinterpret_cast<int*>(d + offsetof(SelfMini, n_edges));
    g.C = c->d_cself; g.B = 1; g.N = 2; g.n_p = 1; g.n_inst = 1; g.edge_cap = 2; g.c_cap = 256;
    g.wb3 = c->precision == 1 ? c->d_wb3 : nullptr;
    hipError_t e = launch_edge_enc(c->d_w, g, st);
    if (e != hipSuccess) return fail(c, AG_ERR_HIP, "self-loop C rows: %s", hipGetErrorString(e));
    return AG_OK;
}
int compute_self_rows(ag_ctx* c) {
    int rc = enqueue_self_rows(c, nullptr);
    if (rc) return rc;
    hipError_t e = hipDeviceSynchronize();
    if (e != hipSuccess) return fail(c, AG_ERR_HIP, "self-loop C rows: %s", hipGetErrorString(e));
    return AG_OK;
}

int check_topk(ag_ctx* c, int N, int topk) {
    if (N < 1 || topk < 1) return fail(c, AG_ERR_INVALID, "N and topk must be >= 1");
    if ((size_t)N > edge_build_max_particles()) return fail(c, AG_ERR_UNSUPPORTED, "N=%d exceeds the LDS-resident edge builder limit %zu", N, edge_build_max_particles());
    if (topk < N && topk > 128) return fail(c, AG_ERR_UNSUPPORTED, "topk=%d: 128 < topk < N is not implemented", topk);
    return AG_OK;
}

// the graph builder entry points (ag_build_edges, ag_build_edges_single): `a` holds the inputs, outputs and rule; the builder
// scratch (ell, deg, slice_tot, cta_flag) is carved from the slot of stream st
int build_edges(ag_ctx* c, hipStream_t st, EdgeArgs& a) {
    HIPCHK(c, hipSetDevice(c->device));
    a.slices = pick_slices(c, a.B, a.N);
    const size_t rows = (size_t)a.B * a.N;
    const int ell_stride = edge_ell_stride(a.N, a.topk);
    CallSlot* sl = nullptr;
    int rc = slot_acquire(c, st, false, &sl);
    if (rc) return rc;
    SlotGuard slot_guard(sl, st, false);
    rc = ensure_slab(c, *sl, rows * (size_t)(ell_stride + 1) * 4 + (size_t)a.B * (a.slices + 1) * 4 + 4096);
    if (rc) return rc;
    a.ell = sl->slab.take<int>(rows * (size_t)std::max(1, ell_stride));
    a.deg = sl->slab.take<int>(rows);
    a.slice_tot = sl->slab.take<int>((size_t)a.B * a.slices);
    a.cta_flag = sl->slab.take<int>(a.B);
    a.pos_bstride = (long)a.N * 3; a.overflow = nullptr; a.max_nR = a.edge_cap; a.zero_on_overflow = 0;
    a.block_min_rows = c->opt.edge_block_min;
    c->prof_stream = st;
    HIPCHK(c, launch_edge_build(a, st, prof_mark, c));
    return AG_OK;
}

// DynamicsPredictor.forward over the batch, in launch chunks of Bc on a workspace carved for Bc (ag_forward, and every step of
// ag_train_step: same kernels, same bits).  n_eff: the guarded per-graph edge counts (launch_edge_guard)
int enqueue_forward(ag_ctx* c, const Work& w, int Bc, const float* d_state, const float* d_attrs, const float* d_action,
                    const float* d_phys, const float* d_group, int n_inst, const int32_t* d_recv, const int32_t* d_send,
                    const int32_t* d_row_ptr, const int* n_eff, int edge_cap, int B, int N, int n_p, float* d_pred_pos,
                    float* d_pred_motion, hipStream_t st) {
    int rc = AG_OK;
    for (int b0 = 0; b0 < B; b0 += Bc) {
        const int nb = std::min(Bc, B - b0);
        GraphBufs g = w.g;
        g.B = nb; g.n_p = n_p; g.n_his = c->dims.n_his;
        g.wb3 = c->precision == 1 ? c->d_wb3 : nullptr;
        g.group = const_cast<float*>(d_group) + (size_t)b0 * N * n_inst;
        g.recv = d_recv + (size_t)b0 * edge_cap; g.send = d_send + (size_t)b0 * edge_cap;
        g.row_ptr = d_row_ptr + (size_t)b0 * (N + 1); g.n_edges = n_eff + b0; g.n_guard = n_eff + b0;
        { Scoped p(c, FAM_PREP);
          HIPCHK(c, launch_prep(d_state + (size_t)b0 * c->dims.n_his * N * 3, d_attrs + (size_t)b0 * N * 2,
                                d_action + (size_t)b0 * N * 3, d_phys + (size_t)b0 * N, g, st)); }
        rc = run_model(c, g, d_pred_pos + (size_t)b0 * n_p * 3, d_pred_motion + (size_t)b0 * n_p * 3, st);
        if (rc) return rc;
    }
    return AG_OK;
}

}  // namespace

// ================================================================================================ C-ABI
extern "C" {

uint32_t ag_abi_version(void) { return AG_ABI_VERSION; }

const char* ag_last_error(const ag_ctx* ctx) { return ctx ? ctx->err.c_str() : "null ctx"; }

int ag_ctx_create(int32_t device_id, const ag_dims* dims, ag_ctx** out) {
    if (!dims || !out) return AG_ERR_INVALID;
    *out = nullptr;
    ag_ctx* c = new ag_ctx();
    c->device = device_id; c->dims = *dims;
    options_from_env(c->opt);
    *out = c;   // returned even on failure so the caller can read ag_last_error, then destroy
    const bool his_ok = (dims->n_his == 4 || dims->n_his == N_HIS_MAX) && dims->rel_dim == 5 + 3 * dims->n_his;
    if (dims->nf != NF || !his_ok || dims->in_dim != IN_DIM)
        return fail(c, AG_ERR_UNSUPPORTED, "kernels are built for nf=150, in_dim=6 and n_his=4 (rel_dim 17) or n_his=5 "
                    "(rel_dim 20) - got nf %d, n_his %d, in_dim %d, rel_dim %d", dims->nf, dims->n_his, dims->in_dim, dims->rel_dim);
    if (dims->pstep < 1) return fail(c, AG_ERR_INVALID, "pstep must be >= 1");
    HIPCHK(c, hipSetDevice(device_id));
    HIPCHK(c, dev_alloc(c, reinterpret_cast<void**>(&c->d_w), (size_t)WeightLayout::TOTAL * 4));
#ifdef AG_DIAG
    c->diag = diag_create();
#endif
    return AG_OK;
}

int ag_ctx_destroy(ag_ctx* c) {
    if (!c) return AG_OK;
    (void)hipSetDevice(c->device);
#ifdef AG_DIAG
    diag_destroy(c->diag);
#endif
    for (auto& p : c->prof_live) { (void)hipEventDestroy(p.e0); (void)hipEventDestroy(p.e1); }
    for (auto e : c->prof_pool) (void)hipEventDestroy(e);
    for (CallSlot& k : c->slots) slot_destroy(c, k);
    if (c->d_base_cache) (void)hipFree(c->d_base_cache);
    if (c->d_w) (void)hipFree(c->d_w);
    if (c->d_wb3) (void)hipFree(c->d_wb3);
    if (c->d_wlat) (void)hipFree(c->d_wlat);
    if (c->d_cself) (void)hipFree(c->d_cself);
    if (c->d_self_mini) (void)hipFree(c->d_self_mini);
    delete c;
    return AG_OK;
}

int ag_ctx_set_precision(ag_ctx* c, int32_t mode) {
    if (!c) return AG_ERR_INVALID;
    if (mode != 0 && mode != 1) return fail(c, AG_ERR_INVALID, "precision mode must be 0 (fp32) or 1 (bf16x3)");
    if (mode == c->precision) return AG_OK;
    if (mode == 1 && c->dims.n_his != 4) return fail(c, AG_ERR_UNSUPPORTED, "the bf16x3 chains are built for n_his=4");
    c->precision = mode;
    ++c->weights_version;
    return c->have_w ? compute_self_rows(c) : AG_OK;
}

int ag_ctx_set_chunk(ag_ctx* c, int32_t n) {
    if (!c || n < 0) return AG_ERR_INVALID;
    c->chunk = n;
    return AG_OK;
}

int ag_ctx_set_option(ag_ctx* c, const char* name, int32_t value) {
    if (!c || !name) return AG_ERR_INVALID;
    for (const OptName& n : kOptions)
        if (!strcmp(name, n.name)) {
            if (value < n.lo || value > n.hi)
                return fail(c, AG_ERR_INVALID, "option '%s' = %d is outside [%d, %d]", name, value, n.lo, n.hi);
            c->opt.*(n.field) = value;
            return AG_OK;
        }
    return fail(c, AG_ERR_INVALID, "unknown option '%s'", name);
}

int ag_ctx_get_option(ag_ctx* c, const char* name, int32_t* out) {
    if (!c || !name || !out) return AG_ERR_INVALID;
    for (const OptName& n : kOptions)
        if (!strcmp(name, n.name)) { *out = c->opt.*(n.field); return AG_OK; }
    return fail(c, AG_ERR_INVALID, "unknown option '%s'", name);
}

int ag_ctx_rollout_counts(ag_ctx* c, int64_t* out_executed, int64_t* out_needed) {
    if (!c || !out_executed || !out_needed) return AG_ERR_INVALID;
    if (c->d_plan_sums) {                                    // device-planned call: the sums are still on the device
        std::vector<int> h((size_t)c->plan_sums_n * 2);
        HIPCHK(c, hipSetDevice(c->device));
        HIPCHK(c, hipDeviceSynchronize());
        HIPCHK(c, hipMemcpy(h.data(), c->d_plan_sums, h.size() * 4, hipMemcpyDeviceToHost));
        c->fwd_needed = 0; c->fwd_executed = 0;
        for (int i = 0; i < c->plan_sums_n; ++i) { c->fwd_needed += h[2 * i]; c->fwd_executed += h[2 * i + 1]; }
        c->d_plan_sums = nullptr;
    }
    *out_executed = c->fwd_executed; *out_needed = c->fwd_needed;
    return AG_OK;
}

int ag_ctx_launch_counts(ag_ctx* c, int64_t* out2) {
    if (!c || !out2) return AG_ERR_INVALID;
    out2[0] = c->steps_enqueued; out2[1] = c->steps_bound;
    return AG_OK;
}

int ag_ctx_alloc_counts(ag_ctx* c, int64_t* out1) {
    if (!c || !out1) return AG_ERR_INVALID;
    out1[0] = c->n_allocs;
    return AG_OK;
}

int ag_ctx_share_counts(ag_ctx* c, int64_t* out3) {
    if (!c || !out3) return AG_ERR_INVALID;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipDeviceSynchronize());
    unsigned long long h[2] = {0, 0};
    int nns = 0;
    if (c->slots[c->last_slot].d_share_stats) HIPCHK(c, hipMemcpy(h, c->slots[c->last_slot].d_share_stats, sizeof h, hipMemcpyDeviceToHost));
    if (c->d_share_nns) HIPCHK(c, hipMemcpy(&nns, c->d_share_nns, 4, hipMemcpyDeviceToHost));
    out3[0] = nns; out3[1] = (int64_t)h[0]; out3[2] = (int64_t)h[1];
    return AG_OK;
}

int ag_ctx_load_weights(ag_ctx* c, const float* const* t, int32_t n) {
    if (!c) return AG_ERR_INVALID;
    if (!t || n != AG_NUM_WEIGHT_TENSORS) return fail(c, AG_ERR_INVALID, "expected %d weight tensors", AG_NUM_WEIGHT_TENSORS);
    for (int i = 0; i < n; ++i) if (!t[i]) return fail(c, AG_ERR_INVALID, "weight tensor %d is null", i);
    // the three images come from one table of the packed blocks (ag_optim.hip), shared with ag_ctx_load_weights_device
    const bool his4 = c->dims.n_his == 4;   // bf16x3 (opt-in precision mode) and latency-mode images: n_his = 4 models only
    std::vector<float> blob((size_t)WeightLayout::TOTAL, 0.f);
    std::vector<uint16_t> img(his4 ? (size_t)B3_PHASES * B3_PHASE_BYTES / 2 : 0, 0);
    std::vector<float> wl(his4 ? lat_weights_floats() : 0, 0.f);
    pack_weights_host(c->dims.rel_dim, t, blob.data(), his4 ? img.data() : nullptr, his4 ? wl.data() : nullptr);
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemcpy(c->d_w, blob.data(), blob.size() * 4, hipMemcpyHostToDevice));
    if (his4) {
        if (!c->d_wb3) HIPCHK(c, dev_alloc(c, reinterpret_cast<void**>(&c->d_wb3), img.size() * 2));
        HIPCHK(c, hipMemcpy(c->d_wb3, img.data(), img.size() * 2, hipMemcpyHostToDevice));
        if (!c->d_wlat) HIPCHK(c, dev_alloc(c, reinterpret_cast<void**>(&c->d_wlat), wl.size() * 4));
        HIPCHK(c, hipMemcpy(c->d_wlat, wl.data(), wl.size() * 4, hipMemcpyHostToDevice));
    }
    c->have_w = true;
    ++c->weights_version;
    return compute_self_rows(c);
}

int ag_build_edges(ag_ctx* c, void* stream, const float* d_pos, const uint8_t* d_mask, const uint8_t* d_tool,
                   int32_t B, int32_t N, float thr, const float* d_thr_vec, int32_t topk, int32_t cta, int32_t edge_cap,
                   int32_t* d_recv, int32_t* d_send, int32_t* d_row_ptr, int32_t* d_n_edges) {
    if (!c) return AG_ERR_INVALID;
    if (!d_pos || !d_mask || !d_tool || !d_recv || !d_send || !d_row_ptr || !d_n_edges || B < 1 || edge_cap < 1)
        return fail(c, AG_ERR_INVALID, "ag_build_edges: null pointer or empty batch");
    int rc = check_topk(c, N, topk);
    if (rc) return rc;
    EdgeArgs a{};
    a.pos = d_pos; a.mask = d_mask; a.tool = d_tool; a.thr_vec = d_thr_vec; a.thr = thr;
    a.B = B; a.N = N; a.topk = topk; a.cta = cta ? 1 : 0; a.edge_cap = edge_cap;
    a.recv = d_recv; a.send = d_send; a.row_ptr = d_row_ptr; a.n_edges = d_n_edges;
    return build_edges(c, static_cast<hipStream_t>(stream), a);
}

int ag_build_edges_single(ag_ctx* c, void* stream, const float* d_pos, const uint8_t* d_mask, const uint8_t* d_tool,
                          int32_t N, float thr2, float cull_radius, int32_t topk, int32_t cta, int32_t edge_cap,
                          int32_t* d_recv, int32_t* d_send, int32_t* d_row_ptr, int32_t* d_n_edges) {
    if (!c) return AG_ERR_INVALID;
    if (!d_pos || !d_mask || !d_tool || !d_recv || !d_send || !d_row_ptr || !d_n_edges || edge_cap < 1)
        return fail(c, AG_ERR_INVALID, "ag_build_edges_single: null pointer");
    if (!(cull_radius * cull_radius >= thr2)) return fail(c, AG_ERR_INVALID, "cull_radius^2 must be >= thr2");
    int rc = check_topk(c, N, topk);
    if (rc) return rc;
    EdgeArgs a{};
    a.pos = d_pos; a.mask = d_mask; a.tool = d_tool; a.thr_vec = nullptr; a.thr = cull_radius;
    a.thr2_override = thr2; a.use_thr2 = 1;
    a.B = 1; a.N = N; a.topk = topk; a.cta = cta ? 2 : 0; a.edge_cap = edge_cap;
    a.recv = d_recv; a.send = d_send; a.row_ptr = d_row_ptr; a.n_edges = d_n_edges;
    return build_edges(c, static_cast<hipStream_t>(stream), a);
}

int ag_edges_apply_tool_rule(ag_ctx* c, void* stream, const float* d_pos, const uint8_t* d_mask, const uint8_t* d_tool,
                             int32_t N, int32_t n_tools, const int32_t* d_send_in, const int32_t* d_row_ptr_in,
                             const uint8_t* d_subset, double kNN, int32_t edge_cap, int32_t* d_recv, int32_t* d_send,
                             int32_t* d_row_ptr, int32_t* d_n_out) {
    if (!c) return AG_ERR_INVALID;
    if (!d_pos || !d_mask || !d_tool || !d_send_in || !d_row_ptr_in || !d_subset || !d_recv || !d_send || !d_row_ptr || !d_n_out)
        return fail(c, AG_ERR_INVALID, "ag_edges_apply_tool_rule: null pointer");
    if (N < 1 || n_tools < 0 || n_tools > N || edge_cap < 1)
        return fail(c, AG_ERR_INVALID, "ag_edges_apply_tool_rule: bad sizes N=%d n_tools=%d edge_cap=%d", N, n_tools, edge_cap);
    if (N > 4096) return fail(c, AG_ERR_UNSUPPORTED, "ag_edges_apply_tool_rule: N=%d exceeds 4096", N);
    if (d_send_in == d_send || d_row_ptr_in == d_row_ptr)
        return fail(c, AG_ERR_INVALID, "ag_edges_apply_tool_rule: input and output arrays must differ");
    HIPCHK(c, hipSetDevice(c->device));
    const size_t pairs = (size_t)N * (size_t)std::max(1, n_tools);
    hipStream_t st = static_cast<hipStream_t>(stream);
    CallSlot* sl = nullptr;
    int rc = slot_acquire(c, st, false, &sl);
    if (rc) return rc;
    SlotGuard slot_guard(sl, st, false);
    rc = ensure_slab(c, *sl, pairs * 6 + (size_t)(N + n_tools + 16) * 4 + 8 * 256);
    if (rc) return rc;
    RuleArgs a{};
    a.pos = d_pos; a.mask = d_mask; a.tool = d_tool; a.subset = d_subset; a.send_in = d_send_in; a.row_ptr_in = d_row_ptr_in;
    a.N = N; a.n_tools = n_tools; a.edge_cap = edge_cap; a.use_knn = (kNN < 1.0 && kNN > 0.0) ? 1 : 0; a.kNN = kNN;   // graph.py:156
    a.tlist = sl->slab.take<int>(std::max(1, n_tools));
    a.misc = sl->slab.take<int>(16);
    a.pdis = sl->slab.take<float>(pairs);
    a.keep = sl->slab.take<uint8_t>(pairs);
    a.kept = sl->slab.take<uint8_t>(pairs);
    a.deg = sl->slab.take<int>(N);
    a.recv = d_recv; a.send = d_send; a.row_ptr = d_row_ptr; a.n_out = d_n_out;
    HIPCHK(c, launch_tool_rule(a, st));
    return AG_OK;
}

int ag_forward(ag_ctx* c, void* stream, const float* d_state, const float* d_attrs, const float* d_action,
               const float* d_phys, const float* d_group, int32_t n_inst, const int32_t* d_recv, const int32_t* d_send,
               const int32_t* d_row_ptr, const int32_t* d_n_edges, int32_t edge_cap, int32_t B, int32_t N, int32_t n_p,
               float* d_pred_pos, float* d_pred_motion) {
    if (!c) return AG_ERR_INVALID;
    if (!c->have_w) return fail(c, AG_ERR_NO_WEIGHTS, "ag_forward before ag_ctx_load_weights");
    if (!d_state || !d_attrs || !d_action || !d_phys || !d_group || !d_recv || !d_send || !d_row_ptr || !d_n_edges ||
        !d_pred_pos || !d_pred_motion)
        return fail(c, AG_ERR_INVALID, "ag_forward: null pointer");
    if (B < 1 || N < 1 || n_p < 1 || n_p > N || n_inst < 1 || edge_cap < 1)
        return fail(c, AG_ERR_INVALID, "ag_forward: bad sizes B=%d N=%d n_p=%d n_inst=%d edge_cap=%d", B, N, n_p, n_inst, edge_cap);
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    c->prof_stream = st;
    const int c_cap = (int)round_up(edge_cap, 256);
    const int Bc = clamp_chunk_for_offsets(auto_chunk(c, B, N), N, c_cap);
    Work w{};
    CallSlot* sl = nullptr;
    int rc = slot_acquire(c, st, false, &sl);
    if (rc) return rc;
    SlotGuard slot_guard(sl, st, false);
    rc = ensure_slab(c, *sl, work_bytes(Bc, N, n_inst, edge_cap, c_cap, 1, false, false, false, n_p, 0) + (size_t)B * 4 + 512);
    if (rc) return rc;
    rc = carve_work(c, sl->slab, w, Bc, N, n_inst, edge_cap, c_cap, 1, false, false, false, n_p, 0);
    if (rc) return rc;
    // the caller's graphs may be overflowed (true count > edge_cap, indices never written): guard, then report
    int* n_eff = sl->slab.take<int>((size_t)B);
    if (sl->slab.used > sl->slab.cap) return fail(c, AG_ERR_INVALID, "internal: workspace carve overflow");
    HIPCHK(c, hipMemsetAsync(sl->d_words, 0, 4, st));
    HIPCHK(c, launch_edge_guard(d_n_edges, B, edge_cap, n_eff, sl->d_words, st));
    rc = enqueue_forward(c, w, Bc, d_state, d_attrs, d_action, d_phys, d_group, n_inst, d_recv, d_send, d_row_ptr, n_eff, edge_cap,
                         B, N, n_p, d_pred_pos, d_pred_motion, st);
    if (rc) return rc;
    int seen = 0;
    HIPCHK(c, hipMemcpyAsync(&seen, sl->d_words, 4, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    if (seen > 0) return fail(c, AG_ERR_MAX_NR, "Exceeds max dims: a graph had %d edges, edge_cap=%d", seen, edge_cap);
    return AG_OK;
}

int ag_backward(ag_ctx* c, void* stream, const float* d_state, const float* d_attrs, const float* d_action,
                const float* d_phys, const float* d_group, int32_t n_inst, const int32_t* d_recv, const int32_t* d_send,
                const int32_t* d_row_ptr, const int32_t* d_n_edges, int32_t edge_cap, int32_t B, int32_t N, int32_t n_p,
                const float* const* d_w, const float* d_grad_pos, const float* d_grad_motion, float* d_grad_state,
                float* const* d_grad_w) {
    return ag_backward_inputs(c, stream, d_state, d_attrs, d_action, d_phys, d_group, n_inst, d_recv, d_send, d_row_ptr, d_n_edges,
                              edge_cap, B, N, n_p, d_w, d_grad_pos, d_grad_motion, d_grad_state, d_grad_w, nullptr, nullptr);
}

int ag_backward_inputs(ag_ctx* c, void* stream, const float* d_state, const float* d_attrs, const float* d_action,
                       const float* d_phys, const float* d_group, int32_t n_inst, const int32_t* d_recv, const int32_t* d_send,
                       const int32_t* d_row_ptr, const int32_t* d_n_edges, int32_t edge_cap, int32_t B, int32_t N, int32_t n_p,
                       const float* const* d_w, const float* d_grad_pos, const float* d_grad_motion, float* d_grad_state,
                       float* const* d_grad_w, float* d_grad_phys, float* d_grad_action) {
    if (!c) return AG_ERR_INVALID;
    if (!d_state || !d_attrs || !d_action || !d_phys || !d_group || !d_recv || !d_send || !d_row_ptr || !d_n_edges || !d_w)
        return fail(c, AG_ERR_INVALID, "ag_backward: null pointer");
    for (int k = 0; k < 22; ++k)
        if (!d_w[k]) return fail(c, AG_ERR_INVALID, "ag_backward: null parameter %d", k);
    if (B < 1 || N < 1 || n_p < 1 || n_p > N || n_inst < 1 || edge_cap < 1)
        return fail(c, AG_ERR_INVALID, "ag_backward: bad sizes B=%d N=%d n_p=%d n_inst=%d edge_cap=%d", B, N, n_p, n_inst, edge_cap);
    if (c->dims.nf != NF || c->dims.in_dim != IN_DIM || c->dims.rel_dim != 5 + 3 * c->dims.n_his || c->dims.pstep < 1 || c->dims.pstep > 7)
        return fail(c, AG_ERR_UNSUPPORTED, "ag_backward: nf %d, in_dim %d, rel_dim %d, pstep %d not served", c->dims.nf, c->dims.in_dim,
                    c->dims.rel_dim, c->dims.pstep);
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    // the edge counts size the workspace (rows per graph = the largest count) and carry the overflow verdict
    std::vector<int32_t> ne((size_t)B);
    HIPCHK(c, hipMemcpyAsync(ne.data(), d_n_edges, (size_t)B * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    int emax = 0;
    for (int v : ne) emax = std::max(emax, v);
    if (emax > edge_cap) return fail(c, AG_ERR_MAX_NR, "Exceeds max dims: a graph had %d edges, edge_cap=%d", emax, edge_cap);
    TrainArgs t{};
    t.state = d_state; t.attrs = d_attrs; t.action = d_action; t.phys = d_phys; t.group = d_group; t.n_inst = n_inst;
    t.recv = d_recv; t.send = d_send; t.row_ptr = d_row_ptr; t.n_edges = d_n_edges; t.edge_cap = edge_cap;
    t.B = B; t.N = N; t.n_p = n_p; t.n_his = c->dims.n_his; t.pstep = c->dims.pstep; t.clamp = c->dims.motion_clamp;
    t.Ep = std::max(1, emax);
    t.dpos = d_grad_pos; t.dmot = d_grad_motion; t.dstate = d_grad_state;
    t.dphys = d_grad_phys; t.daction = d_grad_action;
    for (int k = 0; k < 22 && d_grad_w; ++k) t.want_w = t.want_w || d_grad_w[k] != nullptr;   // else: data gradients only
    // chunk: the context's chunk if set, else as many candidates as fit a 4-GiB workspace
    const size_t per_cand = train_work_floats(1, N, t.Ep, t.n_his, t.pstep) * 4 + train_work_ints(1, N, t.Ep) * 4;
    int Bc = (int)std::max<size_t>(1, std::min<size_t>((size_t)B, (size_t(4) << 30) / per_cand));
    if (c->chunk > 0) Bc = std::min(Bc, (int)c->chunk);
    else if (c->opt.chunk > 0) Bc = std::min(Bc, c->opt.chunk);
    size_t gw_floats = 0;
    const int ncols[11] = {IN_DIM, NF, NF, c->dims.rel_dim, NF, NF, 2 * NF, 3 * NF, NF, NF, NF};
    for (int l = 0; l < 11; ++l) gw_floats += (size_t)(l == 10 ? 3 : NF) * (ncols[l] + 1) + 128;
    const size_t wf = train_work_floats(Bc, N, t.Ep, t.n_his, t.pstep), wi = train_work_ints(Bc, N, t.Ep);
    CallSlot* sl = nullptr;
    int rc = slot_acquire(c, st, false, &sl);
    if (rc) return rc;
    SlotGuard slot_guard(sl, st, false);
    rc = ensure_slab(c, *sl, (wf + train_slab_floats() + gw_floats) * 4 + wi * 4 + 8 * 256);
    if (rc) return rc;
    float* wsf = sl->slab.take<float>(wf);
    float* slab = sl->slab.take<float>(train_slab_floats());
    int* wsi = sl->slab.take<int>(wi);
    float* acc[22];
    for (int l = 0; l < 11; ++l) {
        const int rows = l == 10 ? 3 : NF;
        acc[2 * l] = sl->slab.take<float>((size_t)rows * ncols[l]);
        acc[2 * l + 1] = sl->slab.take<float>(rows);
    }
    if (sl->slab.used > sl->slab.cap) return fail(c, AG_ERR_INVALID, "internal: workspace carve overflow");
    for (int l = 0; l < 11; ++l) {
        const int rows = l == 10 ? 3 : NF;
        HIPCHK(c, hipMemsetAsync(acc[2 * l], 0, (size_t)rows * ncols[l] * 4, st));
        HIPCHK(c, hipMemsetAsync(acc[2 * l + 1], 0, (size_t)rows * 4, st));
    }
    for (int k = 0; k < 22; ++k) { t.w[k] = d_w[k]; t.g[k] = acc[k]; }
    for (int b0 = 0; b0 < B; b0 += Bc)
        HIPCHK(c, train_backward_chunk(t, b0, std::min(Bc, B - b0), wsf, wsi, slab, st));
    for (int l = 0; l < 11 && d_grad_w; ++l) {
        const int rows = l == 10 ? 3 : NF;
        if (d_grad_w[2 * l]) HIPCHK(c, hipMemcpyAsync(d_grad_w[2 * l], acc[2 * l], (size_t)rows * ncols[l] * 4, hipMemcpyDeviceToDevice, st));
        if (d_grad_w[2 * l + 1]) HIPCHK(c, hipMemcpyAsync(d_grad_w[2 * l + 1], acc[2 * l + 1], (size_t)rows * 4, hipMemcpyDeviceToDevice, st));
    }
    HIPCHK(c, hipStreamSynchronize(st));
    return AG_OK;
}

// the three weight images from 22 plain device tensors, by kernels on `st`; no host copy, no wait (first call: allocations)
static int load_weights_device(ag_ctx* c, hipStream_t st, const float* const* d_w) {
    const bool his4 = c->dims.n_his == 4;
    if (his4 && !c->d_wb3) {
        HIPCHK(c, dev_alloc(c, reinterpret_cast<void**>(&c->d_wb3), (size_t)B3_PHASES * B3_PHASE_BYTES));
        HIPCHK(c, hipMemset(c->d_wb3, 0, (size_t)B3_PHASES * B3_PHASE_BYTES));
    }
    if (his4 && !c->d_wlat) {
        HIPCHK(c, dev_alloc(c, reinterpret_cast<void**>(&c->d_wlat), lat_weights_floats() * 4));
        HIPCHK(c, hipMemset(c->d_wlat, 0, lat_weights_floats() * 4));
    }
    HIPCHK(c, launch_pack_weights(c->dims.rel_dim, d_w, c->d_w, his4 ? reinterpret_cast<uint16_t*>(c->d_wb3) : nullptr,
                                  his4 ? c->d_wlat : nullptr, st));
    c->have_w = true;
    ++c->weights_version;
    return enqueue_self_rows(c, st);
}

int ag_ctx_load_weights_device(ag_ctx* c, void* stream, const float* const* d_w) {
    if (!c) return AG_ERR_INVALID;
    if (!d_w) return fail(c, AG_ERR_INVALID, "ag_ctx_load_weights_device: null pointer");
    for (int k = 0; k < 22; ++k)
        if (!d_w[k]) return fail(c, AG_ERR_INVALID, "ag_ctx_load_weights_device: weight tensor %d is null", k);
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    CallSlot* sl = nullptr;
    int rc = slot_acquire(c, st, false, &sl);
    if (rc) return rc;
    SlotGuard slot_guard(sl, st, false);
    return load_weights_device(c, st, d_w);
}

int ag_adam_step(ag_ctx* c, void* stream, float* const* d_w, const float* const* d_grad, float* const* d_exp_avg,
                 float* const* d_exp_avg_sq, int32_t step, double lr, double beta1, double beta2, double eps, double weight_decay,
                 int32_t* d_status) {
    if (!c) return AG_ERR_INVALID;
    if (!d_w || !d_grad || !d_exp_avg || !d_exp_avg_sq || !d_status) return fail(c, AG_ERR_INVALID, "ag_adam_step: null pointer");
    for (int k = 0; k < 22; ++k)
        if (!d_w[k] || !d_grad[k] || !d_exp_avg[k] || !d_exp_avg_sq[k]) return fail(c, AG_ERR_INVALID, "ag_adam_step: null tensor %d", k);
    if (step < 1 || !(lr >= 0.0) || !(beta1 >= 0.0 && beta1 < 1.0) || !(beta2 >= 0.0 && beta2 < 1.0) || !(eps >= 0.0) || !(weight_decay >= 0.0))
        return fail(c, AG_ERR_INVALID, "ag_adam_step: step %d, lr %g, betas (%g, %g), eps %g, weight_decay %g", step, lr, beta1, beta2, eps,
                    weight_decay);
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    CallSlot* sl = nullptr;
    int rc = slot_acquire(c, st, false, &sl);
    if (rc) return rc;
    SlotGuard slot_guard(sl, st, false);
    AdamArgs a{};
    weight_tensor_sizes(c->dims.rel_dim, a.n);
    for (int k = 0; k < 22; ++k) { a.w[k] = d_w[k]; a.g[k] = d_grad[k]; a.m[k] = d_exp_avg[k]; a.v[k] = d_exp_avg_sq[k]; }
    // torch.optim.Adam forms the bias corrections and the step size as Python floats (doubles); a kernel sees them rounded to fp32
    const double bc1 = 1.0 - std::pow(beta1, (double)step), bc2 = 1.0 - std::pow(beta2, (double)step);
    a.wd = (float)weight_decay; a.one_minus_b1 = (float)(1.0 - beta1); a.b2 = (float)beta2; a.one_minus_b2 = (float)(1.0 - beta2);
    a.bc2_sqrt = (float)std::sqrt(bc2); a.eps = (float)eps; a.neg_step_size = (float)(-(lr / bc1));
    a.status = d_status;
    HIPCHK(c, launch_adam(a, st));
    return load_weights_device(c, st, d_w);
}

int ag_train_step(ag_ctx* c, void* stream, const float* d_state, const float* d_attrs, const float* d_action, const float* d_phys,
                  const float* d_group, int32_t n_inst, const int32_t* d_recv, const int32_t* d_send, const int32_t* d_row_ptr,
                  const int32_t* d_n_edges, int32_t edge_cap, int32_t B, int32_t N, int32_t n_p, const float* const* d_w,
                  int32_t n_future, const float* d_state_future, const float* d_eef_future, const float* d_action_future,
                  int32_t store_rest_state, int32_t edge_rows, int32_t want_grad, float* const* d_grad_w, float* d_loss,
                  float* d_pred, int32_t* d_status) {
    return ag_train_step_part(c, stream, d_state, d_attrs, d_action, d_phys, d_group, n_inst, d_recv, d_send, d_row_ptr, d_n_edges,
                              edge_cap, B, N, n_p, d_w, n_future, d_state_future, d_eef_future, d_action_future, store_rest_state,
                              edge_rows, want_grad, d_grad_w, d_loss, d_pred, d_status, B, 0);
}

// B_total = B, accumulate = 0 is ag_train_step: the same launches with the same arguments, so the same bits
int ag_train_step_part(ag_ctx* c, void* stream, const float* d_state, const float* d_attrs, const float* d_action, const float* d_phys,
                       const float* d_group, int32_t n_inst, const int32_t* d_recv, const int32_t* d_send, const int32_t* d_row_ptr,
                       const int32_t* d_n_edges, int32_t edge_cap, int32_t B, int32_t N, int32_t n_p, const float* const* d_w,
                       int32_t n_future, const float* d_state_future, const float* d_eef_future, const float* d_action_future,
                       int32_t store_rest_state, int32_t edge_rows, int32_t want_grad, float* const* d_grad_w, float* d_loss,
                       float* d_pred, int32_t* d_status, int32_t B_total, int32_t accumulate) {
    if (!c) return AG_ERR_INVALID;
    if (!c->have_w) return fail(c, AG_ERR_NO_WEIGHTS, "ag_train_step before ag_ctx_load_weights / ag_ctx_load_weights_device");
    if (!d_state || !d_attrs || !d_action || !d_phys || !d_group || !d_recv || !d_send || !d_row_ptr || !d_n_edges || !d_state_future ||
        !d_loss || !d_status)
        return fail(c, AG_ERR_INVALID, "ag_train_step: null pointer");
    if (B < 1 || N < 1 || n_p < 1 || n_p > N || n_inst < 1 || edge_cap < 1 || edge_rows < 1 || n_future < 1)
        return fail(c, AG_ERR_INVALID, "ag_train_step: bad sizes B=%d N=%d n_p=%d n_inst=%d edge_cap=%d edge_rows=%d n_future=%d", B, N, n_p,
                    n_inst, edge_cap, edge_rows, n_future);
    if (B_total < B) return fail(c, AG_ERR_INVALID, "ag_train_step_part: B_total=%d is below B=%d", B_total, B);
    if (n_future > 1 && (!d_eef_future || !d_action_future)) return fail(c, AG_ERR_INVALID, "ag_train_step: n_future > 1 needs eef_future and action_future");
    if (want_grad) {
        if (!d_w || !d_grad_w) return fail(c, AG_ERR_INVALID, "ag_train_step: want_grad needs d_w and d_grad_w");
        for (int k = 0; k < 22; ++k)
            if (!d_w[k] || !d_grad_w[k]) return fail(c, AG_ERR_INVALID, "ag_train_step: null parameter or gradient tensor %d", k);
        if (c->dims.pstep > 7) return fail(c, AG_ERR_UNSUPPORTED, "ag_train_step: pstep %d not served by the backward", c->dims.pstep);
    }
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    c->prof_stream = st;
    const int n_his = c->dims.n_his, rest = store_rest_state ? 1 : 0;
    const int cap = std::min(edge_cap, edge_rows);            // a graph beyond it is presented empty and reported in d_status[0]
    // forward workspace and launch chunk exactly as ag_forward's: the same kernels are chosen, the predictions are its bits
    const int c_cap = (int)round_up(edge_cap, 256);
    const int Bc = clamp_chunk_for_offsets(auto_chunk(c, B, N), N, c_cap);
    // backward: edge rows per graph = the caller's bound, launch chunk as ag_backward's
    TrainArgs t{};
    t.attrs = d_attrs; t.phys = d_phys; t.group = d_group; t.n_inst = n_inst;
    t.recv = d_recv; t.send = d_send; t.row_ptr = d_row_ptr; t.edge_cap = edge_cap;
    t.B = B; t.N = N; t.n_p = n_p; t.n_his = n_his; t.pstep = c->dims.pstep; t.clamp = c->dims.motion_clamp;
    t.Ep = cap; t.want_w = true; t.wide = accumulate != 0;
    size_t wf = 0, wi = 0;
    int Bb = 1;
    if (want_grad) {
        const size_t per_cand = train_work_floats(1, N, t.Ep, n_his, t.pstep) * 4 + train_work_ints(1, N, t.Ep) * 4;
        Bb = (int)std::max<size_t>(1, std::min<size_t>((size_t)B, (size_t(4) << 30) / per_cand));
        if (c->chunk > 0) Bb = std::min(Bb, (int)c->chunk);
        else if (c->opt.chunk > 0) Bb = std::min(Bb, c->opt.chunk);
        wf = train_work_floats(Bb, N, t.Ep, n_his, t.pstep); wi = train_work_ints(Bb, N, t.Ep);
    }
    const size_t n_state = (size_t)B * n_his * N * 3, n_act = (size_t)B * N * 3, n_pred = (size_t)B * n_p * 3;
    size_t bytes = work_bytes(Bc, N, n_inst, edge_cap, c_cap, 1, false, false, false, n_p, 0) + (size_t)B * 4;
    bytes += ((size_t)(n_future - 1) * (n_state + n_act) + (size_t)(n_future + 2) * n_pred + 2 * n_state) * 4 + train_glue_doubles() * 8;
    bytes += (wf + (want_grad ? train_slab_floats() : 0) + wi) * 4 + 32 * 256;
    CallSlot* sl = nullptr;
    int rc = slot_acquire(c, st, false, &sl);
    if (rc) return rc;
    SlotGuard slot_guard(sl, st, false);
    rc = ensure_slab(c, *sl, bytes);
    if (rc) return rc;
    Work w{};
    rc = carve_work(c, sl->slab, w, Bc, N, n_inst, edge_cap, c_cap, 1, false, false, false, n_p, 0);
    if (rc) return rc;
    int* n_eff = sl->slab.take<int>((size_t)B);
    float* S = sl->slab.take<float>((size_t)(n_future - 1) * n_state);     // model inputs of steps 1.. (step 0: the caller's)
    float* A = sl->slab.take<float>((size_t)(n_future - 1) * n_act);
    float* P = d_pred ? d_pred : sl->slab.take<float>((size_t)n_future * n_pred);
    float* motion = sl->slab.take<float>(n_pred);
    double* part = sl->slab.take<double>(train_glue_doubles());
    float* dpos = nullptr; float* D[2] = {nullptr, nullptr}; float* wsf = nullptr; float* slab = nullptr; int* wsi = nullptr;
    if (want_grad) {
        dpos = sl->slab.take<float>(n_pred);
        if (n_future > 1) { D[0] = sl->slab.take<float>(n_state); D[1] = sl->slab.take<float>(n_state); }
        wsf = sl->slab.take<float>(wf); slab = sl->slab.take<float>(train_slab_floats()); wsi = sl->slab.take<int>(wi);
    }
    if (sl->slab.used > sl->slab.cap) return fail(c, AG_ERR_INVALID, "internal: workspace carve overflow");
    HIPCHK(c, launch_edge_guard(d_n_edges, B, cap, n_eff, d_status, st));
    auto state_of = [&](int fi) { return fi == 0 ? d_state : S + (size_t)(fi - 1) * n_state; };
    auto action_of = [&](int fi) { return fi == 0 ? d_action : A + (size_t)(fi - 1) * n_act; };
    // ---- train.py:94-119: n_future chained forwards, MSE of each prediction, the next model input from it
    for (int fi = 0; fi < n_future; ++fi) {
        float* pred = P + (size_t)fi * n_pred;
        rc = enqueue_forward(c, w, Bc, state_of(fi), d_attrs, action_of(fi), d_phys, d_group, n_inst, d_recv, d_send, d_row_ptr, n_eff,
                             edge_cap, B, N, n_p, pred, motion, st);
        if (rc) return rc;
        HIPCHK(c, launch_step_loss(pred, d_state_future, B, n_p, n_future, fi, B_total, accumulate ? 1 : 0, part, d_loss, st));
        if (fi + 1 < n_future)
            HIPCHK(c, launch_next_state(state_of(fi), pred, d_eef_future, d_action_future, B, N, n_p, n_his, n_future, fi, rest,
                                        S + (size_t)fi * n_state, A + (size_t)fi * n_act, st));
    }
    if (!want_grad) return AG_OK;
    // ---- train.py:122 loss_sum.backward(): last step first; the weight gradients accumulate in the caller's tensors in that order
    int n22[22];
    weight_tensor_sizes(c->dims.rel_dim, n22);
    for (int k = 0; k < 22; ++k) {
        if (!accumulate) HIPCHK(c, hipMemsetAsync(d_grad_w[k], 0, (size_t)n22[k] * 4, st));   // else: the earlier parts' sums stay
        t.w[k] = d_w[k]; t.g[k] = d_grad_w[k];
    }
    t.n_edges = n_eff; t.dpos = dpos;
    for (int fi = n_future - 1; fi >= 0; --fi) {
        const float* dnext = fi + 1 < n_future ? D[1] : nullptr;     // total dLoss/dstate of step fi + 1
        HIPCHK(c, launch_pred_grad(P + (size_t)fi * n_pred, d_state_future, dnext, B, N, n_p, n_his, n_future, fi, B_total, dpos, st));
        t.state = state_of(fi); t.action = action_of(fi);
        t.dstate = fi > 0 ? D[0] : nullptr;                          // step 0's input is data
        for (int b0 = 0; b0 < B; b0 += Bb) HIPCHK(c, train_backward_chunk(t, b0, std::min(Bb, B - b0), wsf, wsi, slab, st));
        if (fi > 0) {
            if (dnext) HIPCHK(c, launch_dstate_carry(D[0], dnext, B, N, n_his, rest, st));
            std::swap(D[0], D[1]);
        }
    }
    return AG_OK;
}

int ag_ppm_grad_step(ag_ctx* c, void* stream, const ag_rollout_params* p, const float* d_state0, const uint8_t* d_obj_mask,
                     const float* d_eef_xz, const float* d_eef_delta, const int32_t* h_repeat, const int32_t* d_repeat,
                     const float* d_phys, const float* d_obs, const uint8_t* d_obs_mask, int32_t N_t, const float* d_row_weight,
                     const float* const* d_w, int32_t edge_rows, int32_t want_grad, float* d_state_seqs, float* d_err,
                     float* d_grad_phys, int32_t* d_status) {
    if (!c) return AG_ERR_INVALID;
    if (!c->have_w) return fail(c, AG_ERR_NO_WEIGHTS, "ag_ppm_grad_step before ag_ctx_load_weights / ag_ctx_load_weights_device");
    if (!p || !d_state0 || !d_obj_mask || !d_eef_xz || !d_eef_delta || !h_repeat || !d_repeat || !d_phys || !d_obs || !d_obs_mask ||
        !d_state_seqs || !d_err || !d_status)
        return fail(c, AG_ERR_INVALID, "ag_ppm_grad_step: null pointer");
    const int B = p->B, N_o = p->N_o, M = p->M, N = N_o + M;
    if (B < 1 || N_o < 1 || M < 0 || p->H != 1 || p->y_mode != 1 || N_t < 1 || edge_rows < 1 || p->max_nR < 1)
        return fail(c, AG_ERR_INVALID, "ag_ppm_grad_step: bad sizes B=%d N_o=%d M=%d H=%d y_mode=%d N_t=%d edge_rows=%d max_nR=%d", B, N_o, M,
                    p->H, p->y_mode, N_t, edge_rows, p->max_nR);
    if ((size_t)N_o + (size_t)N_t > chamfer_max_points())
        return fail(c, AG_ERR_UNSUPPORTED, "ag_ppm_grad_step: N_o+N_t=%d exceeds the chamfer LDS tile (%zu points)", N_o + N_t, chamfer_max_points());
    int rc = check_topk(c, N, p->topk);
    if (rc) return rc;
    if (want_grad) {
        if (!d_w || !d_grad_phys || !d_row_weight) return fail(c, AG_ERR_INVALID, "ag_ppm_grad_step: want_grad needs d_w, d_row_weight and d_grad_phys");
        for (int k = 0; k < 22; ++k)
            if (!d_w[k]) return fail(c, AG_ERR_INVALID, "ag_ppm_grad_step: null parameter tensor %d", k);
        if (c->dims.pstep > 7) return fail(c, AG_ERR_UNSUPPORTED, "ag_ppm_grad_step: pstep %d not served by the backward", c->dims.pstep);
    }
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    c->prof_stream = st;
    const int n_his = c->dims.n_his;
    // the step count and the live prefix of every step come from the host-resident repeat counts: no read-back
    int S = 0;
    for (int b = 0; b < B; ++b) S = std::max(S, (int)h_repeat[b]);
    std::vector<int> live((size_t)S + 2, 0);                  // live[s] = rows [0, live[s]) hold every row with repeat >= s
    for (int b = 0; b < B; ++b)
        for (int s = 1; s <= std::min(S, (int)h_repeat[b]); ++s) live[s] = b + 1;
    const int cap = std::min(p->max_nR, edge_rows);           // a graph beyond it is presented empty and reported in d_status[0]
    const int c_cap = (int)round_up(cap, 256);
    const int Bc = clamp_chunk_for_offsets(auto_chunk(c, B, N), N, c_cap);
    const int slices = pick_slices(c, B, N), ell = edge_ell_stride(N, p->topk);
    TrainArgs t{};
    t.n_inst = 1; t.edge_cap = cap; t.N = N; t.n_p = N_o; t.n_his = n_his; t.pstep = c->dims.pstep; t.clamp = c->dims.motion_clamp;
    t.Ep = cap; t.want_w = false;
    size_t wf = 0, wi = 0;
    int Bb = 1;
    if (want_grad) {
        const size_t per_cand = train_work_floats(1, N, t.Ep, n_his, t.pstep) * 4 + train_work_ints(1, N, t.Ep) * 4;
        Bb = (int)std::max<size_t>(1, std::min<size_t>((size_t)B, (size_t(4) << 30) / per_cand));
        if (c->chunk > 0) Bb = std::min(Bb, (int)c->chunk);
        else if (c->opt.chunk > 0) Bb = std::min(Bb, c->opt.chunk);
        wf = train_work_floats(Bb, N, t.Ep, n_his, t.pstep); wi = train_work_ints(Bb, N, t.Ep);
    }
    // workspace: [forward | builder scratch | model inputs | per-step inputs and edge lists | chamfer and backward]
    const size_t rows = (size_t)B * N, n_state = (size_t)B * n_his * N * 3, n_pred = (size_t)B * N_o * 3;
    const size_t nS = want_grad ? (size_t)std::max(S, 1) : 2, nE = want_grad ? (size_t)std::max(S, 1) : 1;
    const size_t e_ints = 2 * (size_t)B * cap + (size_t)B * (N + 1) + 2 * (size_t)B;
    size_t bytes = work_bytes(Bc, N, 1, cap, c_cap, 1, false, false, false, N_o, 0);
    bytes += (rows * (size_t)(std::max(1, ell) + 1) + (size_t)B * (slices + 1)) * 4;
    bytes += rows * 7 * 4 + 2 * rows + 2 * (size_t)B * 4 + 2 * n_pred * 4;
    bytes += nS * n_state * 4 + nE * e_ints * 4;
    if (want_grad) bytes += ((size_t)B * (N_o + N_t + 2) + 2 * n_pred + 2 * n_state + rows + wf + wi) * 4;
    bytes += (32 + 5 * nE) * 256;
    CallSlot* sl = nullptr;
    rc = slot_acquire(c, st, false, &sl);
    if (rc) return rc;
    SlotGuard slot_guard(sl, st, false);
    rc = ensure_slab(c, *sl, bytes);
    if (rc) return rc;
    Work w{};
    rc = carve_work(c, sl->slab, w, Bc, N, 1, cap, c_cap, 1, false, false, false, N_o, 0);
    if (rc) return rc;
    Slab& sb = sl->slab;
    EdgeArgs ea{};
    ea.ell = sb.take<int>(rows * (size_t)std::max(1, ell)); ea.deg = sb.take<int>(rows);
    ea.slice_tot = sb.take<int>((size_t)B * slices); ea.cta_flag = sb.take<int>(B);
    PpmBufs pb{};
    pb.B = B; pb.N_o = N_o; pb.M = M; pb.n_his = n_his;
    pb.state0 = d_state0; pb.obj_mask = d_obj_mask; pb.eef_xz = d_eef_xz; pb.eef_delta = d_eef_delta; pb.phys = d_phys;
    pb.repeat = d_repeat; pb.grip = p->gripper_offset; pb.grip_on = p->gripper_enable;
    pb.attrs = sb.take<float>(rows * 2); pb.action = sb.take<float>(rows * 3); pb.group = sb.take<float>(rows);
    pb.physN = sb.take<float>(rows); pb.mask = sb.take<uint8_t>(rows); pb.tool = sb.take<uint8_t>(rows);
    pb.ymean = sb.take<float>(B); pb.cnt = sb.take<int>(B);
    float* pred = sb.take<float>(n_pred); float* motion = sb.take<float>(n_pred);
    float* states = sb.take<float>(nS * n_state);
    std::vector<int*> e_recv(nE), e_send(nE), e_rptr(nE), e_n(nE), e_eff(nE);
    for (size_t k = 0; k < nE; ++k) {
        e_recv[k] = sb.take<int>((size_t)B * cap); e_send[k] = sb.take<int>((size_t)B * cap);
        e_rptr[k] = sb.take<int>((size_t)B * (N + 1)); e_n[k] = sb.take<int>(B); e_eff[k] = sb.take<int>(B);
    }
    int* nn = nullptr; float* cntf = nullptr; float* gseq = nullptr; float* dpos = nullptr; float* D[2] = {nullptr, nullptr};
    float* gphys = nullptr; float* wsf = nullptr; int* wsi = nullptr;
    if (want_grad) {
        nn = sb.take<int>((size_t)B * (N_o + N_t)); cntf = sb.take<float>((size_t)B * 2); gseq = sb.take<float>(n_pred);
        dpos = sb.take<float>(n_pred); D[0] = sb.take<float>(n_state); D[1] = sb.take<float>(n_state);
        gphys = sb.take<float>(rows); wsf = sb.take<float>(wf); wsi = sb.take<int>(wi);
    }
    if (sb.used > sb.cap) return fail(c, AG_ERR_INVALID, "internal: workspace carve overflow");
    auto state_of = [&](int s) { return states + (want_grad ? (size_t)(s - 1) : (size_t)((s - 1) & 1)) * n_state; };
    auto eslot = [&](int s) { return want_grad ? (size_t)(s - 1) : (size_t)0; };
    ea.mask = pb.mask; ea.tool = pb.tool; ea.thr = p->adj_thresh; ea.N = N; ea.topk = p->topk; ea.cta = p->connect_tools_all ? 1 : 0;
    ea.edge_cap = cap; ea.max_nR = cap; ea.slices = slices; ea.pos_bstride = (long)n_his * N * 3;
    ea.block_min_rows = c->opt.edge_block_min;

    // ---- forward_dynamics.py:225-372: the masked rollout, every step's model input and edge lists kept for the backward
    HIPCHK(c, hipMemsetAsync(d_state_seqs, 0, n_pred * 4, st));
    HIPCHK(c, launch_ppm_mean_y(pb, d_state0, B, st));
    HIPCHK(c, launch_ppm_init(pb, state_of(1), st));
    for (int s = 1; s <= S; ++s) {
        const int L = live[s], Ln = live[s + 1];
        const size_t k = eslot(s);
        float* cur = state_of(s);
        ea.pos = cur + (size_t)(n_his - 1) * N * 3; ea.B = L;
        ea.recv = e_recv[k]; ea.send = e_send[k]; ea.row_ptr = e_rptr[k]; ea.n_edges = e_n[k];
        HIPCHK(c, launch_edge_build(ea, st, prof_mark, c));
        HIPCHK(c, launch_edge_guard(e_n[k], L, cap, e_eff[k], d_status, st));
        rc = enqueue_forward(c, w, Bc, cur, pb.attrs, pb.action, pb.physN, pb.group, 1, e_recv[k], e_send[k], e_rptr[k], e_eff[k], cap,
                             L, N, N_o, pred, motion, st);
        if (rc) return rc;
        if (Ln > 0) HIPCHK(c, launch_ppm_mean_y(pb, pred, Ln, st));
        HIPCHK(c, launch_ppm_advance(pb, cur, pred, s, L, Ln, Ln > 0 ? state_of(s + 1) : cur, d_state_seqs, st));
    }
    // ---- the masked chamfer to the observed clouds (physics_param_optimizer.py:219-226)
    { Scoped pr(c, FAM_COST);
      HIPCHK(c, launch_chamfer(d_state_seqs, d_obs, d_obj_mask, d_obs_mask, B, N_o, N_t, B, d_err, st)); }
    if (!want_grad) return AG_OK;
    HIPCHK(c, hipMemsetAsync(d_grad_phys, 0, (size_t)B * N_o * 4, st));
    { Scoped pr(c, FAM_COST);
      HIPCHK(c, launch_chamfer_backward(d_state_seqs, d_obs, d_obj_mask, d_obs_mask, B, N_o, N_t, B, d_row_weight, nn, cntf, gseq, st)); }
    // ---- backward through the chain, last step first; edges are constants
    // (pb.cnt still holds the valid counts: a row's mask never changes)
    for (int k = 0; k < 22; ++k) { t.w[k] = d_w[k]; t.g[k] = nullptr; }
    t.attrs = pb.attrs; t.action = pb.action; t.phys = pb.physN; t.group = pb.group; t.dpos = dpos; t.dphys = gphys;
    for (int s = S; s >= 1; --s) {
        const int L = live[s], Ln = live[s + 1];
        const size_t k = eslot(s);
        HIPCHK(c, launch_ppm_pred_grad(pb, gseq, Ln > 0 ? D[1] : nullptr, s, L, Ln, dpos, st));
        t.state = state_of(s); t.recv = e_recv[k]; t.send = e_send[k]; t.row_ptr = e_rptr[k]; t.n_edges = e_eff[k]; t.B = L;
        t.dstate = s > 1 ? D[0] : nullptr;                      // step 1's input is data
        // no split-K slab: want_w = false makes every linear_dw return before it touches one (wsf stands in for the pointer; a
        // caller that turns want_w on must carve train_slab_floats() as ag_train_step does)
        for (int b0 = 0; b0 < L; b0 += Bb) HIPCHK(c, train_backward_chunk(t, b0, std::min(Bb, L - b0), wsf, wsi, wsf, st));
        HIPCHK(c, launch_ppm_accum(gphys, L, N, N_o, d_grad_phys, st));
        if (s > 1) {
            if (Ln > 0) HIPCHK(c, launch_dstate_carry(D[0], D[1], Ln, N, n_his, 0, st));
            std::swap(D[0], D[1]);
        }
    }
    return AG_OK;
}

int ag_ppm_adam_step(ag_ctx* c, void* stream, const float* d_err, const float* d_grad_phys, int32_t n_starts, int32_t n_rows,
                     int32_t N_o, int32_t start_major, int32_t apply_update, double lr, double bias_correction1,
                     double bias_correction2, double lo, double hi, float* d_x, double* d_exp_avg, double* d_exp_avg_sq,
                     int32_t hist_cap, float* d_hist_x, double* d_hist_err, double* d_best, double* d_grad_start, float* d_phys,
                     int32_t* d_status) {
    if (!c) return AG_ERR_INVALID;
    if (!d_err || !d_x || !d_hist_x || !d_hist_err || !d_best || !d_grad_start || !d_status)
        return fail(c, AG_ERR_INVALID, "ag_ppm_adam_step: null pointer");
    if (n_starts < 1 || n_rows < 1 || N_o < 1 || hist_cap < 0)
        return fail(c, AG_ERR_INVALID, "ag_ppm_adam_step: bad sizes n_starts=%d n_rows=%d N_o=%d hist_cap=%d", n_starts, n_rows, N_o, hist_cap);
    if (apply_update && (!d_grad_phys || !d_exp_avg || !d_exp_avg_sq || !d_phys || !(lr >= 0.0) || !(bias_correction1 > 0.0) ||
                         !(bias_correction2 > 0.0) || !(lo <= hi)))
        return fail(c, AG_ERR_INVALID, "ag_ppm_adam_step: update needs gradient, moments and d_phys; lr %g, bias corrections (%g, %g), bounds [%g, %g]",
                    lr, bias_correction1, bias_correction2, lo, hi);
    HIPCHK(c, hipSetDevice(c->device));
    PpmAdamArgs a{};
    a.err = d_err; a.grad = d_grad_phys; a.K = n_starts; a.n = n_rows; a.N_o = N_o; a.start_major = start_major ? 1 : 0;
    a.hist_cap = hist_cap; a.apply = apply_update ? 1 : 0; a.x = d_x; a.m = d_exp_avg; a.v = d_exp_avg_sq; a.hist_x = d_hist_x;
    a.hist_e = d_hist_err; a.best = d_best; a.gk = d_grad_start; a.phys = d_phys; a.lr = lr; a.bc1 = bias_correction1;
    a.bc2 = bias_correction2; a.lo = lo; a.hi = hi; a.status = d_status;
    HIPCHK(c, launch_ppm_adam(a, static_cast<hipStream_t>(stream)));
    return AG_OK;
}

}  // extern "C"

namespace {
// where a rollout's actions come from: decoded on the host by the caller (ag_rollout / ag_rollout_async), or raw on the
// device (ag_rollout_actions: decode + launch plan by k_roll_plan, the host never sees them)
struct ActionSrc {
    const float* d_eef_xz = nullptr; const float* d_eef_delta = nullptr; const int32_t* h_repeat = nullptr;   // host plan
    const float* d_action = nullptr; float push_length = 0.f; const float* h_tool_off = nullptr; int max_repeat = 0;
    float* d_action_seqs = nullptr;                                                                            // device plan
    int32_t* h_work = nullptr;    // ag_rollout_work: plan only - forwards each candidate would be stepped, to the host; nothing is rolled out
};

// One rollout call: its arguments and what the phases of rollout_impl decide about it, in the order they decide it.
struct RollCall {
    // ---- the call (rollout_impl)
    ag_ctx* c = nullptr; const ag_rollout_params* p = nullptr; const ActionSrc* src = nullptr;
    const float* d_state0 = nullptr; const uint8_t* d_obj_mask = nullptr; const float* d_phys_vec = nullptr;
    float* d_state_seqs = nullptr; int32_t* d_overflow = nullptr;
    hipStream_t st = nullptr; CallSlot* sl = nullptr;
    bool capturing = false, dev_plan = false, work_only = false;
    int N = 0, n_his = 0, R = 0;                           // R: the caller's bound of action_repeat (device plan)
    size_t nrep = 0;
    // ---- launch shape (plan_launch)
    int k = 0, edge_cap = 0;
    bool dedupe = false, ell_full = false, ragged = false, sort_on = false;
    int ns = 1, Bc = 1, Ba = 1, slices = 1, ell = 0, n_chunks_all = 0;
    bool prefix = false, auto_prefix = false, base_in_ctx = false, share = false;
    int R_base = 0, kb = 0, base_cap = 0, base_slices = 0;
    // ---- launch plan (upload_host_plan / launch_device_plan)
    const int32_t* h_repeat = nullptr; int* h_cand = nullptr;
    int *pl_repeat = nullptr, *pl_cand = nullptr, *pl_live = nullptr, *pl_rows = nullptr, *pl_sums = nullptr;
    const float* d_eef_xz = nullptr; const float* d_eef_delta = nullptr;   // the caller's, or decoded by the device plan
    // ---- contact-free prefix (reserve_call_memory, decide_prefix, run_prefix)
    BaseKey key{};
    float* b_states = nullptr; float* b_y = nullptr;
    int* b_rep_eff = nullptr; int* b_start = nullptr; float* b_eef = nullptr; int* b_zero = nullptr;
    bool kept = false;                                     // a kept base rollout serves the call; its contact plan has landed
    const int* d_start = nullptr; const float* d_base_states = nullptr; const float* d_base_y = nullptr;
    // ---- shared first forward (build_shared_base_graph)
    const int* base_send = nullptr; const int* base_deg = nullptr; const float* C_share = nullptr;
    // ---- chunk loop
    Work ws[ag_ctx::kMaxStreams] = {};
    hipStream_t streams[ag_ctx::kMaxStreams] = {};

    // repeat counts as the caller gave them, on the device
    const int* rep_orig() const { return dev_plan ? pl_repeat : sl->d_repeat; }
};

int check_rollout_args(ag_ctx* c, const ag_rollout_params* p, const float* d_state0, const ActionSrc& src,
                       const float* d_state_seqs, const int32_t* d_overflow_flag) {
    if (!c) return AG_ERR_INVALID;
    if (!c->have_w) return fail(c, AG_ERR_NO_WEIGHTS, "ag_rollout before ag_ctx_load_weights");
    const bool dev_plan = src.d_action != nullptr, work_only = src.h_work != nullptr;
    if (!p || !d_state0 || (!d_state_seqs && !work_only) || !d_overflow_flag ||
        (!dev_plan && (!src.d_eef_xz || !src.d_eef_delta || !src.h_repeat)) ||
        (dev_plan && (!src.d_action_seqs || (p->M > 1 && !src.h_tool_off))))
        return fail(c, AG_ERR_INVALID, "ag_rollout: null pointer");
    if (dev_plan && (src.max_repeat < 0 || src.max_repeat > 1024 || p->M > 8))
        return fail(c, AG_ERR_INVALID, "ag_rollout_actions: max_repeat must be in [0, 1024] and M <= 8 (got %d, %d)", src.max_repeat, p->M);
    if (dev_plan && p->y_mode != 0)
        return fail(c, AG_ERR_UNSUPPORTED, "ag_rollout_actions serves dynamics() (y_mode 0); the masked variant takes host-decoded actions");
    if (p->B < 1 || p->H < 1 || p->N_o < 1 || p->M < 1 || p->max_nR < 1)
        return fail(c, AG_ERR_INVALID, "ag_rollout: bad sizes B=%d H=%d N_o=%d M=%d max_nR=%d", p->B, p->H, p->N_o, p->M, p->max_nR);
    if (p->y_mode != 0 && p->y_mode != 1) return fail(c, AG_ERR_INVALID, "y_mode must be 0 or 1");
    if (p->y_mode == 1 && p->H != 1) return fail(c, AG_ERR_INVALID, "masked rollout has a single look-ahead step");
    return check_topk(c, p->N_o + p->M, p->topk);
}

// streams, launch chunks, row slices, ragged rows, and whether the contact-free prefix and the first forward are shared
void plan_launch(RollCall& r) {
    ag_ctx* c = r.c; const ag_rollout_params* p = r.p; const int N = r.N;
    const int k = r.k = std::min(N, p->topk);
    const long bound = (long)N * (k + p->M);                 // in-degree <= topk + M (radius-AND-top-k, then tool rule)
    // Fast path (top-k active; the rollout keeps its tool particles behind the object particles): the count kernel's
    // per-row sender lists are used as the graph, slot-indexed (EdgeArgs::ell_full) - no emit pass, no CSR copy.
    // Every row then owns topk + M slots whatever max_nR is (the max_nR rule is applied by k_ell_index).
    r.dedupe = c->opt.self_dedupe != 0;
    r.ell_full = c->opt.ell_graph && r.dedupe && k < N;
    r.edge_cap = (int)round_up((size_t)(r.ell_full ? bound : std::min<long>(bound, p->max_nR)), 256);
    int ns = std::max(1, std::min(c->n_streams, (int)ag_ctx::kMaxStreams));
    {   // batches of eight or more full-size chunks run on four streams (two chunks each): the memory-bound phases of
        // three chunks then hide under the MFMA-bound k_edge_enc of a fourth (1024 x 2026 cloth: 497.8 ms on two streams,
        // 491.8 on three, 488.6 on four; with fewer chunks the streams would only cut them smaller)
        const int full = auto_chunk(c, p->B, N);
        if (c->n_streams == 2 && (p->B + full - 1) / full >= 8) ns = 4;
    }
    if ((long)p->B * N < c->opt.stream_min_rows) ns = 1;   // small batches are dispatch-bound: a second stream only doubles the launches
                                          // (rope 64 x 301 rows x 20 steps: 9.99 ms on one stream, 11.3 on two; 128 x 301: 14.2 / 13.4)
    // a caller that pipelines independent calls over several streams (the planner's chunk loop) already fills the chip across
    // calls: no fork inside a call that starts while a call of another stream is still running
    if (ns > 1 && !r.capturing && c->opt.pipeline_fork == 0 && other_slot_busy(c, r.sl)) ns = 1;
    if (c->opt.streams > 0) ns = std::min(c->opt.streams, (int)ag_ctx::kMaxStreams);
    // per-kernel event times are only meaningful without cross-stream interference; bit 30 of the mask keeps the
    // streams (the durations then include whatever the other stream ran beside the kernel)
    if ((c->prof_mask & 0x3fffffffu) && !(c->prof_mask & (1u << 30))) ns = 1;
    // Ragged batches (the masked variant: every candidate has its own number of valid particles): the propagate chains
    // walk a compact row list, and one extra candidate slot per workspace - the phantom candidate, see GraphBufs - stands
    // for every masked-out particle.  Options::ragged = 0 keeps the dense rows (A/B measurements).
    r.ragged = c->opt.ragged && p->y_mode == 1 && r.d_obj_mask != nullptr;
    // (the phantom candidate's rows must stay inside the 32-bit element offsets too)
    int Bc = r.ragged ? std::max(1, clamp_chunk_for_offsets(auto_chunk(c, p->B, N) + 1, N, r.edge_cap) - 1)
                      : clamp_chunk_for_offsets(auto_chunk(c, p->B, N), N, r.edge_cap);
    if (ns > 1) Bc = std::min(Bc, (p->B + ns - 1) / ns);      // at least one chunk per stream
    {   // equal-sized chunks, a multiple of the stream count of them (no short last chunk, no idle stream at the end)
        int n_chunks = (p->B + Bc - 1) / Bc;
        if (ns > 1) n_chunks = (n_chunks + ns - 1) / ns * ns;
        Bc = (p->B + n_chunks - 1) / n_chunks;
    }
    if (p->B <= 1) ns = 1;
    if (r.work_only) { ns = 1; Bc = 1; }                     // plan only: the one workspace a base rollout needs
    r.ns = ns; r.Bc = Bc;
    r.slices = pick_slices(c, Bc, N);
    r.ell = edge_ell_stride(N, p->topk);
    r.Ba = Bc + (r.ragged ? 1 : 0);                          // candidate slots per workspace

    // Repeat-aware launch order (Options::repeat_sort).  The reference steps the WHOLE batch to the batch maximum of
    // action_repeat and discards the surplus forwards (forward_dynamics.py:156-161).  Here, per launch chunk and
    // look-ahead step, the chunk's candidates are put in descending order of their repeat count (stable): the candidates
    // that still have forwards to run at step ai are then a PREFIX of the chunk's slots, and every kernel of that step is
    // launched over that prefix only.  Executed candidate-forwards = sum of action_repeat, exactly.  A slot's candidate
    // may change between look-ahead steps: the state carried from one to the next lives in d_state_seqs, which k_roll_init
    // reads by candidate id.  Candidates are independent, so every candidate's result is bit-identical to the unsorted
    // order's.  Ragged batches (one look-ahead step) build their row list in the sorted slot order, with the row count of
    // every live prefix tabulated beside it.
    r.sort_on = c->opt.repeat_sort != 0;
    r.n_chunks_all = (p->B + Bc - 1) / Bc;
    c->d_plan_sums = nullptr;
    // Contact-free prefix (Options::share_prefix; RollArgs::start).  A tool acts on the object only through the edges it takes
    // part in, and it takes part in none while no object particle is inside its radius.  Until then a
    // candidate's object particles evolve exactly - bit for bit: a row's result does not depend on the rest of its batch - like
    // the start state WITHOUT a tool.  That base rollout is computed once per call (one candidate, tool parked out of reach);
    // k_contact_plan replays every candidate's tool along it and finds the forward of its first contact; a candidate is then
    // stepped only from there on (its slot starts from the base state and history of that step), and one that never touches
    // takes the base state of its last step.  The reference's planner samples its pushes uniformly over the workspace
    // (plan_utils.py:48-50 with planning/*.yaml:28-29): most of them never reach the object.  Look-ahead step 0 only (later
    // steps start from per-candidate states).  The contact plan decides the launch sizes, so the call waits for it once - the GPU
    // is busy with the base rollout meanwhile.
    // (connect_tools_all does not change the argument: its tool -> object edges are all-or-nothing on "some object sits inside a
    // tool particle's radius", graph.py:276-286 - the very contact that is tested; shipped cloth pushes just start on the cloth)
    bool prefix = c->opt.share_prefix != 0 && p->y_mode == 0 && !r.d_obj_mask && p->M <= 8 && !r.capturing;
    if (c->opt.share_prefix < 0 && (p->B < 64 || (long)p->B * N < 32768)) prefix = false;
    int R_base = 0;                                          // steps of the base rollout = the largest repeat of look-ahead step 0
    if (prefix) {
        if (r.dev_plan) R_base = r.R;
        else for (int b = 0; b < p->B; ++b) R_base = std::max(R_base, (int)r.h_repeat[(size_t)b * p->H]);
        if (R_base < 1) prefix = false;
    }
    r.prefix = prefix; r.R_base = R_base;
    r.auto_prefix = prefix && c->opt.share_prefix < 0;
    r.base_in_ctx = r.auto_prefix && !r.d_phys_vec;           // automatic mode: the base rollout lives in the context, for later calls

    // Shared first forward (Options::share_first).  dynamics() broadcasts ONE start state to all candidates with a constant
    // history (forward_dynamics.py:25), then builds and encodes every candidate's graph separately (:125, model.py:303).  At
    // that forward the relation input of an object-object edge - attrs, group difference, position / residual differences
    // (model.py:249-282) - does not depend on the candidate, so neither does its C row; and the object senders a candidate's
    // receiver keeps are a subset of what it keeps in the start state's graph WITHOUT the tool (a tool can only push senders
    // out of a row's top-k).  So: build that base graph once per call, run the edge chain once over its non-self edges into
    // a shared table, and let the first forward's message passing take the C row of every slot found in the base row from
    // there (k_ell_index: send_pk); per candidate only the edges with a tool at either end are encoded.  Bit-identical: a
    // row's chain does not depend on the lane / workgroup / launch that computes it.
    r.kb = std::min(p->N_o, p->topk);
    // (with the prefix sharing only the candidates that touch at once start from the start state: EdgeArgs::share_start)
    bool share = c->opt.share_first != 0 && p->y_mode == 0 && !r.d_obj_mask && r.ell_full && p->topk < p->N_o && k <= 255;
    if (c->opt.share_first < 0 && p->B < 8) share = false;   // a handful of candidates: the base build costs more than it saves
    if (r.work_only) share = false;
    {   // launches small enough for the latency-mode propagate chains (ag_lat.hip) keep their own C rows
        GraphBufs gt{};
        gt.B = std::min(Bc, p->B); gt.N = N; gt.n_his = r.n_his; gt.wb3 = c->precision == 1 ? c->d_wb3 : nullptr;
        if (lat_node_for(c, gt)) share = false;
    }
    r.share = share;
    r.base_cap = (int)round_up((size_t)p->N_o * r.kb, 256);
    r.base_slices = pick_slices(c, 1, p->N_o);
}

// the call's slab (its workspaces, the shared base graph, the prefix sharing's scratch) and the contact plan's pinned read-back
int reserve_call_memory(RollCall& r) {
    ag_ctx* c = r.c; const ag_rollout_params* p = r.p; CallSlot& sl = *r.sl; const size_t nrep = r.nrep;
    const size_t base_bytes = !r.share ? 0 : (size_t)r.base_cap * (NFP + 3) * 4 + (size_t)p->N_o * (NODE_IN + F15_PITCH + 2) * 4 +
                                             2 * (size_t)p->N_o + (size_t)(r.base_slices + 8) * 4 + 24 * 256;
    // (sized before decide_prefix may still switch the sharing off: its scratch is carved first)
    const size_t prefix_bytes = !r.prefix ? 0 : ((r.base_in_ctx ? 0 : (size_t)(r.R_base + 1) * (p->N_o * 3 + 1)) + 2 * nrep + p->B +
                                                 5 * p->M + 64) * 4 + 16 * 256;
    const size_t wb = work_bytes(r.Ba, r.N, 1, r.edge_cap, r.edge_cap, r.slices, true, true, true, p->N_o, r.ell);
    int rc = ensure_slab(c, sl, wb * r.ns + base_bytes + prefix_bytes);
    if (rc) return rc;
    if (r.prefix) {
        if (!r.base_in_ctx) { r.b_states = sl.slab.take<float>((size_t)(r.R_base + 1) * p->N_o * 3); r.b_y = sl.slab.take<float>(r.R_base + 1); }
        r.b_rep_eff = sl.slab.take<int>(nrep); r.b_start = sl.slab.take<int>(p->B);
        r.b_eef = sl.slab.take<float>((size_t)5 * p->M);     // parked tool: xz (M,2), delta (M,3)
        r.b_zero = sl.slab.take<int>(1);
        if (sl.slab.used > sl.slab.cap) return fail(c, AG_ERR_INVALID, "internal: workspace carve overflow");
    }
    for (int i = 0; i < r.ns; ++i) {
        rc = carve_work(c, sl.slab, r.ws[i], r.Ba, r.N, 1, r.edge_cap, r.edge_cap, r.slices, true, true, true, p->N_o, r.ell);
        if (rc) return rc;
    }
    // pinned read-back of the contact plan: [forwards left | repeat | flag, census x4]
    if (r.prefix || r.work_only) return grow(c, true, sl.h_rep_pin, sl.rep_pin_cap, 2 * nrep + 8, 2 * nrep + 64);
    return AG_OK;
}

// host plan: repeat counts -> per chunk and look-ahead step the launch order (descending repeat, stable), both uploaded
int upload_host_plan(RollCall& r, const int32_t* rep_src) {
    ag_ctx* c = r.c; const ag_rollout_params* p = r.p; CallSlot& sl = *r.sl; const size_t nrep = r.nrep; const int Bc = r.Bc;
    int rc = grow(c, false, sl.d_repeat, sl.repeat_cap, 2 * nrep, 2 * nrep + (nrep >> 2));
    if (rc) return rc;
    sl.h_repeat.resize(2 * nrep);
    if (rep_src != sl.h_repeat.data()) std::copy(rep_src, rep_src + nrep, sl.h_repeat.begin());
    const int32_t* h_repeat = r.h_repeat = sl.h_repeat.data();
    int* h_cand = r.h_cand = sl.h_repeat.data() + nrep;      // [li][slot] -> candidate
    for (int li = 0; li < p->H; ++li)
        for (int b0 = 0; b0 < p->B; b0 += Bc) {
            const int nb = std::min(Bc, p->B - b0);
            int* seg = h_cand + (size_t)li * p->B + b0;
            for (int b = 0; b < nb; ++b) seg[b] = b0 + b;
            if (r.sort_on)
                std::stable_sort(seg, seg + nb, [&](int x, int y) { return h_repeat[(size_t)x * p->H + li] > h_repeat[(size_t)y * p->H + li]; });
        }
    HIPCHK(c, hipMemcpyAsync(sl.d_repeat, h_repeat, 2 * nrep * 4, hipMemcpyHostToDevice, r.st));
    return AG_OK;
}

// Device plan: one kernel decodes the actions (plan_utils.py:11-20, forward_dynamics.py:42-75), orders every chunk's
// candidates by action_repeat and tabulates how many are live at every step; the launches of the chunk loop take their live
// counts from that table (device memory), so nothing of the actions ever crosses to the host.
int launch_device_plan(RollCall& r) {
    ag_ctx* c = r.c; const ag_rollout_params* p = r.p; CallSlot& sl = *r.sl; const size_t nrep = r.nrep; const int R = r.R;
    const size_t tab = (size_t)r.n_chunks_all * p->H * (R + 2);
    const size_t n_int = 2 * nrep + 2 * tab + (size_t)r.n_chunks_all * p->H * 3;
    const size_t n_flt = nrep * p->M * 5;
    const size_t bytes = round_up(n_int * 4, 256) + n_flt * 4;
    int rc = grow(c, false, sl.d_plan, sl.plan_cap, bytes, bytes + (bytes >> 2));
    if (rc) return rc;
    r.pl_repeat = reinterpret_cast<int*>(sl.d_plan); r.pl_cand = r.pl_repeat + nrep; r.pl_live = r.pl_cand + nrep;
    r.pl_rows = r.pl_live + tab; r.pl_sums = r.pl_rows + tab;
    float* pl_xz = reinterpret_cast<float*>(sl.d_plan + round_up(n_int * 4, 256)); float* pl_delta = pl_xz + nrep * p->M * 2;
    RollPlan rp{};
    rp.action = r.src->d_action; rp.push_length = r.src->push_length; rp.M = p->M;
    for (int kk = 1; kk < p->M; ++kk) rp.tool_off[kk] = r.src->h_tool_off[kk];
    rp.B = p->B; rp.H = p->H; rp.Bc = r.Bc; rp.N = r.N; rp.max_repeat = R;
    rp.decoded = r.src->d_action_seqs; rp.eef_xz = pl_xz; rp.eef_delta = pl_delta; rp.repeat = r.pl_repeat; rp.cand = r.pl_cand;
    rp.live = r.pl_live; rp.rows = r.pl_rows; rp.sums = r.pl_sums; rp.flags = r.d_overflow; rp.sort = r.sort_on ? 1 : 0;
    rp.maxrep = r.pl_sums + (size_t)r.n_chunks_all * p->H * 2;
    HIPCHK(c, launch_roll_plan(rp, r.st));
    // Every (chunk, look-ahead step)'s own maximum comes back into pinned host memory behind an event - asynchronously:
    // nothing waits for it.  The enqueue loop polls the event (hipEventQuery) and, once it has fired, stops enqueuing
    // a look-ahead step's repeats at that maximum instead of at the caller's bound (whose surplus steps would find no live
    // slot: full grids of workgroups that exit).  Until it fires the loop goes by the bound, as before.
    const size_t n_max = (size_t)r.n_chunks_all * p->H;
    rc = grow(c, true, sl.h_plan_max, sl.plan_max_cap, n_max, n_max + 64);
    if (rc) return rc;
    if (!r.capturing) {
        HIPCHK(c, hipMemcpyAsync(sl.h_plan_max, rp.maxrep, n_max * 4, hipMemcpyDeviceToHost, r.st));
        HIPCHK(c, hipEventRecord(sl.ev_plan, r.st));
    }
    r.d_eef_xz = pl_xz; r.d_eef_delta = pl_delta;
    c->d_plan_sums = r.pl_sums; c->plan_sums_n = r.n_chunks_all * p->H;
    c->fwd_executed = -1; c->fwd_needed = -1;
    return AG_OK;
}

// ---- contact plan along the base rollout (base_states, base_y: R forwards) -> forwards left per candidate, back on the host
// (the one wait of a prefix-sharing call): sl.h_rep_pin = [forwards left | repeat (device plan) | overflow flag, census x4
// (d_cnt, when given)]
int contact_plan_and_wait(RollCall& r, const float* base_states, const float* base_y, int R, const int* d_cnt) {
    ag_ctx* c = r.c; const ag_rollout_params* p = r.p; CallSlot& sl = *r.sl; const size_t nrep = r.nrep; hipStream_t st = r.st;
    ContactPlan cp{};
    cp.base_states = base_states; cp.base_y = base_y; cp.R = R;
    cp.R_bound = r.dev_plan ? r.R : 0x7fffffff;             // a device-planned candidate beyond the caller's bound is never captured
    cp.eef_xz = r.d_eef_xz; cp.eef_delta = r.d_eef_delta; cp.repeat = r.rep_orig();
    cp.B = p->B; cp.H = p->H; cp.N_o = p->N_o; cp.M = p->M; cp.thr = p->adj_thresh; cp.rep_eff = r.b_rep_eff; cp.start = r.b_start;
    cp.state_seqs = r.d_state_seqs;
    HIPCHK(c, launch_contact_plan(cp, st));
    HIPCHK(c, hipMemcpyAsync(sl.h_rep_pin, r.b_rep_eff, nrep * 4, hipMemcpyDeviceToHost, st));
    if (r.dev_plan) HIPCHK(c, hipMemcpyAsync(sl.h_rep_pin + nrep, r.pl_repeat, nrep * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipMemcpyAsync(sl.h_rep_pin + 2 * nrep, r.d_overflow, 4, hipMemcpyDeviceToHost, st));
    if (d_cnt) HIPCHK(c, hipMemcpyAsync(sl.h_rep_pin + 2 * nrep + 1, d_cnt, 16, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipEventRecord(sl.ev_plan, st));
    HIPCHK(c, hipEventSynchronize(sl.ev_plan));
    return AG_OK;
}

// Fills r.key (what a kept base rollout and a census verdict are valid for) and, in the automatic mode, decides whether the
// call shares its prefix at all (r.prefix) and whether a kept base rollout serves it (r.kept).
int decide_prefix(RollCall& r) {
    ag_ctx* c = r.c; const ag_rollout_params* p = r.p; CallSlot& sl = *r.sl; hipStream_t st = r.st;
    BaseKey& key = r.key;
    memset(&key, 0, sizeof key);                             // (padding bytes too: the keys are compared with memcmp)
    key.N_o = p->N_o; key.M = p->M; key.topk = p->topk; key.cta = p->connect_tools_all;
    key.max_nR = p->max_nR; key.n_his = r.n_his; key.precision = c->precision;
    key.pstep = c->dims.pstep; key.grip_on = p->gripper_enable; key.thr = p->adj_thresh;
    key.grip = p->gripper_offset; key.phys = p->physics_param; key.clamp = c->dims.motion_clamp;
    key.phys_vec = r.d_phys_vec; key.weights_version = c->weights_version;
    // censuses that nobody waited for (below): one that has landed and finds enough free candidates lifts the standing "not worth
    // it" verdict, so that the next call of that shape takes a proper census again
    for (CallSlot& q : c->slots)
        if (q.census_pending && !r.capturing) {
            if (hipEventQuery(q.ev_census) == hipSuccess) {
                q.census_pending = false;
                const int free_now = q.h_census[1] - q.h_census[0], rb = std::min(q.census_R, std::max(1, q.h_census[2]));
                if (c->decision.decline && c->decision.B == q.census_B && c->decision.H == q.census_H &&
                    memcmp(&c->decision.key, &q.census_key, sizeof(BaseKey)) == 0 && free_now >= std::max(64, 8 * rb))
                    c->decision.decline = false;
            } else (void)hipGetLastError();
        }
    if (!r.auto_prefix) return AG_OK;
    // Automatic mode: is the base rollout worth its latency-bound forwards?  Census of the FIRST forward (its graph needs
    // the start state only): how many candidates touch at once.  Sharing is kept when enough of them do not - a batch of
    // pushes aimed at the object (every candidate in contact from the first forward on) steps all of them anyway: worth it
    // when enough candidates are still free at the first forward to pay for the base rollout's latency-bound forwards (each
    // costs about as much as eight candidate-forwards of a full launch).
    int* d_cnt = sl.d_words + 8;                              // [0] touch at the first forward, [1] have a forward to run, [2] max repeat, [3] state words that differ
    // is the base rollout of an earlier call still good?  Same model and task scalars: compared here; same start state:
    // compared bit for bit on the device ([3])
    const bool key_ok = c->base_cache_R >= 1 && !r.d_phys_vec && memcmp(&key, &c->base_key, sizeof key) == 0;
    const bool declined = !key_ok && c->decision.decline && c->decision.B == p->B && c->decision.H == p->H &&
                          memcmp(&key, &c->decision.key, sizeof key) == 0;
    if (declined) {
        // the last census of this shape found (nearly) every push on the object: no sharing, and no waiting either - a census
        // goes out that the call does not wait for (read by a later call, above)
        r.prefix = false;
        if (sl.census_pending) return AG_OK;
    }
    ContactPlan cen{};
    cen.base_states = r.d_state0; cen.R = 1; cen.eef_xz = r.d_eef_xz; cen.eef_delta = r.d_eef_delta; cen.repeat = r.rep_orig();
    cen.B = p->B; cen.H = p->H; cen.N_o = p->N_o; cen.M = p->M; cen.thr = p->adj_thresh;
    cen.grip = p->gripper_offset; cen.grip_on = p->gripper_enable; cen.count = d_cnt;
    HIPCHK(c, hipMemsetAsync(d_cnt, 0, 16, st));
    HIPCHK(c, launch_contact_plan(cen, st));
    if (declined) {
        HIPCHK(c, hipMemcpyAsync(sl.h_census, d_cnt, 16, hipMemcpyDeviceToHost, st));
        HIPCHK(c, hipEventRecord(sl.ev_census, st));
        sl.census_pending = true; sl.census_B = p->B; sl.census_H = p->H; sl.census_R = r.R_base;
        memcpy(&sl.census_key, &key, sizeof key);
        return AG_OK;
    }
    const int* h_cnt = nullptr;
    if (key_ok) {
        // A base rollout is kept: census, state compare and the contact plan ALONG THE KEPT ROLLOUT go out together and the
        // call waits once.  (The planner calls dynamics() 40 times with one start state, plan.py:241-247: calls 2..40 come here.)
        HIPCHK(c, launch_count_diff(r.d_state0, c->d_base_cache, (long)p->N_o * 3, d_cnt + 3, st));
        const int rc = contact_plan_and_wait(r, c->d_base_cache, c->d_base_cache + (size_t)(c->base_cache_capR + 1) * p->N_o * 3,
                                             c->base_cache_R, d_cnt);
        if (rc) return rc;
        h_cnt = sl.h_rep_pin + 2 * r.nrep + 1;
    } else {
        // one tiny kernel and one wait (for it and whatever the caller enqueued on this stream before the call)
        HIPCHK(c, hipMemcpyAsync(sl.h_census + 4, d_cnt, 16, hipMemcpyDeviceToHost, st));
        HIPCHK(c, hipEventRecord(sl.ev_plan, st));
        HIPCHK(c, hipEventSynchronize(sl.ev_plan));
        h_cnt = sl.h_census + 4;
    }
    r.R_base = std::min(r.R_base, std::max(1, h_cnt[2]));     // the batch's own maximum (the device plan only knows the bound)
    r.kept = key_ok && h_cnt[3] == 0 && c->base_cache_R >= r.R_base;   // a kept base rollout is free: share
    // another start state (or a longer push than the kept rollout covers): what the plan along the kept rollout wrote is void
    if (key_ok && !r.kept && r.d_state_seqs) HIPCHK(c, hipMemsetAsync(r.d_state_seqs, 0, (size_t)p->B * p->H * p->N_o * 3 * 4, st));
    if (!r.kept && h_cnt[1] - h_cnt[0] < std::max(64, 8 * r.R_base)) r.prefix = false;
    // a census was taken: its verdict stands for later calls of this key and shape
    c->decision.decline = !r.prefix;
    if (!r.prefix) { memcpy(&c->decision.key, &key, sizeof key); c->decision.B = p->B; c->decision.H = p->H; }
    return AG_OK;
}

// GraphBufs of workspace w for nb candidate slots; with the self-loop dedupe the two constant C rows are copied behind the
// last candidate's C rows of the workspace.  Also sets the workspace's RollBufs flags.
int workspace_graph(RollCall& r, Work& w, int nb, hipStream_t s, GraphBufs& g) {
    ag_ctx* c = r.c;
    g = w.g;
    g.B = nb; g.n_p = r.p->N_o; g.n_his = r.n_his;
    g.wb3 = c->precision == 1 ? c->d_wb3 : nullptr;
    if (r.dedupe) {
        g.c_self = c->d_cself; g.ns_edge = w.ns_edge; g.n_ns = w.n_ns;
        g.self_row = (long)r.Ba * r.edge_cap;     // behind the last candidate's C rows of this workspace
        HIPCHK(c, hipMemcpyAsync(w.g.C + (size_t)g.self_row * NFP, c->d_cself, 2 * NFP * 4, hipMemcpyDeviceToDevice, s));
    }
    if (r.ell_full) { g.deg = w.deg; g.ell_stride = r.k + r.p->M; }
    w.r.ragged = r.ragged ? 1 : 0; w.r.clamp = c->dims.motion_clamp;   // (never ragged when the prefix is shared: no mask)
    return AG_OK;
}

// edge build over nb candidate slots of workspace w, from the newest frame of their histories
EdgeArgs workspace_edge_args(const RollCall& r, const Work& w, int nb) {
    const ag_rollout_params* p = r.p; const int N = r.N, n_his = r.n_his;
    EdgeArgs ea{};
    ea.pos = w.r.hist + (size_t)(n_his - 1) * N * 3; ea.pos_bstride = (long)n_his * N * 3;   // the newest frame
    ea.mask = w.r.mask; ea.tool = w.r.tool; ea.thr_vec = nullptr; ea.thr = p->adj_thresh;
    ea.B = nb; ea.N = N; ea.topk = p->topk; ea.cta = p->connect_tools_all ? 1 : 0; ea.edge_cap = r.edge_cap;
    ea.slices = r.slices; ea.ell = w.ell; ea.deg = w.deg; ea.slice_tot = w.slice_tot; ea.cta_flag = w.cta_flag;
    ea.recv = w.recv; ea.send = w.send; ea.row_ptr = w.row_ptr; ea.n_edges = w.n_edges;
    ea.overflow = r.d_overflow; ea.max_nR = p->max_nR; ea.zero_on_overflow = 1; ea.block_min_rows = r.c->opt.edge_block_min;
    if (r.ell_full) {
        ea.ell_full = 1; ea.ell = w.send; ea.ell_stride = r.k + p->M; ea.ell_bstride = r.edge_cap;
        ea.ns_edge = w.ns_edge; ea.n_ns = w.n_ns;
    }
    return ea;
}

// the RollArgs every launch of the call shares: nb slots from candidate b0 on
RollArgs roll_args(const RollCall& r, int b0, int nb) {
    const ag_rollout_params* p = r.p;
    RollArgs ra{};
    ra.B = nb; ra.B_slots = nb; ra.b0 = b0; ra.N_o = p->N_o; ra.M = p->M;
    ra.grip = p->gripper_offset; ra.grip_on = p->gripper_enable; ra.phys = p->physics_param; ra.phys_vec = r.d_phys_vec;
    ra.state0 = r.d_state0;
    return ra;
}

// shared first forward: the start state's tool-free graph, and the edge chain once over its non-self edges -> r.C_share
int build_shared_base_graph(RollCall& r) {
    ag_ctx* c = r.c; const ag_rollout_params* p = r.p; hipStream_t st = r.st; const int base_cap = r.base_cap;
    Slab& sb = r.sl->slab;
    float* b_C = sb.take<float>((size_t)base_cap * NFP);
    int* b_send = sb.take<int>(base_cap); int* b_recv = sb.take<int>(base_cap); int* b_ns = sb.take<int>(base_cap);
    float* b_node_in = sb.take<float>((size_t)p->N_o * NODE_IN);
    float* b_feat = sb.take<float>((size_t)p->N_o * F15_PITCH);
    float* b_group = sb.take<float>(p->N_o);
    int* b_deg = sb.take<int>(p->N_o);
    uint8_t* b_mask = sb.take<uint8_t>(p->N_o); uint8_t* b_tool = sb.take<uint8_t>(p->N_o);
    int* b_slice_tot = sb.take<int>(r.base_slices); int* b_cta = sb.take<int>(1);
    int* b_n_edges = sb.take<int>(1); int* b_n_ns = sb.take<int>(1);
    if (sb.used > sb.cap) return fail(c, AG_ERR_INVALID, "internal: workspace carve overflow");
    HIPCHK(c, launch_share_prep(r.d_state0, p->N_o, r.n_his, b_node_in, b_feat, b_group, b_mask, b_tool, st));
    EdgeArgs be{};
    be.pos = r.d_state0; be.pos_bstride = (long)p->N_o * 3; be.mask = b_mask; be.tool = b_tool; be.thr = p->adj_thresh;
    be.B = 1; be.N = p->N_o; be.topk = p->topk; be.cta = 0; be.edge_cap = base_cap; be.slices = r.base_slices;
    be.ell_full = 1; be.ell = b_send; be.ell_stride = r.kb; be.ell_bstride = base_cap; be.deg = b_deg;
    be.slice_tot = b_slice_tot; be.cta_flag = b_cta; be.recv = b_recv; be.send = b_send; be.n_edges = b_n_edges;
    be.ns_edge = b_ns; be.n_ns = b_n_ns; be.max_nR = 0x7fffffff; be.block_min_rows = c->opt.edge_block_min;
    HIPCHK(c, launch_edge_build(be, st, prof_mark, c));
    GraphBufs gb{};
    gb.node_in = b_node_in; gb.feat12 = b_feat; gb.group = b_group; gb.C = b_C; gb.recv = b_recv; gb.send = b_send;
    gb.n_edges = b_n_edges; gb.ns_edge = b_ns; gb.n_ns = b_n_ns; gb.B = 1; gb.N = p->N_o; gb.n_p = p->N_o; gb.n_inst = 1;
    gb.edge_cap = base_cap; gb.c_cap = base_cap; gb.n_his = r.n_his; gb.wb3 = c->precision == 1 ? c->d_wb3 : nullptr;
    gb.diag = c->diag;
    int rc = run_edge_chain(c, gb, st);
    if (rc) return rc;
    r.base_send = b_send; r.base_deg = b_deg; r.C_share = b_C; c->d_share_nns = b_n_ns;
    return AG_OK;
}

// ---- the base rollout: one candidate on workspace 0, R_base forwards with the tool parked out of reach, every state recorded
int run_base_rollout(RollCall& r) {
    ag_ctx* c = r.c; const ag_rollout_params* p = r.p; hipStream_t st = r.st;
    const float far = 1.0e6f;                                // out of every particle's reach; delta 0: it stays there
    int far_bits; memcpy(&far_bits, &far, 4);
    HIPCHK(c, hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(r.b_eef), far_bits, (size_t)2 * p->M, st));
    HIPCHK(c, hipMemsetAsync(r.b_eef + 2 * p->M, 0, (size_t)3 * p->M * 4, st));
    HIPCHK(c, hipMemsetAsync(r.b_zero, 0, 4, st));
    HIPCHK(c, hipMemcpyAsync(r.b_states, r.d_state0, (size_t)p->N_o * 3 * 4, hipMemcpyDeviceToDevice, st));   // S_0
    Work& w = r.ws[0];
    GraphBufs g;
    int rc = workspace_graph(r, w, 1, st, g);
    if (rc) return rc;
    RollArgs ra = roll_args(r, 0, 1);
    ra.H = 1; ra.eef_xz = r.b_eef; ra.eef_delta = r.b_eef + 2 * p->M; ra.repeat = r.b_zero;
    ra.write_obj_cls = 1; ra.all_states = r.b_states; ra.all_y = r.b_y;
    const EdgeArgs ea = workspace_edge_args(r, w, 1);        // (the parked tool has no object in reach: the cta rule's flag stays 0)
    { Scoped sc(c, FAM_ROLL_INIT); HIPCHK(c, launch_roll_init(ra, w.r, g, st)); }
    { Scoped sc(c, FAM_NODE_ENC); HIPCHK(c, node_enc_for(c, g, 0, 2L * p->N_o + p->M, st)); }
    for (int ai = 1; ai <= r.R_base; ++ai) {
        HIPCHK(c, launch_edge_build(ea, st, prof_mark, c));
        if (g.ns_edge && !r.ell_full) { Scoped sc(c, FAM_EDGE_EMIT); HIPCHK(c, launch_edge_nonself(w.recv, w.send, w.row_ptr, 1, r.N, r.edge_cap, w.ns_edge, w.n_ns, nullptr, st)); }
        rc = run_model(c, g, w.r.pred, w.r.motion, st);
        if (rc) return rc;
        ra.ai = ai;
        { Scoped sc(c, FAM_ROLL_UPDATE); HIPCHK(c, launch_roll_update(ra, w.r, g, st)); }
    }
    return AG_OK;
}

// ---- contact-free prefix: the base rollout (unless a kept one serves the call) and its contact plan; then the launch plan of
// the forwards that are left
int run_prefix(RollCall& r) {
    ag_ctx* c = r.c; const ag_rollout_params* p = r.p; CallSlot& sl = *r.sl; const size_t nrep = r.nrep;
    int rc = AG_OK;
    if (r.base_in_ctx) {
        const size_t row = (size_t)p->N_o * 3 + 1;
        if (!r.kept) {
            // the kept rollout is about to be replaced: calls of other streams that still read it come first
            for (CallSlot& q : c->slots)
                if (&q != &sl && q.bound && q.have_done) HIPCHK(c, hipStreamWaitEvent(r.st, q.ev_done, 0));
            c->base_cache_R = -1;
            // (room for the longest push the caller's bound allows: a later call with longer pushes re-uses the buffer)
            const size_t need = (size_t)(r.R_base + 1) * row;
            rc = grow(c, false, c->d_base_cache, c->base_cache_cap, need, std::max(need, (size_t)((r.dev_plan ? r.R : r.R_base) + 1) * row));
            if (rc) return rc;
            c->base_cache_capR = (int)(c->base_cache_cap / row) - 1;
        }
        r.b_states = c->d_base_cache; r.b_y = c->d_base_cache + (size_t)(c->base_cache_capR + 1) * p->N_o * 3;
    }
    if (!r.kept) {
        rc = run_base_rollout(r);
        if (rc) return rc;
        rc = contact_plan_and_wait(r, r.b_states, r.b_y, r.R_base, nullptr);
        if (rc) return rc;
        if (r.base_in_ctx) {
            // keep the base rollout for later calls - unless its graphs overflowed max_nR (that call must raise by itself).
            // (memcmp compares the keys, padding included: both sides are memset + field-wise filled and copied with memcpy; a
            // spurious mismatch could only cost a re-computation, never a wrong re-use)
            const bool clean = sl.h_rep_pin[2 * nrep] <= p->max_nR;
            c->base_cache_R = clean ? r.R_base : -1;
            memcpy(&c->base_key, &r.key, sizeof r.key);
        }
    }
    if (r.dev_plan) {
        c->fwd_needed = 0;
        for (size_t i = 0; i < nrep; ++i) c->fwd_needed += std::min(std::max(0, sl.h_rep_pin[nrep + i]), r.R);
        c->d_plan_sums = nullptr;
    }
    c->fwd_executed = r.kept ? 0 : r.R_base;                 // the base rollout's forwards (none when an earlier call's is re-used)
    if (!r.work_only) {
        rc = upload_host_plan(r, sl.h_rep_pin);              // launch order and sizes from the forwards that are LEFT
        if (rc) return rc;
    }
    r.d_start = r.b_start; r.d_base_states = r.b_states; r.d_base_y = r.b_y;
    return AG_OK;
}

// ag_rollout_work: forwards candidate b would be stepped by the call this one stands for: what is left of look-ahead step 0
// after its first contact (prefix sharing in play) or all of it, plus the later steps' repeats, each at most the caller's bound
int report_work(RollCall& r) {
    ag_ctx* c = r.c; const ag_rollout_params* p = r.p; CallSlot& sl = *r.sl;
    if (!r.prefix) {
        HIPCHK(c, hipMemcpyAsync(sl.h_rep_pin, r.pl_repeat, r.nrep * 4, hipMemcpyDeviceToHost, r.st));
        HIPCHK(c, hipEventRecord(sl.ev_plan, r.st));
        HIPCHK(c, hipEventSynchronize(sl.ev_plan));
    }
    for (int b = 0; b < p->B; ++b) {
        long w = 0;
        for (int li = 0; li < p->H; ++li) w += std::min(std::max(0, sl.h_rep_pin[(size_t)b * p->H + li]), r.R);
        r.src->h_work[b] = (int32_t)w;
    }
    c->d_plan_sums = nullptr;
    return AG_OK;
}

// ---- the chunk / look-ahead / repeat enqueue loop: chunk ci runs on workspace and stream ci % ns
int enqueue_chunks(RollCall& r) {
    ag_ctx* c = r.c; const ag_rollout_params* p = r.p; CallSlot& sl = *r.sl;
    const int N = r.N, ns = r.ns, Bc = r.Bc, R = r.R; const size_t nrep = r.nrep; const int32_t* h_repeat = r.h_repeat;
    const bool loop_dev = r.dev_plan && !r.prefix;           // the live counts come from the device plan's tables
    int fail_at = -1, timing_skip = 0;
#ifdef AG_DIAG   // AG_TEST_FAIL_AT_CHUNK=n (diagnostic build only): fail with AG_ERR_HIP before enqueuing chunk n, as a failed launch would
    fail_at = diag_fail_at_chunk(c->diag);
    timing_skip = diag_timing_skip(c->diag);         // AG_TIMING_SKIP (diagnostic build only): timing-only, wrong results
#endif
    bool obj_cls_ready[ag_ctx::kMaxStreams] = {false, false, false, false};   // per workspace, per call
    bool plan_landed = false;                                // device plan: the chunk maxima are in sl.h_plan_max
    c->steps_enqueued = 0; c->steps_bound = 0;
    int ci = 0;
    for (int b0 = 0; b0 < p->B; b0 += Bc, ++ci) {
        if (ci == fail_at) return fail(c, AG_ERR_HIP, "test hook: injected failure before chunk %d", ci);
        const int nb = std::min(Bc, p->B - b0);
        Work& w = r.ws[ci % ns];
        hipStream_t cs = r.streams[ci % ns];
        c->prof_stream = cs;
        GraphBufs g;
        int rc = workspace_graph(r, w, nb, cs, g);
        if (rc) return rc;
        RollArgs ra = roll_args(r, b0, nb);
        ra.H = p->H; ra.y_mode = p->y_mode; ra.state0_batched = p->y_mode == 1; ra.obj_mask = r.d_obj_mask;
        ra.eef_xz = r.d_eef_xz; ra.eef_delta = r.d_eef_delta; ra.repeat = loop_dev ? r.pl_repeat : sl.d_repeat; ra.state_seqs = r.d_state_seqs;
        ra.start = r.d_start; ra.base_states = r.d_base_states; ra.base_y = r.d_base_y;
        EdgeArgs ea = workspace_edge_args(r, w, nb);
        if (r.ragged) {   // the mask does not change during a rollout: one work list per chunk and call, in slot order (H = 1)
            const int* d_cand0 = r.sort_on ? sl.d_repeat + nrep + b0 : nullptr;
            HIPCHK(c, launch_build_rowlist(r.d_obj_mask, d_cand0, b0, nb, p->N_o, p->M, w.rowlist, w.n_rows, w.r.mask, w.deg, cs));
            HIPCHK(c, hipMemsetAsync(w.row_ptr + (size_t)nb * (N + 1), 0, (size_t)(N + 1) * 4, cs));   // CSR path: no edges
            g.rowlist = w.rowlist; g.n_rows = w.n_rows + nb;
        }
        for (int li = 0; li < p->H; ++li) {
            const int* seg = loop_dev ? nullptr : r.h_cand + (size_t)li * p->B + b0;   // slot -> candidate of this chunk and look-ahead step
            int max_rep = loop_dev ? R : 0;                  // device plan: the caller's bound; steps past a chunk's own maximum find no live slot
            if (!loop_dev) for (int b = 0; b < nb; ++b) max_rep = std::max(max_rep, h_repeat[(size_t)seg[b] * p->H + li]);
            if (max_rep == 0 && !loop_dev) continue;          // nothing of this chunk is stepped in this look-ahead step
            ra.li = li; ra.ai = 0; ra.B = nb; ra.live = nullptr;
            ra.cand = loop_dev ? r.pl_cand + (size_t)li * p->B + b0 : r.sort_on ? sl.d_repeat + nrep + (size_t)li * p->B + b0 : nullptr;
            const int* live_row = loop_dev ? r.pl_live + ((size_t)ci * p->H + li) * (R + 2) : nullptr;
            const int* rows_row = loop_dev ? r.pl_rows + ((size_t)ci * p->H + li) * (R + 2) : nullptr;
            // masked variant: the object rows depend on nothing per-candidate either (both validity variants are
            // tabulated), so they are encoded once per call and workspace; tool rows once per look-ahead step
            ra.write_obj_cls = obj_cls_ready[ci % ns] ? 0 : 1;
            { Scoped s(c, FAM_ROLL_INIT); HIPCHK(c, launch_roll_init(ra, w.r, g, cs)); }
            { Scoped s(c, FAM_NODE_ENC);
              const long tool0 = 2L * p->N_o;
              if (!obj_cls_ready[ci % ns]) HIPCHK(c, node_enc_for(c, g, 0, tool0 + (long)nb * p->M, cs));
              else HIPCHK(c, node_enc_for(c, g, tool0, (long)nb * p->M, cs)); }
            obj_cls_ready[ci % ns] = true;
            int n_live = nb;
            c->steps_bound += max_rep;
            for (int ai = 1; ai <= max_rep; ++ai) {           // forward_dynamics.py:156
                if (loop_dev) {
                    // past this chunk's own maximum no slot is live: stop as soon as the plan's maxima are known (no waiting)
                    if (!plan_landed && ai > 1 && !r.capturing) {
                        if (hipEventQuery(sl.ev_plan) == hipSuccess) plan_landed = true;
                        else (void)hipGetLastError();       // "not ready" must not be taken for a failed launch by the next check
                    }
                    if (plan_landed && ai > sl.h_plan_max[(size_t)ci * p->H + li]) break;
                }
                ++c->steps_enqueued;
                if (loop_dev) {   // grids cover the whole chunk; the kernels read how many slots are live from the plan's table
                    ea.live = live_row + ai; ra.live = live_row + ai; g.n_rows = rows_row + ai;
                } else {
                    if (r.sort_on) while (n_live > 0 && h_repeat[(size_t)seg[n_live - 1] * p->H + li] < ai) --n_live;   // descending order: a prefix
                    c->fwd_executed += n_live;
                    if (r.ragged) g.n_rows = w.n_rows + n_live;   // rows of the live slots (+ the phantom candidate's)
                }
                ea.B = n_live; g.B = n_live; ra.B = n_live;
                // the call's first forward (start state, constant history): object-object C rows from the shared table
                const bool share_step = r.share && li == 0 && ai == 1 && !lat_node_for(c, g);
                ea.send_pk = share_step ? w.send_pk : nullptr; g.send_pk = ea.send_pk;
                if (share_step) {
                    ea.base_send = r.base_send; ea.base_deg = r.base_deg; ea.base_stride = r.kb; ea.share_No = p->N_o;
                    ea.share_stats = sl.d_share_stats; g.C_share = r.C_share; g.share_kb = r.kb;
                    ea.share_start = r.d_start; ea.share_cand = ra.cand; ea.share_b0 = b0;
                }
                if (!(timing_skip & 1) || ai == 1) {
                    HIPCHK(c, launch_edge_build(ea, cs, prof_mark, c));
                    if (g.ns_edge && !r.ell_full) { Scoped s(c, FAM_EDGE_EMIT); HIPCHK(c, launch_edge_nonself(w.recv, w.send, w.row_ptr, n_live, N, r.edge_cap, w.ns_edge, w.n_ns, ea.live, cs)); }
                }
                rc = run_model(c, g, w.r.pred, w.r.motion, cs);
                if (rc) return rc;
                ra.ai = ai;
                if (!(timing_skip & 2) || ai == max_rep) { Scoped s(c, FAM_ROLL_UPDATE); HIPCHK(c, launch_roll_update(ra, w.r, g, cs)); }
            }
        }
    }
    return AG_OK;
}

// Every rollout entry point: the phases above, in order.  Each returns an AG_* code; the slot guard records the end of the
// call on every exit, and once the streams have forked they are joined whatever the chunk loop returned.
int rollout_impl(ag_ctx* c, void* stream, const ag_rollout_params* p, const float* d_state0, const uint8_t* d_obj_mask,
                 const ActionSrc& src, const float* d_phys_vec, float* d_state_seqs, int32_t* d_overflow_flag) {
    int rc = check_rollout_args(c, p, d_state0, src, d_state_seqs, d_overflow_flag);
    if (rc) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    RollCall r;
    r.c = c; r.p = p; r.src = &src; r.st = static_cast<hipStream_t>(stream);
    r.d_state0 = d_state0; r.d_obj_mask = d_obj_mask; r.d_phys_vec = d_phys_vec; r.d_state_seqs = d_state_seqs; r.d_overflow = d_overflow_flag;
    r.dev_plan = src.d_action != nullptr; r.work_only = src.h_work != nullptr; r.R = src.max_repeat;
    r.h_repeat = src.h_repeat; r.d_eef_xz = src.d_eef_xz; r.d_eef_delta = src.d_eef_delta;
    r.N = p->N_o + p->M; r.n_his = c->dims.n_his;            // n_his 4 (every planner task config) or 5 (softbody.yaml:29)
    r.nrep = (size_t)p->B * p->H;
    c->prof_stream = r.st;
    // A caller may be capturing this call into a hipGraph (tools/graph_replay.py): nothing of it may then look at the host side of
    // an event or wait - no polling of the plan's maxima, no prefix sharing (both only save work; results are the same)
    hipStreamCaptureStatus cap_status = hipStreamCaptureStatusNone;
    r.capturing = hipStreamIsCapturing(r.st, &cap_status) == hipSuccess && cap_status == hipStreamCaptureStatusActive;
    // workspace, plans and read-back buffers of this call: the slot of the caller's stream (calls on other streams have their own
    // and may still be running; a taken-over slot has been waited for)
    rc = slot_acquire(c, r.st, r.capturing, &r.sl);
    if (rc) return rc;
    SlotGuard slot_guard(r.sl, r.st, r.capturing);           // (a captured event could not be waited for outside its graph)
    c->last_slot = (int)(r.sl - c->slots);
    c->d_share_nns = nullptr;                                // pointed into a workspace of an earlier call
    if (d_state_seqs) HIPCHK(c, hipMemsetAsync(d_state_seqs, 0, (size_t)p->B * p->H * p->N_o * 3 * 4, r.st));   // forward_dynamics.py:32

    plan_launch(r);
    rc = reserve_call_memory(r);
    if (rc) return rc;
    rc = r.dev_plan ? launch_device_plan(r) : upload_host_plan(r, src.h_repeat);   // (prefix sharing plans again, with the forwards that are left)
    if (rc) return rc;
    if (!r.dev_plan) {
        c->fwd_executed = 0; c->fwd_needed = 0;
        for (size_t i = 0; i < r.nrep; ++i) c->fwd_needed += std::max(0, r.h_repeat[i]);
    }
    rc = decide_prefix(r);
    if (rc) return rc;
    HIPCHK(c, hipMemsetAsync(r.sl->d_share_stats, 0, 16, r.st));   // counters of this call (ag_ctx_share_counts)
    if (r.share) {
        rc = build_shared_base_graph(r);
        if (rc) return rc;
    }
    if (r.prefix) {
        rc = run_prefix(r);
        if (rc) return rc;
    }
    if (r.work_only) return report_work(r);
    CallSlot& sl = *r.sl;
    for (hipStream_t& s : r.streams) s = r.st;
    if (r.ns > 1) {
        HIPCHK(c, hipEventRecord(sl.ev_fork, r.st));          // inputs / memset / repeat upload are ordered before
        for (int i = 1; i < r.ns; ++i) {
            if (!sl.aux_stream[i]) {
                HIPCHK(c, stream_new(c, &sl.aux_stream[i]));
                HIPCHK(c, event_new(c, &sl.ev_join[i]));
            }
            r.streams[i] = sl.aux_stream[i];
            HIPCHK(c, hipStreamWaitEvent(sl.aux_stream[i], sl.ev_fork, 0));
        }
    }
    // whatever the chunk loop returns, the forked streams are joined back into the caller's stream, so that a failure in the
    // middle never leaves work of this call in flight on a stream the caller cannot see
    const int rc_loop = enqueue_chunks(r);
    int rc_join = AG_OK;
    for (int i = 1; i < r.ns; ++i) {
        hipError_t e = hipEventRecord(sl.ev_join[i], sl.aux_stream[i]);
        if (e == hipSuccess) e = hipStreamWaitEvent(r.st, sl.ev_join[i], 0);
        if (e != hipSuccess && rc_join == AG_OK && rc_loop == AG_OK)
            rc_join = fail(c, AG_ERR_HIP, "joining stream %d failed: %s", i, hipGetErrorString(e));
    }
    c->prof_stream = r.st;
    return rc_loop ? rc_loop : rc_join;
}
}  // namespace

extern "C" {

int ag_rollout_async(ag_ctx* c, void* stream, const ag_rollout_params* p, const float* d_state0,
                     const uint8_t* d_obj_mask, const float* d_eef_xz, const float* d_eef_delta,
                     const int32_t* h_repeat, const float* d_phys_vec, float* d_state_seqs, int32_t* d_overflow_flag) {
    ActionSrc src;
    src.d_eef_xz = d_eef_xz; src.d_eef_delta = d_eef_delta; src.h_repeat = h_repeat;
    if (c && (!d_eef_xz || !d_eef_delta || !h_repeat)) return fail(c, AG_ERR_INVALID, "ag_rollout: null pointer");
    return rollout_impl(c, stream, p, d_state0, d_obj_mask, src, d_phys_vec, d_state_seqs, d_overflow_flag);
}

int ag_rollout_actions(ag_ctx* c, void* stream, const ag_rollout_params* p, const float* d_state0, const float* d_action,
                       float push_length, const float* h_tool_offsets, int32_t max_repeat, const float* d_phys_vec,
                       float* d_state_seqs, float* d_action_seqs, int32_t* d_flags) {
    if (!c) return AG_ERR_INVALID;
    if (!d_action || !d_action_seqs || !d_flags) return fail(c, AG_ERR_INVALID, "ag_rollout_actions: null pointer");
    ActionSrc src;
    src.d_action = d_action; src.push_length = push_length; src.h_tool_off = h_tool_offsets; src.max_repeat = max_repeat;
    src.d_action_seqs = d_action_seqs;
    return rollout_impl(c, stream, p, d_state0, nullptr, src, d_phys_vec, d_state_seqs, d_flags);
}

int ag_rollout_work(ag_ctx* c, void* stream, const ag_rollout_params* p, const float* d_state0, const float* d_action,
                    float push_length, const float* h_tool_offsets, int32_t max_repeat, const float* d_phys_vec, int32_t* h_work) {
    if (!c) return AG_ERR_INVALID;
    if (!p || !d_action || !h_work) return fail(c, AG_ERR_INVALID, "ag_rollout_work: null pointer");
    hipStream_t st = static_cast<hipStream_t>(stream);
    HIPCHK(c, hipSetDevice(c->device));
    CallSlot* sl = nullptr;
    int rc = slot_acquire(c, st, false, &sl);
    if (rc) return rc;
    SlotGuard slot_guard(sl, st, false);
    const size_t nrep = (size_t)p->B * p->H;
    // scratch for what the plan kernel writes besides the plan: decoded actions (B,H,4) and the two flag words
    rc = grow(c, false, sl->d_work, sl->work_cap, nrep * 4 + 64, (nrep * 4 + 64) * 2);
    if (rc) return rc;
    HIPCHK(c, hipMemsetAsync(sl->d_work, 0, 64 * 4, st));
    ActionSrc src;
    src.d_action = d_action; src.push_length = push_length; src.h_tool_off = h_tool_offsets; src.max_repeat = max_repeat;
    src.d_action_seqs = sl->d_work + 64; src.h_work = h_work;
    return rollout_impl(c, stream, p, d_state0, nullptr, src, d_phys_vec, nullptr, reinterpret_cast<int32_t*>(sl->d_work));
}

int ag_rollout(ag_ctx* c, void* stream, const ag_rollout_params* p, const float* d_state0, const uint8_t* d_obj_mask,
               const float* d_eef_xz, const float* d_eef_delta, const int32_t* h_repeat, const float* d_phys_vec,
               float* d_state_seqs) {
    if (!c) return AG_ERR_INVALID;
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    CallSlot* sl = nullptr;
    int rc = slot_acquire(c, st, false, &sl);                 // (the call below finds the same slot: same stream)
    if (rc) return rc;
    SlotGuard slot_guard(sl, st, false);
    int* d_word = sl->d_words;
    HIPCHK(c, hipMemsetAsync(d_word, 0, 4, st));
    rc = ag_rollout_async(c, stream, p, d_state0, d_obj_mask, d_eef_xz, d_eef_delta, h_repeat, d_phys_vec, d_state_seqs, d_word);
    if (rc) return rc;
    int seen = 0;
    HIPCHK(c, hipMemcpyAsync(&seen, d_word, 4, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    if (seen > p->max_nR) return fail(c, AG_ERR_MAX_NR, "Exceeds max dims: a graph had %d edges, max_nR=%d", seen, p->max_nR);
    return AG_OK;
}

int ag_cost_chamfer(ag_ctx* c, void* stream, const float* d_x, const float* d_y, const uint8_t* d_xmask,
                    const uint8_t* d_ymask, int32_t R, int32_t N, int32_t M, int32_t By, float* d_out) {
    if (!c) return AG_ERR_INVALID;
    if (!d_x || !d_y || !d_out || R < 1 || N < 1 || M < 1 || (By != 1 && By != R))
        return fail(c, AG_ERR_INVALID, "ag_cost_chamfer: bad arguments R=%d N=%d M=%d By=%d", R, N, M, By);
    if ((size_t)N + (size_t)M > chamfer_max_points())
        return fail(c, AG_ERR_UNSUPPORTED, "ag_cost_chamfer: N+M=%d exceeds the LDS tile (%zu points)", N + M, chamfer_max_points());
    HIPCHK(c, hipSetDevice(c->device));
    c->prof_stream = static_cast<hipStream_t>(stream);
    Scoped p(c, FAM_COST);
    HIPCHK(c, launch_chamfer(d_x, d_y, d_xmask, d_ymask, R, N, M, By, d_out, static_cast<hipStream_t>(stream)));
    return AG_OK;
}

int ag_cost_chamfer_backward(ag_ctx* c, void* stream, const float* d_x, const float* d_y, const uint8_t* d_xmask,
                             const uint8_t* d_ymask, int32_t R, int32_t N, int32_t M, int32_t By, const float* d_grad_out,
                             float* d_grad_x) {
    if (!c) return AG_ERR_INVALID;
    if (!d_x || !d_y || !d_grad_out || !d_grad_x || R < 1 || N < 1 || M < 1 || (By != 1 && By != R))
        return fail(c, AG_ERR_INVALID, "ag_cost_chamfer_backward: bad arguments R=%d N=%d M=%d By=%d", R, N, M, By);
    if ((size_t)N + (size_t)M > chamfer_max_points())
        return fail(c, AG_ERR_UNSUPPORTED, "ag_cost_chamfer_backward: N+M=%d exceeds the LDS tile (%zu points)", N + M, chamfer_max_points());
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    c->prof_stream = st;
    CallSlot* sl = nullptr;
    int rc = slot_acquire(c, st, false, &sl);
    if (rc) return rc;
    SlotGuard slot_guard(sl, st, false);
    rc = ensure_slab(c, *sl, (size_t)R * (N + M + 2) * 4 + 4 * 256);
    if (rc) return rc;
    int* nn = sl->slab.take<int>((size_t)R * (N + M));
    float* cnt = sl->slab.take<float>((size_t)R * 2);
    if (sl->slab.used > sl->slab.cap) return fail(c, AG_ERR_INVALID, "internal: workspace carve overflow");
    Scoped p(c, FAM_COST);
    HIPCHK(c, launch_chamfer_backward(d_x, d_y, d_xmask, d_ymask, R, N, M, By, d_grad_out, nn, cnt, d_grad_x, st));
    return AG_OK;
}

int ag_cost_state_stats(ag_ctx* c, void* stream, const float* d_state, int32_t R, int32_t N, const float* h_box4,
                        float* d_out) {
    if (!c) return AG_ERR_INVALID;
    if (!d_state || !d_out || R < 1 || N < 1) return fail(c, AG_ERR_INVALID, "ag_cost_state_stats: bad arguments");
    HIPCHK(c, hipSetDevice(c->device));
    c->prof_stream = static_cast<hipStream_t>(stream);
    Scoped p(c, FAM_COST);
    HIPCHK(c, launch_state_stats(d_state, R, N, h_box4, d_out, static_cast<hipStream_t>(stream)));
    return AG_OK;
}

int ag_cost_penalty(ag_ctx* c, void* stream, const float* d_state_pred, const float* d_action,
                    const float* d_state_init, int32_t B, int32_t H, int32_t N, int32_t kind, float ratio, float* d_out) {
    if (!c) return AG_ERR_INVALID;
    if (!d_state_pred || !d_action || !d_state_init || !d_out || B < 1 || H < 1 || N < 1)
        return fail(c, AG_ERR_INVALID, "ag_cost_penalty: bad arguments");
    if (kind < 0 || kind > 2) return fail(c, AG_ERR_UNSUPPORTED, "penalty kind %d not implemented", kind);
    HIPCHK(c, hipSetDevice(c->device));
    c->prof_stream = static_cast<hipStream_t>(stream);
    Scoped p(c, FAM_COST);
    HIPCHK(c, launch_penalty(d_state_pred, d_action, d_state_init, B, H, N, kind, ratio, d_out, static_cast<hipStream_t>(stream)));
    return AG_OK;
}

int ag_cost_reward(ag_ctx* c, void* stream, const float* d_error, const float* d_penalty, const float* d_stats,
                   const float* d_error_max, const double* h_bbox4, int32_t B, int32_t H, float* d_reward) {
    if (!c) return AG_ERR_INVALID;
    if (!d_error || !d_penalty || !d_stats || !h_bbox4 || !d_reward || B < 1 || H < 1)
        return fail(c, AG_ERR_INVALID, "ag_cost_reward: bad arguments B=%d H=%d", B, H);
    HIPCHK(c, hipSetDevice(c->device));
    c->prof_stream = static_cast<hipStream_t>(stream);
    Scoped p(c, FAM_COST);
    HIPCHK(c, launch_reward(d_error, d_penalty, d_stats, d_error_max, h_bbox4, B, H, d_reward, static_cast<hipStream_t>(stream)));
    return AG_OK;
}

int ag_cost_cloth_combine(ag_ctx* c, void* stream, const float* d_raw, const float* d_dmax, int64_t n, float* d_out) {
    if (!c) return AG_ERR_INVALID;
    if (!d_raw || !d_out || n < 1) return fail(c, AG_ERR_INVALID, "ag_cost_cloth_combine: bad arguments");
    HIPCHK(c, hipSetDevice(c->device));
    c->prof_stream = static_cast<hipStream_t>(stream);
    Scoped p(c, FAM_COST);
    HIPCHK(c, launch_cloth_combine(d_raw, d_dmax, (long)n, d_out, static_cast<hipStream_t>(stream)));
    return AG_OK;
}

int ag_mppi_sample(ag_ctx* c, void* stream, const float* d_act_seq, const float* d_lo, const float* d_hi, const float* d_rnd,
                   const float* d_scale, int32_t S, int32_t H, int32_t mode, float push_length, float* d_out) {
    if (!c) return AG_ERR_INVALID;
    if (!d_lo || !d_hi || !d_rnd || !d_out || S < 1 || H < 1 || (mode != 0 && mode != 1) || (mode == 1 && (!d_act_seq || !d_scale)))
        return fail(c, AG_ERR_INVALID, "ag_mppi_sample: bad arguments S=%d H=%d mode=%d", S, H, mode);
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, launch_mppi_sample(d_act_seq, d_lo, d_hi, d_rnd, d_scale, S, H, mode, push_length, d_out, static_cast<hipStream_t>(stream)));
    return AG_OK;
}

int ag_mppi_update(ag_ctx* c, void* stream, const float* d_act_seqs, const float* d_reward, const float* d_lo,
                   const float* d_hi, int32_t B, int32_t H, float reward_weight, float push_length, float* d_out) {
    if (!c) return AG_ERR_INVALID;
    if (!d_act_seqs || !d_reward || !d_lo || !d_hi || !d_out || B < 1 || H < 1)
        return fail(c, AG_ERR_INVALID, "ag_mppi_update: bad arguments B=%d H=%d", B, H);
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, launch_mppi_update(d_act_seqs, d_reward, d_lo, d_hi, B, H, reward_weight, push_length, d_out, static_cast<hipStream_t>(stream)));
    return AG_OK;
}

int ag_mppi_clip(ag_ctx* c, void* stream, const float* d_in, const float* d_lo, const float* d_hi, int64_t n, float* d_out) {
    if (!c) return AG_ERR_INVALID;
    if (!d_in || !d_lo || !d_hi || !d_out || n < 1) return fail(c, AG_ERR_INVALID, "ag_mppi_clip: bad arguments");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, launch_mppi_clip(d_in, d_lo, d_hi, d_out, (long)n, static_cast<hipStream_t>(stream)));
    return AG_OK;
}

int ag_ctx_set_profiling(ag_ctx* c, int32_t mask) {
    if (!c) return AG_ERR_INVALID;
    c->prof_mask = (unsigned)mask;
    return AG_OK;
}

static int prof_collect(ag_ctx* c) {
    for (auto& p : c->prof_live) {
        hipError_t e = hipEventSynchronize(p.e1);
        if (e != hipSuccess) return fail(c, AG_ERR_HIP, "hipEventSynchronize: %s", hipGetErrorString(e));
        float ms = 0.f;
        e = hipEventElapsedTime(&ms, p.e0, p.e1);
        if (e != hipSuccess) return fail(c, AG_ERR_HIP, "hipEventElapsedTime: %s", hipGetErrorString(e));
        c->prof_ms[p.fam] += ms; c->prof_n[p.fam] += 1;
        c->prof_pool.push_back(p.e0); c->prof_pool.push_back(p.e1);
    }
    c->prof_live.clear();
    return AG_OK;
}

int ag_ctx_kernel_stats(ag_ctx* c, const char* kernel, double* out_ms, int64_t* out_n) {
    if (!c || !kernel || !out_ms || !out_n) return AG_ERR_INVALID;
    int rc = prof_collect(c);
    if (rc) return rc;
    for (int f = 0; f < FAM_COUNT; ++f)
        if (!strcmp(kernel, kFamilyNames[f])) { *out_ms = c->prof_ms[f]; *out_n = c->prof_n[f]; return AG_OK; }
    return fail(c, AG_ERR_INVALID, "unknown kernel family '%s'", kernel);
}

int ag_ctx_reset_stats(ag_ctx* c) {
    if (!c) return AG_ERR_INVALID;
    int rc = prof_collect(c);
    for (int f = 0; f < FAM_COUNT; ++f) { c->prof_ms[f] = 0; c->prof_n[f] = 0; }
    return rc;
}

}  // extern "C"
