// C-ABI of the MI355X-native GNN-dynamics rollout engine (see include/adaptigraph_amd.h).
// Host orchestration only: context, workspace, weight repacking, launch sequences.  No CPU compute fallback.
#include "ag_host.h"
#include "ag_cost.h"

#include <cstdarg>

using namespace ag;

namespace {

const char* kFamilyNames[FAM_COUNT] = {"edge_count", "edge_emit", "prep", "node_enc", "edge_enc",
                                       "mp", "node_prop", "node_final", "roll_init", "roll_update", "cost", "fps", "assemble", "rule", "surface"};

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
    {"zero_skip", "AG_ZERO_SKIP", &Options::zero_skip, false, 0, 1},
    {"half_step", "AG_HALF_STEP", &Options::half_step, false, 0, 1},
    {"share_prefix", "AG_SHARE_PREFIX", &Options::share_prefix, false, -1, 1},
    {"stream_min_rows", "AG_STREAM_MIN_ROWS", &Options::stream_min_rows, false, 0, 0x7fffffff},
    {"pipeline_fork", "AG_PIPELINE_FORK", &Options::pipeline_fork, false, 0, 1},
    {"edge_order", "AG_EDGE_ORDER", &Options::edge_order, false, 0, 2},
    {"ell_lds_words", "AG_ELL_LDS_WORDS", &Options::ell_lds_words, false, 0, 16384},
};
void options_from_env(Options& o) {   // values from the environment are clamped into the option's range
    for (const OptName& n : kOptions)
        if (const char* e = getenv(n.env)) o.*(n.field) = n.env_negates ? (atoi(e) ? 0 : 1) : std::min(n.hi, std::max(n.lo, atoi(e)));
}

}  // namespace

// ---- the helpers ag_host.h declares: defined here, once, for the three host files
namespace ag {

int fail(ag_ctx* c, int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (c) c->err = buf;
    return code;
}

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
void slot_release(CallSlot* s, hipStream_t st, bool capturing) {
    if (capturing || !s || !s->ev_done) return;
    if (hipEventRecord(s->ev_done, st) == hipSuccess) s->have_done = true;
}
bool other_slot_busy(ag_ctx* c, const CallSlot* me) {
    bool busy = false;
    for (CallSlot& k : c->slots)
        if (&k != me && k.bound && k.have_done) {
            if (hipEventQuery(k.ev_done) == hipErrorNotReady) busy = true;
            (void)hipGetLastError();
        }
    return busy;
}
int begin_call(ag_ctx* c, void* stream, SlotGuard& call, bool watch_capture) {
    HIPCHK(c, hipSetDevice(c->device));
    call.st = static_cast<hipStream_t>(stream);
    c->prof_stream = call.st;
    if (watch_capture) {
        hipStreamCaptureStatus status = hipStreamCaptureStatusNone;
        call.capturing = hipStreamIsCapturing(call.st, &status) == hipSuccess && status == hipStreamCaptureStatusActive;
    }
    return slot_acquire(c, call.st, call.capturing, &call.sl);
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

void carve_work(const ag_ctx* c, Slab& s, Work& w, int Bc, int N, int n_inst, int edge_cap, int c_cap, int slices, bool own_edges,
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
    w.g.zero_skip = c->opt.zero_skip && c->w_finite; w.g.half_step = w.g.zero_skip && c->opt.half_step;
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
        w.n_oo = s.take<int>(Bc);
        w.ck_bits = nullptr; w.ck_off = nullptr; w.ck_list = nullptr;
        // chunk list of Options::edge_order 2.  Carved whatever edge_order, ell_graph and self_dedupe say now: they are options of the
        // context and may change between calls; the cost is small.  4 bytes per (candidate, slot) of list, 2 bits of bitmap and
        // 512 counters per candidate - about 6 MB at the bench shape, under 1 % of the C rows of the same slots (NFP floats each).
        if (roll && ell_stride > 0) {
            const size_t slots = (size_t)N * (ell_stride + N - N_o);   // a row owns top-k + M slots
            w.ck_bits = s.take<unsigned long long>((size_t)Bc * 2 * ((slots + 63) / 64));
            w.ck_off = s.take<int>(2 + slots + (size_t)CHUNK_TOOL_KEYS * Bc);
            w.ck_list = s.take<unsigned>((size_t)Bc * edge_cap);
        }
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
constexpr long kMaxOffsetRows = ((1L << 32) / NFP) - 512;    // rows of NFP floats addressable with a 32-bit element offset
// A launch chunk is at least one graph, so the clamp below cannot help a single graph whose node rows or edge slots exceed the
// bound (reachable since the cell-list builder serves graphs beyond the LDS builder's 4096 particles): refused here.
int check_graph_rows(ag_ctx* c, const char* me, int N, int edge_cap) {
    const long c_cap = (long)round_up((size_t)edge_cap, 256);
    if (N > kMaxOffsetRows || c_cap > kMaxOffsetRows)
        return fail(c, AG_ERR_UNSUPPORTED, "%s: N=%d / edge_cap=%d exceed the %ld rows per graph that 32-bit activation offsets address", me, N,
                    edge_cap, kMaxOffsetRows);
    return AG_OK;
}
int clamp_chunk_for_offsets(int Bc, int N, int c_cap) {
    const long max_rows = kMaxOffsetRows;
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

ForwardFrame::ForwardFrame(const ag_ctx* c, int B, int N_, int n_inst_, int edge_cap_, int n_p_, int n_guard_)
    : N(N_), n_inst(n_inst_), edge_cap(edge_cap_), n_p(n_p_), n_guard(n_guard_), c_cap((int)round_up(edge_cap_, 256)),
      Bc(clamp_chunk_for_offsets(auto_chunk(c, B, N_), N_, c_cap)) {}
void ForwardFrame::carve(const ag_ctx* c, Slab& s) {
    carve_work(c, s, w, Bc, N, n_inst, edge_cap, c_cap, 1, false, false, false, n_p, 0);
    n_eff = n_guard ? s.take<int>((size_t)n_guard) : nullptr;
}

// (ag_forward, and every step of ag_train_step: same kernels, same bits)
int enqueue_forward(ag_ctx* c, const ForwardFrame& f, const float* d_state, const float* d_attrs, const float* d_action,
                    const float* d_phys, const float* d_group, const int32_t* d_recv, const int32_t* d_send,
                    const int32_t* d_row_ptr, const int* n_eff, int B, float* d_pred_pos, float* d_pred_motion, hipStream_t st) {
    const int Bc = f.Bc, N = f.N, n_inst = f.n_inst, edge_cap = f.edge_cap, n_p = f.n_p;
    int rc = AG_OK;
    for (int b0 = 0; b0 < B; b0 += Bc) {
        const int nb = std::min(Bc, B - b0);
        GraphBufs g = f.w.g;
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

}  // namespace ag

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
    // read-only: what the next call's chains will do - the option, and the guard on the loaded weights
    if (!strcmp(name, "zero_skip_active")) { *out = c->opt.zero_skip && c->w_finite ? 1 : 0; return AG_OK; }
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
    // zero skip leaves out products with an activation that is exactly 0: the same bits only while no weight is inf or NaN
    c->w_finite = std::all_of(blob.begin(), blob.end(), [](float v) { return std::isfinite(v); });
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
    if (int rc0 = check_graph_rows(c, "ag_forward", N, edge_cap)) return rc0;
    SlotGuard call;
    int rc = begin_call(c, stream, call);
    if (rc) return rc;
    hipStream_t st = call.st; CallSlot* sl = call.sl;
    // n_eff: the caller's graphs may be overflowed (true count > edge_cap, indices never written): guard, then report
    ForwardFrame f(c, B, N, n_inst, edge_cap, n_p, B);
    rc = carve_slab(c, *sl, [&](Slab& s) { f.carve(c, s); });
    if (rc) return rc;
    HIPCHK(c, hipMemsetAsync(sl->d_words, 0, 4, st));
    HIPCHK(c, launch_edge_guard(d_n_edges, B, edge_cap, f.n_eff, sl->d_words, st));
    rc = enqueue_forward(c, f, d_state, d_attrs, d_action, d_phys, d_group, d_recv, d_send, d_row_ptr, f.n_eff, B, d_pred_pos,
                         d_pred_motion, st);
    if (rc) return rc;
    int seen = 0;
    HIPCHK(c, hipMemcpyAsync(&seen, sl->d_words, 4, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    if (seen > 0) return fail(c, AG_ERR_MAX_NR, "Exceeds max dims: a graph had %d edges, edge_cap=%d", seen, edge_cap);
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
    SlotGuard call;
    int rc = begin_call(c, stream, call);
    if (rc) return rc;
    hipStream_t st = call.st; CallSlot* sl = call.sl;
    int* nn = nullptr; float* cnt = nullptr;
    rc = carve_slab(c, *sl, [&](Slab& s) { nn = s.take<int>((size_t)R * (N + M)); cnt = s.take<float>((size_t)R * 2); });
    if (rc) return rc;
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
