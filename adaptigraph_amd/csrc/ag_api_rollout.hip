// C-ABI, the rollout engine (see include/adaptigraph_amd.h): one RollCall per call, its phases, rollout_impl and the four
// rollout entry points.  Host orchestration only; context and shared helpers: ag_host.h.
#include "ag_host.h"

using namespace ag;

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
    struct BaseGraph { float* C; int *send, *recv, *ns; float *node_in, *feat, *group; int* deg; uint8_t *mask, *tool;
                       int *slice_tot, *cta, *n_edges, *n_ns; } bg{};   // carved by reserve_call_memory
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

// the call's slab, in this order: the prefix sharing's scratch (taken before decide_prefix may still switch the sharing off), the
// workspaces, the shared base graph; and the contact plan's pinned read-back
int reserve_call_memory(RollCall& r) {
    ag_ctx* c = r.c; const ag_rollout_params* p = r.p; CallSlot& sl = *r.sl; const size_t nrep = r.nrep;
    int rc = carve_slab(c, sl, [&](Slab& s) {
        if (r.prefix) {
            if (!r.base_in_ctx) { r.b_states = s.take<float>((size_t)(r.R_base + 1) * p->N_o * 3); r.b_y = s.take<float>(r.R_base + 1); }
            r.b_rep_eff = s.take<int>(nrep); r.b_start = s.take<int>(p->B);
            r.b_eef = s.take<float>((size_t)5 * p->M);         // parked tool: xz (M,2), delta (M,3)
            r.b_zero = s.take<int>(1);
        }
        for (int i = 0; i < r.ns; ++i)
            carve_work(c, s, r.ws[i], r.Ba, r.N, 1, r.edge_cap, r.edge_cap, r.slices, true, true, true, p->N_o, r.ell);
        if (r.share) {
            RollCall::BaseGraph& b = r.bg;
            b.C = s.take<float>((size_t)r.base_cap * NFP);
            b.send = s.take<int>(r.base_cap); b.recv = s.take<int>(r.base_cap); b.ns = s.take<int>(r.base_cap);
            b.node_in = s.take<float>((size_t)p->N_o * NODE_IN); b.feat = s.take<float>((size_t)p->N_o * F15_PITCH);
            b.group = s.take<float>(p->N_o); b.deg = s.take<int>(p->N_o);
            b.mask = s.take<uint8_t>(p->N_o); b.tool = s.take<uint8_t>(p->N_o);
            b.slice_tot = s.take<int>(r.base_slices); b.cta = s.take<int>(1);
            b.n_edges = s.take<int>(1); b.n_ns = s.take<int>(1);
        }
    });
    if (rc) return rc;
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

// Options::edge_order 2 for one launch: the relation encoder reads ONE list over the launch's live candidates (EdgeArgs::ck_list).
// Only where the fp32 throughput chain runs on the slot-indexed graph with the self-loop dedupe, and (candidate, slot) fits the 32-bit
// entry; every other launch keeps order 1.  g.B = the launch's candidates (the latency chains take over small launches).
void chunk_list_for(const RollCall& r, const Work& w, EdgeArgs& ea, GraphBufs& g) {
    ag_ctx* c = r.c;
    ea.ck_list = nullptr; ea.ck_bits = nullptr; ea.ck_off = nullptr; ea.ck_shift = 0;
    g.ck_list = nullptr; g.ck_n = nullptr; g.ck_shift = 0;
    if (c->opt.edge_order != 2 || !r.ell_full || !r.dedupe || !w.ck_list || g.wb3 || g.B <= 0 || lat_edge_for(c, g)) return;
    const long slots = (long)r.N * (r.k + r.p->M);
    int shift = 1;
    while ((1L << shift) < slots) ++shift;
    if (shift >= 32 || ((unsigned long)(g.B - 1) >> (32 - shift)) != 0) return;
    ea.ck_list = w.ck_list; ea.ck_bits = w.ck_bits; ea.ck_off = w.ck_off; ea.ck_shift = shift;
    g.ck_list = w.ck_list; g.ck_n = w.ck_off; g.ck_shift = shift;
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
        g.n_oo = r.ell_full && c->opt.edge_order ? w.n_oo : nullptr;
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
        ea.n_oo = r.c->opt.edge_order ? w.n_oo : nullptr; ea.lds_words = r.c->opt.ell_lds_words;
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
    const RollCall::BaseGraph& b = r.bg;
    HIPCHK(c, launch_share_prep(r.d_state0, p->N_o, r.n_his, b.node_in, b.feat, b.group, b.mask, b.tool, st));
    EdgeArgs be{};
    be.pos = r.d_state0; be.pos_bstride = (long)p->N_o * 3; be.mask = b.mask; be.tool = b.tool; be.thr = p->adj_thresh;
    be.B = 1; be.N = p->N_o; be.topk = p->topk; be.cta = 0; be.edge_cap = base_cap; be.slices = r.base_slices;
    be.ell_full = 1; be.ell = b.send; be.ell_stride = r.kb; be.ell_bstride = base_cap; be.deg = b.deg;
    be.slice_tot = b.slice_tot; be.cta_flag = b.cta; be.recv = b.recv; be.send = b.send; be.n_edges = b.n_edges;
    be.ns_edge = b.ns; be.n_ns = b.n_ns; be.max_nR = 0x7fffffff; be.block_min_rows = c->opt.edge_block_min;
    HIPCHK(c, launch_edge_build(be, st, prof_mark, c));
    GraphBufs gb{};
    gb.node_in = b.node_in; gb.feat12 = b.feat; gb.group = b.group; gb.C = b.C; gb.recv = b.recv; gb.send = b.send;
    gb.n_edges = b.n_edges; gb.ns_edge = b.ns; gb.n_ns = b.n_ns; gb.B = 1; gb.N = p->N_o; gb.n_p = p->N_o; gb.n_inst = 1;
    gb.edge_cap = base_cap; gb.c_cap = base_cap; gb.n_his = r.n_his; gb.wb3 = c->precision == 1 ? c->d_wb3 : nullptr;
    gb.diag = c->diag; gb.zero_skip = c->opt.zero_skip && c->w_finite; gb.half_step = gb.zero_skip && c->opt.half_step;
    int rc = run_edge_chain(c, gb, st);
    if (rc) return rc;
    r.base_send = b.send; r.base_deg = b.deg; r.C_share = b.C; c->d_share_nns = b.n_ns;
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
    EdgeArgs ea = workspace_edge_args(r, w, 1);              // (the parked tool has no object in reach: the cta rule's flag stays 0)
    chunk_list_for(r, w, ea, g);
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
                chunk_list_for(r, w, ea, g);
                if (!(timing_skip & 1) || ai == 1) {
                    HIPCHK(c, launch_edge_build(ea, cs, prof_mark, c));
#ifdef AG_DIAG
                    diag_chunk_dump(c->diag, ea, p->M, cs);  // AG_CHUNK_DUMP (diagnostic build only)
#endif
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
    RollCall r;
    // A caller may be capturing this call into a hipGraph (tools/graph_replay.py): nothing of it may then look at the host side of
    // an event or wait - no polling of the plan's maxima, no prefix sharing (both only save work; results are the same).
    // Workspace, plans and read-back buffers of this call: the slot of the caller's stream (calls on other streams have their own
    // and may still be running; a taken-over slot has been waited for); a captured event could not be waited for outside its graph
    SlotGuard call;
    rc = begin_call(c, stream, call, true);
    if (rc) return rc;
    r.c = c; r.p = p; r.src = &src; r.st = call.st; r.sl = call.sl; r.capturing = call.capturing;
    r.d_state0 = d_state0; r.d_obj_mask = d_obj_mask; r.d_phys_vec = d_phys_vec; r.d_state_seqs = d_state_seqs; r.d_overflow = d_overflow_flag;
    r.dev_plan = src.d_action != nullptr; r.work_only = src.h_work != nullptr; r.R = src.max_repeat;
    r.h_repeat = src.h_repeat; r.d_eef_xz = src.d_eef_xz; r.d_eef_delta = src.d_eef_delta;
    r.N = p->N_o + p->M; r.n_his = c->dims.n_his;            // n_his 4 (every planner task config) or 5 (softbody.yaml:29)
    r.nrep = (size_t)p->B * p->H;
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
    SlotGuard call;
    int rc = begin_call(c, stream, call);
    if (rc) return rc;
    hipStream_t st = call.st; CallSlot* sl = call.sl;
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
    SlotGuard call;
    int rc = begin_call(c, stream, call);
    if (rc) return rc;
    hipStream_t st = call.st; CallSlot* sl = call.sl;
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

}  // extern "C"
