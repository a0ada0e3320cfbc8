// C-ABI of the cell-list edge builder, of the rollout over its graphs, of the tiled Chamfer cost and of the cell-pruned farthest-point sampler (include/adaptigraph_amd_cells.h): libadaptigraph_hip_cells.so, a library of its own
// beside the engine's - the engine's export list is closed at ABI version 7 - that works on the engine's contexts: it links
// against libadaptigraph_hip.so and takes its stream slot and its scratch from the context like every engine entry point.
#include "../../include/adaptigraph_amd_cells.h"
#include "ag_cells.h"
#include "ag_chamfer_tiled.h"
#include "ag_fps_grid.h"
#include "ag_host.h"

#include <climits>

using namespace ag;

namespace {
// ints of the builder's zeroed region for B graphs [cell counts (B, cells_cap) | degrees (B, N) | batch flags (B)]: what a launch over
// B graphs clears, and - ag_cells.hip lays the three parts out by the launch's own B - what it may touch of the region
size_t cells_zeroed_ints(int B, int N, int cells_cap) { return (size_t)B * cells_cap + (size_t)B * N + (size_t)B; }
// the cell builder's scratch for up to B graphs of N particles (CellArgs says what each part holds); sets cells_cap and zeroed_ints for B
void carve_cells(Slab& s, CellArgs& a, int B, int N, int topk) {
    const size_t nB = (size_t)B, rows = nB * (size_t)N, cells = cells_cap_for(N);
    a.cells_cap = (int)cells; a.zeroed_ints = cells_zeroed_ints(B, N, a.cells_cap);
    a.zeroed = s.take<int>(a.zeroed_ints); a.grid = s.take<char>(nB * cells_grid_bytes());
    a.cell_start = s.take<int>(nB * (cells + 1)); a.cid = s.take<int>(rows); a.slot = s.take<int>(rows);
    a.sorted = s.take<float>(rows * 4); a.ell = s.take<int>(rows * (size_t)std::min(N, topk));
    a.tlist = s.take<int>(rows); a.ntool = s.take<int>(nB);
}
}  // namespace

extern "C" int ag_build_edges_cells(ag_ctx* c, void* stream, const float* d_pos, int64_t pos_bstride, const uint8_t* d_mask,
                                    const uint8_t* d_tool, int32_t B, int32_t N, float thr, const float* d_thr_vec,
                                    const float* d_thr2_vec, int32_t topk, int32_t rule, int64_t edge_cap, int32_t* d_recv,
                                    int32_t* d_send, int32_t* d_row_ptr, int32_t* d_n_edges) {
    if (!c) return AG_ERR_INVALID;
    const char* me = "ag_build_edges_cells";
    if (!d_pos || !d_mask || !d_tool || !d_recv || !d_send || !d_row_ptr || !d_n_edges || B < 1 || edge_cap < 1)
        return fail(c, AG_ERR_INVALID, "%s: null pointer or empty batch", me);
    if (N < 1 || topk < 1) return fail(c, AG_ERR_INVALID, "%s: N and topk must be >= 1", me);
    if (rule < 0 || rule > 2) return fail(c, AG_ERR_INVALID, "%s: rule %d is not 0 (none), 1 (batch) or 2 (single graph)", me, rule);
    if (d_thr_vec && d_thr2_vec) return fail(c, AG_ERR_INVALID, "%s: give the thresholds or their squares, not both", me);
    if (pos_bstride != 0 && pos_bstride < (int64_t)N * 3)
        return fail(c, AG_ERR_INVALID, "%s: pos_bstride %lld is below N*3 = %lld", me, (long long)pos_bstride, (long long)N * 3);
    if (topk > CELLS_MAX_TOPK) return fail(c, AG_ERR_UNSUPPORTED, "%s: topk=%d exceeds %d", me, topk, CELLS_MAX_TOPK);
    if (N > CELLS_MAX_PARTICLES) return fail(c, AG_ERR_UNSUPPORTED, "%s: N=%d exceeds the cell-list builder's limit %d", me, N, CELLS_MAX_PARTICLES);
    if (B > CELLS_MAX_GRAPHS) return fail(c, AG_ERR_UNSUPPORTED, "%s: B=%d exceeds %d graphs per call", me, B, CELLS_MAX_GRAPHS);
    if (edge_cap > (int64_t)INT32_MAX)
        return fail(c, AG_ERR_UNSUPPORTED, "%s: edge_cap=%lld does not fit the int32 edge offsets (at most %d)", me, (long long)edge_cap, INT32_MAX);
    SlotGuard call;
    int rc = begin_call(c, stream, call);
    if (rc) return rc;
    CellArgs a{};
    a.pos = d_pos; a.pos_bstride = (long)pos_bstride; a.mask = d_mask; a.tool = d_tool;
    a.thr = thr; a.thr_vec = d_thr_vec; a.thr2_vec = d_thr2_vec;
    a.B = B; a.N = N; a.topk = topk; a.rule = rule; a.edge_cap = (long)edge_cap;
    a.recv = d_recv; a.send = d_send; a.row_ptr = d_row_ptr; a.n_edges = d_n_edges;
    rc = carve_slab(c, *call.sl, [&](Slab& s) { carve_cells(s, a, B, N, topk); });
    if (rc) return rc;
    HIPCHK(c, launch_cells_build(a, call.st));
    return AG_OK;
}

// ================================================================================================ ag_rollout_cells
// The rollout of ag_rollout_async over graphs of any size the cell-list builder serves.  A plain driver: one workspace, the caller's
// stream, per step cell-list build -> overflow guard -> self-loop pass -> model forward -> tool height -> row update.  None of
// rollout_impl's machinery (device plan, contact-free prefix, shared first forward, slot-indexed graphs, chunk lists, forked
// streams) applies to a handful of candidates of tens of thousands of rows each.
namespace {
constexpr int kMaxTools = 8;       // tool keypoints per candidate the rollout's tool layout serves (ag_rollout_actions: M <= 8)

}  // namespace

extern "C" int ag_rollout_cells(ag_ctx* c, void* stream, const ag_rollout_params* p, const float* d_state0, const uint8_t* d_obj_mask,
                                const float* d_eef_xz, const float* d_eef_delta, const int32_t* h_repeat, const float* d_phys_vec,
                                float* d_state_seqs, int32_t* d_overflow_flag) {
    if (!c) return AG_ERR_INVALID;
    const char* me = "ag_rollout_cells";
    if (!c->have_w) return fail(c, AG_ERR_NO_WEIGHTS, "%s before ag_ctx_load_weights", me);
    if (!p || !d_state0 || !d_eef_xz || !d_eef_delta || !h_repeat || !d_state_seqs || !d_overflow_flag)
        return fail(c, AG_ERR_INVALID, "%s: null pointer", me);
    if (p->B < 1 || p->H < 1 || p->N_o < 1 || p->M < 1 || p->max_nR < 1 || p->topk < 1)
        return fail(c, AG_ERR_INVALID, "%s: bad sizes B=%d H=%d N_o=%d M=%d topk=%d max_nR=%d", me, p->B, p->H, p->N_o, p->M, p->topk, p->max_nR);
    if (p->y_mode != 0 && p->y_mode != 1) return fail(c, AG_ERR_INVALID, "y_mode must be 0 or 1");
    if (p->y_mode == 1 && p->H != 1) return fail(c, AG_ERR_INVALID, "masked rollout has a single look-ahead step");
    // ---- refusals, before anything is enqueued or counted
    const long N_l = (long)p->N_o + p->M;
    if (N_l > CELLS_MAX_PARTICLES) return fail(c, AG_ERR_UNSUPPORTED, "%s: N=%ld exceeds the cell-list builder's limit %d", me, N_l, CELLS_MAX_PARTICLES);
    if (p->topk > CELLS_MAX_TOPK) return fail(c, AG_ERR_UNSUPPORTED, "%s: topk=%d exceeds %d", me, p->topk, CELLS_MAX_TOPK);
    if (p->M > kMaxTools) return fail(c, AG_ERR_UNSUPPORTED, "%s: M=%d tool particles, the tool layout serves at most %d", me, p->M, kMaxTools);
    const int n_his = c->dims.n_his;
    if (c->precision == 1 && n_his != 4) return fail(c, AG_ERR_UNSUPPORTED, "the bf16x3 chains are built for n_his=4");
    const int N = (int)N_l, k = std::min(N, p->topk);
    const long bound = (long)N * (k + p->M);                 // in-degree <= topk + M (radius-AND-top-k, then tool rule)
    const int edge_cap = (int)round_up((size_t)std::min<long>(bound, p->max_nR), 256);
    int rc = check_graph_rows(c, me, N, edge_cap);
    if (rc) return rc;

    SlotGuard call;
    rc = begin_call(c, stream, call);
    if (rc) return rc;
    hipStream_t st = call.st; CallSlot& sl = *call.sl;
    const int Bc = std::min(clamp_chunk_for_offsets(auto_chunk(c, p->B, N), N, edge_cap), CELLS_MAX_GRAPHS);
    const bool dedupe = c->opt.self_dedupe != 0;
    const size_t nrep = (size_t)p->B * p->H;

    // ---- host plan: per chunk and look-ahead step the slots in descending order of their repeat (stable), so that the candidates
    // with a forward left at step ai are a prefix of the slots and every launch of that step covers that prefix only
    rc = grow(c, false, sl.d_repeat, sl.repeat_cap, 2 * nrep, 2 * nrep + (nrep >> 2));
    if (rc) return rc;
    sl.h_repeat.resize(2 * nrep);
    std::copy(h_repeat, h_repeat + nrep, sl.h_repeat.begin());
    const int32_t* rep = sl.h_repeat.data();
    int* h_cand = sl.h_repeat.data() + nrep;                 // [li][slot] -> candidate
    for (int li = 0; li < p->H; ++li)
        for (int b0 = 0; b0 < p->B; b0 += Bc) {
            const int nb = std::min(Bc, p->B - b0);
            int* seg = h_cand + (size_t)li * p->B + b0;
            for (int b = 0; b < nb; ++b) seg[b] = b0 + b;
            std::stable_sort(seg, seg + nb, [&](int x, int y) { return rep[(size_t)x * p->H + li] > rep[(size_t)y * p->H + li]; });
        }

    // ---- one slab: the workspace, the builder's scratch, the guarded counts, tool heights and valid-row counts
    Work w{}; CellArgs ca{}; int* n_eff = nullptr; float* height = nullptr; int* count = nullptr;
    rc = carve_slab(c, sl, [&](Slab& s) {
        carve_work(c, s, w, Bc, N, 1, edge_cap, edge_cap, 1, true, true, true, p->N_o, 0);
        carve_cells(s, ca, Bc, N, p->topk);
        n_eff = s.take<int>(Bc); height = s.take<float>(Bc); count = s.take<int>(Bc);
    });
    if (rc) return rc;
    // nothing below fails without having enqueued: from here on the call counts (a refusal or a failed allocation above leaves the
    // counters of the context's last rollout as they were)
    c->last_slot = (int)(call.sl - c->slots);
    c->d_share_nns = nullptr; c->d_plan_sums = nullptr;
    c->fwd_executed = 0; c->fwd_needed = 0;
    for (size_t i = 0; i < nrep; ++i) c->fwd_needed += std::max(0, rep[i]);
    c->steps_enqueued = 0; c->steps_bound = 0;

    HIPCHK(c, hipMemsetAsync(d_state_seqs, 0, (size_t)p->B * p->H * p->N_o * 3 * 4, st));   // forward_dynamics.py:32
    HIPCHK(c, hipMemcpyAsync(sl.d_repeat, rep, 2 * nrep * 4, hipMemcpyHostToDevice, st));

    ca.pos = w.r.hist + (size_t)(n_his - 1) * N * 3; ca.pos_bstride = (long)n_his * N * 3;   // the newest frame, in place
    ca.mask = w.r.mask; ca.tool = w.r.tool; ca.thr = p->adj_thresh;
    ca.N = N; ca.topk = p->topk; ca.rule = p->connect_tools_all ? 1 : 0; ca.edge_cap = edge_cap;
    ca.recv = w.recv; ca.send = w.send; ca.row_ptr = w.row_ptr; ca.n_edges = w.n_edges;

    bool obj_cls_ready = false;
    for (int b0 = 0; b0 < p->B; b0 += Bc) {
        const int nb = std::min(Bc, p->B - b0);
        GraphBufs g = w.g;
        g.B = nb; g.n_p = p->N_o; g.n_his = n_his; g.n_edges = n_eff;
        g.wb3 = c->precision == 1 ? c->d_wb3 : nullptr;
        if (dedupe) {
            g.c_self = c->d_cself; g.ns_edge = w.ns_edge; g.n_ns = w.n_ns;
            g.self_row = (long)Bc * edge_cap;                // behind the last candidate's C rows of the workspace
            HIPCHK(c, hipMemcpyAsync(w.g.C + (size_t)g.self_row * NFP, c->d_cself, 2 * NFP * 4, hipMemcpyDeviceToDevice, st));
        }
        RollRows ra{};
        ra.b0 = b0; ra.N_o = p->N_o; ra.M = p->M; ra.H = p->H; ra.y_mode = p->y_mode; ra.n_his = n_his; ra.n_inst = 1;
        ra.grip = p->gripper_offset; ra.grip_on = p->gripper_enable; ra.phys = p->physics_param; ra.phys_vec = d_phys_vec;
        ra.state0 = d_state0; ra.state0_batched = p->y_mode == 1; ra.obj_mask = d_obj_mask;
        ra.eef_xz = d_eef_xz; ra.eef_delta = d_eef_delta; ra.repeat = sl.d_repeat; ra.state_seqs = d_state_seqs;
        ra.hist = w.r.hist; ra.pred = w.r.pred; ra.mask = w.r.mask; ra.tool = w.r.tool;
        ra.node_in = w.g.node_in; ra.feat12 = w.g.feat12; ra.group = w.g.group; ra.c_node_in = w.g.c_node_in;
        ra.height = height; ra.count = count;
        for (int li = 0; li < p->H; ++li) {
            const int* seg = h_cand + (size_t)li * p->B + b0;
            const int max_rep = std::max(0, rep[(size_t)seg[0] * p->H + li]);   // descending order
            if (max_rep == 0) continue;                      // nothing of this chunk is stepped in this look-ahead step
            ra.li = li; ra.ai = 0; ra.B = nb; ra.cand = sl.d_repeat + nrep + (size_t)li * p->B + b0;
            ra.write_obj_cls = obj_cls_ready ? 0 : 1;
            { Scoped s(c, FAM_ROLL_INIT);
              HIPCHK(c, launch_tool_height(ra, false, st));
              HIPCHK(c, launch_roll_init_rows(ra, st)); }
            { Scoped s(c, FAM_NODE_ENC);                     // object rows once per call, tool rows per look-ahead step
              const long tool0 = 2L * p->N_o;
              g.B = nb;
              if (!obj_cls_ready) HIPCHK(c, node_enc_for(c, g, 0, tool0 + (long)nb * p->M, st));
              else HIPCHK(c, node_enc_for(c, g, tool0, (long)nb * p->M, st)); }
            obj_cls_ready = true;
            int n_live = nb;
            c->steps_bound += max_rep;
            for (int ai = 1; ai <= max_rep; ++ai) {          // forward_dynamics.py:156
                while (n_live > 0 && rep[(size_t)seg[n_live - 1] * p->H + li] < ai) --n_live;
                ++c->steps_enqueued;
                c->fwd_executed += n_live;
                ca.B = n_live;
                ca.zeroed_ints = cells_zeroed_ints(n_live, N, ca.cells_cap);
                { Scoped s(c, FAM_EDGE_COUNT); HIPCHK(c, launch_cells_build(ca, st)); }
                { Scoped s(c, FAM_EDGE_EMIT);
                  HIPCHK(c, launch_cells_guard(w.n_edges, n_live, N, p->max_nR, n_eff, w.row_ptr, d_overflow_flag, st));
                  if (dedupe) HIPCHK(c, launch_edge_nonself(w.recv, w.send, w.row_ptr, n_live, N, edge_cap, w.ns_edge, w.n_ns, nullptr, st)); }
                g.B = n_live;
                rc = run_model(c, g, w.r.pred, w.r.motion, st);
                if (rc) return rc;
                ra.B = n_live; ra.ai = ai;
                { Scoped s(c, FAM_ROLL_UPDATE);
                  HIPCHK(c, launch_tool_height(ra, true, st));
                  HIPCHK(c, launch_roll_update_rows(ra, st)); }
            }
        }
    }
    return AG_OK;
}

// ================================================================================================ ag_cost_chamfer_tiled
// ag_cost_chamfer / ag_cost_chamfer_backward past the LDS limit of ag_cost.hip (ag_chamfer_tiled.hip).  The per-point tables come from
// the call slot's slab; everything is enqueued on the caller's stream.
namespace {
// the checks both entry points share; *tile becomes the tile the kernels run with
int chamfer_tiled_check(ag_ctx* c, const char* me, bool ptrs_ok, int R, int N, int M, int By, int32_t* tile) {
    if (!ptrs_ok || R < 1 || N < 1 || M < 1 || (By != 1 && By != R))
        return fail(c, AG_ERR_INVALID, "%s: bad arguments R=%d N=%d M=%d By=%d", me, R, N, M, By);
    if (*tile == 0) *tile = CHAMFER_TILED_DEFAULT_TILE;
    if (*tile < 2 || *tile > CHAMFER_TILED_MAX_TILE || (*tile & 1))
        return fail(c, AG_ERR_INVALID, "%s: tile_points=%d is not 0 or an even number in [2, %d]", me, *tile, CHAMFER_TILED_MAX_TILE);
    if (N > CHAMFER_TILED_MAX_POINTS || M > CHAMFER_TILED_MAX_POINTS)
        return fail(c, AG_ERR_UNSUPPORTED, "%s: N=%d, M=%d exceed the tiled kernels' limit of %d points per cloud", me, N, M, CHAMFER_TILED_MAX_POINTS);
    // the tables' entries, and with them the workgroups of every launch (each covers at least one entry), are counted in int32
    if ((long)R * ((long)N + M) > (long)INT32_MAX)
        return fail(c, AG_ERR_UNSUPPORTED, "%s: R*(N+M)=%ld table entries exceed %d", me, (long)R * ((long)N + M), INT32_MAX);
    return AG_OK;
}
}  // namespace

extern "C" int ag_cost_chamfer_tiled(ag_ctx* c, void* stream, const float* d_x, const float* d_y, const uint8_t* d_xmask,
                                     const uint8_t* d_ymask, int32_t R, int32_t N, int32_t M, int32_t By, int32_t tile_points,
                                     float* d_out) {
    if (!c) return AG_ERR_INVALID;
    int rc = chamfer_tiled_check(c, "ag_cost_chamfer_tiled", d_x && d_y && d_out, R, N, M, By, &tile_points);
    if (rc) return rc;
    SlotGuard call;
    rc = begin_call(c, stream, call);
    if (rc) return rc;
    float* d2 = nullptr;
    rc = carve_slab(c, *call.sl, [&](Slab& s) { d2 = s.take<float>((size_t)R * ((size_t)N + M)); });
    if (rc) return rc;
    Scoped p(c, FAM_COST);
    HIPCHK(c, launch_chamfer_tiled(d_x, d_y, d_xmask, d_ymask, R, N, M, By, tile_points, d2, d_out, call.st));
    return AG_OK;
}

extern "C" int ag_cost_chamfer_tiled_backward(ag_ctx* c, void* stream, const float* d_x, const float* d_y, const uint8_t* d_xmask,
                                              const uint8_t* d_ymask, int32_t R, int32_t N, int32_t M, int32_t By, int32_t tile_points,
                                              const float* d_grad_out, float* d_grad_x) {
    if (!c) return AG_ERR_INVALID;
    int rc = chamfer_tiled_check(c, "ag_cost_chamfer_tiled_backward", d_x && d_y && d_grad_out && d_grad_x, R, N, M, By, &tile_points);
    if (rc) return rc;
    SlotGuard call;
    rc = begin_call(c, stream, call);
    if (rc) return rc;
    int* nn = nullptr; float* cnt = nullptr;
    rc = carve_slab(c, *call.sl, [&](Slab& s) { nn = s.take<int>((size_t)R * ((size_t)N + M)); cnt = s.take<float>((size_t)R * 2); });
    if (rc) return rc;
    Scoped p(c, FAM_COST);
    HIPCHK(c, launch_chamfer_tiled_backward(d_x, d_y, d_xmask, d_ymask, R, N, M, By, tile_points, d_grad_out, nn, cnt, d_grad_x, call.st));
    return AG_OK;
}

// ================================================================================================ ag_fps_cloud_grid
// ag_fps_cloud past its 1024 samples (ag_fps_grid.hip): both stages binned into cells and pruned by the cells' boxes, same indices.
namespace {
// one binning pass's scratch for B clouds of up to P points (FpsBinWs says what each part holds)
void carve_fps_bin(Slab& s, FpsBinWs& w, int B, int P, int cells) {
    const size_t nB = (size_t)B, rows = nB * (size_t)P, cc = (size_t)fps_grid_cells_cap(P, cells);
    w.cells_cap = (int)cc; w.zeroed_words = nB * (6 + cc + 1);
    w.zeroed = s.take<unsigned>(w.zeroed_words); w.grid = s.take<char>(nB * fps_grid_bytes());
    w.start = s.take<int>(nB * (cc + 2)); w.cid = s.take<int>(rows); w.slot = s.take<int>(rows);
    w.sorted = s.take<float>(rows * 4); w.md = s.take<float>(rows);
    w.box = s.take<float>(nB * (cc + 1) * 6); w.key0 = s.take<unsigned long long>(nB * (cc + 1));
    w.tab = s.take<char>(nB * fps_grid_tab_bytes((int)cc));
}
}  // namespace

extern "C" int ag_fps_cloud_grid(ag_ctx* c, void* stream, const float* d_pos, const int64_t* d_pt_off, const int64_t* d_npts,
                                 int32_t stride, const int32_t* d_fps_start, const float* d_fps_radius, const int32_t* d_rad_start,
                                 int32_t B, int32_t max_nobj, int32_t max_pts, int32_t cells, int32_t* d_fps_idx, int32_t* d_n_obj) {
    if (!c) return AG_ERR_INVALID;
    const char* me = "ag_fps_cloud_grid";
    if (!d_pos || !d_pt_off || !d_npts || !d_fps_start || !d_fps_radius || !d_rad_start || !d_fps_idx || !d_n_obj)
        return fail(c, AG_ERR_INVALID, "%s: null pointer", me);
    if (B < 1 || stride < 1 || max_nobj < 1 || max_pts < 1)
        return fail(c, AG_ERR_INVALID, "%s: B=%d stride=%d max_nobj=%d max_pts=%d", me, B, stride, max_nobj, max_pts);
    if (cells < 0 || (cells & (cells - 1)) || cells > FPS_GRID_MAX_CELLS)
        return fail(c, AG_ERR_INVALID, "%s: cells=%d is not 0 or a power of two up to %d", me, cells, FPS_GRID_MAX_CELLS);
    if (max_pts > FPS_GRID_MAX_POINTS)
        return fail(c, AG_ERR_UNSUPPORTED, "%s: a cloud of %d points exceeds the limit %d", me, max_pts, FPS_GRID_MAX_POINTS);
    if (max_nobj > FPS_GRID_MAX_NOBJ) return fail(c, AG_ERR_UNSUPPORTED, "%s: max_nobj=%d exceeds %d", me, max_nobj, FPS_GRID_MAX_NOBJ);
    if (B > CELLS_MAX_GRAPHS) return fail(c, AG_ERR_UNSUPPORTED, "%s: B=%d exceeds %d clouds per call", me, B, CELLS_MAX_GRAPHS);
    SlotGuard call;
    int rc = begin_call(c, stream, call);
    if (rc) return rc;
    FpsGridArgs a{};
    a.pos = d_pos; a.pt_off = reinterpret_cast<const long long*>(d_pt_off); a.npts = reinterpret_cast<const long long*>(d_npts);
    a.stride = stride; a.fps_start = d_fps_start; a.fps_radius = d_fps_radius; a.rad_start = d_rad_start;
    a.B = B; a.max_nobj = max_nobj; a.max_pts = max_pts; a.cells = cells; a.fps_idx = d_fps_idx; a.n_obj = d_n_obj;
    rc = carve_slab(c, *call.sl, [&](Slab& s) {
        carve_fps_bin(s, a.w1, B, max_pts, cells);
        carve_fps_bin(s, a.w2, B, max_nobj, cells);
        a.s1pos = s.take<float>((size_t)B * max_nobj * 3); a.s1idx = s.take<int>((size_t)B * max_nobj);
        a.off2 = s.take<long long>(B); a.n2 = s.take<long long>(B);
    });
    if (rc) return rc;
    Scoped p(c, FAM_FPS);
    HIPCHK(c, launch_fps_grid(a, call.st));
    return AG_OK;
}
