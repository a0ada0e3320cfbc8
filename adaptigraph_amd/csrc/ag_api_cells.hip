// C-ABI of the cell-list edge builder (include/adaptigraph_amd_cells.h): libadaptigraph_hip_cells.so, a library of its own
// beside the engine's - the engine's export list is closed at ABI version 7 - that works on the engine's contexts: it links
// against libadaptigraph_hip.so and takes its stream slot and its scratch from the context like every engine entry point.
#include "../../include/adaptigraph_amd_cells.h"
#include "ag_cells.h"
#include "ag_host.h"

#include <climits>

using namespace ag;

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
    const size_t nB = (size_t)B, rows = nB * (size_t)N, cells = cells_cap_for(N);
    a.cells_cap = (int)cells; a.zeroed_ints = nB * cells + rows + nB;
    rc = carve_slab(c, *call.sl, [&](Slab& s) {
        a.zeroed = s.take<int>(a.zeroed_ints); a.grid = s.take<char>(nB * cells_grid_bytes());
        a.cell_start = s.take<int>(nB * (cells + 1)); a.cid = s.take<int>(rows); a.slot = s.take<int>(rows);
        a.sorted = s.take<float>(rows * 4); a.ell = s.take<int>(rows * (size_t)std::min(N, topk));
        a.tlist = s.take<int>(rows); a.ntool = s.take<int>(nB);
    });
    if (rc) return rc;
    HIPCHK(c, launch_cells_build(a, call.st));
    return AG_OK;
}
