// C-ABI, graph construction: the edge builder entry points and the tool-attachment rules (see include/adaptigraph_amd.h).
#include "ag_host.h"
#include "ag_rules.h"

using namespace ag;

namespace {
// the graph builder entry points (ag_build_edges, ag_build_edges_single): `a` holds the inputs, outputs and rule; the builder
// scratch (ell, deg, slice_tot, cta_flag) is carved from the slot of stream st
int build_edges(ag_ctx* c, void* stream, EdgeArgs& a) {
    SlotGuard call;
    int rc = begin_call(c, stream, call);
    if (rc) return rc;
    a.slices = pick_slices(c, a.B, a.N);
    const size_t rows = (size_t)a.B * a.N;
    const int ell_stride = edge_ell_stride(a.N, a.topk);
    rc = carve_slab(c, *call.sl, [&](Slab& s) {
        a.ell = s.take<int>(rows * (size_t)std::max(1, ell_stride)); a.deg = s.take<int>(rows);
        a.slice_tot = s.take<int>((size_t)a.B * a.slices); a.cta_flag = s.take<int>(a.B);
    });
    if (rc) return rc;
    if (!a.pos_bstride) a.pos_bstride = (long)a.N * 3;      // (ag_build_edges_graphs reads the graphs out of a larger tensor)
    a.overflow = nullptr; a.max_nR = a.edge_cap; a.zero_on_overflow = 0;
    a.block_min_rows = c->opt.edge_block_min;
    HIPCHK(c, launch_edge_build(a, call.st, prof_mark, c));
    return AG_OK;
}

// What ag_edges_nonfixed_rule_graphs and ag_edges_surface_rule_graphs share (P: the export's public struct; the two name their
// common fields alike): the checks on those fields, under the export's own name, and the launch arguments made of them.  own_ok: p and
// the export's own required pointers are there; own_size / own_value / own_bad: its own size field, reported behind the common ones.
template <typename P>
int rule_graphs_base(ag_ctx* c, const char* me, const P* p, bool own_ok, const char* own_size, int own_value, bool own_bad, RuleGraphsBase& g) {
    if (!own_ok || !p->d_pos || !p->d_mask || !p->d_tool_mask || !p->d_send_in || !p->d_row_ptr_in || !p->d_n_edges_in || !p->d_bounds_pos ||
        !p->d_bounds_first || !p->d_bounds_n || !p->d_recv || !p->d_send || !p->d_row_ptr || !p->d_n_edges_out)
        return fail(c, AG_ERR_INVALID, "%s: null pointer", me);
    if (p->B < 1 || p->N < 1 || p->n_tools < 0 || p->n_tools > p->N || p->base_cap < 1 || p->edge_cap < 1 || p->bounds_points < 1 ||
        p->pad_rows < 0 || (p->d_bounds_idx && p->idx_stride < 1) || own_bad) {
        char own[48] = "";
        if (own_size) snprintf(own, sizeof own, " %s=%d", own_size, own_value);
        return fail(c, AG_ERR_INVALID, "%s: bad sizes B=%d N=%d n_tools=%d base_cap=%d edge_cap=%d bounds_points=%lld pad_rows=%d "
                    "idx_stride=%d%s", me, p->B, p->N, p->n_tools, p->base_cap, p->edge_cap, (long long)p->bounds_points, p->pad_rows,
                    p->idx_stride, own);
    }
    if (p->pos_bstride != 0 && p->pos_bstride < (int64_t)p->N * 3)
        return fail(c, AG_ERR_INVALID, "%s: pos_bstride %lld is below N*3 = %d", me, (long long)p->pos_bstride, p->N * 3);
    if (p->N > 4096) return fail(c, AG_ERR_UNSUPPORTED, "%s: N=%d exceeds 4096", me, p->N);
    if (p->d_send_in == p->d_send || p->d_row_ptr_in == p->d_row_ptr || p->d_n_edges_in == p->d_n_edges_out)
        return fail(c, AG_ERR_INVALID, "%s: input and output arrays must differ", me);
    g.pos = p->d_pos; g.pos_bstride = p->pos_bstride ? (long)p->pos_bstride : (long)p->N * 3; g.mask = p->d_mask; g.tool = p->d_tool_mask;
    g.send_in = p->d_send_in; g.row_ptr_in = p->d_row_ptr_in; g.n_edges_in = p->d_n_edges_in; g.base_cap = p->base_cap;
    g.B = p->B; g.N = p->N; g.n_tools = p->n_tools; g.edge_cap = p->edge_cap;
    g.bnd_pos = p->d_bounds_pos; g.bnd_points = (long)p->bounds_points; g.bnd_first = (const long long*)p->d_bounds_first;
    g.bnd_idx = p->d_bounds_idx; g.idx_stride = p->idx_stride; g.bnd_n = p->d_bounds_n; g.pad_rows = p->pad_rows; g.ratio = (float)p->ratio;
    g.recv = p->d_recv; g.send = p->d_send; g.row_ptr = p->d_row_ptr; g.n_out = p->d_n_edges_out;
    return AG_OK;
}
}  // namespace

extern "C" {

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
    return build_edges(c, stream, a);
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
    return build_edges(c, stream, a);
}

int ag_build_edges_graphs(ag_ctx* c, void* stream, const float* d_pos, int64_t pos_bstride, const uint8_t* d_mask,
                          const uint8_t* d_tool, int32_t B, int32_t N, const float* d_thr2, const float* d_cull, int32_t topk,
                          int32_t cta, int32_t edge_cap, int32_t* d_recv, int32_t* d_send, int32_t* d_row_ptr, int32_t* d_n_edges) {
    if (!c) return AG_ERR_INVALID;
    if (!d_pos || !d_mask || !d_tool || !d_thr2 || !d_cull || !d_recv || !d_send || !d_row_ptr || !d_n_edges || B < 1 || edge_cap < 1)
        return fail(c, AG_ERR_INVALID, "ag_build_edges_graphs: null pointer or empty batch");
    int rc = check_topk(c, N, topk);
    if (rc) return rc;
    if (pos_bstride != 0 && pos_bstride < (int64_t)N * 3)
        return fail(c, AG_ERR_INVALID, "ag_build_edges_graphs: pos_bstride %lld is below N*3 = %d", (long long)pos_bstride, N * 3);
    EdgeArgs a{};
    a.pos = d_pos; a.pos_bstride = (long)pos_bstride; a.mask = d_mask; a.tool = d_tool; a.thr_vec = d_cull; a.thr2_vec = d_thr2;
    a.B = B; a.N = N; a.topk = topk; a.cta = cta ? 2 : 0; a.edge_cap = edge_cap;
    a.recv = d_recv; a.send = d_send; a.row_ptr = d_row_ptr; a.n_edges = d_n_edges;
    return build_edges(c, stream, a);
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
    SlotGuard call;
    int rc = begin_call(c, stream, call);
    if (rc) return rc;
    hipStream_t st = call.st; CallSlot* sl = call.sl;
    const size_t pairs = (size_t)N * (size_t)std::max(1, n_tools);
    RuleArgs a{};
    a.pos = d_pos; a.mask = d_mask; a.tool = d_tool; a.subset = d_subset; a.send_in = d_send_in; a.row_ptr_in = d_row_ptr_in;
    a.N = N; a.n_tools = n_tools; a.edge_cap = edge_cap; a.use_knn = (kNN < 1.0 && kNN > 0.0) ? 1 : 0; a.kNN = kNN;   // graph.py:156
    rc = carve_slab(c, *sl, [&](Slab& s) {
        a.tlist = s.take<int>(std::max(1, n_tools)); a.misc = s.take<int>(16); a.pdis = s.take<float>(pairs);
        a.keep = s.take<uint8_t>(pairs); a.kept = s.take<uint8_t>(pairs);
    });
    if (rc) return rc;
    a.recv = d_recv; a.send = d_send; a.row_ptr = d_row_ptr; a.n_out = d_n_out;
    HIPCHK(c, launch_tool_rule(a, st));
    return AG_OK;
}

int ag_edges_nonfixed_rule_graphs(ag_ctx* c, void* stream, const ag_rule_graphs_args* p) {
    if (!c) return AG_ERR_INVALID;
    RuleGraphsArgs a{};                                   // every table of a graph lives in its workgroup's LDS: no slab carve
    int rc = rule_graphs_base(c, "ag_edges_nonfixed_rule_graphs", p, p && p->d_kNN, nullptr, 0, false, a.g);
    if (rc) return rc;
    if (p->n_tools > RULE_GRAPHS_MAX_TOOLS || (int64_t)p->N * p->n_tools > RULE_GRAPHS_MAX_PAIRS)
        return fail(c, AG_ERR_UNSUPPORTED, "ag_edges_nonfixed_rule_graphs: N=%d x n_tools=%d exceeds the LDS-resident pair tables "
                    "(at most %d tools and N * n_tools <= %d pairs)", p->N, p->n_tools, RULE_GRAPHS_MAX_TOOLS, RULE_GRAPHS_MAX_PAIRS);
    SlotGuard call;
    rc = begin_call(c, stream, call);
    if (rc) return rc;
    a.kNN = p->d_kNN; a.thr_out = p->d_thr;
    Scoped pr(c, FAM_RULE);
    HIPCHK(c, launch_rule_graphs(a, call.st));
    return AG_OK;
}

int ag_edges_surface_rule_graphs(ag_ctx* c, void* stream, const ag_surface_rule_graphs_args* p) {
    if (!c) return AG_ERR_INVALID;
    const int order = p ? p->bounds_order : 0;
    SurfaceGraphsArgs a{};                                // flags, scan and tool list of a graph live in LDS: no slab carve
    int rc = rule_graphs_base(c, "ag_edges_surface_rule_graphs", p, p != nullptr, "bounds_order", order, order != 0 && order != 1, a.g);
    if (rc) return rc;
    if (p->n_tools > RULE_GRAPHS_MAX_TOOLS)
        return fail(c, AG_ERR_UNSUPPORTED, "ag_edges_surface_rule_graphs: n_tools=%d exceeds the LDS-resident tool list (at most %d)",
                    p->n_tools, RULE_GRAPHS_MAX_TOOLS);
    SlotGuard call;
    rc = begin_call(c, stream, call);
    if (rc) return rc;
    a.bounds_order = order; a.one_minus_ratio = (float)(1.0 - p->ratio); a.bounds_out = p->d_bounds; a.planes_out = p->d_planes;
    Scoped pr(c, FAM_SURFACE);
    HIPCHK(c, launch_surface_graphs(a, call.st));
    return AG_OK;
}

}  // extern "C"
