// The tool-attachment rules' launch arguments (ag_rules.hip).  Internal, not part of the C-ABI.
#pragma once
#include "ag_common.h"

namespace ag {

// one tool-attachment rule of the single-graph builder applied to a CSR edge list (ag_rules.hip)
struct RuleArgs {
    const float* pos; const uint8_t* mask; const uint8_t* tool; const uint8_t* subset;
    const int* send_in; const int* row_ptr_in;
    int N, n_tools, edge_cap, use_knn; double kNN;
    int* tlist; int* misc; float* pdis; uint8_t* keep; uint8_t* kept;               // scratch
    int* recv; int* send; int* row_ptr; int* n_out;
};
hipError_t launch_tool_rule(const RuleArgs& a, hipStream_t st);
// the same rules for B graphs in one launch, one workgroup per graph (ag_rules.hip).  What the two launches share:
struct RuleGraphsBase {
    const float* pos; long pos_bstride; const uint8_t* mask; const uint8_t* tool;   // as EdgeArgs
    const int* send_in; const int* row_ptr_in; const int* n_edges_in; int base_cap; // the input graphs, (B, base_cap) / (B, N+1) / (B,)
    int B, N, n_tools, edge_cap;
    // bounds source: graph b's extents come from rows first[b] + (idx ? idx[b, r] : r), r < n[b], of a flat point buffer (indices
    // clamped into it), plus a zero row iff pad_rows > n[b]
    const float* bnd_pos; long bnd_points; const long long* bnd_first; const int* bnd_idx; int idx_stride; const int* bnd_n;
    int pad_rows; float ratio;                                                      // fp32(ratio)
    int* recv; int* send; int* row_ptr; int* n_out;
};
// the non-fixed rule and its kNN filter; the tool list and the (N, n_tools) pair tables of a graph live in LDS, which sets the two limits
constexpr int RULE_GRAPHS_MAX_PAIRS = 8192;
constexpr int RULE_GRAPHS_MAX_TOOLS = 64;
struct RuleGraphsArgs {
    RuleGraphsBase g;
    const double* kNN; float* thr_out;                                              // (B,); (B,) or null
};
hipError_t launch_rule_graphs(const RuleGraphsArgs& a, hipStream_t st);
// the two-closest-planes rule (graph.py:175-221): bounds, plane choice and subset are formed on the device; no pair tables, so only
// N and the tool list are limited
struct SurfaceGraphsArgs {
    RuleGraphsBase g;
    int bounds_order; float one_minus_ratio;                                        // fp32(1 - ratio in double)
    float* bounds_out; int* planes_out;                                             // (B, 6) / (B, 2), may be null
};
hipError_t launch_surface_graphs(const SurfaceGraphsArgs& a, hipStream_t st);

}  // namespace ag
