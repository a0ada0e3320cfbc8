// The cell-list edge builder's launch arguments (ag_cells.hip; entry point in ag_api_cells.hip).  Internal.
#pragma once
#include "ag_common.h"

namespace ag {

// Same rules and outputs as EdgeArgs' plain CSR form, any N up to CELLS_MAX_PARTICLES.
// Squared threshold of graph b: thr2_vec[b], else fp32(t) * fp32(t) with t = thr_vec[b], else t = thr.
constexpr int CELLS_MAX_PARTICLES = 1 << 20, CELLS_MAX_TOPK = 128, CELLS_MAX_GRAPHS = 65535;
struct CellArgs {
    const float* pos; long pos_bstride; const uint8_t* mask; const uint8_t* tool;
    float thr; const float* thr_vec; const float* thr2_vec;
    int B, N, topk, rule; long edge_cap;      // rule: 0 off, 1 batch rule, 2 single-graph rule (EdgeArgs::cta)
    int* recv; int* send; int* row_ptr; int* n_edges;
    // scratch, all of it written before it is read: zeroed = [cell counts (B, cells_cap) | degrees (B, N) | batch flags (B)],
    // cleared by the launch; grid (B x cells_grid_bytes()); cell_start (B, cells_cap + 1); cid, slot, tlist (B, N); sorted
    // (B, N, 4) floats, 16-byte aligned; ell (B, N, min(topk, N)); ntool (B)
    int cells_cap; int* zeroed; size_t zeroed_ints;
    char* grid; int* cell_start; int* cid; int* slot; float* sorted; int* ell; int* tlist; int* ntool;
};
size_t cells_cap_for(int N);                  // cells per graph the builder may use: a power of two >= N within [64, 2^20]
size_t cells_grid_bytes();
hipError_t launch_cells_build(const CellArgs& a, hipStream_t st);

}  // namespace ag
