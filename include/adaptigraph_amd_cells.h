/* adaptigraph_amd_cells.h - C-ABI of the cell-list edge builder, gfx950 only.  A library of its own,
 * libadaptigraph_hip_cells.so, beside the engine's (adaptigraph_amd.h, whose export list is closed at ABI version 7): it works on
 * the ENGINE'S contexts - an ag_ctx of ag_ctx_create - and links against libadaptigraph_hip.so, so load both (the engine's first,
 * or let the dynamic linker find it next to this one).  Conventions as in adaptigraph_amd.h: 0 on success, a negative AG_ERR_*
 * code otherwise with the message in ag_last_error(ctx); d_* pointers are device memory; `stream` is a hipStream_t. */
#ifndef ADAPTIGRAPH_AMD_CELLS_H
#define ADAPTIGRAPH_AMD_CELLS_H
#include "adaptigraph_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The same graphs as ag_build_edges (rule 1) or ag_build_edges_graphs (rule 2), bit for bit, from a builder whose memory per
 * workgroup does not grow with N and whose work does not grow with N^2: particles are binned into a uniform grid of cells and a
 * receiver is tested against the 27 cells around its own.  It derives its cell edge itself (no culling radius argument).
 *   d_pos        graph b's (N,3) positions start at d_pos + b * pos_bstride floats (0: N*3)
 *   d_mask, d_tool_mask   (B,N) uint8
 *   threshold    squared threshold of graph b = d_thr2_vec[b] if that is non-NULL, else fp32(t)*fp32(t) with t = d_adj_thresh_vec[b]
 *                if that is non-NULL, else t = adj_thresh.  At most one of the two vectors.
 *   rule         connect_tools_all: 0 off, 1 the batch rule (per-graph flag, tool<->tool edges stay: graph.py:276-286),
 *                2 the single-graph rule (unconditional, no tool<->tool edge: graph.py:119-122)
 * A valid particle with a NaN or infinite coordinate is in no radius edge (it fails the reference's test in every pair) and
 * stays valid for the connect_tools_all rules.
 * Outputs as ag_build_edges: d_recv, d_send (B,edge_cap) sorted by (receiver, sender), d_row_ptr (B,N+1), d_n_edges (B,) = the
 * TRUE count even above edge_cap (saturated at INT32_MAX); above edge_cap nothing else - d_row_ptr included - is written for graph b.
 * Limits, refused with AG_ERR_UNSUPPORTED before anything is enqueued: N <= 1,048,576; 1 <= topk <= 128; B <= 65,535;
 * edge_cap <= INT32_MAX.  Any number of tool particles per graph (their list is in global memory).
 * Enqueue only: no host wait inside the call.  The output is a pure function of the inputs. */
int ag_build_edges_cells(ag_ctx* ctx, void* stream, const float* d_pos, int64_t pos_bstride, const uint8_t* d_mask,
                         const uint8_t* d_tool_mask, int32_t B, int32_t N, float adj_thresh, const float* d_adj_thresh_vec,
                         const float* d_thr2_vec, int32_t topk, int32_t rule, int64_t edge_cap, int32_t* d_recv, int32_t* d_send,
                         int32_t* d_row_ptr, int32_t* d_n_edges);

#ifdef __cplusplus
}
#endif
#endif
