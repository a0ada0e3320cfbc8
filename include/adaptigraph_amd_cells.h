/* adaptigraph_amd_cells.h - C-ABI of the cell-list edge builder, of the rollout over its graphs, of the tiled Chamfer cost and of the cell-pruned
 * farthest-point sampler, gfx950 only.  A library of its own,
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

/* ag_rollout_async over graphs of up to 1,048,576 particles: same arguments, same contract (enqueue only, on the caller's stream;
 * d_state_seqs (B,H,N_o,3) is cleared first; h_repeat may die right after the call), and - where both apply, N_o + M <= 4096 - the
 * same bits as ag_rollout_async.  Per rollout step: the cell-list builder above on the newest history frame (rule = connect_tools_all
 * ? 1 : 0), an overflow guard, the self-loop pass (option self_dedupe), the model forward, then the tool height and the history
 * shift with a candidate's rows spread over the grid.  Actions are host-decoded (d_eef_xz, d_eef_delta, h_repeat as ag_rollout_async
 * takes them); every chunk's candidates are stepped in descending order of their repeat, live ones only, so ag_ctx_rollout_counts
 * reports executed == needed.  The engine's options that select kernels (precision, latency, self_dedupe, zero_skip, half_step,
 * chunk) apply; those of ag_rollout_async's own machinery (ell_graph, share_first, share_prefix, streams, device_decode, ragged,
 * repeat_sort, edge_order) are not read.
 *   overflow   a graph with more than max_nR edges is stepped as an EMPTY graph (its count and row_ptr are zeroed before anything
 *              walks them) and *d_overflow_flag = max(*d_overflow_flag, its edge count); the caller zeroes the flag before the call
 *              and raises when it reads a value above max_nR.
 * Refused with AG_ERR_UNSUPPORTED before anything is enqueued: N_o + M > 1,048,576; topk > 128; M > 8; a graph whose rows or edge
 * slots exceed the 32-bit activation offsets; bf16x3 with n_his 5. */
int ag_rollout_cells(ag_ctx* ctx, void* stream, const ag_rollout_params* p, const float* d_state0, const uint8_t* d_obj_mask,
                     const float* d_eef_xz, const float* d_eef_delta, const int32_t* h_repeat, const float* d_phys_vec,
                     float* d_state_seqs, int32_t* d_overflow_flag);

/* The Chamfer cost of the engine's cost entry and its backward, for clouds of up to 1,048,576 points each: the same arguments and
 * conventions (d_x (R,N,3), d_y (By,M,3) with By == 1 or By == R, optional (R,N) / (By,M) uint8 masks that may be NULL, d_out (R,);
 * the backward takes d_grad_out (R,) and writes d_grad_x (R,N,3), exact zeros for masked-out points), and - wherever the engine's
 * entries apply, N + M <= 13,480 - their bits, for every tile size: on finite input for the gradient; for the cost also on
 * non-finite input as far as NaN and +inf go (a row with a NaN or infinite coordinate in a valid point is NaN where the engine's
 * entry gives NaN and +inf where it gives +inf; the other rows keep their bits).  What a masked-out slot holds is never read.
 * A workgroup owns up to 1024 points of one cloud of one row and streams the other cloud through a tile of tile_points points in
 * LDS, so the memory per workgroup does not grow with the clouds and a row is spread over ceil(N/1024) + ceil(M/1024) workgroups.
 *   tile_points  0: the default (2048); else an even number in [2, 4096]; anything else: AG_ERR_INVALID
 * Among equal distances the gradient routes to the lowest index, across tiles as well.  An empty valid set on either side gives
 * what the engine's entries give: the cost of that row is NaN (the mean over no point is 0/0), its gradient is zero.
 * Limits, refused with AG_ERR_UNSUPPORTED before anything is enqueued and with d_out / d_grad_x untouched: N or M above 1,048,576;
 * R * (N + M) above INT32_MAX (the per-point tables, R * (N + M) floats or ints from the call's workspace, are indexed - and the
 * workgroups of every launch counted - in int32).  Enqueue only, on the caller's stream: no host wait inside the call. */
int ag_cost_chamfer_tiled(ag_ctx* ctx, void* stream, const float* d_x, const float* d_y, const uint8_t* d_xmask,
                          const uint8_t* d_ymask, int32_t R, int32_t N, int32_t M, int32_t By, int32_t tile_points, float* d_out);
int ag_cost_chamfer_tiled_backward(ag_ctx* ctx, void* stream, const float* d_x, const float* d_y, const uint8_t* d_xmask,
                                   const uint8_t* d_ymask, int32_t R, int32_t N, int32_t M, int32_t By, int32_t tile_points,
                                   const float* d_grad_out, float* d_grad_x);

/* ag_fps_cloud (adaptigraph_amd.h) past its 1024 samples: the same arguments plus `cells`, the same contract and outputs -
 * d_fps_idx (B,max_nobj) int32 = stage1[stage2] in selection order, then -1; d_n_obj (B,) the counts; start indices clamped, a
 * count above max_pts truncated.  Both stages are exact cell-pruned farthest-point
 * sampling: the points are binned into cells, a cell keeps its tight box and the largest running minimum among its members, and
 * after a new centre only the cells whose box is nearer than that maximum are visited.  The minima are updated with ag_fps_cloud's
 * arithmetic and the argmax is its packed key, so the result is that of the brute-force sweep whatever the partition; a point with
 * a NaN or infinite coordinate lives in a cell of its own kind that is never pruned, and is treated as that sweep treats it.
 * Stage 2's square root is correctly rounded (np.linalg.norm's); ag_fps_cloud's is the native one, good to 1 ulp, so the two entries
 * give the same bits wherever that ulp decides no pick - on every cloud ag_fps_cloud's own tests hold - and this one follows the
 * numpy restatement where they part (lattices with many distances within an ulp of each other or of the radius).
 *   cells   0: the default policy (a power of two with about 64 points per cell, at most 16,384 cells per cloud); else a power of
 *           two up to 16,384 that forces the cell count per cloud (1 = the brute-force sweep through the same code); anything else:
 *           AG_ERR_INVALID
 * Limits, refused with AG_ERR_UNSUPPORTED before anything is allocated or enqueued: max_nobj <= 65,536; max_pts <= 1,048,576;
 * B <= 65,535.  Enqueue only, on the caller's stream; the workspace comes from the call slot's slab. */
int ag_fps_cloud_grid(ag_ctx* ctx, void* stream, const float* d_pos, const int64_t* d_pt_off, const int64_t* d_npts, int32_t stride,
                      const int32_t* d_fps_start, const float* d_fps_radius, const int32_t* d_rad_start, int32_t B, int32_t max_nobj,
                      int32_t max_pts, int32_t cells, int32_t* d_fps_idx, int32_t* d_n_obj);

#ifdef __cplusplus
}
#endif
#endif
