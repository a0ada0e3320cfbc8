// The LDS edge builder's launch arguments (ag_edges.hip).  Internal, not part of the C-ABI.
#pragma once
#include "ag_common.h"

namespace ag {

constexpr int CHUNK_TOOL_KEYS = 32 * 16;   // tool keys of the chunk list (Options::edge_order 2): sectors x rings, ag_edges.hip: chunk_tool_key
struct EdgeArgs {
    const float* pos;           // (B,N,3) with `pos_bstride` floats between candidates
    long pos_bstride;
    const uint8_t* mask;        // (B,N)
    const uint8_t* tool;        // (B,N)
    const float* thr_vec;       // (B,) or null
    float thr;                  // also the chunk-culling radius: must satisfy thr*thr >= the squared threshold in use
    float thr2_override; int use_thr2;   // single-graph builder (graph.py:86,101)
    const float* thr2_vec;      // (B,) or null: B single-graph builds in one launch (ag_build_edges_graphs) - graph b's squared
                                // threshold; thr_vec then holds its culling radius (thr_vec[b]^2 >= thr2_vec[b])
    int B, N, topk, cta, edge_cap, slices;   // cta: 0 off, 1 batch rule (graph.py:276-286), 2 single-graph rule (:119-122)
    int* ell;                   // (B,N,min(topk,N)) scratch: kept senders per row (unused when topk >= N)
    int* deg;                   // (B,N) scratch
    int* slice_tot;             // (B,slices) scratch
    int* cta_flag;              // (B,) scratch: connect_tools_all batch flag
    int* recv; int* send;       // (B,edge_cap)
    int* row_ptr;               // (B,N+1)
    int* n_edges;               // (B,)
    int* overflow;              // single int: max edge count seen above max_nR (atomicMax), may be null
    int max_nR;
    int zero_on_overflow;       // internal rollout use: present an EMPTY graph downstream when E > edge_cap
    // Rollout fast path (top-k active, tool particles behind the object particles): the per-row sender lists ARE the
    // graph.  `ell` then points at the `send` array, a row owns `ell_stride` = topk + M slots (kept senders ascending,
    // then the tool senders of the connect_tools_all rule), a candidate `ell_bstride` = edge_cap slots; slot ids
    // replace CSR edge ids, `deg` replaces row_ptr, and k_edge_emit is skipped.  k_ell_index writes recv per slot,
    // the non-self-loop slot list (ns_edge, n_ns), n_edges, and applies the max_nR rule.
    int ell_full; int ell_stride; long ell_bstride;   // 0 / unset: ell_stride = min(topk,N), ell_bstride = N*ell_stride
    int* ns_edge; int* n_ns;
    // Options::edge_order 1: ns_edge is written class-major (see there) and n_oo[b] = entries in front of the tool class (0 when the
    // classes did not fit the LDS budget `lds_words` and the list stayed in slot order).  n_oo null: slot order, nothing written.
    int* n_oo; int lds_words;
    // Options::edge_order 2 (ck_list non-null; ell_full only): k_ell_index leaves the candidate's two slot bitmaps (object-object,
    // tool) in ck_bits (B, 2, words) instead of a list of its own (n_ns[b] is still the count, n_oo[b] 0), and k_chunk_count / _scan /
    // _fill write ONE list over the live candidates: ck_list[t] = candidate << ck_shift | slot, sorted by key (chunk_key in
    // ag_edges.hip), ck_off[0] = entries, ck_off[1] = entries in front of the first tool key, behind them the scan scratch.
    unsigned long long* ck_bits; int* ck_off; unsigned* ck_list; int ck_shift;
    int block_min_rows;         // Options::edge_block_min (-1: built-in threshold)
    const int* live;            // null, or device int: candidates [*live, B) of this launch have no forward left (device-planned
                                // rollout, RollPlan): their workgroups exit and their graphs are presented as empty
    // First forward of a dynamics() call (GraphBufs::send_pk): k_ell_index looks every object-object slot up in the BASE graph
    // (the start state's graph without the tool: base_send / base_deg, base_stride slots per row) and writes, per slot,
    // send_pk = sender | (position in the base row + 1) << 12 (0 in the upper bits: not in the base row); slots found there are
    // left out of ns_edge - their C row is the base table's.  share_stats (device, 2 x uint64, may be null): += slots served by
    // the base table, += slots this candidate encodes itself.
    int* send_pk; const int* base_send; const int* base_deg; int base_stride; int share_No;
    unsigned long long* share_stats;
    // with the contact-free prefix active only the candidates that start from the start state itself (start == 0) are at "the
    // first forward": share_start (per candidate, or null = all), share_cand (slot -> candidate, or null = share_b0 + slot)
    const int* share_start; const int* share_cand; int share_b0;
};
hipError_t launch_edge_build(const EdgeArgs& a, hipStream_t st, void (*mark)(void*, int, int), void* mark_ctx);
size_t edge_build_max_particles();
int edge_ell_stride(int N, int topk);
// list of non-self-loop edges per candidate (self-loop dedupe, see GraphBufs)
hipError_t launch_edge_nonself(const int* recv, const int* send, const int* row_ptr, int B, int N, int edge_cap,
                               int* ns_edge, int* n_ns, const int* live, hipStream_t st);

}  // namespace ag
