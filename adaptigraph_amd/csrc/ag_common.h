// Shared constants and host-side declarations for the gfx950 kernels (internal, not part of the C-ABI).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace ag {

// ---- model geometry (every shipped config: src/config/dynamics/*.yaml model_config) --------------------
constexpr int NF = 150;        // real feature width of every hidden layer
constexpr int NFP = 160;       // row pitch of every activation buffer (5 MFMA tiles of 32)
constexpr int ONE_F = 150;     // slot that carries the constant 1.0 (bias rides in weight column 150)
constexpr int N_HIS = 4;       // history frames of the ROLLOUT path (every planner task config: n_his 4)
constexpr int IN_DIM = 6;      // [attr_obj, attr_tool, phys, act_x, act_y, act_z]
constexpr int REL_DIM = 17;    // [attr_r(2), attr_s(2), group_diff, (res0,res1,res2,cur)_r - (...)_s]
constexpr int F12 = 3 * N_HIS; // per-particle history feature row
// The forward path (ag_forward) also serves the softbody model variant: n_his = 5, rel_input_dim = 20
// (src/config/dynamics/softbody.yaml:29).  Its feature rows are 15 floats at a 16-float pitch.
constexpr int N_HIS_MAX = 5;
constexpr int F15_PITCH = 16;
inline int feat_pitch(int n_his) { return n_his == 5 ? F15_PITCH : F12; }
constexpr int NODE_IN = 8;     // node input row: 6 features, 1.0, pad

// ---- packed weight geometry ----------------------------------------------------------------------------
// A hidden layer consumes K = 152 input slots = 76 MFMA k-steps (v_mfma_f32_32x32x2_f32 eats 2 k per step:
// lanes 0-31 supply k_a, lanes 32-63 supply k_b).  Step s reads accumulator register (tile t, reg r) of the
// previous layer: t = s/16, r = s%16 (tile 4 only has r < 12), i.e. features 32t + (r&3) + 8(r>>2) + 4h.
// Weights are packed [chunk q = s/4][m-block][lane][4 steps] so one ds_read_b128 feeds 4 MFMAs.
constexpr int KSTEPS = 76;
constexpr int KCH = 19;               // chunks of 4 steps
constexpr int KCH_H0 = 10;            // chunks staged in the first half-phase
constexpr int KCH_H1 = KCH - KCH_H0;  // 9
constexpr int CHUNK_FLOATS_MB5 = 5 * 64 * 4;  // 1280 floats per chunk for a 160-wide output
constexpr int CHUNK_FLOATS_MB1 = 1 * 64 * 4;
constexpr int HALF0_FLOATS = KCH_H0 * CHUNK_FLOATS_MB5;  // 12800
constexpr int HALF1_FLOATS = KCH_H1 * CHUNK_FLOATS_MB5;  // 11520
constexpr int LAYER_FLOATS = HALF0_FLOATS + HALF1_FLOATS;  // 24320
constexpr int EDGE_L1_CHUNKS = 3;     // 18 inputs -> 9 steps, padded to 12
constexpr int NODE_L1_CHUNKS = 1;     // 8 inputs -> 4 steps
constexpr int OUT3_FLOATS = KCH * CHUNK_FLOATS_MB1;  // predictor head (3 outputs, one m-block)

// Offsets (floats) into the packed weight blob, in the order the chains stage them.
struct WeightLayout {
    // edge chain: L1, L2, L3, W1(+b_rp)
    static constexpr int E_L1 = 0;
    static constexpr int E_L2 = E_L1 + EDGE_L1_CHUNKS * CHUNK_FLOATS_MB5;
    static constexpr int E_L3 = E_L2 + LAYER_FLOATS;
    static constexpr int E_W1 = E_L3 + LAYER_FLOATS;
    // node encode chain: L1, L2, L3, Wa(+b_pp), W2, W3
    static constexpr int N_L1 = E_W1 + LAYER_FLOATS;
    static constexpr int N_L2 = N_L1 + NODE_L1_CHUNKS * CHUNK_FLOATS_MB5;
    static constexpr int N_L3 = N_L2 + LAYER_FLOATS;
    static constexpr int N_WA = N_L3 + LAYER_FLOATS;
    static constexpr int N_W2 = N_WA + LAYER_FLOATS;
    static constexpr int N_W3 = N_W2 + LAYER_FLOATS;
    // node propagate chain: Wb, then (W2, W3) again, or the predictor P0, P1, P2
    static constexpr int P_WB = N_W3 + LAYER_FLOATS;
    static constexpr int P_P0 = P_WB + LAYER_FLOATS;
    static constexpr int P_P1 = P_P0 + LAYER_FLOATS;
    static constexpr int P_P2 = P_P1 + LAYER_FLOATS;
    static constexpr int TOTAL = P_P2 + OUT3_FLOATS;
};

// ---- build switches of the fp32 chains (ag_mlp.hip, where they are described: "Zero skip" and "Half-steps").  They sit here because
// the weight packer (ag_optim.hip) has to agree with the chains on them: a chain built with half-steps reads its 160-wide layers
// from a PAIRED image (pack_elem_f32), a chain built without reads the plain one.  -DAG_ZS_EDGE=0|2 / -DAG_ZS_ENC=1 / -DAG_ZS_NODE=0 /
// -DAG_HS_EDGE=0 / -DAG_HS_NODE=0: experiment builds (tools/build_experiment.sh hands the flags to every source file).
#ifndef AG_ZS_EDGE
#define AG_ZS_EDGE 2
#endif
#ifndef AG_ZS_ENC
#define AG_ZS_ENC 0
#endif
#ifndef AG_ZS_NODE
#define AG_ZS_NODE 1
#endif
#ifndef AG_HS_EDGE
#define AG_HS_EDGE 1
#endif
#ifndef AG_HS_NODE
#define AG_HS_NODE 1
#endif
constexpr bool ZS_EDGE = AG_ZS_EDGE != 0, ZS_EDGE_ALL = AG_ZS_EDGE == 2, ZS_ENC = AG_ZS_ENC != 0, ZS_NODE = AG_ZS_NODE != 0;
constexpr bool HS_EDGE = ZS_EDGE && AG_HS_EDGE != 0, HS_NODE = ZS_NODE && AG_HS_NODE != 0;

// ---- kernel families (profiling ids) ------------------------------------------------------------------
enum Family { FAM_EDGE_COUNT = 0, FAM_EDGE_EMIT, FAM_PREP, FAM_NODE_ENC, FAM_EDGE_ENC, FAM_MP, FAM_NODE_PROP,
              FAM_NODE_FINAL, FAM_ROLL_INIT, FAM_ROLL_UPDATE, FAM_COST, FAM_FPS, FAM_ASSEMBLE, FAM_RULE, FAM_SURFACE, FAM_COUNT };

// ---- per-context tuning / A-B switches.  Defaults come from the environment ONCE, at ag_ctx_create (the AG_* name in
// brackets); ag_ctx_set_option changes them per context afterwards.  None of them changes a result (bit-identical paths),
// with ONE exception: device_decode (see there).  Every option has a valid range (kOptions in ag_api.hip): ag_ctx_set_option
// refuses a value outside it, values from the environment are clamped into it.
struct Options {
    int streams = 0;          // [AG_STREAMS]        in-library streams of a rollout: 0 = by batch size, else 1..4
    int chunk = 0;            // [AG_CHUNK]          candidates per launch chunk: 0 = automatic (ag_ctx_set_chunk overrides)
    int latency = -1;         // [AG_LATENCY]        latency-mode chains: -1 by size, 0 never, 1 always
    int ragged = 1;           // [AG_NO_RAGGED]      masked rollouts walk a compact row list
    int ell_graph = 1;        // [AG_NO_ELL_GRAPH]   rollout graphs stay slot-indexed (no CSR emit pass)
    int self_dedupe = 1;      // [AG_NO_SELF_DEDUPE] self-loop edges skip the relation encoder
    int repeat_sort = 1;      // [AG_NO_REPEAT_SORT] candidates of a chunk ordered by action_repeat, finished ones dropped
    int edge_wgs = 256;       // [AG_EDGE_WGS]       edge-builder workgroups aimed at per launch
    int edge_block_min = -1;  // [AG_EDGE_BLOCK_MIN] rows per slice from which the 64-rows-per-wavefront schedule is used (-1: built-in)
    int enc_persist = 0;      // [AG_ENC_PERSIST]    persistent workgroups of k_edge_enc (0 = one per tile)
    int stagger_us = 0;       // [AG_STAGGER_US]     offset between the two workgroups of a CU in the propagate chains
    int zigzag = 1;           // [AG_ZIGZAG]         odd message-passing rounds walk the row tiles backwards: what the previous round
                              //                     read last from HBM is read first, while it is still in the 256-MB Infinity Cache
                              //                     (one stream: k_node_prop 170.5 -> 168.3, final round 83.4 -> 81.4 ms per rollout;
                              //                     four streams: 477.3 -> 475.8 ms - the other chunks' traffic evicts most of it)
    int device_decode = -1;   // [AG_DEVICE_DECODE]  consumed by the Python shim: dynamics() hands GPU-resident actions to
                              //                     ag_rollout_actions (-1: when the task config bounds the repeat, 0 never, 1 always).
                              //                     The one switch that is NOT bit-neutral: cos/sin of the decode are then the device's,
                              //                     so action_seqs agrees with a host decode to ~1e-7, not bit for bit
    int share_prefix = -1;    // [AG_SHARE_PREFIX]   contact-free prefix of look-ahead step 0: candidates whose tool has
                              //                     not touched the object yet follow ONE tool-free base rollout (-1: batches of >= 64
                              //                     candidates and >= 32768 rows, 0 never, 1 whenever possible).  Waits once per call
                              //                     for the contact plan (the GPU is busy with the base rollout meanwhile)
    int stream_min_rows = 32768;  // [AG_STREAM_MIN_ROWS] batches below this many rows (candidates x particles) stay on the caller's stream
                              //                     (r05 A/B, rope x 20 steps: 64 x 301 rows 9.99 ms on one stream / 11.3 on two,
                              //                     128 x 301 rows 14.2 / 13.4: the break-even lies between 19k and 38k rows)
    int pipeline_fork = 0;    // [AG_PIPELINE_FORK]  1: a call forks onto in-library streams even while a call issued on ANOTHER caller
                              //                     stream is still running (0: such a call stays on its stream - the caller is
                              //                     already spreading independent calls over streams, adaptigraph_amd/planner.py)
    int zero_skip = 1;        // [AG_ZERO_SKIP]      exact-fp32 chains: a k-step of a 160-wide layer whose two input features are exactly
                              //                     zero in all 32 rows of a wavefront is branched over (ag_mlp.hip: mma_act).  Exact for
                              //                     finite weights; a weight upload that holds a non-finite value turns it off for that
                              //                     model (0 * inf must stay NaN), and so does a device-side upload, which no host code sees
    int half_step = 1;        // [AG_HALF_STEP]      where zero_skip runs: a k-step with exactly ONE of its two input features zero in all 32
                              //                     rows takes 3 MFMAs instead of 5 - tiles (0,1) and (2,3) one two-block
                              //                     v_mfma_f32_32x32x1_2b_f32 each over the live feature alone (ag_mlp.hip: mma_act).  Same
                              //                     bits: the dropped term is fma(w, 0, acc) with finite w.  No effect where zero_skip is off.
                              //                     0 does not bring back the 5-MFMA step: a step with both features live is two two-block
                              //                     MFMAs per tile pair either way (same bits); only a build with -DAG_HS_EDGE=0
                              //                     -DAG_HS_NODE=0 has the former code
    int edge_order = 2;       // [AG_EDGE_ORDER]     order of the relation encoder's work list (k_ell_index): 0 = slot order (receiver-major),
                              //                     1 = class-major - object-object slots by the signs and the dominant axis of
                              //                     pos_r - pos_s (24 classes), then every slot with a tool at either end, slot order inside
                              //                     a class.  The wavefronts of k_edge_enc then hold like edges and more of their k-steps are
                              //                     all zero (zero_skip).  A C row does not depend on the lane that computes it: same bits.
                              //                     2 = chunk list: ONE list per launch over all its live candidates (k_chunk_*), object-object
                              //                     slots by the transposed slot index (position in row, receiver) - the same slot of every
                              //                     candidate adjacent, in candidate order - then the tool slots by sector and ring of
                              //                     pos_r - pos_s.  fp32 throughput chain on the slot-indexed rollout graphs only; every other
                              //                     launch, and a chunk whose (candidate, slot) does not fit 32 bits, takes order 1
    int ell_lds_words = 0;    // [AG_ELL_LDS_WORDS]  debug: LDS budget of k_ell_index's class bitmaps in 64-bit words (0 = the built-in
                              //                     16384); below 25 bitmaps the classes fall back to (object-object, tool), then to one list
    int share_first = -1;     // [AG_SHARE_FIRST]    first forward of a dynamics() call: the relation encoder runs ONCE over the
                              //                     object-object edges of the start state's tool-free graph and every candidate reads
                              //                     those C rows (-1: batches of 8 candidates or more, 0 never, 1 whenever possible)
};

// ---- launchers (defined in the .hip files) ------------------------------------------------------------
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
// both farthest-point stages of B samples (ag_dataset.hip); pt_off / npts are read at [b * stride]
struct FpsArgs {
    const float* pos; const long long* pt_off; const long long* npts; int stride;
    const int* fps_start; const float* fps_radius; const int* rad_start;
    int B, max_nobj, max_pts;
    int* fps_idx; int* n_obj;
};
hipError_t launch_fps_batch(const FpsArgs& a, hipStream_t st);
size_t fps_max_points();
int fps_max_nobj();
// the same on clouds beyond LDS (k_fps_cloud); ws: fps_cloud_ws_floats(B, max_pts) floats of the call's workspace
hipError_t launch_fps_cloud(const FpsArgs& a, float* ws, hipStream_t st);
size_t fps_cloud_max_points();
size_t fps_cloud_switch_points();
size_t fps_cloud_ws_floats(int B, int max_pts);
// list of non-self-loop edges per candidate (self-loop dedupe, see GraphBufs)
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
hipError_t launch_edge_nonself(const int* recv, const int* send, const int* row_ptr, int B, int N, int edge_cap,
                               int* ns_edge, int* n_ns, const int* live, hipStream_t st);

struct GraphBufs {
    // per-chunk activations; node rows = b*N + i, edge rows = b*c_cap + e, pitch NFP floats
    float* node_in;   // (B*N, NODE_IN)  [attr_obj, attr_tool, phys, act xyz, 1, 0]
    float* feat12;    // (B*N, F12)      [res0, res1, res2, cur] (model.py:156-166)
    float* group;     // (B*N, n_inst)   [p_instance ; 0]        (model.py:264)
    float* eff;       // particle effect, updated in place by the propagate chain
    float* P;
    float* UV[2][2];  // [parity][0 = U, 1 = V]: message-passing round r reads parity (r-1)&1 and writes parity r&1 (the gather
                      // is fused into the chain that rewrites U/V, so a launch must not read what it writes); k_node_enc
                      // writes parity 1, which round 0 reads
    float* C;         // (B*c_cap, NFP)  W1*rel_enc + b_rp
    const int* recv; const int* send; const int* row_ptr; const int* n_edges;
    const int* deg; int ell_stride;   // ell_stride > 0: slot-indexed graph of the rollout fast path (row i owns slots
                                      // [i*ell_stride, i*ell_stride + deg[i]) of send / C), row_ptr unused
    int B, N, n_p, n_inst;
    int edge_cap;     // pitch of recv/send per candidate
    int c_cap;        // pitch of C per candidate, multiple of 256
    // ---- class table (rollout only).  The particle-encoder chain depends only on [attrs, phys, action]: for an object
    // particle that row is the same for every candidate and every rollout step (action is zero for objects,
    // forward_dynamics.py:87-88; phys is broadcast, :151), for a tool particle it changes per look-ahead step.
    // So p_enc / P / U0 / V0 live in a small table: rows [0,N_o) valid object i, [N_o,2N_o) masked-out object i,
    // 2N_o + b*M + m tool m of candidate b.  cls_on = 0: plain per-(b,i) rows (ag_forward).
    int cls_on, N_o, M;
    const uint8_t* vmask;                  // (B,N) validity, selects the object variant
    float* c_node_in;                      // (2N_o + B*M, NODE_IN)
    float* c_eff; float* c_P; float* c_U; float* c_V;   // (2N_o + B*M, NFP)
    // ---- self-loop dedupe (rollout only).  A self-loop edge (i,i) has relation input [attrs_i, attrs_i, 0, 0..0]
    // (group and position differences of a particle with itself are exactly 0), so its C row is one of two
    // constants of the model: c_self[0] for an object particle (attrs 1,0), c_self[1] for a tool (attrs 0,1).
    // ns_edge lists the edges that are NOT self-loops; only those go through the relation encoder.
    const float* c_self;                   // (2, NFP) or null
    long self_row;                         // row of C where c_self[0..1] were copied (k_mp reads them from there)
    const int* ns_edge; const int* n_ns;   // (B,edge_cap), (B,) or null
    const int* n_oo;                       // (B,) or null: class-major list (Options::edge_order), entries [n_oo[b], n_ns[b]) are tool edges
    // chunk list (Options::edge_order 2, EdgeArgs::ck_list) or null: k_edge_enc's tile t takes entries [128 t, 128 t + 128) of ck_list,
    // candidate << ck_shift | slot each; ck_n[0] = entries (device side: the grid stays the host's upper bound), ck_n[1] = object-object ones
    const unsigned* ck_list; const int* ck_n; int ck_shift;
    const float* wb3;                      // bf16x3 weight image: non-null selects the bf16x3 chains (ag_mlp.hip)
    const int* n_guard;                    // ag_forward: guarded per-candidate edge counts (k_edge_guard), else null
    // ---- ragged batches (masked rollouts, forward_dynamics.py:286-309: every candidate has its own number of valid
    // particles).  The propagate chains walk `rowlist` (dense rows b*N + i of the valid object particles and the tools,
    // ascending) instead of all B*N rows.  A masked-out particle takes part in no edge and its node input does not depend
    // on the candidate, so what the reference computes for it (model.py:338: pos + clamp(motion), a constant motion per
    // particle index) is computed ONCE, on the rows of a phantom candidate B (all particles masked out, no tools, no
    // edges) appended to the list; k_roll_update applies it to the masked-out rows of every real candidate.
    const int* rowlist; const int* n_rows; // (B*N + N_o,), device int; null = all rows
    // ---- first forward of a dynamics() call (forward_dynamics.py:25: ONE start state broadcast to all candidates, constant
    // history).  The relation input of an object-object edge is then the same in every candidate, so its C row is too: it is
    // encoded once per call into C_share (row = receiver * share_kb + position in the receiver's row of the tool-free base
    // graph), and the message passing of that forward reads send_pk (EdgeArgs) instead of send: sender in the low 12 bits,
    // position + 1 above them when the slot's C row is the base table's.  Null: every candidate's own C rows (all other forwards).
    const int* send_pk; const float* C_share; int share_kb;
    int n_his;                             // 4 (0 = 4), or 5 on the forward path (feature rows then have pitch F15_PITCH)
    int enc_persist, stagger_us, zigzag;   // Options of the owning context
    int zero_skip;                         // Options::zero_skip, and the loaded weights are known to be finite (ag_ctx::w_finite)
    int half_step;                         // Options::half_step, and zero_skip above is 1
    void* diag;                            // diagnostic build (-DAG_DIAG, ag_diag.hip) only: the context's probe state, else null
};
constexpr int B3_PHASE_BYTES = 2 * 5 * 3 * 64 * 16;   // 30,720
constexpr int B3_PHASES = 58;
inline long cls_rows(int N_o, int M, int B) { return 2L * N_o + (long)B * M; }
// row0/nrows select a slice of the class table when g.cls_on, else all B*N rows are encoded
hipError_t launch_node_enc(const float* wblob, const GraphBufs& g, long row0, long nrows, hipStream_t st);
hipError_t launch_edge_enc(const float* wblob, const GraphBufs& g, hipStream_t st);
// message-passing round `round` (gather fused into the chain); round 0: U/V/eff come from the class table (when g.cls_on)
hipError_t launch_node_prop(const float* wblob, const GraphBufs& g, int round, hipStream_t st);
hipError_t launch_node_final(const float* wblob, const GraphBufs& g, int round, float clamp, float* pred_pos,
                             float* pred_motion, hipStream_t st);

hipError_t launch_edge_guard(const int* n_edges, int B, int edge_cap, int* n_eff, int* overflow, hipStream_t st);
// model-input preparation for ag_forward: state (B,n_his,N,3) etc. -> node_in, feat12
hipError_t launch_prep(const float* state, const float* attrs, const float* action, const float* phys,
                       const GraphBufs& g, hipStream_t st);   // state has g.n_his frames

struct RollBufs {
    float* hist;        // (B, N_HIS, N, 3)
    float* pred;        // (B, N_o, 3) latest prediction
    float* motion;      // (B, N_o, 3) latest raw motion; ragged batches: row block B = the phantom candidate's motion, i.e.
                        // the constant motion of a masked-out particle per particle index
    int ragged;         // masked rollout with a work list (GraphBufs::rowlist)
    float clamp;        // model.py:86 motion clamp, for the masked-out rows
    uint8_t* mask;      // (B,N) valid particles incl. tools
    uint8_t* tool;      // (B,N)
};
struct RollArgs {
    int B, N_o, M, H, li, ai, y_mode, b0;  // B = slots this launch covers; b0 = first candidate of this chunk in the full batch
    int B_slots;                           // slots of the chunk (the phantom candidate of a ragged batch sits behind them)
    float grip; int grip_on; float phys;
    int write_obj_cls;                        // roll_init also writes the object rows of the class table
    const float* phys_vec;                    // null or (N_o,) per-particle physics parameter
    const float* state0; int state0_batched;  // (N_o,3) or (Bfull,N_o,3)
    const uint8_t* obj_mask;                  // (Bfull,N_o) or null
    const float* eef_xz; const float* eef_delta;  // (Bfull,H,M,2), (Bfull,H,M,3)
    const int* repeat;                        // device (Bfull,H)
    const int* live;                          // null, or device int: slots [*live, B) have no forward left (k_roll_update exits)
    const int* cand;                          // null, or (B,) device: slot b of this chunk holds candidate cand[b] of the full
                                              // batch (repeat-sorted launch order); null = candidate b0 + b
    float* state_seqs;                        // (Bfull,H,N_o,3)
    // ---- contact-free prefix (Options::share_prefix; look-ahead step 0 of dynamics() only).  Until a candidate's tool first
    // comes within the radius of an object particle its graph holds no tool edge, so its object particles evolve exactly as
    // in the tool-free BASE rollout of the start state, which is computed once per call: base_states (R+1, N_o, 3) = S_0
    // (the start state) .. S_R, base_y (R+1) = the tool height the reference derives from S_s (forward_dynamics.py:40,163).
    // start (Bfull,) = base step a candidate's own stepping starts from (its first contact is at forward start + 1); k_roll_init
    // then fills the slot's history with S_(start-3) .. S_start and the tool positions replayed up to there, and `repeat`
    // holds the forwards that are LEFT.  Null: every candidate starts from the start state.
    const float* base_states; const float* base_y; const int* start;
    // the base rollout itself: every step's prediction and tool height are recorded (null for ordinary candidates)
    float* all_states; float* all_y;
};
// Contact plan of the prefix sharing (ag_graph.hip: k_contact_plan).  Per candidate: replay the tool keypoints along the base
// rollout (x, z advance by fp32 adds exactly as k_roll_update advances them; y = base_y) and find the first forward whose graph
// would hold a tool-object pair inside the radius - the edge builder's own arithmetic (ag_edges.hip: dist_exact, (dis - thr^2) < 0),
// so "no contact" is exactly "no tool edge in either direction, whatever top-k keeps".
struct ContactPlan {
    const float* base_states; const float* base_y; int R;   // S_0..S_R, base_y[0..R]
    const float* eef_xz; const float* eef_delta; const int* repeat;   // (B,H,M,2), (B,H,M,3), (B,H): look-ahead step 0 is read
    int B, H, N_o, M; float thr;
    int* rep_eff;               // (B,H) out: forwards left per look-ahead step (step 0: repeat - first contact + 1, or 0; others: repeat)
    int* start;                 // (B,) out: base step the candidate starts from (0 when it never touches or touches at once)
    float* state_seqs;          // (B,H,N_o,3): candidates that never touch get S_repeat at look-ahead step 0 here
    // census mode (count != null; base_states = the start state, base_y = null, R = 1): nothing is planned or written except
    // count[0] += candidates with a forward to run whose tool touches at the FIRST forward, count[1] += candidates with a forward
    // to run, count[2] = max repeat of look-ahead step 0; the tool height of the start state is formed here (min object y +
    // gripper offset, forward_dynamics.py:40,80-81)
    int* count; float grip; int grip_on;
    // device-planned calls (ag_rollout_actions): the caller's bound of action_repeat.  A candidate beyond it is treated as the
    // plain device-planned path treats it - never captured (its rows stay zero; the shim marks them NaN) - and later look-ahead
    // steps are stepped at most R_bound times.  Host-planned calls: INT_MAX.
    int R_bound;
};
// count += number of 32-bit words in which a and b differ (bitwise)
hipError_t launch_count_diff(const float* a, const float* b, long n, int* count, hipStream_t st);
hipError_t launch_contact_plan(const ContactPlan& p, hipStream_t st);
// cost kernels (ag_cost.hip)
hipError_t launch_chamfer(const float* x, const float* y, const uint8_t* xm, const uint8_t* ym, int R, int N, int M,
                          int By, float* out, hipStream_t st);
hipError_t launch_state_stats(const float* state, int R, int N, const float* box4, float* out, hipStream_t st);
hipError_t launch_penalty(const float* state_pred, const float* action, const float* state_init, int B, int H, int N,
                          int kind, float ratio, float* out, hipStream_t st);
size_t chamfer_max_points();
// gradient of chamfer toward x: nn (R, N+M) ints and cnt (R,2) floats are workspace
hipError_t launch_chamfer_backward(const float* x, const float* y, const uint8_t* xm, const uint8_t* ym, int R, int N, int M,
                                   int By, const float* gout, int* nn, float* cnt, float* gx, hipStream_t st);
hipError_t launch_reward(const float* error, const float* pen, const float* stats, const float* emax, const double* bbox4, int B,
                         int H, float* out, hipStream_t st);
hipError_t launch_cloth_combine(const float* raw, const float* dmax, long n, float* out, hipStream_t st);

// MPPI sampling / update (ag_mppi.hip)
hipError_t launch_mppi_sample(const float* act_seq, const float* lo, const float* hi, const float* rnd,
                              const float* scale, int S, int H, int mode, float pl, float* out, hipStream_t st);
hipError_t launch_mppi_update(const float* acts, const float* reward, const float* lo, const float* hi, int B, int H,
                              float rw, float pl, float* out, hipStream_t st);
hipError_t launch_mppi_clip(const float* in, const float* lo, const float* hi, float* out, long n, hipStream_t st);

// Device-side launch plan of a rollout whose actions are resident on the GPU (ag_rollout_actions): decode_action + tool
// keypoints (plan_utils.py:11-20, forward_dynamics.py:42-75) and the repeat-aware launch order, without the host ever seeing
// an action.  One wavefront per (launch chunk, look-ahead step): decodes the chunk's actions, orders its candidates by
// action_repeat (descending, stable) and tabulates for every step ai = 0..max_repeat how many of them are still live.
struct RollPlan {
    const float* action;        // (B,H,4) raw [x, z, theta, length]
    float push_length; int M; float tool_off[8];   // pusher_points[k][1] * sim_real_ratio, k < M (entry 0 unused)
    int B, H, Bc, N, max_repeat;
    float* decoded;             // (B,H,4) [x_start, z_start, x_end, z_end]        -> action_seqs
    float* eef_xz; float* eef_delta; int* repeat;  // (B,H,M,2), (B,H,M,3), (B,H)
    int* cand;                  // (H,B) slot -> candidate, per chunk segment
    int* live; int* rows;       // (n_chunks, H, max_repeat + 2): candidates live at step ai, and that times N
    int* sums;                  // (n_chunks, H, 2): sum of min(repeat, max_repeat), sum of live over the steps
    int* maxrep;                // (n_chunks, H): largest min(repeat, max_repeat) of the chunk = steps that find a live slot
    int* flags;                 // caller's flag words: [1] = atomicMax of a repeat beyond max_repeat
    int sort;                   // 0: keep the candidate order (live counts then stay at the chunk size while any candidate is live)
};
hipError_t launch_roll_plan(const RollPlan& p, hipStream_t st);

// work list of a ragged batch (see GraphBufs::rowlist): phantom rows (if any particle is masked out), then the valid rows of
// slots [0,B) in slot order; tab (B+1 ints): entries when only the first n slots are live; cand: slot -> candidate or null;
// also clears the phantom candidate's mask and degree rows
hipError_t launch_build_rowlist(const uint8_t* obj_mask, const int* cand, int b0, int B, int N_o, int M, int* rowlist, int* tab,
                                uint8_t* mask, int* deg, hipStream_t st);
// inputs of the shared first-forward edge encode (GraphBufs::C_share): the object rows of look-ahead step 0, as k_roll_init writes them
hipError_t launch_share_prep(const float* state0, int N_o, int n_his, float* node_in, float* feat, float* group, uint8_t* mask,
                             uint8_t* tool, hipStream_t st);
hipError_t launch_roll_init(const RollArgs& a, const RollBufs& r, const GraphBufs& g, hipStream_t st);
hipError_t launch_roll_update(const RollArgs& a, const RollBufs& r, const GraphBufs& g, hipStream_t st);

// ---- backward pass (ag_train.hip; ag_backward).  Weights are the 22 plain fp32 tensors in ag_ctx_load_weights order,
// (out, in) / (out,) row-major; g[k] the matching gradient accumulators (zeroed by the caller, += per chunk in chunk order).
struct TrainArgs {
    const float* state; const float* attrs; const float* action; const float* phys; const float* group; int n_inst;
    const int* recv; const int* send; const int* row_ptr; const int* n_edges; int edge_cap;
    int B, N, n_p, n_his, pstep; float clamp;
    int Ep;                     // edge rows per graph in the workspace: max n_edges of the call (>= 1)
    const float* w[22]; float* g[22];
    const float* dpos; const float* dmot;   // (B,n_p,3) or null (= zero)
    float* dstate;                          // (B,n_his,N,3) or null (= not wanted)
    float* dphys; float* daction;           // (B,N), (B,N,3) or null (= not wanted): ag_backward_inputs
    bool want_w;                            // false: none of the 22 weight gradients is wanted, their GEMMs are skipped
    bool wide;                              // true: g[k] holds an earlier part's gradients; each reduction adds them in fp64, one rounding
};
size_t train_slab_floats();
size_t train_work_floats(int Bc, int N, int Ep, int n_his, int pstep);
size_t train_work_ints(int Bc, int N, int Ep);
// candidates [b0, b0+nb) of t; wsf / wsi / slab: train_work_floats(nb,...) floats, train_work_ints(nb,...) ints, train_slab_floats()
hipError_t train_backward_chunk(const TrainArgs& t, int b0, int nb, float* wsf, int* wsi, float* slab, hipStream_t st);

// ---- device-resident training step (ag_optim.hip).  The weight images of the forward chains (fp32 MFMA blob of WeightLayout::TOTAL
// floats; bf16x3 image of B3_PHASES phases and latency image, n_his = 4 models only, else null) from the 22 plain tensors in
// ag_ctx_load_weights order: on the host, and by kernels on `st` from device tensors - the same table and element functions.
void pack_weights_host(int rel_dim, const float* const* t, float* blob, uint16_t* b3, float* lat);
hipError_t launch_pack_weights(int rel_dim, const float* const* d_t, float* d_blob, uint16_t* d_b3, float* d_lat, hipStream_t st);
void weight_tensor_sizes(int rel_dim, int* n22);   // floats of each of the 22 tensors
// Adam over the 22 tensors in one launch; scalars pre-rounded to fp32 by the caller from double (ag_adam_step)
struct AdamArgs {
    float* w[22]; const float* g[22]; float* m[22]; float* v[22]; int n[22];
    float wd, one_minus_b1, b2, one_minus_b2, bc2_sqrt, eps, neg_step_size;
    int* status;                // [0] != 0: skip; else [1] += 1
};
hipError_t launch_adam(const AdamArgs& a, hipStream_t st);
// glue of the chained step (train.py:86-124); fut = state_future (B,n_future,n_p,3), part = train_glue_doubles() doubles.
// B_total: rows of the whole optimiser step, the mean's denominator (= B for a one-call step); accumulate: loss[] holds the
// earlier parts' shares and is added to (in fp64, one rounding)
size_t train_glue_doubles();
hipError_t launch_step_loss(const float* pred, const float* fut, int B, int n_p, int n_future, int fi, int B_total, int accumulate,
                            double* part, float* loss, hipStream_t st);
hipError_t launch_next_state(const float* state, const float* pred, const float* eef, const float* act_f, int B, int N, int n_p,
                             int n_his, int n_future, int fi, int rest, float* state_next, float* action_next, hipStream_t st);
hipError_t launch_pred_grad(const float* pred, const float* fut, const float* dnext, int B, int N, int n_p, int n_his, int n_future,
                            int fi, int B_total, float* dpos, hipStream_t st);
hipError_t launch_dstate_carry(float* d, const float* dnext, int B, int N, int n_his, int rest, hipStream_t st);
// the two halves of launch_step_loss / launch_pred_grad that a step with a loss list (ag_train_step_losses) uses on their own:
// the MSE partial sums (same kernel, same launch), and dLoss/dpred with the MSE factor given (mse_scale = weight * 2 / n; 0 with
// no MSE term: dpos is then dnext's rows, or zero)
hipError_t launch_mse_part(const float* pred, const float* fut, int B, int n_p, int n_future, int fi, double* part, hipStream_t st);
hipError_t launch_pred_grad_scaled(const float* pred, const float* fut, const float* dnext, int B, int N, int n_p, int n_his,
                                   int n_future, int fi, float mse_scale, float* dpos, hipStream_t st);

// ---- set losses of the training side (ag_setloss.hip, ag_emd.hip; ag_set_loss, ag_set_loss_backward, ag_train_step_losses):
// Chamfer, Hausdorff and Earth-mover over a batch of cloud pairs, reference src/dynamics/gnn/loss.py.  Kinds as AG_LOSS_* of the
// C-ABI.
constexpr int SET_LOSS_MSE = 0, SET_LOSS_CHAMFER = 1, SET_LOSS_HAUSDORFF = 2, SET_LOSS_EMD = 3;
// AG_LOSS_ROWS, or-ed onto a set kind: every graph's real rows are a prefix, x[b, :nx[b]] and y[b, :ny[b]]; the rows behind the
// counts are never read.  A graph with an empty side is wholly empty.  The kernels are templates on the flag: ROWS = false is the
// code of the plain kinds, the same arithmetic in the same order.
constexpr int SET_LOSS_ROWS = 16;
struct SetRows {                        // both null: the plain kinds
    const int* nx; const int* ny;       // (B) each, as the caller gave them: clamped into [0, N] / [0, M] where they are read
};
// a count clamped into [0, n], before it bounds a loop or addresses anything
__device__ __forceinline__ int clamp_count(int v, int n) { return v < 0 ? 0 : (v > n ? n : v); }
// graph b's real rows (nx, ny) under ROWS: the clamped counts, both 0 when either side is empty
__device__ __forceinline__ void set_rows_of(const SetRows& r, int b, int N, int M, int& nx, int& ny) {
    nx = clamp_count(r.nx[b], N); ny = clamp_count(r.ny[b], M);
    if (nx == 0 || ny == 0) nx = ny = 0;
}
// what the set-loss kernels of both files share: the fp32 distance, every operation rounded on its own
__device__ __forceinline__ float set_dist(float ax, float ay, float az, float bx, float by, float bz) {
    const float dx = __fsub_rn(ax, bx), dy = __fsub_rn(ay, by), dz = __fsub_rn(az, bz);
    return __fsqrt_rn(__fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz)));
}
// g += s * d||x_i - y_j|| / dx_i; zero at zero distance and at no other: a NaN distance gives a NaN row, as torch's norm does
// (the test was !(dist > 0), which a NaN passes: the row of a diverged point came out as 0, the one number that hides it)
__device__ __forceinline__ void set_pull(const float* xi, const float* yj, float s, float (&g)[3]) {
    const float dx = __fsub_rn(xi[0], yj[0]), dy = __fsub_rn(xi[1], yj[1]), dz = __fsub_rn(xi[2], yj[2]);
    const float dist = __fsqrt_rn(__fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz)));
    if (dist == 0.f) return;
    const float q = s / dist;
    g[0] += dx * q; g[1] += dy * q; g[2] += dz * q;
}
__device__ __forceinline__ int clampi(int v, int n) { return v < 0 ? 0 : (v >= n ? n - 1 : v); }   // a table is never trusted as an address
struct SetLossDev {
    const float* x; const float* y;     // graph b's clouds start at x + b * x_bstride (N,3) and y + b * y_bstride (M,3)
    long x_bstride, y_bstride;
    int B, N, M;                        // N + M <= chamfer_max_points()
    int* nn;                            // (B, N+M): nearest y of every x, then nearest x of every y
    double* part; int* pidx;            // set_loss_part_doubles(B) / set_loss_part_ints(B): per-graph partials, see k_set_nn
};
struct SetGradDev {
    const float* gout;                  // device scalar dLoss/dout, or null (= 1)
    float w_chamfer, w_hausdorff;       // the terms' weights (0: term absent)
    float w_emd;                        // the Earth-mover term's weight (k_emd_grad; k_set_grad does not read it)
    int B_total;                        // rows of the whole optimiser step: the means' denominator
    const int* win;                     // the finaliser's Hausdorff winners {b, i, b, j} (read only with w_hausdorff != 0)
    float* gx; int add;                 // (B,N,3): overwritten, or added to (every element has one writer)
};
struct StepLossDev {                    // closes step fi of a chained training step with a loss list
    int n_terms, kind[4]; float weight[4];
    const double* mse_part; int n_mse_part; long mse_n;   // k_mse_part's partial sums and B_total * n_p * 3; null: no MSE term
    const double* set_part; const int* set_idx;           // k_set_nn's partials; null: no Chamfer / Hausdorff term
    const double* emd_part;                               // k_emd_assign's partials (B); null: no Earth-mover term
    int B, n_p, B_total, fi, n_future, accumulate;
    float* loss; float* terms;          // (n_future + 1), (n_future, n_terms)
    int* win;                           // 4 ints of this step
};
size_t set_loss_part_doubles(int B);
size_t set_loss_part_ints(int B);
// rows.nx non-null: the ROWS instance of the kernel; the partials are then per-graph means, the arg-min entries of padding rows 0
hipError_t launch_set_nn(const SetLossDev& a, const SetRows& rows, hipStream_t st);
// kind SET_LOSS_EMD reads emd_part (B doubles of k_emd_assign) and neither a.part, a.pidx nor win; kind may carry SET_LOSS_ROWS
hipError_t launch_set_final(const SetLossDev& a, const double* emd_part, int B_total, int kind, float* out, int* win, hipStream_t st);
hipError_t launch_step_loss_final(const StepLossDev& a, hipStream_t st);   // a.kind[] may carry SET_LOSS_ROWS
hipError_t launch_set_grad(const SetLossDev& a, const SetRows& rows, const SetGradDev& g, hipStream_t st);
// n[b] = the first i < n_p with attrs[b, i, 0] <= 0, or n_p: the live prefix of a padded training batch (attrs (B, N, 2))
hipError_t launch_prefix_rows(const float* attrs, int B, int N, int n_p, int* n, hipStream_t st);

// Earth-mover loss (ag_emd.hip; reference loss.py:25-60): the exact one-to-one matching of min(N, M) pairs per graph.
constexpr int EMD_MAX_MATCH = 512;      // K = min(N, M) served: the serial search steps of one graph are at most K (K + 1) / 2
constexpr int EMD_OK = 0, EMD_NONFINITE = 1, EMD_EXHAUSTED = 2;   // status word of a graph
struct EmdDev {
    const float* x; const float* y;     // as SetLossDev
    long x_bstride, y_bstride;
    int B, N, M;                        // N + M <= emd_max_points(), min(N, M) <= EMD_MAX_MATCH
    int* match;                         // (B, N): the y index matched to x_i, or -1
    int* status;                        // (B): EMD_*
    double* part;                       // (B): sum of the matched fp32 distances in ascending i; NaN for a failed graph
};
size_t emd_max_points();                // N + M that fits the LDS tile with the solver's arrays beside the clouds
hipError_t launch_emd_assign(const EmdDev& a, const SetRows& rows, hipStream_t st);
hipError_t launch_emd_grad(const EmdDev& a, const SetRows& rows, const SetGradDev& g, hipStream_t st);

// ---- device-resident physics-parameter fit (ag_ppm.hip; ag_ppm_grad_step, ag_ppm_adam_step): the glue of the masked rollout
// (forward_dynamics.py:209-399) around the forwards and the backward chunks, and the per-start reduction + Adam.  Rows [0,L) of a
// launch are the live prefix of the batch (rows past it have no forward left); no float atomics, every sum in a fixed order.
struct PpmBufs {
    int B, N_o, M, n_his;                         // N = N_o + M
    const float* state0; const uint8_t* obj_mask; // (B,N_o,3), (B,N_o)
    const float* eef_xz; const float* eef_delta;  // (B,M,2), (B,M,3)
    const float* phys;                            // (B,N_o)
    const int* repeat;                            // (B,) device
    float grip; int grip_on;
    float* ymean; int* cnt;                       // (B,) masked mean y of the latest cloud (fp64 sum, rounded once), valid count
    float* attrs; float* action; float* group; float* physN; uint8_t* mask; uint8_t* tool;   // model inputs, (B,N,...)
};
// masked mean y of pos (L,N_o,3) -> b.ymean, b.cnt
hipError_t launch_ppm_mean_y(const PpmBufs& b, const float* pos, int L, hipStream_t st);
// model inputs of step 1 from the start clouds (needs launch_ppm_mean_y of state0): state1 (B,n_his,N,3) and the constants
hipError_t launch_ppm_init(const PpmBufs& b, float* state1, hipStream_t st);
// after the forward of step s on rows [0,L): seqs[r] = pred[r] where repeat[r] == s; state_next rows [0,Ln) = the shifted
// history with [pred ; tools advanced by delta at the masked mean height of pred] as the last frame (needs launch_ppm_mean_y of pred)
hipError_t launch_ppm_advance(const PpmBufs& b, const float* state, const float* pred, int s, int L, int Ln, float* state_next,
                              float* seqs, hipStream_t st);
// dLoss/dpred of step s, rows [0,L): gseq where repeat == s, + the object rows of dnext's last frame, + the mean-y path (sum of
// dnext's tool rows' y / valid count, on the y of every valid object row); dnext (rows [0,Ln)) = total dLoss/dstate of step s + 1
hipError_t launch_ppm_pred_grad(const PpmBufs& b, const float* gseq, const float* dnext, int s, int L, int Ln, float* dpos,
                                hipStream_t st);
// grad (B,N_o) += the object rows of gphys (L,N)
hipError_t launch_ppm_accum(const float* gphys, int L, int N, int N_o, float* grad, hipStream_t st);
struct PpmAdamArgs {
    const float* err; const float* grad;          // (R,), (R,N_o) of ag_ppm_grad_step
    int K, n, N_o, start_major, hist_cap, apply;  // row of (start k, interaction i) = start_major ? k*n + i : i*K + k
    float* x; double* m; double* v;               // (K,) evaluated parameter (fp32), Adam moments
    float* hist_x; double* hist_e;                // (hist_cap,K)
    double* best;                                 // [best error, its parameter, its start, init_error]
    double* gk;                                   // (K,) the reduced gradient of this call
    float* phys;                                  // (R,N_o)
    double lr, bc1, bc2, lo, hi;
    int* status;
};
hipError_t launch_ppm_adam(const PpmAdamArgs& a, hipStream_t st);

// ---- CMA-ES search (ag_cma.hip; ag_cma_init / ask / tell).  The whole optimiser state is ONE caller-owned buffer of doubles; its
// layout (include/adaptigraph_amd_cma.h documents it for callers) is a header of CMA_HDR words and then the arrays below.  n and popsize
// are read from the header by the kernels themselves: ask and tell take no sizes, so their launch geometry is fixed.
constexpr int CMA_MAX_N = 64, CMA_MIN_POP = 4, CMA_MAX_POP = 32768, CMA_HDR = 24;
constexpr double CMA_MAGIC = 20231105.0;          // header word CMA_H_MAGIC of a buffer ag_cma_init has filled
enum { CMA_H_N = 0, CMA_H_POP, CMA_H_MU, CMA_H_MAXIMIZE, CMA_H_GEN, CMA_H_STATUS, CMA_H_SIGMA, CMA_H_MUEFF, CMA_H_CS, CMA_H_DS,
       CMA_H_CC, CMA_H_C1, CMA_H_CMU, CMA_H_CHIN, CMA_H_PERIOD, CMA_H_BEST_V, CMA_H_BEST_G, CMA_H_MAGIC };
struct CmaLayout {                                // offsets in doubles
    int n, mu, m, C, ps, pc, A, Ai, scale, lo, hi, periodic, best_x, w, total;
    __host__ __device__ CmaLayout(int n_, int mu_) : n(n_), mu(mu_) {
        m = CMA_HDR; C = m + n; ps = C + n * n; pc = ps + n; A = pc + n; Ai = A + n * n; scale = Ai + n * n; lo = scale + n;
        hi = lo + n; periodic = hi + n; best_x = periodic + n; w = best_x + n; total = w + mu;
    }
};
hipError_t launch_cma_ask(const double* state, const double* z, double* y, float* x, hipStream_t st);
hipError_t launch_cma_tell(double* state, const double* y, const float* x, const float* values, int* order, uint8_t* improved,
                           hipStream_t st);

}  // namespace ag
