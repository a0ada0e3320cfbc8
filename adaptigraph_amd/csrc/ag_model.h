// The model: its geometry, the packed weight images and the forward chains over a graph (ag_mlp.hip, ag_lat.hip; the weight packers
// of ag_optim.hip).  Internal, not part of the C-ABI.
#pragma once
#include "ag_common.h"

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
// ---- launchers (defined in the .hip files) ------------------------------------------------------------
// row0/nrows select a slice of the class table when g.cls_on, else all B*N rows are encoded
hipError_t launch_node_enc(const float* wblob, const GraphBufs& g, long row0, long nrows, hipStream_t st);
hipError_t launch_edge_enc(const float* wblob, const GraphBufs& g, hipStream_t st);
// message-passing round `round` (gather fused into the chain); round 0: U/V/eff come from the class table (when g.cls_on)
hipError_t launch_node_prop(const float* wblob, const GraphBufs& g, int round, hipStream_t st);
hipError_t launch_node_final(const float* wblob, const GraphBufs& g, int round, float clamp, float* pred_pos,
                             float* pred_motion, hipStream_t st);
// the latency-mode chains (ag_lat.hip) over their own weight image of lat_weights_floats() floats
size_t lat_weights_floats();
hipError_t launch_edge_enc_lat(const float* wl, const GraphBufs& g, hipStream_t st);
hipError_t launch_node_enc_lat(const float* wl, const GraphBufs& g, long row0, long nrows, hipStream_t st);
hipError_t launch_node_prop_lat(const float* wl, const GraphBufs& g, int round, bool last, float clamp, float* pred_pos,
                                float* pred_motion, hipStream_t st);

// ---- the weight packers (ag_optim.hip).  The weight images of the forward chains (fp32 MFMA blob of WeightLayout::TOTAL
// floats; bf16x3 image of B3_PHASES phases and latency image, n_his = 4 models only, else null) from the 22 plain tensors in
// ag_ctx_load_weights order: on the host, and by kernels on `st` from device tensors - the same table and element functions.
void pack_weights_host(int rel_dim, const float* const* t, float* blob, uint16_t* b3, float* lat);
hipError_t launch_pack_weights(int rel_dim, const float* const* d_t, float* d_blob, uint16_t* d_b3, float* d_lat, hipStream_t st);
void weight_tensor_sizes(int rel_dim, int* n22);   // floats of each of the 22 tensors

}  // namespace ag
