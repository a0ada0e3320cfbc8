// The glue kernels around the model (ag_graph.hip): model-input preparation, the rollout's state update, its device-side launch
// plan and the contact plan of the prefix sharing.  Internal, not part of the C-ABI.
#pragma once
#include "ag_model.h"

namespace ag {

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

// The same bookkeeping with a candidate's rows spread over the grid, for the rollout over cell-list graphs (ag_rollout_cells: few
// candidates, up to 2^20 rows each).  What RollArgs / RollBufs / GraphBufs give the kernels above, without the prefix sharing, the
// device plan's live count and the ragged phantom, which that driver does not use.
struct RollRows {
    int B, N_o, M, H, li, ai, y_mode, b0;     // B = slots this launch covers; b0 = first candidate of the chunk in the full batch
    int n_his, n_inst;
    float grip; int grip_on; float phys;
    int write_obj_cls;                        // the init kernel also writes the object rows of the class table
    const float* phys_vec;                    // null or (N_o,)
    const float* state0; int state0_batched;  // (N_o,3) or (Bfull,N_o,3)
    const uint8_t* obj_mask;                  // (Bfull,N_o) or null
    const float* eef_xz; const float* eef_delta;  // (Bfull,H,M,2), (Bfull,H,M,3)
    const int* repeat;                        // device (Bfull,H)
    const int* cand;                          // null, or (B,) device: slot -> candidate of the full batch
    float* state_seqs;                        // (Bfull,H,N_o,3)
    float* hist; float* pred; uint8_t* mask; uint8_t* tool;   // RollBufs
    float* node_in; float* feat12; float* group; float* c_node_in;   // GraphBufs
    float* height; int* count;                // (slots,): k_tool_height's output, read by the two row kernels
};
// tool height (+ gripper offset) per slot from the cloud the look-ahead step starts from (and the masked rollout's count of valid
// rows), or - from_pred - from the latest prediction
hipError_t launch_tool_height(const RollRows& a, bool from_pred, hipStream_t st);
hipError_t launch_roll_init_rows(const RollRows& a, hipStream_t st);
hipError_t launch_roll_update_rows(const RollRows& a, hipStream_t st);
// graphs of the cell-list builder above max_nR become empty graphs (n_eff 0, row_ptr zeroed), *overflow = max of their counts
hipError_t launch_cells_guard(const int* n_edges, int B, int N, int max_nR, int* n_eff, int* row_ptr, int* overflow, hipStream_t st);

}  // namespace ag
