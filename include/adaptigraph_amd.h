/*
 * adaptigraph_amd.h - C-ABI of the MI355X-native GNN-dynamics rollout engine.
 *
 * Drop-in boundary for ONE path of jhyau/AdaptiGraph: the GNN dynamics forward /
 * rollout the MPC planner calls.  The reference has no FFI for this path - the
 * boundary there is a Python callable (src/planning/real_world/planner.py:246,270
 * -> src/planning/forward_dynamics.py:12).  This header is the C boundary placed
 * UNDER that callable; adaptigraph_amd/ (Python, ctypes) keeps the reference's
 * Python signatures on top of it.  INTEGRATION.md shows the binding.
 *
 * Conventions
 *   - Every function returns 0 on success, a negative AG_ERR_* code otherwise;
 *     ag_last_error(ctx) gives the message of the last failure on that ctx.
 *   - Pointers named d_* are DEVICE pointers (e.g. torch tensor.data_ptr()),
 *     h_* are host pointers.  All floating data is fp32, indices int32, masks
 *     uint8 (0/1, the memory layout of a torch.bool tensor).
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream).  All
 *     work is enqueued on it; no function synchronises the stream unless its
 *     comment says so.
 *   - The caller owns every input/output buffer.  The library owns only its
 *     ctx workspace (grown monotonically, freed by ag_ctx_destroy).
 *   - One ctx per (process, device); a ctx is not re-entrant (one host thread at a time).  Calls on ONE stream are ordered by
 *     the stream.  Calls issued on DIFFERENT streams run side by side: the launch plan, the repeat table, the workspace and the
 *     pinned read-back buffers of a call belong to a per-stream "call slot" (up to 8 per ctx; r05).  A ninth stream takes over the
 *     least recently used slot and first waits (GPU side, an event) for that slot's last call.  That is what lets a caller deal
 *     the 40 independent dynamics() calls of the planner's chunk loop (plan.py:241-247) to a few streams
 *     (adaptigraph_amd/planner.py).  Early returns before any work was enqueued (argument errors) record nothing.  A call that is
 *     being captured into a hipGraph neither waits nor records: the caller serialises around a capture.
 *   - WHICH ENTRY POINTS BLOCK THE HOST, and when (everything else only enqueues):
 *       ag_ctx_load_weights, ag_ctx_set_precision     always (host repack + copies)
 *       ag_forward, ag_rollout                        once, at the end: they return the overflow verdict (AG_ERR_MAX_NR)
 *       ag_backward, ag_backward_inputs               at the start (edge counts) and at the end
 *       ag_ctx_load_weights_device, ag_adam_step, ag_train_step, ag_train_step_part, ag_train_step_losses, ag_set_loss, ag_set_loss_backward, ag_ppm_grad_step, ag_ppm_adam_step   NEVER: they only enqueue on the caller's stream; an overflowed
 *           graph is reported in device memory (d_status), which the caller reads when it chooses to
 *       ag_rollout_work                               for its plan (and a base rollout, if none is kept): it returns host numbers
 *       ag_ctx_rollout_counts (after a device-planned call without prefix sharing), ag_ctx_share_counts   wait for the device
 *       ag_rollout_async, ag_rollout_actions          only when the contact-free prefix is in play (option "share_prefix";
 *           y_mode 0, by default batches of >= 64 candidates and >= 32768 rows), and then for SMALL plan kernels at the start
 *           of the call, never for the rollout: (a) a base rollout of this start state is kept in the ctx: ONE wait for census +
 *           state compare + contact plan, enqueued together; (b) the last census of this shape said "not worth it" (e.g. every
 *           push starts on the object): NO wait - a census goes out that a later call reads; (c) otherwise: one wait for the
 *           census, and if it keeps the sharing a second one for the contact plan, the GPU running the base rollout meanwhile.
 *           An event wait on the caller's stream: it also covers whatever the caller enqueued on that stream before the call.
 *           "share_prefix" 0 keeps both purely asynchronous.
 *     Device memory, pinned memory, events and streams are created when a call slot first sees a shape and kept: a repeated call
 *     of the same shape on the same stream allocates nothing (ag_ctx_alloc_counts; hipMalloc / hipFree are device-wide syncs).
 *   - No float atomics anywhere: results are bit-reproducible and independent
 *     of how candidates are chunked or sharded across GPUs.
 */
#ifndef ADAPTIGRAPH_AMD_H
#define ADAPTIGRAPH_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AG_OK 0
#define AG_ERR_INVALID -1      /* bad argument (mirrors the reference's asserts, model.py:89,187,222,240,250) */
#define AG_ERR_HIP -2          /* a HIP runtime call failed                                                  */
#define AG_ERR_MAX_NR -3       /* a graph had more edges than max_nR: reference raises Exception("Exceeds max dims"),
                                  src/dynamics/utils.py:63-65 via forward_dynamics.py:127-128,173-174          */
#define AG_ERR_UNSUPPORTED -4  /* configuration outside what the kernels implement                            */
#define AG_ERR_NO_WEIGHTS -5   /* forward/rollout before ag_ctx_load_weights                                   */

#define AG_ABI_VERSION 7
#define AG_NUM_WEIGHT_TENSORS 22

typedef struct ag_ctx ag_ctx;

/* Model dimensions = what DynamicsPredictor.__init__ derives from model_config
 * (src/dynamics/gnn/model.py:78-123).  Every shipped config has nf=150, in_dim=6 (attr 2 + physics 1 + action 3) and
 * rel_dim = 2*attr 2 + group 1 + 3*n_his: 17 with n_his=4 (rope, granular, cloth, ... and every planner task config),
 * 20 with n_his=5 (config/dynamics/softbody.yaml:29).  Both are served by ag_forward and by the rollout driver (dynamics()
 * takes n_his from the task config it is handed, forward_dynamics.py:16); the bf16x3 arithmetic and the latency-mode chains
 * are built for n_his=4 (ag_ctx_set_precision returns AG_ERR_UNSUPPORTED for an n_his=5 model; small n_his=5 launches
 * simply run the throughput kernels). */
typedef struct ag_dims {
    int32_t nf;            /* nf_particle == nf_relation == nf_effect; kernels are built for 150 */
    int32_t n_his;         /* history frames: 4 or 5                                             */
    int32_t pstep;         /* message-passing rounds (3; softbody.yaml uses 4)                   */
    int32_t in_dim;        /* particle-encoder input width, must be 6                            */
    int32_t rel_dim;       /* relation-encoder input width, must be 5 + 3*n_his                  */
    float motion_clamp;    /* model.py:86, 100.0                                                 */
} ag_dims;

/* Pusher/tool description for the rollout driver (forward_dynamics.py:40-81,163-168). */
typedef struct ag_rollout_params {
    int32_t B;             /* candidates                                                          */
    int32_t H;             /* look-ahead steps (n_look_forward); 1 for the masked variant         */
    int32_t N_o;           /* object particles (max_nobj)                                         */
    int32_t M;             /* tool particles (eef_num)                                            */
    int32_t topk;
    int32_t connect_tools_all;
    int32_t max_nR;        /* reference raises when a graph has more edges                        */
    int32_t y_mode;        /* 0: tool y = min object y (dynamics, :40,:163); 1: masked mean (dynamics_masked, :235,:359) */
    float adj_thresh;
    float gripper_offset;  /* fp32(0.01*sim_real_ratio) if gripper_enable else 0 (:80-81,:167-168) */
    int32_t gripper_enable;
    float physics_param;   /* homogeneous physics parameter (forward_dynamics.py:151)             */
} ag_rollout_params;

uint32_t ag_abi_version(void);

/* Create / destroy.  device_id is the HIP ordinal.  Does not touch the GPU beyond hipSetDevice + small mallocs. */
int ag_ctx_create(int32_t device_id, const ag_dims* dims, ag_ctx** out_ctx);
int ag_ctx_destroy(ag_ctx* ctx);
const char* ag_last_error(const ag_ctx* ctx);

/* Upload the 22 state_dict tensors of DynamicsPredictor (model.py:104-123), HOST pointers, torch layout
 * (weight = (out,in) row-major), in this order:
 *   0..5   particle_encoder.model.{0,2,4}.{weight,bias}      (150x6,150 | 150x150,150 | 150x150,150)
 *   6..11  relation_encoder.model.{0,2,4}.{weight,bias}      (150x17,150 | 150x150,150 | 150x150,150)
 *   12,13  particle_propagator.linear.{weight,bias}          (150x300,150)
 *   14,15  relation_propagator.linear.{weight,bias}          (150x450,150)
 *   16..21 non_rigid_predictor.linear_{0,1,2}.{weight,bias}  (150x150,150 | 150x150,150 | 3x150,3)
 * Synchronous (repacks on the host, copies, waits). */
int ag_ctx_load_weights(ag_ctx* ctx, const float* const* h_tensors, int32_t n_tensors);

/* Arithmetic of the MLP chains.  0 (default): exact fp32 on v_mfma_f32_32x32x2_f32.  1: "bf16x3" - every fp32 operand
 * is split exactly into three bf16 pieces and each product is rebuilt from its six leading partial products on the
 * bf16 matrix pipe with fp32 accumulation (error per product ~2^-24, i.e. fp32-grade; ~2.7x the fp32-MFMA rate).
 * Edge construction is unaffected (always exact).  Re-derives the self-loop constant rows; synchronous. */
int ag_ctx_set_precision(ag_ctx* ctx, int32_t mode);

/* Tuning: candidates per launch wave of the rollout (0 = automatic). */
int ag_ctx_set_chunk(ag_ctx* ctx, int32_t candidates_per_chunk);

/* Per-context switches between bit-identical execution paths (A/B measurements, tests) - with ONE exception, "device_decode",
 * which moves the cos / sin of the action decode to the device (see there).  A context takes its defaults
 * from the environment ONCE, at ag_ctx_create (AG_* name in brackets; values outside an option's range are clamped into it);
 * afterwards only these calls change them, so two contexts of one process can differ.  No call of the library reads the
 * environment after ag_ctx_create.
 *   "streams"        [AG_STREAMS]         in-library HIP streams of a rollout: 0 = by batch size (default), 1..4
 *   "chunk"          [AG_CHUNK]           candidates per launch chunk, 0 = automatic (ag_ctx_set_chunk takes precedence)
 *   "latency"        [AG_LATENCY]         latency-mode chains: -1 by launch size (default), 0 never, 1 always
 *   "ragged"         [AG_NO_RAGGED=1 -> 0]      masked rollouts walk a compact row list (default 1)
 *   "ell_graph"      [AG_NO_ELL_GRAPH=1 -> 0]   rollout graphs stay slot-indexed, no CSR emit pass (default 1)
 *   "self_dedupe"    [AG_NO_SELF_DEDUPE=1 -> 0] self-loop edges skip the relation encoder (default 1)
 *   "repeat_sort"    [AG_NO_REPEAT_SORT=1 -> 0] repeat-aware launch order of ag_rollout (default 1, see there)
 *   "edge_wgs"       [AG_EDGE_WGS]        workgroups the edge builder aims at per launch (default 256)
 *   "edge_block_min" [AG_EDGE_BLOCK_MIN]  rows per slice from which the 64-rows-per-wavefront schedule is used (-1 = built-in 256)
 *   "enc_persist"    [AG_ENC_PERSIST]     persistent workgroups of k_edge_enc (default 0 = one workgroup per tile)
 *   "stagger_us"     [AG_STAGGER_US]      start offset between the two workgroups of a CU in the propagate chains (default 0)
 *   "zigzag"         [AG_ZIGZAG]          odd message-passing rounds walk the row tiles backwards (default 1; Infinity-Cache reuse of
 *                                         the C rows the previous round read last)
 *   "device_decode"  [AG_DEVICE_DECODE]   consumed by the Python shim: dynamics() with GPU-resident actions goes through
 *                                         ag_rollout_actions: -1 when task_config bounds the repeat (default), 0 never, 1 always.
 *                                         NOT bit-neutral: the decode's cos / sin are then the device's, 'action_seqs' agrees
 *                                         with a host decode to ~1e-7 (and a rollout can part from the host-decoded one at a
 *                                         near-tie of the edge selection).  No reference fixture pins GPU-evaluated trig:
 *                                         parity unpinned for that decode; the goldens are compared on the host-decode path
 *   "share_first"    [AG_SHARE_FIRST]     first forward of an ag_rollout* call with y_mode 0 (one start state broadcast to all
 *                                         candidates, forward_dynamics.py:25): the relation encoder runs once over the
 *                                         object-object edges of the start state's tool-free graph, every candidate reads those
 *                                         C rows; -1 = batches of >= 8 candidates (default), 0 never, 1 whenever possible
 *   "share_prefix"   [AG_SHARE_PREFIX]    contact-free prefix of look-ahead step 0 (y_mode 0): a candidate whose tool has not yet come
 *                                         within adj_thresh of an object particle has no tool edge (graph.py:253-286), so its
 *                                         object particles evolve exactly like the start state without a tool.  That base rollout runs
 *                                         once per call; every candidate is stepped only from its first contact on and one that never
 *                                         touches takes the base state of its last step (same bits as stepping it).  -1 = batches of
 *                                         >= 64 candidates and >= 32768 particle rows of which at most half touch at the first forward
 *                                         (a census: one more tiny kernel and wait) (default), 0 never, 1 whenever possible.  The call
 *                                         WAITS once for the contact plan (the GPU is running the base rollout meanwhile), so
 *                                         ag_rollout_async / ag_rollout_actions are then not purely asynchronous
 *   "stream_min_rows" [AG_STREAM_MIN_ROWS] batches below this many rows (candidates x particles) stay on the caller's stream
 *                                         (default 32768: small batches are dispatch-bound, a second stream only doubles the launches)
 *   "pipeline_fork"  [AG_PIPELINE_FORK]   0 (default): a call that starts while a call issued on ANOTHER caller stream is still running
 *                                         does not fork onto in-library streams (the caller is already spreading independent calls
 *                                         over streams); 1: it forks as usual
 *   "zero_skip"      [AG_ZERO_SKIP]       1 (default): the exact-fp32 chains branch over a k-step of a 160-wide layer whose two input
 *                                         features are exactly zero in all 32 rows of a wavefront (ReLU outputs that are off over a
 *                                         local patch).  Same results for finite weights; ag_ctx_load_weights turns it off for a
 *                                         model that holds an inf or NaN weight, ag_ctx_load_weights_device / ag_adam_step always
 *                                         (no host code sees those values).  ag_ctx_get_option "zero_skip_active" (read-only) = 1
 *                                         when the option is on and the guard has not turned it off
 *   "half_step"      [AG_HALF_STEP]       1 (default): where "zero_skip" is active, a k-step with exactly one of its two input features
 *                                         zero in all 32 rows of a wavefront issues 3 MFMAs instead of 5 (two two-block
 *                                         v_mfma_f32_32x32x1_2b_f32 over the live feature, one ordinary MFMA).  Same bits; no effect
 *                                         where "zero_skip_active" is 0.  0 does not restore the 5-MFMA step: a step with
 *                                         both features live stays two two-block MFMAs per tile pair (same bits); only a build
 *                                         with -DAG_HS_EDGE=0 -DAG_HS_NODE=0 has the former code
 *   "edge_order"     [AG_EDGE_ORDER]      order of the relation encoder's work list on the rollout's slot-indexed graphs: 0 = slot
 *                                         order (receiver-major); 1 = class-major: the object-object slots by the sign bits
 *                                         and the dominant axis of pos_r - pos_s at the current frame (24 classes), then every slot
 *                                         with a tool particle at either end, slot order inside a class.  Wavefronts of the relation
 *                                         encoder then hold like edges, more of their k-steps are all zero, and with "zero_skip" the
 *                                         fp32 relation-encoder chain branches over them (in every tile, also with order 0).
 *                                         2 (default) = chunk list: one list per launch over all its live candidates - the
 *                                         object-object slots by the transposed slot index (position in row, receiver), the same
 *                                         slot of every candidate adjacent and in candidate order, then the tool slots by sector
 *                                         (32, x-z plane) and ring (16, |pos_r - pos_s| in adjacency thresholds).  The candidates of
 *                                         a chunk stay close to one start state, so a wavefront's 32 rows are alike.  It serves the
 *                                         fp32 throughput chain on the slot-indexed graphs; bf16x3, the latency-mode chains, the
 *                                         shared base graph and a chunk whose (candidate, slot) does not fit 32 bits take order 1.
 *                                         A C row is stored by slot and does not depend on the lane that computes it: same bits
 *   "ell_lds_words"  [AG_ELL_LDS_WORDS]   debug: LDS budget, in 64-bit words, of the class bitmaps of "edge_order" 1 (0 = the
 *                                         built-in 16384 = 128 KB).  A graph whose 25 bitmaps do not fit takes two classes
 *                                         (object-object, tool), then the one list of slot order; tests reach the fallbacks with it
 * Unknown names and values outside an option's range return AG_ERR_INVALID (ranges: edge_order 0..2, ell_lds_words 0..16384, stream_min_rows 0..INT32_MAX, pipeline_fork 0..1, streams 0..4, chunk 0..2^20, latency -1..1,
 * the 0/1 switches 0..1, edge_wgs 1..65536, edge_block_min -1..INT32_MAX, enc_persist 0..2^20, stagger_us 0..1000,
 * device_decode -1..1, share_first -1..1, share_prefix -1..1). */
int ag_ctx_set_option(ag_ctx* ctx, const char* name, int32_t value);
int ag_ctx_get_option(ag_ctx* ctx, const char* name, int32_t* out_value);

/* Candidate-forwards of the LAST ag_rollout / ag_rollout_async / ag_rollout_actions call on this context: executed (sum over
 * launches of the candidates each model forward was launched over) and needed (sum of action_repeat over the batch).  With
 * the repeat-aware launch order (default; masked batches included) the two are equal; with "repeat_sort" 0 every candidate of
 * a launch chunk is stepped to the chunk's maximum, as the reference steps the whole batch to the batch maximum
 * (forward_dynamics.py:156-161); with "share_prefix" active executed (which then includes the base rollout's forwards) is
 * SMALLER than needed: the forwards before a candidate's first contact are the base rollout's.  After an ag_rollout_actions
 * call without prefix sharing the call waits for the device (the sums live there). */
int ag_ctx_rollout_counts(ag_ctx* ctx, int64_t* out_executed, int64_t* out_needed);

/* Model forwards (per launch chunk and look-ahead step) ENQUEUED by the LAST ag_rollout / ag_rollout_async /
 * ag_rollout_actions call: out2[0] = enqueued, out2[1] = what the loop bounds alone give (host plan: the chunk maxima, equal
 * to out2[0]; device plan: max_repeat per chunk and look-ahead step).  On the device-planned path the chunk maxima come back
 * to the host asynchronously (pinned memory + event, never waited for); once they have landed the enqueue loop stops a
 * look-ahead step at the chunk's own maximum, so out2[0] <= out2[1].  Host bookkeeping only: no device access. */
int ag_ctx_launch_counts(ag_ctx* ctx, int64_t* out2);

/* out[0] = number of device / pinned allocations and frees, event and stream creations this context has made so far.  A
 * steady-state call - same shape, same stream as an earlier one - makes none (tests/test_gpu_share_prefix.py).  Host
 * bookkeeping only. */
int ag_ctx_alloc_counts(ag_ctx* ctx, int64_t* out1);

/* Shared first forward ("share_first") of the LAST ag_rollout / ag_rollout_async / ag_rollout_actions call on this context:
 * out3[0] = edges the once-per-call base encode ran over (0 when the call did not share), out3[1] = edge slots of all
 * candidates that took their C row from the shared table, out3[2] = edge slots the candidates encoded themselves at that
 * forward (edges with a tool at either end).  Without sharing the relation encoder would have run over out3[1] + out3[2]
 * edges.  Waits for the device. */
int ag_ctx_share_counts(ag_ctx* ctx, int64_t* out3);

/* Replaces construct_edges_from_states_batch (src/dynamics/dataset/graph.py:233-298).
 *   d_pos (B,N,3); d_mask,d_tool_mask (B,N) uint8; adj_thresh scalar, or d_adj_thresh_vec (B,) if non-NULL.
 * Outputs, per batch element b, in the reference's nonzero order (sorted by receiver, then sender):
 *   d_recv,d_send (B,edge_cap) int32 (entries past n_edges[b] are left untouched),
 *   d_row_ptr (B,N+1) int32 CSR offsets by receiver, d_n_edges (B,) int32 = TRUE edge count even when > edge_cap
 *   (then nothing is written for that element).  The caller compares n_edges with its max_nR (pad_torch semantics). */
int ag_build_edges(ag_ctx* ctx, void* stream, const float* d_pos, const uint8_t* d_mask, const uint8_t* d_tool_mask,
                   int32_t B, int32_t N, float adj_thresh, const float* d_adj_thresh_vec, int32_t topk,
                   int32_t connect_tools_all, int32_t edge_cap, int32_t* d_recv, int32_t* d_send,
                   int32_t* d_row_ptr, int32_t* d_n_edges);

/* Replaces the default-argument path of construct_edges_from_states (src/dynamics/dataset/graph.py:68-231, single
 * graph; the dataset / eval-rollout builder).  Differences from the batch builder that are reproduced: the squared
 * threshold is formed in double precision and then rounded (h: thr2 = (float)((double)adj*adj), graph.py:86,101 - one ulp
 * away from the batch builder's fp32 square for e.g. 0.4); connect_tools_all is unconditional and leaves no
 * tool<->tool edge (graph.py:119-122).  cull_radius: any float with cull_radius^2 >= thr2 (e.g. nextafter(adj)).
 * The tool-surface / kNN / non-fixed-particle options of that function (max_y, kNN, ...) are applied afterwards, one
 * rule at a time, with ag_edges_apply_tool_rule. */
int ag_build_edges_single(ag_ctx* ctx, void* stream, const float* d_pos, const uint8_t* d_mask, const uint8_t* d_tool_mask,
                          int32_t N, float thr2, float cull_radius, int32_t topk, int32_t connect_tools_all,
                          int32_t edge_cap, int32_t* d_recv, int32_t* d_send, int32_t* d_row_ptr, int32_t* d_n_edges);

/* One tool-attachment rule of construct_edges_from_states applied to an edge list produced by ag_build_edges_single
 * (src/dynamics/dataset/graph.py:144-170 "tool to all non-fixed particles", :208-218 "tool to the closest surfaces").
 * d_subset (N,) uint8 marks the rule's particle subset S (the kernel ANDs it with d_mask); forming S from max_y, the
 * plane bounds etc. is scalar host arithmetic (graph.py:134-143, :190-207) and stays with the caller.  Effect:
 *   edges (tool receiver <- sender in S) are removed; every (receiver in S <- tool) edge is present; if 0 < kNN < 1
 *   only the keepK = (int)(kNN * #pairs) of those pairs with the smallest fp32 distance survive, ranked over the flat
 *   row-major pair list, ties by pair position (graph.py:156-169); no tool<->tool edge remains.
 * n_tools must equal the number of set entries of d_tool_mask (else *d_n_out = -1 and nothing else is written).
 * Outputs like ag_build_edges_single: sorted by (receiver, sender); d_n_out is the TRUE count even when > edge_cap (then
 * d_recv_out/d_send_out are not written).  Input and output arrays must not overlap. */
int ag_edges_apply_tool_rule(ag_ctx* ctx, void* stream, const float* d_pos, const uint8_t* d_mask, const uint8_t* d_tool_mask,
                             int32_t N, int32_t n_tools, const int32_t* d_send_in, const int32_t* d_row_ptr_in,
                             const uint8_t* d_subset, double kNN, int32_t edge_cap, int32_t* d_recv_out, int32_t* d_send_out,
                             int32_t* d_row_ptr_out, int32_t* d_n_out);

/* Replaces DynamicsPredictor.forward (src/dynamics/gnn/model.py:130-342) on index-list graphs.
 *   d_state (B,n_his,N,3) with the ctx's n_his; d_attrs (B,N,2); d_action (B,N,3); d_phys (B,N) physics parameter per particle, zero
 *   for the trailing N-n_p tool particles (model.py:206-207); d_group (B,N,n_inst) = [p_instance ; 0] (model.py:264);
 *   edges as produced by ag_build_edges (must be sorted by receiver; row_ptr consistent).
 * Outputs d_pred_pos, d_pred_motion (B,n_p,3) (model.py:335-338).
 * A graph whose d_n_edges[b] exceeds edge_cap (ag_build_edges reports the true count and writes no indices then) is
 * never walked: the call returns AG_ERR_MAX_NR - the reference raises Exception("Exceeds max dims") at the pad_torch in
 * front of its forward (utils.py:63-65).  Synchronises the stream once at the end to read that flag. */
int ag_forward(ag_ctx* ctx, void* stream, const float* d_state, const float* d_attrs, const float* d_action,
               const float* d_phys, const float* d_group, int32_t n_inst, const int32_t* d_recv, const int32_t* d_send,
               const int32_t* d_row_ptr, const int32_t* d_n_edges, int32_t edge_cap, int32_t B, int32_t N, int32_t n_p,
               float* d_pred_pos, float* d_pred_motion);

/* Backward pass of ag_forward (model.py:130-342 under torch autograd), exact fp32 whatever ag_ctx_set_precision says.
 *   Inputs: those of ag_forward, plus d_w[22]: the 22 fp32 parameter tensors in ag_ctx_load_weights order, plain (out, in) /
 *   (out,) row-major (the gradient is taken with respect to exactly these; the ctx's loaded weights are not used), and
 *   d_grad_pos, d_grad_motion (B,n_p,3): dLoss/dpred_pos, dLoss/dpred_motion, either NULL (= zero).
 *   Outputs (each NULL = not wanted): d_grad_state (B,n_his,N,3) dLoss/dstate; d_grad_w[22] matching d_w
 *   (when d_grad_w is NULL or all of its entries are, the weight-gradient contractions are skipped).  Gradients reach
 *   state and the parameters only; attrs, action, phys and group are data.  Edges beyond d_n_edges[b] and particles without
 *   edges and beyond n_p get zero gradient.  Deterministic: no float atomics, fixed reduction order (two calls on the same
 *   inputs give the same bits).
 * Reads d_n_edges on the host first (one stream synchronisation) and returns AG_ERR_MAX_NR ("Exceeds max dims"), with nothing
 * enqueued, when a graph has more than edge_cap edges.  Synchronises the stream once more at the end. */
int ag_backward(ag_ctx* ctx, void* stream, const float* d_state, const float* d_attrs, const float* d_action,
                const float* d_phys, const float* d_group, int32_t n_inst, const int32_t* d_recv, const int32_t* d_send,
                const int32_t* d_row_ptr, const int32_t* d_n_edges, int32_t edge_cap, int32_t B, int32_t N, int32_t n_p,
                const float* const* d_w, const float* d_grad_pos, const float* d_grad_motion, float* d_grad_state,
                float* const* d_grad_w);

/* ag_backward plus the data gradients of the particle encoder's input (model.py:206-223): d_grad_phys (B,N) dLoss/dphys (zero
 * for the tool rows n >= n_p, which the forward pads with a constant zero) and d_grad_action (B,N,3) dLoss/daction, each NULL =
 * not wanted.  One implementation: ag_backward is this call with both NULL, and every other output carries the same bits either
 * way.  Same rules: exact fp32, no float atomics, fixed reduction order; a row's data gradient does not depend on which other
 * rows share the call.  Edges are constants: nothing is differentiated through the graph construction. */
int ag_backward_inputs(ag_ctx* ctx, void* stream, const float* d_state, const float* d_attrs, const float* d_action,
                       const float* d_phys, const float* d_group, int32_t n_inst, const int32_t* d_recv, const int32_t* d_send,
                       const int32_t* d_row_ptr, const int32_t* d_n_edges, int32_t edge_cap, int32_t B, int32_t N, int32_t n_p,
                       const float* const* d_w, const float* d_grad_pos, const float* d_grad_motion, float* d_grad_state,
                       float* const* d_grad_w, float* d_grad_phys, float* d_grad_action);

/* ---- Device-resident training step (reference src/dynamics/train/train.py:86-124).  None of the three waits for the GPU. ---- */

/* ag_ctx_load_weights from 22 plain fp32 DEVICE tensors (same order and layout): every weight image the context keeps - the
 * fp32 MFMA image and, for n_his = 4 models, the bf16x3 and the latency-mode images - is built by kernels on `stream`,
 * bit-identical to the host-packed ones, and the self-loop constant rows are re-derived behind them.  No host copy, no wait
 * (the first call allocates the images it finds missing).  The tensors are read when the kernels run.  The images belong to
 * the context, not to a call slot, and are rewritten in place: while this call (or ag_adam_step, which ends with it) is in flight
 * no other call on this context may be in flight on another stream. */
int ag_ctx_load_weights_device(ag_ctx* ctx, void* stream, const float* const* d_w);

/* One torch.optim.Adam step (single-tensor formula; no amsgrad, no maximize) over the 22 parameter tensors in one launch:
 *   g += weight_decay * w;  m += (g - m) * (1 - beta1);  v = v * beta2 + (1 - beta2) * g * g;
 *   w -= (lr / bc1) * m / (sqrt(v) / sqrt(bc2) + eps),   bc_i = 1 - beta_i^step formed here in double (step >= 1).
 * d_status (int32 x 4, device): when d_status[0] != 0 (ag_train_step found an overflowed graph) nothing is touched; otherwise
 * d_status[1] += 1, the count of applied steps.  Ends by enqueuing ag_ctx_load_weights_device(d_w). */
int ag_adam_step(ag_ctx* ctx, void* stream, float* const* d_w, const float* const* d_grad, float* const* d_exp_avg,
                 float* const* d_exp_avg_sq, int32_t step, double lr, double beta1, double beta2, double eps, double weight_decay,
                 int32_t* d_status);

/* The training loop body (train.py:94-122) as one enqueue-only call: n_future chained forwards (each the kernels and bits of
 * ag_forward on the context's loaded weights), per step the MSE of the prediction against d_state_future[:, fi] (summed in
 * fp64 in a fixed order, rounded once) and the next model input (last frame = d_eef_future[:, fi] with the object rows replaced by
 * the prediction, history shifted by one, frame 0 kept when store_rest_state; action = d_action_future[:, fi]); then, when
 * want_grad, the backward through the chain, last step first.
 *   Inputs: those of ag_backward (d_w[22] = the plain parameters the gradient is taken toward; they must hold the values the
 *   context's weights were loaded from), d_state_future (B,n_future,n_p,3), d_eef_future, d_action_future (B,n_future-1,N,3; may
 *   be NULL when n_future == 1), edge_rows = the caller's bound on the largest d_n_edges[b] (sizes the backward workspace).
 *   Outputs: d_grad_w[22] (overwritten; ignored when want_grad == 0), d_loss (n_future + 1 floats: per-step MSE, then their
 *   sum), d_pred (n_future,B,n_p,3) or NULL, d_status (int32 x 4): [0] receives (atomic max, never cleared here) the edge count of
 *   a graph with more than min(edge_cap, edge_rows) edges - such a graph is walked as an empty one, nothing reads unwritten
 *   indices, and ag_adam_step skips its update; [1] is ag_adam_step's; [2], [3] reserved.
 * Returns AG_OK for an overflowed graph: the caller maps d_status[0] != 0 to AG_ERR_MAX_NR when it reads it.  No float atomics:
 * two calls on the same inputs give the same bits. */
int ag_train_step(ag_ctx* ctx, void* stream, const float* d_state, const float* d_attrs, const float* d_action, const float* d_phys,
                  const float* d_group, int32_t n_inst, const int32_t* d_recv, const int32_t* d_send, const int32_t* d_row_ptr,
                  const int32_t* d_n_edges, int32_t edge_cap, int32_t B, int32_t N, int32_t n_p, const float* const* d_w,
                  int32_t n_future, const float* d_state_future, const float* d_eef_future, const float* d_action_future,
                  int32_t store_rest_state, int32_t edge_rows, int32_t want_grad, float* const* d_grad_w, float* d_loss,
                  float* d_pred, int32_t* d_status);

/* ---- Device-resident physics-parameter fit (reference src/planning/physics_param_optimizer.py:178-226 under autograd).  Neither
 * call waits for the GPU. ---- */

/* One evaluation of the fit's objective and its gradient toward the physics parameter, enqueue only: dynamics_masked
 * (forward_dynamics.py:209-399) on R = p->B rows (p->H must be 1, p->y_mode 1; p->physics_param is unused), the masked chamfer of
 * each row's captured cloud to its observed cloud, and - when want_grad - the backward through the chain.  Edges are constants
 * of the gradient, as under the reference's autograd.
 *   d_state0 (R,N_o,3), d_obj_mask (R,N_o): per-row padded start clouds and masks; d_eef_xz (R,M,2), d_eef_delta (R,M,3): the
 *   shim's host decode, as for ag_rollout; h_repeat (R) HOST int32 = action_repeat: the step count S = max repeat and every
 *   step's live prefix come from it without a read-back, d_repeat (R) the same values on the device (the capture reads them).
 *   Step s runs over rows [0, L_s), L_s = 1 + the last row with repeat >= s: a caller that orders its rows by descending repeat
 *   steps every row exactly repeat times; any order gives the same outputs (the reference steps every row S times and discards).
 *   d_phys (R,N_o) the per-particle parameter; d_obs (R,N_t,3), d_obs_mask (R,N_t) the observed clouds; d_row_weight (R) the
 *   weight of each row's chamfer distance in the loss; d_w[22] the plain parameters (the values the context's weights were
 *   loaded from); edge_rows the caller's bound on a graph's edge count (sizes the workspace:
 *   per step B*(n_his*N*3 + 2*cap + N + 3) words kept for the backward, cap = min(max_nR, edge_rows), N = N_o + M, plus one
 *   backward chunk of ag_train_step's size).
 *   Per step: the batch edge builder on the last frame, the forward of ag_forward (same kernels, same bits), capture into
 *   d_state_seqs where repeat == s, tool rows = last + delta with y = the masked mean y of the prediction (fp64, fixed order,
 *   rounded once) + gripper offset, history shift.  Backward, last step first: dLoss/dpred = chamfer gradient where captured +
 *   the object rows of the next step's dLoss/dstate + its tool rows' y / valid count on every valid object row's y; the backward
 *   of ag_backward_inputs without the weight gradients; d_grad_phys accumulates the steps' dLoss/dphys in that order.
 *   Outputs: d_state_seqs (R,N_o,3), d_err (R) the chamfer distances, d_grad_phys (R,N_o) (want_grad), d_status (int32 x 4):
 *   [0] receives (atomic max, never cleared here) the edge count of a graph with more than min(max_nR, edge_rows) edges - such a
 *   graph is walked as an empty one and ag_ppm_adam_step skips; [1], [2] are ag_ppm_adam_step's.
 * Returns AG_OK for an overflowed graph.  No float atomics; a row's outputs do not depend on which other rows share the call. */
int ag_ppm_grad_step(ag_ctx* ctx, void* stream, const ag_rollout_params* p, const float* d_state0, const uint8_t* d_obj_mask,
                     const float* d_eef_xz, const float* d_eef_delta, const int32_t* h_repeat, const int32_t* d_repeat,
                     const float* d_phys, const float* d_obs, const uint8_t* d_obs_mask, int32_t N_t, const float* d_row_weight,
                     const float* const* d_w, int32_t edge_rows, int32_t want_grad, float* d_state_seqs, float* d_err,
                     float* d_grad_phys, int32_t* d_status);

/* The optimiser's side of one iteration, one small launch over n_starts starts of n_rows rows each (row of start k, interaction
 * i = k*n_rows + i when start_major, else i*n_starts + k).  Does nothing while d_status[0] != 0.  Otherwise, with it =
 * d_status[1]: per start the mean of its rows' d_err and the sum of its rows' d_grad_phys over rows and particles, in fp64 in a
 * fixed order (-> d_grad_start (n_starts); left as it is when d_grad_phys is NULL); d_hist_x / d_hist_err (hist_cap,n_starts)
 * row `it` = the evaluated parameter d_x and its error (it < hist_cap); d_best = [lowest error so far, its parameter, its
 * start, the first error of start 0]; when apply_update: Adam in double (beta 0.9 / 0.999, eps 1e-8; the bias corrections
 * 1 - beta^step are formed by the caller), clamp to [lo, hi], round to fp32 into d_x and into that start's rows of d_phys
 * (R,N_o); d_status[1] = it + 1, and d_status[2] += 1 when the update was applied (the count the caller's next bias
 * corrections continue from).
 * d_best[0] must start at +inf, the moments at zero. */
int ag_ppm_adam_step(ag_ctx* ctx, void* stream, const float* d_err, const float* d_grad_phys, int32_t n_starts, int32_t n_rows,
                     int32_t N_o, int32_t start_major, int32_t apply_update, double lr, double bias_correction1,
                     double bias_correction2, double lo, double hi, float* d_x, double* d_exp_avg, double* d_exp_avg_sq,
                     int32_t hist_cap, float* d_hist_x, double* d_hist_err, double* d_best, double* d_grad_start, float* d_phys,
                     int32_t* d_status);

/* Replaces the device side of dynamics() / dynamics_masked() (src/planning/forward_dynamics.py:12-205, 209-399):
 * the whole look-ahead x action-repeat loop, graph rebuilt every step, no host sync inside.
 *   d_state0      y_mode 0: (N_o,3) one start cloud broadcast to all candidates (:25);
 *                 y_mode 1: (B,N_o,3) per-candidate padded clouds (:225-227)
 *   d_obj_mask    (B,N_o) uint8 or NULL (= all valid)                                   (:107-115 / :302-309)
 *   d_eef_xz      (B,H,M,2) tool start x,z per look-ahead step; d_eef_delta (B,H,M,3)   (:42-75, computed by the shim
 *                 with torch CPU ops exactly as the reference does, so cos/sin bits match)
 *   h_repeat      (B,H) int32 HOST array = action_repeat (plan_utils.py:16).  A candidate is stepped exactly
 *                 h_repeat[b,h] times in look-ahead step h: per launch chunk the candidates are put in descending order
 *                 of their repeat count and every step is launched over the prefix that is still live (the reference steps
 *                 all of them to the batch maximum and discards the surplus, forward_dynamics.py:156-161; same outputs)
 *   d_phys_vec    NULL (use p->physics_param for every object particle), or (N_o,) per-particle physics parameters
 *                 shared by all candidates (the (B,n_p) branch of model.py:200-204 fed by forward_dynamics.py:151)
 *   d_state_seqs  (B,H,N_o,3) output, fully written (zeros where repeat==0, :32)
 * Synchronises the stream once at the end to read the overflow flag; returns AG_ERR_MAX_NR if any consumed graph
 * had more than max_nR edges (the shim re-raises Exception("Exceeds max dims")). */
int ag_rollout(ag_ctx* ctx, void* stream, const ag_rollout_params* p, const float* d_state0, const uint8_t* d_obj_mask,
               const float* d_eef_xz, const float* d_eef_delta, const int32_t* h_repeat, const float* d_phys_vec,
               float* d_state_seqs);

/* Same, but does not wait for the rollout: enqueue only.  *d_overflow_flag (int32, device, caller-zeroed) receives the max
 * edge count seen if it exceeded max_nR.  Used by bench.py to time the pure device path.  One exception: a call that shares the
 * contact-free prefix (option "share_prefix") waits for small plan kernels at its start, never for the rollout - when and how
 * often is stated once, at the top of this header ("WHICH ENTRY POINTS BLOCK THE HOST"). */
int ag_rollout_async(ag_ctx* ctx, void* stream, const ag_rollout_params* p, const float* d_state0,
                     const uint8_t* d_obj_mask, const float* d_eef_xz, const float* d_eef_delta,
                     const int32_t* h_repeat, const float* d_phys_vec, float* d_state_seqs,
                     int32_t* d_overflow_flag);

/* dynamics() for actions that are RESIDENT ON THE GPU (the planner samples them there): decode_action
 * (src/planning/plan_utils.py:11-20), the tool-keypoint layout (forward_dynamics.py:42-75) and the repeat-aware launch plan
 * all run in one device kernel; the host never reads an action, so nothing between the caller's sampling kernel and the
 * first rollout kernel waits for the GPU.  Enqueue only (like ag_rollout_async, incl. its "share_prefix" exception).
 *   d_action        (B,H,4) raw [x, z, theta, length]
 *   push_length     task_config push_length;  h_tool_offsets (M,) HOST: pusher_points[k][1] * sim_real_ratio (entry 0 unused;
 *                   may be NULL when M == 1)
 *   max_repeat      upper bound of action_repeat = int(length) the caller guarantees (e.g. its action_upper_lim[3]); a
 *                   look-ahead step is launched at most max_repeat times: steps past a chunk's own maximum find no live slot
 *                   and exit, and are no longer enqueued once the plan's maxima have reached the host (ag_ctx_launch_counts)
 *   d_action_seqs   (B,H,4) output: decoded actions [x_start, z_start, x_end, z_end] (the reference's 'action_seqs')
 *   d_flags         (>= 2 int32, device, caller-zeroed): [0] max edge count seen if it exceeded max_nR (as ag_rollout_async),
 *                   [1] largest action_repeat seen if it exceeded max_repeat (the results of such a candidate are invalid)
 * cos / sin are the device's: decoded values agree with a host decode to an ulp or two (a CUDA-resident reference would
 * use device transcendental functions too); everything downstream is the same arithmetic as ag_rollout. y_mode must be 0
 * (the masked variant takes host-decoded actions), M <= 8, 0 <= max_repeat <= 1024 (AG_ERR_INVALID / AG_ERR_UNSUPPORTED
 * otherwise). */
int ag_rollout_actions(ag_ctx* ctx, void* stream, const ag_rollout_params* p, const float* d_state0, const float* d_action,
                       float push_length, const float* h_tool_offsets, int32_t max_repeat, const float* d_phys_vec,
                       float* d_state_seqs, float* d_action_seqs, int32_t* d_flags);

/* The work an ag_rollout_actions call on (d_state0, d_action) would do, per candidate, WITHOUT rolling anything out:
 * h_work[b] (HOST, (B,) int32) = model forwards candidate b would be stepped = sum over look-ahead steps of min(action_repeat,
 * max_repeat), where look-ahead step 0 counts only the forwards from the candidate's first contact on when the contact-free
 * prefix applies to the batch (option "share_prefix": a candidate that never touches counts 0).  Runs the plan kernels and, if
 * none is kept for this start state, the tool-free base rollout - which then stays in the ctx for the rollout call that follows.
 * For cutting WORK-balanced shards of a candidate batch across GPUs (adaptigraph_amd/sharding.py): every rank calls
 * it on the full batch and gets the same numbers, no exchange.  The reference has no counterpart (one device, plan.py:87).
 * Arguments as ag_rollout_actions.  Synchronous (waits for the plan). */
int ag_rollout_work(ag_ctx* ctx, void* stream, const ag_rollout_params* p, const float* d_state0, const float* d_action,
                    float push_length, const float* h_tool_offsets, int32_t max_repeat, const float* d_phys_vec, int32_t* h_work);

/* ---- Per-candidate cost functions: SURVEY §8(f) rank 1 (reference src/planning/losses.py, src/planning/plan.py:27-59) ----
 * Non-finite inputs: every ag_cost_* entry does what torch.min / max / maximum do in the reference - a NaN that a reduction reads
 * comes out as NaN (never as "that particle was not there"), an infinity as the infinity the formula gives.  What a mask excludes
 * is never read.  The chamfer backward is specified for finite inputs only. */

/* chamfer(x, y) (losses.py:4-10): d_x (R,N,3); d_y (By,M,3) with By == 1 (one target for all rows, plan.py:146) or
 * By == R; optional uint8 masks d_xmask (R,N), d_ymask (By,M) keep only masked-in points (mean_chamfer, losses.py:12-24).
 * d_out (R,).  N + M must fit the LDS tile (<= ~13k points).  A row with a NaN coordinate in a masked-in point of either cloud
 * is NaN (By == 1: a NaN in y makes every row NaN); an infinite coordinate gives +inf; the other rows keep their bits. */
int ag_cost_chamfer(ag_ctx* ctx, void* stream, const float* d_x, const float* d_y, const uint8_t* d_xmask,
                    const uint8_t* d_ymask, int32_t R, int32_t N, int32_t M, int32_t By, float* d_out);

/* Gradient of ag_cost_chamfer toward x as torch autograd defines it on losses.py:4-10: inputs of ag_cost_chamfer plus
 * d_grad_out (R,) dLoss/dout -> d_grad_x (R,N,3), fully written.  Each min routes to its arg-min (lowest index among equal
 * distances), the norm has zero gradient at zero distance, masked-out x points get zero.  No atomics: repeated calls give the
 * same bits.  Asynchronous on the stream. */
int ag_cost_chamfer_backward(ag_ctx* ctx, void* stream, const float* d_x, const float* d_y, const uint8_t* d_xmask,
                             const uint8_t* d_ymask, int32_t R, int32_t N, int32_t M, int32_t By, const float* d_grad_out,
                             float* d_grad_x);

/* Particle statistics of d_state (R,N,3) -> d_out (R,5) = [box_loss, xmin, xmax, zmin, zmax]: box_loss (losses.py:26-35)
 * against h_box4 = {xmin, xmax, zmin, zmax} (NULL: entry 0 is 0), and the x/z bounds running_cost needs (plan.py:41-44).
 * A NaN x (z) coordinate makes the row's box_loss and its two x (z) bounds NaN. */
int ag_cost_state_stats(ag_ctx* ctx, void* stream, const float* d_state, int32_t R, int32_t N, const float* h_box4,
                        float* d_out);

/* Collision penalties (losses.py:37-92): kind 0 rope, 1 cloth, 2 granular.  d_state_pred (B,H,N,3), d_action (B,H,4)
 * raw [x,z,theta,len], d_state_init (N,3).  d_out (B,H,2) = [exp(-max(dmin - size,0)*100), min(dmax, 0.4*ratio)];
 * rope/granular: entry 0 is the penalty; cloth: 1 - e0 - 0.2 * e1 / max_batch(e1) (the caller owns the global max).
 * A NaN in the cloud a step reads, or in its action, makes both entries of that (b,h) NaN. */
int ag_cost_penalty(ag_ctx* ctx, void* stream, const float* d_state_pred, const float* d_action,
                    const float* d_state_init, int32_t B, int32_t H, int32_t N, int32_t kind, float sim_real_ratio,
                    float* d_out);

/* cloth_penalty's tail (losses.py:62-63) on the (B,H,2) output of ag_cost_penalty(kind 1): d_out[i] = 1 - e0 - 0.2 * e1 / max(e1),
 * n = B*H entries.  d_dmax: NULL = the maximum over this batch is formed here; else a device float holding it (a sharded batch
 * all-reduces it first).  One launch.  The maximum formed here is NaN if any e1 is (torch.max): then every d_out is. */
int ag_cost_cloth_combine(ag_ctx* ctx, void* stream, const float* d_raw, const float* d_dmax, int64_t n, float* d_out);

/* What is left of running_cost (src/planning/plan.py:35-53) once the particle reductions are done, in one launch:
 *   error_weight = fp32(2 / (double(max error) + 1e-6)); box penalty from the x / z bounds of ag_cost_state_stats against
 *   h_bbox4 = {x_lo, x_hi, z_lo, z_hi} (doubles, rounded to fp32 as torch rounds a Python scalar); reward[b] =
 *   -error_weight * error[b,H-1] - 5 * mean_h penalty[b,h] - 5 * mean_h box_penalty[b,h].
 * d_error, d_penalty (B,H); d_stats (B*H,5) as ag_cost_state_stats writes it; d_error_max: NULL = batch maximum formed here,
 * else a device float holding it (sharded batches all-reduce it first); d_reward (B,).  One NaN error makes the maximum formed
 * here, hence every reward, NaN; NaN bounds make that candidate's box penalty, hence its reward, NaN. */
int ag_cost_reward(ag_ctx* ctx, void* stream, const float* d_error, const float* d_penalty, const float* d_stats,
                   const float* d_error_max, const double* h_bbox4, int32_t B, int32_t H, float* d_reward);

/* ---- MPPI sampling / update: SURVEY §8(f) rank 2 (reference src/planning/plan_utils.py:31-101) ---- */

/* sample_action_seq (plan_utils.py:42-77).  d_act_seq (H,4) nominal actions [x, z, theta, length]; d_lo, d_hi (4,)
 * action limits; d_out (S,H,4).
 *   mode 0 (iter_index == 0, :48-50): d_rnd (S,H,4) uniform [0,1) draws -> d_out = u*(hi-lo)+lo; d_act_seq, d_scale unused.
 *   mode 1 (:51-77): d_rnd (H,S,4) = for look-ahead step i the (S,4) draws of N(0, noise_level) in the reference's draw
 *     order; d_scale (H,) = fp32(0.1 * 10^i) (:62); start and end point of the nominal push are perturbed, re-encoded
 *     as (theta, length) and limited (:31-39); sample 0 keeps the nominal action (:75).
 * The random draws are an input so that the function is testable against the reference's vectors. */
int ag_mppi_sample(ag_ctx* ctx, void* stream, const float* d_act_seq, const float* d_lo, const float* d_hi,
                   const float* d_rnd, const float* d_scale, int32_t S, int32_t H, int32_t mode, float push_length,
                   float* d_out);

/* optimize_action_mppi (plan_utils.py:80-101): softmax(reward * reward_weight) over the B candidates, weighted mean of
 * the start and end points per look-ahead step, re-encoded and limited.  d_act_seqs (B,H,4), d_reward (B,), d_out (H,4).
 * One workgroup per look-ahead step, fixed-order reductions (deterministic). */
int ag_mppi_update(ag_ctx* ctx, void* stream, const float* d_act_seqs, const float* d_reward, const float* d_lo,
                   const float* d_hi, int32_t B, int32_t H, float reward_weight, float push_length, float* d_out);

/* clip_actions (plan_utils.py:35-39) on n actions: theta wrapped into [-pi, pi), every component clamped. */
int ag_mppi_clip(ag_ctx* ctx, void* stream, const float* d_in, const float* d_lo, const float* d_hi, int64_t n,
                 float* d_out);

/* Introspection for bench.py / tests: HIP-event time of every launch of a kernel family, recorded on the stream the
 * kernels run on.  family_mask bit i enables family i of: edge_count, edge_emit, prep, node_enc, edge_enc, mp,
 * node_prop, node_final, roll_init, roll_update, cost (0 = off; "mp" is kept for index stability and never records: the
 * message passing is fused into node_prop / node_final).  A non-zero mask pins the rollout to ONE stream so that a
 * duration measures the kernel alone; bit 30 keeps the streams instead (durations then include the other stream's
 * co-running kernels - what a kernel trace of a normal run shows).  ag_ctx_kernel_stats waits for the recorded
 * events and returns the total milliseconds and launch count since the last reset. */
int ag_ctx_set_profiling(ag_ctx* ctx, int32_t family_mask);
int ag_ctx_kernel_stats(ag_ctx* ctx, const char* kernel, double* out_total_ms, int64_t* out_launches);
int ag_ctx_reset_stats(ag_ctx* ctx);

/* ag_train_step on one PART of an optimiser step (a micro-batch of this rank, or this rank's share of a data-parallel batch):
 * every argument of ag_train_step in the same order, then
 *   B_total     rows of the whole step over all parts and ranks (>= B, else AG_ERR_INVALID).  The MSE mean and its gradient
 *               divide by B_total * n_p * 3 instead of B * n_p * 3 (n_p is the same in every part), so d_loss and d_grad_w are
 *               this part's share of the full batch's: the shares of the parts sum to the one-call values.
 *   accumulate  0: d_grad_w[22] and d_loss[0..n_future] are overwritten (the first part of a step); != 0: they hold the earlier
 *               parts' sums and are added to.  The old fp32 value joins the fixed-order fp64 sum of each weight-gradient
 *               reduction (and of each step's MSE) before its one rounding: no second rounding, no float atomics, no extra pass.
 *               d_loss[n_future] is again the fp32 sum of d_loss[0..n_future-1] in step order.  d_pred is this part's own.
 * d_status[0] stays the sticky atomic max: an overflowed graph in any part makes the following ag_adam_step skip.
 * ag_train_step is this call with B_total = B and accumulate = 0 (one implementation, the same bits).  Enqueue only. */
int ag_train_step_part(ag_ctx* ctx, void* stream, const float* d_state, const float* d_attrs, const float* d_action,
                       const float* d_phys, const float* d_group, int32_t n_inst, const int32_t* d_recv, const int32_t* d_send,
                       const int32_t* d_row_ptr, const int32_t* d_n_edges, int32_t edge_cap, int32_t B, int32_t N, int32_t n_p,
                       const float* const* d_w, int32_t n_future, const float* d_state_future, const float* d_eef_future,
                       const float* d_action_future, int32_t store_rest_state, int32_t edge_rows, int32_t want_grad,
                       float* const* d_grad_w, float* d_loss, float* d_pred, int32_t* d_status, int32_t B_total,
                       int32_t accumulate);

/* ---- set losses of the training side (reference src/dynamics/gnn/loss.py: ChamferLoss :4-22, HausdorffLoss :63-82) and the
 * training step with a list of losses (train.py:65, 100-102: loss_funcs = [(func, weight), ...]).  Additive exports. ---- */
#define AG_LOSS_MSE 0
#define AG_LOSS_CHAMFER 1
#define AG_LOSS_HAUSDORFF 2
#define AG_LOSS_EMD 3
#define AG_LOSS_ROWS 16         /* flag, or-ed onto AG_LOSS_CHAMFER, _HAUSDORFF or _EMD: the loss over each graph's real rows (below) */
typedef struct ag_loss_spec {
    int32_t n_terms;            /* 1..4 */
    int32_t kind[4];            /* AG_LOSS_*, a set kind optionally | AG_LOSS_ROWS */
    float weight[4];            /* finite */
} ag_loss_spec;

/* One set loss over a batch of cloud pairs: d_x (B,N,3) the prediction, d_y (B,M,3) the label -> d_out[0].  With
 * d(b,i,j) = sqrt(dx*dx + dy*dy + dz*dz) in fp32 (every operation rounded on its own), mx(b,i) = min_j d, my(b,j) = min_i d:
 *   AG_LOSS_CHAMFER    sum_{b,i} mx / (B_total * N) + sum_{b,j} my / (B_total * M)   (loss.py:14-17; B_total >= B: the rows of
 *                      the whole batch when this call holds a part of it - the parts' values then add up to the whole's)
 *   AG_LOSS_HAUSDORFF  max_{b,i} mx + max_{b,j} my                                    (loss.py:74-77; B_total must equal B, else
 *                      AG_ERR_UNSUPPORTED: a max does not split into parts)
 * The sums run in fp64 in a fixed order (inside a graph, then over the graphs in index order) and are rounded once.  Arg-min and
 * arg-max take the lowest index among equals.  A NaN coordinate makes the loss NaN.  N + M must fit the LDS tile of
 * ag_cost_chamfer (<= ~13k points), else AG_ERR_UNSUPPORTED before anything is enqueued.  The plain kinds count every row, as
 * the reference's training losses do; kind | AG_LOSS_ROWS counts each graph's real rows (below).
 * d_work: NULL, or B*(N+M) + 4 int32 that receive the arg-min tables (per graph: nearest y of every x, then nearest x of every
 * y) and the Hausdorff winners {b, i, b, j}.  Enqueue only.
 *   AG_LOSS_EMD        sum_b sum_{(i,j) in A_b} d(b,i,j) / (B_total * K), K = min(N, M)    (loss.py:25-60; splits into parts through
 *                      B_total as Chamfer does)
 * A_b is the one-to-one matching of K pairs of graph b with the smallest sum of distances - the linear assignment problem on the
 * fp32 distances, solved exactly on the device in fp64 (shortest augmenting paths with dual variables), one workgroup per graph;
 * the smaller cloud is the row side, x when N == M.  Tie rule of the search: among equal path costs a free column wins, then the
 * lowest column index (the optimum of generic clouds is unique and does not depend on it).  Limits, AG_ERR_UNSUPPORTED before
 * anything is enqueued: K <= 512, and N + M must fit the solver's LDS tile (<= ~4k points).  A graph with a non-finite coordinate
 * is not solved: it is marked failed and makes the loss NaN; ag_set_loss_backward then writes NaN into its rows.  (The reference
 * prints a message and reuses the previous graph's indices there; that is not reproduced.)
 * d_work for AG_LOSS_EMD: the same B*(N+M) + 4 int32, holding first the (B, N) match table - entry (b, i) is the y index matched
 * to x_i of graph b, or -1 (N > M: N - M rows stay unmatched; a failed graph: every row) - then B status words (0 solved, 1
 * non-finite input, 2 a loop bound ran out).
 *
 * kind | AG_LOSS_ROWS (valid on the three set kinds only; AG_LOSS_MSE | AG_LOSS_ROWS is AG_ERR_INVALID): padded batches.  Graph b's
 * real rows are the first nx[b] rows of x[b] and the first ny[b] rows of y[b].  d_work is then REQUIRED (NULL: AG_ERR_INVALID) and
 * has B*(N+M) + 4 + 2B int32: everything before the last 2B words keeps the layout and meaning above, and the last 2B words are
 * INPUTS, nx[0..B) then ny[0..B).  The counts are clamped into [0, N] and [0, M] on the device before they bound a loop or address
 * anything; rows behind them are never read, so NaN or inf there changes no output bit.  d, the arg-min rule, the tie rules and
 * NaN propagation are those above, over the real rows:
 *   AG_LOSS_CHAMFER | AG_LOSS_ROWS    (1/B_total) sum_b [ (1/nx_b) sum_{i<nx_b} min_{j<ny_b} d + (1/ny_b) sum_{j<ny_b} min_{i<nx_b} d ]
 *                      - the mean over graphs of each graph's own Chamfer distance, not the pooled mean; it splits into parts
 *                      through B_total with no count exchanged.  With full counts it is the plain kind up to the last place.
 *   AG_LOSS_HAUSDORFF | AG_LOSS_ROWS  max_{b, i<nx_b} mx + max_{b, j<ny_b} my; with full counts the plain kind's bits.  Refused in parts.
 *   AG_LOSS_EMD | AG_LOSS_ROWS        (1/B_total) sum_b (1/K_b) sum_{(i,j) in A_b} d, K_b = min(nx_b, ny_b), A_b the optimal assignment of
 *                      the real rows; the smaller real cloud is the row side, x when the counts are equal.  The limits stay on
 *                      the padded sizes N, M.  A non-finite coordinate in a real row fails that graph alone.
 * A graph with an empty side (nx_b == 0 or ny_b == 0) is batch padding, a rule of this library (torch's mean over nothing is
 * NaN): it adds 0 to Chamfer and Earth-mover, has no Hausdorff candidate, its gradient rows are 0, and it still counts in
 * B_total; with every graph empty Hausdorff is 0 and the winners are -1.  Arg-min entries of padding rows are 0, match entries of
 * padding or unmatched rows -1. */
int ag_set_loss(ag_ctx* ctx, void* stream, const float* d_x, const float* d_y, int32_t B, int32_t N, int32_t M, int32_t B_total,
                int32_t kind, float* d_out, int32_t* d_work);

/* Gradient of ag_set_loss toward x as torch autograd defines it on loss.py: the same inputs, d_grad_out[0] = dLoss/dout ->
 * d_grad_x (B,N,3), fully written.  Each min routes to its arg-min, the norm has zero gradient at zero distance, Hausdorff
 * reaches only its two winning pairs.  The label is data: no gradient toward y.  d_work: NULL (the nearest-neighbour pass runs
 * again), or the buffer an ag_set_loss call on the same inputs and kind filled (its tables are used; indices are clamped before
 * they address anything).  No atomics: repeated calls give the same bits.  Enqueue only.
 * AG_LOSS_EMD: d_grad_x[b,i] = d_grad_out[0] / (B_total * K) * (x_i - y_j) / d(b,i,j) for the matched pair (i, j), zero for an
 * unmatched x_i and at zero distance, NaN in every row of a failed graph.
 * kind | AG_LOSS_ROWS: d_work is required - the buffer of the forward, whose last 2B words hold the counts.  Rows i >= nx[b] are
 * written as exact 0; a real row's scale is d_grad_out[0] / (B_total * nx_b) for the x-side Chamfer sum, / (B_total * ny_b) for
 * the y-side sum, / (B_total * K_b) for Earth-mover; a failed Earth-mover graph has NaN in its real rows. */
int ag_set_loss_backward(ag_ctx* ctx, void* stream, const float* d_x, const float* d_y, int32_t B, int32_t N, int32_t M,
                         int32_t B_total, int32_t kind, const float* d_grad_out, float* d_grad_x, const int32_t* d_work);

/* ag_train_step_part with a list of losses: every argument of ag_train_step_part in the same order, then
 *   spec          1..4 terms (kind, weight); per step loss = the fp32 sum over the list, in list order, of weight * term
 *                 (train.py:100-102), a set term being ag_set_loss of the step's prediction (B,n_p,3) against
 *                 d_state_future[:, fi].  d_loss keeps its layout (n_future step losses, then their fp32 sum), the backward
 *                 starts from the list's gradient.  Terms of one kind share their kernels; one nearest-neighbour pass per step
 *                 serves every set term.
 *   d_loss_terms  NULL, or (n_future, n_terms) floats: every step's terms before weighting.  Required when accumulate != 0:
 *                 the parts' running sums live there, each part's share joining in fp64 before the one rounding.
 * B_total and accumulate act on MSE and Chamfer terms as in ag_train_step_part (both are means over the batch: a part's share
 * is B / B_total), and on an Earth-mover term (AG_LOSS_EMD, a mean over the B_total * n_p matched pairs; n_p <= 512 and 2 * n_p
 * within its LDS tile, else AG_ERR_UNSUPPORTED).  A Hausdorff term with B_total != B or accumulate != 0 returns AG_ERR_UNSUPPORTED; an unknown kind, a
 * non-finite weight or n_terms outside 1..4 AG_ERR_INVALID; 2 * n_p beyond the LDS tile with a set term AG_ERR_UNSUPPORTED - all
 * before anything is enqueued.  A set kind may carry AG_LOSS_ROWS (Chamfer and Hausdorff terms of one list must agree on it, and
 * Earth-mover terms among themselves, else AG_ERR_INVALID): graph b's real rows, of the prediction and of d_state_future[:, fi]
 * alike, are then its first n_b rows, n_b = the first i < n_p with d_attrs[b, i, 0] <= 0, or n_p if there is none - the live
 * prefix that the device data set writes.  An MSE term of the same list runs over all rows, as in train.py.
 * spec = {1, {AG_LOSS_MSE}, {1}} gives ag_train_step_part's bits; ag_train_step and
 * ag_train_step_part themselves are unchanged and never run this path.  Enqueue only. */
int ag_train_step_losses(ag_ctx* ctx, void* stream, const float* d_state, const float* d_attrs, const float* d_action,
                         const float* d_phys, const float* d_group, int32_t n_inst, const int32_t* d_recv, const int32_t* d_send,
                         const int32_t* d_row_ptr, const int32_t* d_n_edges, int32_t edge_cap, int32_t B, int32_t N, int32_t n_p,
                         const float* const* d_w, int32_t n_future, const float* d_state_future, const float* d_eef_future,
                         const float* d_action_future, int32_t store_rest_state, int32_t edge_rows, int32_t want_grad,
                         float* const* d_grad_w, float* d_loss, float* d_pred, int32_t* d_status, int32_t B_total,
                         int32_t accumulate, const ag_loss_spec* spec, float* d_loss_terms);

/* ---- training batches on the device: the sampling, assembly and graph half of DynDataset.__getitem__
 * (src/dynamics/dataset/dataset.py:117-383).  Episode positions live in two flat fp32 buffers (object points, end-effector
 * points), episode after episode, frame after frame, without padding.  All three calls only enqueue. */

/* Both farthest-point stages of dataset/graph.py:8-36 (fps) for B samples in one launch, one workgroup per sample.
 *   d_pos        flat object positions; sample b's cloud is the d_npts[b*stride] points from point d_pt_off[b*stride] on
 *                (int64 arrays read with an element stride, so that both may be columns of one per-sample table)
 *   d_fps_start  first point of stage 1, in [0, N_e); d_fps_radius fp32 radius of stage 2 (>= 0); d_rad_start first point of
 *                stage 2, in [0, min(max_nobj, N_e))   (out-of-range starts are clamped into range)
 *   max_pts      the caller's bound on d_npts (a larger count is truncated to it)
 * Stage 1 is dgl.geometry.farthest_point_sampler restated from its CPU implementation (dgl itself was not available to
 * check against): min(max_nobj, N_e) points; running minimum of the fp32 squared distance ((dx*dx + dy*dy) + dz*dz), no
 * contraction, initialised to 1e10; the next point is the strict-greater argmax, so the lowest index wins ties.  Stage 2
 * is fps_rad_idx (src/dynamics/utils.py:10-24) on the stage-1 points in stage-1 order: distance = correctly rounded sqrt of
 * the same sum; while the maximum exceeds the radius (fp32 against fp32) append the argmax (lowest index) and take the
 * minimum.  Outputs: d_fps_idx (B, max_nobj) int32 = stage1[stage2] in selection order, -1 behind the d_n_obj[b] entries.
 * Limits: 1 <= max_nobj <= 1024, 1 <= max_pts <= 8192 (the cloud is LDS-resident), else AG_ERR_UNSUPPORTED. */
int ag_fps_batch(ag_ctx* ctx, void* stream, const float* d_pos, const int64_t* d_pt_off, const int64_t* d_npts, int32_t stride,
                 const int32_t* d_fps_start, const float* d_fps_radius, const int32_t* d_rad_start, int32_t B, int32_t max_nobj,
                 int32_t max_pts, int32_t* d_fps_idx, int32_t* d_n_obj);

/* ag_fps_batch for clouds that do not fit into LDS: the perceived tabletop cloud of perception.py:259-315 (construct_graph), one
 * workgroup per cloud, any number of clouds per launch.  Arguments, both stages, their fp32 arithmetic, the tie rule, the clamping
 * of the starts and the outputs are ag_fps_batch's: for every input that both entries accept the outputs are equal bit for bit (an
 * empty cloud gives d_n_obj[b] = 0 and -1 throughout).  The cloud is read from global memory on every sweep; the running minima
 * of a cloud's first 32768 points stay in registers, those of the points behind live in the call's workspace
 * (B * (max_pts - 32768) floats, carved from the context: a second call of the same shape allocates nothing).
 * Limits: 1 <= max_nobj <= 1024, 1 <= max_pts <= 1048576, else AG_ERR_UNSUPPORTED before anything is enqueued.  Enqueue only. */
int ag_fps_cloud(ag_ctx* ctx, void* stream, const float* d_pos, const int64_t* d_pt_off, const int64_t* d_npts, int32_t stride,
                 const int32_t* d_fps_start, const float* d_fps_radius, const int32_t* d_rad_start, int32_t B, int32_t max_nobj,
                 int32_t max_pts, int32_t* d_fps_idx, int32_t* d_n_obj);

/* One training batch (dataset.py:171-300), N = max_nobj + n_eef rows per sample.  T = n_his + n_future pair frames per sample: a
 * rest frame (store_rest_state with a short pair) is just frame index 0 in front. */
typedef struct ag_dataset_batch {
    const float* d_obj_pos;        /* flat object positions                                                              */
    const float* d_eef_pos;        /* flat end-effector positions, n_eef points per frame                                */
    const int64_t* d_sample;       /* (B, 5 + T): [unused, N_e, first object point of the episode, first end-effector point
                                      of the episode, episode index, frame index x T]; frame t of the episode starts at point
                                      first + frame * N_e (n_eef)                                                        */
    const int32_t* d_fps_idx;      /* (B, max_nobj), d_n_obj (B,): ag_fps_batch's outputs                                */
    const int32_t* d_n_obj;
    const double* d_phys;          /* (n_episodes, phys_dim) stored physics parameter                                    */
    const double* d_phys_noise;    /* (B, phys_dim) or NULL                                                              */
    const double* d_state_noise;   /* (B, n_his, N, 3) or NULL: added to EVERY row of state (padding and tool rows too, as
                                      the reference does), in double, one rounding = numpy's float32 += float64          */
    const double* d_rot;           /* (B,) angle or NULL: then state, action, eef_future, action_future and state_future are
                                      multiplied by the fp32 matrix of dataset.py:277-285: x' = x*c + y*s, y' = x*(-s) + y*c
                                      (c, s = cos, sin in double, rounded to fp32; separate products, one sum), z' = z    */
    const double* d_adj_thresh;    /* (B,) or NULL: edge radius -> d_thr2 = fp32(adj*adj in double) (graph.py:86,101) and
                                      d_cull = nextafter(fp32(|adj|), inf), the inputs of ag_build_edges_graphs          */
    int32_t B, n_his, n_future, max_nobj, n_eef, phys_dim, n_mat, mat_col;
    float* d_state;                /* (B, n_his, N, 3)                                                                    */
    float* d_action;               /* (B, N, 3) fp32 difference of the end-effector rows, frames n_his and n_his - 1      */
    float* d_eef_future;           /* (B, n_future - 1, N, 3)                                                             */
    float* d_action_future;        /* (B, n_future - 1, N, 3)                                                             */
    float* d_state_future;         /* (B, n_future, max_nobj, 3)                                                          */
    float* d_attrs;                /* (B, N, 2)                                                                           */
    float* d_p_instance;           /* (B, max_nobj, 1)                                                                    */
    uint8_t* d_obj_mask;           /* (B, max_nobj)                                                                       */
    uint8_t* d_state_mask;         /* (B, N) valid particle; d_eef_mask (B, N) tool particle: the edge builder's masks    */
    uint8_t* d_eef_mask;
    int64_t* d_material_index;     /* (B, max_nobj, n_mat): column mat_col is 1 on the sampled rows                       */
    float* d_physics_param;        /* (B, phys_dim) = fp32(stored + noise): the noise goes to a copy, the stored value
                                      never changes (the reference adds in place, dataset.py:261-266)                    */
    float* d_thr2; float* d_cull;  /* (B,) each; written only with d_adj_thresh                                           */
} ag_dataset_batch;
/* One launch writes every output above, zero padding included; nothing else is allocated or staged. */
int ag_dataset_assemble(ag_ctx* ctx, void* stream, const ag_dataset_batch* batch);

/* B independent graphs under ag_build_edges_single's rule (construct_edges_from_states, graph.py:68-231, default arguments:
 * threshold squared in double then rounded, connect_tools_all unconditional, no tool<->tool edge) in one launch pair.
 *   d_pos        graph b's (N,3) positions start at d_pos + b * pos_bstride floats (0: N*3) - e.g. the last history frame of
 *                a (B, n_his, N, 3) state
 *   d_thr2       (B,) squared threshold per graph; d_cull_radius (B,) with cull^2 >= thr2 per graph (the caller's duty)
 * Outputs as ag_build_edges: d_n_edges[b] is the TRUE count even above edge_cap (then nothing is written for graph b). */
int ag_build_edges_graphs(ag_ctx* ctx, void* stream, const float* d_pos, int64_t pos_bstride, const uint8_t* d_mask,
                          const uint8_t* d_tool_mask, int32_t B, int32_t N, const float* d_thr2, const float* d_cull_radius,
                          int32_t topk, int32_t connect_tools_all, int32_t edge_cap, int32_t* d_recv, int32_t* d_send,
                          int32_t* d_row_ptr, int32_t* d_n_edges);

/* ---- open-loop eval rollout (src/dynamics/rollout/rollout.py:103-260, rollout_from_start_graph's loop) for B rollouts at once.
 * One call is one step of all B: the forward on the current graphs, the ground-truth error of its prediction, the next model
 * input, and the next graphs at top-k `topk` into the OTHER half of the caller's double-buffered edge arrays.  Enqueue only: the
 * caller reads d_n_edges_next back (its one wait per step), rebuilds the graphs above max_nR at a smaller top-k
 * (ag_build_edges_graphs on d_state_next's last frames) and swaps the halves.  N = max_nobj + n_eef rows per graph. */
typedef struct ag_eval_step_args {
    /* the step's model input, as ag_forward takes it */
    const float* d_state;          /* (B, n_his, N, 3)                                                                   */
    const float* d_action;         /* (B, N, 3)                                                                          */
    const float* d_attrs;          /* (B, N, 2)                                                                          */
    const float* d_phys;           /* (B, N)                                                                             */
    const float* d_group;          /* (B, N, n_inst)                                                                     */
    const int32_t* d_recv;         /* (B, edge_cap); d_send alike; d_row_ptr (B, N + 1); d_n_edges (B,)                  */
    const int32_t* d_send;
    const int32_t* d_row_ptr;
    const int32_t* d_n_edges;
    /* ground truth and tool trajectory: the flat episode buffers of ag_dataset_batch and the sampling of the start graphs */
    const float* d_obj_pos;        /* obj_points points                                                                  */
    const float* d_eef_pos;        /* eef_points points                                                                  */
    const int32_t* d_fps_idx;      /* (B, max_nobj), d_n_obj (B,): ag_fps_batch's outputs for the start graphs           */
    const int32_t* d_n_obj;
    const int64_t* d_frames;       /* (B, 3) for THIS step: [first object point of the frame the prediction is compared
                                      with, first tool point of the next pair's start frame or -1 (the rollout ended), first
                                      tool point of the next pair's end frame]                                           */
    /* the edge builder's per-graph inputs (ag_build_edges_graphs) */
    const uint8_t* d_state_mask;   /* (B, N) valid particle; d_eef_mask (B, N) tool particle                             */
    const uint8_t* d_eef_mask;
    const float* d_thr2;           /* (B,) squared threshold; d_cull (B,) culling radius, cull^2 >= thr2                 */
    const float* d_cull;
    int64_t obj_points, eef_points;   /* sizes of the two flat buffers in points: indices formed from d_frames are clamped */
    int32_t B, max_nobj, n_eef, n_inst, edge_cap;
    int32_t edge_rows;             /* every graph is promised to have at most this many edges (the back-off has run); a
                                      graph beyond min(edge_cap, edge_rows) is presented empty and its count is raised into
                                      d_status[0] (sticky atomic max, as ag_train_step)                                  */
    int32_t topk, connect_tools_all, store_rest_state;
    int32_t pred_given;            /* != 0: no forward, d_pred is an INPUT (the advance and the builder alone)           */
    int32_t step, err_stride;      /* the error of graph b goes to d_err[step * err_stride + b]                          */
    /* outputs */
    float* d_pred;                 /* (B, max_nobj, 3): ag_forward's d_pred_pos, bit for bit                             */
    float* d_err;                  /* fp32(mean over n < d_n_obj[b] of |pred[b,n] - obj_pos[frames[b,0] + fps_idx[b,n]]|):
                                      differences, squares, sqrt and the sum in fp64 in a fixed order (no atomics), one
                                      rounding; a NaN prediction gives NaN; d_n_obj[b] == 0 gives NaN                    */
    float* d_state_next;           /* (B, n_his, N, 3), not d_state: history shifted by one (store_rest_state: frame 0 stays,
                                      frame 1 leaves), last frame = all max_nobj predicted rows, then the n_eef tool rows of
                                      the next start frame.  d_action_next (B, N, 3): zero on the object rows, the fp32
                                      difference end - start on the tool rows.  A graph that ended writes neither.       */
    float* d_action_next;
    int32_t* d_recv_next;          /* the next graphs, as ag_build_edges_graphs writes them; d_n_edges_next[b] is the TRUE */
    int32_t* d_send_next;          /* count even above edge_cap, and 0 for a graph that ended                            */
    int32_t* d_row_ptr_next;
    int32_t* d_n_edges_next;
    int32_t* d_status;             /* [0]: see edge_rows                                                                 */
} ag_eval_step_args;
/* Limits: N <= 4096 (the LDS-resident edge builder), max_nobj <= 1024, topk as ag_build_edges; else AG_ERR_UNSUPPORTED before
 * anything is enqueued.  The predictions are ag_forward's for the same B (same launch chunk, same kernels). */
int ag_eval_step(ag_ctx* ctx, void* stream, const ag_eval_step_args* args);

/* ---- the "tool to all non-fixed particles" rule (graph.py:125-171) and its flat kNN filter for B graphs in one launch.
 * Semantics are ag_edges_apply_tool_rule's, per graph b, with the subset S = d_mask AND (y > thr[b]) formed on the device:
 *   the rule applies only if the base list holds at least one edge whose sender is a tool (graph.py:128-135), otherwise the base
 *   graph is copied through; with 0 < d_kNN[b] < 1 only keepK = (int)(kNN * #pairs) (in double) of the (receiver in S <- tool)
 *   pairs survive, ranked by (fp32 distance, flat row-major pair index), tool receivers in S counting as pairs at distance 1e10;
 *   no tool<->tool edge remains.
 * thr[b] = fadd(fmul(fsub(fmul(max_y, fp32(ratio)), min_y), fp32(0.1)), min_y), four separately rounded fp32 operations
 * (rollout.py:136 and graph.py:134 on numpy float32 scalars), max_y / min_y over the y of the rows the bounds source names:
 *   row r < d_bounds_n[b] is point d_bounds_first[b] + (d_bounds_idx ? d_bounds_idx[b * idx_stride + r] : r) of the flat
 *   (bounds_points, 3) buffer d_bounds_pos (indices are clamped into the buffer; with d_bounds_idx, r < idx_stride); a zero row
 *   takes part iff pad_rows > d_bounds_n[b].  A NaN among them makes thr NaN (as np.max does) and S empty; so does no row at all.
 *   Dataset: the episode buffer, first point of frame n_his - 1, ag_fps_batch's d_fps_idx / d_n_obj, pad_rows = max_nobj
 *   (dataset.py:186-209).  Eval rollout: d_state_next, b * n_his * N + (n_his - 1) * N, no gather, d_n_obj, pad_rows 0
 *   (rollout.py:125-133).
 * The base graphs are ag_build_edges_graphs' outputs with capacity base_cap.  A graph whose d_n_edges_in[b] is outside
 * [0, base_cap], whose CSR is not consistent (rows ascending, senders strictly ascending within [0, N)) or whose tool count is
 * not n_tools gets d_n_edges_out[b] = -1 and nothing else.  Outputs as ag_build_edges_graphs: sorted by (receiver, sender),
 * d_n_edges_out[b] the TRUE count even above edge_cap (then nothing else is written for graph b).  A graph's result does not
 * depend on the others in the launch.  Input and output arrays must not overlap.  Enqueue only.
 * Limits: N <= 4096, n_tools <= 64, N * n_tools <= 8192 (a graph's pair tables live in LDS); beyond them AG_ERR_UNSUPPORTED
 * before anything is enqueued. */
typedef struct ag_rule_graphs_args {
    const float* d_pos;            /* graph b's (N,3) positions start at d_pos + b * pos_bstride floats (0: N*3)          */
    int64_t pos_bstride;
    const uint8_t* d_mask;         /* (B, N) valid particle; d_tool_mask (B, N) tool particle                            */
    const uint8_t* d_tool_mask;
    const int32_t* d_send_in;      /* (B, base_cap); d_row_ptr_in (B, N + 1); d_n_edges_in (B,)                          */
    const int32_t* d_row_ptr_in;
    const int32_t* d_n_edges_in;
    const double* d_kNN;           /* (B,)                                                                               */
    const float* d_bounds_pos;     /* the bounds source, see above                                                       */
    const int64_t* d_bounds_first; /* (B,)                                                                               */
    const int32_t* d_bounds_idx;   /* (B, idx_stride) or NULL                                                            */
    const int32_t* d_bounds_n;     /* (B,)                                                                               */
    int64_t bounds_points;
    double ratio;                  /* connect_tool_surface_ratio; rounded to fp32 before use                             */
    int32_t B, N, n_tools, base_cap, idx_stride, pad_rows, edge_cap;
    int32_t* d_recv;               /* (B, edge_cap); d_send alike; d_row_ptr (B, N + 1); d_n_edges_out (B,)              */
    int32_t* d_send;
    int32_t* d_row_ptr;
    int32_t* d_n_edges_out;
    float* d_thr;                  /* (B,) or NULL: the thresholds                                                       */
} ag_rule_graphs_args;
int ag_edges_nonfixed_rule_graphs(ag_ctx* ctx, void* stream, const ag_rule_graphs_args* args);

/* ---- the "tool to the two closest surface planes" rule (graph.py:175-221) for B graphs in one launch: bounds, plane choice and
 * subset are formed on the device.  Per graph b, on the input list (ag_build_edges_graphs' output or, chained, the output of
 * ag_edges_nonfixed_rule_graphs):
 *   bounds : max / min of x, y and z over the rows the bounds source names (ag_rule_graphs_args' source, field for field: a zero row
 *            takes part iff pad_rows > d_bounds_n[b]; a NaN makes the bounds of its axis NaN, as np.max does; so does no row at all),
 *            then, in separately rounded fp32 operations with r = fp32(ratio) and q = fp32(1 - ratio formed in double):
 *              bounds_order 0 (the eval step loop, rollout.py:132-139): max_a = max_a * r, min_a = (max_a*r - min_a) * q + min_a
 *              bounds_order 1 (construct_graph, rollout/graph.py:446-458): min_a = (max_a - min_a) * q + min_a, then max_a = max_a * r
 *            for a in {x, z}; max_y = max_y * r; min_y as it is.  The two orders agree at ratio 1.
 *   contact: check = the number of input edges whose sender is a tool.  0: the input graph is copied through.
 *   planes : value = N * (n0 * d_0 + n1 * d_1) in double, n1 = check, n0 = (#d_mask) * n_tools - check, d_k the fp32 squared distance
 *            (one fsub, one fmul) of particle k's coordinate to the bound, k = 0 and min(1, N - 1) whatever their mask (graph.py:190-196
 *            index with 0 / 1 values), for the planes max_y, min_x, max_x, min_z, max_z in this order (0 .. 4); the two smallest by
 *            (value, index), NaN last.
 *   subset : S = d_mask AND side(first) AND side(second), >= for the max planes and <= for the min planes; every tool becomes a
 *            sender to every receiver in S, edges from a sender in S to a tool receiver are dropped, no tool<->tool edge remains
 *            (ag_edges_apply_tool_rule at kNN 1).
 * Guard, outputs and d_n_edges_out (-1 = refused graph; the TRUE count even above edge_cap, then nothing else is written for graph b)
 * as ag_edges_nonfixed_rule_graphs.  A graph's result does not depend on the others in the launch.  Input and output arrays must
 * not overlap.  Enqueue only: the call never waits for the GPU.
 * Limits: N <= 4096, n_tools <= 64; beyond them AG_ERR_UNSUPPORTED before anything is enqueued. */
typedef struct ag_surface_rule_graphs_args {
    const float* d_pos;            /* graph b's (N,3) positions start at d_pos + b * pos_bstride floats (0: N*3)          */
    int64_t pos_bstride;
    const uint8_t* d_mask;         /* (B, N) valid particle; d_tool_mask (B, N) tool particle                            */
    const uint8_t* d_tool_mask;
    const int32_t* d_send_in;      /* (B, base_cap); d_row_ptr_in (B, N + 1); d_n_edges_in (B,)                          */
    const int32_t* d_row_ptr_in;
    const int32_t* d_n_edges_in;
    const float* d_bounds_pos;     /* the bounds source, as ag_rule_graphs_args                                          */
    const int64_t* d_bounds_first; /* (B,)                                                                               */
    const int32_t* d_bounds_idx;   /* (B, idx_stride) or NULL                                                            */
    const int32_t* d_bounds_n;     /* (B,)                                                                               */
    int64_t bounds_points;
    double ratio;                  /* connect_tool_surface_ratio                                                         */
    int32_t B, N, n_tools, base_cap, idx_stride, pad_rows, bounds_order, edge_cap;
    int32_t* d_recv;               /* (B, edge_cap); d_send alike; d_row_ptr (B, N + 1); d_n_edges_out (B,)              */
    int32_t* d_send;
    int32_t* d_row_ptr;
    int32_t* d_n_edges_out;
    float* d_bounds;               /* (B, 6) or NULL: max_y, min_y, max_x, max_z, min_x, min_z as the rule used them     */
    int32_t* d_planes;             /* (B, 2) or NULL: the two chosen planes (0 .. 4), -1 -1 without contact              */
} ag_surface_rule_graphs_args;
int ag_edges_surface_rule_graphs(ag_ctx* ctx, void* stream, const ag_surface_rule_graphs_args* args);

#ifdef __cplusplus
}
#endif
#endif /* ADAPTIGRAPH_AMD_H */
