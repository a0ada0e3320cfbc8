// Kernel families (profiling ids) and the per-context switches.  Internal, not part of the C-ABI.
#pragma once

namespace ag {

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

}  // namespace ag
