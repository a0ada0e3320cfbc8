// The training side: the backward pass (ag_train.hip), Adam and the glue of the chained step (ag_optim.hip).  Internal, not part
// of the C-ABI.
#pragma once
#include "ag_common.h"

namespace ag {

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

// ---- device-resident training step (ag_optim.hip; the weight packers that go with it: ag_model.h).
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

}  // namespace ag
