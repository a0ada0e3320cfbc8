// The device-resident physics-parameter fit's launch arguments (ag_ppm.hip).  Internal, not part of the C-ABI.
#pragma once
#include "ag_common.h"

namespace ag {

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

}  // namespace ag
