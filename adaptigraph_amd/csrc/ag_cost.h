// The planner's cost kernels (ag_cost.hip) and MPPI sampling / update (ag_mppi.hip).  Internal, not part of the C-ABI.
#pragma once
#include "ag_common.h"

namespace ag {

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

}  // namespace ag
