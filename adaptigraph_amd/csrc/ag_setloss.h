// The set losses of the training side (ag_setloss.hip, ag_emd.hip) with the device helpers the two files share.  Internal, not part
// of the C-ABI.
#pragma once
#include "ag_dist.h"

namespace ag {

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
    return __fsqrt_rn(dist_exact(ax, ay, az, bx, by, bz));
}
// g += s * d||x_i - y_j|| / dx_i; zero at zero distance and at no other: a NaN distance gives a NaN row, as torch's norm does
// (the test was !(dist > 0), which a NaN passes: the row of a diverged point came out as 0, the one number that hides it)
__device__ __forceinline__ void set_pull(const float* xi, const float* yj, float s, float (&g)[3]) {
    const float dx = __fsub_rn(xi[0], yj[0]), dy = __fsub_rn(xi[1], yj[1]), dz = __fsub_rn(xi[2], yj[2]);
    const float dist = __fsqrt_rn(dist_exact(xi[0], xi[1], xi[2], yj[0], yj[1], yj[2]));
    if (dist == 0.f) return;
    const float q = s / dist;
    g[0] += dx * q; g[1] += dy * q; g[2] += dz * q;
}
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

}  // namespace ag
