// Open-loop eval rollout, the step between two forwards (reference src/dynamics/rollout/rollout.py:116-171, 224-233) for B
// rollouts per launch.  gfx950 only.
//
//   k_eval_advance   one workgroup per graph: the ground-truth error of the step's prediction, then - for a graph that goes on -
//                    the next model input (history shift, predicted rows + tool rows of the next frame pair, action) and the
//                    particle mask the edge builder reads for it (all zero for a graph that ended: it builds an empty graph)
//
// Error (rollout.py:116-147): mean over the n_obj sampled rows of the Euclidean distance between the prediction and the frame's
// point the row was sampled from.  fp32 inputs, everything else in fp64: a thread sums its rows in ascending order, the 64 lanes
// of a wave are summed by an xor butterfly (offsets 32, 16, ..., 1: every lane ends with the same sum), the four wave sums are added
// in wave order from LDS, one division, one rounding to fp32.  No atomics; the order depends on n_obj alone, so a graph's error
// does not depend on its neighbours in the launch.  Plain arithmetic only: a NaN in a sampled row of the prediction gives NaN.
#include "../../include/adaptigraph_amd.h"
#include "ag_common.h"

namespace ag {

constexpr int EW = 256;                 // threads per workgroup: 4 wavefronts
constexpr int EWAVES = EW / 64;

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

__device__ __forceinline__ long long clamp_ll(long long v, long long hi) { return v < 0 ? 0 : v > hi ? hi : v; }

__global__ __launch_bounds__(EW) void k_eval_advance(ag_eval_step_args a, int nh, unsigned char* mask_next) {
    __shared__ double wsum[EWAVES];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int No = a.max_nobj, Ne = a.n_eef, N = No + Ne;
    const int64_t* m = a.d_frames + (long)b * 3;
    const float* pred = a.d_pred + (long)b * No * 3;
    // (the host built the table from validated frames; the clamps keep a wrong entry inside the two flat buffers)
    const long long gt0 = clamp_ll(m[0], a.obj_points - 1);
    const int n_obj = min(max(a.d_n_obj[b], 0), No);
    double acc = 0.0;
    for (int n = tid; n < n_obj; n += EW) {
        const long long src = clamp_ll(gt0 + max(a.d_fps_idx[(long)b * No + n], 0), a.obj_points - 1);
        const float* g = a.d_obj_pos + src * 3;
        const float* p = pred + (long)n * 3;
        const double dx = (double)p[0] - (double)g[0], dy = (double)p[1] - (double)g[1], dz = (double)p[2] - (double)g[2];
        acc += sqrt((dx * dx + dy * dy) + dz * dz);
    }
    acc = wave_sum_f64(acc);
    if ((tid & 63) == 0) wsum[tid >> 6] = acc;
    __syncthreads();
    if (tid == 0) {
        double s = wsum[0];
#pragma unroll
        for (int k = 1; k < EWAVES; ++k) s += wsum[k];
        a.d_err[(long)a.step * a.err_stride + b] = (float)(s / (double)n_obj);       // n_obj == 0: NaN, numpy's mean of nothing
    }
    // ---- the next model input (rollout.py:163-171, 224-233)
    const bool on = m[1] >= 0;
    for (int i = tid; i < N; i += EW) mask_next[(long)b * N + i] = on ? a.d_state_mask[(long)b * N + i] : 0;
    if (!on) return;
    const long long es = clamp_ll(m[1], a.eef_points - Ne), ee = clamp_ll(m[2], a.eef_points - Ne);
    const float* s = a.d_state + (long)b * nh * N * 3;
    float* o = a.d_state_next + (long)b * nh * N * 3;
    float* act = a.d_action_next + (long)b * N * 3;
    const long fr = (long)N * 3;
    for (int i = tid; i < N * 3; i += EW) {
        const int r = i / 3, c = i % 3;
        for (int t = 0; t < nh - 1; ++t) o[t * fr + i] = s[((a.store_rest_state && t == 0) ? 0 : t + 1) * fr + i];
        float last, d = 0.f;
        if (r < No) {
            last = pred[i];                                                          // every row, padded ones included
        } else {
            const float e0 = a.d_eef_pos[(es + (r - No)) * 3 + c], e1 = a.d_eef_pos[(ee + (r - No)) * 3 + c];
            last = e0;
            d = __fsub_rn(e1, e0);
        }
        o[(nh - 1) * fr + i] = last;
        act[i] = d;
    }
}

hipError_t launch_eval_advance(const ag_eval_step_args& a, int n_his, unsigned char* mask_next, hipStream_t st) {
    hipLaunchKernelGGL(k_eval_advance, dim3(a.B), dim3(EW), 0, st, a, n_his, mask_next);
    return hipGetLastError();
}

}  // namespace ag
