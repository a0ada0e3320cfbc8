// Device-resident physics-parameter fit (ag_ppm_grad_step, ag_ppm_adam_step): what lives between the edge builder, the model
// forwards (enqueue_forward) and the backward chunks (train_backward_chunk) of one masked rollout toward the physics parameter
// (reference src/planning/forward_dynamics.py:209-399, physics_param_optimizer.py:178-226), gfx950 only.
//   * the model inputs of step 1 from the padded start clouds; per step the capture of the prediction, the tool keypoints at the
//     masked mean height of the prediction and the history shift, each step's input kept for the backward
//   * dLoss/dpred of a step: chamfer gradient where the row is captured, what the next step's dLoss/dstate says about the object
//     rows of its last frame, and the mean-y path from its tool rows
//   * the per-start reduction of error and gradient, history, best-so-far and Adam in double, in one small launch
// No float atomics; every sum has a fixed order that does not depend on which other rows share the call.
#include "ag_ppm.h"

namespace ag {
namespace {

constexpr int RT = 256;

// fixed-order block sum: thread t holds the sum of its strided elements, then a binary tree over the 256 partials
__device__ inline double block_sum(double s, double* sh) {
    sh[threadIdx.x] = s;
    __syncthreads();
    for (int w = RT / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) sh[threadIdx.x] += sh[threadIdx.x + w];
        __syncthreads();
    }
    const double r = sh[0];
    __syncthreads();
    return r;
}

// forward_dynamics.py:233 / :360: mean y of the valid object particles, summed in fp64 and rounded once.  One workgroup per row.
__global__ __launch_bounds__(RT) void k_ppm_mean_y(const float* pos, const uint8_t* obj_mask, int N_o, float* ymean, int* cnt) {
    __shared__ double sh[RT];
    const int b = blockIdx.x;
    const float* p = pos + (long)b * N_o * 3;
    const uint8_t* m = obj_mask + (long)b * N_o;
    double s = 0.0, c = 0.0;
    for (int i = threadIdx.x; i < N_o; i += RT)
        if (m[i]) { s += (double)p[3 * i + 1]; c += 1.0; }
    s = block_sum(s, sh);
    c = block_sum(c, sh);
    if (threadIdx.x == 0) { ymean[b] = (float)(s / c); cnt[b] = (int)c; }
}

__device__ inline float tool_y(const PpmBufs& a, int b) { return a.grip_on ? a.ymean[b] + a.grip : a.ymean[b]; }

// forward_dynamics.py:225-309: states, attrs, action, p_instance, physics parameter and the two masks of the edge builder
__global__ void k_ppm_init(PpmBufs a, float* state1) {
    const int N = a.N_o + a.M;
    const long r = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= (long)a.B * N) return;
    const int b = (int)(r / N), i = (int)(r % N);
    float p[3], act[3] = {0.f, 0.f, 0.f};
    if (i < a.N_o) {
        const float* s = a.state0 + ((long)b * a.N_o + i) * 3;
        p[0] = s[0]; p[1] = s[1]; p[2] = s[2];
        const int valid = a.obj_mask[(long)b * a.N_o + i] ? 1 : 0;
        a.attrs[r * 2] = (float)valid; a.attrs[r * 2 + 1] = 0.f;
        a.group[r] = i < a.cnt[b] ? 1.f : 0.f;                      // one instance: a prefix of the row (:292-300)
        a.physN[r] = a.phys[(long)b * a.N_o + i];
        a.mask[r] = (uint8_t)valid; a.tool[r] = 0;
    } else {
        const int m = i - a.N_o;
        const float* xz = a.eef_xz + ((long)b * a.M + m) * 2;
        const float* d = a.eef_delta + ((long)b * a.M + m) * 3;
        p[0] = xz[0]; p[1] = tool_y(a, b); p[2] = xz[1];
        act[0] = d[0]; act[1] = d[1]; act[2] = d[2];
        a.attrs[r * 2] = 0.f; a.attrs[r * 2 + 1] = 1.f;
        a.group[r] = 0.f; a.physN[r] = 0.f;
        a.mask[r] = 1; a.tool[r] = 1;
    }
    for (int c = 0; c < 3; ++c) {
        a.action[r * 3 + c] = act[c];
        for (int t = 0; t < a.n_his; ++t) state1[(((long)b * a.n_his + t) * N + i) * 3 + c] = p[c];
    }
}

// :356-372 for rows [0,L): capture, and for rows [0,Ln) the next model input
__global__ void k_ppm_advance(PpmBufs a, const float* state, const float* pred, int s, int L, int Ln, float* state_next, float* seqs) {
    const int N = a.N_o + a.M;
    const long r = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= (long)L * N) return;
    const int b = (int)(r / N), i = (int)(r % N);
    const float* pr = pred + ((long)b * a.N_o + i) * 3;
    if (i < a.N_o && a.repeat[b] == s) {
        float* o = seqs + ((long)b * a.N_o + i) * 3;
        o[0] = pr[0]; o[1] = pr[1]; o[2] = pr[2];
    }
    if (b >= Ln) return;
    const float* in = state + (long)b * a.n_his * N * 3;
    float* out = state_next + (long)b * a.n_his * N * 3;
    for (int t = 0; t < a.n_his - 1; ++t)
        for (int c = 0; c < 3; ++c) out[((long)t * N + i) * 3 + c] = in[((long)(t + 1) * N + i) * 3 + c];
    float* o = out + ((long)(a.n_his - 1) * N + i) * 3;
    if (i < a.N_o) { o[0] = pr[0]; o[1] = pr[1]; o[2] = pr[2]; }
    else {
        const float* last = in + ((long)(a.n_his - 1) * N + i) * 3;
        const float* d = a.eef_delta + ((long)b * a.M + (i - a.N_o)) * 3;
        o[0] = last[0] + d[0]; o[1] = tool_y(a, b); o[2] = last[2] + d[2];
    }
}

__global__ void k_ppm_pred_grad(PpmBufs a, const float* gseq, const float* dnext, int s, int L, int Ln, float* dpos) {
    const int N = a.N_o + a.M;
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long row = (long)a.N_o * 3;
    if (i >= (long)L * row) return;
    const int b = (int)(i / row); const int q = (int)(i % row), n = q / 3, c = q % 3;
    float v = a.repeat[b] == s ? gseq[i] : 0.f;
    if (dnext && b < Ln) {
        const float* dl = dnext + (((long)b * a.n_his + (a.n_his - 1)) * N) * 3;
        v += dl[q];
        if (c == 1 && a.obj_mask[(long)b * a.N_o + n]) {
            float t = 0.f;
            for (int m = 0; m < a.M; ++m) t += dl[(long)(a.N_o + m) * 3 + 1];
            v += (float)((double)t / (double)a.cnt[b]);
        }
    }
    dpos[i] = v;
}

__global__ void k_ppm_accum(const float* gphys, int L, int N, int N_o, float* grad) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long)L * N_o) return;
    const long b = i / N_o; const int n = (int)(i % N_o);
    grad[i] += gphys[b * N + n];
}

__device__ inline long ppm_row(const PpmAdamArgs& a, int k, int i) { return a.start_major ? (long)k * a.n + i : (long)i * a.K + k; }

// One workgroup.  Per start, in start order: error = mean of its rows' errors, gradient = sum over its rows and particles, both
// in fp64 in an order that depends on the start's own rows only.  Then history, best-so-far, Adam (physics_param_optimizer
// optimize_grad's loop body) and the new per-particle parameter.
__global__ __launch_bounds__(RT) void k_ppm_adam(PpmAdamArgs a) {
    __shared__ double sh[RT];
    __shared__ int s_it;
    if (a.status[0] != 0) return;
    if (threadIdx.x == 0) s_it = a.status[1];
    __syncthreads();
    const int it = s_it;
    const long per = (long)a.n * a.N_o;
    for (int k = 0; k < a.K; ++k) {
        double e = 0.0, g = 0.0;
        if (threadIdx.x == 0) {
            for (int i = 0; i < a.n; ++i) e += (double)a.err[ppm_row(a, k, i)];
            e /= (double)a.n;
        }
        if (a.grad)
            for (long j = threadIdx.x; j < per; j += RT) g += (double)a.grad[ppm_row(a, k, (int)(j / a.N_o)) * a.N_o + j % a.N_o];
        g = block_sum(g, sh);
        if (threadIdx.x == 0) {
            const float xe = a.x[k];
            if (a.grad) a.gk[k] = g;                       // an evaluation without a gradient leaves the last step's
            if (it < a.hist_cap) { a.hist_x[(long)it * a.K + k] = xe; a.hist_e[(long)it * a.K + k] = e; }
            if (e < a.best[0]) { a.best[0] = e; a.best[1] = (double)xe; a.best[2] = (double)k; }   // ascending k: the first minimum wins
            if (it == 0 && k == 0) a.best[3] = e;
            if (a.apply) {
                const double m = 0.9 * a.m[k] + 0.1 * g;
                const double v = 0.999 * a.v[k] + 0.001 * g * g;
                const double step = a.lr * (m / a.bc1) / (sqrt(v / a.bc2) + 1e-8);
                double x = (double)xe - step;
                x = x < a.lo ? a.lo : (x > a.hi ? a.hi : x);
                a.m[k] = m; a.v[k] = v; a.x[k] = (float)x;
            }
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) { a.status[1] = it + 1; if (a.apply) a.status[2] += 1; }
    if (!a.apply) return;
    const long R = (long)a.K * a.n;
    for (long j = threadIdx.x; j < R * a.N_o; j += RT) {
        const long r = j / a.N_o;
        a.phys[j] = a.x[a.start_major ? r / a.n : r % a.K];
    }
}

inline unsigned blocks(long n) { return (unsigned)((n + 255) / 256); }
}  // namespace

hipError_t launch_ppm_mean_y(const PpmBufs& b, const float* pos, int L, hipStream_t st) {
    if (L <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_ppm_mean_y, dim3(L), dim3(RT), 0, st, pos, b.obj_mask, b.N_o, b.ymean, b.cnt);
    return hipGetLastError();
}
hipError_t launch_ppm_init(const PpmBufs& b, float* state1, hipStream_t st) {
    hipLaunchKernelGGL(k_ppm_init, dim3(blocks((long)b.B * (b.N_o + b.M))), dim3(256), 0, st, b, state1);
    return hipGetLastError();
}
hipError_t launch_ppm_advance(const PpmBufs& b, const float* state, const float* pred, int s, int L, int Ln, float* state_next,
                              float* seqs, hipStream_t st) {
    if (L <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_ppm_advance, dim3(blocks((long)L * (b.N_o + b.M))), dim3(256), 0, st, b, state, pred, s, L, Ln, state_next, seqs);
    return hipGetLastError();
}
hipError_t launch_ppm_pred_grad(const PpmBufs& b, const float* gseq, const float* dnext, int s, int L, int Ln, float* dpos,
                                hipStream_t st) {
    if (L <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_ppm_pred_grad, dim3(blocks((long)L * b.N_o * 3)), dim3(256), 0, st, b, gseq, dnext, s, L, Ln, dpos);
    return hipGetLastError();
}
hipError_t launch_ppm_accum(const float* gphys, int L, int N, int N_o, float* grad, hipStream_t st) {
    if (L <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_ppm_accum, dim3(blocks((long)L * N_o)), dim3(256), 0, st, gphys, L, N, N_o, grad);
    return hipGetLastError();
}
hipError_t launch_ppm_adam(const PpmAdamArgs& a, hipStream_t st) {
    hipLaunchKernelGGL(k_ppm_adam, dim3(1), dim3(RT), 0, st, a);
    return hipGetLastError();
}

}  // namespace ag
