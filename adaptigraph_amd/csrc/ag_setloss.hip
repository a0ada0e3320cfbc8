// Set losses of the training side (reference src/dynamics/gnn/loss.py: ChamferLoss :4-22, HausdorffLoss :63-82) over a BATCH of
// cloud pairs x (B,N,3), y (B,M,3), gfx950 only.  Both reduce over the whole batch - Chamfer is the mean of all B*N (B*M) nearest
// distances, Hausdorff the max of them - so a call is three kernels:
//   k_set_nn     one workgroup per graph, both clouds in LDS as SoA (the tiling of k_chamfer_nn, ag_cost.hip); threads stride over
//                the points.  For every x_i the nearest y_j and for every y_j the nearest x_i: dist = sqrt(dx*dx + dy*dy + dz*dz) in
//                fp32, every operation rounded on its own; the arg-min is the lowest index of the smallest distance.  Per graph:
//                both arg-min tables (int32) and four fp64 partials [sum of x-side minima, sum of y-side minima, largest x-side
//                minimum, largest y-side minimum] with the indices of the two maxima (lowest index among equals).
//   finaliser    one thread walks the B graphs in index order in fp64: chamfer = S_xy / (B_total N) + S_yx / (B_total M),
//                hausdorff = max x-side + max y-side with the winning (b, i) and (b, j), lowest (b, index) among equals.
//                k_set_final is the standalone form; k_step_loss_final also closes a training step's loss (MSE partials of
//                k_mse_part, the per-term table, the weighted fp32 sum in list order, train.py:100-102).
//                The Earth-mover term (ag_emd.hip) joins both finalisers: the mean of its matched distances.
//   k_set_grad   one workgroup per graph, the y arg-min table in LDS: the thread of x_i takes its own nearest y, then walks the
//                table for the j whose arg-min is i, in ascending j.  Hausdorff: only the two winning pairs.  The norm's gradient
//                at zero distance is zero (torch).  Every x_i has one writer: no atomics, repeated runs give the same bits.
// A NaN distance wins a min and a max, as in torch.min / torch.max, so a diverged prediction gives a NaN loss; its pull is NaN too
// (set_pull, ag_common.h), so the gradient row of a NaN point is NaN and the rows of graphs without one keep their bits.
// Equal maxima: the Hausdorff winner is the lowest (b, index), and k_set_grad gives that one pair the whole weight.  torch.max()
// over the batch splits its gradient evenly among equal maxima instead (each of k tied rows gets 1/k).  Values and arg-min tables
// are torch's either way; the gradients differ only at exact ties, which need duplicated points.  Kept: one winner per side is
// what lets the backward read four ints instead of searching for ties (tests/test_set_loss_edges.py has the difference on record).
#include "ag_common.h"

namespace ag {

namespace {
constexpr int ST = 256;

// nearest point of the other cloud (SoA in LDS, on points, stride opad): lowest index of the smallest distance; a NaN distance
// is taken at its first occurrence and kept
__device__ __forceinline__ float set_nearest(const float* os, int opad, int on, float qx, float qy, float qz, int& arg) {
    float best = __builtin_inff();
    arg = 0;
    for (int i = 0; i < on; ++i) {
        const float d = set_dist(qx, qy, qz, os[i], os[opad + i], os[2 * opad + i]);
        if (d < best || (d != d && best == best)) { best = d; arg = i; }
    }
    return best;
}
// does (ov, oi) beat (v, i) as a maximum?  larger value, or the lower index of equal values; NaN beats every number
__device__ __forceinline__ bool max_beats(double ov, int oi, double v, int i) {
    if (ov != ov) return v == v || oi < i;
    return v == v && (ov > v || (ov == v && oi < i));
}
// fixed trees over the 256 threads: shuffles inside a wave, then thread 0 over the four waves in wave order
__device__ __forceinline__ double block_sum_f64(double v, double* sh) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    double r = 0.0;
    if (threadIdx.x == 0) r = ((sh[0] + sh[1]) + sh[2]) + sh[3];
    __syncthreads();
    return r;                                                   // valid in thread 0
}
__device__ __forceinline__ void block_argmax_f64(double& v, int& i, double* sh, int* shi) {
    for (int o = 32; o > 0; o >>= 1) {
        const double ov = __shfl_down(v, o); const int oi = __shfl_down(i, o);
        if (max_beats(ov, oi, v, i)) { v = ov; i = oi; }
    }
    if ((threadIdx.x & 63) == 0) { sh[threadIdx.x >> 6] = v; shi[threadIdx.x >> 6] = i; }
    __syncthreads();
    if (threadIdx.x == 0)
        for (int w = 1; w < ST / 64; ++w)
            if (max_beats(sh[w], shi[w], v, i)) { v = sh[w]; i = shi[w]; }
    __syncthreads();                                            // valid in thread 0
}

__global__ __launch_bounds__(ST) void k_set_nn(SetLossDev a) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    __shared__ double sh[ST / 64];
    __shared__ int shi[ST / 64];
    const int b = blockIdx.x, tid = threadIdx.x;
    float* xs = sm;                  // [3][N]
    float* ys = sm + 3 * a.N;        // [3][M]
    const float* xr = a.x + (long)b * a.x_bstride;
    const float* yr = a.y + (long)b * a.y_bstride;
    for (int i = tid; i < a.N; i += ST) { xs[i] = xr[3 * i]; xs[a.N + i] = xr[3 * i + 1]; xs[2 * a.N + i] = xr[3 * i + 2]; }
    for (int j = tid; j < a.M; j += ST) { ys[j] = yr[3 * j]; ys[a.M + j] = yr[3 * j + 1]; ys[2 * a.M + j] = yr[3 * j + 2]; }
    __syncthreads();
    int* nnx = a.nn + (long)b * (a.N + a.M);
    int* nny = nnx + a.N;
    double sx = 0.0, sy = 0.0, mx = -1.0, my = -1.0;          // distances are >= 0: -1 loses to every point
    int ix = 0x7fffffff, iy = 0x7fffffff;
    // one stride over the N + M points of both clouds, so that small clouds (N + M <= 256) search both directions at once
    for (int p = tid; p < a.N + a.M; p += ST) {
        int arg;
        if (p < a.N) {
            const int i = p;
            const double d = (double)set_nearest(ys, a.M, a.M, xs[i], xs[a.N + i], xs[2 * a.N + i], arg);
            nnx[i] = arg;
            sx += d;
            if (max_beats(d, i, mx, ix)) { mx = d; ix = i; }
        } else {
            const int j = p - a.N;
            const double d = (double)set_nearest(xs, a.N, a.N, ys[j], ys[a.M + j], ys[2 * a.M + j], arg);
            nny[j] = arg;
            sy += d;
            if (max_beats(d, j, my, iy)) { my = d; iy = j; }
        }
    }
    const double tsx = block_sum_f64(sx, sh), tsy = block_sum_f64(sy, sh);
    block_argmax_f64(mx, ix, sh, shi);
    block_argmax_f64(my, iy, sh, shi);
    if (tid == 0) {
        double* p = a.part + (long)b * 4;
        p[0] = tsx; p[1] = tsy; p[2] = mx; p[3] = my;
        a.pidx[2 * b] = ix; a.pidx[2 * b + 1] = iy;
    }
}

// the B graphs in index order; win = {b of the x-side winner, its i, b of the y-side winner, its j}
__device__ inline void set_reduce(const double* part, const int* pidx, int B, int N, int M, int B_total, double& chamfer,
                                  double& hausdorff, int (&win)[4]) {
    double sx = 0.0, sy = 0.0, mx = part[2], my = part[3];
    win[0] = 0; win[1] = pidx[0]; win[2] = 0; win[3] = pidx[1];
    for (int b = 0; b < B; ++b) {
        sx += part[4 * b]; sy += part[4 * b + 1];
        // a later graph wins only with a strictly larger value (or the first NaN): the lowest (b, index) among equals stays
        const double vx = part[4 * b + 2], vy = part[4 * b + 3];
        if (b > 0 && (vx > mx || (vx != vx && mx == mx))) { mx = vx; win[0] = b; win[1] = pidx[2 * b]; }
        if (b > 0 && (vy > my || (vy != vy && my == my))) { my = vy; win[2] = b; win[3] = pidx[2 * b + 1]; }
    }
    chamfer = sx / ((double)B_total * N) + sy / ((double)B_total * M);
    hausdorff = mx + my;
}

// the Earth-mover term: the B partials of k_emd_assign in index order, over the B_total * K matched pairs of the whole batch
// (torch.mean over the (B, K) matched norms, loss.py:54).  A failed graph's partial is NaN, and so is the term
__device__ inline double emd_reduce(const double* part, int B, int K, int B_total) {
    double s = 0.0;
    for (int b = 0; b < B; ++b) s += part[b];
    return s / ((double)B_total * K);
}

__global__ void k_set_final(const double* part, const int* pidx, const double* emd_part, int B, int N, int M, int B_total, int kind,
                            float* out, int* win_out) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    if (kind == SET_LOSS_EMD) { out[0] = (float)emd_reduce(emd_part, B, N < M ? N : M, B_total); return; }
    double ch, hd; int win[4];
    set_reduce(part, pidx, B, N, M, B_total, ch, hd, win);
    out[0] = (float)(kind == SET_LOSS_CHAMFER ? ch : hd);
    for (int k = 0; k < 4; ++k) win_out[k] = win[k];
}

__global__ void k_step_loss_final(StepLossDev a) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    double mse = 0.0, ch = 0.0, hd = 0.0, em = 0.0;
    if (a.mse_part) {
        for (int k = 0; k < a.n_mse_part; ++k) mse += a.mse_part[k];
        mse = mse / (double)a.mse_n;
    }
    if (a.set_part) {
        int win[4];
        set_reduce(a.set_part, a.set_idx, a.B, a.n_p, a.n_p, a.B_total, ch, hd, win);
        for (int k = 0; k < 4; ++k) a.win[k] = win[k];
    }
    if (a.emd_part) em = emd_reduce(a.emd_part, a.B, a.n_p, a.B_total);
    // every term is this call's share of a mean (or, Hausdorff, the whole batch's max: never in parts); an earlier part's share
    // joins in fp64 before the one rounding.  The step's loss is then the fp32 sum of weight * term in list order
    float l = 0.f;
    for (int k = 0; k < a.n_terms; ++k) {
        double v = a.kind[k] == SET_LOSS_MSE ? mse : a.kind[k] == SET_LOSS_CHAMFER ? ch : a.kind[k] == SET_LOSS_HAUSDORFF ? hd : em;
        float* t = a.terms + (long)a.fi * a.n_terms + k;
        if (a.accumulate) v += (double)*t;
        *t = (float)v;
        l = l + a.weight[k] * *t;
    }
    a.loss[a.fi] = l;
    if (a.fi == a.n_future - 1) {
        float s = 0.f;
        for (int k = 0; k < a.n_future; ++k) s += a.loss[k];
        a.loss[a.n_future] = s;
    }
}

__global__ __launch_bounds__(ST) void k_set_grad(SetLossDev a, SetGradDev g) {
    extern __shared__ int tab[];     // [M] arg-min of every y_j
    const int b = blockIdx.x, tid = threadIdx.x;
    const int* nnx = a.nn + (long)b * (a.N + a.M);
    const int* nny = nnx + a.N;
    for (int j = tid; j < a.M; j += ST) tab[j] = nny[j];
    __syncthreads();
    const float go = g.gout ? g.gout[0] : 1.f;
    const float* xr = a.x + (long)b * a.x_bstride;
    const float* yr = a.y + (long)b * a.y_bstride;
    float* gr = g.gx + (long)b * a.N * 3;
    // chamfer: the means' 1 / (B_total N) and 1 / (B_total M); hausdorff: the two winners take the whole weight
    const float cx = (float)((double)go * g.w_chamfer / ((double)g.B_total * a.N));
    const float cy = (float)((double)go * g.w_chamfer / ((double)g.B_total * a.M));
    const float wh = go * g.w_hausdorff;
    const bool ch = g.w_chamfer != 0.f, hd = g.w_hausdorff != 0.f;
    const int wbx = hd ? g.win[0] : -1, wi = hd ? g.win[1] : -1, wby = hd ? g.win[2] : -1, wj = hd ? clampi(g.win[3], a.M) : -1;
    for (int i = tid; i < a.N; i += ST) {
        const float* xi = xr + 3 * i;
        float v[3] = {0.f, 0.f, 0.f};
        const float* y0 = yr + 3 * clampi(nnx[i], a.M);
        if (ch) {
            set_pull(xi, y0, cx, v);
            for (int j = 0; j < a.M; ++j)
                if (tab[j] == i) set_pull(xi, yr + 3 * j, cy, v);
        }
        if (b == wbx && i == wi) set_pull(xi, y0, wh, v);
        if (b == wby && tab[wj] == i) set_pull(xi, yr + 3 * wj, wh, v);
        if (g.add) { gr[3 * i] += v[0]; gr[3 * i + 1] += v[1]; gr[3 * i + 2] += v[2]; }
        else { gr[3 * i] = v[0]; gr[3 * i + 1] = v[1]; gr[3 * i + 2] = v[2]; }
    }
}
}  // namespace

size_t set_loss_part_doubles(int B) { return (size_t)B * 4; }
size_t set_loss_part_ints(int B) { return (size_t)B * 2; }

hipError_t launch_set_nn(const SetLossDev& a, hipStream_t st) {
    const size_t lds = (size_t)3 * ((size_t)a.N + a.M) * 4;
    static unsigned long long attr_devices = 0;              // per-device function attribute (see launch_chamfer)
    int dev_id = 0;
    if (hipGetDevice(&dev_id) != hipSuccess) dev_id = 0;
    if (dev_id >= 64 || !(attr_devices >> dev_id & 1ull)) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(k_set_nn), hipFuncAttributeMaxDynamicSharedMemorySize,
                                           160 * 1024 - 2048);
        if (e != hipSuccess) return e;
        if (dev_id < 64) attr_devices |= 1ull << dev_id;
    }
    hipLaunchKernelGGL(k_set_nn, dim3(a.B), dim3(ST), lds, st, a);
    return hipGetLastError();
}
hipError_t launch_set_final(const SetLossDev& a, const double* emd_part, int B_total, int kind, float* out, int* win, hipStream_t st) {
    hipLaunchKernelGGL(k_set_final, dim3(1), dim3(64), 0, st, (const double*)a.part, (const int*)a.pidx, emd_part, a.B, a.N, a.M, B_total, kind,
                       out, win);
    return hipGetLastError();
}
hipError_t launch_step_loss_final(const StepLossDev& a, hipStream_t st) {
    hipLaunchKernelGGL(k_step_loss_final, dim3(1), dim3(64), 0, st, a);
    return hipGetLastError();
}
hipError_t launch_set_grad(const SetLossDev& a, const SetGradDev& g, hipStream_t st) {
    hipLaunchKernelGGL(k_set_grad, dim3(a.B), dim3(ST), (size_t)a.M * 4, st, a, g);
    return hipGetLastError();
}

}  // namespace ag
