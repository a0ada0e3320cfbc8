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
// (set_pull, ag_setloss.h), so the gradient row of a NaN point is NaN and the rows of graphs without one keep their bits.
// Equal maxima: the Hausdorff winner is the lowest (b, index), and k_set_grad gives that one pair the whole weight.  torch.max()
// over the batch splits its gradient evenly among equal maxima instead (each of k tied rows gets 1/k).  Values and arg-min tables
// are torch's either way; the gradients differ only at exact ties, which need duplicated points.  Kept: one winner per side is
// what lets the backward read four ints instead of searching for ties (tests/test_set_loss_edges.py has the difference on record).
// REAL ROWS (AG_LOSS_ROWS, template <bool ROWS>): on a padded batch graph b's clouds are the prefixes x[b, :nx_b], y[b, :ny_b], the
// counts clamped into range where they are read (set_rows_of, ag_setloss.h) and a graph with an empty side wholly empty.  Only real
// rows are loaded, strided over and searched; chamfer = (1 / B_total) sum_b [sx_b / nx_b + sy_b / ny_b] - the mean over graphs of
// each graph's own Chamfer distance -, hausdorff = the max over the real rows of every graph (an empty graph has no candidate; none
// at all: 0, winners -1); gradient rows behind nx_b are exact zeros.  ROWS = false is the code the plain kinds always had.
#include "ag_setloss.h"
#include "ag_lds_optin.h"

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

// ROWS: graph b's clouds are the prefixes x[b, :nx] and y[b, :ny] (set_rows_of); only they are loaded, strided over and searched.
// The partials are then the graph's own means sx / nx and sy / ny (0 for an empty graph), the max partials stay at the sentinel -1
// for an empty graph, and the arg-min entries of padding rows are written as 0.
template <bool ROWS>
__global__ __launch_bounds__(ST) void k_set_nn(SetLossDev a, SetRows r) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    __shared__ double sh[ST / 64];
    __shared__ int shi[ST / 64];
    const int b = blockIdx.x, tid = threadIdx.x;
    int nx = a.N, ny = a.M;
    if constexpr (ROWS) set_rows_of(r, b, a.N, a.M, nx, ny);
    float* xs = sm;                  // [3][N]
    float* ys = sm + 3 * a.N;        // [3][M]
    const float* xr = a.x + (long)b * a.x_bstride;
    const float* yr = a.y + (long)b * a.y_bstride;
    for (int i = tid; i < nx; i += ST) { xs[i] = xr[3 * i]; xs[a.N + i] = xr[3 * i + 1]; xs[2 * a.N + i] = xr[3 * i + 2]; }
    for (int j = tid; j < ny; j += ST) { ys[j] = yr[3 * j]; ys[a.M + j] = yr[3 * j + 1]; ys[2 * a.M + j] = yr[3 * j + 2]; }
    __syncthreads();
    int* nnx = a.nn + (long)b * (a.N + a.M);
    int* nny = nnx + a.N;
    double sx = 0.0, sy = 0.0, mx = -1.0, my = -1.0;          // distances are >= 0: -1 loses to every point
    int ix = 0x7fffffff, iy = 0x7fffffff;
    // one stride over the N + M points of both clouds, so that small clouds (N + M <= 256) search both directions at once
    for (int p = tid; p < nx + ny; p += ST) {
        int arg;
        if (p < nx) {
            const int i = p;
            const double d = (double)set_nearest(ys, a.M, ny, xs[i], xs[a.N + i], xs[2 * a.N + i], arg);
            nnx[i] = arg;
            sx += d;
            if (max_beats(d, i, mx, ix)) { mx = d; ix = i; }
        } else {
            const int j = p - nx;
            const double d = (double)set_nearest(xs, a.N, nx, ys[j], ys[a.M + j], ys[2 * a.M + j], arg);
            nny[j] = arg;
            sy += d;
            if (max_beats(d, j, my, iy)) { my = d; iy = j; }
        }
    }
    if constexpr (ROWS) {
        for (int i = nx + tid; i < a.N; i += ST) nnx[i] = 0;
        for (int j = ny + tid; j < a.M; j += ST) nny[j] = 0;
    }
    const double tsx = block_sum_f64(sx, sh), tsy = block_sum_f64(sy, sh);
    block_argmax_f64(mx, ix, sh, shi);
    block_argmax_f64(my, iy, sh, shi);
    if (tid == 0) {
        double* p = a.part + (long)b * 4;
        if constexpr (ROWS) { p[0] = nx ? tsx / (double)nx : 0.0; p[1] = ny ? tsy / (double)ny : 0.0; }
        else { p[0] = tsx; p[1] = tsy; }
        p[2] = mx; p[3] = my;
        a.pidx[2 * b] = ix; a.pidx[2 * b + 1] = iy;
    }
}

// the B graphs in index order; win = {b of the x-side winner, its i, b of the y-side winner, its j}
template <bool ROWS>
__device__ inline void set_reduce(const double* part, const int* pidx, int B, int N, int M, int B_total, double& chamfer,
                                  double& hausdorff, int (&win)[4]) {
    if constexpr (ROWS) {
        // the per-graph means in index order, over the B_total graphs of the whole batch.  The Hausdorff walk starts at the
        // sentinel of "no candidate", which an empty graph's partial equals and therefore never beats: the first graph with a
        // real row takes over, then only a strictly larger value (or the first NaN).  No candidate at all: 0, winners -1
        double sx = 0.0, sy = 0.0, mx = -1.0, my = -1.0;
        win[0] = -1; win[1] = -1; win[2] = -1; win[3] = -1;
        for (int b = 0; b < B; ++b) {
            sx += part[4 * b]; sy += part[4 * b + 1];
            const double vx = part[4 * b + 2], vy = part[4 * b + 3];
            if (vx > mx || (vx != vx && mx == mx)) { mx = vx; win[0] = b; win[1] = pidx[2 * b]; }
            if (vy > my || (vy != vy && my == my)) { my = vy; win[2] = b; win[3] = pidx[2 * b + 1]; }
        }
        chamfer = sx / (double)B_total + sy / (double)B_total;
        hausdorff = (mx < 0.0 ? 0.0 : mx) + (my < 0.0 ? 0.0 : my);
        return;
    }
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
// (torch.mean over the (B, K) matched norms, loss.py:54).  A failed graph's partial is NaN, and so is the term.  ROWS: the
// partials are per-graph means over K_b pairs already, and the term their mean over the B_total graphs
template <bool ROWS>
__device__ inline double emd_reduce(const double* part, int B, int K, int B_total) {
    double s = 0.0;
    for (int b = 0; b < B; ++b) s += part[b];
    if constexpr (ROWS) return s / (double)B_total;
    return s / ((double)B_total * K);
}

// kind without the flag; ROWS = false is the finaliser the plain kinds always had
template <bool ROWS>
__global__ void k_set_final(const double* part, const int* pidx, const double* emd_part, int B, int N, int M, int B_total, int kind,
                            float* out, int* win_out) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    if (kind == SET_LOSS_EMD) { out[0] = (float)emd_reduce<ROWS>(emd_part, B, N < M ? N : M, B_total); return; }
    double ch, hd; int win[4];
    set_reduce<ROWS>(part, pidx, B, N, M, B_total, ch, hd, win);
    out[0] = (float)(kind == SET_LOSS_CHAMFER ? ch : hd);
    for (int k = 0; k < 4; ++k) win_out[k] = win[k];
}

// SROWS / EROWS: the flag of the Chamfer-and-Hausdorff pass and of the Earth-mover pass (one per pass: ag_train_step_losses checks
// it; launch_step_loss_final reads it off a.kind[]).  <false, false> is the finaliser a plain list always had
template <bool SROWS, bool EROWS>
__global__ void k_step_loss_final(StepLossDev a) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    double mse = 0.0, ch = 0.0, hd = 0.0, em = 0.0;
    if (a.mse_part) {
        for (int k = 0; k < a.n_mse_part; ++k) mse += a.mse_part[k];
        mse = mse / (double)a.mse_n;
    }
    if (a.set_part) {
        int win[4];
        set_reduce<SROWS>(a.set_part, a.set_idx, a.B, a.n_p, a.n_p, a.B_total, ch, hd, win);
        for (int k = 0; k < 4; ++k) a.win[k] = win[k];
    }
    if (a.emd_part) em = emd_reduce<EROWS>(a.emd_part, a.B, a.n_p, a.B_total);
    // every term is this call's share of a mean (or, Hausdorff, the whole batch's max: never in parts); an earlier part's share
    // joins in fp64 before the one rounding.  The step's loss is then the fp32 sum of weight * term in list order
    float l = 0.f;
    for (int k = 0; k < a.n_terms; ++k) {
        const int kind = (SROWS || EROWS) ? a.kind[k] & ~SET_LOSS_ROWS : a.kind[k];
        double v = kind == SET_LOSS_MSE ? mse : kind == SET_LOSS_CHAMFER ? ch : kind == SET_LOSS_HAUSDORFF ? hd : em;
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

// ROWS: the scales are the graph's own, 1 / (B_total nx) and 1 / (B_total ny); the y-table walk covers the real y rows; padding
// rows of x get exact zeros (added to the chain's dpos they leave it as it is)
template <bool ROWS>
__global__ __launch_bounds__(ST) void k_set_grad(SetLossDev a, SetRows r, SetGradDev g) {
    extern __shared__ int tab[];     // [M] arg-min of every y_j
    const int b = blockIdx.x, tid = threadIdx.x;
    int nx = a.N, ny = a.M;
    if constexpr (ROWS) set_rows_of(r, b, a.N, a.M, nx, ny);
    const int* nnx = a.nn + (long)b * (a.N + a.M);
    const int* nny = nnx + a.N;
    for (int j = tid; j < ny; j += ST) tab[j] = nny[j];
    __syncthreads();
    const float go = g.gout ? g.gout[0] : 1.f;
    const float* xr = a.x + (long)b * a.x_bstride;
    const float* yr = a.y + (long)b * a.y_bstride;
    float* gr = g.gx + (long)b * a.N * 3;
    // chamfer: the means' 1 / (B_total N) and 1 / (B_total M); hausdorff: the two winners take the whole weight
    const int ycl = ROWS ? (ny > 0 ? ny : 1) : a.M;             // what a y index is clamped to (an empty graph reads no table)
    const float cx = (float)((double)go * g.w_chamfer / ((double)g.B_total * (ROWS ? (nx > 0 ? nx : 1) : a.N)));
    const float cy = (float)((double)go * g.w_chamfer / ((double)g.B_total * ycl));
    const float wh = go * g.w_hausdorff;
    const bool ch = g.w_chamfer != 0.f, hd = g.w_hausdorff != 0.f;
    const int wbx = hd ? g.win[0] : -1, wi = hd ? g.win[1] : -1, wby = hd ? g.win[2] : -1, wj = hd ? clampi(g.win[3], ycl) : -1;
    for (int i = tid; i < a.N; i += ST) {
        float v[3] = {0.f, 0.f, 0.f};
        if (!ROWS || i < nx) {
            const float* xi = xr + 3 * i;
            const float* y0 = yr + 3 * clampi(nnx[i], ycl);
            if (ch) {
                set_pull(xi, y0, cx, v);
                for (int j = 0; j < ny; ++j)
                    if (tab[j] == i) set_pull(xi, yr + 3 * j, cy, v);
            }
            if (b == wbx && i == wi) set_pull(xi, y0, wh, v);
            if (b == wby && tab[wj] == i) set_pull(xi, yr + 3 * wj, wh, v);
        }
        if (g.add) { gr[3 * i] += v[0]; gr[3 * i + 1] += v[1]; gr[3 * i + 2] += v[2]; }
        else { gr[3 * i] = v[0]; gr[3 * i + 1] = v[1]; gr[3 * i + 2] = v[2]; }
    }
}

// the live prefix of a padded training batch: one workgroup per graph, the lowest i with attrs[b, i, 0] <= 0
__global__ __launch_bounds__(ST) void k_prefix_rows(const float* attrs, int N, int n_p, int* n) {
    __shared__ int sh[ST / 64];
    const int b = blockIdx.x, tid = threadIdx.x;
    int first = n_p;
    for (int i = tid; i < n_p; i += ST)
        if (attrs[((long)b * N + i) * 2] <= 0.f) { first = i; break; }     // a thread's rows ascend: its first hit is its lowest
    for (int o = 32; o > 0; o >>= 1) { const int ov = __shfl_down(first, o); first = ov < first ? ov : first; }
    if ((tid & 63) == 0) sh[tid >> 6] = first;
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < ST / 64; ++w) first = sh[w] < first ? sh[w] : first;
        n[b] = first;
    }
}
}  // namespace

size_t set_loss_part_doubles(int B) { return (size_t)B * 4; }
size_t set_loss_part_ints(int B) { return (size_t)B * 2; }

hipError_t launch_set_nn(const SetLossDev& a, const SetRows& rows, hipStream_t st) {
    const size_t lds = (size_t)3 * ((size_t)a.N + a.M) * 4;
    static std::atomic<unsigned long long> done{0};          // the dynamic-LDS opt-in, per device (ag_lds_optin.h)
    if (hipError_t e = lds_opt_in(done, 160 * 1024 - 2048, k_set_nn<false>, k_set_nn<true>); e != hipSuccess) return e;
    if (rows.nx) hipLaunchKernelGGL(k_set_nn<true>, dim3(a.B), dim3(ST), lds, st, a, rows);
    else hipLaunchKernelGGL(k_set_nn<false>, dim3(a.B), dim3(ST), lds, st, a, rows);
    return hipGetLastError();
}
hipError_t launch_set_final(const SetLossDev& a, const double* emd_part, int B_total, int kind, float* out, int* win, hipStream_t st) {
    const int base = kind & ~SET_LOSS_ROWS;
    if (kind & SET_LOSS_ROWS)
        hipLaunchKernelGGL(k_set_final<true>, dim3(1), dim3(64), 0, st, (const double*)a.part, (const int*)a.pidx, emd_part, a.B, a.N, a.M,
                           B_total, base, out, win);
    else
        hipLaunchKernelGGL(k_set_final<false>, dim3(1), dim3(64), 0, st, (const double*)a.part, (const int*)a.pidx, emd_part, a.B, a.N, a.M,
                           B_total, base, out, win);
    return hipGetLastError();
}
hipError_t launch_step_loss_final(const StepLossDev& a, hipStream_t st) {
    bool srows = false, erows = false;
    for (int k = 0; k < a.n_terms; ++k) {
        const bool rows = (a.kind[k] & SET_LOSS_ROWS) != 0;
        if ((a.kind[k] & ~SET_LOSS_ROWS) == SET_LOSS_EMD) erows = erows || rows;
        else srows = srows || rows;
    }
    if (srows && erows) hipLaunchKernelGGL((k_step_loss_final<true, true>), dim3(1), dim3(64), 0, st, a);
    else if (srows) hipLaunchKernelGGL((k_step_loss_final<true, false>), dim3(1), dim3(64), 0, st, a);
    else if (erows) hipLaunchKernelGGL((k_step_loss_final<false, true>), dim3(1), dim3(64), 0, st, a);
    else hipLaunchKernelGGL((k_step_loss_final<false, false>), dim3(1), dim3(64), 0, st, a);
    return hipGetLastError();
}
hipError_t launch_set_grad(const SetLossDev& a, const SetRows& rows, const SetGradDev& g, hipStream_t st) {
    if (rows.nx) hipLaunchKernelGGL(k_set_grad<true>, dim3(a.B), dim3(ST), (size_t)a.M * 4, st, a, rows, g);
    else hipLaunchKernelGGL(k_set_grad<false>, dim3(a.B), dim3(ST), (size_t)a.M * 4, st, a, rows, g);
    return hipGetLastError();
}
hipError_t launch_prefix_rows(const float* attrs, int B, int N, int n_p, int* n, hipStream_t st) {
    hipLaunchKernelGGL(k_prefix_rows, dim3(B), dim3(ST), 0, st, attrs, N, n_p, n);
    return hipGetLastError();
}

}  // namespace ag
