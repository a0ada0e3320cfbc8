// Earth-mover loss of the training side (reference src/dynamics/gnn/loss.py: EarthMoverLoss :25-60) over a BATCH of cloud pairs
// x (B,N,3), y (B,M,3), gfx950 only: per graph the one-to-one matching of K = min(N, M) pairs with the smallest sum of distances,
// and the mean of all B*K matched distances.  The reference solves it on the host (scipy.optimize.linear_sum_assignment per
// graph); here the solve is a kernel, so a training step never waits for the host.
//   k_emd_assign one workgroup per graph, both clouds in LDS as SoA.  The smaller cloud is the row side (x when N == M), L = max(N, M)
//                columns.  cost(row, column) is set_dist of the pair - fp32, every operation rounded on its own, recomputed from
//                LDS whenever it is needed and widened to fp64; no N x M matrix exists.  The solver is the rectangular
//                shortest-augmenting-path algorithm with dual variables (Jonker & Volgenant 1987; Crouse 2016, "On implementing
//                2D rectangular assignment algorithms"), written from the papers' description: rows are added one at a time; for
//                each a Dijkstra search over the columns in reduced costs finds the cheapest alternating path to a free column,
//                the duals u (rows) and v (columns) move so that the path is tight, and the path is flipped.  Duals, path costs
//                and the running minimum are fp64.  One search step = every thread relaxes its columns from the current row, then
//                a block arg-min over the unscanned columns (shuffle tree in a wave, then the waves in wave order).
//                TIE RULE: among equal path costs a free (unassigned) column wins, then the lowest column index.
//                Every loop is bounded before it is entered: K augmentations, at most L search steps each, a path walk of at most
//                K links; every index read from a table is clamped before it addresses anything.  A bound that runs out (it
//                cannot with finite costs) marks the graph failed.  No atomics, no spin-waits, nothing between workgroups.
//                NON-FINITE INPUT: the clouds are scanned first; a graph with a non-finite coordinate is not solved.  A failed
//                graph gets a match table of -1, a NaN partial and a non-zero status word; the loss is then NaN and its rows of
//                the gradient are NaN.
//                Per graph: match[i] = the y index matched to x_i or -1 (int32, N), one fp64 partial = the sum of the matched
//                fp32 distances in ascending i, a status word.
//   finaliser    k_set_final / k_step_loss_final (ag_setloss.hip): the B partials in index order in fp64, / (B_total K), one rounding.
//   k_emd_grad   g_x[b,i] = s (x_i - y_match(i)) / dist with s = g_out w / (B_total K); zero at zero distance and for an unmatched
//                x_i (N > M only).  One writer per element: overwrites, or adds to the chain's dLoss/dpred.
// REAL ROWS (AG_LOSS_ROWS, template <bool ROWS>): the matching runs over the prefixes x[b, :nx_b], y[b, :ny_b] with K_b = min(nx_b,
// ny_b) pairs, the loss is the mean over graphs of sum_b matched / K_b, the gradient scale g_out w / (B_total K_b); see k_emd_assign.
#include "ag_setloss.h"
#include "ag_lds_optin.h"

namespace ag {

namespace {
#ifndef AG_EMD_THREADS
#define AG_EMD_THREADS 256                      // 64: one wavefront per graph, no barrier in a search step (docs/EXPERIMENTS.md)
#endif
constexpr int EA = AG_EMD_THREADS;              // threads of k_emd_assign
constexpr int ET = 256;                         // threads of k_emd_grad
static_assert(EA == 64 || EA == 128 || EA == 256, "k_emd_assign runs 1, 2 or 4 wavefronts");
constexpr int EMD_ASSIGNED = 1 << 30;           // key = column | EMD_ASSIGNED for a column that has a row: a free column's key is lower
constexpr int EMD_NONE = 0x7fffffff;            // key of "no candidate"; its value is +inf, every candidate's is below
constexpr int EMD_LDS_BUDGET = 160 * 1024 - 2048;

__device__ __forceinline__ bool finite_f(float v) { return fabsf(v) < __builtin_inff(); }
// does (ov, ok) beat (v, k) as a minimum?  smaller value, or the lower key of equal values (keys are distinct per column)
__device__ __forceinline__ bool min_beats(double ov, int ok, double v, int k) { return ov < v || (ov == v && ok < k); }

// the block's smallest (value, key); every thread returns with it.  NT == 64: shuffles only, no barrier.  NT > 64: one barrier,
// sh / shk alternate between two halves by `par` so that a step's writes never meet the previous step's reads
template <int NT>
__device__ __forceinline__ void block_argmin_f64(double& v, int& k, double (*sh)[NT / 64], int (*shk)[NT / 64], int par) {
    for (int o = 32; o > 0; o >>= 1) {
        const double ov = __shfl_xor(v, o); const int ok = __shfl_xor(k, o);
        if (min_beats(ov, ok, v, k)) { v = ov; k = ok; }
    }
    if constexpr (NT > 64) {
        if ((threadIdx.x & 63) == 0) { sh[par][threadIdx.x >> 6] = v; shk[par][threadIdx.x >> 6] = k; }
        __syncthreads();
        v = sh[par][0]; k = shk[par][0];
        for (int w = 1; w < NT / 64; ++w)
            if (min_beats(sh[par][w], shk[par][w], v, k)) { v = sh[par][w]; k = shk[par][w]; }
    }
}

// LDS of one graph, K rows and L columns: fp64 u[K] v[L] sp[L]; fp32 rows [3][K], columns [3][L]; int32 col4row[K] row4col[L]
// path[L] scanned[L]  = 24 K + 40 L bytes
__host__ __device__ inline size_t emd_lds_bytes(int K, int L) { return (size_t)24 * K + (size_t)40 * L; }

// ROWS: the graph's clouds are the prefixes x[b, :nx], y[b, :ny] (set_rows_of).  K, L and the row side come from these clamped
// counts, before any loop is entered, so every loop below keeps its bound; the LDS arrays are carved for the padded sizes
// (Kp = min(N, M) >= K, Lp = max(N, M) >= L).  An empty graph is solved by nothing: match -1, partial 0, status EMD_OK.  Padding
// rows are never read; their match entries are -1; the partial is the graph's own mean, sum of matched / K.
template <int NT, bool ROWS>
__global__ __launch_bounds__(NT) void k_emd_assign(EmdDev a, SetRows rw) {
    extern __shared__ __attribute__((aligned(16))) unsigned char emd_sm[];
    __shared__ double sh[2][NT / 64];
    __shared__ int shk[2][NT / 64];
    __shared__ int s_fail;
    const int b = blockIdx.x, tid = threadIdx.x;
    const int N = a.N, M = a.M;
    int nx = N, ny = M;
    if constexpr (ROWS) set_rows_of(rw, b, N, M, nx, ny);
    int* match = a.match + (long)b * N;
    if constexpr (ROWS) {
        if (nx == 0) {                                          // uniform: an empty graph adds 0 and matches nothing
            for (int i = tid; i < N; i += NT) match[i] = -1;
            if (tid == 0) { a.part[b] = 0.0; a.status[b] = EMD_OK; }
            return;
        }
    }
    const bool xrows = nx <= ny;                                // the smaller cloud is the row side, x when N == M
    const int K = xrows ? nx : ny, L = xrows ? ny : nx;
    const int Kp = N <= M ? N : M, Lp = N <= M ? M : N;         // the carving; Kp == K and Lp == L without ROWS
    double* u = reinterpret_cast<double*>(emd_sm);              // [K] row duals
    double* v = u + Kp;                                         // [L] column duals
    double* sp = v + Lp;                                        // [L] cost of the cheapest path found to a column in this search
    float* rs = reinterpret_cast<float*>(sp + Lp);              // [3][K]
    float* cs = rs + 3 * Kp;                                    // [3][L]
    int* col4row = reinterpret_cast<int*>(cs + 3 * Lp);         // [K]
    int* row4col = col4row + Kp;                                // [L]
    int* path = row4col + Lp;                                   // [L] the row a column's cheapest path comes from
    int* scanned = path + Lp;                                   // [L]
    const float* xr = a.x + (long)b * a.x_bstride;
    const float* yr = a.y + (long)b * a.y_bstride;
    const float* rr = xrows ? xr : yr;
    const float* cr = xrows ? yr : xr;
    int bad = 0;
    for (int i = tid; i < K; i += NT) {
        const float p = rr[3 * i], q = rr[3 * i + 1], r = rr[3 * i + 2];
        rs[i] = p; rs[K + i] = q; rs[2 * K + i] = r;
        bad |= !(finite_f(p) && finite_f(q) && finite_f(r));
        u[i] = 0.0; col4row[i] = -1;
    }
    for (int j = tid; j < L; j += NT) {
        const float p = cr[3 * j], q = cr[3 * j + 1], r = cr[3 * j + 2];
        cs[j] = p; cs[L + j] = q; cs[2 * L + j] = r;
        bad |= !(finite_f(p) && finite_f(q) && finite_f(r));
        v[j] = 0.0; row4col[j] = -1; path[j] = 0;
    }
    if (tid == 0) s_fail = 0;
    bad = __syncthreads_or(bad);
    int fail = bad ? EMD_NONFINITE : EMD_OK;
    for (int cur = 0; cur < K && !fail; ++cur) {                // ---- one augmentation per row
        for (int j = tid; j < L; j += NT) { sp[j] = __builtin_inf(); scanned[j] = 0; }   // a thread's own columns: no barrier
        double minv = 0.0;
        int i = cur, sink = -1;
        for (int step = 0; step < L; ++step) {                  // ---- the search: scans one column per step
            const float rx = rs[i], ry = rs[K + i], rz = rs[2 * K + i];
            const double ui = u[i];
            double bv = __builtin_inf();
            int bk = EMD_NONE;
            for (int j = tid; j < L; j += NT) {
                if (scanned[j]) continue;
                const float d = xrows ? set_dist(rx, ry, rz, cs[j], cs[L + j], cs[2 * L + j])
                                      : set_dist(cs[j], cs[L + j], cs[2 * L + j], rx, ry, rz);      // always x - y
                const double r = ((minv + (double)d) - ui) - v[j];
                if (r < sp[j]) { sp[j] = r; path[j] = i; }
                const double s = sp[j];
                const int key = j | (row4col[j] >= 0 ? EMD_ASSIGNED : 0);
                if (s < __builtin_inf() && min_beats(s, key, bv, bk)) { bv = s; bk = key; }
            }
            block_argmin_f64<NT>(bv, bk, sh, shk, step & 1);
            if (bk == EMD_NONE) break;                          // no finite path cost left: sink stays -1
            const int j = clampi(bk & (EMD_ASSIGNED - 1), L);
            minv = bv;
            if (j % NT == tid) scanned[j] = 1;                  // the column's owner
            if (!(bk & EMD_ASSIGNED)) { sink = j; break; }
            i = clampi(row4col[j], K);
        }
        if (sink < 0) { fail = EMD_EXHAUSTED; break; }          // uniform: every thread holds the same (bv, bk)
        // the duals: scanned columns and their rows move by what the search overshot them; the new row by the whole path cost
        for (int j = tid; j < L; j += NT) {
            if (!scanned[j]) continue;
            const double d = minv - sp[j];
            const int r = row4col[j];
            if (r >= 0) u[clampi(r, K)] += d;                   // distinct columns hold distinct rows, and none holds `cur`
            v[j] -= d;
        }
        if (tid == 0) u[cur] += minv;
        __syncthreads();
        if (tid == 0) {                                         // flip the path from the sink back to `cur`
            int j = sink;
            bool closed = false;
            for (int n = 0; n < K; ++n) {
                const int r = clampi(path[j], K);
                row4col[j] = r;
                const int prev = col4row[r];
                col4row[r] = j;
                if (r == cur) { closed = true; break; }
                j = clampi(prev, L);
            }
            if (!closed) s_fail = EMD_EXHAUSTED;
        }
        __syncthreads();
        fail = s_fail;
    }
    // ---- the graph's output
    if (fail) {
        for (int i = tid; i < N; i += NT) match[i] = -1;
        if (tid == 0) { a.part[b] = __builtin_nan(""); a.status[b] = fail; }
        return;
    }
    for (int i = tid; i < N; i += NT) {                         // N <= Lp: sp has room for every x_i's matched distance
        const int m = (!ROWS || i < nx) ? (xrows ? col4row[i] : row4col[i]) : -1;
        match[i] = m;
        double d = 0.0;
        if (m >= 0) {
            const int c = clampi(m, ny);
            d = xrows ? (double)set_dist(rs[i], rs[K + i], rs[2 * K + i], cs[c], cs[L + c], cs[2 * L + c])
                      : (double)set_dist(cs[i], cs[L + i], cs[2 * L + i], rs[c], rs[K + c], rs[2 * K + c]);
        }
        sp[i] = d;
    }
    __syncthreads();
    if (tid == 0) {
        double s = 0.0;
        for (int i = 0; i < N; ++i) s += sp[i];                 // ascending i; an unmatched x_i adds +0
        a.part[b] = ROWS ? s / (double)K : s;
        a.status[b] = EMD_OK;
    }
}

// ROWS: the scale is the graph's own 1 / (B_total K_b); padding rows get exact zeros, a failed graph NaN in its real rows only
template <bool ROWS>
__global__ __launch_bounds__(ET) void k_emd_grad(EmdDev a, SetRows rw, SetGradDev g) {
    const int b = blockIdx.x, tid = threadIdx.x;
    int nx = a.N, ny = a.M;
    if constexpr (ROWS) set_rows_of(rw, b, a.N, a.M, nx, ny);
    const int Kb = nx < ny ? nx : ny;
    const int K = ROWS ? (Kb > 0 ? Kb : 1) : (a.N < a.M ? a.N : a.M);    // an empty graph has no real row to scale
    const float go = g.gout ? g.gout[0] : 1.f;
    const float s = (float)((double)go * g.w_emd / ((double)g.B_total * K));      // the mean's 1 / (B_total K)
    const bool failed = a.status[b] != EMD_OK;
    const int* match = a.match + (long)b * a.N;
    const float* xr = a.x + (long)b * a.x_bstride;
    const float* yr = a.y + (long)b * a.y_bstride;
    float* gr = g.gx + (long)b * a.N * 3;
    for (int i = tid; i < a.N; i += ET) {
        float v[3] = {0.f, 0.f, 0.f};
        const int m = match[i];
        if (ROWS && i >= nx) {}
        else if (failed) v[0] = v[1] = v[2] = __builtin_nanf("");
        else if (m >= 0) set_pull(xr + 3 * i, yr + 3 * clampi(m, ny), s, v);
        if (g.add) { gr[3 * i] += v[0]; gr[3 * i + 1] += v[1]; gr[3 * i + 2] += v[2]; }
        else { gr[3 * i] = v[0]; gr[3 * i + 1] = v[1]; gr[3 * i + 2] = v[2]; }
    }
}
}  // namespace

size_t emd_max_points() { return EMD_LDS_BUDGET / 40 - 2; }     // 40 bytes a point covers 24 K + 40 L

hipError_t launch_emd_assign(const EmdDev& a, const SetRows& rows, hipStream_t st) {
    const int K = a.N < a.M ? a.N : a.M, L = a.N < a.M ? a.M : a.N;
    static std::atomic<unsigned long long> done{0};             // the dynamic-LDS opt-in, per device (ag_lds_optin.h)
    if (hipError_t e = lds_opt_in(done, EMD_LDS_BUDGET, k_emd_assign<EA, false>, k_emd_assign<EA, true>); e != hipSuccess) return e;
    if (rows.nx) hipLaunchKernelGGL((k_emd_assign<EA, true>), dim3(a.B), dim3(EA), emd_lds_bytes(K, L), st, a, rows);
    else hipLaunchKernelGGL((k_emd_assign<EA, false>), dim3(a.B), dim3(EA), emd_lds_bytes(K, L), st, a, rows);
    return hipGetLastError();
}
hipError_t launch_emd_grad(const EmdDev& a, const SetRows& rows, const SetGradDev& g, hipStream_t st) {
    if (rows.nx) hipLaunchKernelGGL(k_emd_grad<true>, dim3(a.B), dim3(ET), 0, st, a, rows, g);
    else hipLaunchKernelGGL(k_emd_grad<false>, dim3(a.B), dim3(ET), 0, st, a, rows, g);
    return hipGetLastError();
}

}  // namespace ag
