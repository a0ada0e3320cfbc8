// (mu/mu_w, lambda)-CMA-ES on the device, gfx950 only: the optimiser behind CmaSearch and Planner(planner_type='CMA').  Standard
// algorithm (Hansen, "The CMA Evolution Strategy: A Tutorial", 2016): positive weights only, no active update, no restarts, fp64
// throughout.  The state is one caller-owned buffer of doubles (CmaLayout, ag_cma.h); a generation is
//   k_cma_ask   y_k = A z_k, genotype g_k = m + (sigma scale) o y_k, phenotype x_k = bound(g_k) rounded once to fp32.  One thread per
//               (candidate, coordinate), grid-stride; A = C^(1/2) is staged in LDS (it is symmetric, so row j serves as column j and
//               consecutive lanes read consecutive words).
//   k_cma_rank  rank_i = #{ j : (v_j, j) < (v_i, i) }, v the value to minimise (the fp32 input, negated when maximising); NaN is
//               greater than everything and NaNs are ordered by index.  order[rank_i] = i: ranks are unique by construction, so there
//               is one writer per slot - no sort, no atomics.  O(lambda^2) over at most 128 KB of values; 64 candidates per workgroup,
//               its four wavefronts each counting over a quarter of the population.
//   k_cma_tell  ONE workgroup, the state in LDS.  Recombination, the two evolution paths, the rank-1 / rank-mu covariance update,
//               sigma, then the eigendecomposition of the symmetrised C by Jacobi rotations and the SYMMETRIC roots
//               A = B diag(sqrt d) B^T, A^-1 = B diag(1 / sqrt d) B^T (they do not depend on the sign or order of the eigenvectors).
//               Nothing is written to the state before the update has been checked: a skipped (status bit 0) or discarded (bit 1)
//               generation leaves every word but the status as it was.
// SUMS OVER RANKS (y_w and the rank-mu matrix): E entries, CT threads; the ranked rows of y pass through LDS in tiles.  E >= CT: a
// thread walks r = 0 .. mu-1 for each of its entries.  E < CT: G = min(CT / E, mu) groups, group g adds r = g, g + G, ... in ascending r, and the G partials are added in
// ascending g.  G depends on (n, mu) alone - never on a launch parameter - so a state is bit-identical run to run.
// JACOBI: round-robin order (circle method over n, padded to even): a step holds floor(n / 2) rotations in disjoint planes, applied
// together as D <- J^T (D J), V <- V J (V is kept transposed): all column updates, a barrier, all row updates.  A sweep is n - 1 (n even) or n steps.  Before
// every sweep the off-diagonal norm is summed from the off-diagonal entries themselves; the sweeps end at off <= 1e-15 |diag|, or
// after CMA_SWEEPS.
// No float atomics, no inter-workgroup traffic, every loop bounded before it is entered, every index read from a table clamped.
#include "ag_cma.h"
#include "ag_lds_optin.h"

namespace ag {

namespace {
constexpr int CT = 1024;                        // threads of k_cma_tell
constexpr int CMA_SWEEPS = 60;
constexpr int CMA_GRID = 256, CMA_RANK_GRID = 512, CMA_BLOCK = 256;   // ask, rank: fixed grids, grid-stride loops (the sizes live in the state)
constexpr size_t CMA_TELL_LDS = (size_t)(4 * CMA_MAX_N * CMA_MAX_N + 6 * CMA_MAX_N + CMA_MAX_N + CT) * sizeof(double) +
                                (size_t)CMA_MAX_N * sizeof(int);

__device__ __forceinline__ bool finite_d(double v) { return fabs(v) < __builtin_inf(); }

struct CmaSizes { int n, pop, mu; bool ok; };
__device__ __forceinline__ CmaSizes cma_sizes(const double* st) {
    CmaSizes s{0, 0, 0, false};
    if (st[CMA_H_MAGIC] != CMA_MAGIC) return s;
    s.n = (int)st[CMA_H_N]; s.pop = (int)st[CMA_H_POP]; s.mu = (int)st[CMA_H_MU];
    s.ok = s.n >= 1 && s.n <= CMA_MAX_N && s.pop >= CMA_MIN_POP && s.pop <= CMA_MAX_POP && s.mu >= 1 && s.mu <= s.pop;
    return s;
}

// a genotype coordinate -> inside its limits.  A periodic coordinate is wrapped into [-P/2, P/2) first; finite lo < hi fold the
// line onto [lo, hi] (a triangle wave of period 2 (hi - lo): continuous, the identity inside); an infinite limit passes through.
__device__ __forceinline__ double cma_bound(double g, double lo, double hi, bool periodic, double P) {
    if (periodic) {
        double r = fmod(g + 0.5 * P, P);
        if (r < 0.0) { r += P; if (r >= P) r = 0.0; }
        g = r - 0.5 * P;
    }
    if (!(finite_d(lo) && finite_d(hi) && lo < hi)) return g;
    if (g >= lo && g <= hi) return g;
    const double w = hi - lo, w2 = 2.0 * w;
    double t = fmod(g - lo, w2);
    if (t < 0.0) t += w2;
    const double f = lo + (t <= w ? t : w2 - t);
    return f != f ? f : fmin(fmax(f, lo), hi);
}

__global__ __launch_bounds__(CMA_BLOCK) void k_cma_ask(const double* __restrict__ st, const double* __restrict__ z,
                                                       double* __restrict__ y, float* __restrict__ x) {
    __shared__ double sA[CMA_MAX_N * CMA_MAX_N];
    const CmaSizes s = cma_sizes(st);
    if (!s.ok) return;
    const int n = s.n;
    const long total = (long)s.pop * n;
    const long first = (long)blockIdx.x * CMA_BLOCK;
    if (first >= total) return;                                 // uniform per block: before the barrier
    const CmaLayout L(n, s.mu);
    for (int e = threadIdx.x; e < n * n; e += CMA_BLOCK) sA[e] = st[L.A + e];
    __syncthreads();
    const double sigma = st[CMA_H_SIGMA], P = st[CMA_H_PERIOD];
    for (long t = first + threadIdx.x; t < total; t += (long)gridDim.x * CMA_BLOCK) {
        const int k = (int)(t / n), i = (int)(t - (long)k * n);
        const double* zk = z + (long)k * n;
        double acc = 0.0;
        for (int j = 0; j < n; ++j) acc += sA[j * n + i] * zk[j];      // A[i][j] = A[j][i], bit for bit
        y[t] = acc;
        const double g = st[L.m + i] + (sigma * st[L.scale + i]) * acc;
        x[t] = (float)cma_bound(g, st[L.lo + i], st[L.hi + i], st[L.periodic + i] != 0.0, P);
    }
}

// is (a, ia) before (b, ib)?  NaN after everything, equal values (and NaNs) by index
__device__ __forceinline__ bool cma_before(float a, int ia, float b, int ib) {
    if (a != a) return b != b && ia < ib;
    if (b != b) return true;
    return a < b || (a == b && ia < ib);
}

// A workgroup ranks 64 candidates at a time: wavefront p of its four counts the candidates j of the p-th quarter of the population
// that come before candidate i (j is uniform in a wavefront: the values arrive by scalar loads), and the four integer counts are added.
__global__ __launch_bounds__(CMA_BLOCK) void k_cma_rank(const double* __restrict__ st, const float* __restrict__ val,
                                                        int* __restrict__ order) {
    __shared__ int cnt[CMA_BLOCK];
    const CmaSizes s = cma_sizes(st);
    if (!s.ok) return;
    const bool neg = st[CMA_H_MAXIMIZE] != 0.0;
    const int lane = threadIdx.x & 63, part = threadIdx.x >> 6;
    const int j0 = (int)((long)s.pop * part / 4), j1 = (int)((long)s.pop * (part + 1) / 4);
    for (int base = blockIdx.x * 64; base < s.pop; base += (int)gridDim.x * 64) {      // uniform in the workgroup
        const int i = base + lane;
        const bool live = i < s.pop;
        const float vi = live ? (neg ? -val[i] : val[i]) : 0.f;
        int c = 0;
#pragma unroll 8
        for (int j = j0; j < j1; ++j) {
            const float vj = neg ? -val[j] : val[j];
            c += cma_before(vj, j, vi, i) ? 1 : 0;
        }
        cnt[threadIdx.x] = c;
        __syncthreads();
        if (part == 0 && live) order[clampi(cnt[lane] + cnt[64 + lane] + cnt[128 + lane] + cnt[192 + lane], s.pop)] = i;
        __syncthreads();
    }
}

// out[e] = sum over r = 0 .. mu-1 of term(e, y_order[r], w_r) for e < E, in the fixed grouping of the file header.  The ranks are
// walked in tiles of R: the tile's rows of y (gathered through `order`) and its weights are staged in LDS by all threads, so that
// no thread waits for a chain of two global loads per term; the order in which a sum is formed is that of the file header.
// Ends with a barrier; `tile` (R (n + 1) doubles) is free again afterwards.
constexpr int CMA_EPT = CMA_MAX_N * CMA_MAX_N / CT;             // entries a thread holds at most
template <typename F>
__device__ __forceinline__ void cma_rank_sums(int E, int n, int mu, int pop, const double* __restrict__ y,
                                              const int* __restrict__ order, const double* __restrict__ wts, double* tile, int R,
                                              double* out, double* sP, F term) {
    const int tid = threadIdx.x;
    double* tw = tile + (size_t)R * n;
    int G = 1;
    if (E < CT) { G = CT / E; if (G > mu) G = mu; }
    const int e0 = E < CT ? tid % E : tid, g = E < CT ? tid / E : 0;
    const bool live = g < G;
    double acc[CMA_EPT];
#pragma unroll
    for (int q = 0; q < CMA_EPT; ++q) acc[q] = 0.0;
    for (int r0 = 0; r0 < mu; r0 += R) {
        const int rn = mu - r0 < R ? mu - r0 : R;
        __syncthreads();                                        // the previous tile has been used
        for (int idx = tid; idx < rn * n; idx += CT) {
            const int rr = idx / n, i = idx - rr * n;
            tile[idx] = y[(long)clampi(order[r0 + rr], pop) * n + i];
        }
        for (int rr = tid; rr < rn; rr += CT) tw[rr] = wts[r0 + rr];
        __syncthreads();
        if (live) {
            for (int rr = (g - r0 % G + G) % G; rr < rn; rr += G) {      // the group's ranks inside this tile, ascending
                const double* row = tile + rr * n;
                const double w = tw[rr];
#pragma unroll
                for (int q = 0; q < CMA_EPT; ++q) {
                    const int e = e0 + q * CT;
                    if (e < E) acc[q] += term(e, row, w);
                }
            }
        }
    }
    __syncthreads();
    if (E >= CT) {
#pragma unroll
        for (int q = 0; q < CMA_EPT; ++q) {
            const int e = e0 + q * CT;
            if (e < E) out[e] = acc[q];
        }
        __syncthreads();
        return;
    }
    if (live) sP[g * E + e0] = acc[0];
    __syncthreads();
    if (tid < E) {
        double t = 0.0;
        for (int k = 0; k < G; ++k) t += sP[k * E + tid];
        out[tid] = t;
    }
    __syncthreads();
}

__global__ __launch_bounds__(CT) void k_cma_tell(double* __restrict__ st, const double* __restrict__ y, const float* __restrict__ x,
                                                 const float* __restrict__ val, const int* __restrict__ order,
                                                 uint8_t* __restrict__ improved) {
    extern __shared__ __attribute__((aligned(16))) unsigned char cma_sm[];
    const int tid = threadIdx.x;
    const CmaSizes sz = cma_sizes(st);
    if (!sz.ok) { if (tid == 0) improved[0] = 0; return; }
    const int n = sz.n, pop = sz.pop, mu = sz.mu, nn = n * n;
    const CmaLayout L(n, mu);
    const int status = (int)st[CMA_H_STATUS];
    // ---- bit 0: fewer than mu values are not NaN <=> the value of rank mu - 1 is NaN (NaNs rank last)
    {
        const float vl = val[clampi(order[mu - 1], pop)];
        if (vl != vl) {                                         // uniform
            if (tid == 0) { st[CMA_H_STATUS] = (double)(status | 1); improved[0] = 0; }
            return;
        }
    }
    double* sC = reinterpret_cast<double*>(cma_sm);             // C, then the new C
    double* sD = sC + nn;                                       // rank-mu sum, Jacobi's working matrix, then A
    double* sV = sD + nn;                                       // eigenvectors, one per ROW (V^T: a rotation mixes two rows)
    double* tile = sV;                                          // until then: the rank sums' tile, over sV and sI and what n leaves free
    const int R = (4 * CMA_MAX_N * CMA_MAX_N - 2 * nn) / (n + 1);
    double* sI = sV + nn;                                       // A^-1
    double* sm = reinterpret_cast<double*>(cma_sm) + 4 * CMA_MAX_N * CMA_MAX_N;   // m (behind the matrices' full-size region)
    double* sps = sm + n;                                       // p_sigma
    double* spc = sps + n;                                      // p_c
    double* syw = spc + n;                                      // y_w
    double* sdv = syw + n;                                      // sqrt of the eigenvalues
    double* sdi = sdv + n;                                      // 1 / sqrt of the eigenvalues
    double* srot = sdi + n;                                     // [c | s] of a step's rotations, CMA_MAX_N / 2 each
    double* sP = srot + CMA_MAX_N;                              // CT partials
    int* spq = reinterpret_cast<int*>(sP + CT);                 // [p | q] of a step's rotations
    const double sigma = st[CMA_H_SIGMA], mueff = st[CMA_H_MUEFF], cs = st[CMA_H_CS], ds = st[CMA_H_DS], cc = st[CMA_H_CC],
                 c1 = st[CMA_H_C1], cmu = st[CMA_H_CMU], chin = st[CMA_H_CHIN], gen = st[CMA_H_GEN];
    const double* wts = st + L.w;
    for (int e = tid; e < nn; e += CT) sC[e] = st[L.C + e];
    if (tid < n) { sm[tid] = st[L.m + tid]; sps[tid] = st[L.ps + tid]; spc[tid] = st[L.pc + tid]; }
    // ---- 1. y_w = sum_r w_r y_order[r]
    cma_rank_sums(n, n, mu, pop, y, order, wts, tile, R, syw, sP, [](int e, const double* row, double w) { return w * row[e]; });
    // ---- 2, 3. the mean and p_sigma (A^-1 of the state is still the old one)
    if (tid < n) {
        sm[tid] = sm[tid] + (sigma * st[L.scale + tid]) * syw[tid];
        double t = 0.0;
        for (int j = 0; j < n; ++j) t += st[L.Ai + j * n + tid] * syw[j];      // A^-1 is symmetric bit for bit: row j as column j
        sps[tid] = (1.0 - cs) * sps[tid] + sqrt(cs * (2.0 - cs) * mueff) * t;
    }
    __syncthreads();
    // ---- 4, 5. |p_sigma| (every thread, ascending), h_sigma, p_c
    double ps2 = 0.0;
    for (int i = 0; i < n; ++i) ps2 += sps[i] * sps[i];
    const double psn = sqrt(ps2);
    const double hs = psn / sqrt(1.0 - pow(1.0 - cs, 2.0 * (gen + 1.0))) < (1.4 + 2.0 / (n + 1.0)) * chin ? 1.0 : 0.0;
    if (tid < n) spc[tid] = (1.0 - cc) * spc[tid] + (hs * sqrt(cc * (2.0 - cc) * mueff)) * syw[tid];
    __syncthreads();
    // ---- 6. C: the rank-mu sum into sD (a product of two coordinates first: the sum is symmetric bit for bit), then the update
    cma_rank_sums(nn, n, mu, pop, y, order, wts, tile, R, sD, sP,
                  [n](int e, const double* row, double w) { return (row[e / n] * row[e % n]) * w; });
    for (int e = tid; e < nn; e += CT) {
        const double c = sC[e];
        sC[e] = (1.0 - c1 - cmu) * c + c1 * (spc[e / n] * spc[e % n] + ((1.0 - hs) * cc * (2.0 - cc)) * c) + cmu * sD[e];
    }
    // ---- 7. sigma
    const double sigma_new = sigma * exp((cs / ds) * (psn / chin - 1.0));
    __syncthreads();
    // ---- symmetrise; D = C, V = I
    for (int e = tid; e < nn; e += CT) {
        const int i = e / n, j = e % n;
        sD[e] = 0.5 * (sC[e] + sC[j * n + i]);
        sV[e] = i == j ? 1.0 : 0.0;
    }
    __syncthreads();
    for (int e = tid; e < nn; e += CT) sC[e] = sD[e];
    // ---- Jacobi
    const int ne = n + (n & 1), half = ne / 2;
    // a step has half * n <= 2 CT tasks (a rotation, an index k); a thread's tasks and their split are the same in every step.
    // Columns: the rotation varies fastest, so a wavefront touches different columns of a row or two; rows: k varies fastest.
    static_assert(CMA_MAX_N / 2 * CMA_MAX_N <= 2 * CT, "two tasks per thread");
    int c_pr[2], c_k[2], r_pr[2], r_k[2];
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        const int task = tid + q * CT;
        c_k[q] = task / half; c_pr[q] = task - c_k[q] * half;
        r_pr[q] = task / n; r_k[q] = task - r_pr[q] * n;
    }
    for (int sweep = 0; sweep < CMA_SWEEPS; ++sweep) {
        if (tid < n) {                                          // column tid: consecutive lanes, consecutive words
            double off = 0.0;
            for (int j = 0; j < n; ++j) if (j != tid) off += sD[j * n + tid] * sD[j * n + tid];
            sP[tid] = off; sP[CMA_MAX_N + tid] = sD[tid * n + tid] * sD[tid * n + tid];
        }
        __syncthreads();
        double off = 0.0, dg = 0.0;
        for (int i = 0; i < n; ++i) { off += sP[i]; dg += sP[CMA_MAX_N + i]; }
        __syncthreads();
        if (!(off > 1e-30 * dg)) break;                         // uniform; a NaN ends the sweeps too (the check below sees it)
        for (int step = 0; step < ne - 1; ++step) {
            if (tid < half) {
                int a, b;
                if (tid == 0) { a = ne - 1; b = step; }
                else { a = (step + tid) % (ne - 1); b = (step - tid + ne - 1) % (ne - 1); }
                const int p = a < b ? a : b, q = a < b ? b : a;
                double c = 1.0, s = 0.0;
                if (q < n) {                                    // q == n: the padding index of an odd n
                    const double apq = sD[p * n + q];
                    if (apq != 0.0) {
                        const double theta = (sD[q * n + q] - sD[p * n + p]) / (2.0 * apq);
                        const double t = (theta < 0.0 ? -1.0 : 1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                        c = 1.0 / sqrt(t * t + 1.0);
                        s = t * c;
                    }
                }
                spq[tid] = p; spq[CMA_MAX_N / 2 + tid] = q < n ? q : p;
                srot[tid] = c; srot[CMA_MAX_N / 2 + tid] = s;
            }
            __syncthreads();
#pragma unroll
            for (int t = 0; t < 2; ++t) {                                // columns p, q of D
                if (tid + t * CT >= half * n) continue;
                const int pr = c_pr[t], k = c_k[t];
                const int p = spq[pr], q = spq[CMA_MAX_N / 2 + pr];
                const double c = srot[pr], s = srot[CMA_MAX_N / 2 + pr];
                if (s != 0.0) {
                    const double dp = sD[k * n + p], dq = sD[k * n + q];
                    sD[k * n + p] = c * dp - s * dq; sD[k * n + q] = s * dp + c * dq;
                }
            }
            __syncthreads();
#pragma unroll
            for (int t = 0; t < 2; ++t) {                                // rows p, q of D - the rotated entry is zero exactly - and of V^T
                if (tid + t * CT >= half * n) continue;
                const int pr = r_pr[t], k = r_k[t];
                const int p = spq[pr], q = spq[CMA_MAX_N / 2 + pr];
                const double c = srot[pr], s = srot[CMA_MAX_N / 2 + pr];
                if (s != 0.0) {
                    const double dp = sD[p * n + k], dq = sD[q * n + k];
                    sD[p * n + k] = k == q ? 0.0 : c * dp - s * dq;
                    sD[q * n + k] = k == p ? 0.0 : s * dp + c * dq;
                    const double vp = sV[p * n + k], vq = sV[q * n + k];
                    sV[p * n + k] = c * vp - s * vq; sV[q * n + k] = s * vp + c * vq;
                }
            }
            __syncthreads();
        }
    }
    // ---- the roots
    int bad = 0;
    if (tid < n) {
        const double d = sD[tid * n + tid];
        bad |= !(d > 0.0 && finite_d(d));
        const double r = sqrt(d);
        sdv[tid] = r; sdi[tid] = 1.0 / r;
        bad |= !(finite_d(sm[tid]) && finite_d(sps[tid]) && finite_d(spc[tid]) && finite_d(1.0 / r));
    }
    bad |= !(finite_d(sigma_new) && sigma_new > 0.0);
    __syncthreads();
    for (int e = tid; e < nn; e += CT) {
        const int i = e / n, j = e % n;
        double a = 0.0, ai = 0.0;
        for (int k = 0; k < n; ++k) {
            const double vv = sV[k * n + i] * sV[k * n + j];
            a += vv * sdv[k];
            ai += vv * sdi[k];
        }
        sI[e] = ai;
        bad |= !(finite_d(a) && finite_d(ai) && finite_d(sC[e]));
        sD[e] = a;                                              // (the diagonal of D was read before the barrier)
    }
    bad = __syncthreads_or(bad);
    // ---- bit 1: the update is dropped; nothing of the state has been written yet
    if (bad) {
        if (tid == 0) { st[CMA_H_STATUS] = (double)(status | 2); improved[0] = 0; }
        return;
    }
    // ---- commit
    for (int e = tid; e < nn; e += CT) { st[L.C + e] = sC[e]; st[L.A + e] = sD[e]; st[L.Ai + e] = sI[e]; }
    if (tid < n) { st[L.m + tid] = sm[tid]; st[L.ps + tid] = sps[tid]; st[L.pc + tid] = spc[tid]; }
    const int b = clampi(order[0], pop);
    const float vb = val[b];
    const bool neg = st[CMA_H_MAXIMIZE] != 0.0;
    const double key = neg ? -(double)vb : (double)vb, best = neg ? -st[CMA_H_BEST_V] : st[CMA_H_BEST_V];
    const bool better = key < best;                             // strictly; a NaN never is
    __syncthreads();                                            // every thread has read the old best value
    if (better && tid < n) st[L.best_x + tid] = (double)x[(long)b * n + tid];
    if (tid == 0) {
        if (better) { st[CMA_H_BEST_V] = (double)vb; st[CMA_H_BEST_G] = gen; }
        st[CMA_H_SIGMA] = sigma_new;
        st[CMA_H_GEN] = gen + 1.0;
        improved[0] = better ? 1 : 0;
    }
}

hipError_t cma_tell_attr() {
    static std::atomic<unsigned long long> done{0};             // the dynamic-LDS opt-in, per device (ag_lds_optin.h)
    return lds_opt_in(done, (int)CMA_TELL_LDS, k_cma_tell);
}
}  // namespace

hipError_t launch_cma_ask(const double* state, const double* z, double* y, float* x, hipStream_t st) {
    hipLaunchKernelGGL(k_cma_ask, dim3(CMA_GRID), dim3(CMA_BLOCK), 0, st, state, z, y, x);
    return hipGetLastError();
}
hipError_t launch_cma_tell(double* state, const double* y, const float* x, const float* values, int* order, uint8_t* improved,
                           hipStream_t st) {
    hipError_t e = cma_tell_attr();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_cma_rank, dim3(CMA_RANK_GRID), dim3(CMA_BLOCK), 0, st, state, values, order);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_cma_tell, dim3(1), dim3(CT), CMA_TELL_LDS, st, state, y, x, values, order, improved);
    return hipGetLastError();
}

}  // namespace ag
