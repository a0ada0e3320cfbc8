// Backward pass of DynamicsPredictor.forward (reference src/dynamics/gnn/model.py:130-342) on exact-fp32 MFMA, gfx950 only.
//
// The forward chains of ag_mlp.hip keep every activation in registers and never store one, so the backward RECOMPUTES what it
// needs, layer by layer, into a workspace (ag_backward chunks the batch to bound it; DESIGN.md "Training").  Every contraction
// is one strided GEMM kernel on v_mfma_f32_32x32x2_f32 (k_gemm), in three shapes:
//   Y  = X * W^T (+ b)       recompute                      rows = B*N or B*E
//   dX = dY * W              input gradient                 rows = B*N or B*E
//   dW = dY^T * [X | 1]      weight + bias gradient         reduced over rows: split-K slabs, summed in slab order in fp64 (k_reduce)
// No float atomics anywhere: node sums walk the receiver CSR (row_ptr) and a per-graph sender CSR built here by a stable
// counting sort (k_send_csr), in ascending edge order.  Two calls on the same inputs are bit-identical, and a row's input
// gradient does not depend on which other rows share its launch.  ag_backward_inputs adds one more dX GEMM: the particle
// encoder's input gradient dH1 * W0, whose columns are dLoss/dphys and dLoss/daction.
#include "ag_model.h"
#include "ag_train.h"
#include <algorithm>
#include <cstdint>

namespace ag {
namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int TM = 64, TN = 64, TK = 32;   // workgroup tile; four wavefronts of 32x32
constexpr int kMaxSlabs = 1024;            // split-K slabs of a weight-gradient reduction

struct GemmArgs {
    const float* A; long sam, sak;               // A(m,k) = A[m*sam + k*sak]
    const float* Bm; long sbk, sbn; int ones_col; // B(k,n) = Bm[k*sbk + n*sbn]; column ones_col (if >= 0) is all ones
    int M, N, K, kslab;                          // blockIdx.z covers k in [z*kslab, min(K, (z+1)*kslab))
    float* C; long ldc; long slab_stride;        // C + z*slab_stride
    const float* bias;                           // (N,) or null
    const float* add; long ld_add;               // + add(m,n), or null
    int accumulate;                              // + C(m,n) as it was
    const float* mask; long ld_mask;             // result kept where mask(m,n) > 0 (ReLU backward), or null
    int relu;
};

__global__ __launch_bounds__(256) void k_gemm(GemmArgs a) {
    __shared__ float As[TK][TM + 4];
    __shared__ float Bs[TK][TN + 4];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int wm = w >> 1, wn = w & 1;
    const long m0 = (long)blockIdx.x * TM;
    const int n0 = blockIdx.y * TN;
    const int kb = blockIdx.z * a.kslab, ke = min(a.K, kb + a.kslab);
    const bool a_kfast = a.sak == 1, b_nfast = a.sbn == 1;
    f32x16 acc;
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    for (int k0 = kb; k0 < ke; k0 += TK) {
#pragma unroll
        for (int i = 0; i < TM * TK / 256; ++i) {
            const int idx = t + 256 * i;
            const int kk = a_kfast ? (idx & (TK - 1)) : (idx / TM);
            const int mm = a_kfast ? (idx / TK) : (idx & (TM - 1));
            const long m = m0 + mm; const int k = k0 + kk;
            As[kk][mm] = (m < a.M && k < ke) ? a.A[m * a.sam + (long)k * a.sak] : 0.f;
        }
#pragma unroll
        for (int i = 0; i < TN * TK / 256; ++i) {
            const int idx = t + 256 * i;
            const int kk = b_nfast ? (idx / TN) : (idx & (TK - 1));
            const int nn = b_nfast ? (idx & (TN - 1)) : (idx / TK);
            const int n = n0 + nn; const int k = k0 + kk;
            float v = 0.f;
            if (k < ke && n < a.N) v = n == a.ones_col ? 1.f : a.Bm[(long)k * a.sbk + (long)n * a.sbn];
            Bs[kk][nn] = v;
        }
        __syncthreads();
#pragma unroll
        for (int s = 0; s < TK / 2; ++s) {
            const float av = As[2 * s + (lane >> 5)][wm * 32 + (lane & 31)];
            const float bv = Bs[2 * s + (lane >> 5)][wn * 32 + (lane & 31)];
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, acc, 0, 0, 0);
        }
        __syncthreads();
    }
    float* C = a.C + (long)blockIdx.z * a.slab_stride;
    const int n = n0 + wn * 32 + (lane & 31);
    if (n >= a.N) return;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const long m = m0 + wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
        if (m >= a.M) continue;
        float v = acc[r];
        if (a.bias) v += a.bias[n];
        if (a.add) v += a.add[m * a.ld_add + n];
        if (a.accumulate) v += C[m * a.ldc + n];
        if (a.mask && !(a.mask[m * a.ld_mask + n] > 0.f)) v = 0.f;
        if (a.relu) v = fmaxf(v, 0.f);
        C[m * a.ldc + n] = v;
    }
}

// Weight-gradient reduction of the split-K slabs, fixed order, fp64: part[g][i] = sum of slabs 32g .. 32g+31 (k_reduce_part), then
// dst_w[m*ldw + col0 + n] (n < n_w) or dst_b[m] (n == n_w) += sum over g ascending, rounded once (k_reduce).  wide: the old value
// joins the fp64 sum before that one rounding (a later part of an accumulated step, ag_train_step_part); else it is added in fp32
constexpr int kSlabGroup = 32;
__global__ void k_reduce_part(const float* slab, int elems, int nz, double* part) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= elems) return;
    const int g = blockIdx.y, z1 = min(nz, (g + 1) * kSlabGroup);
    double s = 0.0;
    for (int z = g * kSlabGroup; z < z1; ++z) s += (double)slab[(long)z * elems + i];
    part[(long)g * elems + i] = s;
}
__global__ void k_reduce(const double* part, int M, int Ncols, int ng, float* dst_w, int ldw, int col0, int n_w, float* dst_b, int wide) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= M * Ncols) return;
    const int m = i / Ncols, n = i % Ncols;
    double s = 0.0;
    for (int g = 0; g < ng; ++g) s += part[(long)g * M * Ncols + i];
    float* d = n < n_w ? dst_w + (long)m * ldw + col0 + n : (dst_b ? dst_b + m : nullptr);
    if (!d) return;
    *d = wide ? (float)((double)*d + s) : *d + (float)s;
}

__device__ inline int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// node input [attr(2), phys, action(3)] (model.py:169,206-223; state_dim 0)
__global__ void k_train_prep_node(const float* attrs, const float* phys, const float* action, long rows, float* xn) {
    const long r = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= rows) return;
    xn[r * 6 + 0] = attrs[r * 2]; xn[r * 6 + 1] = attrs[r * 2 + 1]; xn[r * 6 + 2] = phys[r];
    xn[r * 6 + 3] = action[r * 3]; xn[r * 6 + 4] = action[r * 3 + 1]; xn[r * 6 + 5] = action[r * 3 + 2];
}

__device__ inline float snt_at(const float* s, int n_his, int N, int i, int f) {   // state_norm_t (model.py:156-166)
    const int t = f / 3, c = f % 3;
    const float cur = s[((long)t * N + i) * 3 + c];
    return t < n_his - 1 ? s[((long)(t + 1) * N + i) * 3 + c] - cur : cur;
}

// relation input [attr_r(2), attr_s(2), group diff, pos_diff(3 n_his)] (model.py:247-282); padding edges are zero rows
__global__ void k_train_prep_edge(const float* state, const float* attrs, const float* group, int n_inst, const int* recv,
                                  const int* send, const int* n_edges, int edge_cap, int B, int N, int Ep, int n_his, float* xe) {
    const long r = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= (long)B * Ep) return;
    const int b = (int)(r / Ep), e = (int)(r % Ep);
    const int R = 5 + 3 * n_his;
    float* o = xe + r * R;
    if (e >= n_edges[b]) { for (int f = 0; f < R; ++f) o[f] = 0.f; return; }
    const int i = clampi(recv[(long)b * edge_cap + e], 0, N - 1), j = clampi(send[(long)b * edge_cap + e], 0, N - 1);
    const float* at = attrs + (long)b * N * 2;
    o[0] = at[i * 2]; o[1] = at[i * 2 + 1]; o[2] = at[j * 2]; o[3] = at[j * 2 + 1];
    const float* g = group + (long)b * N * n_inst;
    float gd = 0.f;
    for (int k = 0; k < n_inst; ++k) gd += fabsf(g[(long)i * n_inst + k] - g[(long)j * n_inst + k]);
    o[4] = gd;
    const float* s = state + (long)b * n_his * N * 3;
    for (int f = 0; f < 3 * n_his; ++f) o[5 + f] = snt_at(s, n_his, N, i, f) - snt_at(s, n_his, N, j, f);
}

// er = relu(C + U[recv] + V[send]): the relation propagator on the factored W = [W1 | W2 | W3] (model.py:312-318)
__global__ void k_edge_act(const float* C, const float* U, const float* V, const int* recv, const int* send, const int* n_edges,
                           int edge_cap, int B, int N, int Ep, float* er) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long)B * Ep * NF) return;
    const long r = i / NF; const int f = (int)(i % NF);
    const int b = (int)(r / Ep), e = (int)(r % Ep);
    if (e >= n_edges[b]) { er[i] = 0.f; return; }
    const long u = (long)b * N + clampi(recv[(long)b * edge_cap + e], 0, N - 1);
    const long v = (long)b * N + clampi(send[(long)b * edge_cap + e], 0, N - 1);
    er[i] = fmaxf(C[i] + U[u * NF + f] + V[v * NF + f], 0.f);
}

// dpre = dAgg[recv] where er > 0 (ReLU backward of the relation propagator; model.py:324 scatter-sum backward = gather)
__global__ void k_edge_dpre(const float* dagg, const float* er, const int* recv, const int* n_edges, int edge_cap, int B, int N,
                            int Ep, float* dpre) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long)B * Ep * NF) return;
    const long r = i / NF; const int f = (int)(i % NF);
    const int b = (int)(r / Ep), e = (int)(r % Ep);
    if (e >= n_edges[b] || !(er[i] > 0.f)) { dpre[i] = 0.f; return; }
    const long u = (long)b * N + clampi(recv[(long)b * edge_cap + e], 0, N - 1);
    dpre[i] = dagg[u * NF + f];
}

// out[b*N+i][col_out + f] (=|+=) sign * sum over the edges of node i, in ascending CSR order, of src[b*Ep + e][col0 + f].
// ptr (B, N+1) CSR offsets; idx null: the CSR positions are the edge ids (receiver CSR), else idx (B, Ep) maps them.
__global__ void k_segsum(const float* src, int ld_src, int col0, int width, const int* ptr, const int* idx, const int* n_edges,
                         int B, int N, int Ep, float sign, int accumulate, float* out, int ld_out, int col_out) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long)B * N * width) return;
    const long node = i / width; const int f = (int)(i % width);
    const int b = (int)(node / N), n = (int)(node % N);
    const int ne = n_edges[b];
    const int* p = ptr + (long)b * (N + 1);
    const int lo = clampi(p[n], 0, ne), hi = clampi(p[n + 1], lo, ne);
    float s = 0.f;
    for (int q = lo; q < hi; ++q) {
        const int e = idx ? clampi(idx[(long)b * Ep + q], 0, Ep - 1) : q;
        s += src[((long)b * Ep + e) * ld_src + col0 + f];
    }
    float* o = out + node * ld_out + col_out + f;
    *o = accumulate ? *o + sign * s : sign * s;
}

// Sender CSR of every graph by a stable counting sort: one wavefront per graph.  sptr (B, N+1); sidx (B, Ep) edge ids grouped
// by sender, ascending within a sender; cur (B, N) scratch.
__global__ __launch_bounds__(64) void k_send_csr(const int* send, const int* n_edges, int edge_cap, int N, int Ep, int* sptr,
                                                 int* sidx, int* cur) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const int ne = n_edges[b];
    int* p = sptr + (long)b * (N + 1);
    int* c = cur + (long)b * N;
    for (int i = lane; i < N; i += 64) c[i] = 0;
    __syncthreads();
    for (int e = lane; e < ne; e += 64) atomicAdd(&c[clampi(send[(long)b * edge_cap + e], 0, N - 1)], 1);
    __syncthreads();
    if (lane == 0) {
        int run = 0;
        for (int i = 0; i < N; ++i) { p[i] = run; const int k = c[i]; c[i] = run; run += k; }
        p[N] = run;
    }
    __syncthreads();
    for (int e0 = 0; e0 < ne; e0 += 64) {
        const int e = e0 + lane;
        const int s = e < ne ? clampi(send[(long)b * edge_cap + e], 0, N - 1) : -1;
        int rank = 0, later = 0;
        for (int l = 0; l < 64; ++l) {
            const int o = __shfl(s, l);
            if (o == s) { if (l < lane) ++rank; else if (l > lane) ++later; }
        }
        const int base = s >= 0 ? c[s] : 0;
        __syncthreads();
        if (s >= 0) {
            sidx[(long)b * Ep + base + rank] = e;
            if (later == 0) c[s] = base + rank + 1;
        }
        __syncthreads();
    }
}

// dMotion of the head: d_motion + d_pos where -clamp <= motion <= clamp (torch clamp_backward, inclusive); rows i >= n_p zero
__global__ void k_head_grad(const float* motion, const float* dpos, const float* dmot, int B, int N, int n_p, float clamp,
                            float* g) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long)B * N * 3) return;
    const long r = i / 3; const int c = (int)(i % 3);
    const int b = (int)(r / N), n = (int)(r % N);
    float v = 0.f;
    if (n < n_p) {
        const long o = ((long)b * n_p + n) * 3 + c;
        const float m = motion[i];
        if (dmot) v = dmot[o];
        if (dpos && m >= -clamp && m <= clamp) v += dpos[o];
    }
    g[i] = v;
}

// out = (a + b) where m > 0
__global__ void k_add_mask(const float* a, const float* b, const float* m, long n, float* out) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    out[i] = m[i] > 0.f ? a[i] + b[i] : 0.f;
}

// dState from dSnt (the position-difference features) through state_res = state[1:] - state[:-1] (model.py:156), plus d_pos on
// the last frame of the object particles (model.py:338)
__global__ void k_dstate(const float* dsnt, const float* dpos, int B, int N, int n_p, int n_his, float* dstate) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long)B * N * 3) return;
    const long r = i / 3; const int c = (int)(i % 3);
    const int b = (int)(r / N), n = (int)(r % N);
    const int F = 3 * n_his;
    const float* d = dsnt + r * F;
    for (int t = 0; t < n_his; ++t) {
        float v;
        if (t == n_his - 1) {
            v = d[3 * t + c];
            if (n_his >= 2) v += d[3 * (t - 1) + c];
            if (dpos && n < n_p) v += dpos[((long)b * n_p + n) * 3 + c];
        } else {
            v = -d[3 * t + c];
            if (t > 0) v += d[3 * (t - 1) + c];
        }
        dstate[(((long)b * n_his + t) * N + n) * 3 + c] = v;
    }
}

// Data gradients from dXn = dH1 * W0 (rows x 6, columns [attr(2), phys, action(3)]): column 2 is dLoss/dphys of the object
// particles (the forward pads the tool rows with a constant zero, model.py:206-207, so rows i >= n_p get zero), columns 3..5
// dLoss/daction of every row (model.py:223).  Either output may be null.
__global__ void k_input_grad(const float* dxn, int B, int N, int n_p, float* gphys, float* gaction) {
    const long r = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= (long)B * N) return;
    if (gphys) gphys[r] = (int)(r % N) < n_p ? dxn[r * 6 + 2] : 0.f;
    if (gaction) { gaction[r * 3] = dxn[r * 6 + 3]; gaction[r * 3 + 1] = dxn[r * 6 + 4]; gaction[r * 3 + 2] = dxn[r * 6 + 5]; }
}

inline unsigned blocks(long n, int t = 256) { return (unsigned)((n + t - 1) / t); }

// ---------------------------------------------------------------------------------------------------------- host helpers
struct Ctx { hipStream_t st; float* slab; double* part; bool want_w; bool wide; };   // want_w false: no weight gradient is wanted, linear_dw is skipped; wide: k_reduce

// C (M x N) = A (M x K) * B (K x N) with the epilogue of GemmArgs
hipError_t gemm(hipStream_t st, GemmArgs a) {
    if (a.M <= 0 || a.N <= 0) return hipSuccess;
    if (a.kslab <= 0) a.kslab = ((a.K + TK - 1) / TK) * TK;
    const unsigned nz = (unsigned)std::max(1, (a.K + a.kslab - 1) / a.kslab);
    hipLaunchKernelGGL(k_gemm, dim3((unsigned)((a.M + TM - 1) / TM), (unsigned)((a.N + TN - 1) / TN), nz), dim3(256), 0, st, a);
    return hipGetLastError();
}

GemmArgs ga() { GemmArgs a{}; a.ones_col = -1; return a; }

// Y (rows x out) = X (rows x in, pitch ldx) * W^T (+ bias) (+ add) [relu]; W row-major (out, ldw) starting at column wcol0
hipError_t linear(hipStream_t st, const float* X, long ldx, long rows, int in, const float* W, int ldw, int wcol0, int out,
                  const float* bias, float* Y, long ldy, bool relu, const float* add = nullptr, int accumulate = 0) {
    GemmArgs a = ga();
    a.A = X; a.sam = ldx; a.sak = 1;
    a.Bm = W + wcol0; a.sbk = 1; a.sbn = ldw;
    a.M = (int)rows; a.N = out; a.K = in;
    a.C = Y; a.ldc = ldy; a.bias = bias; a.add = add; a.ld_add = ldy; a.accumulate = accumulate; a.relu = relu;
    return gemm(st, a);
}

// dX (rows x in) (=|+=) dY (rows x out) * W[:, wcol0:wcol0+in] [+ add] [kept where mask > 0]
hipError_t linear_dx(hipStream_t st, const float* dY, long lddy, long rows, int out, const float* W, int ldw, int wcol0, int in,
                     float* dX, long lddx, int accumulate, const float* mask, long ldmask, const float* add = nullptr) {
    GemmArgs a = ga();
    a.A = dY; a.sam = lddy; a.sak = 1;
    a.Bm = W + wcol0; a.sbk = ldw; a.sbn = 1;
    a.M = (int)rows; a.N = in; a.K = out;
    a.C = dX; a.ldc = lddx; a.accumulate = accumulate; a.mask = mask; a.ld_mask = ldmask; a.add = add; a.ld_add = lddx;
    return gemm(st, a);
}

// gW[:, col0:col0+in] += dY^T X and (if gb) gb += column sums of dY, over `rows` rows: split-K slabs reduced in slab order
hipError_t linear_dw(const Ctx& c, const float* dY, long lddy, long rows, int out, const float* X, long ldx, int in, float* gW,
                     int ldw, int col0, float* gb) {
    if (rows <= 0 || !c.want_w) return hipSuccess;
    const int ncols = in + (gb ? 1 : 0);
    // short fma chains: slabs of 32 rows (one K tile), more only beyond 1024 slabs (32,768 rows)
    const int kslab = (int)(TK * ((rows + (long)TK * kMaxSlabs - 1) / ((long)TK * kMaxSlabs)));
    const int nz = (int)((rows + kslab - 1) / kslab);
    GemmArgs a = ga();
    a.A = dY; a.sam = 1; a.sak = lddy;
    a.Bm = X; a.sbk = ldx; a.sbn = 1; a.ones_col = gb ? in : -1;
    a.M = out; a.N = ncols; a.K = (int)rows; a.kslab = kslab;
    a.C = c.slab; a.ldc = ncols; a.slab_stride = (long)out * ncols;
    hipError_t e = gemm(c.st, a);
    if (e != hipSuccess) return e;
    const int elems = out * ncols, ng = (nz + kSlabGroup - 1) / kSlabGroup;
    hipLaunchKernelGGL(k_reduce_part, dim3(blocks(elems), (unsigned)ng), dim3(256), 0, c.st, c.slab, elems, nz, c.part);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(k_reduce, dim3(blocks(elems)), dim3(256), 0, c.st, c.part, out, ncols, ng, gW, ldw, col0, in, gb, c.wide ? 1 : 0);
    return hipGetLastError();
}

}  // namespace

// ------------------------------------------------------------------------------------------------------------ driver
// slabs of the widest reduction (150 x (150 + bias)), then the fp64 group partials behind them
size_t train_slab_floats() { return (size_t)kMaxSlabs * NF * (NF + 1) + 2 * (size_t)(kMaxSlabs / kSlabGroup) * NF * (NF + 1); }

size_t train_work_floats(int Bc, int N, int Ep, int n_his, int pstep) {
    const size_t n = (size_t)Bc * N, e = (size_t)Bc * Ep;
    const size_t R = 5 + 3 * n_his;
    size_t f = 0;
    f += n * 6 + n * NF * (3 + (pstep + 1) + pstep + 2) + n * 3 * 2;   // xn, ph1, ph2, penc, eff[0..P], agg[0..P-1], hd0, hd1, motion, gm
    f += n * NF * 6 + n * 2 * NF;                                      // U, V, dq, T, dpenc, dagg, S2
    f += n * 3 * n_his;                                                // dsnt
    f += e * R * 2 + e * NF * (4 + pstep) + e * NF * 3;                // xe, dxe, rh1, rh2, renc, C, er[0..P-1], dpre, dren, dtmp
    f += 64 * 64;                                                      // take() rounds every buffer up to 64 floats
    return f;
}
size_t train_work_ints(int Bc, int N, int Ep) { return (size_t)Bc * (N + 1) + (size_t)Bc * Ep + (size_t)Bc * N + 256 * 4; }

hipError_t train_backward_chunk(const TrainArgs& t, int b0, int nb, float* wsf, int* wsi, float* slab, hipStream_t st) {
    const int N = t.N, n_p = t.n_p, Ep = t.Ep, n_his = t.n_his, P = t.pstep;
    const int R = 5 + 3 * n_his;
    const long n = (long)nb * N, ne = (long)nb * Ep;
    const float* const* W = t.w;
    float* const* G = t.g;
    Ctx c{st, slab, reinterpret_cast<double*>(slab + (size_t)kMaxSlabs * NF * (NF + 1)), t.want_w, t.wide};
    size_t off = 0;
    auto take = [&](size_t k) { float* p = wsf + off; off += (k + 63) / 64 * 64; return p; };
    float* xn = take(n * 6); float* ph1 = take(n * NF); float* ph2 = take(n * NF); float* penc = take(n * NF);
    float* eff[8]; eff[0] = penc;
    for (int r = 1; r <= P; ++r) eff[r] = take(n * NF);
    float* agg[8]; for (int r = 0; r < P; ++r) agg[r] = take(n * NF);
    float* hd0 = take(n * NF); float* hd1 = take(n * NF); float* mot = take(n * 3); float* gm = take(n * 3);
    float* U = take(n * NF); float* V = take(n * NF); float* dq = take(n * NF); float* T = take(n * NF);
    float* dpenc = take(n * NF); float* dagg = take(n * NF); float* S2 = take(n * 2 * NF); float* dsnt = take(n * 3 * n_his);
    float* xe = take(ne * R); float* dxe = take(ne * R);
    float* rh1 = take(ne * NF); float* rh2 = take(ne * NF); float* renc = take(ne * NF); float* Cb = take(ne * NF);
    float* er[8]; for (int r = 0; r < P; ++r) er[r] = take(ne * NF);
    float* dpre = take(ne * NF); float* dren = take(ne * NF); float* dtmp = take(ne * NF);
    int* sptr = wsi; int* sidx = sptr + (size_t)nb * (N + 1); int* cur = sidx + (size_t)nb * Ep;

    const float* state = t.state + (long)b0 * n_his * N * 3;
    const float* attrs = t.attrs + (long)b0 * N * 2;
    const float* group = t.group + (long)b0 * N * t.n_inst;
    const int* recv = t.recv + (long)b0 * t.edge_cap; const int* send = t.send + (long)b0 * t.edge_cap;
    const int* row_ptr = t.row_ptr + (long)b0 * (N + 1); const int* n_edges = t.n_edges + b0;
    const float* dpos = t.dpos ? t.dpos + (long)b0 * n_p * 3 : nullptr;
    const float* dmot = t.dmot ? t.dmot + (long)b0 * n_p * 3 : nullptr;
    hipError_t e;
#define TRY(x) do { e = (x); if (e != hipSuccess) return e; } while (0)
#define LAUNCH(k, n_, ...) do { hipLaunchKernelGGL(k, dim3(blocks(n_)), dim3(256), 0, st, __VA_ARGS__); TRY(hipGetLastError()); } while (0)

    // ---- recompute (model.py:156-330)
    LAUNCH(k_train_prep_node, n, attrs, t.phys + (long)b0 * N, t.action + (long)b0 * N * 3, n, xn);
    LAUNCH(k_train_prep_edge, ne, state, attrs, group, t.n_inst, recv, send, n_edges, t.edge_cap, nb, N, Ep, n_his, xe);
    hipLaunchKernelGGL(k_send_csr, dim3(nb), dim3(64), 0, st, send, n_edges, t.edge_cap, N, Ep, sptr, sidx, cur);
    TRY(hipGetLastError());
    TRY(linear(st, xn, 6, n, 6, W[0], 6, 0, NF, W[1], ph1, NF, true));
    TRY(linear(st, ph1, NF, n, NF, W[2], NF, 0, NF, W[3], ph2, NF, true));
    TRY(linear(st, ph2, NF, n, NF, W[4], NF, 0, NF, W[5], penc, NF, true));
    TRY(linear(st, xe, R, ne, R, W[6], R, 0, NF, W[7], rh1, NF, true));
    TRY(linear(st, rh1, NF, ne, NF, W[8], NF, 0, NF, W[9], rh2, NF, true));
    TRY(linear(st, rh2, NF, ne, NF, W[10], NF, 0, NF, W[11], renc, NF, true));
    const float* Wpp = W[12]; const float* Wrp = W[14];
    TRY(linear(st, renc, NF, ne, NF, Wrp, 3 * NF, 0, NF, W[15], Cb, NF, false));
    for (int r = 0; r < P; ++r) {
        TRY(linear(st, eff[r], NF, n, NF, Wrp, 3 * NF, NF, NF, nullptr, U, NF, false));
        TRY(linear(st, eff[r], NF, n, NF, Wrp, 3 * NF, 2 * NF, NF, nullptr, V, NF, false));
        LAUNCH(k_edge_act, ne * NF, Cb, U, V, recv, send, n_edges, t.edge_cap, nb, N, Ep, er[r]);
        LAUNCH(k_segsum, n * NF, er[r], NF, 0, NF, row_ptr, (const int*)nullptr, n_edges, nb, N, Ep, 1.f, 0, agg[r], NF, 0);
        TRY(linear(st, penc, NF, n, NF, Wpp, 2 * NF, 0, NF, W[13], eff[r + 1], NF, false, eff[r]));
        TRY(linear(st, agg[r], NF, n, NF, Wpp, 2 * NF, NF, NF, nullptr, eff[r + 1], NF, true, nullptr, 1));
    }
    TRY(linear(st, eff[P], NF, n, NF, W[16], NF, 0, NF, W[17], hd0, NF, true));
    TRY(linear(st, hd0, NF, n, NF, W[18], NF, 0, NF, W[19], hd1, NF, true));
    TRY(linear(st, hd1, NF, n, NF, W[20], NF, 0, 3, W[21], mot, 3, false));

    // ---- head (model.py:335-338)
    LAUNCH(k_head_grad, n * 3, mot, dpos, dmot, nb, N, n_p, t.clamp, gm);
    TRY(linear_dw(c, gm, 3, n, 3, hd1, NF, NF, G[20], NF, 0, G[21]));
    TRY(linear_dx(st, gm, 3, n, 3, W[20], NF, 0, NF, T, NF, 0, hd1, NF));
    TRY(linear_dw(c, T, NF, n, NF, hd0, NF, NF, G[18], NF, 0, G[19]));
    TRY(linear_dx(st, T, NF, n, NF, W[18], NF, 0, NF, dq, NF, 0, hd0, NF));
    TRY(linear_dw(c, dq, NF, n, NF, eff[P], NF, NF, G[16], NF, 0, G[17]));
    TRY(linear_dx(st, dq, NF, n, NF, W[16], NF, 0, NF, T, NF, 0, eff[P], NF));   // T = dq of the last round
    std::swap(T, dq);

    // ---- message passing, last round first.  dq = gradient at the pre-ReLU particle propagator output of round r
    for (int r = P - 1; r >= 0; --r) {
        TRY(linear_dw(c, dq, NF, n, NF, penc, NF, NF, G[12], 2 * NF, 0, G[13]));
        TRY(linear_dw(c, dq, NF, n, NF, agg[r], NF, NF, G[12], 2 * NF, NF, nullptr));
        TRY(linear_dx(st, dq, NF, n, NF, Wpp, 2 * NF, 0, NF, dpenc, NF, r < P - 1, nullptr, 0));
        TRY(linear_dx(st, dq, NF, n, NF, Wpp, 2 * NF, NF, NF, dagg, NF, 0, nullptr, 0));
        LAUNCH(k_edge_dpre, ne * NF, dagg, er[r], recv, n_edges, t.edge_cap, nb, N, Ep, dpre);
        TRY(linear_dw(c, dpre, NF, ne, NF, renc, NF, NF, G[14], 3 * NF, 0, G[15]));
        TRY(linear_dx(st, dpre, NF, ne, NF, Wrp, 3 * NF, 0, NF, dren, NF, r < P - 1, r == 0 ? renc : nullptr, NF));
        LAUNCH(k_segsum, n * NF, dpre, NF, 0, NF, row_ptr, (const int*)nullptr, n_edges, nb, N, Ep, 1.f, 0, S2, 2 * NF, 0);
        LAUNCH(k_segsum, n * NF, dpre, NF, 0, NF, sptr, (const int*)sidx, n_edges, nb, N, Ep, 1.f, 0, S2, 2 * NF, NF);
        TRY(linear_dw(c, S2, 2 * NF, n, NF, eff[r], NF, NF, G[14], 3 * NF, NF, nullptr));
        TRY(linear_dw(c, S2 + NF, 2 * NF, n, NF, eff[r], NF, NF, G[14], 3 * NF, 2 * NF, nullptr));
        // dEff_r = dq (residual) + W2^T SR + W3^T SS; masked by eff_r > 0 it is the dq of round r-1
        TRY(linear_dx(st, S2, 2 * NF, n, NF, Wrp, 3 * NF, NF, NF, T, NF, 0, nullptr, 0, dq));
        TRY(linear_dx(st, S2 + NF, 2 * NF, n, NF, Wrp, 3 * NF, 2 * NF, NF, T, NF, 1, r > 0 ? eff[r] : nullptr, NF));
        std::swap(T, dq);
    }
    // ---- particle encoder: dPenc = dEff_0 + sum_r Wa^T dq_r, through its ReLU (model.py:297)
    LAUNCH(k_add_mask, n * NF, dq, dpenc, penc, n * NF, T);
    TRY(linear_dw(c, T, NF, n, NF, ph2, NF, NF, G[4], NF, 0, G[5]));
    TRY(linear_dx(st, T, NF, n, NF, W[4], NF, 0, NF, dq, NF, 0, ph2, NF));
    TRY(linear_dw(c, dq, NF, n, NF, ph1, NF, NF, G[2], NF, 0, G[3]));
    TRY(linear_dx(st, dq, NF, n, NF, W[2], NF, 0, NF, T, NF, 0, ph1, NF));
    TRY(linear_dw(c, T, NF, n, NF, xn, 6, 6, G[0], 6, 0, G[1]));
    // ---- data gradients (ag_backward_inputs): dXn = dH1 * W0 into dq, which nothing reads any more (model.py:206-223)
    if (t.dphys || t.daction) {
        TRY(linear_dx(st, T, NF, n, NF, W[0], 6, 0, 6, dq, 6, 0, nullptr, 0));
        LAUNCH(k_input_grad, n, dq, nb, N, n_p, t.dphys ? t.dphys + (long)b0 * N : nullptr,
               t.daction ? t.daction + (long)b0 * N * 3 : nullptr);
    }
    // ---- relation encoder (model.py:303); dren already carries the ReLU mask of renc
    TRY(linear_dw(c, dren, NF, ne, NF, rh2, NF, NF, G[10], NF, 0, G[11]));
    TRY(linear_dx(st, dren, NF, ne, NF, W[10], NF, 0, NF, dtmp, NF, 0, rh2, NF));
    TRY(linear_dw(c, dtmp, NF, ne, NF, rh1, NF, NF, G[8], NF, 0, G[9]));
    TRY(linear_dx(st, dtmp, NF, ne, NF, W[8], NF, 0, NF, dpre, NF, 0, rh1, NF));
    TRY(linear_dw(c, dpre, NF, ne, NF, xe, R, R, G[6], R, 0, G[7]));
    // ---- state: only the position differences of the relation input carry it (+ receiver, - sender; model.py:277-282)
    if (t.dstate) {
        TRY(linear_dx(st, dpre, NF, ne, NF, W[6], R, 0, R, dxe, R, 0, nullptr, 0));
        const int F = 3 * n_his;
        LAUNCH(k_segsum, n * F, dxe, R, 5, F, row_ptr, (const int*)nullptr, n_edges, nb, N, Ep, 1.f, 0, dsnt, F, 0);
        LAUNCH(k_segsum, n * F, dxe, R, 5, F, sptr, (const int*)sidx, n_edges, nb, N, Ep, -1.f, 1, dsnt, F, 0);
        LAUNCH(k_dstate, n * 3, dsnt, dpos, nb, N, n_p, n_his, t.dstate + (long)b0 * n_his * N * 3);
    }
#undef LAUNCH
#undef TRY
    return hipSuccess;
}

}  // namespace ag
