// The "tool to all non-fixed particles" rule of construct_edges_from_states (reference src/dynamics/dataset/graph.py:125-171) and
// its flat kNN filter for B graphs in ONE launch.  gfx950 only.
//
// Semantics are ag_rules.hip's (k_rule_prep / k_rule_dis / k_rule_rank / k_rule_apply) with the subset S = mask AND (y > thr)
// formed here, thr from a per-graph bounds source (graph.py:134 on rollout.py:132-139's max_y / min_y).  One workgroup owns one
// graph; the tool list, the pair tables and the per-particle flags live in LDS, nothing is kept in global scratch, and a graph
// reads nothing of its neighbours.  Phases:
//   guard     : base edge list and tool count are checked before any index from device memory is used  (-> n_out = -1)
//   threshold : max / min of the bounds rows' y (NaN propagates as np.max does), thr in four separately rounded fp32 operations
//   contact   : does the base list hold a tool-sender edge (graph.py:128-135)?  no: the base graph is copied through
//   pairs     : fp32 distance of every (receiver in S, tool) pair, row-major = the reference's flat order    (0 < kNN < 1 only)
//   rank      : rank of each pair by (distance, flat index) -> keep flag                                     (0 < kNN < 1 only)
//   merge     : per receiver row, base senders and tool senders merged in index order; count -> scan -> write
// Integer counters only; no float atomics.
// k_surface_graphs, below, is the two-closest-planes rule (graph.py:175-221) in the same pattern; it shares the guard and the merge.
#include <math.h>
#include "ag_common.h"

namespace ag {

constexpr int GW = 1024;                 // one workgroup of 16 wavefronts per graph: the rank phase is O(pairs^2) and sets its time
constexpr int RG_MAX_N = 4096;
constexpr float RG_BIG = 1e10f;              // graph.py:92,96

__device__ __forceinline__ int rg_excl_scan(int* sh, int v) {   // GW threads, returns exclusive prefix; sh[GW-1] = total
    __syncthreads();                                             // sh may still be read from an earlier use
    sh[threadIdx.x] = v;
    __syncthreads();
    for (int off = 1; off < GW; off <<= 1) {
        int t = 0;
        if ((int)threadIdx.x >= off) t = sh[threadIdx.x - off];
        __syncthreads();
        sh[threadIdx.x] += t;
        __syncthreads();
    }
    return sh[threadIdx.x] - v;
}

// One receiver row: walks the base senders (ascending) and the tool list (ascending) as one merged sequence (ag_rules.hip:
// rule_row).  apply = false copies the base row through.  flag: bit 0 in S, bit 1 tool.
template <bool WRITE>
__device__ __forceinline__ int rg_row(const int* send_in, int e, int e1, const uint8_t* flag, const int* tl, const uint8_t* kept,
                                      int i, int M, bool apply, bool use_knn, int* recv, int* send, int out) {
    const bool i_tool = flag[i] & 2, i_sub = flag[i] & 1;
    int m = apply ? 0 : M, n = 0;
    while (e < e1 || m < M) {
        const int sj = e < e1 ? send_in[e] : 0x7fffffff;
        const int tj = m < M ? tl[m] : 0x7fffffff;
        const int j = min(sj, tj);
        const bool base = sj == j;
        bool on;
        if (tj == j) {                                                  // tool sender
            on = base;
            if (i_sub) on = use_knn ? kept[i * M + m] != 0 : true;      // graph.py:154,168
            if (i_tool) on = false;                                     // graph.py:170
            ++m;
        } else {
            on = base && !(apply && i_tool && (flag[j] & 1));           // graph.py:153
        }
        if (base) ++e;
        if (on) {
            if (WRITE) { recv[out + n] = i; send[out + n] = j; }
            ++n;
        }
    }
    return n;
}

// The guard both kernels of this file share: the input list as ag_build_edges_graphs (or the sibling rule) writes it - count within
// [0, base_cap], rows ascending from 0 to the count, senders strictly ascending within [0, N) - and the tool count, checked before
// any index from device memory is used.  Fills tl with the first M tool indices, ascending.  Returns the verdict on every thread.
__device__ __forceinline__ bool rg_guard(const int* send_in, const int* rp_in, const uint8_t* tool, int nb, int base_cap, int N, int M,
                                         int i0, int i1, int* s_scan, int* tl) {
    const int t = threadIdx.x;
    int bad = (nb < 0 || nb > base_cap) ? 1 : 0;
    if (!bad) {                                                         // nb is uniform over the workgroup
        for (int i = i0; i < i1; ++i) {
            const int e0 = rp_in[i], e1 = rp_in[i + 1];
            if (e0 < 0 || e1 < e0 || e1 > nb) { bad = 1; continue; }
            int prev = -1;
            for (int e = e0; e < e1; ++e) {
                const int j = send_in[e];
                if (j <= prev || j >= N) bad = 1;
                prev = max(prev, j);
            }
        }
        if (t == 0 && (rp_in[0] != 0 || rp_in[N] != nb)) bad = 1;
    }
    int c = 0;
    for (int i = i0; i < i1; ++i) c += tool[i] ? 1 : 0;
    int r = rg_excl_scan(s_scan, c);
    const int ntool = s_scan[GW - 1];
    for (int i = i0; i < i1; ++i)
        if (tool[i] && r < M) tl[r++] = i;
    if (ntool != M) bad = 1;
    return __syncthreads_or(bad) != 0;
}

// The merge both kernels end with: count -> scan -> write.  *n_out is the TRUE count even when nothing was written.
__device__ __forceinline__ void rg_merge(const int* send_in, const int* rp_in, const uint8_t* flag, const int* tl, const uint8_t* kept,
                                         int* s_scan, int N, int M, int i0, int i1, bool apply, bool use_knn, int edge_cap, int* recv,
                                         int* send, int* row_ptr, int* n_out) {
    int mine = 0;
    for (int i = i0; i < i1; ++i)
        mine += rg_row<false>(send_in, rp_in[i], rp_in[i + 1], flag, tl, kept, i, M, apply, use_knn, nullptr, nullptr, 0);
    int run = rg_excl_scan(s_scan, mine);
    const int total = s_scan[GW - 1];
    if (total <= edge_cap) {
        for (int i = i0; i < i1; ++i) {
            row_ptr[i] = run;
            run += rg_row<true>(send_in, rp_in[i], rp_in[i + 1], flag, tl, kept, i, M, apply, use_knn, recv, send, run);
        }
        if (threadIdx.x == 0) row_ptr[N] = total;
    }
    if (threadIdx.x == 0) *n_out = total;
}

__global__ __launch_bounds__(GW) void k_rule_graphs(RuleGraphsArgs a) {
    __shared__ float s_dis[RULE_GRAPHS_MAX_PAIRS];
    __shared__ uint8_t s_keep[RULE_GRAPHS_MAX_PAIRS];     // 1 = pair of the rule, 2 = not
    __shared__ uint8_t s_kept[RULE_GRAPHS_MAX_PAIRS];     // verdict of the kNN filter
    __shared__ uint8_t s_flag[RG_MAX_N];
    __shared__ int s_scan[GW];
    __shared__ int s_tl[RULE_GRAPHS_MAX_TOOLS];
    const int b = blockIdx.x, t = threadIdx.x, N = a.N, M = a.n_tools;
    const float* pos = a.pos + (long)b * a.pos_bstride;
    const uint8_t* mask = a.mask + (long)b * N;
    const uint8_t* tool = a.tool + (long)b * N;
    const int* send_in = a.send_in + (long)b * a.base_cap;
    const int* rp_in = a.row_ptr_in + (long)b * (N + 1);
    const int nb = a.n_edges_in[b];
    const int per = (N + GW - 1) / GW;
    const int i0 = min(N, t * per), i1 = min(N, i0 + per);

    if (rg_guard(send_in, rp_in, tool, nb, a.base_cap, N, M, i0, i1, s_scan, s_tl)) {   // refuse, loudly: -1 and nothing else
        if (t == 0) a.n_out[b] = -1;
        return;
    }

    // ---- threshold (the reduce borrows s_dis, which the pair phase fills later)
    int n = max(a.bnd_n[b], 0);
    if (a.bnd_idx) n = min(n, a.idx_stride);
    const long first = a.bnd_first[b];
    float mx = -INFINITY, mn = INFINITY;
    int nan = 0, any = 0;
    for (int q = t; q < n; q += GW) {
        long pt = first + (a.bnd_idx ? (long)a.bnd_idx[(long)b * a.idx_stride + q] : (long)q);
        pt = min(max(pt, 0L), a.bnd_points - 1);
        const float y = a.bnd_pos[3 * pt + 1];
        if (y != y) nan = 1;
        else { mx = fmaxf(mx, y); mn = fminf(mn, y); }
        any = 1;
    }
    if (t == 0 && a.pad_rows > n) { mx = fmaxf(mx, 0.0f); mn = fminf(mn, 0.0f); any = 1; }   // the padding's zero rows
    s_dis[t] = mx; s_dis[GW + t] = mn;
    nan = __syncthreads_or(nan);
    any = __syncthreads_or(any);
    for (int off = GW / 2; off > 0; off >>= 1) {
        if (t < off) { s_dis[t] = fmaxf(s_dis[t], s_dis[t + off]); s_dis[GW + t] = fminf(s_dis[GW + t], s_dis[GW + t + off]); }
        __syncthreads();
    }
    mx = s_dis[0]; mn = s_dis[GW];
    if (nan || !any) mx = mn = NAN;                                     // np.max propagates NaN; no row at all: empty subset
    const float thr = __fadd_rn(__fmul_rn(__fsub_rn(__fmul_rn(mx, a.ratio), mn), 0.1f), mn);   // rollout.py:136, graph.py:134
    if (t == 0 && a.thr_out) a.thr_out[b] = thr;
    __syncthreads();

    // ---- per-particle flags, contact check
    for (int i = t; i < N; i += GW) {
        const bool mk = mask[i] != 0;
        s_flag[i] = (uint8_t)(((mk && pos[3 * i + 1] > thr) ? 1 : 0) | (tool[i] ? 2 : 0));
    }
    __syncthreads();
    int touch = 0;
    for (int e = t; e < nb; e += GW) touch |= (s_flag[send_in[e]] & 2) ? 1 : 0;   // senders were bounded by the guard
    const bool apply = __syncthreads_or(touch) != 0;                    // graph.py:128-135
    const double kNN = a.kNN[b];
    const bool use_knn = apply && M > 0 && kNN < 1.0 && kNN > 0.0;      // graph.py:156

    // ---- pair distances and the flat kNN filter
    if (use_knn) {
        const int P = N * M;
        int cnt = 0;
        for (int p = t; p < P; p += GW) {
            const int i = p / M, j = s_tl[p % M];
            if (!(s_flag[i] & 1)) { s_keep[p] = 2; s_dis[p] = 0.0f; continue; }
            float d = RG_BIG;
            if (mask[j] && !((s_flag[i] & 2) && (s_flag[j] & 2))) {     // graph.py:89-96
                const float dx = __fsub_rn(pos[3 * i], pos[3 * j]), dy = __fsub_rn(pos[3 * i + 1], pos[3 * j + 1]),
                            dz = __fsub_rn(pos[3 * i + 2], pos[3 * j + 2]);
                d = __fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz));   // graph.py:87-88
            }
            s_dis[p] = d;
            s_keep[p] = 1;
            ++cnt;
        }
        (void)rg_excl_scan(s_scan, cnt);                                // also the barrier behind the pair tables
        const int keepK = (int)(kNN * (double)s_scan[GW - 1]);          // graph.py:160 int(kNN * count)
        for (int p = t; p < P; p += GW) {
            if (s_keep[p] == 2) continue;
            const float dp = s_dis[p];
            int rank = 0;
            for (int q = 0; q < P; ++q)
                rank += (s_keep[q] != 2 && (s_dis[q] < dp || (s_dis[q] == dp && q < p))) ? 1 : 0;
            s_kept[p] = rank < keepK ? 1 : 0;
        }
    }
    __syncthreads();

    rg_merge(send_in, rp_in, s_flag, s_tl, s_kept, s_scan, N, M, i0, i1, apply, use_knn, a.edge_cap, a.recv + (long)b * a.edge_cap,
             a.send + (long)b * a.edge_cap, a.row_ptr + (long)b * (N + 1), a.n_out + b);
}

hipError_t launch_rule_graphs(const RuleGraphsArgs& a, hipStream_t st) {
    hipLaunchKernelGGL(k_rule_graphs, dim3((unsigned)a.B), dim3(GW), 0, st, a);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------------------------------
// "Tool to the two closest surface planes" (reference src/dynamics/dataset/graph.py:175-221) for B graphs in one launch, decision
// for decision what construct_edges_from_states' surface branch does on the host for one graph.  Phases:
//   guard   : rg_guard, as k_rule_graphs                                                                  (-> n_out = -1)
//   bounds  : max / min of x, y, z over the bounds rows (per axis, NaN propagates as np.max does), then the six bounds in separately
//             rounded fp32 operations; order 0 = the step loop's (rollout.py:132-139: min_x / min_z from the SCALED maxima), order 1
//             = construct_graph's (rollout/graph.py:446-458: from the UNSCALED maxima, the maxima scaled afterwards)
//   contact : check = tool-sender edges of the INPUT list (graph.py:180-181); 0: the input graph is copied through
//   planes  : graph.py:190-197 index s_receiv with the 0 / 1 VALUES of adj[obj_tool_mask_2], so each of its (#mask * n_tools) entries
//             selects particle 0 or particle 1, broadcast over N senders: value = N * (n0 * d_0 + n1 * d_1) in fp64, d_k the fp32
//             squared distance of particle k to the plane; the two smallest by (value, index), NaN last = np.argsort on five values
//   merge   : S = side(first) AND side(second) AND mask; rg_merge without the kNN filter
// LDS: the particle flags, the scan, the tool list and a per-wavefront reduction scratch (about 8.5 KB).
constexpr int SG_WAVES = GW / 64;

__device__ __forceinline__ bool sg_side(int plane, float x, float y, float z, const float* bd) {   // graph.py:47-66; bd as bounds_out
    switch (plane) {
        case 0: return y >= bd[0];      // max_y
        case 1: return x <= bd[4];      // min_x
        case 2: return x >= bd[2];      // max_x
        case 3: return z <= bd[5];      // min_z
        default: return z >= bd[3];     // max_z
    }
}

__global__ __launch_bounds__(GW) void k_surface_graphs(SurfaceGraphsArgs a) {
    __shared__ uint8_t s_flag[RG_MAX_N];
    __shared__ int s_scan[GW];
    __shared__ int s_tl[RULE_GRAPHS_MAX_TOOLS];
    __shared__ float s_red[6][SG_WAVES];
    __shared__ int s_cnt[2];
    const int b = blockIdx.x, t = threadIdx.x, N = a.N, M = a.n_tools;
    const float* pos = a.pos + (long)b * a.pos_bstride;
    const uint8_t* mask = a.mask + (long)b * N;
    const uint8_t* tool = a.tool + (long)b * N;
    const int* send_in = a.send_in + (long)b * a.base_cap;
    const int* rp_in = a.row_ptr_in + (long)b * (N + 1);
    const int nb = a.n_edges_in[b];
    const int per = (N + GW - 1) / GW;
    const int i0 = min(N, t * per), i1 = min(N, i0 + per);

    if (rg_guard(send_in, rp_in, tool, nb, a.base_cap, N, M, i0, i1, s_scan, s_tl)) {
        if (t == 0) a.n_out[b] = -1;
        return;
    }

    // ---- bounds
    int n = max(a.bnd_n[b], 0);
    if (a.bnd_idx) n = min(n, a.idx_stride);
    const long first = a.bnd_first[b];
    float ext[6] = {-INFINITY, -INFINITY, -INFINITY, INFINITY, INFINITY, INFINITY};   // max x y z, min x y z
    int nan = 0, any = 0;                                                             // nan: bit per axis
    for (int q = t; q < n; q += GW) {
        long pt = first + (a.bnd_idx ? (long)a.bnd_idx[(long)b * a.idx_stride + q] : (long)q);
        pt = min(max(pt, 0L), a.bnd_points - 1);
        for (int ax = 0; ax < 3; ++ax) {
            const float v = a.bnd_pos[3 * pt + ax];
            if (v != v) nan |= 1 << ax;
            else { ext[ax] = fmaxf(ext[ax], v); ext[3 + ax] = fminf(ext[3 + ax], v); }
        }
        any = 1;
    }
    if (t == 0 && a.pad_rows > n) {                                                   // the padding's zero rows
        for (int ax = 0; ax < 3; ++ax) { ext[ax] = fmaxf(ext[ax], 0.0f); ext[3 + ax] = fminf(ext[3 + ax], 0.0f); }
        any = 1;
    }
    for (int off = 32; off > 0; off >>= 1)
        for (int k = 0; k < 6; ++k) {
            const float o = __shfl_xor(ext[k], off, 64);
            ext[k] = k < 3 ? fmaxf(ext[k], o) : fminf(ext[k], o);
        }
    if ((t & 63) == 0)
        for (int k = 0; k < 6; ++k) s_red[k][t >> 6] = ext[k];
    if (t < 2) s_cnt[t] = 0;
    const int nan_x = __syncthreads_or(nan & 1), nan_y = __syncthreads_or(nan & 2), nan_z = __syncthreads_or(nan & 4);
    any = __syncthreads_or(any);                                                      // (also the barrier behind s_red / s_cnt)
    for (int k = 0; k < 6; ++k) {
        float v = s_red[k][0];
        for (int w = 1; w < SG_WAVES; ++w) v = k < 3 ? fmaxf(v, s_red[k][w]) : fminf(v, s_red[k][w]);
        ext[k] = v;
    }
    if (nan_x || !any) ext[0] = ext[3] = NAN;                                         // np.max propagates NaN; no row at all: empty subset
    if (nan_y || !any) ext[1] = ext[4] = NAN;
    if (nan_z || !any) ext[2] = ext[5] = NAN;
    float bd[6];                                                                      // max_y, min_y, max_x, max_z, min_x, min_z
    const float r = a.ratio, q1 = a.one_minus_ratio;
    bd[0] = __fmul_rn(ext[1], r); bd[1] = ext[4]; bd[2] = __fmul_rn(ext[0], r); bd[3] = __fmul_rn(ext[2], r);
    const float hx = a.bounds_order ? ext[0] : bd[2], hz = a.bounds_order ? ext[2] : bd[3];
    bd[4] = __fadd_rn(__fmul_rn(__fsub_rn(hx, ext[3]), q1), ext[3]);
    bd[5] = __fadd_rn(__fmul_rn(__fsub_rn(hz, ext[5]), q1), ext[5]);
    if (t < 6 && a.bounds_out) a.bounds_out[(long)b * 6 + t] = bd[t];

    // ---- contact: tool-sender edges of the input list, valid particles
    for (int i = t; i < N; i += GW) s_flag[i] = (uint8_t)(tool[i] ? 2 : 0);
    __syncthreads();
    int check = 0, nmask = 0;
    for (int e = t; e < nb; e += GW) check += (s_flag[send_in[e]] & 2) ? 1 : 0;       // senders were bounded by the guard
    for (int i = t; i < N; i += GW) nmask += mask[i] ? 1 : 0;
    if (check) atomicAdd(&s_cnt[0], check);
    if (nmask) atomicAdd(&s_cnt[1], nmask);
    __syncthreads();
    check = s_cnt[0]; nmask = s_cnt[1];
    const bool apply = check > 0;                                                     // graph.py:188

    // ---- planes (uniform over the workgroup) and the subset
    int p1 = -1, p2 = -1;
    if (apply) {
        const double n1 = (double)check, n0 = (double)((long)nmask * M - check);
        const int k1 = min(1, N - 1);
        const int axis[5] = {1, 0, 0, 2, 2};
        const float bound[5] = {bd[0], bd[4], bd[2], bd[5], bd[3]};                   // max_y, min_x, max_x, min_z, max_z (graph.py:40)
        double val[5];
        for (int k = 0; k < 5; ++k) {
            const float e0 = __fsub_rn(pos[axis[k]], bound[k]), e1 = __fsub_rn(pos[3 * k1 + axis[k]], bound[k]);
            const double d0 = (double)__fmul_rn(e0, e0), d1 = (double)__fmul_rn(e1, e1);
            val[k] = __dmul_rn((double)N, __dadd_rn(__dmul_rn(n0, d0), __dmul_rn(n1, d1)));
        }
        for (int k = 0; k < 5; ++k) {                                                 // rank by (value, index), NaN last
            int rank = 0;
            for (int j = 0; j < 5; ++j) {
                const bool kn = val[k] != val[k], jn = val[j] != val[j];
                const bool before = jn ? (kn && j < k) : (kn || val[j] < val[k] || (val[j] == val[k] && j < k));
                rank += (j != k && before) ? 1 : 0;
            }
            if (rank == 0) p1 = k;
            if (rank == 1) p2 = k;
        }
        for (int i = t; i < N; i += GW) {
            const float x = pos[3 * i], y = pos[3 * i + 1], z = pos[3 * i + 2];
            if (mask[i] && sg_side(p1, x, y, z, bd) && sg_side(p2, x, y, z, bd)) s_flag[i] |= 1;
        }
    }
    if (t < 2 && a.planes_out) a.planes_out[(long)b * 2 + t] = t == 0 ? p1 : p2;
    __syncthreads();

    rg_merge(send_in, rp_in, s_flag, s_tl, nullptr, s_scan, N, M, i0, i1, apply, false, a.edge_cap, a.recv + (long)b * a.edge_cap,
             a.send + (long)b * a.edge_cap, a.row_ptr + (long)b * (N + 1), a.n_out + b);
}

hipError_t launch_surface_graphs(const SurfaceGraphsArgs& a, hipStream_t st) {
    hipLaunchKernelGGL(k_surface_graphs, dim3((unsigned)a.B), dim3(GW), 0, st, a);
    return hipGetLastError();
}

}  // namespace ag
