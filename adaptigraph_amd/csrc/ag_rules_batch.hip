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

    // ---- guard: the base list as ag_build_edges_graphs writes it (rows ascending, senders strictly ascending within [0, N))
    int bad = (nb < 0 || nb > a.base_cap) ? 1 : 0;
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
        if (tool[i] && r < M) s_tl[r++] = i;
    if (ntool != M) bad = 1;
    if (__syncthreads_or(bad)) {                                        // refuse, loudly: -1 and nothing else
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

    // ---- merge: count -> scan -> write
    int mine = 0;
    for (int i = i0; i < i1; ++i)
        mine += rg_row<false>(send_in, rp_in[i], rp_in[i + 1], s_flag, s_tl, s_kept, i, M, apply, use_knn, nullptr, nullptr, 0);
    int run = rg_excl_scan(s_scan, mine);
    const int total = s_scan[GW - 1];
    if (total <= a.edge_cap) {
        int* recv = a.recv + (long)b * a.edge_cap;
        int* send = a.send + (long)b * a.edge_cap;
        int* row_ptr = a.row_ptr + (long)b * (N + 1);
        for (int i = i0; i < i1; ++i) {
            row_ptr[i] = run;
            run += rg_row<true>(send_in, rp_in[i], rp_in[i + 1], s_flag, s_tl, s_kept, i, M, apply, use_knn, recv, send, run);
        }
        if (t == 0) row_ptr[N] = total;
    }
    if (t == 0) a.n_out[b] = total;                                     // the TRUE count even when nothing was written
}

hipError_t launch_rule_graphs(const RuleGraphsArgs& a, hipStream_t st) {
    hipLaunchKernelGGL(k_rule_graphs, dim3((unsigned)a.B), dim3(GW), 0, st, a);
    return hipGetLastError();
}

}  // namespace ag
