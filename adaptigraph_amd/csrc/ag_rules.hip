// Tool-attachment rules of the single-graph edge builder, applied to existing CSR edge lists.  gfx950 only.
//
// construct_edges_from_states (reference src/dynamics/dataset/graph.py:68-231) has two optional rules that both
// have the form "given a particle SUBSET S (already restricted to valid particles)":
//     adj[tool receiver, sender in S]   = 0                                   graph.py:153 / :216
//     adj[receiver in S, tool sender]   = 1                                   graph.py:154 / :217
//     optional: of those (receiver in S, tool sender) pairs keep only the keepK = int(kNN * #pairs) with the
//               smallest distance, taken over the FLAT row-major list of pairs                  graph.py:156-169
//     adj[tool, tool]                   = 0                                   graph.py:170 / :218
// S = "non-fixed" particles (y above the bottom 10 %, graph.py:134-143) or the particles beyond the two surface
// planes closest to the tool (graph.py:190-207).  Integer / byte work, bit-exact; integer counters only, no float atomics.
//
// One copy of the mechanism - the workgroup scan, the tool list, the pair distance, the row walk and the merge - under three launches:
//   launch_tool_rule      one graph, S formed by the caller (host shim), any n_tools: the tool list and the (N, n_tools) pair
//                         tables live in global scratch.  k_rule_prep (tool list, counters), k_rule_dis / k_rule_rank (the kNN
//                         filter over the flat pair list, only with 0 < kNN < 1), k_rule_apply (merge)
//   launch_rule_graphs    the non-fixed rule for B graphs, one workgroup per graph, S = mask AND (y > thr) formed on the device and
//                         everything of a graph in LDS; a graph reads nothing of its neighbours (k_rule_graphs)
//   launch_surface_graphs the two-closest-planes rule for B graphs in the same pattern (k_surface_graphs)
#include <math.h>
#include "ag_rules.h"
#include "ag_dist.h"

namespace ag {

constexpr int RW = 1024;                     // one workgroup of 16 wavefronts per graph: the rank phase is O(pairs^2) and sets its time
constexpr int RULE_MAX_N = 4096;             // the particle flags of a graph live in LDS
constexpr float RULE_BIG = 1e10f;            // graph.py:92,96

// ---------------------------------------------------------------------------------------------------------------- shared mechanism
__device__ __forceinline__ int block_excl_scan(int* sh, int v) {   // RW threads, returns exclusive prefix; sh[RW-1] = total
    __syncthreads();                                             // sh may still be read from an earlier use
    sh[threadIdx.x] = v;
    __syncthreads();
    for (int off = 1; off < RW; off <<= 1) {
        int t = 0;
        if ((int)threadIdx.x >= off) t = sh[threadIdx.x - off];
        __syncthreads();
        sh[threadIdx.x] += t;
        __syncthreads();
    }
    return sh[threadIdx.x] - v;
}

// One graph as its workgroup sees it: inputs, outputs and the rows [i0, i1) this thread owns (rows striped over the RW threads).
struct RuleGraph {
    const float* pos; const uint8_t* mask; const uint8_t* tool;
    const int* send_in; const int* rp_in; int nb;            // nb: edge count of the input list (batched launches)
    int i0, i1;
    int* recv; int* send; int* row_ptr; int* n_out;
};
__device__ __forceinline__ void rule_stripe(RuleGraph& g, int N) {
    const int per = (N + RW - 1) / RW;
    g.i0 = min(N, (int)threadIdx.x * per); g.i1 = min(N, g.i0 + per);
}

// The tool count (returned on every thread) and the first M tool indices, ascending, in tl (LDS or global; visible to the other
// threads after the caller's next barrier).
__device__ __forceinline__ int rule_tool_list(const RuleGraph& g, int M, int* s_scan, int* tl) {
    int c = 0;
    for (int i = g.i0; i < g.i1; ++i) c += g.tool[i] ? 1 : 0;
    int r = block_excl_scan(s_scan, c);
    for (int i = g.i0; i < g.i1; ++i)
        if (g.tool[i] && r < M) tl[r++] = i;                            // the pair tables hold M columns
    return s_scan[RW - 1];
}

// fp32 distance of the pair (receiver i, tool sender j), spelled like the edge builder's; both_tool: i is a tool too
__device__ __forceinline__ float rule_pair_dis(const float* pos, const uint8_t* mask, int i, int j, bool both_tool) {
    if (!mask[j] || both_tool) return RULE_BIG;                         // graph.py:89-96
    return dist_exact(pos[3 * i], pos[3 * i + 1], pos[3 * i + 2], pos[3 * j], pos[3 * j + 1], pos[3 * j + 2]);   // graph.py:87-88
}

// One receiver row: walks the base senders [e, e1) (ascending) and the tool list (ascending) as one merged sequence.  flag: bit 0
// in S, bit 1 tool; tl / kept (the kNN filter's verdicts, (N, M) row-major): LDS or global.  apply = false copies the base row through.
template <bool WRITE>
__device__ __forceinline__ int rule_row(const int* send_in, int e, int e1, const uint8_t* flag, const int* tl, const uint8_t* kept,
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
            if (i_sub) on = use_knn ? kept[(long)i * M + m] != 0 : true;   // graph.py:154,168 | :217
            if (i_tool) on = false;                                     // graph.py:170 | :218
            ++m;
        } else {
            on = base && !(apply && i_tool && (flag[j] & 1));           // graph.py:153 | :216
        }
        if (base) ++e;
        if (on) {
            if (WRITE) { recv[out + n] = i; send[out + n] = j; }
            ++n;
        }
    }
    return n;
}

// The merge every launch ends with: count -> scan -> write.  *n_out is the TRUE count.  Above edge_cap recv / send are never
// written; row_ptr is then written only with row_ptr_on_overflow (the single-graph export's contract; the batched exports write
// nothing else for such a graph).
__device__ __forceinline__ void rule_merge(const RuleGraph& g, const uint8_t* flag, const int* tl, const uint8_t* kept, int* s_scan,
                                           int N, int M, bool apply, bool use_knn, int edge_cap, bool row_ptr_on_overflow) {
    int mine = 0;
    for (int i = g.i0; i < g.i1; ++i)
        mine += rule_row<false>(g.send_in, g.rp_in[i], g.rp_in[i + 1], flag, tl, kept, i, M, apply, use_knn, nullptr, nullptr, 0);
    int run = block_excl_scan(s_scan, mine);
    const int total = s_scan[RW - 1];
    const bool fits = total <= edge_cap;
    if (fits || row_ptr_on_overflow) {
        for (int i = g.i0; i < g.i1; ++i) {
            g.row_ptr[i] = run;
            run += fits ? rule_row<true>(g.send_in, g.rp_in[i], g.rp_in[i + 1], flag, tl, kept, i, M, apply, use_knn, g.recv, g.send, run)
                        : rule_row<false>(g.send_in, g.rp_in[i], g.rp_in[i + 1], flag, tl, kept, i, M, apply, use_knn, nullptr, nullptr, 0);
        }
        if (threadIdx.x == 0) g.row_ptr[N] = total;
    }
    if (threadIdx.x == 0) *g.n_out = total;
}

// ---------------------------------------------------------------------------------------------------------------- one graph
struct RuleDev {
    RuleGraph g;
    const uint8_t* subset;
    int N, n_tools, edge_cap, use_knn; double kNN;
    int* tlist; int* misc;                   // misc: 0 ntool, 1 pair count, 2 tool count differs from the caller's n_tools
    float* pdis; uint8_t* keep; uint8_t* kept;   // (N, ntool) pair tables, row-major = the reference's flat order:
                                             // distance, 1 = pair of the rule / 2 = not, verdict of the kNN filter
};

__global__ __launch_bounds__(RW) void k_rule_prep(RuleDev a) {
    __shared__ int sh[RW];
    rule_stripe(a.g, a.N);
    const int ntool = rule_tool_list(a.g, a.n_tools, sh, a.tlist);
    if (threadIdx.x == 0) { a.misc[0] = ntool; a.misc[1] = 0; a.misc[2] = ntool != a.n_tools; }
}

__global__ void k_rule_dis(RuleDev a) {
    const int M = a.misc[0];
    const long p = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (a.misc[2] || M == 0 || p >= (long)a.N * M) return;
    const int i = (int)(p / M), j = a.tlist[p % M];
    if (!(a.subset[i] && a.g.mask[i])) { a.keep[p] = 2; return; }       // 2 = not a pair of the rule
    a.pdis[p] = rule_pair_dis(a.g.pos, a.g.mask, i, j, a.g.tool[i] && a.g.tool[j]);
    a.keep[p] = 1;
    atomicAdd(&a.misc[1], 1);                                          // integer: order-independent
}

__global__ __launch_bounds__(256) void k_rule_rank(RuleDev a) {
    __shared__ float sd[1024];
    __shared__ uint8_t sk[1024];
    const int M = a.misc[0];
    const long L = (long)a.N * M;
    if (a.misc[2] || M == 0) return;                                    // uniform over the grid
    const int keepK = (int)(a.kNN * (double)a.misc[1]);                // graph.py:160 int(kNN * count)
    const long p = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const bool mine = p < L && a.keep[p] != 2;
    const float dp = mine ? a.pdis[p] : 0.0f;
    int rank = 0;
    for (long q0 = 0; q0 < L; q0 += 1024) {
        __syncthreads();
        for (int t = threadIdx.x; t < 1024; t += 256) {
            const long q = q0 + t;
            sk[t] = q < L ? a.keep[q] : 2;
            sd[t] = (q < L && sk[t] != 2) ? a.pdis[q] : 0.0f;
        }
        __syncthreads();
        if (mine) {
            const int n = (int)min(1024L, L - q0);
            for (int t = 0; t < n; ++t)
                rank += (sk[t] != 2 && (sd[t] < dp || (sd[t] == dp && q0 + t < p))) ? 1 : 0;
        }
    }
    if (mine) a.kept[p] = rank < keepK ? 1 : 0;
}

__global__ __launch_bounds__(RW) void k_rule_apply(RuleDev a) {
    __shared__ int sh[RW];
    __shared__ uint8_t s_flag[RULE_MAX_N];
    if (a.misc[2]) {                                                    // caller's n_tools is wrong: refuse, loudly
        if (threadIdx.x == 0) *a.g.n_out = -1;
        return;
    }
    rule_stripe(a.g, a.N);
    for (int i = threadIdx.x; i < a.N; i += RW)
        s_flag[i] = (uint8_t)(((a.subset[i] && a.g.mask[i]) ? 1 : 0) | (a.g.tool[i] ? 2 : 0));
    __syncthreads();
    rule_merge(a.g, s_flag, a.tlist, a.kept, sh, a.N, a.misc[0], true, a.use_knn != 0, a.edge_cap, true);
}

hipError_t launch_tool_rule(const RuleArgs& h, hipStream_t st) {
    RuleDev a{};
    a.g.pos = h.pos; a.g.mask = h.mask; a.g.tool = h.tool; a.subset = h.subset;
    a.g.send_in = h.send_in; a.g.rp_in = h.row_ptr_in;
    a.N = h.N; a.n_tools = h.n_tools; a.edge_cap = h.edge_cap; a.use_knn = h.use_knn; a.kNN = h.kNN;
    a.tlist = h.tlist; a.misc = h.misc; a.pdis = h.pdis; a.keep = h.keep; a.kept = h.kept;
    a.g.recv = h.recv; a.g.send = h.send; a.g.row_ptr = h.row_ptr; a.g.n_out = h.n_out;
    hipLaunchKernelGGL(k_rule_prep, dim3(1), dim3(RW), 0, st, a);
    if (h.use_knn && h.n_tools > 0) {
        const long L = (long)h.N * h.n_tools;
        const unsigned grid = (unsigned)((L + 255) / 256);
        hipLaunchKernelGGL(k_rule_dis, dim3(grid), dim3(256), 0, st, a);
        hipLaunchKernelGGL(k_rule_rank, dim3(grid), dim3(256), 0, st, a);
    }
    hipLaunchKernelGGL(k_rule_apply, dim3(1), dim3(RW), 0, st, a);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------------- B graphs
__device__ __forceinline__ RuleGraph rg_view(const RuleGraphsBase& a, int b) {
    RuleGraph g;
    g.pos = a.pos + (long)b * a.pos_bstride;
    g.mask = a.mask + (long)b * a.N; g.tool = a.tool + (long)b * a.N;
    g.send_in = a.send_in + (long)b * a.base_cap; g.rp_in = a.row_ptr_in + (long)b * (a.N + 1); g.nb = a.n_edges_in[b];
    rule_stripe(g, a.N);
    g.recv = a.recv + (long)b * a.edge_cap; g.send = a.send + (long)b * a.edge_cap;
    g.row_ptr = a.row_ptr + (long)b * (a.N + 1); g.n_out = a.n_out + b;
    return g;
}

// The guard of the batched launches: the input list as ag_build_edges_graphs (or the sibling rule) writes it - count within
// [0, base_cap], rows ascending from 0 to the count, senders strictly ascending within [0, N) - and the tool count, checked before
// any index from device memory is used.  Fills tl with the first M tool indices, ascending.  Returns the verdict on every thread.
__device__ __forceinline__ bool rg_guard(const RuleGraph& g, int base_cap, int N, int M, int* s_scan, int* tl) {
    const int nb = g.nb;
    int bad = (nb < 0 || nb > base_cap) ? 1 : 0;
    if (!bad) {                                                         // nb is uniform over the workgroup
        for (int i = g.i0; i < g.i1; ++i) {
            const int e0 = g.rp_in[i], e1 = g.rp_in[i + 1];
            if (e0 < 0 || e1 < e0 || e1 > nb) { bad = 1; continue; }
            int prev = -1;
            for (int e = e0; e < e1; ++e) {
                const int j = g.send_in[e];
                if (j <= prev || j >= N) bad = 1;
                prev = max(prev, j);
            }
        }
        if (threadIdx.x == 0 && (g.rp_in[0] != 0 || g.rp_in[N] != nb)) bad = 1;
    }
    if (rule_tool_list(g, M, s_scan, tl) != M) bad = 1;
    return __syncthreads_or(bad) != 0;
}

// max x y z, min x y z (ext[0..5], on every thread) over graph b's bounds rows; per axis a NaN among them makes both NaN, as np.max
// does, and so does no row at all.  A thread folds its rows in order, a wavefront folds by xor-shuffle, then every thread folds the
// 16 wavefronts' values in wavefront order (through s_scan).  Max and min are exact, so the order changes no value.
__device__ __forceinline__ void rg_extents(const RuleGraphsBase& a, int b, int* s_scan, float* ext) {
    constexpr int WAVES = RW / 64;
    const int t = threadIdx.x;
    int n = max(a.bnd_n[b], 0);
    if (a.bnd_idx) n = min(n, a.idx_stride);
    const long first = a.bnd_first[b];
    for (int k = 0; k < 6; ++k) ext[k] = k < 3 ? -INFINITY : INFINITY;
    int nan = 0, any = 0;                                                             // nan: bit per axis
    for (int q = t; q < n; q += RW) {
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
    if ((t & 63) == 0)                                                                // (the guard's barrier lies behind s_scan's last use)
        for (int k = 0; k < 6; ++k) s_scan[k * WAVES + (t >> 6)] = __float_as_int(ext[k]);
    const int nan_x = __syncthreads_or(nan & 1), nan_y = __syncthreads_or(nan & 2), nan_z = __syncthreads_or(nan & 4);
    any = __syncthreads_or(any);                                                      // (also the barrier behind the stores)
    for (int k = 0; k < 6; ++k) {
        float v = __int_as_float(s_scan[k * WAVES]);
        for (int w = 1; w < WAVES; ++w) v = k < 3 ? fmaxf(v, __int_as_float(s_scan[k * WAVES + w])) : fminf(v, __int_as_float(s_scan[k * WAVES + w]));
        ext[k] = v;
    }
    if (nan_x || !any) ext[0] = ext[3] = NAN;
    if (nan_y || !any) ext[1] = ext[4] = NAN;
    if (nan_z || !any) ext[2] = ext[5] = NAN;
}

// "Tool to all non-fixed particles" (graph.py:125-171) and its flat kNN filter.  Phases:
//   guard     : rg_guard                                                                                     (-> n_out = -1)
//   threshold : max / min of the bounds rows' y, thr in four separately rounded fp32 operations
//   contact   : does the base list hold a tool-sender edge (graph.py:128-135)?  no: the base graph is copied through
//   pairs     : fp32 distance of every (receiver in S, tool) pair, row-major = the reference's flat order    (0 < kNN < 1 only)
//   rank      : rank of each pair by (distance, flat index) -> keep flag                                     (0 < kNN < 1 only)
//   merge     : rule_merge
__global__ __launch_bounds__(RW) void k_rule_graphs(RuleGraphsArgs a) {
    __shared__ float s_dis[RULE_GRAPHS_MAX_PAIRS];
    __shared__ uint8_t s_keep[RULE_GRAPHS_MAX_PAIRS];     // 1 = pair of the rule, 2 = not
    __shared__ uint8_t s_kept[RULE_GRAPHS_MAX_PAIRS];     // verdict of the kNN filter
    __shared__ uint8_t s_flag[RULE_MAX_N];
    __shared__ int s_scan[RW];
    __shared__ int s_tl[RULE_GRAPHS_MAX_TOOLS];
    const int b = blockIdx.x, t = threadIdx.x, N = a.g.N, M = a.g.n_tools;
    const RuleGraph g = rg_view(a.g, b);

    if (rg_guard(g, a.g.base_cap, N, M, s_scan, s_tl)) {                // refuse, loudly: -1 and nothing else
        if (t == 0) *g.n_out = -1;
        return;
    }

    // ---- threshold
    float ext[6];
    rg_extents(a.g, b, s_scan, ext);
    const float mx = ext[1], mn = ext[4];
    const float thr = __fadd_rn(__fmul_rn(__fsub_rn(__fmul_rn(mx, a.g.ratio), mn), 0.1f), mn);   // rollout.py:136, graph.py:134
    if (t == 0 && a.thr_out) a.thr_out[b] = thr;

    // ---- per-particle flags, contact check
    for (int i = t; i < N; i += RW) {
        const bool mk = g.mask[i] != 0;
        s_flag[i] = (uint8_t)(((mk && g.pos[3 * i + 1] > thr) ? 1 : 0) | (g.tool[i] ? 2 : 0));
    }
    __syncthreads();
    int touch = 0;
    for (int e = t; e < g.nb; e += RW) touch |= (s_flag[g.send_in[e]] & 2) ? 1 : 0;   // senders were bounded by the guard
    const bool apply = __syncthreads_or(touch) != 0;                    // graph.py:128-135
    const double kNN = a.kNN[b];
    const bool use_knn = apply && M > 0 && kNN < 1.0 && kNN > 0.0;      // graph.py:156

    // ---- pair distances and the flat kNN filter
    if (use_knn) {
        const int P = N * M;
        int cnt = 0;
        for (int p = t; p < P; p += RW) {
            const int i = p / M, j = s_tl[p % M];
            if (!(s_flag[i] & 1)) { s_keep[p] = 2; s_dis[p] = 0.0f; continue; }
            s_dis[p] = rule_pair_dis(g.pos, g.mask, i, j, (s_flag[i] & 2) && (s_flag[j] & 2));
            s_keep[p] = 1;
            ++cnt;
        }
        (void)block_excl_scan(s_scan, cnt);                             // also the barrier behind the pair tables
        const int keepK = (int)(kNN * (double)s_scan[RW - 1]);          // graph.py:160 int(kNN * count)
        for (int p = t; p < P; p += RW) {
            if (s_keep[p] == 2) continue;
            const float dp = s_dis[p];
            int rank = 0;
            for (int q = 0; q < P; ++q)
                rank += (s_keep[q] != 2 && (s_dis[q] < dp || (s_dis[q] == dp && q < p))) ? 1 : 0;
            s_kept[p] = rank < keepK ? 1 : 0;
        }
    }
    __syncthreads();

    rule_merge(g, s_flag, s_tl, s_kept, s_scan, N, M, apply, use_knn, a.g.edge_cap, false);
}

hipError_t launch_rule_graphs(const RuleGraphsArgs& a, hipStream_t st) {
    hipLaunchKernelGGL(k_rule_graphs, dim3((unsigned)a.g.B), dim3(RW), 0, st, a);
    return hipGetLastError();
}

// "Tool to the two closest surface planes" (graph.py:175-221), decision for decision what construct_edges_from_states' surface
// branch does on the host for one graph.  Phases:
//   guard   : rg_guard                                                                                    (-> n_out = -1)
//   bounds  : rg_extents, then the six bounds in separately rounded fp32 operations; order 0 = the step loop's (rollout.py:132-139:
//             min_x / min_z from the SCALED maxima), order 1 = construct_graph's (rollout/graph.py:446-458: from the UNSCALED maxima,
//             the maxima scaled afterwards)
//   contact : check = tool-sender edges of the INPUT list (graph.py:180-181); 0: the input graph is copied through
//   planes  : graph.py:190-197 index s_receiv with the 0 / 1 VALUES of adj[obj_tool_mask_2], so each of its (#mask * n_tools) entries
//             selects particle 0 or particle 1, broadcast over N senders: value = N * (n0 * d_0 + n1 * d_1) in fp64, d_k the fp32
//             squared distance of particle k to the plane; the two smallest by (value, index), NaN last = np.argsort on five values
//   merge   : S = side(first) AND side(second) AND mask; rule_merge without the kNN filter
// LDS: the particle flags, the scan and the tool list (about 8.3 KB).
__device__ __forceinline__ bool sg_side(int plane, float x, float y, float z, const float* bd) {   // graph.py:47-66; bd as bounds_out
    switch (plane) {
        case 0: return y >= bd[0];      // max_y
        case 1: return x <= bd[4];      // min_x
        case 2: return x >= bd[2];      // max_x
        case 3: return z <= bd[5];      // min_z
        default: return z >= bd[3];     // max_z
    }
}

__global__ __launch_bounds__(RW) void k_surface_graphs(SurfaceGraphsArgs a) {
    __shared__ uint8_t s_flag[RULE_MAX_N];
    __shared__ int s_scan[RW];
    __shared__ int s_tl[RULE_GRAPHS_MAX_TOOLS];
    __shared__ int s_cnt[2];
    const int b = blockIdx.x, t = threadIdx.x, N = a.g.N, M = a.g.n_tools;
    const RuleGraph g = rg_view(a.g, b);
    const float* pos = g.pos;

    if (rg_guard(g, a.g.base_cap, N, M, s_scan, s_tl)) {
        if (t == 0) *g.n_out = -1;
        return;
    }

    // ---- bounds
    if (t < 2) s_cnt[t] = 0;                                                          // (rg_extents' barriers lie behind it)
    float ext[6];
    rg_extents(a.g, b, s_scan, ext);
    float bd[6];                                                                      // max_y, min_y, max_x, max_z, min_x, min_z
    const float r = a.g.ratio, q1 = a.one_minus_ratio;
    bd[0] = __fmul_rn(ext[1], r); bd[1] = ext[4]; bd[2] = __fmul_rn(ext[0], r); bd[3] = __fmul_rn(ext[2], r);
    const float hx = a.bounds_order ? ext[0] : bd[2], hz = a.bounds_order ? ext[2] : bd[3];
    bd[4] = __fadd_rn(__fmul_rn(__fsub_rn(hx, ext[3]), q1), ext[3]);
    bd[5] = __fadd_rn(__fmul_rn(__fsub_rn(hz, ext[5]), q1), ext[5]);
    if (t < 6 && a.bounds_out) a.bounds_out[(long)b * 6 + t] = bd[t];

    // ---- contact: tool-sender edges of the input list, valid particles
    for (int i = t; i < N; i += RW) s_flag[i] = (uint8_t)(g.tool[i] ? 2 : 0);
    __syncthreads();
    int check = 0, nmask = 0;
    for (int e = t; e < g.nb; e += RW) check += (s_flag[g.send_in[e]] & 2) ? 1 : 0;   // senders were bounded by the guard
    for (int i = t; i < N; i += RW) nmask += g.mask[i] ? 1 : 0;
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
        for (int i = t; i < N; i += RW) {
            const float x = pos[3 * i], y = pos[3 * i + 1], z = pos[3 * i + 2];
            if (g.mask[i] && sg_side(p1, x, y, z, bd) && sg_side(p2, x, y, z, bd)) s_flag[i] |= 1;
        }
    }
    if (t < 2 && a.planes_out) a.planes_out[(long)b * 2 + t] = t == 0 ? p1 : p2;
    __syncthreads();

    rule_merge(g, s_flag, s_tl, nullptr, s_scan, N, M, apply, false, a.g.edge_cap, false);
}

hipError_t launch_surface_graphs(const SurfaceGraphsArgs& a, hipStream_t st) {
    hipLaunchKernelGGL(k_surface_graphs, dim3((unsigned)a.g.B), dim3(RW), 0, st, a);
    return hipGetLastError();
}

}  // namespace ag
