// Radius-AND-top-k graph construction over a uniform grid of cells: the builder for graphs beyond the LDS-resident one's
// 4096 particles (ag_edges.hip), same rules, same output bit for bit.  gfx950 only.
//
// ag_edges.hip keeps a graph's positions, flags and tool tables in LDS and tests a receiver against chunks of consecutive
// sender INDICES; memory per workgroup grows with N and, without spatial order in the indices, work grows with N^2.  Here
// nothing in LDS is sized by N: particles are binned into cells whose edge exceeds the radius, a receiver is tested against
// the 27 cells around its own, and every table (cell starts, cell-ordered particles, ELL rows, tool list) is in global memory.
//
// The rules are those of ag_edges.hip's header (SURVEY.md section 8 a5'), spelled with the same functions (ag_edge_select.h):
//     dis = ((dx*dx + dy*dy) + dz*dz), separate mul/add; adjacent <=> (dis - thr2) < 0; masked and tool-tool pairs excluded;
//     top-k per receiver over the in-radius senders by (dis, sender index); connect_tools_all rules of either builder;
//     CSR sorted by (receiver, sender); n_edges[b] the true count, and above edge_cap nothing else is written for graph b.
//
// The C entry point is ag_build_edges_cells (ag_api_cells.hip, include/adaptigraph_amd_cells.h).
//
// Exactness of the grid (DESIGN.md section 3.24 has the proof; tests/cells_restate.py restates cell_axis for the CPU attack):
//   * r is a float with fl(r*r) >= thr2.  A pair that passes the test has fl(d*d) < thr2 on each axis (the sum of
//     non-negative terms rounds monotonically), hence |fl(x_i - x_j)| < r, hence |x_i - x_j| < r in the reals;
//   * cell_axis is monotone in x, the cell edge h is at least 1.001 r, and an axis has at most 1023 cells, which keeps the
//     rounding of fl(fl(x - lo) * inv_h) below 2.5e-4 cells: two coordinates less than r apart differ by at most one cell;
//   * only finite coordinates of valid particles get a cell.  A valid particle with a NaN or infinite coordinate fails the
//     adjacency test in every pair (the reference's own arithmetic), so it is in no cell and its row has no radius edge; it
//     stays valid for the connect_tools_all rules.
//
// Kernels (one launch sequence serves all B graphs; no float atomics; the integer atomics count and slot particles inside a
// cell, and no result depends on the order inside a cell: the selection is by key and the rows leave sorted by index):
//   k_cells_bounds   per graph: bounds of the binned particles, squared threshold, cell edge, cells per axis
//   k_cells_bin      cell id per particle, count per cell, slot inside the cell
//   k_cells_starts   exclusive scan of the counts
//   k_cells_scatter  particles in cell order: (x, y, z, index and tool bit) as one float4
//   k_cells_rows     one wavefront per receiver: the 9 runs of 3 cells, top-k, ELL row sorted by index, degree, tool flag
//   k_cells_rowptr   per graph: ascending tool list, scan of the degrees -> row_ptr, n_edges
//   k_cells_emit     one wavefront per row: (recv, send) with the tool senders merged in index order
#include "ag_cells.h"
#include "ag_edge_select.h"
#include <algorithm>
#include <climits>

namespace ag {

constexpr int CW = 1024;             // threads of the per-graph kernels (bounds, starts, rowptr)
constexpr int CWAVES = CW / 64;
constexpr int RW = 256;              // threads of the per-particle / per-row kernels: 4 rows per workgroup
constexpr int RWAVES = RW / 64;
constexpr int CELLS_AXIS_MAX = 1024; // cells per axis stay below this (the proof's bound on the index rounding)

struct CellGrid {                    // one per graph, written by k_cells_bounds
    float lo[3]; float inv_h; int n[3]; int ncells; float thr2;
};

struct CellDev {
    const float* pos; long pos_bstride; const uint8_t* mask; const uint8_t* tool;
    float thr; const float* thr_vec; const float* thr2_vec;
    int B, N, k, cta, cells_cap; long edge_cap;
    CellGrid* grid; int* cell_cnt; int* cell_start; int* cid; int* slot; float4* sorted;
    int* ell; int* deg; int* cta_flag; int* tlist; int* ntool;
    int* recv; int* send; int* row_ptr; int* n_edges;
};

// cell of coordinate x on an axis with n cells from lo: monotone non-decreasing in x (each step is), x >= lo
__device__ __forceinline__ int cell_axis(float x, float lo, float inv_h, int n) {
    if (n == 1) return 0;
    const float u = __fmul_rn(__fsub_rn(x, lo), inv_h);
    return u >= (float)(n - 1) ? n - 1 : (int)u;
}
__device__ __forceinline__ bool finite3(float x, float y, float z) {
    const float INF = __builtin_huge_valf();
    return fabsf(x) < INF && fabsf(y) < INF && fabsf(z) < INF;       // false for NaN
}

// exclusive scan of one value per thread over the workgroup (Hillis-Steele on integers); *total = the sum
template <typename T>
__device__ T block_scan_excl(T v, T* buf, T* total) {
    const int tid = threadIdx.x;
    buf[tid] = v;
    __syncthreads();
    for (int off = 1; off < CW; off <<= 1) {
        T o = 0;
        if (tid >= off) o = buf[tid - off];
        __syncthreads();
        buf[tid] += o;
        __syncthreads();
    }
    const T incl = buf[tid];
    *total = buf[CW - 1];
    __syncthreads();                                                    // buf may be reused by the caller
    return incl - v;
}

__global__ __launch_bounds__(CW) void k_cells_bounds(CellDev a) {
    __shared__ float red[6][CWAVES];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float INF = __builtin_huge_valf();
    const float* p = a.pos + (long)b * a.pos_bstride;
    float mn[3] = {INF, INF, INF}, mx[3] = {-INF, -INF, -INF};
    for (int i = tid; i < a.N; i += CW) {
        const float x = p[3 * (long)i + 0], y = p[3 * (long)i + 1], z = p[3 * (long)i + 2];
        if (a.mask[(long)b * a.N + i] && finite3(x, y, z)) {
            mn[0] = fminf(mn[0], x); mx[0] = fmaxf(mx[0], x);
            mn[1] = fminf(mn[1], y); mx[1] = fmaxf(mx[1], y);
            mn[2] = fminf(mn[2], z); mx[2] = fmaxf(mx[2], z);
        }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) { mn[c] = fminf(mn[c], __shfl_xor(mn[c], o)); mx[c] = fmaxf(mx[c], __shfl_xor(mx[c], o)); }
        if (lane == 0) { red[2 * c][wave] = mn[c]; red[2 * c + 1][wave] = mx[c]; }
    }
    __syncthreads();
    if (tid != 0) return;
    for (int c = 0; c < 3; ++c)
        for (int w = 0; w < CWAVES; ++w) { mn[c] = fminf(mn[c], red[2 * c][w]); mx[c] = fmaxf(mx[c], red[2 * c + 1][w]); }
    const float t = a.thr_vec ? a.thr_vec[b] : a.thr;
    const float thr2 = a.thr2_vec ? a.thr2_vec[b] : __fmul_rn(t, t);
    CellGrid g;
    g.thr2 = thr2;
    g.lo[0] = mn[0]; g.lo[1] = mn[1]; g.lo[2] = mn[2];
    g.inv_h = 0.0f; g.n[0] = g.n[1] = g.n[2] = 1;
    // no pair passes (dis - thr2) < 0 unless thr2 > 0 (dis >= 0; a NaN threshold compares false): then nothing is binned
    g.ncells = (thr2 > 0.0f && mn[0] <= mx[0]) ? 1 : 0;
    const float FMAX = 3.402823466e38f;
    const float r = __fmul_rn(sqrtf(thr2), 1.0001f);                    // fl(r*r) >= thr2: the margin dwarfs the roundings
    if (g.ncells && r < FMAX) {
        float E[3]; bool on[3];
        float h = __fmul_rn(r, 1.001f);
        for (int c = 0; c < 3; ++c) {
            E[c] = __fsub_rn(mx[c], mn[c]);
            on[c] = E[c] < FMAX;                                        // an extent that overflows fp32 keeps one cell on its axis
            if (on[c]) h = fmaxf(h, __fmul_rn(E[c] / (float)CELLS_AXIS_MAX, 1.001f));
        }
        bool fits = false;
        for (int it = 0; it < 256 && !fits; ++it) {                     // any edge above the minimum is correct, only slower
            const float inv = 1.0f / h;
            long cells = 1;
            for (int c = 0; c < 3; ++c) {
                g.n[c] = on[c] ? (int)__fmul_rn(E[c], inv) + 1 : 1;
                cells *= g.n[c];
            }
            fits = g.n[0] < CELLS_AXIS_MAX && g.n[1] < CELLS_AXIS_MAX && g.n[2] < CELLS_AXIS_MAX && cells <= a.cells_cap;
            if (fits) { g.inv_h = inv; g.ncells = (int)cells; }
            else h = __fmul_rn(h, 1.26f);
        }
        if (!fits) { g.n[0] = g.n[1] = g.n[2] = 1; g.ncells = 1; g.inv_h = 0.0f; }
    }
    a.grid[b] = g;
}

__global__ __launch_bounds__(RW) void k_cells_bin(CellDev a) {
    const int b = blockIdx.y, i = blockIdx.x * RW + threadIdx.x;
    if (i >= a.N) return;
    const CellGrid g = a.grid[b];
    const float* p = a.pos + (long)b * a.pos_bstride + 3 * (long)i;
    const float x = p[0], y = p[1], z = p[2];
    int cid = -1, slot = 0;
    if (g.ncells && a.mask[(long)b * a.N + i] && finite3(x, y, z)) {
        const int cx = cell_axis(x, g.lo[0], g.inv_h, g.n[0]), cy = cell_axis(y, g.lo[1], g.inv_h, g.n[1]),
                  cz = cell_axis(z, g.lo[2], g.inv_h, g.n[2]);
        cid = (cz * g.n[1] + cy) * g.n[0] + cx;
        slot = atomicAdd(&a.cell_cnt[(long)b * a.cells_cap + cid], 1);  // which slot is whose is not defined; no result depends on it
    }
    a.cid[(long)b * a.N + i] = cid;
    a.slot[(long)b * a.N + i] = slot;
}

__global__ __launch_bounds__(CW) void k_cells_starts(CellDev a) {
    __shared__ int buf[CW];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int nc = a.grid[b].ncells;
    const int* cnt = a.cell_cnt + (long)b * a.cells_cap;
    int* start = a.cell_start + (long)b * (a.cells_cap + 1);
    const int per = (nc + CW - 1) / CW;
    const int c0 = min(nc, tid * per), c1 = min(nc, c0 + per);
    int mine = 0;
    for (int c = c0; c < c1; ++c) mine += cnt[c];
    int total;
    int run = block_scan_excl<int>(mine, buf, &total);
    for (int c = c0; c < c1; ++c) { start[c] = run; run += cnt[c]; }
    if (tid == 0) start[nc] = total;                                    // = particles that have a cell
}

__global__ __launch_bounds__(RW) void k_cells_scatter(CellDev a) {
    const int b = blockIdx.y, i = blockIdx.x * RW + threadIdx.x;
    if (i >= a.N) return;
    const int cid = a.cid[(long)b * a.N + i];
    if (cid < 0) return;
    const float* p = a.pos + (long)b * a.pos_bstride + 3 * (long)i;
    const int at = a.cell_start[(long)b * (a.cells_cap + 1) + cid] + a.slot[(long)b * a.N + i];
    const int tag = (i << 1) | (a.tool[(long)b * a.N + i] ? 1 : 0);
    a.sorted[(long)b * a.N + at] = make_float4(p[0], p[1], p[2], __int_as_float(tag));
}

// One receiver per wavefront, taken in cell order (neighbouring wavefronts read the same cells).  The senders of the 3 x 3
// runs of up to three x-adjacent cells - each run contiguous in cell order - are walked as one sequence, 64 at a time.
__global__ __launch_bounds__(RW) void k_cells_rows(CellDev a) {
    __shared__ unsigned long long keys_all[RWAVES * CAP];
    const int b = blockIdx.y, lane = lane_id(), wave = threadIdx.x >> 6;
    const int s = blockIdx.x * RWAVES + wave;
    const CellGrid g = a.grid[b];
    const int* start = a.cell_start + (long)b * (a.cells_cap + 1);
    if (s >= a.N || g.ncells == 0 || s >= start[g.ncells]) return;     // wave-uniform
    unsigned long long* keys = keys_all + wave * CAP;
    const float4* sorted = a.sorted + (long)b * a.N;
    const float4 me = sorted[s];
    const int itag = __float_as_int(me.w), i = itag >> 1, ti = itag & 1;
    const int cid = a.cid[(long)b * a.N + i];
    const int nx = g.n[0], ny = g.n[1], nz = g.n[2];
    const int cx = cid % nx, cy = (cid / nx) % ny, cz = cid / (nx * ny);
    int beg = 0, len = 0;
    if (lane < 9) {
        const int zz = cz + lane / 3 - 1, yy = cy + lane % 3 - 1;
        if (zz >= 0 && zz < nz && yy >= 0 && yy < ny) {
            const int row = (zz * ny + yy) * nx;
            beg = start[row + max(cx - 1, 0)];
            len = start[row + min(cx + 1, nx - 1) + 1] - beg;
        }
    }
    int rb[9], pre[10];
    pre[0] = 0;
#pragma unroll
    for (int r = 0; r < 9; ++r) {
        rb[r] = __builtin_amdgcn_readlane(beg, r);
        pre[r + 1] = pre[r] + __builtin_amdgcn_readlane(len, r);
    }
    const int nsend = pre[9];
    const float thr2 = g.thr2;
    int nb = 0;
    unsigned long long T = KEY_INF;
    for (int base = 0; base < nsend; base += 64) {
        const int t = base + lane;
        const bool in = t < nsend;
        int q = s;
#pragma unroll
        for (int r = 0; r < 9; ++r)
            if (in && t >= pre[r] && t < pre[r + 1]) q = rb[r] + (t - pre[r]);
        const float4 o = sorted[q];
        const int jtag = __float_as_int(o.w);
        const float d = dist_exact(me.x, me.y, me.z, o.x, o.y, o.z);
        const bool within = in && (__fsub_rn(d, thr2) < 0.0f) && !(ti && (jtag & 1));   // tool-tool pairs are excluded
        const unsigned long long bw = __ballot(within);
        if (!bw) continue;
        const unsigned long long key = ((unsigned long long)__float_as_uint(d) << 32) | (unsigned)jtag;   // (dis, index), tool bit last
        const bool push = within && key < T;
        const unsigned long long bp = __ballot(push);
        if (bp) {
            if (push) keys[nb + __popcll(bp & lanes_below(lane))] = key;
            nb += __popcll(bp);
            wave_lds_sync();
            if (nb > CAP - 64) {                                        // keep only the k smallest so far; tighten T
                T = select_kth(keys, nb, a.k, true);
                nb = a.k;
            }
        }
    }
    if (nb > a.k) { select_kth(keys, nb, a.k, true); nb = a.k; }      // the k smallest (dis, index) keys; nb <= 128 from here
    // what is kept leaves sorted by sender index; senders governed by the connect_tools_all rule are decided at emit
    unsigned mine[2]; bool outm[2]; int posn[2];
    int raw = 0, total = 0;
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        const int e = lane + 64 * u;
        const bool kept = e < nb;
        mine[u] = kept ? (unsigned)(keys[e] & 0xffffffffull) : 0u;
        const bool jt = mine[u] & 1u;
        raw += __popcll(__ballot(kept && !jt));
        outm[u] = kept && (!a.cta || (!jt && !ti));
        posn[u] = 0;
    }
    for (int t = 0; t < nb; ++t) {
        const unsigned jo = (unsigned)(keys[t] & 0xffffffffull);       // same address in every lane: LDS broadcast
        const bool oo = !a.cta || (!(jo & 1u) && !ti);
#pragma unroll
        for (int u = 0; u < 2; ++u) posn[u] += (oo && jo < mine[u]) ? 1 : 0;
    }
    int* ell_row = a.ell + ((long)b * a.N + i) * a.k;
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        if (outm[u]) ell_row[posn[u]] = (int)(mine[u] >> 1);
        total += __popcll(__ballot(outm[u]));
    }
    if (lane == 0) {
        a.deg[(long)b * a.N + i] = total;
        if (a.cta == 1 && ti && raw) atomicOr(&a.cta_flag[b], 1);      // batch rule: a tool row kept a non-tool sender
    }
}

__device__ __forceinline__ bool row_takes_tools(const CellDev& a, int b, int i) {
    // every valid receiver takes every tool sender; under the single-graph rule a tool receiver takes none
    return a.mask[(long)b * a.N + i] && !(a.cta == 2 && a.tool[(long)b * a.N + i]);
}

__global__ __launch_bounds__(CW) void k_cells_rowptr(CellDev a) {
    __shared__ long long buf[CW];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int per = (a.N + CW - 1) / CW;
    const int i0 = (int)min((long)a.N, (long)tid * per), i1 = min(a.N, i0 + per);
    int ntool = 0;
    if (a.cta) {                                                        // ascending tool list for the merge at emit
        int c = 0;
        for (int i = i0; i < i1; ++i) c += a.tool[(long)b * a.N + i] ? 1 : 0;
        long long tot;
        int at = (int)block_scan_excl<long long>(c, buf, &tot);
        ntool = (int)tot;
        for (int i = i0; i < i1; ++i)
            if (a.tool[(long)b * a.N + i]) a.tlist[(long)b * a.N + at++] = i;
    }
    const int flag = a.cta == 2 ? 1 : a.cta == 1 ? a.cta_flag[b] : 0;
    const int add = flag ? ntool : 0;
    long long mine = 0;
    for (int i = i0; i < i1; ++i) mine += a.deg[(long)b * a.N + i] + ((add && row_takes_tools(a, b, i)) ? add : 0);
    long long total;
    long long run = block_scan_excl<long long>(mine, buf, &total);
    if (tid == 0) {
        a.ntool[b] = total > a.edge_cap ? -1 : add;                     // tool senders per served row; -1: the graph does not fit
        a.n_edges[b] = (int)min(total, (long long)INT_MAX);             // the true count (saturated where int32 cannot hold it)
    }
    if (total > a.edge_cap) return;                                     // nothing else is written for this graph
    int* rp = a.row_ptr + (long)b * (a.N + 1);
    for (int i = i0; i < i1; ++i) {
        rp[i] = (int)run;
        run += a.deg[(long)b * a.N + i] + ((add && row_takes_tools(a, b, i)) ? add : 0);
    }
    if (tid == 0) rp[a.N] = (int)total;
}

__global__ __launch_bounds__(RW) void k_cells_emit(CellDev a) {
    const int b = blockIdx.y, lane = lane_id();
    const int i = blockIdx.x * RWAVES + (threadIdx.x >> 6);
    const int tools = a.ntool[b];
    if (i >= a.N || tools < 0) return;                                  // wave-uniform; a graph above edge_cap has no row_ptr
    const int off = a.row_ptr[(long)b * (a.N + 1) + i];
    const int nk = a.deg[(long)b * a.N + i];
    const int nt = (tools && row_takes_tools(a, b, i)) ? tools : 0;
    const int* ell = a.ell + ((long)b * a.N + i) * a.k;
    const int* tl = a.tlist + (long)b * a.N;
    int* recv = a.recv + (long)b * a.edge_cap;
    int* send = a.send + (long)b * a.edge_cap;
    for (int t = lane; t < nk; t += 64) {
        const int j = ell[t];
        int lo = 0, hi = nt;                                            // tools with a smaller index (the ELL row holds none itself)
        while (lo < hi) { const int mid = (lo + hi) >> 1; if (tl[mid] < j) lo = mid + 1; else hi = mid; }
        recv[off + t + lo] = i; send[off + t + lo] = j;
    }
    for (int m = lane; m < nt; m += 64) {
        const int j = tl[m];
        int before = 0;
        for (int t = 0; t < nk; ++t) before += ell[t] < j ? 1 : 0;
        recv[off + m + before] = i; send[off + m + before] = j;
    }
}

size_t cells_cap_for(int N) {
    size_t c = 64;
    while (c < (size_t)N && c < ((size_t)1 << 20)) c <<= 1;
    return c;
}

size_t cells_grid_bytes() { return sizeof(CellGrid); }

hipError_t launch_cells_build(const CellArgs& h, hipStream_t st) {
    CellDev a;
    a.pos = h.pos; a.pos_bstride = h.pos_bstride ? h.pos_bstride : (long)h.N * 3; a.mask = h.mask; a.tool = h.tool;
    a.thr = h.thr; a.thr_vec = h.thr_vec; a.thr2_vec = h.thr2_vec;
    a.B = h.B; a.N = h.N; a.k = std::min(h.N, h.topk); a.cta = h.rule; a.cells_cap = h.cells_cap; a.edge_cap = h.edge_cap;
    a.grid = reinterpret_cast<CellGrid*>(h.grid);
    a.cell_cnt = h.zeroed; a.deg = h.zeroed + (size_t)h.B * h.cells_cap; a.cta_flag = a.deg + (size_t)h.B * h.N;
    a.cell_start = h.cell_start; a.cid = h.cid; a.slot = h.slot; a.sorted = reinterpret_cast<float4*>(h.sorted);
    a.ell = h.ell; a.tlist = h.tlist; a.ntool = h.ntool;
    a.recv = h.recv; a.send = h.send; a.row_ptr = h.row_ptr; a.n_edges = h.n_edges;
    hipError_t e = hipMemsetAsync(h.zeroed, 0, h.zeroed_ints * sizeof(int), st);
    if (e != hipSuccess) return e;
    const dim3 per_particle((unsigned)((h.N + RW - 1) / RW), (unsigned)h.B), per_row((unsigned)((h.N + RWAVES - 1) / RWAVES), (unsigned)h.B);
    hipLaunchKernelGGL(k_cells_bounds, dim3(h.B), dim3(CW), 0, st, a);
    hipLaunchKernelGGL(k_cells_bin, per_particle, dim3(RW), 0, st, a);
    hipLaunchKernelGGL(k_cells_starts, dim3(h.B), dim3(CW), 0, st, a);
    hipLaunchKernelGGL(k_cells_scatter, per_particle, dim3(RW), 0, st, a);
    hipLaunchKernelGGL(k_cells_rows, per_row, dim3(RW), 0, st, a);
    hipLaunchKernelGGL(k_cells_rowptr, dim3(h.B), dim3(CW), 0, st, a);
    hipLaunchKernelGGL(k_cells_emit, per_row, dim3(RW), 0, st, a);
    return hipGetLastError();
}

}  // namespace ag
