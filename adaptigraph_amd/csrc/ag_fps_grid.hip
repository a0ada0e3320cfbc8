// Farthest-point sampling beyond k_fps_cloud's 1024 samples: the same two stages, the same indices bit for bit, with the work per
// selected point shrinking as the samples get dense.  gfx950 only.  Entry point: ag_fps_cloud_grid (ag_api_cells.hip).
//
// k_fps_cloud sweeps the whole cloud once per selected point.  Here the cloud is binned into cells; a cell keeps its tight box and
// the packed key (fps_key) of the largest running minimum among its members.  After a new centre c is chosen, a cell whose box is
// at least that far from c is left alone: none of its members' minima can change (DESIGN.md section 3.27 has the proof; the
// numpy restatement the kernel is read against is tests/fps_grid_restate.py).  The partition itself never enters the result: the
// minima are updated with k_fps_cloud's arithmetic, operation for operation (stage 2's square root excepted: sqrt_exact below), and
// the argmax is the maximum of packed keys, which
// does not depend on grouping - so neither the cell arithmetic nor the cell count nor the order inside a cell can change a bit.
//
// Binning (grid-parallel over all B clouds of the call; the only atomics are integer ones: ordered-integer max for the bounds, add
// for the counts; which slot of its cell a point gets is not defined and no result depends on it):
//   k_fg_bounds   per cloud: bounds of the points with finite coordinates
//   k_fg_grid     per cloud: cells per axis (powers of two, the halving always on the axis with the longest cells), their scale
//   k_fg_bin      cell per point, count per cell, slot inside the cell; a point with a non-finite coordinate goes to cell `ncells`
//   k_fg_starts   exclusive scan of the counts
//   k_fg_scatter  points in cell order: (x, y, z, original index) as one float4, the running minimum beside it
//   k_fg_boxes    one wavefront per cell: tight box and initial key; the non-finite cell's box is all of space, so it is never pruned
// Selection: k_fps_select<STAGE2, INLDS>, one workgroup of 1024 threads per cloud; nothing waits for another workgroup.  Every
//   cell belongs to one lane of one wavefront (owned_cell): neighbouring cells - what a new centre touches - go to different
//   wavefronts.  Per selected point every lane tests its cells (all slots' loads in flight together), the wavefront then visits
//   those that are not pruned (one ballot per slot, no list, no barrier), 64 members at a time, and refreshes their keys; then one
//   block_max_u64 over the keys - ONE barrier per selected point.  A cell's table entries are read and written by their owner lane only, its members by the owner's wavefront only.
//   The tables (key, box, start, count: 40 bytes per cell) live in LDS up to FPS_GRID_LDS_CELLS cells, in the workspace beyond.
// Stage 2 runs on the stage-1 points in selection order, binned by a second pass of the same kernels.
#include "ag_fps_grid.h"
#include "ag_dist.h"
#include "ag_fps_key.h"
#include "ag_lds_optin.h"

#include <algorithm>

namespace ag {

constexpr int GW = 1024, GWAVES = GW / 64;       // the selection's workgroup, and the per-cloud scan's
constexpr int BW = 256;                          // threads of the per-point kernels
constexpr int LDS_SLOTS = (FPS_GRID_LDS_CELLS + 1 + GW - 1) / GW;   // table slots per thread in LDS (+ 1: the non-finite cell)
constexpr int CELL_BYTES = 40;                   // key 8, box 24, start 4, count 4
constexpr int SEL_LDS_HEAD = 256;                // block_max_u64's 2 * GWAVES keys

struct FpsGrid {                                 // one per cloud, written by k_fg_grid
    float lo[3]; float inv[3]; int n[3]; int ncells;
};

struct BinDev {
    const float* pos; const long long* pt_off; const long long* npts; int stride;
    int P, cells, cells_cap; float md0;          // P: points per cloud at most; cells: forced count or 0; md0: initial minimum
    unsigned* zeroed; FpsGrid* grid; int* start; int* cid; int* slot; float4* sorted; float* md; float* box; unsigned long long* key0;
};
struct SelDev {
    BinDev bin;
    const int* first; const float* radius;       // fps_start (stage 1) or rad_start (stage 2); fps_radius
    int max_nobj; char* tab; size_t tab_bytes;
    float* s1pos; int* s1idx; long long* off2; long long* n2;
    int* fps_idx; int* n_obj;
};

int fps_grid_cells_cap(int points, int cells) {
    if (cells > 0) return cells;
    int c = 1;
    while (c < FPS_GRID_MAX_CELLS && (long)c * FPS_GRID_CELL_POINTS < (long)points) c <<= 1;
    return c;
}
size_t fps_grid_bytes() { return sizeof(FpsGrid); }
__host__ __device__ inline size_t tab_cells(int cells_cap) { return ((size_t)cells_cap + 1 + GW - 1) / GW * GW; }
size_t fps_grid_tab_bytes(int cells_cap) { return cells_cap > FPS_GRID_LDS_CELLS ? tab_cells(cells_cap) * CELL_BYTES : 0; }

// floats as unsigned integers of the same order; 0 is below every finite float's image
__device__ __forceinline__ unsigned ord_of(float f) {
    const unsigned u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float ord_to(unsigned o) { return __uint_as_float((o & 0x80000000u) ? (o & 0x7fffffffu) : ~o); }
__device__ __forceinline__ bool fg_finite3(float x, float y, float z) {
    const float INF = __builtin_huge_valf();
    return fabsf(x) < INF && fabsf(y) < INF && fabsf(z) < INF;       // false for NaN
}
__device__ __forceinline__ int cloud_points(const BinDev& a, int b) {
    const long long nraw = a.npts[(long)b * a.stride];
    return (int)(nraw < 0 ? 0 : nraw > (long long)a.P ? (long long)a.P : nraw);      // keeps every table inside its stride
}
__device__ __forceinline__ size_t zeroed_stride(const BinDev& a) { return 6 + (size_t)a.cells_cap + 1; }
// cell of coordinate x on an axis of n cells: any value in [0, n) is correct, NaN (0 * inf) included
__device__ __forceinline__ int fg_axis(float x, float lo, float inv, int n) {
    const float u = __fmul_rn(__fsub_rn(x, lo), inv);
    return u >= (float)(n - 1) ? n - 1 : u > 0.0f ? (int)u : 0;
}

__global__ __launch_bounds__(BW) void k_fg_bounds(BinDev a) {
    const int b = blockIdx.y, lane = threadIdx.x & 63;
    const int n = cloud_points(a, b);
    const float* p = a.pos + a.pt_off[(long)b * a.stride] * 3;
    const float INF = __builtin_huge_valf();
    float v[6] = {-INF, -INF, -INF, -INF, -INF, -INF};               // max of -x, -y, -z, x, y, z
    bool any = false;
    for (long i = (long)blockIdx.x * BW + threadIdx.x; i < n; i += (long)gridDim.x * BW) {
        const float x = p[3 * i], y = p[3 * i + 1], z = p[3 * i + 2];
        if (fg_finite3(x, y, z)) {
            any = true;
            v[0] = fmaxf(v[0], -x); v[1] = fmaxf(v[1], -y); v[2] = fmaxf(v[2], -z);
            v[3] = fmaxf(v[3], x); v[4] = fmaxf(v[4], y); v[5] = fmaxf(v[5], z);
        }
    }
    const bool wave_any = __ballot(any) != 0ull;
#pragma unroll
    for (int k = 0; k < 6; ++k) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v[k] = fmaxf(v[k], __shfl_xor(v[k], o));
    }
    if (lane == 0 && wave_any) {
        unsigned* bnd = a.zeroed + (size_t)b * zeroed_stride(a);
#pragma unroll
        for (int k = 0; k < 6; ++k) atomicMax(&bnd[k], ord_of(v[k]));
    }
}

__global__ __launch_bounds__(64) void k_fg_grid(BinDev a, int B) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= B) return;
    const int n = cloud_points(a, b);
    const unsigned* bnd = a.zeroed + (size_t)b * zeroed_stride(a);
    FpsGrid g;
    for (int c = 0; c < 3; ++c) { g.lo[c] = 0.0f; g.inv[c] = 0.0f; g.n[c] = 1; }
    g.ncells = 1;
    if (bnd[0] != 0u) {                                              // there is a finite point
        const float FMAX = 3.402823466e38f;
        const float ex = __fsub_rn(ord_to(bnd[3]), -ord_to(bnd[0])), ey = __fsub_rn(ord_to(bnd[4]), -ord_to(bnd[1])),
                    ez = __fsub_rn(ord_to(bnd[5]), -ord_to(bnd[2]));
        g.lo[0] = -ord_to(bnd[0]); g.lo[1] = -ord_to(bnd[1]); g.lo[2] = -ord_to(bnd[2]);
        int want = a.cells;
        if (want <= 0) { want = 1; while (want < a.cells_cap && (long)want * FPS_GRID_CELL_POINTS < (long)n) want <<= 1; }
        want = min(want, a.cells_cap);
        // halve, each time, the axis whose cells are longest; an axis of zero (or overflowing) extent keeps one cell, so a flat,
        // collinear or single-point cloud degenerates to fewer cells and nothing divides by zero
        const bool okx = ex > 0.0f && ex <= FMAX, oky = ey > 0.0f && ey <= FMAX, okz = ez > 0.0f && ez <= FMAX;
        int nx = 1, ny = 1, nz = 1;
        for (int c = 1; c < want; c <<= 1) {
            const float lx = okx ? ex / (float)nx : 0.0f, ly = oky ? ey / (float)ny : 0.0f, lz = okz ? ez / (float)nz : 0.0f;
            if (lx > 0.0f && lx >= ly && lx >= lz) nx <<= 1;
            else if (ly > 0.0f && ly >= lz) ny <<= 1;
            else if (lz > 0.0f) nz <<= 1;
            else break;
        }
        g.n[0] = nx; g.n[1] = ny; g.n[2] = nz; g.ncells = nx * ny * nz;
        g.inv[0] = nx > 1 ? (float)nx / ex : 0.0f; g.inv[1] = ny > 1 ? (float)ny / ey : 0.0f; g.inv[2] = nz > 1 ? (float)nz / ez : 0.0f;
    }
    a.grid[b] = g;
}

__global__ __launch_bounds__(BW) void k_fg_bin(BinDev a) {
    const int b = blockIdx.y, i = blockIdx.x * BW + threadIdx.x;
    if (i >= cloud_points(a, b)) return;
    const FpsGrid g = a.grid[b];
    const float* p = a.pos + (a.pt_off[(long)b * a.stride] + i) * 3;
    const float x = p[0], y = p[1], z = p[2];
    int cid = g.ncells;                                              // the cell of the non-finite points
    if (fg_finite3(x, y, z)) {
        const int cx = fg_axis(x, g.lo[0], g.inv[0], g.n[0]), cy = fg_axis(y, g.lo[1], g.inv[1], g.n[1]),
                  cz = fg_axis(z, g.lo[2], g.inv[2], g.n[2]);
        cid = (cz * g.n[1] + cy) * g.n[0] + cx;
    }
    int* cnt = reinterpret_cast<int*>(a.zeroed + (size_t)b * zeroed_stride(a) + 6);
    a.cid[(long)b * a.P + i] = cid;
    a.slot[(long)b * a.P + i] = atomicAdd(&cnt[cid], 1);             // which slot is whose is not defined; no result depends on it
}

__global__ __launch_bounds__(GW) void k_fg_starts(BinDev a) {
    __shared__ int buf[GW];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int nc = a.grid[b].ncells + 1;
    const int* cnt = reinterpret_cast<const int*>(a.zeroed + (size_t)b * zeroed_stride(a) + 6);
    int* start = a.start + (long)b * (a.cells_cap + 2);
    const int per = (nc + GW - 1) / GW;
    const int c0 = min(nc, tid * per), c1 = min(nc, c0 + per);
    int mine = 0;
    for (int c = c0; c < c1; ++c) mine += cnt[c];
    buf[tid] = mine;
    __syncthreads();
    for (int off = 1; off < GW; off <<= 1) {                         // Hillis-Steele on integers
        int o = 0;
        if (tid >= off) o = buf[tid - off];
        __syncthreads();
        buf[tid] += o;
        __syncthreads();
    }
    int run = buf[tid] - mine;
    for (int c = c0; c < c1; ++c) { start[c] = run; run += cnt[c]; }
    if (tid == GW - 1) start[nc] = buf[GW - 1];                      // = the cloud's points
}

__global__ __launch_bounds__(BW) void k_fg_scatter(BinDev a) {
    const int b = blockIdx.y, i = blockIdx.x * BW + threadIdx.x;
    if (i >= cloud_points(a, b)) return;
    const float* p = a.pos + (a.pt_off[(long)b * a.stride] + i) * 3;
    const int at = a.start[(long)b * (a.cells_cap + 2) + a.cid[(long)b * a.P + i]] + a.slot[(long)b * a.P + i];
    a.sorted[(long)b * a.P + at] = make_float4(p[0], p[1], p[2], __int_as_float(i));
    a.md[(long)b * a.P + at] = a.md0;
}

__global__ __launch_bounds__(BW) void k_fg_boxes(BinDev a) {
    const int b = blockIdx.y, lane = threadIdx.x & 63;
    const int c = blockIdx.x * (BW / 64) + (threadIdx.x >> 6);
    const int ncells = a.grid[b].ncells;
    if (c > ncells) return;                                          // wave-uniform
    const int* start = a.start + (long)b * (a.cells_cap + 2);
    const int s = start[c], e = start[c + 1];
    const float4* sorted = a.sorted + (long)b * a.P;
    const float INF = __builtin_huge_valf();
    float lo[3] = {INF, INF, INF}, hi[3] = {-INF, -INF, -INF};
    int first = 0x7fffffff;
    for (int i = s + lane; i < e; i += 64) {
        const float4 q = sorted[i];
        lo[0] = fminf(lo[0], q.x); lo[1] = fminf(lo[1], q.y); lo[2] = fminf(lo[2], q.z);
        hi[0] = fmaxf(hi[0], q.x); hi[1] = fmaxf(hi[1], q.y); hi[2] = fmaxf(hi[2], q.z);
        first = min(first, __float_as_int(q.w));
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
        for (int k = 0; k < 3; ++k) { lo[k] = fminf(lo[k], __shfl_xor(lo[k], o)); hi[k] = fmaxf(hi[k], __shfl_xor(hi[k], o)); }
        first = min(first, __shfl_xor(first, o));
    }
    if (lane != 0) return;
    float* box = a.box + ((long)b * (a.cells_cap + 1) + c) * 6;
    // the non-finite cell's box is all of space: gap 0, bound 0, visited while its maximum is positive (it stays at md0)
    const bool plain = e > s && c != ncells, open = c == ncells;
    for (int k = 0; k < 3; ++k) { box[k] = plain ? lo[k] : open ? -INF : 0.0f; box[3 + k] = plain ? hi[k] : open ? INF : 0.0f; }
    // every member starts at md0, so the cell's key is md0 at its lowest original index; an empty cell's key 0 loses everywhere
    a.key0[(long)b * (a.cells_cap + 1) + c] = e > s ? fps_key(a.md0, first) : 0ull;
}

// ---------------------------------------------------------------------------------------------- selection
// Stage 2's square root is np.linalg.norm's: correctly rounded (and with that monotone, which the bound needs).  sqrtf is that -
// hipcc's default -fhip-fp32-correctly-rounded-divide-sqrt.  __fsqrt_rn is NOT with this toolchain's headers: unless
// OCML_BASIC_ROUNDED_OPERATIONS is defined it is the native square root, good to 1 ulp (DESIGN.md section 3.27 has what follows).
__device__ __forceinline__ float sqrt_exact(float x) { return sqrtf(x); }

// One point of a visit: k_fps_cloud's / fps_stage2's update of the running minimum, and the lane's running key.
template <bool STAGE2>
__device__ __forceinline__ float select_visit(float4 q, float m, float cx, float cy, float cz, unsigned long long& best) {
    float d = dist_exact(q.x, q.y, q.z, cx, cy, cz);
    if (STAGE2) d = sqrt_exact(d);
    m = m > d ? d : m;
    const unsigned long long key = fps_key(m, __float_as_int(q.w));
    best = key > best ? key : best;
    return m;
}

// The cell that lane `lane` of wavefront `wave` owns in table slot j: a bijection between (j, lane, wave) and the cells.  16
// consecutive cells go to 16 different wavefronts, and - the wavefront being the cell's low four bits XOR three higher groups of
// four - so do cells that are 16, 256 or 4096 apart: with power-of-two cells per axis, the neighbours of a cell along every axis.
__device__ __forceinline__ int owned_cell(int j, int lane, int wave) {
    const int rest = j * 64 + lane;
    return rest * GWAVES + ((wave ^ rest ^ (rest >> 4) ^ (rest >> 8)) & (GWAVES - 1));
}

template <bool STAGE2, bool INLDS>
__global__ __launch_bounds__(GW) void k_fps_select(SelDev a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned long long* wkey = reinterpret_cast<unsigned long long*>(smem);          // [2][GWAVES]
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const BinDev& g = a.bin;
    const int Q = a.max_nobj;
    const int n = cloud_points(g, b);
    if (n == 0) {
        if (STAGE2) {
            for (int t = tid; t < Q; t += GW) a.fps_idx[(long)b * Q + t] = -1;
            if (tid == 0) a.n_obj[b] = 0;
        } else if (tid == 0) { a.off2[b] = (long long)b * Q; a.n2[b] = 0; }
        return;
    }
    const float* p = g.pos + g.pt_off[(long)b * g.stride] * 3;
    const int ncp = INLDS ? LDS_SLOTS * GW : (int)tab_cells(g.cells_cap);
    // the per-cell tables, one entry per (slot, thread): key | box lo xyz hi xyz | start | count
    unsigned long long* key; float* bx; int* cst; int* ccnt;
    if constexpr (INLDS) key = reinterpret_cast<unsigned long long*>(smem + SEL_LDS_HEAD);
    else key = reinterpret_cast<unsigned long long*>(a.tab + (size_t)b * a.tab_bytes);
    bx = reinterpret_cast<float*>(key + ncp); cst = reinterpret_cast<int*>(bx + 6 * (size_t)ncp); ccnt = cst + ncp;
    const int nc = g.grid[b].ncells + 1;
    const int slots = (nc + GW - 1) / GW;                            // <= ncp / GW: nc <= cells_cap + 1
    {
        const int* start = g.start + (long)b * (g.cells_cap + 2);
        const float* box = g.box + (long)b * (g.cells_cap + 1) * 6;
        const unsigned long long* key0 = g.key0 + (long)b * (g.cells_cap + 1);
        for (int j = 0; j < slots; ++j) {
            const int o = j * GW + tid, c = owned_cell(j, lane, wave);
            const bool live = c < nc;
            key[o] = live ? key0[c] : 0ull;
#pragma unroll
            for (int k = 0; k < 6; ++k) bx[k * (size_t)ncp + o] = live ? box[(long)c * 6 + k] : 0.0f;
            cst[o] = live ? start[c] : 0;
            ccnt[o] = live ? start[c + 1] - start[c] : 0;
        }
    }   // (a thread reads back its own entries only: no barrier)
    const float4* __restrict__ sorted = g.sorted + (long)b * g.P;
    float* __restrict__ md = g.md + (long)b * g.P;
    int* out = a.fps_idx + (long)b * Q;
    const int n1 = STAGE2 ? n : min(Q, n);
    const float radius = STAGE2 ? a.radius[b] : 0.0f;
    int cur = min(max(a.first[b], 0), n - 1);                        // (stage 2: n == n1)
    int it = 0, count = 0;
    while (true) {
        const float cx = p[3 * (long)cur], cy = p[3 * (long)cur + 1], cz = p[3 * (long)cur + 2];   // same address in every lane
        if (tid == 0) {
            if (STAGE2) out[count] = a.s1idx[(long)b * Q + cur];
            else {
                a.s1idx[(long)b * Q + count] = cur;
                float* s = a.s1pos + ((long)b * Q + count) * 3;
                s[0] = cx; s[1] = cy; s[2] = cz;
            }
        }
        ++count;
        if (!STAGE2 && count >= n1) break;
        // ---- every lane tests its cells: no load of a slot waits for another slot's
        unsigned long long mine = 0;
        unsigned vis = 0;                                            // bit j: my cell of slot j is visited
#pragma unroll 4
        for (int j = 0; j < slots; ++j) {
            const int o = j * GW + tid;
            const unsigned long long kk = key[o];
            // the cell's bound: dist_exact of the per-axis gaps max(lo - c, c - hi, 0)
            const float gx = fmaxf(fmaxf(__fsub_rn(bx[o], cx), __fsub_rn(cx, bx[3 * (size_t)ncp + o])), 0.0f);
            const float gy = fmaxf(fmaxf(__fsub_rn(bx[(size_t)ncp + o], cy), __fsub_rn(cy, bx[4 * (size_t)ncp + o])), 0.0f);
            const float gz = fmaxf(fmaxf(__fsub_rn(bx[2 * (size_t)ncp + o], cz), __fsub_rn(cz, bx[5 * (size_t)ncp + o])), 0.0f);
            float bound = dist_exact(gx, gy, gz, 0.0f, 0.0f, 0.0f);
            if (STAGE2) bound = sqrt_exact(bound);
            // a NaN bound visits; key 0 is an empty cell (a member's key holds its inverted index, never 0)
            const bool visit = !(bound >= __uint_as_float((unsigned)(kk >> 32))) && kk != 0ull;
            vis |= visit ? 1u << j : 0u;
            mine = visit || mine > kk ? mine : kk;
        }
        // ---- the wavefront visits them, 64 members at a time, and refreshes their keys
        for (int j = 0; j < slots; ++j) {
            const bool visit = (vis >> j & 1u) != 0u;
            unsigned long long todo = __ballot(visit);
            if (todo == 0ull) continue;                              // wave-uniform
            const int o = j * GW + tid;
            int my_s = 0, my_n = 0;
            if (visit) { my_s = cst[o]; my_n = ccnt[o]; }
            unsigned long long kk = 0;
            while (todo) {                                           // wave-uniform
                const int L = __ffsll((long long)todo) - 1;
                todo &= todo - 1;
                const int s = __shfl(my_s, L), e = s + __shfl(my_n, L);
                unsigned long long best = 0;
                for (int base = s; base < e; base += 4 * 64) {
                    float4 q[4]; float m[4];
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        const int i = base + u * 64 + lane;
                        if (i < e) { q[u] = sorted[i]; m[u] = md[i]; }
                    }
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        const int i = base + u * 64 + lane;
                        if (i < e) md[i] = select_visit<STAGE2>(q[u], m[u], cx, cy, cz, best);
                    }
                }
                best = wave_max_u64(best);
                if (lane == L) kk = best;
            }
            if (visit) { key[o] = kk; mine = kk > mine ? kk : mine; }
        }
        const unsigned long long gk = block_max_u64<GWAVES>(mine, wkey, it);          // the same value in every thread
        if (STAGE2 && (!(__uint_as_float((unsigned)(gk >> 32)) > radius) || count >= n1)) break;
        cur = (int)(0xffffffffu - (unsigned)(gk & 0xffffffffull));
    }
    if (STAGE2) {
        for (int t = count + tid; t < Q; t += GW) out[t] = -1;
        if (tid == 0) a.n_obj[b] = count;
    } else if (tid == 0) { a.off2[b] = (long long)b * Q; a.n2[b] = n1; }
}

// ---------------------------------------------------------------------------------------------- host
static BinDev bin_dev(const FpsBinWs& w, const float* pos, const long long* pt_off, const long long* npts, int stride, int P,
                      int cells, float md0) {
    BinDev d;
    d.pos = pos; d.pt_off = pt_off; d.npts = npts; d.stride = stride; d.P = P; d.cells = cells; d.cells_cap = w.cells_cap; d.md0 = md0;
    d.zeroed = w.zeroed; d.grid = reinterpret_cast<FpsGrid*>(w.grid); d.start = w.start; d.cid = w.cid; d.slot = w.slot;
    d.sorted = reinterpret_cast<float4*>(w.sorted); d.md = w.md; d.box = w.box; d.key0 = w.key0;
    return d;
}

static hipError_t launch_bin(const BinDev& d, const FpsBinWs& w, int B, hipStream_t st) {
    if (hipError_t e = hipMemsetAsync(w.zeroed, 0, w.zeroed_words * 4, st); e != hipSuccess) return e;
    const int per_point = (d.P + BW - 1) / BW;
    hipLaunchKernelGGL(k_fg_bounds, dim3(std::min(per_point, 256), B), dim3(BW), 0, st, d);
    hipLaunchKernelGGL(k_fg_grid, dim3((B + 63) / 64), dim3(64), 0, st, d, B);
    hipLaunchKernelGGL(k_fg_bin, dim3(per_point, B), dim3(BW), 0, st, d);
    hipLaunchKernelGGL(k_fg_starts, dim3(B), dim3(GW), 0, st, d);
    hipLaunchKernelGGL(k_fg_scatter, dim3(per_point, B), dim3(BW), 0, st, d);
    hipLaunchKernelGGL(k_fg_boxes, dim3((d.cells_cap + 1 + BW / 64 - 1) / (BW / 64), B), dim3(BW), 0, st, d);
    return hipGetLastError();
}

template <bool STAGE2>
static hipError_t launch_select(const SelDev& s, int B, hipStream_t st) {
    if (s.bin.cells_cap > FPS_GRID_LDS_CELLS) {
        hipLaunchKernelGGL((k_fps_select<STAGE2, false>), dim3(B), dim3(GW), SEL_LDS_HEAD, st, s);
        return hipGetLastError();
    }
    const int lds = SEL_LDS_HEAD + LDS_SLOTS * GW * CELL_BYTES;      // above 64 KB: a per-device opt-in of the function
    static std::atomic<unsigned long long> done{0};
    if (hipError_t e = lds_opt_in(done, lds, k_fps_select<STAGE2, true>); e != hipSuccess) return e;
    hipLaunchKernelGGL((k_fps_select<STAGE2, true>), dim3(B), dim3(GW), lds, st, s);
    return hipGetLastError();
}

hipError_t launch_fps_grid(const FpsGridArgs& h, hipStream_t st) {
    SelDev s{};
    s.max_nobj = h.max_nobj; s.radius = h.fps_radius;
    s.s1pos = h.s1pos; s.s1idx = h.s1idx; s.off2 = h.off2; s.n2 = h.n2; s.fps_idx = h.fps_idx; s.n_obj = h.n_obj;
    // ---- stage 1 over the clouds: initial minimum 1e10
    s.bin = bin_dev(h.w1, h.pos, h.pt_off, h.npts, h.stride, h.max_pts, h.cells, 1e10f);
    s.first = h.fps_start; s.tab = h.w1.tab; s.tab_bytes = fps_grid_tab_bytes(h.w1.cells_cap);
    if (hipError_t e = launch_bin(s.bin, h.w1, h.B, st); e != hipSuccess) return e;
    if (hipError_t e = launch_select<false>(s, h.B, st); e != hipSuccess) return e;
    // ---- stage 2 over the stage-1 points in selection order: initial minimum +inf
    s.bin = bin_dev(h.w2, h.s1pos, h.off2, h.n2, 1, h.max_nobj, h.cells, __builtin_huge_valf());
    s.first = h.rad_start; s.tab = h.w2.tab; s.tab_bytes = fps_grid_tab_bytes(h.w2.cells_cap);
    if (hipError_t e = launch_bin(s.bin, h.w2, h.B, st); e != hipSuccess) return e;
    return launch_select<true>(s, h.B, st);
}

}  // namespace ag
