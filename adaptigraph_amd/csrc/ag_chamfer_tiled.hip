// chamfer(x, y) and its gradient toward x for clouds of any size up to CHAMFER_TILED_MAX_POINTS each: what
// k_chamfer / k_chamfer_nn / k_chamfer_grad of ag_cost.hip compute, with k_chamfer's bits, from kernels whose LDS does not grow
// with the clouds and whose rows are spread over many workgroups.  gfx950 only.
//
//   k_chamfer_tiled_nn     a workgroup owns up to 1024 consecutive points of one cloud of one row (4 per lane, in registers) and
//                          streams the other cloud through LDS in tiles; per owned point the smallest squared distance (the
//                          forward) or the index of the nearest point (the gradient) goes to a per-point table
//   k_chamfer_tiled_final  one workgroup per row: k_chamfer's sums over the table, in k_chamfer's order
//   k_chamfer_tiled_count  one workgroup per row: the valid points of both clouds (the gradient's means)
//   k_chamfer_tiled_grad   one thread per x point: k_chamfer_grad over the arg-min table
// No atomics; every sum has a fixed order.  The helpers restate ag_cost.hip's (file-local there), expression for expression.
#include "ag_chamfer_tiled.h"

namespace ag {
namespace {

constexpr int CT = 256, CH_PT = 4;
constexpr int OWN = CHAMFER_TILED_OWN;
static_assert(OWN == CT * CH_PT, "a lane owns CH_PT consecutive points");
constexpr float BIG = 3.0e38f;         // where masked-out points and the pad are parked: (BIG - finite)^2 = +inf
typedef float f2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ float block_sum(float v, float* red) {
    const int tid = threadIdx.x;
    red[tid] = v;
    __syncthreads();
    for (int o = CT / 2; o > 0; o >>= 1) {
        if (tid < o) red[tid] += red[tid + o];
        __syncthreads();
    }
    const float r = red[0];
    __syncthreads();
    return r;
}
__device__ __forceinline__ float nan_min(float a, float b) { return a != a ? a : b != b ? b : fminf(a, b); }
__device__ __forceinline__ bool finite3(float a, float b, float c) {
    return __builtin_isfinite(a) && __builtin_isfinite(b) && __builtin_isfinite(c);
}

struct TiledDev {
    const float* x; const float* y; const uint8_t* xm; const uint8_t* ym;
    int R, N, M, By, tile, bx, by;     // bx, by: owning blocks of x and of y per row
    float* d2; int* nn;                // (R, N+M) tables: the x points' entries, then the y points'
};

// k_chamfer's sweep over `cnt` (even) tile points, SoA with stride `ts`: two tile points per step on the packed fp32 pipe.
__device__ __forceinline__ void tile_sweep(const float* os, int ts, int cnt, const float (&qx)[CH_PT], const float (&qy)[CH_PT],
                                           const float (&qz)[CH_PT], float (&m)[CH_PT]) {
    const f2* ox = reinterpret_cast<const f2*>(os);
    const f2* oy = reinterpret_cast<const f2*>(os + ts);
    const f2* oz = reinterpret_cast<const f2*>(os + 2 * ts);
    for (int i = 0; i < cnt / 2; ++i) {
        const f2 px = ox[i], py = oy[i], pz = oz[i];
#pragma unroll
        for (int k = 0; k < CH_PT; ++k) {
            const f2 dx = px - qx[k], dy = py - qy[k], dz = pz - qz[k];
            const f2 d = __builtin_elementwise_fma(dz, dz, __builtin_elementwise_fma(dy, dy, dx * dx));
            m[k] = fminf(fminf(m[k], d.x), d.y);
        }
    }
}
// The same distances with the arg-min carried along: strict <, points in ascending order, so the lowest index wins among equal
// distances - inside a tile and, the tiles coming in ascending order, across them (chamfer_nearest of ag_cost.hip).
__device__ __forceinline__ void tile_sweep_arg(const float* os, int ts, int cnt, int t0, const float (&qx)[CH_PT],
                                               const float (&qy)[CH_PT], const float (&qz)[CH_PT], float (&m)[CH_PT],
                                               int (&arg)[CH_PT]) {
    const f2* ox = reinterpret_cast<const f2*>(os);
    const f2* oy = reinterpret_cast<const f2*>(os + ts);
    const f2* oz = reinterpret_cast<const f2*>(os + 2 * ts);
    for (int i = 0; i < cnt / 2; ++i) {
        const f2 px = ox[i], py = oy[i], pz = oz[i];
#pragma unroll
        for (int k = 0; k < CH_PT; ++k) {
            const f2 dx = px - qx[k], dy = py - qy[k], dz = pz - qz[k];
            const f2 d = __builtin_elementwise_fma(dz, dz, __builtin_elementwise_fma(dy, dy, dx * dx));
            if (d.x < m[k]) { m[k] = d.x; arg[k] = t0 + 2 * i; }
            if (d.y < m[k]) { m[k] = d.y; arg[k] = t0 + 2 * i + 1; }
        }
    }
}

// ARG = false: d2 gets min_j |o_j - q|^2 per owned point (BIG where nothing is below it, as k_chamfer's register starts there).
// ARG = true:  nn gets the arg-min (-1: the owned point is masked out, or nothing is nearer than BIG), as k_chamfer_nn writes it.
// Which points count comes from index and mask only; a masked-out slot's value is never read.
template <bool ARG>
__global__ __launch_bounds__(CT) void k_chamfer_tiled_nn(TiledDev a) {
    extern __shared__ __attribute__((aligned(16))) float sm[];   // [3][tile]
    const int tid = threadIdx.x;
    const int nblk = a.bx + a.by;
    const int r = blockIdx.x / nblk, b = blockIdx.x % nblk;
    const bool own_x = b < a.bx;
    const int ry = a.By == 1 ? 0 : r;
    const float* xr = a.x + (long)r * a.N * 3;
    const float* yr = a.y + (long)ry * a.M * 3;
    const uint8_t* xm = a.xm ? a.xm + (long)r * a.N : nullptr;
    const uint8_t* ym = a.ym ? a.ym + (long)ry * a.M : nullptr;
    const float* own = own_x ? xr : yr;  const uint8_t* ownm = own_x ? xm : ym;  const int on = own_x ? a.N : a.M;
    const float* oth = own_x ? yr : xr;  const uint8_t* othm = own_x ? ym : xm;  const int tn = own_x ? a.M : a.N;
    const int o0 = (own_x ? b : b - a.bx) * OWN + tid * CH_PT;   // this lane's first owned point

    float qx[CH_PT], qy[CH_PT], qz[CH_PT], m[CH_PT], slow[CH_PT];
    int arg[CH_PT];
    bool v[CH_PT];
    int own_odd = 0;
#pragma unroll
    for (int k = 0; k < CH_PT; ++k) {
        const int i = o0 + k;
        v[k] = i < on && (ownm ? ownm[i] != 0 : true);
        qx[k] = BIG; qy[k] = BIG; qz[k] = BIG;
        if (v[k]) { qx[k] = own[3 * (long)i]; qy[k] = own[3 * (long)i + 1]; qz[k] = own[3 * (long)i + 2]; }
        own_odd |= !finite3(qx[k], qy[k], qz[k]);
        m[k] = BIG; slow[k] = __builtin_inff(); arg[k] = -1;
    }
    // fminf drops NaN and the parking needs finite points (ag_cost.hip, chamfer_nearest_nan): a tile with a non-finite valid point,
    // and every tile of a workgroup that owns one, is walked point by point with torch.min's rule instead.  The arg-min variant
    // does what k_chamfer_nn does on such input: nothing special.
    if (!ARG) own_odd = __syncthreads_or(own_odd);
    bool slow_seen = false;
    for (int t0 = 0; t0 < tn; t0 += a.tile) {
        const int cnt = min(a.tile, tn - t0), pad = (cnt + 1) & ~1;          // pad <= tile: the tile is even
        int odd = 0;
        for (int i = tid; i < pad; i += CT) {
            const int j = t0 + i;
            const bool ok = i < cnt && (othm ? othm[j] != 0 : true);
            float px = BIG, py = BIG, pz = BIG;
            if (ok) { px = oth[3 * (long)j]; py = oth[3 * (long)j + 1]; pz = oth[3 * (long)j + 2]; }
            sm[i] = px; sm[a.tile + i] = py; sm[2 * a.tile + i] = pz;
            odd |= !finite3(px, py, pz);
        }
        if (ARG) {
            __syncthreads();
            tile_sweep_arg(sm, a.tile, pad, t0, qx, qy, qz, m, arg);
        } else {
            odd = __syncthreads_or(odd) | own_odd;                           // (the barrier the fill needs anyway)
            if (odd) {
                slow_seen = true;
#pragma unroll
                for (int k = 0; k < CH_PT; ++k) {
                    if (!v[k]) continue;
                    for (int j = t0; j < t0 + cnt; ++j) {
                        if (othm && othm[j] == 0) continue;
                        const float dx = oth[3 * (long)j] - qx[k], dy = oth[3 * (long)j + 1] - qy[k], dz = oth[3 * (long)j + 2] - qz[k];
                        slow[k] = nan_min(slow[k], __builtin_fmaf(dz, dz, __builtin_fmaf(dy, dy, dx * dx)));
                    }
                }
            } else {
                tile_sweep(sm, a.tile, pad, qx, qy, qz, m);
            }
        }
        __syncthreads();                                                     // the tile is free again
    }
    const long row = (long)r * ((long)a.N + a.M) + (own_x ? 0 : a.N);
#pragma unroll
    for (int k = 0; k < CH_PT; ++k) {
        const int i = o0 + k;
        if (i >= on) continue;
        if (ARG) a.nn[row + i] = (v[k] && qx[k] < BIG) ? arg[k] : -1;
        // a row that went round the sweep is non-finite in chamfer() too: NaN where a distance was, +inf where all were infinite
        else a.d2[row + i] = slow_seen ? nan_min(slow[k], m[k] < BIG ? m[k] : __builtin_inff()) : m[k];
    }
}

struct FinalDev { const float* d2; const uint8_t* xm; const uint8_t* ym; float* out; int N, M, By; };
// k_chamfer's reduction: lane tid adds sqrtf(d2[j]) for j = tid*4 + k + 1024*s over the valid points, k = 0..3 inside s = 0, 1, ..;
// the counts likewise; then the four trees.
__global__ __launch_bounds__(CT) void k_chamfer_tiled_final(FinalDev a) {
    __shared__ float red[CT];
    const int r = blockIdx.x, tid = threadIdx.x;
    const float* dx = a.d2 + (long)r * ((long)a.N + a.M);
    const float* dy = dx + a.N;
    const uint8_t* xm = a.xm ? a.xm + (long)r * a.N : nullptr;
    const uint8_t* ym = a.ym ? a.ym + (long)(a.By == 1 ? 0 : r) * a.M : nullptr;
    float sum_y = 0.f, cnt_y = 0.f, sum_x = 0.f, cnt_x = 0.f;
    for (int j0 = tid * CH_PT; j0 < a.M; j0 += CT * CH_PT)
#pragma unroll
        for (int k = 0; k < CH_PT; ++k)
            if (j0 + k < a.M && (!ym || ym[j0 + k] != 0)) { sum_y += sqrtf(dy[j0 + k]); cnt_y += 1.f; }
    for (int i0 = tid * CH_PT; i0 < a.N; i0 += CT * CH_PT)
#pragma unroll
        for (int k = 0; k < CH_PT; ++k)
            if (i0 + k < a.N && (!xm || xm[i0 + k] != 0)) { sum_x += sqrtf(dx[i0 + k]); cnt_x += 1.f; }
    const float sy = block_sum(sum_y, red), cy = block_sum(cnt_y, red);
    const float sx = block_sum(sum_x, red), cx = block_sum(cnt_x, red);
    if (tid == 0) a.out[r] = sy / cy + sx / cx;
}

// cnt[r] = {valid x, valid y}: whole numbers below 2^24, exact in fp32 in any order
__global__ __launch_bounds__(CT) void k_chamfer_tiled_count(const uint8_t* xmask, const uint8_t* ymask, int N, int M, int By, float* cnt) {
    __shared__ float red[CT];
    const int r = blockIdx.x, tid = threadIdx.x;
    const uint8_t* xm = xmask ? xmask + (long)r * N : nullptr;
    const uint8_t* ym = ymask ? ymask + (long)(By == 1 ? 0 : r) * M : nullptr;
    float cx = 0.f, cy = 0.f;
    for (int i = tid; i < N; i += CT) cx += (!xm || xm[i] != 0) ? 1.f : 0.f;
    for (int j = tid; j < M; j += CT) cy += (!ym || ym[j] != 0) ? 1.f : 0.f;
    const float sx = block_sum(cx, red), sy = block_sum(cy, red);
    if (tid == 0) { cnt[2 * r] = sx; cnt[2 * r + 1] = sy; }
}

__device__ __forceinline__ void chamfer_pull(const float* xi, const float* yj, float w, float (&g)[3]) {
    const float dx = xi[0] - yj[0], dy = xi[1] - yj[1], dz = xi[2] - yj[2];
    const float dist = sqrtf(dx * dx + dy * dy + dz * dz);
    if (!(dist > 0.f)) return;                                       // torch: the norm's gradient at zero is zero
    const float s = w / dist;
    g[0] += dx * s; g[1] += dy * s; g[2] += dz * s;
}
// k_chamfer_grad with the row taken from the block index (a workgroup lies inside one row, so the walk over the y table reads
// wave-uniform addresses): the thread of x_i takes its own term, then the y points whose arg-min is i, in ascending j.
__global__ __launch_bounds__(CT) void k_chamfer_tiled_grad(TiledDev a, const float* cnt, const float* gout, float* gx) {
    const int nb = (a.N + CT - 1) / CT;
    const int r = blockIdx.x / nb, i = (blockIdx.x % nb) * CT + threadIdx.x;
    if (i >= a.N) return;
    const long t = (long)r * a.N + i;
    const int* row = a.nn + (long)r * ((long)a.N + a.M);
    const float* xi = a.x + t * 3;
    const float* yr = a.y + (long)(a.By == 1 ? 0 : r) * a.M * 3;
    float g[3] = {0.f, 0.f, 0.f};
    const int j0 = row[i];
    if (j0 >= 0) {                                                   // (j0 < 0: x_i is masked out, nothing reaches it)
        const float go = gout[r];
        chamfer_pull(xi, yr + 3 * (long)min(j0, a.M - 1), go / cnt[2 * r], g);
        const float wy = go / cnt[2 * r + 1];
        for (int j = 0; j < a.M; ++j)
            if (row[a.N + j] == i) chamfer_pull(xi, yr + 3 * (long)j, wy, g);
    }
    gx[t * 3] = g[0]; gx[t * 3 + 1] = g[1]; gx[t * 3 + 2] = g[2];
}

TiledDev tiled_args(const float* x, const float* y, const uint8_t* xm, const uint8_t* ym, int R, int N, int M, int By, int tile) {
    TiledDev a{x, y, xm, ym, R, N, M, By, tile, (N + OWN - 1) / OWN, (M + OWN - 1) / OWN, nullptr, nullptr};
    return a;
}

}  // namespace

hipError_t launch_chamfer_tiled(const float* x, const float* y, const uint8_t* xm, const uint8_t* ym, int R, int N, int M, int By,
                                int tile, float* d2, float* out, hipStream_t st) {
    TiledDev a = tiled_args(x, y, xm, ym, R, N, M, By, tile);
    a.d2 = d2;
    const unsigned blocks = (unsigned)((long)(a.bx + a.by) * R);
    hipLaunchKernelGGL(k_chamfer_tiled_nn<false>, dim3(blocks), dim3(CT), (size_t)tile * 12, st, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    FinalDev f{d2, xm, ym, out, N, M, By};
    hipLaunchKernelGGL(k_chamfer_tiled_final, dim3(R), dim3(CT), 0, st, f);
    return hipGetLastError();
}

hipError_t launch_chamfer_tiled_backward(const float* x, const float* y, const uint8_t* xm, const uint8_t* ym, int R, int N, int M,
                                         int By, int tile, const float* gout, int* nn, float* cnt, float* gx, hipStream_t st) {
    TiledDev a = tiled_args(x, y, xm, ym, R, N, M, By, tile);
    a.nn = nn;
    const unsigned blocks = (unsigned)((long)(a.bx + a.by) * R);
    hipLaunchKernelGGL(k_chamfer_tiled_nn<true>, dim3(blocks), dim3(CT), (size_t)tile * 12, st, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_chamfer_tiled_count, dim3(R), dim3(CT), 0, st, xm, ym, N, M, By, cnt);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    const unsigned gblocks = (unsigned)((long)((N + CT - 1) / CT) * R);
    hipLaunchKernelGGL(k_chamfer_tiled_grad, dim3(gblocks), dim3(CT), 0, st, a, (const float*)cnt, gout, gx);
    return hipGetLastError();
}

}  // namespace ag
