// Training-batch construction: the sampling and assembly half of DynDataset.__getitem__ (reference
// src/dynamics/dataset/dataset.py:117-300) for B samples per launch.  gfx950 only.
//
//   k_fps_batch         both farthest-point stages (dataset/graph.py:8-36) of B samples, one workgroup per sample
//   k_dataset_assemble  every dense tensor of the batch, zero padding included, straight from the flat episode buffers
//   k_fps_cloud         k_fps_batch's two stages for clouds beyond LDS (perception.py:259-315), the cloud read from global memory
//
// Indices and un-augmented tensors must equal the reference bit for bit, so the fp32 arithmetic is spelled out:
//   stage 1 (dgl.geometry.farthest_point_sampler, restated from its CPU implementation - dgl is not available to check
//   against): running minimum of ((dx*dx + dy*dy) + dz*dz), separate mul/add, initialised to 1e10; the next point is the
//   strict-greater argmax, i.e. the LOWEST index among equal distances; the first point is given.
//   stage 2 (fps_rad_idx, src/dynamics/utils.py:10-24) on the stage-1 points in their order: the same sum, then a correctly
//   rounded sqrt (np.linalg.norm); while max > radius (fp32 against fp32): append the argmax (lowest index), take the minimum.
// The argmax is one max-reduction over a packed 64-bit key: distance bits above (non-negative floats order as integers),
// inverted index below - the largest key is the largest distance at the lowest index, no second pass.  The running minima
// live in registers (PPT points per thread), the cloud in LDS as SoA; one barrier per selected point.
// No atomics: every output has one writer.
#include "../../include/adaptigraph_amd.h"
#include "ag_dataset.h"
#include "ag_dist.h"
#include "ag_fps_key.h"
#include "ag_lds_optin.h"

namespace ag {

constexpr int FW = 256;                 // threads per workgroup: 4 wavefronts, so the cross-wave step reads 4 keys
constexpr int FWAVES = FW / 64;
constexpr int FPS_PPT_MAX = 32;         // points per thread of the largest instantiation
constexpr int FPS_MAX_POINTS = FW * FPS_PPT_MAX;   // 8192 points: 96 KB of the CU's 160 KB of LDS for the cloud
constexpr int FPS_PPT2 = 4;
constexpr int FPS_MAX_NOBJ = FW * FPS_PPT2;        // 1024 stage-1 points (16 KB), stage 2 keeps 4 per thread

size_t fps_max_points() { return FPS_MAX_POINTS; }
int fps_max_nobj() { return FPS_MAX_NOBJ; }

// Stage 2 (fps_rad_idx) on the n1 stage-1 points sx / sy / sz (LDS, selection order; sidx: their cloud indices), starting at
// `cur`, by a workgroup of W threads that keeps PPT2 points each (W * PPT2 >= n1): writes the kept cloud indices to out[] in
// selection order and returns their count, the same value in every thread.
template <int W, int PPT2>
__device__ __forceinline__ int fps_stage2(const float* sx, const float* sy, const float* sz, const int* sidx, int n1, float radius,
                                          int cur, int* out, unsigned long long* wkey, int& it) {
    const int tid = threadIdx.x;
    float m2[PPT2];
#pragma unroll
    for (int u = 0; u < PPT2; ++u) m2[u] = __builtin_huge_valf();
    int count = 0;
    while (true) {
        if (tid == 0) out[count] = sidx[cur];
        ++count;
        const float cx = sx[cur], cy = sy[cur], cz = sz[cur];
        unsigned long long best = 0;
#pragma unroll
        for (int u = 0; u < PPT2; ++u) {
            const int i = u * W + tid;
            if (i < n1) {
                const float d = __fsqrt_rn(dist_exact(sx[i], sy[i], sz[i], cx, cy, cz));
                m2[u] = m2[u] > d ? d : m2[u];
                const unsigned long long key = fps_key(m2[u], i);
                best = key > best ? key : best;
            }
        }
        const unsigned long long g = block_max_u64<W / 64>(best, wkey, it);           // the same value in every thread
        if (!(__uint_as_float((unsigned)(g >> 32)) > radius) || count >= n1) break;
        cur = (int)(0xffffffffu - (unsigned)(g & 0xffffffffull));
    }
    return count;
}

struct FpsDev {
    const float* pos; const long long* pt_off; const long long* npts; int stride;
    const int* fps_start; const float* fps_radius; const int* rad_start;
    int max_nobj, max_pts, pad;          // pad: floats per LDS coordinate array
    int* fps_idx; int* n_obj;
};
inline size_t fps_lds_bytes(int pad, int max_nobj) { return 64 + (size_t)pad * 12 + (size_t)max_nobj * 16; }

template <int PPT>
__global__ __launch_bounds__(FW) void k_fps_batch(FpsDev a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned long long* wkey = reinterpret_cast<unsigned long long*>(smem);          // [2][FWAVES]
    float* x = reinterpret_cast<float*>(smem + 64);
    float* y = x + a.pad;
    float* z = y + a.pad;
    float* sx = z + a.pad;               // stage-1 points in selection order
    float* sy = sx + a.max_nobj;
    float* sz = sy + a.max_nobj;
    int* sidx = reinterpret_cast<int*>(sz + a.max_nobj);
    const int b = blockIdx.x, tid = threadIdx.x;
    int* out = a.fps_idx + (long)b * a.max_nobj;
    const long long nraw = a.npts[(long)b * a.stride];
    // (the host refuses clouds above max_pts before it enqueues; the clamp keeps a wrong count inside the LDS arrays)
    const int n = (int)(nraw < 0 ? 0 : nraw > (long long)a.max_pts ? (long long)a.max_pts : nraw);
    if (n == 0) {
        for (int t = tid; t < a.max_nobj; t += FW) out[t] = -1;
        if (tid == 0) a.n_obj[b] = 0;
        return;
    }
    const float* p = a.pos + a.pt_off[(long)b * a.stride] * 3;
    for (int i = tid; i < n; i += FW) { x[i] = p[3 * (long)i]; y[i] = p[3 * (long)i + 1]; z[i] = p[3 * (long)i + 2]; }
    __syncthreads();
    int it = 0;
    // ---- stage 1
    const int n1 = min(a.max_nobj, n);
    float md[PPT];
#pragma unroll
    for (int u = 0; u < PPT; ++u) md[u] = 1e10f;
    int cur = min(max(a.fps_start[b], 0), n - 1);
    if (tid == 0) { sidx[0] = cur; sx[0] = x[cur]; sy[0] = y[cur]; sz[0] = z[cur]; }
    for (int k = 1; k < n1; ++k) {
        const float cx = x[cur], cy = y[cur], cz = z[cur];                            // same address in every lane: broadcast
        unsigned long long best = 0;
#pragma unroll
        for (int u = 0; u < PPT; ++u) {
            const int i = u * FW + tid;
            if (i < n) {
                const float d = dist_exact(x[i], y[i], z[i], cx, cy, cz);
                md[u] = md[u] > d ? d : md[u];
                const unsigned long long key = fps_key(md[u], i);
                best = key > best ? key : best;
            }
        }
        const unsigned long long g = block_max_u64<FWAVES>(best, wkey, it);
        cur = (int)(0xffffffffu - (unsigned)(g & 0xffffffffull));
        if (tid == 0) { sidx[k] = cur; sx[k] = x[cur]; sy[k] = y[cur]; sz[k] = z[cur]; }
    }
    __syncthreads();
    // ---- stage 2 on the n1 selected points
    const float radius = a.fps_radius[b];
    cur = min(max(a.rad_start[b], 0), n1 - 1);
    const int count = fps_stage2<FW, FPS_PPT2>(sx, sy, sz, sidx, n1, radius, cur, out, wkey, it);
    for (int t = count + tid; t < a.max_nobj; t += FW) out[t] = -1;
    if (tid == 0) a.n_obj[b] = count;
}

template <int PPT>
static hipError_t launch_fps(const FpsDev& a, int B, size_t lds, hipStream_t st) {
    if (lds > 64 * 1024) {               // above 64 KB of dynamic LDS: a per-device opt-in of the function
        static std::atomic<unsigned long long> done{0};
        if (hipError_t e = lds_opt_in(done, 160 * 1024 - 256, k_fps_batch<PPT>); e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(k_fps_batch<PPT>, dim3(B), dim3(FW), lds, st, a);
    return hipGetLastError();
}

hipError_t launch_fps_batch(const FpsArgs& h, hipStream_t st) {
    FpsDev a;
    a.pos = h.pos; a.pt_off = h.pt_off; a.npts = h.npts; a.stride = h.stride;
    a.fps_start = h.fps_start; a.fps_radius = h.fps_radius; a.rad_start = h.rad_start;
    a.max_nobj = h.max_nobj; a.max_pts = h.max_pts; a.fps_idx = h.fps_idx; a.n_obj = h.n_obj;
    const int ppt = h.max_pts <= 4 * FW ? 4 : h.max_pts <= 16 * FW ? 16 : FPS_PPT_MAX;
    a.pad = ppt * FW;
    const size_t lds = fps_lds_bytes(a.pad, a.max_nobj);   // at most 64 + 96 KB + 16 KB
    if (ppt == 4) return launch_fps<4>(a, h.B, lds, st);
    if (ppt == 16) return launch_fps<16>(a, h.B, lds, st);
    return launch_fps<FPS_PPT_MAX>(a, h.B, lds, st);
}

// ---------------------------------------------------------------------------------------------- clouds beyond LDS
// k_fps_cloud: the same two stages on clouds of up to 2^20 points (perception.py:259-315, the merged tabletop cloud), one
// workgroup per cloud, the cloud read from global memory on every sweep.  Arithmetic, argmax order and outputs are k_fps_batch's.
//   Workgroup: CW = 1024 threads, the largest there is.  One workgroup is all that works on a cloud (the argmax of every selected
//   point is a rendezvous of everything that sweeps), so its 16 wavefronts - four per SIMD - are what hides the latency of the
//   loads; that leaves 128 VGPRs per thread.
//   Points: thread t owns the points u * CW + t, ascending in u, so "strictly greater" inside a thread keeps its lowest index and
//   one packed key per thread goes into the reduction.  (The minima are never negative or NaN - a NaN distance loses "md > d" - so
//   their bit patterns order as signed integers, -1 standing for "no point".)
//   Coordinates: read as they lie, AoS, one 12-byte load per point.  A wavefront's load then covers 768 contiguous bytes and uses
//   every byte of every line it fetches, like three SoA loads of 256 bytes would, with one instruction in place of three - a one-
//   time SoA copy would buy nothing and cost 12 bytes of workspace per point.  (Reading x, y and z with three dword loads at a
//   12-byte stride is what to avoid: each of them would touch all six lines.)
//   Minima: those of the first CLOUD_S = CW * CLOUD_PPT points stay in registers (CLOUD_PPT per thread, in groups of CLOUD_GRP that
//   a wave skips as a whole once past the cloud's end); those of the points behind live in the call's workspace, max_pts - CLOUD_S
//   floats per cloud, read and written by their owner thread only (no barrier needed for them).  A cloud takes the workspace part
//   of the sweep iff it has more than CLOUD_S points, whatever else is in the launch.
// Bounded by: stage 1 makes min(max_nobj, n) - 1 sweeps of n points, stage 2 at most min(max_nobj, n) of as many points; every
// load index is clamped below n.  No atomics, no flag, nothing waits for another workgroup.
constexpr int CW = 1024;
constexpr int CLOUD_PPT = 32;
constexpr int CLOUD_GRP = 8;
constexpr int CLOUD_S = CW * CLOUD_PPT;               // 32768 points with their minima in registers
constexpr int CLOUD_MAX_POINTS = 1 << 20;
static_assert(CW >= FPS_MAX_NOBJ && CLOUD_PPT % CLOUD_GRP == 0, "stage 2 keeps one point per thread");

size_t fps_cloud_max_points() { return CLOUD_MAX_POINTS; }
size_t fps_cloud_switch_points() { return CLOUD_S; }
size_t fps_cloud_ws_floats(int B, int max_pts) { return max_pts > CLOUD_S ? (size_t)B * (size_t)(max_pts - CLOUD_S) : 0; }

struct __attribute__((packed, aligned(4))) P3 { float x, y, z; };

// one point of a sweep: its minimum against the centre, and the thread's running (bits, index) argmax
__device__ __forceinline__ float cloud_visit(const P3* p, int i, int n, float md, float cx, float cy, float cz, int& bestb, int& besti) {
    const P3 q = p[i < n ? i : n - 1];                 // branch-free: a point past the end reads the last one and is not counted
    const float d = dist_exact(q.x, q.y, q.z, cx, cy, cz);
    md = md > d ? d : md;
    const int mb = i < n ? (int)__float_as_uint(md) : -1;
    if (mb > bestb) { bestb = mb; besti = i; }
    return md;
}

__global__ __launch_bounds__(CW) void k_fps_cloud(FpsDev a, float* ws) {
    __shared__ unsigned long long wkey[2 * (CW / 64)];
    __shared__ float sx[FPS_MAX_NOBJ], sy[FPS_MAX_NOBJ], sz[FPS_MAX_NOBJ];           // stage-1 points in selection order
    __shared__ int sidx[FPS_MAX_NOBJ];
    const int b = blockIdx.x, tid = threadIdx.x;
    int* out = a.fps_idx + (long)b * a.max_nobj;
    const long long nraw = a.npts[(long)b * a.stride];
    const int n = (int)(nraw < 0 ? 0 : nraw > (long long)a.max_pts ? (long long)a.max_pts : nraw);   // keeps ws inside its stride
    if (n == 0) {
        for (int t = tid; t < a.max_nobj; t += CW) out[t] = -1;
        if (tid == 0) a.n_obj[b] = 0;
        return;
    }
    const P3* p = reinterpret_cast<const P3*>(a.pos + a.pt_off[(long)b * a.stride] * 3);
    float* wmd = ws + (long)b * (long)max(a.max_pts - CLOUD_S, 0);                    // minimum of point i >= CLOUD_S: wmd[i - CLOUD_S]
    for (int i = CLOUD_S + tid; i < n; i += CW) wmd[i - CLOUD_S] = 1e10f;
    int it = 0;
    // ---- stage 1
    const int n1 = min(a.max_nobj, n);
    float md[CLOUD_PPT];
#pragma unroll
    for (int u = 0; u < CLOUD_PPT; ++u) md[u] = 1e10f;
    int cur = min(max(a.fps_start[b], 0), n - 1);
    for (int k = 0;; ++k) {
        const P3 c = p[cur];                                                         // same address in every lane
        if (tid == 0) { sidx[k] = cur; sx[k] = c.x; sy[k] = c.y; sz[k] = c.z; }
        if (k + 1 >= n1) break;
        int bestb = -1, besti = 0;
#pragma unroll
        for (int g = 0; g < CLOUD_PPT; g += CLOUD_GRP) {
            if (g * CW < n) {                                                        // uniform over the workgroup
#pragma unroll
                for (int u = g; u < g + CLOUD_GRP; ++u) md[u] = cloud_visit(p, u * CW + tid, n, md[u], c.x, c.y, c.z, bestb, besti);
            }
        }
        for (int base = CLOUD_S; base < n; base += 4 * CW) {                         // uniform trip count
            float m[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) { const int i = base + u * CW + tid; m[u] = i < n ? wmd[i - CLOUD_S] : 1e10f; }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int i = base + u * CW + tid;
                m[u] = cloud_visit(p, i, n, m[u], c.x, c.y, c.z, bestb, besti);
                if (i < n) wmd[i - CLOUD_S] = m[u];
            }
        }
        const unsigned long long key = bestb < 0 ? 0ull : fps_key(__uint_as_float((unsigned)bestb), besti);
        const unsigned long long gk = block_max_u64<CW / 64>(key, wkey, it);
        cur = (int)(0xffffffffu - (unsigned)(gk & 0xffffffffull));
    }
    __syncthreads();
    // ---- stage 2 on the n1 selected points
    const float radius = a.fps_radius[b];
    cur = min(max(a.rad_start[b], 0), n1 - 1);
    const int count = fps_stage2<CW, FPS_MAX_NOBJ / CW>(sx, sy, sz, sidx, n1, radius, cur, out, wkey, it);
    for (int t = count + tid; t < a.max_nobj; t += CW) out[t] = -1;
    if (tid == 0) a.n_obj[b] = count;
}

hipError_t launch_fps_cloud(const FpsArgs& h, float* ws, hipStream_t st) {
    FpsDev a;
    a.pos = h.pos; a.pt_off = h.pt_off; a.npts = h.npts; a.stride = h.stride;
    a.fps_start = h.fps_start; a.fps_radius = h.fps_radius; a.rad_start = h.rad_start;
    a.max_nobj = h.max_nobj; a.max_pts = h.max_pts; a.pad = 0; a.fps_idx = h.fps_idx; a.n_obj = h.n_obj;
    hipLaunchKernelGGL(k_fps_cloud, dim3(h.B), dim3(CW), 0, st, a, ws);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------- assembly
// One workgroup per sample, one thread per particle row: the row's history, action, futures, attributes and masks.
// Augmentation (dataset.py:274-285): the noise is added in double and rounded once (numpy's float32 += float64), then the
// row vector is multiplied by the fp32 rotation matrix of the angle - x' = x*c + y*s, y' = x*(-s) + y*c, z' = z - as
// separate fp32 products and one sum (the reference's matmul may contract them: tests allow for that on rotated fixtures).
struct AsmRot { float c, s; bool on; };
__device__ __forceinline__ void rot_store(float* dst, float vx, float vy, float vz, const AsmRot& r) {
    if (r.on) {
        const float nx = __fadd_rn(__fmul_rn(vx, r.c), __fmul_rn(vy, r.s));
        const float ny = __fadd_rn(__fmul_rn(vx, -r.s), __fmul_rn(vy, r.c));
        vx = nx; vy = ny;
    }
    dst[0] = vx; dst[1] = vy; dst[2] = vz;
}

__global__ __launch_bounds__(FW) void k_dataset_assemble(ag_dataset_batch a) {
    const int b = blockIdx.x, tid = threadIdx.x;
    const int nh = a.n_his, nf = a.n_future, No = a.max_nobj, Ne = a.n_eef, N = No + Ne;
    const int64_t* m = a.d_sample + (long)b * (5 + nh + nf);
    const long long n_e = m[1], obj_off = m[2], eef_off = m[3], ep = m[4];
    const int64_t* fr = m + 5;
    const int n_obj = min(max(a.d_n_obj[b], 0), No);
    AsmRot r{1.f, 0.f, a.d_rot != nullptr};
    if (r.on) { const double ang = a.d_rot[b]; r.c = (float)cos(ang); r.s = (float)sin(ang); }
    for (int i = tid; i < N; i += FW) {
        const bool is_obj = i < No, live = i < n_obj, is_eef = !is_obj;
        long long src = 0;
        if (live) { src = a.d_fps_idx[(long)b * No + i]; src = src < 0 ? 0 : src >= n_e ? n_e - 1 : src; }
        // position of this row in pair frame t (zero for the padding rows)
        auto at = [&](int t, float& vx, float& vy, float& vz) {
            vx = vy = vz = 0.f;
            const float* p = nullptr;
            if (live) p = a.d_obj_pos + (obj_off + fr[t] * n_e + src) * 3;
            else if (is_eef) p = a.d_eef_pos + (eef_off + fr[t] * Ne + (i - No)) * 3;
            if (p) { vx = p[0]; vy = p[1]; vz = p[2]; }
        };
        for (int t = 0; t < nh; ++t) {                                               // dataset.py:192-202
            float vx, vy, vz;
            at(t, vx, vy, vz);
            const long o = (((long)b * nh + t) * N + i) * 3;
            if (a.d_state_noise) {                                                   // :275, padding and tool rows included
                vx = (float)((double)vx + a.d_state_noise[o]);
                vy = (float)((double)vy + a.d_state_noise[o + 1]);
                vz = (float)((double)vz + a.d_state_noise[o + 2]);
            }
            rot_store(a.d_state + o, vx, vy, vz, r);
        }
        {                                                                            // :176-179
            float ax = 0.f, ay = 0.f, az = 0.f;
            if (is_eef) {
                float x0, y0, z0, x1, y1, z1;
                at(nh - 1, x0, y0, z0); at(nh, x1, y1, z1);
                ax = __fsub_rn(x1, x0); ay = __fsub_rn(y1, y0); az = __fsub_rn(z1, z0);
            }
            rot_store(a.d_action + ((long)b * N + i) * 3, ax, ay, az, r);
        }
        for (int f = 0; f < nf - 1; ++f) {                                           // :220-225
            float x0 = 0.f, y0 = 0.f, z0 = 0.f, x1 = 0.f, y1 = 0.f, z1 = 0.f;
            if (is_eef) { at(nh + f, x0, y0, z0); at(nh + f + 1, x1, y1, z1); }
            const long o = (((long)b * (nf - 1) + f) * N + i) * 3;
            rot_store(a.d_eef_future + o, x0, y0, z0, r);
            rot_store(a.d_action_future + o, __fsub_rn(x1, x0), __fsub_rn(y1, y0), __fsub_rn(z1, z0), r);
        }
        a.d_attrs[((long)b * N + i) * 2] = live ? 1.f : 0.f;                         // :249-251
        a.d_attrs[((long)b * N + i) * 2 + 1] = is_eef ? 1.f : 0.f;
        a.d_state_mask[(long)b * N + i] = (live || is_eef) ? 1 : 0;                  // :234-239
        a.d_eef_mask[(long)b * N + i] = is_eef ? 1 : 0;
        if (is_obj) {
            for (int f = 0; f < nf; ++f) {                                           // :213-216
                float vx, vy, vz;
                at(nh + f, vx, vy, vz);
                rot_store(a.d_state_future + (((long)b * nf + f) * No + i) * 3, vx, vy, vz, r);
            }
            a.d_p_instance[(long)b * No + i] = live ? 1.f : 0.f;                     // :257-258
            a.d_obj_mask[(long)b * No + i] = live ? 1 : 0;                           // :241-242
            for (int k = 0; k < a.n_mat; ++k)                                        // :269-271
                a.d_material_index[((long)b * No + i) * a.n_mat + k] = (live && k == a.mat_col) ? 1 : 0;
        }
    }
    // physics parameter: the stored value plus the noise, in double, rounded once (:265-266 on a copy, :299)
    for (int k = tid; k < a.phys_dim; k += FW)
        a.d_physics_param[(long)b * a.phys_dim + k] =
            (float)(a.d_phys[ep * a.phys_dim + k] + (a.d_phys_noise ? a.d_phys_noise[(long)b * a.phys_dim + k] : 0.0));
    // squared edge threshold of the single-graph builder (graph.py:86,101) and a culling radius whose square covers it
    if (tid == 0 && a.d_adj_thresh) {
        const double adj = a.d_adj_thresh[b];
        a.d_thr2[b] = (float)(adj * adj);
        a.d_cull[b] = nextafterf((float)fabs(adj), __builtin_huge_valf());
    }
}

hipError_t launch_dataset_assemble(const ag_dataset_batch& a, hipStream_t st) {
    hipLaunchKernelGGL(k_dataset_assemble, dim3(a.B), dim3(FW), 0, st, a);
    return hipGetLastError();
}

}  // namespace ag
