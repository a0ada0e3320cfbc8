// Device-resident training step (ag_ctx_load_weights_device, ag_adam_step, ag_train_step, ag_train_step_part): what lives between the model
// forwards and the backward chunks of ag_train.hip, gfx950 only.
//   * the weight images of the forward chains from the 22 plain fp32 tensors.  ONE table (kPackBlocks) lists the 14 packed blocks
//     of the 11 layers; every image element is one call of an element function (pack_elem_*) that the host packer
//     (pack_weights_host: ag_ctx_load_weights) and the device packer (k_pack_weights*) share, so the two cannot drift apart
//   * Adam in torch.optim.Adam's single-tensor operation order, one launch over the 22 tensors (k_adam)
//   * the glue of the reference's loop body (src/dynamics/train/train.py:86-124): MSE in fp64 in a fixed order, the next state
//     and action, the MSE gradient plus what the later steps say about a prediction, the shift of dLoss/dstate through the history
// No float atomics: two calls on the same inputs give the same bits.
#include "ag_model.h"
#include "ag_train.h"
#include <cstdint>
#include <cstring>

namespace ag {
size_t lat_weights_offset(int which);

namespace {

// kind: 0 hidden layer (152 input slots, bias in slot ONE_F), 1 first layer of an encoder (inputs then the bias), 2 the 3-output head
// in: -1 = the model's rel_dim (5 + 3 n_his); chunks: k-chunks of a first layer in the fp32 / latency image
// pair (kind 0, fp32 image only): the block's readers are half-step chains (ag_mlp.hip, mma_act), which issue the two-block MFMA on
// tile pairs (0,1) and (2,3): m-blocks 2m and 2m+1 then hold the A operands of that form (pack_elem_f32).  It follows the build
// switches of the chains: with half-steps compiled out of a chain its blocks are packed plain and its code is the one before them.
struct PackBlock { int w, b, ld, col0, out, in, kind, off, b3_phase, lat, chunks, lat_chunks, pair; };
using WL = WeightLayout;
constexpr int kNumBlocks = 14;
constexpr PackBlock kPackBlocks[kNumBlocks] = {
    // tensor, bias, ld, col0, out, in, kind, fp32 offset, bf16x3 phase (WLB in ag_mlp.hip), latency slot (ag_lat.hip), chunks, pair
    {0, 1, IN_DIM, 0, NF, IN_DIM, 1, WL::N_L1, 16, 10, NODE_L1_CHUNKS, 1, 0},   // particle encoder
    {2, 3, NF, 0, NF, NF, 0, WL::N_L2, 17, 11, 0, 0, 0},
    {4, 5, NF, 0, NF, NF, 0, WL::N_L3, 22, 12, 0, 0, 0},
    {6, 7, -1, 0, NF, -1, 1, WL::E_L1, 0, 0, EDGE_L1_CHUNKS, 2, 0},             // relation encoder
    {8, 9, NF, 0, NF, NF, 0, WL::E_L2, 1, 1, 0, 0, HS_EDGE},
    {10, 11, NF, 0, NF, NF, 0, WL::E_L3, 6, 2, 0, 0, HS_EDGE},
    {12, 13, 2 * NF, 0, NF, NF, 0, WL::N_WA, 27, 13, 0, 0, 0},                  // particle propagator W_pp = [Wa | Wb], bias with Wa
    {12, -1, 2 * NF, NF, NF, NF, 0, WL::P_WB, 42, 4, 0, 0, HS_NODE},
    {14, 15, 3 * NF, 0, NF, NF, 0, WL::E_W1, 11, 3, 0, 0, HS_EDGE},             // relation propagator W_rp = [W1 | W2 | W3], bias with W1
    {14, -1, 3 * NF, NF, NF, NF, 0, WL::N_W2, 32, 5, 0, 0, HS_NODE},
    {14, -1, 3 * NF, 2 * NF, NF, NF, 0, WL::N_W3, 37, 6, 0, 0, HS_NODE},
    {16, 17, NF, 0, NF, NF, 0, WL::P_P0, 47, 7, 0, 0, HS_NODE},                 // predictor
    {18, 19, NF, 0, NF, NF, 0, WL::P_P1, 52, 8, 0, 0, HS_NODE},
    {20, 21, NF, 0, 3, NF, 2, WL::P_P2, 57, 9, 0, 0, 0},
};

struct PackSrc { const float* W; const float* bias; int ld, col0, out, in, kind, pair; };

__host__ __device__ inline float pack_src_at(const PackSrc& s, int m, int k) {   // hidden layer / head: weight, bias in slot ONE_F, zero padding
    if (m < 0 || m >= s.out || k < 0) return 0.f;
    if (k < s.in) return s.W[(size_t)m * s.ld + s.col0 + k];
    return (k == ONE_F && s.bias) ? s.bias[m] : 0.f;
}
__host__ __device__ inline float pack_first_at(const PackSrc& s, int m, int k) {  // first layer: inputs, then the bias
    if (m < 0 || m >= NF) return 0.f;
    if (k < s.in) return s.W[(size_t)m * s.in + k];
    return k == s.in ? s.bias[m] : 0.f;
}

// ---- MFMA A-operand image of v_mfma_f32_32x32x2_f32: [chunk q][m-block][lane][4 steps]; lane l supplies out-feature
// 32*mb + (l&31) for input slot k(s, l>>5).  See ag_mlp.hip header.
// Paired block (PackBlock::pair): m-blocks 2m + i, m in {0, 1}, are the A operands of v_mfma_f32_32x32x1_2b_f32 instead - lane l
// supplies out-feature 32*(2m + (l>>5)) + (l&31), tile 2m on lanes 0-31 and tile 2m+1 on lanes 32-63, for the ONE input slot
// k(s, i): i = 0 the feature the step carries on lanes 0-31, i = 1 the one on lanes 32-63.  M-block 4 is as in a plain block.
__host__ __device__ inline int slot_of(int s, int h) {
    const int t = s < 64 ? s / 16 : 4, r = s < 64 ? s % 16 : s - 64;
    return 32 * t + (r & 3) + 8 * (r >> 2) + 4 * h;
}
__host__ __device__ inline int f32_elems(const PackBlock& b) { return (b.kind == 1 ? b.chunks * 5 : b.kind == 2 ? KCH : KCH * 5) * 256; }
// element (chunk q, m-block mb, lane, step e) of the image; KIND is the block's kind, so a host loop is compiled per kind
template <int KIND>
__host__ __device__ inline float pack_elem_f32(const PackSrc& s, int q, int mb, int lane, int e) {
    const int m = 32 * mb + (lane & 31);
    if (KIND == 1) return pack_first_at(s, m, 2 * (4 * q + e) + (lane >> 5));
    if (KIND == 0 && s.pair && mb < 4) return pack_src_at(s, 32 * ((mb & ~1) + (lane >> 5)) + (lane & 31), slot_of(4 * q + e, mb & 1));
    return pack_src_at(s, m, slot_of(4 * q + e, lane >> 5));
}

// ---- latency-mode chains (ag_lat.hip): A-operand image of v_mfma_f32_16x16x4_f32, [chunk of 4 k-steps][tile][lane][4].
// Register r of tile T in lane group g stands for feature 16T + 8(r>>1) + 4(g&1) + 2(r&1) + (g>>1): the k sequence of the
// 32-row chains (slot_of) cut into steps of four, so that both kernel families round identically.  >= 152: dead slot.
__host__ __device__ inline int feat_lat(int T, int g, int r) {
    const int f = 16 * T + 8 * (r >> 1) + 4 * (g & 1) + 2 * (r & 1) + (g >> 1);
    return f < 152 ? f : -1;
}
__host__ __device__ inline int lat_elems(const PackBlock& b) { return (b.kind == 1 ? b.lat_chunks * 10 : b.kind == 2 ? 10 : 100) * 256; }
// element (chunk c of 4 k-steps, tile mt, lane, step e)
template <int KIND>
__host__ __device__ inline float pack_elem_lat(const PackSrc& s, int c, int mt, int lane, int e) {
    const int i = lane & 15;
    if (KIND == 1) return pack_first_at(s, feat_lat(mt, i >> 2, i & 3), 4 * (4 * c + e) + (lane >> 4));
    const int st = 4 * c + e;
    if (st >= 38) return 0.f;
    const int T = st < 36 ? st / 4 : 9, r = st < 36 ? st % 4 : st - 36;
    // D row 4g + r of an output tile = A row i: the head keeps its 3 outputs in rows 0..2
    return pack_src_at(s, KIND == 2 ? i : feat_lat(mt, i >> 2, i & 3), feat_lat(T, lane >> 4, r));
}

// ---- bf16x3 weight image (see ag_mlp.hip): every weight is split exactly into three bf16 pieces.  Element idx names
// (k-step, m-block, lane, j); its three parts sit 64 * 8 uint16 apart
__host__ __device__ inline uint32_t f2u(float f) {
#ifdef __HIP_DEVICE_COMPILE__
    return __float_as_uint(f);
#else
    uint32_t u; memcpy(&u, &f, 4); return u;
#endif
}
__host__ __device__ inline float u2f(uint32_t u) {
#ifdef __HIP_DEVICE_COMPILE__
    return __uint_as_float(u);
#else
    float f; memcpy(&f, &u, 4); return f;
#endif
}
__host__ __device__ inline uint16_t bf16_rn(float f) {
    uint32_t u = f2u(f);
    u += 0x7FFFu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
}
__host__ __device__ inline float bf16_f(uint16_t h) { return u2f((uint32_t)h << 16); }
__host__ __device__ inline int b3_elems(const PackBlock& b) { return (b.kind == 1 ? 2 * 5 : b.kind == 2 ? 10 : 50) * 512; }
// element (k-step ks, m-block mb, lane, j): its three parts sit 64 * 8 uint16 apart
template <int KIND>
__host__ __device__ inline void pack_elem_b3(const PackSrc& s, int ks, int mb, int lane, int j, uint16_t* dst) {
    constexpr int MB = KIND == 2 ? 1 : 5;
    const int m = 32 * mb + (lane & 31), h = lane >> 5;
    float v;
    if (KIND == 1) v = pack_first_at(s, m, 16 * ks + 8 * h + j);
    else v = pack_src_at(s, m, 32 * (ks >> 1) + 16 * (ks & 1) + (j & 3) + 8 * (j >> 2) + 4 * h);   // k-step ks = 2*tile + u
    uint16_t p[3];
    p[0] = bf16_rn(v);
    const float r = v - bf16_f(p[0]);
    p[1] = bf16_rn(r);
    const float q = r - bf16_f(p[1]);
    p[2] = bf16_rn(q);
    for (int part = 0; part < 3; ++part) dst[((((size_t)ks * MB + mb) * 3 + part) * 64 + lane) * 8 + j] = p[part];
}

__host__ __device__ inline PackSrc pack_src(const PackBlock& b, const float* const* t, int rel_dim) {
    PackSrc s;
    s.W = t[b.w]; s.bias = b.b >= 0 ? t[b.b] : nullptr;
    s.ld = b.ld < 0 ? rel_dim : b.ld; s.in = b.in < 0 ? rel_dim : b.in;
    s.col0 = b.col0; s.out = b.out; s.kind = b.kind; s.pair = b.pair;
    return s;
}

struct PackDev {
    PackBlock blk[kNumBlocks];
    const float* t[22];
    unsigned lat_off[kNumBlocks];
    int rel_dim;
    float* blob; uint16_t* b3; float* lat;
};
// one thread per image element: the flat index is decoded here, the element functions are the host packer's
template <int KIND>
__device__ inline void pack_thread(const PackDev& p, const PackBlock& b, int img, int i) {
    const PackSrc s = pack_src(b, p.t, p.rel_dim);
    if (img == 0) {
        constexpr int MB = KIND == 2 ? 1 : 5;
        p.blob[b.off + i] = pack_elem_f32<KIND>(s, (i >> 8) / MB, (i >> 8) % MB, (i >> 2) & 63, i & 3);
    } else if (img == 1) {
        constexpr int NT = KIND == 2 ? 1 : 10;
        p.lat[p.lat_off[blockIdx.y] + i] = pack_elem_lat<KIND>(s, (i >> 8) / NT, (i >> 8) % NT, (i >> 2) & 63, i & 3);
    } else {
        constexpr int MB = KIND == 2 ? 1 : 5;
        pack_elem_b3<KIND>(s, (i >> 9) / MB, (i >> 9) % MB, (i >> 3) & 63, i & 7, p.b3 + (size_t)b.b3_phase * (B3_PHASE_BYTES / 2));
    }
}
// img: 0 fp32 MFMA image, 1 latency image, 2 bf16x3 image
__global__ void k_pack_weights(PackDev p, int img) {
    const PackBlock b = p.blk[blockIdx.y];
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (img == 0 ? f32_elems(b) : img == 1 ? lat_elems(b) : b3_elems(b))) return;
    if (b.kind == 0) pack_thread<0>(p, b, img, i);
    else if (b.kind == 1) pack_thread<1>(p, b, img, i);
    else pack_thread<2>(p, b, img, i);
}

// host: nested loops in image order, compiled per kind (no index decoding, no kind test per element)
template <int KIND>
void pack_block_host(const PackBlock& b, const PackSrc& s, float* blob, uint16_t* b3, float* lat) {
    constexpr int MB = KIND == 2 ? 1 : 5, NT = KIND == 2 ? 1 : 10;
    const int nq = f32_elems(b) / (MB * 256), nc = lat_elems(b) / (NT * 256), nks = b3_elems(b) / (MB * 512);
    float* o = blob + b.off;
    for (int q = 0; q < nq; ++q)
        for (int mb = 0; mb < MB; ++mb)
            for (int lane = 0; lane < 64; ++lane)
                for (int e = 0; e < 4; ++e) *o++ = pack_elem_f32<KIND>(s, q, mb, lane, e);
    if (b3) {
        uint16_t* d = b3 + (size_t)b.b3_phase * (B3_PHASE_BYTES / 2);
        for (int ks = 0; ks < nks; ++ks)
            for (int mb = 0; mb < MB; ++mb)
                for (int lane = 0; lane < 64; ++lane)
                    for (int j = 0; j < 8; ++j) pack_elem_b3<KIND>(s, ks, mb, lane, j, d);
    }
    if (lat) {
        float* L = lat + lat_weights_offset(b.lat);
        for (int c = 0; c < nc; ++c)
            for (int mt = 0; mt < NT; ++mt)
                for (int lane = 0; lane < 64; ++lane)
                    for (int e = 0; e < 4; ++e) *L++ = pack_elem_lat<KIND>(s, c, mt, lane, e);
    }
}

}  // namespace

void pack_weights_host(int rel_dim, const float* const* t, float* blob, uint16_t* b3, float* lat) {
    for (const PackBlock& b : kPackBlocks) {
        const PackSrc s = pack_src(b, t, rel_dim);
        if (b.kind == 0) pack_block_host<0>(b, s, blob, b3, lat);
        else if (b.kind == 1) pack_block_host<1>(b, s, blob, b3, lat);
        else pack_block_host<2>(b, s, blob, b3, lat);
    }
}

hipError_t launch_pack_weights(int rel_dim, const float* const* d_t, float* d_blob, uint16_t* d_b3, float* d_lat, hipStream_t st) {
    PackDev p{};
    int nf = 0, nl = 0, nb = 0;
    for (int i = 0; i < kNumBlocks; ++i) {
        p.blk[i] = kPackBlocks[i];
        p.lat_off[i] = (unsigned)lat_weights_offset(kPackBlocks[i].lat);
        nf = nf > f32_elems(p.blk[i]) ? nf : f32_elems(p.blk[i]);
        nl = nl > lat_elems(p.blk[i]) ? nl : lat_elems(p.blk[i]);
        nb = nb > b3_elems(p.blk[i]) ? nb : b3_elems(p.blk[i]);
    }
    for (int i = 0; i < 22; ++i) p.t[i] = d_t[i];
    p.rel_dim = rel_dim; p.blob = d_blob; p.b3 = d_b3; p.lat = d_lat;
    hipLaunchKernelGGL(k_pack_weights, dim3((nf + 255) / 256, kNumBlocks), dim3(256), 0, st, p, 0);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess && d_lat) {
        hipLaunchKernelGGL(k_pack_weights, dim3((nl + 255) / 256, kNumBlocks), dim3(256), 0, st, p, 1);
        e = hipGetLastError();
    }
    if (e == hipSuccess && d_b3) {
        hipLaunchKernelGGL(k_pack_weights, dim3((nb + 255) / 256, kNumBlocks), dim3(256), 0, st, p, 2);
        e = hipGetLastError();
    }
    return e;
}

void weight_tensor_sizes(int rel_dim, int* n22) {
    const int in[11] = {IN_DIM, NF, NF, rel_dim, NF, NF, 2 * NF, 3 * NF, NF, NF, NF};
    for (int l = 0; l < 11; ++l) { const int out = l == 10 ? 3 : NF; n22[2 * l] = out * in[l]; n22[2 * l + 1] = out; }
}

// ------------------------------------------------------------------------------------------------------------------ Adam
namespace {
// torch.optim.Adam, single-tensor formula (no amsgrad, no maximize): g += wd * w; m = m + (g - m) * (1 - beta1);
// v = v * beta2 + (1 - beta2) * g * g; denom = sqrt(v) / sqrt(bc2) + eps; w += -(lr / bc1) * (m / denom).
// status[0] != 0 (a graph overflowed in this or an earlier unchecked step): nothing is touched; else status[1] counts the step.
__global__ void k_adam(AdamArgs a) {
    if (a.status[0] != 0) return;
    const int k = blockIdx.y, i = blockIdx.x * blockDim.x + threadIdx.x;
    if (k == 0 && i == 0) a.status[1] += 1;
    if (i >= a.n[k]) return;
    float g = a.g[k][i];
    const float w = a.w[k][i];
    if (a.wd != 0.f) g = g + a.wd * w;
    const float m0 = a.m[k][i];
    const float m = m0 + a.one_minus_b1 * (g - m0);
    const float v = a.v[k][i] * a.b2 + (a.one_minus_b2 * g) * g;
    const float denom = sqrtf(v) / a.bc2_sqrt + a.eps;
    a.m[k][i] = m; a.v[k][i] = v;
    a.w[k][i] = w + a.neg_step_size * (m / denom);
}
}  // namespace

// Grid: 22 x the blocks of the largest tensor (150 x 450), so the workgroups of the small tensors exit at once (~5,800 launched,
// ~1,000 with work; 5 us per launch measured).  A flat index over a prefix sum of the sizes would launch a sixth of them.
hipError_t launch_adam(const AdamArgs& a, hipStream_t st) {
    int nmax = 0;
    for (int k = 0; k < 22; ++k) nmax = nmax > a.n[k] ? nmax : a.n[k];
    hipLaunchKernelGGL(k_adam, dim3((nmax + 255) / 256, 22), dim3(256), 0, st, a);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------- glue of the chained step
namespace {
constexpr int kLossBlocks = 64;

// squared error of pred (B,n_p,3) against state_future[:, fi] ((B,n_future,n_p,3)): per-block fp64 partial sums in a fixed tree
__global__ __launch_bounds__(256) void k_mse_part(const float* pred, const float* fut, int B, int n_p, int n_future, int fi, double* part) {
    __shared__ double sh[256];
    const long n = (long)B * n_p * 3, row = (long)n_p * 3;
    double s = 0.0;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += 256L * kLossBlocks) {
        const long b = i / row, r = i % row;
        const float d = pred[i] - fut[(b * n_future + fi) * row + r];
        s += (double)d * (double)d;
    }
    sh[threadIdx.x] = s;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (threadIdx.x < w) sh[threadIdx.x] += sh[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) part[blockIdx.x] = sh[0];
}
// loss[fi] = sum / n (n = the elements of the whole step: this call's share of the mean), rounded once; accumulate: the earlier
// parts' loss[fi] joins in fp64 before that rounding.  After the last step loss[n_future] = the fp32 sum of the steps in step
// order (train.py:103)
__global__ void k_mse_final(const double* part, long n, int fi, int n_future, int accumulate, float* loss) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    double s = 0.0;
    for (int k = 0; k < kLossBlocks; ++k) s += part[k];
    s = s / (double)n;
    if (accumulate) s += (double)loss[fi];
    loss[fi] = (float)s;
    if (fi == n_future - 1) {
        float t = 0.f;
        for (int k = 0; k < n_future; ++k) t += loss[k];
        loss[n_future] = t;
    }
}

// next model input (train.py:104-119): the last frame is eef_future[:, fi] with the object rows replaced by the prediction,
// the frames before it the old history shifted by one (frame 0 stays and frame 1 leaves when rest: store_rest_state);
// next action = action_future[:, fi]
__global__ void k_next_state(const float* state, const float* pred, const float* eef, const float* act_f, int B, int N, int n_p,
                             int n_his, int nf1, int fi, int rest, float* state_next, float* action_next) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long)B * N * 3) return;
    const long r = i / 3; const int c = (int)(i % 3);
    const int b = (int)(r / N), n = (int)(r % N);
    const float* s = state + (long)b * n_his * N * 3;
    float* o = state_next + (long)b * n_his * N * 3;
    const long e = ((long)n * 3) + c;
    for (int t = 0; t < n_his - 1; ++t) o[(long)t * N * 3 + e] = s[(long)((rest && t == 0) ? 0 : t + 1) * N * 3 + e];
    const long f = (((long)b * nf1 + fi) * N + n) * 3 + c;
    o[(long)(n_his - 1) * N * 3 + e] = n < n_p ? pred[((long)b * n_p + n) * 3 + c] : eef[f];
    action_next[i] = act_f[f];
}

// dLoss/dpred of step fi: the MSE gradient (2 / n)(pred - gt), plus what step fi + 1's dstate says about the object rows of its
// last frame (dnext null: last step)
__global__ void k_pred_grad(const float* pred, const float* fut, const float* dnext, int B, int N, int n_p, int n_his, int n_future,
                            int fi, float scale, float* dpos) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long row = (long)n_p * 3;
    if (i >= (long)B * row) return;
    const long b = i / row, r = i % row;
    float v = scale * (pred[i] - fut[(b * n_future + fi) * row + r]);
    if (dnext) v += dnext[((b * n_his + (n_his - 1)) * N) * 3 + r];
    dpos[i] = v;
}

// total dLoss/dstate of step fi = its own (d, as the backward wrote it) + step fi + 1's total through the history shift
__global__ void k_dstate_carry(float* d, const float* dnext, int B, int N, int n_his, int rest) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long fr = (long)N * 3;
    if (i >= (long)B * n_his * fr) return;
    const int t = (int)((i / fr) % n_his);
    int src;                                   // frame of the next state that is this frame
    if (rest) src = t == 0 ? 0 : (t == 1 ? -1 : t - 1);
    else src = t - 1;
    if (src >= 0) d[i] += dnext[i + (long)(src - t) * fr];
}

inline unsigned blocks(long n) { return (unsigned)((n + 255) / 256); }
}  // namespace

size_t train_glue_doubles() { return kLossBlocks; }

hipError_t launch_mse_part(const float* pred, const float* fut, int B, int n_p, int n_future, int fi, double* part, hipStream_t st) {
    hipLaunchKernelGGL(k_mse_part, dim3(kLossBlocks), dim3(256), 0, st, pred, fut, B, n_p, n_future, fi, part);
    return hipGetLastError();
}
hipError_t launch_step_loss(const float* pred, const float* fut, int B, int n_p, int n_future, int fi, int B_total, int accumulate,
                            double* part, float* loss, hipStream_t st) {
    hipError_t e = launch_mse_part(pred, fut, B, n_p, n_future, fi, part, st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_mse_final, dim3(1), dim3(64), 0, st, part, (long)B_total * n_p * 3, fi, n_future, accumulate, loss);
    return hipGetLastError();
}
hipError_t launch_next_state(const float* state, const float* pred, const float* eef, const float* act_f, int B, int N, int n_p,
                             int n_his, int n_future, int fi, int rest, float* state_next, float* action_next, hipStream_t st) {
    hipLaunchKernelGGL(k_next_state, dim3(blocks((long)B * N * 3)), dim3(256), 0, st, state, pred, eef, act_f, B, N, n_p, n_his,
                       n_future - 1, fi, rest, state_next, action_next);
    return hipGetLastError();
}
hipError_t launch_pred_grad_scaled(const float* pred, const float* fut, const float* dnext, int B, int N, int n_p, int n_his,
                                   int n_future, int fi, float mse_scale, float* dpos, hipStream_t st) {
    hipLaunchKernelGGL(k_pred_grad, dim3(blocks((long)B * n_p * 3)), dim3(256), 0, st, pred, fut, dnext, B, N, n_p, n_his, n_future,
                       fi, mse_scale, dpos);
    return hipGetLastError();
}
hipError_t launch_pred_grad(const float* pred, const float* fut, const float* dnext, int B, int N, int n_p, int n_his, int n_future,
                            int fi, int B_total, float* dpos, hipStream_t st) {
    return launch_pred_grad_scaled(pred, fut, dnext, B, N, n_p, n_his, n_future, fi, (float)(2.0 / ((double)B_total * n_p * 3)), dpos, st);
}
hipError_t launch_dstate_carry(float* d, const float* dnext, int B, int N, int n_his, int rest, hipStream_t st) {
    hipLaunchKernelGGL(k_dstate_carry, dim3(blocks((long)B * n_his * N * 3)), dim3(256), 0, st, d, dnext, B, N, n_his, rest);
    return hipGetLastError();
}

}  // namespace ag
