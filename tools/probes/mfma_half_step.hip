// Stand-alone probe (not part of the library): what does a "half-step" of the exact-fp32 chains cost, and does it compute the same bits?
// A k-step of v_mfma_f32_32x32x2_f32 carries two features (k = lo on lanes 0-31, k = lo + 4 on lanes 32-63) into five 32 x 32 tiles:
// 5 MFMAs.  When one of the two features is zero in all 32 rows, tiles (0,1) and (2,3) can each take ONE v_mfma_f32_32x32x1_2b_f32
// (one k, two independent blocks; A = the live feature's weights of both tiles, made by one v_permlane32_swap of the two tiles'
// fragments; B = the live lane half, broadcast with blgp) and tile 4 the ordinary MFMA: 3 MFMAs + 2 swaps.  Register-only operands.
//   part 1  issue interval of the 2-block form against the 32x32x2 form, one and two wavefronts per SIMD
//   part 2  the half-step triple against the 5-MFMA step, one and two wavefronts per SIMD; and the FULL step in the same form (2 swaps,
//           2 x 2 two-block MFMAs in K order, 1 x 32x32x2), which is what the chains issue when both features are live: their tile pairs
//           then live in 32-register accumulators on every path
//           and both again as the chains issue them from a PAIRED weight image (ag_optim.hip, pack_elem_f32): the fragments come
//           already in the two-block form, so no swap, and the tile pairs stay in 32-register accumulators across iterations
//           (layer160 joins and splits them once per layer) instead of being re-joined per step
//   part 3  bits: the triple against the 5-MFMA step with the dead half zeroed, both sides, and the two-block full step against the
//           5-MFMA step on live data (this also pins the D register map of the 2-block form - block b = registers 16b .. 16b+15 -
//           the blgp lane-half broadcast, and that one 32x32x2 MFMA is the fmaf chain k = 0, then k = 1); the same three sides with
//           pre-paired fragments (made on the side, as the packer makes them)
//   hipcc --offload-arch=gfx950 -O3 tools/probes/mfma_half_step.hip -o mfma_half_step && ./mfma_half_step
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstring>
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x32 __attribute__((ext_vector_type(32)));

__device__ __forceinline__ void swap32(float& x, float& y) {   // lanes 32-63 of x <-> lanes 0-31 of y
    const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(y), false, false);
    x = __uint_as_float(r[0]); y = __uint_as_float(r[1]);
}
__device__ __forceinline__ f32x32 cat(f32x16 a, f32x16 b) {
    return __builtin_shufflevector(a, b, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22, 23, 24, 25, 26, 27,
                                   28, 29, 30, 31);
}
__device__ __forceinline__ f32x16 lo16(f32x32 c) { return __builtin_shufflevector(c, c, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15); }
__device__ __forceinline__ f32x16 hi16(f32x32 c) {
    return __builtin_shufflevector(c, c, 16, 17, 18, 19, 20, 21, 22, 23, 24, 25, 26, 27, 28, 29, 30, 31);
}

// the half-step: `side` 0 = only lanes 0-31 of b are live, 1 = only lanes 32-63; 2 = the full step in the same form
template <int SIDE>
__device__ __forceinline__ void half_step(float* a, float b, f32x16* acc) {
#pragma unroll
    for (int m = 0; m < 2; ++m) {
        float &w0 = a[2 * m], &w1 = a[2 * m + 1];              // in place: a step's fragments are used by that step only
        swap32(w0, w1);                                        // w0 = [W(2m, lo) | W(2m+1, lo)], w1 = [W(2m, lo+4) | W(2m+1, lo+4)]
        f32x32 c = cat(acc[2 * m], acc[2 * m + 1]);
        if (SIDE != 1) c = __builtin_amdgcn_mfma_f32_32x32x1f32(w0, b, c, 0, 0, 1);
        if (SIDE != 0) c = __builtin_amdgcn_mfma_f32_32x32x1f32(w1, b, c, 0, 0, 2);
        acc[2 * m] = lo16(c); acc[2 * m + 1] = hi16(c);
    }
    acc[4] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[4], b, acc[4], 0, 0, 0);
}

// the same from pre-paired fragments: a[2m] = [W(2m, lo) | W(2m+1, lo)], a[2m+1] = [W(2m, lo+4) | W(2m+1, lo+4)], a[4] as before;
// tile pairs (0,1) and (2,3) live in p[0], p[1]
template <int SIDE>
__device__ __forceinline__ void paired_step(const float* a, float b, f32x32* p, f32x16& acc4) {
    if (SIDE != 1) {
#pragma unroll
        for (int m = 0; m < 2; ++m) p[m] = __builtin_amdgcn_mfma_f32_32x32x1f32(a[2 * m], b, p[m], 0, 0, 1);
    }
    if (SIDE != 0) {
#pragma unroll
        for (int m = 0; m < 2; ++m) p[m] = __builtin_amdgcn_mfma_f32_32x32x1f32(a[2 * m + 1], b, p[m], 0, 0, 2);
    }
    acc4 = __builtin_amdgcn_mfma_f32_32x32x2f32(a[4], b, acc4, 0, 0, 0);
}

// mode 5: half-step, pre-paired; 6: full step, pre-paired
// mode 0: 5-MFMA step; 1: 32x32x2 alone, 4 per iteration; 2: 2-block form alone, 4 per iteration; 3: half-step triple; 4: two-block full step
template <int mode>
__global__ __launch_bounds__(512) void k_time(float* out, int iters) {
    float a[5], b = 0.5f + (threadIdx.x & 63) * 1e-3f;
    for (int m = 0; m < 5; ++m) a[m] = 1.0f + threadIdx.x * 1e-6f + m;
    f32x16 acc[5];
    for (int m = 0; m < 5; ++m) for (int i = 0; i < 16; ++i) acc[m][i] = 0.f;
    f32x32 p[2];
    for (int m = 0; m < 2; ++m) for (int i = 0; i < 32; ++i) p[m][i] = 0.f;
    for (int it = 0; it < iters; ++it) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            if (mode == 0) {
#pragma unroll
                for (int m = 0; m < 5; ++m) acc[m] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[m], b, acc[m], 0, 0, 0);
            } else if (mode == 1) {
                acc[u] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[u], b, acc[u], 0, 0, 0);
            } else if (mode == 2) {
                p[u & 1] = __builtin_amdgcn_mfma_f32_32x32x1f32(a[u], b, p[u & 1], 0, 0, 1);
            } else if (mode == 3) {
                half_step<0>(a, b, acc);
            } else if (mode == 4) {
                half_step<2>(a, b, acc);
            } else if (mode == 5) {
                paired_step<0>(a, b, p, acc[4]);
            } else {
                paired_step<2>(a, b, p, acc[4]);
            }
        }
    }
    float r = 0.f;
    for (int m = 0; m < 5; ++m) for (int i = 0; i < 16; ++i) r += acc[m][i];
    for (int m = 0; m < 2; ++m) for (int i = 0; i < 32; ++i) r += p[m][i];
    out[(size_t)blockIdx.x * blockDim.x + threadIdx.x] = r;
}

// part 3: one wavefront; every lane reports how many of its 80 accumulator registers differ in their bits, per side
__global__ __launch_bounds__(64) void k_bits(const float* in, int* bad) {
    const int lane = threadIdx.x;
    float a[5];
    for (int m = 0; m < 5; ++m) a[m] = in[m * 64 + lane];
    const float b = in[5 * 64 + lane];
    for (int side = 0; side < 3; ++side) {
        f32x16 ref[5], got[5];
        for (int m = 0; m < 5; ++m) for (int i = 0; i < 16; ++i) ref[m][i] = got[m][i] = in[(6 + m) * 64 + lane] * (float)(i + 1);
        const float bz = side == 2 || (lane >= 32) == (side == 1) ? b : 0.0f;   // the dead half is zero in every row; side 2: none dead
        for (int m = 0; m < 5; ++m) ref[m] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[m], bz, ref[m], 0, 0, 0);
        float w[5];
        for (int m = 0; m < 5; ++m) w[m] = a[m];
        // pre-paired: the fragments as the packer writes them (here: one swap per pair, outside of what is compared)
        f32x16 gp[5];
        for (int m = 0; m < 5; ++m) gp[m] = got[m];
        float wp[5];
        for (int m = 0; m < 5; ++m) wp[m] = a[m];
        swap32(wp[0], wp[1]); swap32(wp[2], wp[3]);
        f32x32 pp[2] = {cat(gp[0], gp[1]), cat(gp[2], gp[3])};
        if (side == 0) paired_step<0>(wp, bz, pp, gp[4]); else if (side == 1) paired_step<1>(wp, bz, pp, gp[4]); else paired_step<2>(wp, bz, pp, gp[4]);
        gp[0] = lo16(pp[0]); gp[1] = hi16(pp[0]); gp[2] = lo16(pp[1]); gp[3] = hi16(pp[1]);
        if (side == 0) half_step<0>(w, bz, got); else if (side == 1) half_step<1>(w, bz, got); else half_step<2>(w, bz, got);
        int n = 0, np = 0;
        for (int m = 0; m < 5; ++m) for (int i = 0; i < 16; ++i) {
            n += __float_as_uint(ref[m][i]) != __float_as_uint(got[m][i]);
            np += __float_as_uint(ref[m][i]) != __float_as_uint(gp[m][i]);
        }
        bad[side * 64 + lane] = n;
        bad[(3 + side) * 64 + lane] = np;
    }
}

int main() {
    float* out;
    (void)hipMalloc(&out, 256 * 512 * 4);
    hipEvent_t e0, e1;
    (void)hipEventCreate(&e0); (void)hipEventCreate(&e1);
    const int iters = 4000;
    const char* names[7] = {"5-MFMA step (32x32x2)", "32x32x2 alone", "32x32x1_2b alone", "half-step (2 swaps, 2 x 2b, 1 x 32x32x2)",
                            "full step (2 swaps, 4 x 2b, 1 x 32x32x2)", "half-step, pre-paired (2 x 2b, 1 x 32x32x2)",
                            "full step, pre-paired (4 x 2b, 1 x 32x32x2)"};
    const int per_iter[7] = {4, 4, 4, 4, 4, 4, 4};             // steps (modes 0, 3..6) or MFMAs (modes 1, 2) per iteration
    double ns[2][7];
    for (int wps = 1; wps <= 2; ++wps)
        for (int mode = 0; mode < 7; ++mode) {
            void (*const k)(float*, int) = mode == 0 ? k_time<0> : mode == 1 ? k_time<1> : mode == 2 ? k_time<2> : mode == 3 ? k_time<3>
                                         : mode == 4 ? k_time<4> : mode == 5 ? k_time<5> : k_time<6>;
            hipLaunchKernelGGL(k, dim3(256), dim3(256 * wps), 0, 0, out, iters);
            (void)hipEventRecord(e0);
            hipLaunchKernelGGL(k, dim3(256), dim3(256 * wps), 0, 0, out, iters);
            (void)hipEventRecord(e1); (void)hipEventSynchronize(e1);
            float ms = 0; (void)hipEventElapsedTime(&ms, e0, e1);
            ns[wps - 1][mode] = ms * 1e6 / ((double)iters * per_iter[mode] * wps);   // per SIMD and per step / MFMA of one wavefront
            printf("%d wavefront(s) per SIMD, %-42s %8.3f ms, %7.2f ns per %s per SIMD\n", wps, names[mode], ms, ns[wps - 1][mode],
                   mode == 1 || mode == 2 ? "MFMA" : "step");
        }
    for (int w = 0; w < 2; ++w)
        printf("%d wavefront(s) per SIMD: 2-block / 32x32x2 issue interval %.3f, half-step / step %.3f, two-block full step / step %.3f\n",
               w + 1, ns[w][2] / ns[w][1], ns[w][3] / ns[w][0], ns[w][4] / ns[w][0]);
    for (int w = 0; w < 2; ++w)
        printf("%d wavefront(s) per SIMD, pre-paired: half-step / step %.3f, two-block full step / step %.3f\n", w + 1, ns[w][5] / ns[w][0],
               ns[w][6] / ns[w][0]);

    float h[11 * 64];
    unsigned s = 12345u;
    for (int i = 0; i < 11 * 64; ++i) { s = s * 1664525u + 1013904223u; h[i] = ((int)(s >> 8) % 20001 - 10000) * 1.3e-4f; }
    float* din; int* dbad; int bad[384];
    (void)hipMalloc(&din, sizeof h); (void)hipMalloc(&dbad, sizeof bad);
    (void)hipMemcpy(din, h, sizeof h, hipMemcpyHostToDevice);
    hipLaunchKernelGGL(k_bits, dim3(1), dim3(64), 0, 0, din, dbad);
    if (hipMemcpy(bad, dbad, sizeof bad, hipMemcpyDeviceToHost) != hipSuccess) { printf("bits: copy failed\n"); return 1; }
    int n0 = 0, n1 = 0, n2 = 0;
    for (int i = 0; i < 64; ++i) { n0 += bad[i]; n1 += bad[64 + i]; n2 += bad[128 + i]; }
    printf("bits: lo-only half-step differs in %d of 5120 accumulator words, hi-only in %d, two-block full step in %d\n", n0, n1, n2);
    int q0 = 0, q1 = 0, q2 = 0;
    for (int i = 0; i < 64; ++i) { q0 += bad[192 + i]; q1 += bad[256 + i]; q2 += bad[320 + i]; }
    printf("bits, pre-paired: lo-only half-step differs in %d of 5120 accumulator words, hi-only in %d, two-block full step in %d\n", q0, q1, q2);
    return n0 || n1 || n2 || q0 || q1 || q2 ? 2 : 0;
}
