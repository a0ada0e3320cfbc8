// The farthest-point samplers' argmax: ONE max-reduction over a packed 64-bit key - distance bits above (non-negative floats order
// as integers), inverted index below - so the largest key is the largest distance at the LOWEST index, whatever the grouping.
// Shared by ag_dataset.hip (k_fps_batch, k_fps_cloud) and ag_fps_grid.hip (k_fps_select).  Device code only.
#pragma once
#include "ag_common.h"

namespace ag {

__device__ __forceinline__ unsigned long long fps_key(float d, int i) {
    return ((unsigned long long)__float_as_uint(d) << 32) | (0xffffffffu - (unsigned)i);
}
__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned lo = __shfl_xor((unsigned)(v & 0xffffffffull), o);
        const unsigned hi = __shfl_xor((unsigned)(v >> 32), o);
        const unsigned long long w = ((unsigned long long)hi << 32) | lo;
        v = w > v ? w : v;
    }
    return v;
}
// max of `mine` over the workgroup, in every thread.  `it` counts the reductions of the launch: consecutive ones use
// alternate halves of wkey, so one barrier per reduction is enough (a thread can only overwrite a half after every thread
// has passed the barrier of the reduction in between, i.e. has read it).
// WAVES: wavefronts of the workgroup (wkey holds 2 * WAVES keys).
template <int WAVES>
__device__ __forceinline__ unsigned long long block_max_u64(unsigned long long mine, unsigned long long* wkey, int& it) {
    mine = wave_max_u64(mine);
    unsigned long long* w = wkey + (it & 1) * WAVES;
    if ((threadIdx.x & 63) == 0) w[threadIdx.x >> 6] = mine;
    __syncthreads();
    unsigned long long g = w[0];
#pragma unroll
    for (int k = 1; k < WAVES; ++k) g = w[k] > g ? w[k] : g;
    ++it;
    return g;
}

}  // namespace ag
