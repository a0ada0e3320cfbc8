// The squared fp32 distance of a pair, every operation rounded on its own: ((dx*dx + dy*dy) + dz*dz), the reference's arithmetic
// (graph.py:87-88, 248-267).  ONE definition for everything that has to agree with the edge builders bit for bit: the builders
// themselves (ag_edge_select.h), the contact plan, the tool rules, the chunk list's ring, the farthest-point sampler; the set losses
// take its square root.  Device code only.
#pragma once
#include "ag_common.h"

namespace ag {

__device__ __forceinline__ float dist_exact(float xi, float yi, float zi, float xj, float yj, float zj) {
    const float dx = __fsub_rn(xi, xj), dy = __fsub_rn(yi, yj), dz = __fsub_rn(zi, zj);
    return __fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz));
}

}  // namespace ag
