// The tiled Chamfer kernels (ag_chamfer_tiled.hip; entry points in ag_api_cells.hip).  Internal, not part of the C-ABI.
#pragma once
#include "ag_common.h"

namespace ag {

// Points per cloud the tiled kernels serve, points a workgroup owns, and the tile of the other cloud it streams through LDS
// (even, 2 .. CHAMFER_TILED_MAX_TILE; 12 bytes of LDS per tile point).
constexpr int CHAMFER_TILED_MAX_POINTS = 1 << 20, CHAMFER_TILED_OWN = 1024;
constexpr int CHAMFER_TILED_MAX_TILE = 4096, CHAMFER_TILED_DEFAULT_TILE = 2048;

// chamfer(x, y) with launch_chamfer's arguments and bits.  d2 (R, N+M) floats is workspace: per row the smallest squared distance
// of every x point, then of every y point.
hipError_t launch_chamfer_tiled(const float* x, const float* y, const uint8_t* xm, const uint8_t* ym, int R, int N, int M, int By,
                                int tile, float* d2, float* out, hipStream_t st);
// its gradient toward x with launch_chamfer_backward's arguments and bits: nn (R, N+M) ints and cnt (R,2) floats are workspace
hipError_t launch_chamfer_tiled_backward(const float* x, const float* y, const uint8_t* xm, const uint8_t* ym, int R, int N, int M,
                                         int By, int tile, const float* gout, int* nn, float* cnt, float* gx, hipStream_t st);

}  // namespace ag
