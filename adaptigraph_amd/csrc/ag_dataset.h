// The farthest-point sampler's launch arguments (ag_dataset.hip).  Internal, not part of the C-ABI.
#pragma once
#include "ag_common.h"

namespace ag {

// both farthest-point stages of B samples (ag_dataset.hip); pt_off / npts are read at [b * stride]
struct FpsArgs {
    const float* pos; const long long* pt_off; const long long* npts; int stride;
    const int* fps_start; const float* fps_radius; const int* rad_start;
    int B, max_nobj, max_pts;
    int* fps_idx; int* n_obj;
};
hipError_t launch_fps_batch(const FpsArgs& a, hipStream_t st);
size_t fps_max_points();
int fps_max_nobj();
// the same on clouds beyond LDS (k_fps_cloud); ws: fps_cloud_ws_floats(B, max_pts) floats of the call's workspace
hipError_t launch_fps_cloud(const FpsArgs& a, float* ws, hipStream_t st);
size_t fps_cloud_max_points();
size_t fps_cloud_switch_points();
size_t fps_cloud_ws_floats(int B, int max_pts);

}  // namespace ag
