// What every kernel file needs and nothing of any one subsystem (internal, not part of the C-ABI).  The declarations live in headers
// that follow the .hip files: ag_model.h, ag_options.h, ag_edges.h, ag_rules.h, ag_rollout.h, ag_cost.h, ag_train.h, ag_setloss.h,
// ag_ppm.h, ag_dataset.h, ag_cma.h; device-only helpers in ag_dist.h and ag_edge_select.h, the dynamic-LDS opt-in in ag_lds_optin.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace ag {

__device__ __forceinline__ int clampi(int v, int n) { return v < 0 ? 0 : (v >= n ? n - 1 : v); }   // a table is never trusted as an address

}  // namespace ag
