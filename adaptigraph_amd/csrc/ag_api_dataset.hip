// C-ABI, training-batch entry points: ag_fps_batch, ag_dataset_assemble (kernels in ag_dataset.hip).  The third call of the
// batch build, ag_build_edges_graphs, sits with the other graph builders in ag_api.hip.
#include "ag_host.h"
#include "ag_dataset.h"

using namespace ag;

namespace ag {
hipError_t launch_dataset_assemble(const ag_dataset_batch& a, hipStream_t st);
}

extern "C" {

int ag_fps_batch(ag_ctx* c, void* stream, const float* d_pos, const int64_t* d_pt_off, const int64_t* d_npts, int32_t stride,
                 const int32_t* d_fps_start, const float* d_fps_radius, const int32_t* d_rad_start, int32_t B, int32_t max_nobj,
                 int32_t max_pts, int32_t* d_fps_idx, int32_t* d_n_obj) {
    if (!c) return AG_ERR_INVALID;
    if (!d_pos || !d_pt_off || !d_npts || !d_fps_start || !d_fps_radius || !d_rad_start || !d_fps_idx || !d_n_obj)
        return fail(c, AG_ERR_INVALID, "ag_fps_batch: null pointer");
    if (B < 1 || stride < 1 || max_nobj < 1 || max_pts < 1)
        return fail(c, AG_ERR_INVALID, "ag_fps_batch: B=%d stride=%d max_nobj=%d max_pts=%d", B, stride, max_nobj, max_pts);
    if ((size_t)max_pts > fps_max_points())
        return fail(c, AG_ERR_UNSUPPORTED, "ag_fps_batch: a cloud of %d points exceeds the LDS-resident limit %zu", max_pts, fps_max_points());
    if (max_nobj > fps_max_nobj())
        return fail(c, AG_ERR_UNSUPPORTED, "ag_fps_batch: max_nobj=%d exceeds %d", max_nobj, fps_max_nobj());
    SlotGuard call;
    if (int rc = begin_call(c, stream, call)) return rc;
    FpsArgs a{};
    a.pos = d_pos; a.pt_off = reinterpret_cast<const long long*>(d_pt_off); a.npts = reinterpret_cast<const long long*>(d_npts);
    a.stride = stride; a.fps_start = d_fps_start; a.fps_radius = d_fps_radius; a.rad_start = d_rad_start;
    a.B = B; a.max_nobj = max_nobj; a.max_pts = max_pts; a.fps_idx = d_fps_idx; a.n_obj = d_n_obj;
    Scoped p(c, FAM_FPS);
    HIPCHK(c, launch_fps_batch(a, call.st));
    return AG_OK;
}

int ag_fps_cloud(ag_ctx* c, void* stream, const float* d_pos, const int64_t* d_pt_off, const int64_t* d_npts, int32_t stride,
                 const int32_t* d_fps_start, const float* d_fps_radius, const int32_t* d_rad_start, int32_t B, int32_t max_nobj,
                 int32_t max_pts, int32_t* d_fps_idx, int32_t* d_n_obj) {
    if (!c) return AG_ERR_INVALID;
    if (!d_pos || !d_pt_off || !d_npts || !d_fps_start || !d_fps_radius || !d_rad_start || !d_fps_idx || !d_n_obj)
        return fail(c, AG_ERR_INVALID, "ag_fps_cloud: null pointer");
    if (B < 1 || stride < 1 || max_nobj < 1 || max_pts < 1)
        return fail(c, AG_ERR_INVALID, "ag_fps_cloud: B=%d stride=%d max_nobj=%d max_pts=%d", B, stride, max_nobj, max_pts);
    if ((size_t)max_pts > fps_cloud_max_points())
        return fail(c, AG_ERR_UNSUPPORTED, "ag_fps_cloud: a cloud of %d points exceeds the limit %zu", max_pts, fps_cloud_max_points());
    if (max_nobj > fps_max_nobj())
        return fail(c, AG_ERR_UNSUPPORTED, "ag_fps_cloud: max_nobj=%d exceeds %d", max_nobj, fps_max_nobj());
    SlotGuard call;
    if (int rc = begin_call(c, stream, call)) return rc;
    float* ws = nullptr;                 // running minima of the points behind the register-resident ones, per cloud
    if (int rc = carve_slab(c, *call.sl, [&](Slab& s) { ws = s.take<float>(fps_cloud_ws_floats(B, max_pts)); })) return rc;
    FpsArgs a{};
    a.pos = d_pos; a.pt_off = reinterpret_cast<const long long*>(d_pt_off); a.npts = reinterpret_cast<const long long*>(d_npts);
    a.stride = stride; a.fps_start = d_fps_start; a.fps_radius = d_fps_radius; a.rad_start = d_rad_start;
    a.B = B; a.max_nobj = max_nobj; a.max_pts = max_pts; a.fps_idx = d_fps_idx; a.n_obj = d_n_obj;
    Scoped p(c, FAM_FPS);
    HIPCHK(c, launch_fps_cloud(a, ws, call.st));
    return AG_OK;
}

int ag_dataset_assemble(ag_ctx* c, void* stream, const ag_dataset_batch* d) {
    if (!c) return AG_ERR_INVALID;
    if (!d) return fail(c, AG_ERR_INVALID, "ag_dataset_assemble: null batch");
    if (!d->d_obj_pos || !d->d_eef_pos || !d->d_sample || !d->d_fps_idx || !d->d_n_obj || !d->d_phys || !d->d_state || !d->d_action ||
        !d->d_state_future || !d->d_attrs || !d->d_p_instance || !d->d_obj_mask || !d->d_state_mask || !d->d_eef_mask ||
        !d->d_material_index || !d->d_physics_param)
        return fail(c, AG_ERR_INVALID, "ag_dataset_assemble: null pointer");
    if (d->n_future > 1 && (!d->d_eef_future || !d->d_action_future)) return fail(c, AG_ERR_INVALID, "ag_dataset_assemble: null future tensors");
    if (d->d_adj_thresh && (!d->d_thr2 || !d->d_cull)) return fail(c, AG_ERR_INVALID, "ag_dataset_assemble: d_adj_thresh without d_thr2 / d_cull");
    if (d->B < 1 || d->n_his < 1 || d->n_future < 1 || d->max_nobj < 1 || d->n_eef < 0 || d->phys_dim < 0 || d->n_mat < 1 ||
        d->mat_col < 0 || d->mat_col >= d->n_mat)
        return fail(c, AG_ERR_INVALID, "ag_dataset_assemble: B=%d n_his=%d n_future=%d max_nobj=%d n_eef=%d phys_dim=%d n_mat=%d mat_col=%d",
                    d->B, d->n_his, d->n_future, d->max_nobj, d->n_eef, d->phys_dim, d->n_mat, d->mat_col);
    SlotGuard call;
    if (int rc = begin_call(c, stream, call)) return rc;
    Scoped p(c, FAM_ASSEMBLE);
    HIPCHK(c, launch_dataset_assemble(*d, call.st));
    return AG_OK;
}

}  // extern "C"
