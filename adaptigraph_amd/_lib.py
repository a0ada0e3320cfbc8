"""ctypes binding of the C-ABI in include/adaptigraph_amd.h.

The product path has NO CPU fallback: if the HIP library is missing this module raises at import of the symbols,
and every op needs a ROCm device.  PyTorch is used for device memory and streams only.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# ADAPTIGRAPH_AMD_LIB: load another build of the same C-ABI instead (the diagnostic build libadaptigraph_hip_diag.so, for
# tools/ and the injected-failure test).  The product never sets it.
LIB_PATH = os.environ.get("ADAPTIGRAPH_AMD_LIB") or os.path.join(_HERE, "csrc", "libadaptigraph_hip.so")

AG_OK = 0
AG_ERR_INVALID = -1
AG_ERR_HIP = -2
AG_ERR_MAX_NR = -3
AG_ERR_UNSUPPORTED = -4
AG_ERR_NO_WEIGHTS = -5

KERNEL_FAMILIES = ["edge_count", "edge_emit", "prep", "node_enc", "edge_enc", "mp", "node_prop", "node_final",
                   "roll_init", "roll_update", "cost", "fps", "assemble", "rule", "surface"]

# exactly the symbols include/adaptigraph_amd.h declares (tests/test_abi.py checks both directions)
EXPORTS = ["ag_abi_version", "ag_ctx_create", "ag_ctx_destroy", "ag_last_error", "ag_ctx_load_weights",
           "ag_ctx_set_chunk", "ag_build_edges", "ag_forward", "ag_rollout", "ag_rollout_async",
           "ag_ctx_set_profiling", "ag_ctx_kernel_stats", "ag_ctx_reset_stats",
           "ag_cost_chamfer", "ag_cost_state_stats", "ag_cost_penalty", "ag_ctx_set_precision", "ag_build_edges_single",
           "ag_edges_apply_tool_rule", "ag_mppi_sample", "ag_mppi_update", "ag_mppi_clip",
           "ag_ctx_set_option", "ag_ctx_get_option", "ag_ctx_rollout_counts", "ag_rollout_actions", "ag_ctx_share_counts", "ag_ctx_launch_counts", "ag_cost_reward", "ag_cost_cloth_combine",
           "ag_ctx_alloc_counts", "ag_rollout_work", "ag_backward", "ag_backward_inputs", "ag_cost_chamfer_backward",
           "ag_ctx_load_weights_device", "ag_adam_step", "ag_train_step", "ag_ppm_grad_step", "ag_ppm_adam_step", "ag_train_step_part",
           "ag_fps_batch", "ag_dataset_assemble", "ag_build_edges_graphs", "ag_eval_step",
           "ag_edges_nonfixed_rule_graphs", "ag_edges_surface_rule_graphs",
           "ag_set_loss", "ag_set_loss_backward", "ag_train_step_losses", "ag_fps_cloud"]
# the CMA-ES search is a library of its own (include/adaptigraph_amd_cma.h; tests/test_cma_restate.py holds these to that header)
CMA_LIB_PATH = os.path.join(_HERE, "csrc", "libadaptigraph_hip_cma.so")
CMA_EXPORTS = ["ag_cma_state_doubles", "ag_cma_init", "ag_cma_ask", "ag_cma_tell", "ag_cma_last_error"]
# so is the cell-list edge builder (include/adaptigraph_amd_cells.h; tests/test_cells_restate.py holds this to that header); it works
# on the engine's contexts and links against the engine's library
CELLS_LIB_PATH = os.path.join(_HERE, "csrc", "libadaptigraph_hip_cells.so")
CELLS_EXPORTS = ["ag_build_edges_cells", "ag_rollout_cells", "ag_cost_chamfer_tiled", "ag_cost_chamfer_tiled_backward", "ag_fps_cloud_grid"]
CHAMFER_TILED_MAX_POINTS, CHAMFER_TILED_MAX_TILE, CHAMFER_TILED_DEFAULT_TILE = 1 << 20, 4096, 2048     # ag_chamfer_tiled.h

AG_LOSS_MSE, AG_LOSS_CHAMFER, AG_LOSS_HAUSDORFF, AG_LOSS_EMD = 0, 1, 2, 3
AG_LOSS_ROWS = 16                       # flag on a set kind: each graph's real rows (adaptigraph_amd.h, ag_set_loss)
EMD_MAX_MATCH = 512             # min(N, M) the Earth-mover loss serves (ag_common.h)
CMA_MAX_N, CMA_MIN_POP, CMA_MAX_POP, CMA_HDR = 64, 4, 32768, 24      # limits and header words of a CMA-ES state (ag_common.h)

OPTIONS = ["streams", "chunk", "latency", "ragged", "ell_graph", "self_dedupe", "repeat_sort", "edge_wgs", "edge_block_min",
           "enc_persist", "stagger_us", "device_decode", "zigzag", "share_first", "share_prefix", "stream_min_rows", "pipeline_fork", "zero_skip",
           "edge_order", "ell_lds_words", "half_step"]


class AgDims(C.Structure):
    _fields_ = [("nf", C.c_int32), ("n_his", C.c_int32), ("pstep", C.c_int32), ("in_dim", C.c_int32),
                ("rel_dim", C.c_int32), ("motion_clamp", C.c_float)]


class AgRolloutParams(C.Structure):
    _fields_ = [("B", C.c_int32), ("H", C.c_int32), ("N_o", C.c_int32), ("M", C.c_int32), ("topk", C.c_int32),
                ("connect_tools_all", C.c_int32), ("max_nR", C.c_int32), ("y_mode", C.c_int32),
                ("adj_thresh", C.c_float), ("gripper_offset", C.c_float), ("gripper_enable", C.c_int32),
                ("physics_param", C.c_float)]


class AgDatasetBatch(C.Structure):
    """ag_dataset_batch (include/adaptigraph_amd.h), field for field."""
    _fields_ = ([(n, C.c_void_p) for n in ("d_obj_pos", "d_eef_pos", "d_sample", "d_fps_idx", "d_n_obj", "d_phys", "d_phys_noise",
                                           "d_state_noise", "d_rot", "d_adj_thresh")] +
                [(n, C.c_int32) for n in ("B", "n_his", "n_future", "max_nobj", "n_eef", "phys_dim", "n_mat", "mat_col")] +
                [(n, C.c_void_p) for n in ("d_state", "d_action", "d_eef_future", "d_action_future", "d_state_future", "d_attrs",
                                           "d_p_instance", "d_obj_mask", "d_state_mask", "d_eef_mask", "d_material_index",
                                           "d_physics_param", "d_thr2", "d_cull")])


class AgEvalStepArgs(C.Structure):
    """ag_eval_step_args (include/adaptigraph_amd.h), field for field."""
    _fields_ = ([(n, C.c_void_p) for n in ("d_state", "d_action", "d_attrs", "d_phys", "d_group", "d_recv", "d_send", "d_row_ptr",
                                           "d_n_edges", "d_obj_pos", "d_eef_pos", "d_fps_idx", "d_n_obj", "d_frames", "d_state_mask",
                                           "d_eef_mask", "d_thr2", "d_cull")] +
                [(n, C.c_int64) for n in ("obj_points", "eef_points")] +
                [(n, C.c_int32) for n in ("B", "max_nobj", "n_eef", "n_inst", "edge_cap", "edge_rows", "topk", "connect_tools_all",
                                          "store_rest_state", "pred_given", "step", "err_stride")] +
                [(n, C.c_void_p) for n in ("d_pred", "d_err", "d_state_next", "d_action_next", "d_recv_next", "d_send_next",
                                           "d_row_ptr_next", "d_n_edges_next", "d_status")])


class AgLossSpec(C.Structure):
    """ag_loss_spec (include/adaptigraph_amd.h), field for field."""
    _fields_ = [("n_terms", C.c_int32), ("kind", C.c_int32 * 4), ("weight", C.c_float * 4)]


def _rule_graphs_fields(inputs=(), sizes=(), outputs=()):
    """The fields the two batched rule structs share, with a struct's own ones where it has them: input pointers behind d_n_edges_in,
    int32 sizes behind pad_rows, output pointers last."""
    return ([("d_pos", C.c_void_p), ("pos_bstride", C.c_int64)] +
            [(n, C.c_void_p) for n in ("d_mask", "d_tool_mask", "d_send_in", "d_row_ptr_in", "d_n_edges_in") + inputs +
             ("d_bounds_pos", "d_bounds_first", "d_bounds_idx", "d_bounds_n")] +
            [("bounds_points", C.c_int64), ("ratio", C.c_double)] +
            [(n, C.c_int32) for n in ("B", "N", "n_tools", "base_cap", "idx_stride", "pad_rows") + sizes + ("edge_cap",)] +
            [(n, C.c_void_p) for n in ("d_recv", "d_send", "d_row_ptr", "d_n_edges_out") + outputs])


class AgRuleGraphsArgs(C.Structure):
    """ag_rule_graphs_args (include/adaptigraph_amd.h), field for field."""
    _fields_ = _rule_graphs_fields(inputs=("d_kNN",), outputs=("d_thr",))


class AgSurfaceRuleGraphsArgs(C.Structure):
    """ag_surface_rule_graphs_args (include/adaptigraph_amd.h), field for field."""
    _fields_ = _rule_graphs_fields(sizes=("bounds_order",), outputs=("d_bounds", "d_planes"))


_lib = None


def load():
    """Load the shared library (once).  Raises RuntimeError with build instructions when it is absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"adaptigraph_amd: HIP library not built ({LIB_PATH}). Run `python -c 'import __graft_entry__ as g; "
            f"g.build()'` or adaptigraph_amd/csrc/build.sh. There is no CPU fallback.")
    lib = C.CDLL(LIB_PATH)
    vp, i32, f32 = C.c_void_p, C.c_int32, C.c_float
    lib.ag_abi_version.restype = C.c_uint32
    lib.ag_abi_version.argtypes = []
    lib.ag_ctx_create.argtypes = [i32, C.POINTER(AgDims), C.POINTER(vp)]
    lib.ag_ctx_destroy.argtypes = [vp]
    lib.ag_last_error.argtypes = [vp]
    lib.ag_last_error.restype = C.c_char_p
    lib.ag_ctx_load_weights.argtypes = [vp, C.POINTER(vp), i32]
    lib.ag_ctx_set_chunk.argtypes = [vp, i32]
    lib.ag_ctx_set_precision.argtypes = [vp, i32]
    lib.ag_ctx_set_option.argtypes = [vp, C.c_char_p, i32]
    lib.ag_ctx_get_option.argtypes = [vp, C.c_char_p, C.POINTER(i32)]
    lib.ag_ctx_rollout_counts.argtypes = [vp, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    lib.ag_ctx_share_counts.argtypes = [vp, C.POINTER(C.c_int64)]
    lib.ag_ctx_launch_counts.argtypes = [vp, C.POINTER(C.c_int64)]
    lib.ag_ctx_alloc_counts.argtypes = [vp, C.POINTER(C.c_int64)]
    lib.ag_build_edges.argtypes = [vp, vp, vp, vp, vp, i32, i32, f32, vp, i32, i32, i32, vp, vp, vp, vp]
    lib.ag_build_edges_single.argtypes = [vp, vp, vp, vp, vp, i32, f32, f32, i32, i32, i32, vp, vp, vp, vp]
    lib.ag_edges_apply_tool_rule.argtypes = [vp, vp, vp, vp, vp, i32, i32, vp, vp, vp, C.c_double, i32, vp, vp, vp, vp]
    lib.ag_forward.argtypes = [vp, vp, vp, vp, vp, vp, vp, i32, vp, vp, vp, vp, i32, i32, i32, i32, vp, vp]
    lib.ag_backward.argtypes = [vp, vp, vp, vp, vp, vp, vp, i32, vp, vp, vp, vp, i32, i32, i32, i32,
                                C.POINTER(vp), vp, vp, vp, C.POINTER(vp)]
    lib.ag_backward_inputs.argtypes = lib.ag_backward.argtypes + [vp, vp]
    lib.ag_ctx_load_weights_device.argtypes = [vp, vp, C.POINTER(vp)]
    f64 = C.c_double
    lib.ag_adam_step.argtypes = [vp, vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), i32, f64, f64, f64, f64, f64, vp]
    lib.ag_train_step.argtypes = [vp, vp, vp, vp, vp, vp, vp, i32, vp, vp, vp, vp, i32, i32, i32, i32, C.POINTER(vp),
                                  i32, vp, vp, vp, i32, i32, i32, C.POINTER(vp), vp, vp, vp]
    lib.ag_train_step_part.argtypes = lib.ag_train_step.argtypes + [i32, i32]
    lib.ag_train_step_losses.argtypes = lib.ag_train_step_part.argtypes + [C.POINTER(AgLossSpec), vp]
    lib.ag_set_loss.argtypes = [vp, vp, vp, vp, i32, i32, i32, i32, i32, vp, vp]
    lib.ag_set_loss_backward.argtypes = [vp, vp, vp, vp, i32, i32, i32, i32, i32, vp, vp, vp]
    lib.ag_ppm_grad_step.argtypes = [vp, vp, C.POINTER(AgRolloutParams), vp, vp, vp, vp, vp, vp, vp, vp, vp, i32, vp, C.POINTER(vp),
                                     i32, i32, vp, vp, vp, vp]
    lib.ag_ppm_adam_step.argtypes = [vp, vp, vp, vp, i32, i32, i32, i32, i32, f64, f64, f64, f64, f64, vp, vp, vp, i32, vp, vp, vp,
                                     vp, vp, vp]
    lib.ag_rollout.argtypes = [vp, vp, C.POINTER(AgRolloutParams), vp, vp, vp, vp, vp, vp, vp]  # ..., h_repeat, d_phys_vec, d_state_seqs
    lib.ag_rollout_async.argtypes = [vp, vp, C.POINTER(AgRolloutParams), vp, vp, vp, vp, vp, vp, vp, vp]
    lib.ag_rollout_actions.argtypes = [vp, vp, C.POINTER(AgRolloutParams), vp, vp, f32, vp, i32, vp, vp, vp, vp]
    lib.ag_rollout_work.argtypes = [vp, vp, C.POINTER(AgRolloutParams), vp, vp, f32, vp, i32, vp, vp]
    lib.ag_cost_chamfer.argtypes = [vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, vp]
    lib.ag_cost_chamfer_backward.argtypes = [vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, vp, vp]
    lib.ag_cost_state_stats.argtypes = [vp, vp, vp, i32, i32, vp, vp]
    lib.ag_cost_penalty.argtypes = [vp, vp, vp, vp, vp, i32, i32, i32, i32, f32, vp]
    lib.ag_cost_reward.argtypes = [vp, vp, vp, vp, vp, vp, vp, i32, i32, vp]
    lib.ag_cost_cloth_combine.argtypes = [vp, vp, vp, vp, C.c_int64, vp]
    lib.ag_mppi_sample.argtypes = [vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, f32, vp]
    lib.ag_mppi_update.argtypes = [vp, vp, vp, vp, vp, vp, i32, i32, f32, f32, vp]
    lib.ag_mppi_clip.argtypes = [vp, vp, vp, vp, vp, C.c_int64, vp]
    lib.ag_fps_batch.argtypes = [vp, vp, vp, vp, vp, i32, vp, vp, vp, i32, i32, i32, vp, vp]
    lib.ag_fps_cloud.argtypes = lib.ag_fps_batch.argtypes
    lib.ag_dataset_assemble.argtypes = [vp, vp, C.POINTER(AgDatasetBatch)]
    lib.ag_build_edges_graphs.argtypes = [vp, vp, vp, C.c_int64, vp, vp, i32, i32, vp, vp, i32, i32, i32, vp, vp, vp, vp]
    lib.ag_eval_step.argtypes = [vp, vp, C.POINTER(AgEvalStepArgs)]
    lib.ag_edges_nonfixed_rule_graphs.argtypes = [vp, vp, C.POINTER(AgRuleGraphsArgs)]
    lib.ag_edges_surface_rule_graphs.argtypes = [vp, vp, C.POINTER(AgSurfaceRuleGraphsArgs)]
    lib.ag_ctx_set_profiling.argtypes = [vp, i32]
    lib.ag_ctx_kernel_stats.argtypes = [vp, C.c_char_p, C.POINTER(C.c_double), C.POINTER(C.c_int64)]
    lib.ag_ctx_reset_stats.argtypes = [vp]
    for name in EXPORTS:
        fn = getattr(lib, name)
        if name not in ("ag_abi_version", "ag_last_error"):
            fn.restype = C.c_int
    _lib = lib
    return lib


_cma = None


def load_cma():
    """Load the CMA-ES library (once).  Raises RuntimeError with build instructions when it is absent."""
    global _cma
    if _cma is not None:
        return _cma
    if not os.path.exists(CMA_LIB_PATH):
        raise RuntimeError(
            f"adaptigraph_amd: CMA-ES library not built ({CMA_LIB_PATH}). Run `python -c 'import __graft_entry__ as g; "
            f"g.build()'` or adaptigraph_amd/csrc/build.sh. There is no CPU fallback.")
    lib = C.CDLL(CMA_LIB_PATH)
    vp, i32, f64 = C.c_void_p, C.c_int32, C.c_double
    lib.ag_cma_state_doubles.argtypes = [i32, i32]
    lib.ag_cma_init.argtypes = [i32, vp, i32, i32, vp, f64, vp, vp, vp, vp, f64, i32, vp]
    lib.ag_cma_ask.argtypes = [i32, vp, vp, vp, vp, vp]
    lib.ag_cma_tell.argtypes = [i32, vp, vp, vp, vp, vp, vp, vp]
    lib.ag_cma_last_error.argtypes = []
    lib.ag_cma_last_error.restype = C.c_char_p
    for name in CMA_EXPORTS:
        if name != "ag_cma_last_error":
            getattr(lib, name).restype = C.c_int
    _cma = lib
    return lib


_cells = None


def load_cells():
    """Load the cell-list edge builder's library (once), behind the engine's, which it links against.  Raises RuntimeError with
    build instructions when it is absent."""
    global _cells
    if _cells is not None:
        return _cells
    load()
    if not os.path.exists(CELLS_LIB_PATH):
        raise RuntimeError(
            f"adaptigraph_amd: cell-list edge builder not built ({CELLS_LIB_PATH}). Run `python -c 'import __graft_entry__ as g; "
            f"g.build()'` or adaptigraph_amd/csrc/build.sh. There is no CPU fallback.")
    lib = C.CDLL(CELLS_LIB_PATH)
    vp, i32, f32 = C.c_void_p, C.c_int32, C.c_float
    lib.ag_build_edges_cells.argtypes = [vp, vp, vp, C.c_int64, vp, vp, i32, i32, f32, vp, vp, i32, i32, C.c_int64, vp, vp, vp, vp]
    lib.ag_build_edges_cells.restype = C.c_int
    lib.ag_rollout_cells.argtypes = [vp, vp, C.POINTER(AgRolloutParams), vp, vp, vp, vp, vp, vp, vp, vp]   # as ag_rollout_async
    lib.ag_rollout_cells.restype = C.c_int
    lib.ag_cost_chamfer_tiled.argtypes = [vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, vp]           # as ag_cost_chamfer, + tile_points
    lib.ag_cost_chamfer_tiled.restype = C.c_int
    lib.ag_cost_chamfer_tiled_backward.argtypes = [vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, vp, vp]
    lib.ag_cost_chamfer_tiled_backward.restype = C.c_int
    lib.ag_fps_cloud_grid.argtypes = [vp, vp, vp, vp, vp, i32, vp, vp, vp, i32, i32, i32, i32, vp, vp]    # as ag_fps_cloud, + cells
    lib.ag_fps_cloud_grid.restype = C.c_int
    _cells = lib
    return lib
