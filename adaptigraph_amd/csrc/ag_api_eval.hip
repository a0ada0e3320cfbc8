// C-ABI, eval-rollout entry point: ag_eval_step (kernel in ag_eval.hip).  Host orchestration only; context and shared helpers:
// ag_host.h.
#include "ag_host.h"

using namespace ag;

namespace ag {
hipError_t launch_eval_advance(const ag_eval_step_args& a, int n_his, unsigned char* mask_next, hipStream_t st);
int fps_max_nobj();
}

extern "C" {

int ag_eval_step(ag_ctx* c, void* stream, const ag_eval_step_args* p) {
    if (!c) return AG_ERR_INVALID;
    if (!p) return fail(c, AG_ERR_INVALID, "ag_eval_step: null arguments");
    if (!p->pred_given && !c->have_w) return fail(c, AG_ERR_NO_WEIGHTS, "ag_eval_step before ag_ctx_load_weights / ag_ctx_load_weights_device");
    if (!p->d_state || !p->d_obj_pos || !p->d_eef_pos || !p->d_fps_idx || !p->d_n_obj || !p->d_frames || !p->d_state_mask ||
        !p->d_eef_mask || !p->d_thr2 || !p->d_cull || !p->d_pred || !p->d_err || !p->d_state_next || !p->d_action_next ||
        !p->d_recv_next || !p->d_send_next || !p->d_row_ptr_next || !p->d_n_edges_next || !p->d_status)
        return fail(c, AG_ERR_INVALID, "ag_eval_step: null pointer");
    if (!p->pred_given && (!p->d_action || !p->d_attrs || !p->d_phys || !p->d_group || !p->d_recv || !p->d_send || !p->d_row_ptr || !p->d_n_edges))
        return fail(c, AG_ERR_INVALID, "ag_eval_step: null model input");
    if (p->d_state_next == p->d_state || p->d_recv_next == p->d_recv || p->d_send_next == p->d_send || p->d_row_ptr_next == p->d_row_ptr ||
        p->d_n_edges_next == p->d_n_edges)
        return fail(c, AG_ERR_INVALID, "ag_eval_step: the next state and the next graphs must not be the current ones");
    const int B = p->B, No = p->max_nobj, Ne = p->n_eef;
    if (B < 1 || No < 1 || Ne < 0 || p->n_inst < 1 || p->edge_cap < 1 || p->edge_rows < 1 || p->step < 0 || p->err_stride < B ||
        p->obj_points < 1 || p->eef_points < Ne)
        return fail(c, AG_ERR_INVALID, "ag_eval_step: bad sizes B=%d max_nobj=%d n_eef=%d n_inst=%d edge_cap=%d edge_rows=%d step=%d "
                    "err_stride=%d obj_points=%lld eef_points=%lld", B, No, Ne, p->n_inst, p->edge_cap, p->edge_rows, p->step, p->err_stride,
                    (long long)p->obj_points, (long long)p->eef_points);
    const int N = No + Ne;
    if (No > fps_max_nobj()) return fail(c, AG_ERR_UNSUPPORTED, "ag_eval_step: max_nobj=%d exceeds %d", No, fps_max_nobj());
    if (int rc0 = check_topk(c, N, p->topk)) return rc0;
    SlotGuard call;
    int rc = begin_call(c, stream, call);
    if (rc) return rc;
    hipStream_t st = call.st; CallSlot* sl = call.sl;
    const int n_his = c->dims.n_his;
    const int cap = std::min(p->edge_cap, p->edge_rows);
    // forward workspace and launch chunk exactly as ag_forward's: the same kernels are chosen, the predictions are its bits
    ForwardFrame f(c, B, N, p->n_inst, p->edge_cap, No, B);
    EdgeArgs ea{};
    ea.slices = pick_slices(c, B, N);
    const size_t rows = (size_t)B * N;
    const int ell = edge_ell_stride(N, p->topk);
    float* motion = nullptr; unsigned char* mask_next = nullptr;
    rc = carve_slab(c, *sl, [&](Slab& s) {
        if (!p->pred_given) { f.carve(c, s); motion = s.take<float>((size_t)B * No * 3); }
        mask_next = s.take<unsigned char>(rows);
        ea.ell = s.take<int>(rows * (size_t)std::max(1, ell)); ea.deg = s.take<int>(rows);
        ea.slice_tot = s.take<int>((size_t)B * ea.slices); ea.cta_flag = s.take<int>(B);
    });
    if (rc) return rc;
    if (!p->pred_given) {
        HIPCHK(c, launch_edge_guard(p->d_n_edges, B, cap, f.n_eff, p->d_status, st));
        rc = enqueue_forward(c, f, p->d_state, p->d_attrs, p->d_action, p->d_phys, p->d_group, p->d_recv, p->d_send, p->d_row_ptr, f.n_eff,
                             B, p->d_pred, motion, st);
        if (rc) return rc;
    }
    { Scoped pr(c, FAM_ROLL_UPDATE);
      HIPCHK(c, launch_eval_advance(*p, n_his, mask_next, st)); }
    ea.pos = p->d_state_next + (size_t)(n_his - 1) * N * 3; ea.pos_bstride = (long)n_his * N * 3;
    ea.mask = mask_next; ea.tool = p->d_eef_mask; ea.thr_vec = p->d_cull; ea.thr2_vec = p->d_thr2;
    ea.B = B; ea.N = N; ea.topk = p->topk; ea.cta = p->connect_tools_all ? 2 : 0; ea.edge_cap = p->edge_cap;
    ea.recv = p->d_recv_next; ea.send = p->d_send_next; ea.row_ptr = p->d_row_ptr_next; ea.n_edges = p->d_n_edges_next;
    ea.overflow = nullptr; ea.max_nR = ea.edge_cap; ea.zero_on_overflow = 0;
    ea.block_min_rows = c->opt.edge_block_min;
    HIPCHK(c, launch_edge_build(ea, st, prof_mark, c));
    return AG_OK;
}

}  // extern "C"
