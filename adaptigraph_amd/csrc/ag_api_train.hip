// C-ABI, training side (see include/adaptigraph_amd.h): the backward pass, device-side weight loading and Adam, the chained
// training step and the physics-parameter fit.  Host orchestration only; context and shared helpers: ag_host.h.
#include "ag_host.h"
#include "ag_cost.h"      // chamfer_max_points
#include "ag_ppm.h"
#include "ag_setloss.h"
#include "ag_train.h"

using namespace ag;

namespace {

// Launch chunk and workspace of train_backward_chunk (ag_backward_inputs, ag_train_step_part, ag_ppm_grad_step): the context's
// chunk if set, else as many candidates as fit a 4-GiB workspace.  want_slab: the split-K slab of the weight gradients.
struct BackwardWork {
    int Bb = 1; size_t wf = 0, wi = 0; bool want_slab = false;
    float* wsf = nullptr; float* slab = nullptr; int* wsi = nullptr;
    BackwardWork() = default;                                // no backward asked for: carves nothing
    BackwardWork(const ag_ctx* c, int B, int N, int Ep, int n_his, int pstep, bool want_slab_) : want_slab(want_slab_) {
        const size_t per_cand = train_work_floats(1, N, Ep, n_his, pstep) * 4 + train_work_ints(1, N, Ep) * 4;
        Bb = (int)std::max<size_t>(1, std::min<size_t>((size_t)B, (size_t(4) << 30) / per_cand));
        if (c->chunk > 0) Bb = std::min(Bb, (int)c->chunk);
        else if (c->opt.chunk > 0) Bb = std::min(Bb, c->opt.chunk);
        wf = train_work_floats(Bb, N, Ep, n_his, pstep); wi = train_work_ints(Bb, N, Ep);
    }
    void carve(Slab& s) { wsf = s.take<float>(wf); slab = want_slab ? s.take<float>(train_slab_floats()) : nullptr; wsi = s.take<int>(wi); }
};

// the three weight images from 22 plain device tensors, by kernels on `st`; no host copy, no wait (first call: allocations)
int load_weights_device(ag_ctx* c, hipStream_t st, const float* const* d_w) {
    const bool his4 = c->dims.n_his == 4;
    if (his4 && !c->d_wb3) {
        HIPCHK(c, dev_alloc(c, reinterpret_cast<void**>(&c->d_wb3), (size_t)B3_PHASES * B3_PHASE_BYTES));
        HIPCHK(c, hipMemset(c->d_wb3, 0, (size_t)B3_PHASES * B3_PHASE_BYTES));
    }
    if (his4 && !c->d_wlat) {
        HIPCHK(c, dev_alloc(c, reinterpret_cast<void**>(&c->d_wlat), lat_weights_floats() * 4));
        HIPCHK(c, hipMemset(c->d_wlat, 0, lat_weights_floats() * 4));
    }
    HIPCHK(c, launch_pack_weights(c->dims.rel_dim, d_w, c->d_w, his4 ? reinterpret_cast<uint16_t*>(c->d_wb3) : nullptr,
                                  his4 ? c->d_wlat : nullptr, st));
    c->have_w = true;
    c->w_finite = false;   // values the host never sees (an optimiser may have produced inf): zero skip stays off for them
    ++c->weights_version;
    return enqueue_self_rows(c, st);
}

int train_step_impl(ag_ctx* c, void* stream, const float* d_state, const float* d_attrs, const float* d_action, const float* d_phys,
                    const float* d_group, int32_t n_inst, const int32_t* d_recv, const int32_t* d_send, const int32_t* d_row_ptr,
                    const int32_t* d_n_edges, int32_t edge_cap, int32_t B, int32_t N, int32_t n_p, const float* const* d_w,
                    int32_t n_future, const float* d_state_future, const float* d_eef_future, const float* d_action_future,
                    int32_t store_rest_state, int32_t edge_rows, int32_t want_grad, float* const* d_grad_w, float* d_loss,
                    float* d_pred, int32_t* d_status, int32_t B_total, int32_t accumulate, const ag_loss_spec* spec,
                    float* d_loss_terms);
int set_loss_call(ag_ctx* c, void* stream, const float* d_x, const float* d_y, int B, int N, int M, int B_total, int kind,
                  float* d_out, int32_t* d_work, const float* d_grad_out, float* d_grad_x, bool backward);
int emd_loss_call(ag_ctx* c, void* stream, const float* d_x, const float* d_y, int B, int N, int M, int B_total, float* d_out,
                  int32_t* d_work, const float* d_grad_out, float* d_grad_x, bool backward, const SetRows& rows);

}  // namespace

extern "C" {

int ag_backward(ag_ctx* c, void* stream, const float* d_state, const float* d_attrs, const float* d_action,
                const float* d_phys, const float* d_group, int32_t n_inst, const int32_t* d_recv, const int32_t* d_send,
                const int32_t* d_row_ptr, const int32_t* d_n_edges, int32_t edge_cap, int32_t B, int32_t N, int32_t n_p,
                const float* const* d_w, const float* d_grad_pos, const float* d_grad_motion, float* d_grad_state,
                float* const* d_grad_w) {
    return ag_backward_inputs(c, stream, d_state, d_attrs, d_action, d_phys, d_group, n_inst, d_recv, d_send, d_row_ptr, d_n_edges,
                              edge_cap, B, N, n_p, d_w, d_grad_pos, d_grad_motion, d_grad_state, d_grad_w, nullptr, nullptr);
}

int ag_backward_inputs(ag_ctx* c, void* stream, const float* d_state, const float* d_attrs, const float* d_action,
                       const float* d_phys, const float* d_group, int32_t n_inst, const int32_t* d_recv, const int32_t* d_send,
                       const int32_t* d_row_ptr, const int32_t* d_n_edges, int32_t edge_cap, int32_t B, int32_t N, int32_t n_p,
                       const float* const* d_w, const float* d_grad_pos, const float* d_grad_motion, float* d_grad_state,
                       float* const* d_grad_w, float* d_grad_phys, float* d_grad_action) {
    if (!c) return AG_ERR_INVALID;
    if (!d_state || !d_attrs || !d_action || !d_phys || !d_group || !d_recv || !d_send || !d_row_ptr || !d_n_edges || !d_w)
        return fail(c, AG_ERR_INVALID, "ag_backward: null pointer");
    for (int k = 0; k < 22; ++k)
        if (!d_w[k]) return fail(c, AG_ERR_INVALID, "ag_backward: null parameter %d", k);
    if (B < 1 || N < 1 || n_p < 1 || n_p > N || n_inst < 1 || edge_cap < 1)
        return fail(c, AG_ERR_INVALID, "ag_backward: bad sizes B=%d N=%d n_p=%d n_inst=%d edge_cap=%d", B, N, n_p, n_inst, edge_cap);
    if (int rc0 = check_graph_rows(c, "ag_backward", N, edge_cap)) return rc0;
    if (c->dims.nf != NF || c->dims.in_dim != IN_DIM || c->dims.rel_dim != 5 + 3 * c->dims.n_his || c->dims.pstep < 1 || c->dims.pstep > 7)
        return fail(c, AG_ERR_UNSUPPORTED, "ag_backward: nf %d, in_dim %d, rel_dim %d, pstep %d not served", c->dims.nf, c->dims.in_dim,
                    c->dims.rel_dim, c->dims.pstep);
    SlotGuard call;
    int rc = begin_call(c, stream, call);
    if (rc) return rc;
    hipStream_t st = call.st; CallSlot* sl = call.sl;
    // the edge counts size the workspace (rows per graph = the largest count) and carry the overflow verdict
    std::vector<int32_t> ne((size_t)B);
    HIPCHK(c, hipMemcpyAsync(ne.data(), d_n_edges, (size_t)B * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    int emax = 0;
    for (int v : ne) emax = std::max(emax, v);
    if (emax > edge_cap) return fail(c, AG_ERR_MAX_NR, "Exceeds max dims: a graph had %d edges, edge_cap=%d", emax, edge_cap);
    TrainArgs t{};
    t.state = d_state; t.attrs = d_attrs; t.action = d_action; t.phys = d_phys; t.group = d_group; t.n_inst = n_inst;
    t.recv = d_recv; t.send = d_send; t.row_ptr = d_row_ptr; t.n_edges = d_n_edges; t.edge_cap = edge_cap;
    t.B = B; t.N = N; t.n_p = n_p; t.n_his = c->dims.n_his; t.pstep = c->dims.pstep; t.clamp = c->dims.motion_clamp;
    t.Ep = std::max(1, emax);
    t.dpos = d_grad_pos; t.dmot = d_grad_motion; t.dstate = d_grad_state;
    t.dphys = d_grad_phys; t.daction = d_grad_action;
    for (int k = 0; k < 22 && d_grad_w; ++k) t.want_w = t.want_w || d_grad_w[k] != nullptr;   // else: data gradients only
    BackwardWork bw(c, B, N, t.Ep, t.n_his, t.pstep, true);
    int n22[22]; float* acc[22];
    weight_tensor_sizes(c->dims.rel_dim, n22);
    rc = carve_slab(c, *sl, [&](Slab& s) { bw.carve(s); for (int k = 0; k < 22; ++k) acc[k] = s.take<float>((size_t)n22[k]); });
    if (rc) return rc;
    for (int k = 0; k < 22; ++k) {
        HIPCHK(c, hipMemsetAsync(acc[k], 0, (size_t)n22[k] * 4, st));
        t.w[k] = d_w[k]; t.g[k] = acc[k];
    }
    for (int b0 = 0; b0 < B; b0 += bw.Bb)
        HIPCHK(c, train_backward_chunk(t, b0, std::min(bw.Bb, B - b0), bw.wsf, bw.wsi, bw.slab, st));
    for (int k = 0; k < 22 && d_grad_w; ++k)
        if (d_grad_w[k]) HIPCHK(c, hipMemcpyAsync(d_grad_w[k], acc[k], (size_t)n22[k] * 4, hipMemcpyDeviceToDevice, st));
    HIPCHK(c, hipStreamSynchronize(st));
    return AG_OK;
}

int ag_ctx_load_weights_device(ag_ctx* c, void* stream, const float* const* d_w) {
    if (!c) return AG_ERR_INVALID;
    if (!d_w) return fail(c, AG_ERR_INVALID, "ag_ctx_load_weights_device: null pointer");
    for (int k = 0; k < 22; ++k)
        if (!d_w[k]) return fail(c, AG_ERR_INVALID, "ag_ctx_load_weights_device: weight tensor %d is null", k);
    SlotGuard call;
    if (int rc = begin_call(c, stream, call)) return rc;
    return load_weights_device(c, call.st, d_w);
}

int ag_adam_step(ag_ctx* c, void* stream, float* const* d_w, const float* const* d_grad, float* const* d_exp_avg,
                 float* const* d_exp_avg_sq, int32_t step, double lr, double beta1, double beta2, double eps, double weight_decay,
                 int32_t* d_status) {
    if (!c) return AG_ERR_INVALID;
    if (!d_w || !d_grad || !d_exp_avg || !d_exp_avg_sq || !d_status) return fail(c, AG_ERR_INVALID, "ag_adam_step: null pointer");
    for (int k = 0; k < 22; ++k)
        if (!d_w[k] || !d_grad[k] || !d_exp_avg[k] || !d_exp_avg_sq[k]) return fail(c, AG_ERR_INVALID, "ag_adam_step: null tensor %d", k);
    if (step < 1 || !(lr >= 0.0) || !(beta1 >= 0.0 && beta1 < 1.0) || !(beta2 >= 0.0 && beta2 < 1.0) || !(eps >= 0.0) || !(weight_decay >= 0.0))
        return fail(c, AG_ERR_INVALID, "ag_adam_step: step %d, lr %g, betas (%g, %g), eps %g, weight_decay %g", step, lr, beta1, beta2, eps,
                    weight_decay);
    SlotGuard call;
    if (int rc = begin_call(c, stream, call)) return rc;
    hipStream_t st = call.st;
    AdamArgs a{};
    weight_tensor_sizes(c->dims.rel_dim, a.n);
    for (int k = 0; k < 22; ++k) { a.w[k] = d_w[k]; a.g[k] = d_grad[k]; a.m[k] = d_exp_avg[k]; a.v[k] = d_exp_avg_sq[k]; }
    // torch.optim.Adam forms the bias corrections and the step size as Python floats (doubles); a kernel sees them rounded to fp32
    const double bc1 = 1.0 - std::pow(beta1, (double)step), bc2 = 1.0 - std::pow(beta2, (double)step);
    a.wd = (float)weight_decay; a.one_minus_b1 = (float)(1.0 - beta1); a.b2 = (float)beta2; a.one_minus_b2 = (float)(1.0 - beta2);
    a.bc2_sqrt = (float)std::sqrt(bc2); a.eps = (float)eps; a.neg_step_size = (float)(-(lr / bc1));
    a.status = d_status;
    HIPCHK(c, launch_adam(a, st));
    return load_weights_device(c, st, d_w);
}

int ag_train_step(ag_ctx* c, void* stream, const float* d_state, const float* d_attrs, const float* d_action, const float* d_phys,
                  const float* d_group, int32_t n_inst, const int32_t* d_recv, const int32_t* d_send, const int32_t* d_row_ptr,
                  const int32_t* d_n_edges, int32_t edge_cap, int32_t B, int32_t N, int32_t n_p, const float* const* d_w,
                  int32_t n_future, const float* d_state_future, const float* d_eef_future, const float* d_action_future,
                  int32_t store_rest_state, int32_t edge_rows, int32_t want_grad, float* const* d_grad_w, float* d_loss,
                  float* d_pred, int32_t* d_status) {
    return ag_train_step_part(c, stream, d_state, d_attrs, d_action, d_phys, d_group, n_inst, d_recv, d_send, d_row_ptr, d_n_edges,
                              edge_cap, B, N, n_p, d_w, n_future, d_state_future, d_eef_future, d_action_future, store_rest_state,
                              edge_rows, want_grad, d_grad_w, d_loss, d_pred, d_status, B, 0);
}

// B_total = B, accumulate = 0 is ag_train_step: the same launches with the same arguments, so the same bits
int ag_train_step_part(ag_ctx* c, void* stream, const float* d_state, const float* d_attrs, const float* d_action, const float* d_phys,
                       const float* d_group, int32_t n_inst, const int32_t* d_recv, const int32_t* d_send, const int32_t* d_row_ptr,
                       const int32_t* d_n_edges, int32_t edge_cap, int32_t B, int32_t N, int32_t n_p, const float* const* d_w,
                       int32_t n_future, const float* d_state_future, const float* d_eef_future, const float* d_action_future,
                       int32_t store_rest_state, int32_t edge_rows, int32_t want_grad, float* const* d_grad_w, float* d_loss,
                       float* d_pred, int32_t* d_status, int32_t B_total, int32_t accumulate) {
    return train_step_impl(c, stream, d_state, d_attrs, d_action, d_phys, d_group, n_inst, d_recv, d_send, d_row_ptr, d_n_edges,
                           edge_cap, B, N, n_p, d_w, n_future, d_state_future, d_eef_future, d_action_future, store_rest_state,
                           edge_rows, want_grad, d_grad_w, d_loss, d_pred, d_status, B_total, accumulate, nullptr, nullptr);
}

int ag_train_step_losses(ag_ctx* c, void* stream, const float* d_state, const float* d_attrs, const float* d_action, const float* d_phys,
                         const float* d_group, int32_t n_inst, const int32_t* d_recv, const int32_t* d_send, const int32_t* d_row_ptr,
                         const int32_t* d_n_edges, int32_t edge_cap, int32_t B, int32_t N, int32_t n_p, const float* const* d_w,
                         int32_t n_future, const float* d_state_future, const float* d_eef_future, const float* d_action_future,
                         int32_t store_rest_state, int32_t edge_rows, int32_t want_grad, float* const* d_grad_w, float* d_loss,
                         float* d_pred, int32_t* d_status, int32_t B_total, int32_t accumulate, const ag_loss_spec* spec,
                         float* d_loss_terms) {
    if (!c) return AG_ERR_INVALID;
    if (!spec) return fail(c, AG_ERR_INVALID, "ag_train_step_losses: null loss spec");
    if (spec->n_terms < 1 || spec->n_terms > 4) return fail(c, AG_ERR_INVALID, "ag_train_step_losses: %d loss terms (1..4)", spec->n_terms);
    bool set_term = false, emd_term = false;
    int set_rows = -1, emd_rows = -1;                            // the flag of the terms that share a pass: -1 none yet
    for (int k = 0; k < spec->n_terms; ++k) {
        const int kind = spec->kind[k] & ~AG_LOSS_ROWS, rows = (spec->kind[k] & AG_LOSS_ROWS) ? 1 : 0;
        if (spec->kind[k] < 0 || kind < AG_LOSS_MSE || kind > AG_LOSS_EMD || (rows && kind == AG_LOSS_MSE))
            return fail(c, AG_ERR_INVALID, "ag_train_step_losses: term %d has unknown kind %d", k, spec->kind[k]);
        if (!std::isfinite(spec->weight[k])) return fail(c, AG_ERR_INVALID, "ag_train_step_losses: term %d has a non-finite weight", k);
        set_term = set_term || kind == AG_LOSS_CHAMFER || kind == AG_LOSS_HAUSDORFF;
        emd_term = emd_term || kind == AG_LOSS_EMD;
        if (kind != AG_LOSS_MSE) {
            int& seen = kind == AG_LOSS_EMD ? emd_rows : set_rows;
            if (seen >= 0 && seen != rows)
                return fail(c, AG_ERR_INVALID, "ag_train_step_losses: term %d: terms that share a pass (Chamfer and Hausdorff; Earth-mover) "
                            "must agree on AG_LOSS_ROWS", k);
            seen = rows;
        }
        if (kind == AG_LOSS_HAUSDORFF && (B_total != B || accumulate != 0))
            return fail(c, AG_ERR_UNSUPPORTED, "ag_train_step_losses: a Hausdorff term is a max over the whole batch and does not split "
                        "into parts (B=%d, B_total=%d, accumulate=%d)", B, B_total, accumulate);
    }
    if (accumulate != 0 && !d_loss_terms)
        return fail(c, AG_ERR_INVALID, "ag_train_step_losses: accumulate needs d_loss_terms (the parts' running per-term sums)");
    if (set_term && n_p >= 1 && 2 * (size_t)n_p > chamfer_max_points())
        return fail(c, AG_ERR_UNSUPPORTED, "ag_train_step_losses: 2 * n_p = %d exceeds the set-loss LDS tile (%zu points)", 2 * n_p,
                    chamfer_max_points());
    if (emd_term && n_p >= 1 && (2 * (size_t)n_p > emd_max_points() || n_p > EMD_MAX_MATCH))
        return fail(c, AG_ERR_UNSUPPORTED, "ag_train_step_losses: an Earth-mover term serves n_p <= %d and 2 * n_p <= %zu (the LDS tile), "
                    "got n_p = %d", EMD_MAX_MATCH, emd_max_points(), n_p);
    return train_step_impl(c, stream, d_state, d_attrs, d_action, d_phys, d_group, n_inst, d_recv, d_send, d_row_ptr, d_n_edges,
                           edge_cap, B, N, n_p, d_w, n_future, d_state_future, d_eef_future, d_action_future, store_rest_state,
                           edge_rows, want_grad, d_grad_w, d_loss, d_pred, d_status, B_total, accumulate, spec, d_loss_terms);
}

int ag_set_loss(ag_ctx* c, void* stream, const float* d_x, const float* d_y, int32_t B, int32_t N, int32_t M, int32_t B_total,
                int32_t kind, float* d_out, int32_t* d_work) {
    return set_loss_call(c, stream, d_x, d_y, B, N, M, B_total, kind, d_out, d_work, nullptr, nullptr, false);
}

int ag_set_loss_backward(ag_ctx* c, void* stream, const float* d_x, const float* d_y, int32_t B, int32_t N, int32_t M, int32_t B_total,
                         int32_t kind, const float* d_grad_out, float* d_grad_x, const int32_t* d_work) {
    if (c && (!d_grad_out || !d_grad_x)) return fail(c, AG_ERR_INVALID, "ag_set_loss_backward: null pointer");
    return set_loss_call(c, stream, d_x, d_y, B, N, M, B_total, kind, nullptr, const_cast<int32_t*>(d_work), d_grad_out, d_grad_x, true);
}

}  // extern "C"

namespace {

// ag_train_step_part (spec null: MSE x 1 by the launches it always made) and ag_train_step_losses (a validated spec)
int train_step_impl(ag_ctx* c, void* stream, const float* d_state, const float* d_attrs, const float* d_action, const float* d_phys,
                    const float* d_group, int32_t n_inst, const int32_t* d_recv, const int32_t* d_send, const int32_t* d_row_ptr,
                    const int32_t* d_n_edges, int32_t edge_cap, int32_t B, int32_t N, int32_t n_p, const float* const* d_w,
                    int32_t n_future, const float* d_state_future, const float* d_eef_future, const float* d_action_future,
                    int32_t store_rest_state, int32_t edge_rows, int32_t want_grad, float* const* d_grad_w, float* d_loss,
                    float* d_pred, int32_t* d_status, int32_t B_total, int32_t accumulate, const ag_loss_spec* spec,
                    float* d_loss_terms) {
    if (!c) return AG_ERR_INVALID;
    if (!c->have_w) return fail(c, AG_ERR_NO_WEIGHTS, "ag_train_step before ag_ctx_load_weights / ag_ctx_load_weights_device");
    if (!d_state || !d_attrs || !d_action || !d_phys || !d_group || !d_recv || !d_send || !d_row_ptr || !d_n_edges || !d_state_future ||
        !d_loss || !d_status)
        return fail(c, AG_ERR_INVALID, "ag_train_step: null pointer");
    if (B < 1 || N < 1 || n_p < 1 || n_p > N || n_inst < 1 || edge_cap < 1 || edge_rows < 1 || n_future < 1)
        return fail(c, AG_ERR_INVALID, "ag_train_step: bad sizes B=%d N=%d n_p=%d n_inst=%d edge_cap=%d edge_rows=%d n_future=%d", B, N, n_p,
                    n_inst, edge_cap, edge_rows, n_future);
    if (B_total < B) return fail(c, AG_ERR_INVALID, "ag_train_step_part: B_total=%d is below B=%d", B_total, B);
    if (n_future > 1 && (!d_eef_future || !d_action_future)) return fail(c, AG_ERR_INVALID, "ag_train_step: n_future > 1 needs eef_future and action_future");
    if (want_grad) {
        if (!d_w || !d_grad_w) return fail(c, AG_ERR_INVALID, "ag_train_step: want_grad needs d_w and d_grad_w");
        for (int k = 0; k < 22; ++k)
            if (!d_w[k] || !d_grad_w[k]) return fail(c, AG_ERR_INVALID, "ag_train_step: null parameter or gradient tensor %d", k);
        if (c->dims.pstep > 7) return fail(c, AG_ERR_UNSUPPORTED, "ag_train_step: pstep %d not served by the backward", c->dims.pstep);
    }
    SlotGuard call;
    int rc = begin_call(c, stream, call);
    if (rc) return rc;
    hipStream_t st = call.st; CallSlot* sl = call.sl;
    const int n_his = c->dims.n_his, rest = store_rest_state ? 1 : 0;
    const int cap = std::min(edge_cap, edge_rows);            // a graph beyond it is presented empty and reported in d_status[0]
    // forward workspace and launch chunk exactly as ag_forward's: the same kernels are chosen, the predictions are its bits
    ForwardFrame f(c, B, N, n_inst, edge_cap, n_p, B);
    // backward: edge rows per graph = the caller's bound, launch chunk as ag_backward's
    TrainArgs t{};
    t.attrs = d_attrs; t.phys = d_phys; t.group = d_group; t.n_inst = n_inst;
    t.recv = d_recv; t.send = d_send; t.row_ptr = d_row_ptr; t.edge_cap = edge_cap;
    t.B = B; t.N = N; t.n_p = n_p; t.n_his = n_his; t.pstep = c->dims.pstep; t.clamp = c->dims.motion_clamp;
    t.Ep = cap; t.want_w = true; t.wide = accumulate != 0;
    BackwardWork bw;
    if (want_grad) bw = BackwardWork(c, B, N, t.Ep, n_his, t.pstep, true);
    const size_t n_state = (size_t)B * n_his * N * 3, n_act = (size_t)B * N * 3, n_pred = (size_t)B * n_p * 3;
    float* S = nullptr; float* A = nullptr; float* P = nullptr; float* motion = nullptr; double* part = nullptr;
    float* dpos = nullptr; float* D[2] = {nullptr, nullptr};
    // a loss list: which kernels a step needs, the weights per kind (terms of one kind share their passes)
    bool has_mse = false, has_set = false, has_emd = false;
    double w_mse = 0.0; float w_ch = 0.f, w_hd = 0.f, w_em = 0.f;
    bool set_rows = false, emd_rows = false;                     // AG_LOSS_ROWS: one flag per pass (checked by the caller)
    for (int k = 0; spec && k < spec->n_terms; ++k) {
        const int kind = spec->kind[k] & ~AG_LOSS_ROWS;
        const bool rows = (spec->kind[k] & AG_LOSS_ROWS) != 0;
        if (kind == AG_LOSS_MSE) { has_mse = true; w_mse += (double)spec->weight[k]; }
        else if (kind == AG_LOSS_EMD) { has_emd = true; emd_rows = rows; w_em += spec->weight[k]; }
        else { has_set = true; set_rows = rows; (kind == AG_LOSS_CHAMFER ? w_ch : w_hd) += spec->weight[k]; }
    }
    int* live = nullptr;                                         // (B) live prefix of every graph, from d_attrs (k_prefix_rows)
    SetLossDev sd{};                                             // the set terms' clouds: prediction against state_future[:, fi]
    sd.x_bstride = (long)n_p * 3; sd.y_bstride = (long)n_future * n_p * 3; sd.B = B; sd.N = n_p; sd.M = n_p;
    int* nn_all = nullptr; int* win_all = nullptr; float* terms = d_loss_terms;
    EmdDev ed{};                                                 // the Earth-mover term: the same clouds
    ed.x_bstride = sd.x_bstride; ed.y_bstride = sd.y_bstride; ed.B = B; ed.N = n_p; ed.M = n_p;
    int* match_all = nullptr; int* emd_status_all = nullptr;
    rc = carve_slab(c, *sl, [&](Slab& s) {
        f.carve(c, s);
        if (has_emd) {
            match_all = s.take<int>((size_t)n_future * B * n_p);     // every step's match table and status words wait for the backward
            emd_status_all = s.take<int>((size_t)n_future * B);
            ed.part = s.take<double>((size_t)B);
        }
        if (has_set) {
            nn_all = s.take<int>((size_t)n_future * B * 2 * n_p);    // every step's arg-min tables and winners wait for the backward
            win_all = s.take<int>((size_t)n_future * 4);
            sd.part = s.take<double>(set_loss_part_doubles(B)); sd.pidx = s.take<int>(set_loss_part_ints(B));
        }
        if (set_rows || emd_rows) live = s.take<int>((size_t)B);
        if (spec && !d_loss_terms) terms = s.take<float>((size_t)n_future * spec->n_terms);
        S = s.take<float>((size_t)(n_future - 1) * n_state);     // model inputs of steps 1.. (step 0: the caller's)
        A = s.take<float>((size_t)(n_future - 1) * n_act);
        P = d_pred ? d_pred : s.take<float>((size_t)n_future * n_pred);
        motion = s.take<float>(n_pred);
        part = s.take<double>(train_glue_doubles());
        if (want_grad) {
            dpos = s.take<float>(n_pred);
            if (n_future > 1) { D[0] = s.take<float>(n_state); D[1] = s.take<float>(n_state); }
            bw.carve(s);
        }
    });
    if (rc) return rc;
    HIPCHK(c, launch_edge_guard(d_n_edges, B, cap, f.n_eff, d_status, st));
    // the prediction's and the label's real rows are the graph's live prefix: the same count on both sides
    if (live) HIPCHK(c, launch_prefix_rows(d_attrs, B, N, n_p, live, st));
    const SetRows no_rows{nullptr, nullptr}, live_rows{live, live};
    const SetRows& srows = set_rows ? live_rows : no_rows;
    const SetRows& erows = emd_rows ? live_rows : no_rows;
    auto state_of = [&](int fi) { return fi == 0 ? d_state : S + (size_t)(fi - 1) * n_state; };
    auto action_of = [&](int fi) { return fi == 0 ? d_action : A + (size_t)(fi - 1) * n_act; };
    // ---- train.py:94-119: n_future chained forwards, MSE of each prediction, the next model input from it
    for (int fi = 0; fi < n_future; ++fi) {
        float* pred = P + (size_t)fi * n_pred;
        rc = enqueue_forward(c, f, state_of(fi), d_attrs, action_of(fi), d_phys, d_group, d_recv, d_send, d_row_ptr, f.n_eff, B, pred,
                             motion, st);
        if (rc) return rc;
        if (!spec) HIPCHK(c, launch_step_loss(pred, d_state_future, B, n_p, n_future, fi, B_total, accumulate ? 1 : 0, part, d_loss, st));
        else {
            // train.py:100-102 with a loss list: the MSE partial sums, one nearest-neighbour pass for every set term, one finaliser
            StepLossDev fl{};
            fl.n_terms = spec->n_terms;
            for (int k = 0; k < spec->n_terms; ++k) { fl.kind[k] = spec->kind[k]; fl.weight[k] = spec->weight[k]; }
            fl.B = B; fl.n_p = n_p; fl.B_total = B_total; fl.fi = fi; fl.n_future = n_future; fl.accumulate = accumulate ? 1 : 0;
            fl.loss = d_loss; fl.terms = terms;
            if (has_mse) {
                HIPCHK(c, launch_mse_part(pred, d_state_future, B, n_p, n_future, fi, part, st));
                fl.mse_part = part; fl.n_mse_part = (int)train_glue_doubles(); fl.mse_n = (long)B_total * n_p * 3;
            }
            if (has_set) {
                sd.x = pred; sd.y = d_state_future + (size_t)fi * n_p * 3; sd.nn = nn_all + (size_t)fi * B * 2 * n_p;
                HIPCHK(c, launch_set_nn(sd, srows, st));
                fl.set_part = sd.part; fl.set_idx = sd.pidx; fl.win = win_all + 4 * fi;
            }
            if (has_emd) {
                ed.x = pred; ed.y = d_state_future + (size_t)fi * n_p * 3;
                ed.match = match_all + (size_t)fi * B * n_p; ed.status = emd_status_all + (size_t)fi * B;
                HIPCHK(c, launch_emd_assign(ed, erows, st));
                fl.emd_part = ed.part;
            }
            HIPCHK(c, launch_step_loss_final(fl, st));
        }
        if (fi + 1 < n_future)
            HIPCHK(c, launch_next_state(state_of(fi), pred, d_eef_future, d_action_future, B, N, n_p, n_his, n_future, fi, rest,
                                        S + (size_t)fi * n_state, A + (size_t)fi * n_act, st));
    }
    if (!want_grad) return AG_OK;
    // ---- train.py:122 loss_sum.backward(): last step first; the weight gradients accumulate in the caller's tensors in that order
    int n22[22];
    weight_tensor_sizes(c->dims.rel_dim, n22);
    for (int k = 0; k < 22; ++k) {
        if (!accumulate) HIPCHK(c, hipMemsetAsync(d_grad_w[k], 0, (size_t)n22[k] * 4, st));   // else: the earlier parts' sums stay
        t.w[k] = d_w[k]; t.g[k] = d_grad_w[k];
    }
    t.n_edges = f.n_eff; t.dpos = dpos;
    for (int fi = n_future - 1; fi >= 0; --fi) {
        const float* dnext = fi + 1 < n_future ? D[1] : nullptr;     // total dLoss/dstate of step fi + 1
        if (!spec) HIPCHK(c, launch_pred_grad(P + (size_t)fi * n_pred, d_state_future, dnext, B, N, n_p, n_his, n_future, fi, B_total, dpos, st));
        else {
            const float mse_scale = has_mse ? (float)(w_mse * 2.0 / ((double)B_total * n_p * 3)) : 0.f;
            HIPCHK(c, launch_pred_grad_scaled(P + (size_t)fi * n_pred, d_state_future, dnext, B, N, n_p, n_his, n_future, fi, mse_scale,
                                              dpos, st));
            if (has_set) {                                          // the set terms add their share; every dpos element has one writer
                sd.x = P + (size_t)fi * n_pred; sd.y = d_state_future + (size_t)fi * n_p * 3; sd.nn = nn_all + (size_t)fi * B * 2 * n_p;
                SetGradDev sg{};
                sg.w_chamfer = w_ch; sg.w_hausdorff = w_hd; sg.B_total = B_total; sg.win = win_all + 4 * fi; sg.gx = dpos; sg.add = 1;
                HIPCHK(c, launch_set_grad(sd, srows, sg, st));
            }
            if (has_emd) {                                          // after the other set terms, on the same stream: one writer at a time
                ed.x = P + (size_t)fi * n_pred; ed.y = d_state_future + (size_t)fi * n_p * 3;
                ed.match = match_all + (size_t)fi * B * n_p; ed.status = emd_status_all + (size_t)fi * B;
                SetGradDev sg{};
                sg.w_emd = w_em; sg.B_total = B_total; sg.gx = dpos; sg.add = 1;
                HIPCHK(c, launch_emd_grad(ed, erows, sg, st));
            }
        }
        t.state = state_of(fi); t.action = action_of(fi);
        t.dstate = fi > 0 ? D[0] : nullptr;                          // step 0's input is data
        for (int b0 = 0; b0 < B; b0 += bw.Bb) HIPCHK(c, train_backward_chunk(t, b0, std::min(bw.Bb, B - b0), bw.wsf, bw.wsi, bw.slab, st));
        if (fi > 0) {
            if (dnext) HIPCHK(c, launch_dstate_carry(D[0], dnext, B, N, n_his, rest, st));
            std::swap(D[0], D[1]);
        }
    }
    return AG_OK;
}

// set_loss_call for AG_LOSS_EMD (the arguments are checked there): the assignment solve and the finaliser, then - backward - the
// gradient.  d_work (B*(N+M) + 4 int32, optional): the (B,N) match table, then B status words.  A backward that is given them
// does not solve again (the gradient kernel clamps what it reads from the table).  rows: the counts of a flagged kind (both
// null otherwise), which live behind those words in d_work - required then.
int emd_loss_call(ag_ctx* c, void* stream, const float* d_x, const float* d_y, int B, int N, int M, int B_total, float* d_out,
                  int32_t* d_work, const float* d_grad_out, float* d_grad_x, bool backward, const SetRows& rows) {
    if ((size_t)N + (size_t)M > emd_max_points())
        return fail(c, AG_ERR_UNSUPPORTED, "ag_set_loss: N+M=%d exceeds the Earth-mover LDS tile (%zu points)", N + M, emd_max_points());
    if (std::min(N, M) > EMD_MAX_MATCH)
        return fail(c, AG_ERR_UNSUPPORTED, "ag_set_loss: the Earth-mover loss matches min(N, M) = %d pairs, at most %d are served",
                    std::min(N, M), EMD_MAX_MATCH);
    SlotGuard call;
    int rc = begin_call(c, stream, call);
    if (rc) return rc;
    hipStream_t st = call.st; CallSlot* sl = call.sl;
    EmdDev ed{};
    ed.x = d_x; ed.y = d_y; ed.x_bstride = (long)N * 3; ed.y_bstride = (long)M * 3; ed.B = B; ed.N = N; ed.M = M;
    const bool given = backward && d_work;                       // the forward's table: no solve of our own
    float* val = nullptr;
    rc = carve_slab(c, *sl, [&](Slab& s) {
        ed.match = d_work ? d_work : s.take<int>((size_t)B * N);
        ed.status = d_work ? d_work + (size_t)B * N : s.take<int>((size_t)B);
        if (!given) ed.part = s.take<double>((size_t)B);
        val = d_out ? d_out : s.take<float>(1);
    });
    if (rc) return rc;
    Scoped pr(c, FAM_COST);
    if (!given) {
        HIPCHK(c, launch_emd_assign(ed, rows, st));
        SetLossDev sd{};
        sd.B = B; sd.N = N; sd.M = M;
        HIPCHK(c, launch_set_final(sd, ed.part, B_total, AG_LOSS_EMD | (rows.nx ? AG_LOSS_ROWS : 0), val, nullptr, st));
    }
    if (!backward) return AG_OK;
    SetGradDev sg{};
    sg.gout = d_grad_out; sg.w_emd = 1.f; sg.B_total = B_total; sg.gx = d_grad_x; sg.add = 0;
    HIPCHK(c, launch_emd_grad(ed, rows, sg, st));
    return AG_OK;
}

// ag_set_loss (backward false) and ag_set_loss_backward: the nearest-neighbour pass and the finaliser, then - backward - the
// gradient.  d_work (B*(N+M) + 4 int32, optional): the arg-min tables and the Hausdorff winners.  The forward leaves them there;
// a backward that is given them skips its own pass (the gradient kernel clamps what it reads from a table, so a stale buffer
// gives a wrong gradient, never a wild read).  kind | AG_LOSS_ROWS: d_work is required and 2 B words longer, nx[B] then ny[B], inputs
// (counts are clamped by the kernels that read them).
int set_loss_call(ag_ctx* c, void* stream, const float* d_x, const float* d_y, int B, int N, int M, int B_total, int kind,
                  float* d_out, int32_t* d_work, const float* d_grad_out, float* d_grad_x, bool backward) {
    if (!c) return AG_ERR_INVALID;
    if (!d_x || !d_y || (!backward && !d_out)) return fail(c, AG_ERR_INVALID, "ag_set_loss: null pointer");
    if (B < 1 || N < 1 || M < 1 || B_total < B) return fail(c, AG_ERR_INVALID, "ag_set_loss: bad sizes B=%d N=%d M=%d B_total=%d", B, N, M, B_total);
    const bool flagged = kind >= 0 && (kind & AG_LOSS_ROWS) != 0;
    const int full_kind = kind;
    if (flagged) kind &= ~AG_LOSS_ROWS;
    if (kind != AG_LOSS_CHAMFER && kind != AG_LOSS_HAUSDORFF && kind != AG_LOSS_EMD)
        return fail(c, AG_ERR_INVALID, "ag_set_loss: kind %d is no set loss", full_kind);
    if (flagged && !d_work)
        return fail(c, AG_ERR_INVALID, "ag_set_loss: AG_LOSS_ROWS needs d_work: the counts nx[B], ny[B] are its last 2 B words");
    // AG_LOSS_ROWS: the counts follow the B*(N+M) + 4 words every kind has; the kernels clamp them where they read them
    const size_t n_tab = (size_t)B * ((size_t)N + M) + 4;
    const SetRows rows{flagged ? d_work + n_tab : nullptr, flagged ? d_work + n_tab + B : nullptr};
    if (kind == AG_LOSS_EMD)
        return emd_loss_call(c, stream, d_x, d_y, B, N, M, B_total, d_out, d_work, d_grad_out, d_grad_x, backward, rows);
    if (kind == AG_LOSS_HAUSDORFF && B_total != B)
        return fail(c, AG_ERR_UNSUPPORTED, "ag_set_loss: the Hausdorff loss is a max over the whole batch and does not split into parts");
    if ((size_t)N + (size_t)M > chamfer_max_points())
        return fail(c, AG_ERR_UNSUPPORTED, "ag_set_loss: N+M=%d exceeds the set-loss LDS tile (%zu points)", N + M, chamfer_max_points());
    SlotGuard call;
    int rc = begin_call(c, stream, call);
    if (rc) return rc;
    hipStream_t st = call.st; CallSlot* sl = call.sl;
    SetLossDev sd{};
    sd.x = d_x; sd.y = d_y; sd.x_bstride = (long)N * 3; sd.y_bstride = (long)M * 3; sd.B = B; sd.N = N; sd.M = M;
    const size_t n_nn = (size_t)B * ((size_t)N + M);
    const bool given = backward && d_work;                       // the forward's tables: no pass of our own
    int* win = nullptr; float* val = nullptr;
    rc = carve_slab(c, *sl, [&](Slab& s) {
        sd.nn = d_work ? d_work : s.take<int>(n_nn);
        win = d_work ? d_work + n_nn : s.take<int>(4);
        if (!given) { sd.part = s.take<double>(set_loss_part_doubles(B)); sd.pidx = s.take<int>(set_loss_part_ints(B)); }
        val = d_out ? d_out : s.take<float>(1);
    });
    if (rc) return rc;
    Scoped pr(c, FAM_COST);
    if (!given) {
        HIPCHK(c, launch_set_nn(sd, rows, st));
        HIPCHK(c, launch_set_final(sd, nullptr, B_total, full_kind, val, win, st));
    }
    if (!backward) return AG_OK;
    SetGradDev sg{};
    sg.gout = d_grad_out; sg.B_total = B_total; sg.win = win; sg.gx = d_grad_x; sg.add = 0;
    (kind == AG_LOSS_CHAMFER ? sg.w_chamfer : sg.w_hausdorff) = 1.f;
    HIPCHK(c, launch_set_grad(sd, rows, sg, st));
    return AG_OK;
}

}  // namespace

extern "C" {

int ag_ppm_grad_step(ag_ctx* c, void* stream, const ag_rollout_params* p, const float* d_state0, const uint8_t* d_obj_mask,
                     const float* d_eef_xz, const float* d_eef_delta, const int32_t* h_repeat, const int32_t* d_repeat,
                     const float* d_phys, const float* d_obs, const uint8_t* d_obs_mask, int32_t N_t, const float* d_row_weight,
                     const float* const* d_w, int32_t edge_rows, int32_t want_grad, float* d_state_seqs, float* d_err,
                     float* d_grad_phys, int32_t* d_status) {
    if (!c) return AG_ERR_INVALID;
    if (!c->have_w) return fail(c, AG_ERR_NO_WEIGHTS, "ag_ppm_grad_step before ag_ctx_load_weights / ag_ctx_load_weights_device");
    if (!p || !d_state0 || !d_obj_mask || !d_eef_xz || !d_eef_delta || !h_repeat || !d_repeat || !d_phys || !d_obs || !d_obs_mask ||
        !d_state_seqs || !d_err || !d_status)
        return fail(c, AG_ERR_INVALID, "ag_ppm_grad_step: null pointer");
    const int B = p->B, N_o = p->N_o, M = p->M, N = N_o + M;
    if (B < 1 || N_o < 1 || M < 0 || p->H != 1 || p->y_mode != 1 || N_t < 1 || edge_rows < 1 || p->max_nR < 1)
        return fail(c, AG_ERR_INVALID, "ag_ppm_grad_step: bad sizes B=%d N_o=%d M=%d H=%d y_mode=%d N_t=%d edge_rows=%d max_nR=%d", B, N_o, M,
                    p->H, p->y_mode, N_t, edge_rows, p->max_nR);
    if ((size_t)N_o + (size_t)N_t > chamfer_max_points())
        return fail(c, AG_ERR_UNSUPPORTED, "ag_ppm_grad_step: N_o+N_t=%d exceeds the chamfer LDS tile (%zu points)", N_o + N_t, chamfer_max_points());
    if (int rc0 = check_topk(c, N, p->topk)) return rc0;
    if (want_grad) {
        if (!d_w || !d_grad_phys || !d_row_weight) return fail(c, AG_ERR_INVALID, "ag_ppm_grad_step: want_grad needs d_w, d_row_weight and d_grad_phys");
        for (int k = 0; k < 22; ++k)
            if (!d_w[k]) return fail(c, AG_ERR_INVALID, "ag_ppm_grad_step: null parameter tensor %d", k);
        if (c->dims.pstep > 7) return fail(c, AG_ERR_UNSUPPORTED, "ag_ppm_grad_step: pstep %d not served by the backward", c->dims.pstep);
    }
    SlotGuard call;
    int rc = begin_call(c, stream, call);
    if (rc) return rc;
    hipStream_t st = call.st; CallSlot* sl = call.sl;
    const int n_his = c->dims.n_his;
    // the step count and the live prefix of every step come from the host-resident repeat counts: no read-back
    int S = 0;
    for (int b = 0; b < B; ++b) S = std::max(S, (int)h_repeat[b]);
    std::vector<int> live((size_t)S + 2, 0);                  // live[s] = rows [0, live[s]) hold every row with repeat >= s
    for (int b = 0; b < B; ++b)
        for (int s = 1; s <= std::min(S, (int)h_repeat[b]); ++s) live[s] = b + 1;
    const int cap = std::min(p->max_nR, edge_rows);           // a graph beyond it is presented empty and reported in d_status[0]
    ForwardFrame f(c, B, N, 1, cap, N_o, 0);                 // (guarded edge counts: per step, with the edge lists below)
    const int slices = pick_slices(c, B, N), ell = edge_ell_stride(N, p->topk);
    TrainArgs t{};
    t.n_inst = 1; t.edge_cap = cap; t.N = N; t.n_p = N_o; t.n_his = n_his; t.pstep = c->dims.pstep; t.clamp = c->dims.motion_clamp;
    t.Ep = cap; t.want_w = false;
    BackwardWork bw;
    if (want_grad) bw = BackwardWork(c, B, N, t.Ep, n_his, t.pstep, false);
    // workspace: [forward | builder scratch | model inputs | per-step inputs and edge lists | chamfer and backward]
    const size_t rows = (size_t)B * N, n_state = (size_t)B * n_his * N * 3, n_pred = (size_t)B * N_o * 3;
    const size_t nS = want_grad ? (size_t)std::max(S, 1) : 2, nE = want_grad ? (size_t)std::max(S, 1) : 1;
    EdgeArgs ea{};
    PpmBufs pb{};
    pb.B = B; pb.N_o = N_o; pb.M = M; pb.n_his = n_his;
    pb.state0 = d_state0; pb.obj_mask = d_obj_mask; pb.eef_xz = d_eef_xz; pb.eef_delta = d_eef_delta; pb.phys = d_phys;
    pb.repeat = d_repeat; pb.grip = p->gripper_offset; pb.grip_on = p->gripper_enable;
    float* pred = nullptr; float* motion = nullptr; float* states = nullptr;
    std::vector<int*> e_recv(nE), e_send(nE), e_rptr(nE), e_n(nE), e_eff(nE);
    int* nn = nullptr; float* cntf = nullptr; float* gseq = nullptr; float* dpos = nullptr; float* D[2] = {nullptr, nullptr};
    float* gphys = nullptr;
    rc = carve_slab(c, *sl, [&](Slab& sb) {
        f.carve(c, sb);
        ea.ell = sb.take<int>(rows * (size_t)std::max(1, ell)); ea.deg = sb.take<int>(rows);
        ea.slice_tot = sb.take<int>((size_t)B * slices); ea.cta_flag = sb.take<int>(B);
        pb.attrs = sb.take<float>(rows * 2); pb.action = sb.take<float>(rows * 3); pb.group = sb.take<float>(rows);
        pb.physN = sb.take<float>(rows); pb.mask = sb.take<uint8_t>(rows); pb.tool = sb.take<uint8_t>(rows);
        pb.ymean = sb.take<float>(B); pb.cnt = sb.take<int>(B);
        pred = sb.take<float>(n_pred); motion = sb.take<float>(n_pred);
        states = sb.take<float>(nS * n_state);
        for (size_t k = 0; k < nE; ++k) {
            e_recv[k] = sb.take<int>((size_t)B * cap); e_send[k] = sb.take<int>((size_t)B * cap);
            e_rptr[k] = sb.take<int>((size_t)B * (N + 1)); e_n[k] = sb.take<int>(B); e_eff[k] = sb.take<int>(B);
        }
        if (want_grad) {
            nn = sb.take<int>((size_t)B * (N_o + N_t)); cntf = sb.take<float>((size_t)B * 2); gseq = sb.take<float>(n_pred);
            dpos = sb.take<float>(n_pred); D[0] = sb.take<float>(n_state); D[1] = sb.take<float>(n_state);
            gphys = sb.take<float>(rows); bw.carve(sb);
        }
    });
    if (rc) return rc;
    auto state_of = [&](int s) { return states + (want_grad ? (size_t)(s - 1) : (size_t)((s - 1) & 1)) * n_state; };
    auto eslot = [&](int s) { return want_grad ? (size_t)(s - 1) : (size_t)0; };
    ea.mask = pb.mask; ea.tool = pb.tool; ea.thr = p->adj_thresh; ea.N = N; ea.topk = p->topk; ea.cta = p->connect_tools_all ? 1 : 0;
    ea.edge_cap = cap; ea.max_nR = cap; ea.slices = slices; ea.pos_bstride = (long)n_his * N * 3;
    ea.block_min_rows = c->opt.edge_block_min;

    // ---- forward_dynamics.py:225-372: the masked rollout, every step's model input and edge lists kept for the backward
    HIPCHK(c, hipMemsetAsync(d_state_seqs, 0, n_pred * 4, st));
    HIPCHK(c, launch_ppm_mean_y(pb, d_state0, B, st));
    HIPCHK(c, launch_ppm_init(pb, state_of(1), st));
    for (int s = 1; s <= S; ++s) {
        const int L = live[s], Ln = live[s + 1];
        const size_t k = eslot(s);
        float* cur = state_of(s);
        ea.pos = cur + (size_t)(n_his - 1) * N * 3; ea.B = L;
        ea.recv = e_recv[k]; ea.send = e_send[k]; ea.row_ptr = e_rptr[k]; ea.n_edges = e_n[k];
        HIPCHK(c, launch_edge_build(ea, st, prof_mark, c));
        HIPCHK(c, launch_edge_guard(e_n[k], L, cap, e_eff[k], d_status, st));
        rc = enqueue_forward(c, f, cur, pb.attrs, pb.action, pb.physN, pb.group, e_recv[k], e_send[k], e_rptr[k], e_eff[k], L, pred,
                             motion, st);
        if (rc) return rc;
        if (Ln > 0) HIPCHK(c, launch_ppm_mean_y(pb, pred, Ln, st));
        HIPCHK(c, launch_ppm_advance(pb, cur, pred, s, L, Ln, Ln > 0 ? state_of(s + 1) : cur, d_state_seqs, st));
    }
    // ---- the masked chamfer to the observed clouds (physics_param_optimizer.py:219-226)
    { Scoped pr(c, FAM_COST);
      HIPCHK(c, launch_chamfer(d_state_seqs, d_obs, d_obj_mask, d_obs_mask, B, N_o, N_t, B, d_err, st)); }
    if (!want_grad) return AG_OK;
    HIPCHK(c, hipMemsetAsync(d_grad_phys, 0, (size_t)B * N_o * 4, st));
    { Scoped pr(c, FAM_COST);
      HIPCHK(c, launch_chamfer_backward(d_state_seqs, d_obs, d_obj_mask, d_obs_mask, B, N_o, N_t, B, d_row_weight, nn, cntf, gseq, st)); }
    // ---- backward through the chain, last step first; edges are constants
    // (pb.cnt still holds the valid counts: a row's mask never changes)
    for (int k = 0; k < 22; ++k) { t.w[k] = d_w[k]; t.g[k] = nullptr; }
    t.attrs = pb.attrs; t.action = pb.action; t.phys = pb.physN; t.group = pb.group; t.dpos = dpos; t.dphys = gphys;
    for (int s = S; s >= 1; --s) {
        const int L = live[s], Ln = live[s + 1];
        const size_t k = eslot(s);
        HIPCHK(c, launch_ppm_pred_grad(pb, gseq, Ln > 0 ? D[1] : nullptr, s, L, Ln, dpos, st));
        t.state = state_of(s); t.recv = e_recv[k]; t.send = e_send[k]; t.row_ptr = e_rptr[k]; t.n_edges = e_eff[k]; t.B = L;
        t.dstate = s > 1 ? D[0] : nullptr;                      // step 1's input is data
        // no split-K slab: want_w = false makes every linear_dw return before it touches one (wsf stands in for the pointer; a
        // caller that turns want_w on must carve train_slab_floats() as ag_train_step does)
        for (int b0 = 0; b0 < L; b0 += bw.Bb) HIPCHK(c, train_backward_chunk(t, b0, std::min(bw.Bb, L - b0), bw.wsf, bw.wsi, bw.wsf, st));
        HIPCHK(c, launch_ppm_accum(gphys, L, N, N_o, d_grad_phys, st));
        if (s > 1) {
            if (Ln > 0) HIPCHK(c, launch_dstate_carry(D[0], D[1], Ln, N, n_his, 0, st));
            std::swap(D[0], D[1]);
        }
    }
    return AG_OK;
}

int ag_ppm_adam_step(ag_ctx* c, void* stream, const float* d_err, const float* d_grad_phys, int32_t n_starts, int32_t n_rows,
                     int32_t N_o, int32_t start_major, int32_t apply_update, double lr, double bias_correction1,
                     double bias_correction2, double lo, double hi, float* d_x, double* d_exp_avg, double* d_exp_avg_sq,
                     int32_t hist_cap, float* d_hist_x, double* d_hist_err, double* d_best, double* d_grad_start, float* d_phys,
                     int32_t* d_status) {
    if (!c) return AG_ERR_INVALID;
    if (!d_err || !d_x || !d_hist_x || !d_hist_err || !d_best || !d_grad_start || !d_status)
        return fail(c, AG_ERR_INVALID, "ag_ppm_adam_step: null pointer");
    if (n_starts < 1 || n_rows < 1 || N_o < 1 || hist_cap < 0)
        return fail(c, AG_ERR_INVALID, "ag_ppm_adam_step: bad sizes n_starts=%d n_rows=%d N_o=%d hist_cap=%d", n_starts, n_rows, N_o, hist_cap);
    if (apply_update && (!d_grad_phys || !d_exp_avg || !d_exp_avg_sq || !d_phys || !(lr >= 0.0) || !(bias_correction1 > 0.0) ||
                         !(bias_correction2 > 0.0) || !(lo <= hi)))
        return fail(c, AG_ERR_INVALID, "ag_ppm_adam_step: update needs gradient, moments and d_phys; lr %g, bias corrections (%g, %g), bounds [%g, %g]",
                    lr, bias_correction1, bias_correction2, lo, hi);
    // no call slot: one kernel on the caller's stream over the caller's own buffers - nothing of a slot or of the context is
    // touched, so there is no end of call another stream would ever have to wait for (as the cost and MPPI entry points)
    HIPCHK(c, hipSetDevice(c->device));
    PpmAdamArgs a{};
    a.err = d_err; a.grad = d_grad_phys; a.K = n_starts; a.n = n_rows; a.N_o = N_o; a.start_major = start_major ? 1 : 0;
    a.hist_cap = hist_cap; a.apply = apply_update ? 1 : 0; a.x = d_x; a.m = d_exp_avg; a.v = d_exp_avg_sq; a.hist_x = d_hist_x;
    a.hist_e = d_hist_err; a.best = d_best; a.gk = d_grad_start; a.phys = d_phys; a.lr = lr; a.bc1 = bias_correction1;
    a.bc2 = bias_correction2; a.lo = lo; a.hi = hi; a.status = d_status;
    HIPCHK(c, launch_ppm_adam(a, static_cast<hipStream_t>(stream)));
    return AG_OK;
}

}  // extern "C"
