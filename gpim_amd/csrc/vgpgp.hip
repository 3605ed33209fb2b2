// vgpgp.hip -- host drivers of the multi-output GP (gpimhip_vgp_nll_grad / gpimhip_fit_vgp / gpimhip_predict_vgp): T
// single-task blocks of the batched engine, x_stride 0, whose per-problem theta comes from vgp_setup_kernel (vgp.hip); the
// dense model, the reflection blocks and the bordered blocks.  Host code only: the kernels and their launchers are in
// vgp.hip, the engine's drivers (workspaces, factorisation, prediction loop, training loop) in api.hip.
#include <math.h>
#include "common.hpp"
#include "border.hpp"
#include "vgp.hpp"

struct VgpWs {
    DevBuf<VgpDev> st;
    DevBuf<double> adam;            // 2 x VGP_MAXP: Adam m, v
    DevBuf<int32_t> iter;
    DevBuf<double> kb;              // T x np: K beta_t (reflection mode: T 2^r x np, K_b beta_{t,b})
    DevBuf<double> pred;            // 2 x T x M: the blocks' mean and variance
};
void vgp_release(gpimhip_ctx* h) {
    VgpWs* w = (VgpWs*)h->vgp;
    if (!w) return;
    dev_release(h, w->st, w->adam, w->iter, w->kb, w->pred);
    delete w;
    h->vgp = nullptr;
}
static int vgp_ws(gpimhip_ctx* h, int nprob, int T, int64_t M, VgpWs** out) {
    VgpWs* w = (VgpWs*)h->vgp;
    if (!w) {
        w = new VgpWs();
        h->vgp = w;
        GP_TRY(w->st.alloc(h, 1));
        GP_TRY(w->adam.alloc(h, 2 * VGP_MAXP));
        GP_TRY(w->iter.alloc(h, 1));
    }
    const int64_t kb = (int64_t)nprob * h->np, pr = 2 * (int64_t)T * M;
    GP_TRY(w->kb.grow(h, kb));
    GP_TRY(w->pred.grow(h, pr));
    *out = w;
    return GPIMHIP_OK;
}
// the problems per task: 2^r in reflection mode (r = the reflected axes), else 1
static int vgp_nrep(const gpimhip_ctx* h) { return h->refl.mask ? 1 << __builtin_popcount(h->refl.mask) : 1; }
int vgp_check(gpimhip_ctx* h, const gpimhip_model_t* m, const gpimhip_vgp_t* vg, const double* X, const double* Y, int64_t N) {
    if (!h || !m || !vg || !X || !Y || N < 1) return GPIMHIP_E_BADARG;
    FP64_ONLY(h);
    GP_TRY(check_model(m));
    if (m->kernel != GPIMHIP_KERNEL_RBF && m->kernel != GPIMHIP_KERNEL_MATERN52) {
        gpim_set_error("the multi-output GP takes the RBF or Matern52 kernel");
        return GPIMHIP_E_BADARG;
    }
    if (vg->tasks < 1 || vg->tasks > GPIMHIP_VGP_MAX_TASKS || (!vg->independent && (vg->rank < 1 || vg->rank > vg->tasks)) ||
        vgp_layout(*m, *vg).P > 256) {
        gpim_set_error("the multi-output GP takes 1 .. 16 tasks and an IndexKernel rank of 1 .. tasks");
        return GPIMHIP_E_BADARG;
    }
    if (h->refl.mask && (h->refl.pb_stride != 1 || h->refl.pb_off != 0 || h->refl.raw)) {
        gpim_set_error("the multi-output GP in reflection mode needs all 2^r blocks on one handle (unsharded)");
        return GPIMHIP_E_BADARG;
    }
    return GPIMHIP_OK;
}
// Loss and gradient at u (and, fit mode, one Adam step): setup -> z -> the T blocks' K, L, L^-1, z, beta -> K^-1 ->
// gradient contraction -> K beta -> finalize.  Every launch reads its iteration-dependent values from the device.
// Reflection mode: the same sequence on the T 2^r blocks A_{t,b} of N = N_q points each.
// With a border (gpimhip_set_border) the T borders S_t correct beta and the inverses after the K^-1
// product; everything downstream reads the corrected ones.
static int vgp_iter(gpimhip_ctx* h, const gpimhip_model_t* m, const gpimhip_vgp_t* vg, VgpWs* w, const double* X,
                    const double* Y, int64_t N, double* u, int do_adam, double* loss_out, double* grad_out, FinalizeIter fi) {
    const int64_t np = h->np;
    const int T = vg->tasks;
    const bool refl = h->refl.mask != 0;
    const int nrep = vgp_nrep(h);
    GP_TRY(launch_vgp_setup(h, m, vg, u, w->st, nrep));
    const bool bd = border_on(h);
    if (refl) GP_TRY(launch_vgp_project_refl(h, Y, N, T, nrep, bd ? bws(h)->uo : nullptr, w->st));
    else GP_TRY(launch_vgp_project(h, Y, N, T, w->st));
    GP_TRY(factor_at_u(h, m, X, 0, N, u, true, false));
    { StageTimer t(h, 2); GP_TRY(launch_lauum(h, h->A, h->B, np, h->ld, rag_of(N, np))); }
    if (bd) GP_TRY(border_iter(h, N, true));
    if (refl) {
        GP_TRY(launch_grad_reduce_refl(h, m, h->B, h->ld, X, N, (int)(np / NB), h->alpha, 0));
        GP_TRY(launch_vgp_kbeta_refl(h, m, X, N, T, nrep, w->kb));
    } else {
        GP_TRY(launch_grad_reduce(h, m, h->B, h->ld, X, N, (int)(np / NB), h->alpha, 0));
        GP_TRY(launch_vgp_kbeta(h, m, X, N, T, w->kb));
    }
    const AdamStep st = adam_step_init();
    return launch_vgp_finalize(h, m, vg, N, w->kb, w->st, u, w->adam, w->adam + VGP_MAXP, do_adam, st, loss_out, grad_out, fi,
                               refl ? nrep : 0, bd ? bws(h)->scal : nullptr);
}
static int vgp_begin(gpimhip_ctx* h, const gpimhip_vgp_t* vg, int64_t N, int64_t M, VgpWs** w) {
    HIP_TRY(hipSetDevice(h->device));
    h->nbatch = vg->tasks * vgp_nrep(h);
    HIP_TRY(hipMemsetAsync(h->info, 0, sizeof(int32_t), h->stream));
    GP_TRY(ws_ensure_padded(h, N));
    GP_TRY(vgp_ws(h, h->nbatch, vg->tasks, M, w));
    if (!border_on(h)) return GPIMHIP_OK;
    // the T borders' buffers, and U 1_o for the task means (outside any capture; N = the points of the fundamental domain)
    GP_TRY(border_ensure(h, vg->tasks));
    BorderWs* b = bws(h);
    const int nrep = vgp_nrep(h);
    GP_TRY(b->uo.grow(h, (int64_t)nrep * N));
    return launch_border_ones(h, b, N, nrep, b->uo);
}

extern "C" {

int gpimhip_vgp_nll_grad(gpimhip_handle h, const gpimhip_model_t* m, const gpimhip_vgp_t* vg, const double* X,
                         const double* Y, int64_t N, const double* u, double* loss_out, double* grad_out) {
    GP_TRY(vgp_check(h, m, vg, X, Y, N));
    if (!u) return GPIMHIP_E_BADARG;
    VgpWs* w = nullptr;
    GP_TRY(vgp_begin(h, vg, N, 0, &w));
    GP_TRY(vgp_iter(h, m, vg, w, X, Y, N, const_cast<double*>(u), 0, loss_out, grad_out, FinalizeIter{nullptr, nullptr, 0, nullptr, nullptr}));
    return finish_and_check(h);
}

int gpimhip_fit_vgp(gpimhip_handle h, const gpimhip_model_t* m, const gpimhip_vgp_t* vg, const double* X, const double* Y,
                    int64_t N, double* u_inout, double lr, int32_t T, double* hist_out, double* loss_out) {
    GP_TRY(vgp_check(h, m, vg, X, Y, N));
    if (!u_inout || T < 0) return GPIMHIP_E_BADARG;
    VgpWs* w = nullptr;
    GP_TRY(vgp_begin(h, vg, N, 0, &w));
    GP_TRY(fit_prologue(h, lr, T, w->adam, nullptr, 2 * VGP_MAXP * sizeof(double), w->iter));
    if (T == 0) return finish_and_check(h);
    const FinalizeIter fi{w->iter, h->bc, T, hist_out, loss_out};
    return run_fit_iterations(h, T, FIT_LOOP_DENSE,
                              [&] { return vgp_iter(h, m, vg, w, X, Y, N, u_inout, 1, nullptr, nullptr, fi); });
}

int gpimhip_predict_vgp(gpimhip_handle h, const gpimhip_model_t* m, const gpimhip_vgp_t* vg, const double* X,
                        const double* Y, int64_t N, const double* u, const double* Xs, int64_t M, double* mean_out,
                        double* var_out) {
    GP_TRY(vgp_check(h, m, vg, X, Y, N));
    if (!u || !Xs || M < 1 || !mean_out || !var_out) return GPIMHIP_E_BADARG;
    VgpWs* w = nullptr;
    GP_TRY(vgp_begin(h, vg, N, M, &w));
    const int T = vg->tasks;
    if (h->refl.mask) {          // the blocks' posterior summed per task and mixed straight into the M x T outputs
        const int nrep = vgp_nrep(h);
        GP_TRY(launch_vgp_setup(h, m, vg, u, w->st, nrep));
        const bool bd = border_on(h);
        GP_TRY(launch_vgp_project_refl(h, Y, N, T, nrep, bd ? bws(h)->uo : nullptr, w->st));
        GP_TRY(factor_at_u(h, m, X, 0, N, u, true, false));
        if (bd) {       // the corrected beta and Y_{t,b} (the inverses themselves are not needed)
            GP_TRY(launch_lauum(h, h->A, h->B, h->np, h->ld, rag_of(N, h->np)));
            GP_TRY(border_iter(h, N, false));
        }
        // the batch is T tasks of nrep consecutive problems each: K* at the task's variance, |G| = nrep, and a finisher that
        // sums each task's blocks and mixes the tasks (vgp_group_combine_kernel; the variance on every test point)
        PredictFamily f = stationary_family(h, m, X, 0, N, h->nbatch, Xs, M, mean_out, var_out);
        const VgpDev* st = w->st;
        const double scale = 1.0 / sqrt((double)nrep);
        f.var_on_domain = false;
        f.slab = [=](const PredictChunk& c) {
            return launch_kmat_refl(h, m, X, N, c.Z, c.cnt, h->theta, h->Ks, c.kld, h->np, c.cpad, 0, 0, 0, h->np * c.kld, scale);
        };
        f.finish = [=](const PredictChunk& c) {
            return launch_vgp_group_combine(h, T, nrep, (int)(h->np / NB), c.mcap, c.m0, c.cnt, st, mean_out, var_out, c.radd,
                                            c.radd ? bws(h)->r_cols : 0);
        };
        GP_TRY(predict_cols(h, f, N, h->nbatch));
        return finish_and_check(h);
    }
    GP_TRY(launch_vgp_setup(h, m, vg, u, w->st, 1));
    GP_TRY(launch_vgp_project(h, Y, N, T, w->st));
    GP_TRY(factor_at_u(h, m, X, 0, N, u, true, false));
    double* mblk = w->pred;
    double* vblk = w->pred + (int64_t)T * M;
    GP_TRY(predict_cols(h, stationary_family(h, m, X, 0, N, T, Xs, M, mblk, vblk), N, T));
    GP_TRY(launch_vgp_combine(h, T, M, w->st, mblk, vblk, mean_out, var_out));
    return finish_and_check(h);
}

}  // extern "C"
