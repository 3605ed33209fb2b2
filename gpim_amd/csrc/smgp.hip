// smgp.hip -- host drivers of the spectral-mixture GP (gpimhip_sm_kmat / gpimhip_sm_nll_grad / gpimhip_fit_sm /
// gpimhip_predict_sm and their _batched forms): the general padded exact-GP path at every N (no fused small-N trainer, no
// fused predict), with the covariance, the gradient contraction and the finalize step of sm.hip.  Parameters, Adam state and
// history live here: P = 2 + Q (2 D + 1) exceeds GPIMHIP_MAX_PARAMS.  Host code only: the kernels and their launchers are in
// sm.hip, the engine's drivers (workspaces, factorisation, prediction loop, training loop) in api.hip.
#include <math.h>
#include <algorithm>
#include "common.hpp"
#include "border.hpp"
#include "sm.hpp"

struct SmWs {
    DevBuf<SmDev> st;
    DevBuf<double> adam;            // 2 x SM_MAXP: Adam m, v
    DevBuf<int32_t> iter;
    DevBuf<double> sums;            // SM_MAXP: the gradient records added up over the tiles
    DevBuf<double> csx;             // 2 Q dim x np: phases of the training points
    DevBuf<double> csz;             // 2 Q dim x (test chunk): phases of the test points
    DevBuf<double> part;            // records x lower tiles
};
void sm_release(gpimhip_ctx* h) {
    SmWs* w = (SmWs*)h->sm;
    if (!w) return;
    dev_release(h, w->st, w->adam, w->iter, w->sums, w->csx, w->csz, w->part);
    delete w;
    h->sm = nullptr;
}
// np_x: phase slots of the training points (0: none), mz: of the test points, ntile: lower tiles of the gradient records
static int sm_ws(gpimhip_ctx* h, const gpimhip_sm_t* sm, int64_t np_x, int64_t mz, int64_t ntile, SmWs** out) {
    SmWs* w = (SmWs*)h->sm;
    if (!w) {       // the fixed buffers first; the workspace is published only once all of them exist
        w = new SmWs();
        int rc = w->st.alloc(h, 1);
        if (rc == GPIMHIP_OK) rc = w->adam.alloc(h, 2 * SM_MAXP);
        if (rc == GPIMHIP_OK) rc = w->iter.alloc(h, 1);
        if (rc == GPIMHIP_OK) rc = w->sums.alloc(h, SM_MAXP);
        h->sm = w;
        if (rc != GPIMHIP_OK) {
            sm_release(h);
            return rc;
        }
    }
    const int64_t per = 2 * (int64_t)sm->mixtures * sm->dim;
    GP_TRY(w->csx.grow(h, per * np_x));
    GP_TRY(w->csz.grow(h, per * mz));
    GP_TRY(w->part.grow(h, (int64_t)sm_layout(*sm).P * ntile));
    *out = w;
    return GPIMHIP_OK;
}
// B = 0: a dense entry point (no reflection mode); B > 0: the blocks of a handle in reflection mode
int sm_check(gpimhip_ctx* h, const gpimhip_sm_t* sm, const double* X, int64_t N, int B) {
    if (!h || !sm || !X || N < 1) return GPIMHIP_E_BADARG;
    FP64_ONLY(h);
    if (sm->dim < 1 || sm->dim > GPIMHIP_MAX_DIM || sm->mixtures < 1 || sm->mixtures > GPIMHIP_SM_MAX_MIXTURES) {
        gpim_set_error("the spectral-mixture kernel takes 1 .. 4 dimensions and 1 .. 16 mixtures");
        return GPIMHIP_E_BADARG;
    }
    if (h->refl.mask && B == 0) {
        gpim_set_error("the spectral-mixture kernel on a handle in reflection mode runs through gpimhip_sm_nll_grad_batched / "
                       "gpimhip_fit_sm_batched / gpimhip_predict_sm_batched (the dense entry points need gpimhip_set_reflection(h, 0, ...))");
        return GPIMHIP_E_BADARG;
    }
    if (B > 0 && (!h->refl.mask || (h->refl.mask >> sm->dim) || B != (1 << __builtin_popcount(h->refl.mask)) ||
                  h->refl.pb_stride != 1 || h->refl.pb_off != 0 || h->refl.raw || h->refl.n_total < 1)) {
        gpim_set_error("the spectral-mixture blocks need a handle in reflection mode (gpimhip_set_reflection) with all B = 2^r "
                       "blocks of the reflected axes on it (unsharded), the axes within the kernel's dimensions");
        return GPIMHIP_E_BADARG;
    }
    return GPIMHIP_OK;
}
// ---- One set of drivers for the dense model and for the reflection blocks of a grid.
// B = 0: the dense model, one problem on the N points X with the targets ys (ones unused).
// B > 0: the handle is in reflection mode, the batch is its B = 2^r blocks on the N points X of the fundamental domain, ys /
// ones (B x N) the targets and U 1 (U 1_o with a border) in the adapted basis, ONE parameter vector.  The engine's batched
// factor + inverse, solves and K^-1 product; with a border (gpimhip_set_border) the kernel-agnostic border stage of
// border.hip between the inverse and the contraction.
// The two launchers of sm.hpp that every step needs are selected here.
static int sm_setup(gpimhip_ctx* h, const gpimhip_sm_t* sm, int B, const double* u, const double* P, int64_t n, int64_t ldc,
                    double* cs, const double* ys, const double* ones, double* ypad, SmDev* st, ThetaDev* theta) {
    return B ? launch_sm_setup_refl(h, sm, u, P, n, ldc, cs, ys, ones, ypad, st, theta)
             : launch_sm_setup(h, sm, u, P, n, ldc, cs, ys, ypad, st, theta);
}
// (the blocks lie rows_pad * ld apart; scale: of the blocks' cross-covariance)
static int sm_kmat(gpimhip_ctx* h, const gpimhip_sm_t* sm, int B, const double* X, int64_t N, const double* csx, int64_t ldx,
                   const double* Z, int64_t M, const double* csz, int64_t ldz, const SmDev* st, double* out, int64_t ld,
                   int64_t rows_pad, int64_t cols_pad, int sym, int lower_only, double scale) {
    return B ? launch_sm_kmat_refl(h, sm, X, N, csx, ldx, Z, M, csz, ldz, st, out, ld, rows_pad * ld, rows_pad, cols_pad, sym,
                                   lower_only, scale)
             : launch_sm_kmat(h, sm, X, N, csx, ldx, Z, M, csz, ldz, st, out, ld, rows_pad, cols_pad, sym, lower_only);
}
static int64_t sm_grad_tiles(const gpimhip_ctx* h, int B) {
    const int64_t nb = h->np / NB;
    return (B ? B : 1) * nb * (nb + 1) / 2;
}
static int sm_begin(gpimhip_ctx* h, const gpimhip_sm_t* sm, int64_t N, int B, SmWs** w) {
    HIP_TRY(hipSetDevice(h->device));
    h->nbatch = B ? B : 1;
    HIP_TRY(hipMemsetAsync(h->info, 0, sizeof(int32_t), h->stream));
    GP_TRY(ws_ensure_padded(h, N));
    if (border_on(h)) GP_TRY(border_ensure(h));
    return sm_ws(h, sm, h->np, 0, sm_grad_tiles(h, B), w);
}
// u -> parameters, r = y - c (r_b = ys_b - c ones_b), phases; K -> L^-1; z = L^-1 r, alpha = K^-1 r
static int sm_factor(gpimhip_ctx* h, const gpimhip_sm_t* sm, SmWs* w, int B, const double* X, const double* ys, const double* ones,
                     int64_t N, const double* u) {
    const int64_t np = h->np, ld = h->ld;
    GP_TRY(sm_setup(h, sm, B, u, X, N, np, w->csx, ys, ones, h->ypad, w->st, h->theta));
    { StageTimer t(h, 4); GP_TRY(sm_kmat(h, sm, B, X, N, w->csx, np, nullptr, N, nullptr, np, w->st, h->A, ld, np, np, 1, 1, 1.0)); }
    GP_TRY(launch_potrf_inv(h, h->A, h->Tm, np, ld, h->info, rag_of(N, np)));
    return solve_vectors(h, nullptr, X, 0, N, false);
}
// loss and gradient at u (fit mode: and one Adam step); every launch reads its iteration-dependent values from the device
static int sm_iter(gpimhip_ctx* h, const gpimhip_sm_t* sm, SmWs* w, int B, const double* X, const double* ys, const double* ones,
                   int64_t N, double* u, int do_adam, double* loss_out, double* grad_out, FinalizeIter fi) {
    const int64_t np = h->np;
    GP_TRY(sm_factor(h, sm, w, B, X, ys, ones, N, u));
    { StageTimer t(h, 2); GP_TRY(launch_lauum(h, h->A, h->B, np, h->ld, rag_of(N, np))); }
    const bool bd = border_on(h);
    if (bd) GP_TRY(border_iter(h, N, true));
    {
        StageTimer t(h, 5);
        GP_TRY((B ? launch_sm_grad_refl : launch_sm_grad)(h, sm, h->B, h->ld, X, N, w->csx, np, h->alpha, w->st, w->part, w->sums));
    }
    const AdamStep st = adam_step_init();
    return launch_sm_finalize(h, sm, N, w->sums, w->st, u, w->adam, w->adam + SM_MAXP, do_adam, st, loss_out, grad_out, fi,
                              B ? ones : nullptr, B ? h->refl.n_total : 0, bd ? bws(h)->scal : nullptr);
}
// The provider of predict_cols.  Per chunk the phases of its test points, then K* (the blocks' K*_b / sqrt(B)); the
// finishers add the constant mean c: mean = c + sum_b K*_b^T alpha_b, var = sum w + noise - sum_b |L_b^-1 K*_b|^2
// (+ |sum_b Y_b^T k*_b|^2 with a border).  w->csz holds predict_chunk_cols() columns.
static PredictFamily sm_family(gpimhip_ctx* h, const gpimhip_sm_t* sm, SmWs* w, const double* X, int64_t N, int B, const double* u,
                               const double* Xs, int64_t M, double* mean_out, double* var_out) {
    PredictFamily f{sm->dim, Xs, M};
    const int64_t np = h->np;
    const int nb = (int)(np / NB);
    f.var_on_domain = B > 0;
    f.slab = [=](const PredictChunk& c) {
        GP_TRY(sm_setup(h, sm, B, u, c.Z, c.cnt, c.cpad, w->csz, nullptr, nullptr, nullptr, nullptr, nullptr));
        return sm_kmat(h, sm, B, X, N, w->csx, np, c.Z, c.cnt, w->csz, c.cpad, w->st, h->Ks, c.kld, np, c.cpad, 0, 0,
                       B ? 1.0 / sqrt((double)B) : 1.0);
    };
    if (B) {
        f.finish = [=](const PredictChunk& c) {
            GP_TRY(launch_predict_coupled(h, c.mcap, nb, c.m0, c.cnt, c.nvar, c.mcap, mean_out, var_out, c.radd));
            return launch_sm_addc(h, mean_out + c.m0, c.cnt, w->st);
        };
    } else {
        f.mean = [=](const PredictChunk& c) { return launch_sm_mean(h, h->mean_tmp, c.cnt, w->st, mean_out + c.m0); };
        f.finish = [=](const PredictChunk& c) { return launch_predict_var(h, c.mcap, nb, c.m0, c.cnt, var_out, M); };
    }
    return f;
}

// ---- the bodies of the entry points: the dense ones pass B = 0 and no ones, the _batched ones their B >= 1
static int sm_nll_grad(gpimhip_ctx* h, const gpimhip_sm_t* sm, int B, const double* X, const double* ys, const double* ones,
                       int64_t N, const double* u, double* loss_out, double* grad_out) {
    GP_TRY(sm_check(h, sm, X, N, B));
    if (!ys || (B && !ones) || !u) return GPIMHIP_E_BADARG;
    SmWs* w = nullptr;
    GP_TRY(sm_begin(h, sm, N, B, &w));
    GP_TRY(sm_iter(h, sm, w, B, X, ys, ones, N, const_cast<double*>(u), 0, loss_out, grad_out,
                   FinalizeIter{nullptr, nullptr, 0, nullptr, nullptr}));
    return finish_and_check(h);
}
static int sm_fit(gpimhip_ctx* h, const gpimhip_sm_t* sm, int B, const double* X, const double* ys, const double* ones, int64_t N,
                  double* u_inout, double lr, int32_t T, double* hist_out, double* loss_out) {
    GP_TRY(sm_check(h, sm, X, N, B));
    if (!ys || (B && !ones) || !u_inout || T < 0) return GPIMHIP_E_BADARG;
    SmWs* w = nullptr;
    GP_TRY(sm_begin(h, sm, N, B, &w));
    GP_TRY(fit_prologue(h, lr, T, w->adam, nullptr, 2 * SM_MAXP * sizeof(double), w->iter));
    if (T == 0) return finish_and_check(h);
    const FinalizeIter fi{w->iter, h->bc, T, hist_out, loss_out};
    return run_fit_iterations(h, T, FIT_LOOP_DENSE,
                              [&] { return sm_iter(h, sm, w, B, X, ys, ones, N, u_inout, 1, nullptr, nullptr, fi); });
}
static int sm_predict(gpimhip_ctx* h, const gpimhip_sm_t* sm, int B, const double* X, const double* ys, const double* ones,
                      int64_t N, const double* u, const double* Xs, int64_t M, double* mean_out, double* var_out) {
    GP_TRY(sm_check(h, sm, X, N, B));
    if (!ys || (B && !ones) || !u || !Xs || M < 1 || !mean_out || !var_out) return GPIMHIP_E_BADARG;
    SmWs* w = nullptr;
    GP_TRY(sm_begin(h, sm, N, B, &w));
    GP_TRY(sm_factor(h, sm, w, B, X, ys, ones, N, u));
    if (border_on(h)) {       // the state a prediction through the border starts from (model_state_at_u)
        GP_TRY(launch_lauum(h, h->A, h->B, h->np, h->ld, rag_of(N, h->np)));
        GP_TRY(border_iter(h, N, false));
    }
    GP_TRY(sm_ws(h, sm, h->np, predict_chunk_cols(h->np, h->nbatch, M), sm_grad_tiles(h, B), &w));
    GP_TRY(predict_cols(h, sm_family(h, sm, w, X, N, B, u, Xs, M, mean_out, var_out), N, h->nbatch));
    return finish_and_check(h);
}

extern "C" {

int gpimhip_sm_kmat(gpimhip_handle h, const gpimhip_sm_t* sm, const double* X, int64_t N, const double* Z, int64_t M,
                    const double* u, double* out, int64_t ld) {
    const int B = (h && h->refl.mask) ? 1 << __builtin_popcount(h->refl.mask) : 0;
    GP_TRY(sm_check(h, sm, X, N, B));
    const bool sym = (Z == nullptr);
    const int64_t Mv = sym ? N : M;
    if (!u || !out || Mv < 1 || ld < Mv) return GPIMHIP_E_BADARG;
    HIP_TRY(hipSetDevice(h->device));
    h->nbatch = 1;
    // reflection mode: the B blocks K_s (or K_s(X, Z) / sqrt(B)) stacked, B N rows
    const int nprob = B ? B : 1;
    BatchScope batch(h, nprob);
    const int64_t rp = pad_to(N, NB), cp = pad_to(Mv, NB);
    SmWs* w = nullptr;
    GP_TRY(sm_ws(h, sm, rp, sym ? 0 : cp, 0, &w));
    GP_TRY(ws_ensure_predict(h, rp, cp));
    const int64_t kld = h->ks_cols + 16;
    GP_TRY(sm_setup(h, sm, B, u, X, N, rp, w->csx, nullptr, nullptr, nullptr, w->st, nullptr));
    if (!sym) GP_TRY(sm_setup(h, sm, B, u, Z, M, cp, w->csz, nullptr, nullptr, nullptr, nullptr, nullptr));
    GP_TRY(sm_kmat(h, sm, B, X, N, w->csx, rp, Z, Mv, w->csz, cp, w->st, h->Ks, kld, rp, cp, sym ? 1 : 0, 0,
                   sym ? 1.0 : 1.0 / sqrt((double)nprob)));
    for (int b = 0; b < nprob; ++b)
        HIP_TRY(hipMemcpy2DAsync(out + (int64_t)b * N * ld, (size_t)ld * sizeof(double), h->Ks + (int64_t)b * rp * kld,
                                 (size_t)kld * sizeof(double), (size_t)Mv * sizeof(double), (size_t)N,
                                 hipMemcpyDeviceToDevice, h->stream));
    return GPIMHIP_OK;
}

int gpimhip_sm_nll_grad(gpimhip_handle h, const gpimhip_sm_t* sm, const double* X, const double* y, int64_t N,
                        const double* u, double* loss_out, double* grad_out) {
    return sm_nll_grad(h, sm, 0, X, y, nullptr, N, u, loss_out, grad_out);
}

int gpimhip_fit_sm(gpimhip_handle h, const gpimhip_sm_t* sm, const double* X, const double* y, int64_t N, double* u_inout,
                   double lr, int32_t T, double* hist_out, double* loss_out) {
    return sm_fit(h, sm, 0, X, y, nullptr, N, u_inout, lr, T, hist_out, loss_out);
}

int gpimhip_predict_sm(gpimhip_handle h, const gpimhip_sm_t* sm, const double* X, const double* y, int64_t N,
                       const double* u, const double* Xs, int64_t M, double* mean_out, double* var_out) {
    return sm_predict(h, sm, 0, X, y, nullptr, N, u, Xs, M, mean_out, var_out);
}

int gpimhip_sm_nll_grad_batched(gpimhip_handle h, const gpimhip_sm_t* sm, const double* X, const double* ys, const double* ones,
                                int64_t N, int32_t B, const double* u, double* loss_out, double* grad_out) {
    if (B < 1) return GPIMHIP_E_BADARG;
    return sm_nll_grad(h, sm, B, X, ys, ones, N, u, loss_out, grad_out);
}

int gpimhip_fit_sm_batched(gpimhip_handle h, const gpimhip_sm_t* sm, const double* X, const double* ys, const double* ones,
                           int64_t N, int32_t B, double* u_inout, double lr, int32_t T, double* hist_out, double* loss_out) {
    if (B < 1) return GPIMHIP_E_BADARG;
    return sm_fit(h, sm, B, X, ys, ones, N, u_inout, lr, T, hist_out, loss_out);
}

int gpimhip_predict_sm_batched(gpimhip_handle h, const gpimhip_sm_t* sm, const double* X, const double* ys, const double* ones,
                               int64_t N, int32_t B, const double* u, const double* Xs, int64_t M, double* mean_out,
                               double* var_out) {
    if (B < 1) return GPIMHIP_E_BADARG;
    return sm_predict(h, sm, B, X, ys, ones, N, u, Xs, M, mean_out, var_out);
}

}  // extern "C"
