// draws.hip -- host side of the posterior draws: the workspace, the kernel families and the drivers of the draw methods, and
// the extern "C" entries gpimhip_sample_* (gpimhip_sample_kron: kron.hip, gpimhip_sample_pkron: pkrongp.hip).  Host code only:
// the kernels are in sample.hip, sm.hip and vgp.hip; the engine's drivers (workspaces, factorisations, tile engine) in api.hip.
#include <math.h>
#include <stdio.h>
#include <algorithm>
#include "common.hpp"
#include "border.hpp"
#include "vgp.hpp"
#include "kron.hpp"
#include "sm.hpp"
#include "sample.hpp"

// ------------------------------------------------------------------------------------------
// joint posterior draws of the exact GP (sample.hip): one factorisation of the joint covariance of
// [X; Xs].  The matrix belongs to this path: a Bayesian-optimisation step alternates training at order N with a draw at
// order N + M, and sending the draw through ws_ensure would free and re-allocate A, B and Tm twice per step (two of the
// three unused here).  `sub` is a handle of its own on the model handle's stream, as the border's: its workspace holds
// what the step schedule needs (diagonal-block inverses, plans, status word, theta, O(order) vectors), no matrices.
// J, the stacked coordinates and the vectors grow only when a larger order arrives.
// ------------------------------------------------------------------------------------------
struct SampleWs {
    gpimhip_ctx* sub = nullptr;
    DevBuf<double> J;               // padded (N + M)^2 joint covariance -> its factor
    DevBuf<double> XX;              // [X; Xs]
    DevBuf<double> vec;             // t (order) | piece (512) | mean (M): forward substitution, draws
    // pathwise draws (sample_pathwise_impl): a context per matrix order (a call factors at both, and a context that changes
    // its order rebuilds its launch plan), one block of the prior, the training matrix, the vectors
    gpimhip_ctx* subp = nullptr;                    // order M / 2^r: the reflection blocks of the grid, one after the other
    gpimhip_ctx* subt = nullptr;                    // order N: K + (noise + jitter) I
    DevBuf<double> Pb;
    DevBuf<double> Kt;
    DevBuf<double> pw;
    // multi-output draws (sample_vgp_impl / sample_vgp_blocks_impl): the state of the reduction, the T
    // latent blocks' thetas, their targets z_t (T x N), draws H (T x S x M) and moments (2 x T x M: mean, variance)
    DevBuf<VgpDev> vst;
    DevBuf<ThetaDev> vth;
    DevBuf<double> vz;
    DevBuf<double> vH;
    DevBuf<double> vmom;
    // draws of the dense-by-Kronecker blocks (pkrongp.hip: gpimhip_sample_pkron, through sample_pkron_ws): one arena carved
    // per call and the union of the complete axes when the training axes do not serve; `sub` factors L_P
    DevBuf<double> ck;
    KronAxes ck_un;
    // draws of the spectral-mixture model (sm_family): the two parameter sets of launch_sm_params, the
    // phases of the dense rows ([X; Xs], or the training rows), of the fundamental domain and of the grid G, and y - c
    DevBuf<SmDev> smst;
    DevBuf<double> phx;
    DevBuf<double> phq;
    DevBuf<double> phg;
    DevBuf<double> smy;
};
// the handle's draw workspace, created on first use
static SampleWs* sws(gpimhip_ctx* h) {
    if (!h->sample) h->sample = new SampleWs();
    return (SampleWs*)h->sample;
}
PkronDrawWs sample_pkron_ws(gpimhip_ctx* h) {
    SampleWs* w = sws(h);
    return PkronDrawWs{w->sub, w->ck, w->ck_un};
}
int64_t sample_bytes(const gpimhip_ctx* h) {
    const SampleWs* w = (const SampleWs*)h->sample;
    if (!w) return 0;
    return (w->sub ? w->sub->bytes : 0) + (w->subp ? w->subp->bytes : 0) + (w->subt ? w->subt->bytes : 0);
}
void sample_release(gpimhip_ctx* h) {
    SampleWs* w = (SampleWs*)h->sample;
    if (!w) return;
    dev_release(h, w->J, w->XX, w->vec, w->Pb, w->Kt, w->pw, w->vst, w->vth, w->vz, w->vH, w->vmom, w->ck, w->smst, w->phx, w->phq,
                w->phg, w->smy);
    kron_axes_free(h, w->ck_un);
    if (w->sub) gpimhip_destroy(w->sub);
    if (w->subp) gpimhip_destroy(w->subp);
    if (w->subt) gpimhip_destroy(w->subt);
    delete w;
    h->sample = nullptr;
}

// ------------------------------------------------------------------------------------------
// What the draw drivers below (sample_enqueue, sample_pathwise_impl, sample_blocks_enqueue) need of a kernel family.  The
// vectors, the factorisations, the sweeps, the basis changes and the workspaces are shared; a family sets the parameters up,
// builds a dense or a reflection-block covariance, and applies K(G, X) -- and, where its mean is a constant c, centres y and
// shifts the results.  `ctx` is the context the launch runs on (its theta, its reflection state, its stream).
//   params       ctx->theta at u (var, noise, diag_add = the model's diagonal term s); `other`: the call's second diagonal
//                term (0 for the joint matrix, the draw's jitter d for the prior blocks), for a family that keeps it itself
//   kmat         lower tiles of K(X, X) (+ s I if model_diag), identity padding up to np
//   kmat_refl    block ctx->refl.pb_off of the grid's covariance on the fundamental domain, + s I if model_diag, else + the
//                other term (the stationary kernels read either from ctx->theta->diag_add, which the drivers set)
//   cross_apply  launch_pw_cross_apply (sample.hpp); Xt must be the rows of the latest kmat on ctx
//   reserve      the family's own buffers for dense rows / a fundamental domain / a grid of these (padded) sizes and n_y targets
//   centre       out = y - c;  shift: v += c   (null: a zero mean)
// ------------------------------------------------------------------------------------------
struct DrawFamily {
    int dim = 0;
    const gpimhip_model_t* m = nullptr;         // the stationary kernels of kfun.hpp
    const gpimhip_sm_t* sm = nullptr;           // the spectral mixture
    const double* u = nullptr;
    int (*params)(const DrawFamily&, gpimhip_ctx* ctx, double other) = nullptr;
    int (*kmat)(const DrawFamily&, gpimhip_ctx* ctx, const double* X, int64_t N, bool model_diag, double* out, int64_t ld,
                int64_t np) = nullptr;
    int (*kmat_refl)(const DrawFamily&, gpimhip_ctx* ctx, const double* Xq, int64_t Nq, bool model_diag, double* out, int64_t ld,
                     int64_t np) = nullptr;
    int (*cross_apply)(const DrawFamily&, gpimhip_ctx* ctx, const double* G, int64_t M, const double* Xt, int64_t N,
                       const double* Al, int64_t npt, int S, int s0, const double* g, const double* Z, int64_t zw, int64_t zn_off,
                       int noiseless, double* mean_out, double* out) = nullptr;
    int (*reserve)(const DrawFamily&, gpimhip_ctx* h, int64_t rows_x, int64_t rows_q, int64_t rows_g, int64_t n_y) = nullptr;
    int (*centre)(const DrawFamily&, gpimhip_ctx* ctx, const double* y, int64_t n, double* out) = nullptr;
    int (*shift)(const DrawFamily&, gpimhip_ctx* ctx, double* v, int64_t n) = nullptr;
    SampleWs* w = nullptr;                      // where reserve's buffers live (the model handle's)
};

static DrawFamily stationary_family(const gpimhip_model_t* m, const double* u) {
    DrawFamily F;
    F.dim = m->dim;
    F.m = m;
    F.u = u;
    F.params = [](const DrawFamily& F, gpimhip_ctx* c, double) { return launch_theta(c, F.m, F.u); };
    F.kmat = [](const DrawFamily& F, gpimhip_ctx* c, const double* X, int64_t N, bool model_diag, double* out, int64_t ld,
                int64_t np) {
        return launch_kmat(c, F.m, X, N, nullptr, N, c->theta, 0.0, model_diag ? 1 : 0, out, ld, np, np, 1, 1, 0, 0, 0);
    };
    F.kmat_refl = [](const DrawFamily& F, gpimhip_ctx* c, const double* Xq, int64_t Nq, bool, double* out, int64_t ld,
                     int64_t np) { return launch_kmat_refl(c, F.m, Xq, Nq, nullptr, Nq, c->theta, out, ld, np, np, 1, 0, 0, 0, 1.0); };
    F.cross_apply = [](const DrawFamily& F, gpimhip_ctx* c, const double* G, int64_t M, const double* Xt, int64_t N,
                       const double* Al, int64_t npt, int S, int s0, const double* g, const double* Z, int64_t zw, int64_t zn_off,
                       int noiseless, double* mean_out, double* out) {
        return launch_pw_cross_apply(c, F.m, G, M, Xt, N, c->theta, Al, npt, S, s0, g, Z, zw, zn_off, noiseless, mean_out, out);
    };
    return F;
}

// The spectral mixture: the phases of a build's points are computed right before it (O(points Q d) next to the build's
// O(points^2 Q d)); those of the dense rows stay in phx for cross_apply, which adds the phases of G once per call.
static DrawFamily sm_family(gpimhip_ctx* h, const gpimhip_sm_t* sm, const double* u) {
    DrawFamily F;
    F.dim = sm->dim;
    F.sm = sm;
    F.u = u;
    F.w = sws(h);
    F.reserve = [](const DrawFamily& F, gpimhip_ctx* h, int64_t rows_x, int64_t rows_q, int64_t rows_g, int64_t n_y) {
        const int64_t per = 2 * (int64_t)F.sm->mixtures * F.sm->dim;
        if (!F.w->smst) GP_TRY(F.w->smst.alloc(h, 2));
        GP_TRY(F.w->phx.grow(h, per * rows_x));
        GP_TRY(F.w->phq.grow(h, per * rows_q));
        GP_TRY(F.w->phg.grow(h, per * rows_g));
        return F.w->smy.grow(h, n_y);
    };
    F.params = [](const DrawFamily& F, gpimhip_ctx* c, double other) {
        return launch_sm_params(c, F.sm, F.u, F.w->smst, c->theta, other);
    };
    F.kmat = [](const DrawFamily& F, gpimhip_ctx* c, const double* X, int64_t N, bool model_diag, double* out, int64_t ld,
                int64_t np) {
        GP_TRY(launch_sm_setup(c, F.sm, F.u, X, N, np, F.w->phx, nullptr, nullptr, nullptr, nullptr));
        return launch_sm_kmat(c, F.sm, X, N, F.w->phx, np, nullptr, N, nullptr, np, F.w->smst + (model_diag ? 0 : 1), out, ld, np,
                              np, 1, 1);
    };
    F.kmat_refl = [](const DrawFamily& F, gpimhip_ctx* c, const double* Xq, int64_t Nq, bool model_diag, double* out, int64_t ld,
                     int64_t np) {
        GP_TRY(launch_sm_setup_refl(c, F.sm, F.u, Xq, Nq, np, F.w->phq, nullptr, nullptr, nullptr, nullptr, nullptr));
        return launch_sm_kmat_refl(c, F.sm, Xq, Nq, F.w->phq, np, nullptr, Nq, nullptr, np, F.w->smst + (model_diag ? 0 : 1), out,
                                   ld, 0, np, np, 1, 1, 1.0);
    };
    F.cross_apply = [](const DrawFamily& F, gpimhip_ctx* c, const double* G, int64_t M, const double* Xt, int64_t N,
                       const double* Al, int64_t npt, int S, int s0, const double* g, const double* Z, int64_t zw, int64_t zn_off,
                       int noiseless, double* mean_out, double* out) {
        const int64_t ldg = pad_to(M, NB);
        if (s0 == 0) GP_TRY(launch_sm_setup(c, F.sm, F.u, G, M, ldg, F.w->phg, nullptr, nullptr, nullptr, nullptr));
        return launch_sm_cross_apply(c, F.sm, G, M, F.w->phg, ldg, Xt, N, F.w->phx, npt, F.w->smst, c->theta, Al, npt, S, s0, g, Z,
                                     zw, zn_off, noiseless, mean_out, out);
    };
    F.centre = [](const DrawFamily& F, gpimhip_ctx* c, const double* y, int64_t n, double* out) {
        return launch_sm_centre(c, y, n, F.w->smst, out);
    };
    F.shift = [](const DrawFamily& F, gpimhip_ctx* c, double* v, int64_t n) { return launch_sm_addc(c, v, n, F.w->smst); };
    return F;
}
// y - c in the family's buffer when its mean is a constant (reserve has sized it), else y itself
static int centred(const DrawFamily& F, gpimhip_ctx* ctx, const double* y, int64_t n, const double** out) {
    *out = y;
    if (!F.centre) return GPIMHIP_OK;
    GP_TRY(F.centre(F, ctx, y, n, F.w->smy));
    *out = F.w->smy;
    return GPIMHIP_OK;
}

// zf = L^-1 r over the first nbr block rows of the factor L (r padded to them): block forward substitution, a panel of four
// blocks at a time against the inverted diagonal blocks the step schedule left in sub->dinv (distops.hip).
// t (order of the matrix): the running products L(rows, panels so far) zf; piece: 512.
static int forward_panels(gpimhip_ctx* sub, const double* L, int64_t ld, int nbr, const double* r, double* zf, double* t,
                          double* piece) {
    HIP_TRY(hipMemsetAsync(t, 0, (size_t)sub->np * sizeof(double), sub->stream));
    for (int g0 = 0; g0 < nbr; g0 += OUTER_W) {
        const int nblk = std::min(OUTER_W, nbr - g0), wd = nblk * NB;
        const int64_t r0 = (int64_t)g0 * NB;
        const double* P = L + r0 * ld + r0;
        GP_TRY(launch_dist_trsv(sub, P, ld, sub->dinv + (int64_t)g0 * NB * NB, nblk, 0, r + r0, t + r0, piece));
        HIP_TRY(hipMemcpyAsync(zf + r0, piece, (size_t)wd * sizeof(double), hipMemcpyDeviceToDevice, sub->stream));
        GP_TRY(launch_dist_rows_acc(sub, P + (int64_t)wd * ld, ld, (int64_t)nbr * NB - r0 - wd, wd, piece, t + r0 + wd));
    }
    return GPIMHIP_OK;
}

// sub->z = L11^-1 y from the factor L of the joint matrix: the block rows that hold training points.  The last of these may
// hold test points too: their entries of z are never read.
static int sample_forward(gpimhip_ctx* sub, const double* L, int64_t ld, const double* y, int64_t N, double* t, double* piece) {
    GP_TRY(launch_pad_copy(sub, y, N, sub->ypad, sub->np));
    return forward_panels(sub, L, ld, (int)((N + NB - 1) / NB), sub->ypad, sub->z, t, piece);
}

// (sample.hpp; see SampleWs)
int draw_sub(gpimhip_ctx* h, gpimhip_ctx** sub, int64_t order) {
    if (!*sub) GP_TRY(gpimhip_create(sub, h->device, h->stream));
    (*sub)->stream = h->stream;
    (*sub)->nbatch = 1;
    return ws_ensure_b(*sub, order, 1, 1, false);
}

// Everything of one draw call but the closing synchronisation.  theta_src (optional, device): the hyper-parameters, copied
// into the context's theta in place of the family's params -- a latent block of the multi-output model (variance
// lambda_t, noise 1, diag_add 1: sample_vgp_impl); the family's u is not read then.  reset_info: clear the context's status word first
// (a call of several blocks clears it once: the word keeps the first failure).
static int sample_enqueue(gpimhip_ctx* h, const DrawFamily& F, const double* X, const double* y, int64_t N,
                          const double* Xs, int64_t M, const double* Z, int S, int noiseless, double jitter_s, double* mean_out,
                          double* var_out, double* samples_out, const ThetaDev* theta_src, bool reset_info) {
    HIP_TRY(hipSetDevice(h->device));
    SampleWs* w = sws(h);
    const int64_t NM = N + M, d = F.dim;
    GP_TRY(draw_sub(h, &w->sub, NM));
    gpimhip_ctx* sub = w->sub;
    const int64_t np = sub->np, ld = sub->ld;
    GP_TRY(w->J.grow(h, np * ld));
    GP_TRY(w->XX.grow(h, np * GPIMHIP_MAX_DIM));
    GP_TRY(w->vec.grow(h, 2 * np + 4 * NB));
    if (F.reserve) GP_TRY(F.reserve(F, h, np, 0, 0, N));
    double *t = w->vec, *piece = t + np, *mean_ws = piece + 4 * NB;
    if (reset_info) HIP_TRY(hipMemsetAsync(sub->info, 0, sizeof(int32_t), h->stream));
    HIP_TRY(hipMemcpyAsync(w->XX, X, (size_t)(N * d) * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(w->XX + N * d, Xs, (size_t)(M * d) * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
    // J (lower tiles; identity padding at the end), the two diagonal terms, L
    // (stage timers of the model handle: 4 covariance build, 0 factorisation, 1 forward substitution, 5 each sweep of the draws)
    if (theta_src) HIP_TRY(hipMemcpyAsync(sub->theta, theta_src, sizeof(ThetaDev), hipMemcpyDeviceToDevice, h->stream));
    else GP_TRY(F.params(F, sub, 0.0));
    {
        StageTimer tm(h, 4);
        GP_TRY(F.kmat(F, sub, w->XX, NM, false, w->J, ld, np));
        GP_TRY(launch_sample_diag(sub, w->J, ld, N, M, sub->theta, noiseless, jitter_s));
    }
    { StageTimer tm(h, 0); GP_TRY(launch_potrf(sub, w->J, np, ld, sub->info)); }
    {
        StageTimer tm(h, 1);
        const double* yc;
        GP_TRY(centred(F, sub, y, N, &yc));
        GP_TRY(sample_forward(sub, w->J, ld, yc, N, t, piece));
    }
    for (int s0 = 0; s0 < S; s0 += sample_draw_group(S - s0)) {
        StageTimer tm(h, 5);
        GP_TRY(launch_sample_draws(sub, w->J, ld, N, M, sub->z, Z, S, s0, sub->theta, noiseless, jitter_s, mean_ws, mean_out,
                                   var_out, samples_out));
    }
    if (F.shift) {
        StageTimer tm(h, 5);
        if (mean_out) GP_TRY(F.shift(F, sub, mean_out, M));
        GP_TRY(F.shift(F, sub, samples_out, (int64_t)S * M));
    }
    return GPIMHIP_OK;
}
static int sample_impl(gpimhip_ctx* h, const DrawFamily& F, const double* X, const double* y, int64_t N,
                       const double* Xs, int64_t M, const double* Z, int S, int noiseless, double jitter_s, double* mean_out,
                       double* var_out, double* samples_out) {
    GP_TRY(sample_enqueue(h, F, X, y, N, Xs, M, Z, S, noiseless, jitter_s, mean_out, var_out, samples_out, nullptr, true));
    return finish_and_check(sws(h)->sub);
}

// ------------------------------------------------------------------------------------------
// pathwise draws: f_s = mean + g - (K_GX + d P)(K + s I)^-1 (g[idx] + sqrt(s - d) z_e), g a prior
// draw on the complete grid G through its 2^r reflection blocks.  The prior factor is shared by the S draws of a call.
// ------------------------------------------------------------------------------------------
// a = (L L^T)^-1 r for one padded vector r (np): the panel-wise substitutions of the distributed model (distops.hip) against
// the inverted diagonal blocks the step schedule left in sub->dinv.  zf, t: np; piece, work: 512.
static int pathwise_solve(gpimhip_ctx* sub, const double* L, int64_t ld, const double* r, double* a, double* zf, double* t,
                          double* piece, double* work) {
    const int64_t np = sub->np;
    const int nb = (int)(np / NB);
    GP_TRY(forward_panels(sub, L, ld, nb, r, zf, t, piece));
    for (int g0 = ((nb - 1) / OUTER_W) * OUTER_W; g0 >= 0; g0 -= OUTER_W) {
        const int nblk = std::min(OUTER_W, nb - g0), wd = nblk * NB;
        const int64_t r0 = (int64_t)g0 * NB, below = np - r0 - wd;
        const double* P = L + r0 * ld + r0;
        if (below > 0) GP_TRY(launch_gemv_t(sub, P + (int64_t)wd * ld, ld, below, wd, a + r0 + wd, work, 0, 0, 0, 0));
        else HIP_TRY(hipMemsetAsync(work, 0, (size_t)wd * sizeof(double), sub->stream));
        GP_TRY(launch_dist_trsv(sub, P, ld, sub->dinv + (int64_t)g0 * NB * NB, nblk, 1, zf + r0, work, piece));
        HIP_TRY(hipMemcpyAsync(a + r0, piece, (size_t)wd * sizeof(double), hipMemcpyDeviceToDevice, sub->stream));
    }
    return GPIMHIP_OK;
}

// ---- the prior draw on a grid through its B reflection blocks, shared by the pathwise, block and border drivers ----
// the reflection state of the prior's context: the B blocks of the grid of M points, unsharded
static void prior_refl(gpimhip_ctx* sp, const PwGrid& gd, const double* twoc, int64_t M, int B) {
    sp->refl.mask = gd.mask;
    for (int k = 0; k < GPIMHIP_MAX_DIM; ++k) sp->refl.twoc[k] = twoc[k];
    sp->refl.n_total = M;
    sp->refl.var_count = 0;
    sp->refl.pb_stride = 1;
    sp->refl.nblocks_total = B;
    sp->refl.raw = 0;
}
// block b is the one the next kmat_refl builds
static void prior_block(gpimhip_ctx* sp, int b, const double* wts, int64_t Nq) {
    sp->refl.pb_off = b;
    sp->refl.wts = wts + (int64_t)b * Nq;
}
// c_b = chol(K_b + d I) z_b for the S draws: the block's covariance in Pb (timer 4), its factor (0; status into `info`), the
// sweeps L_b z_p a group of draws at a time (5)
static int prior_block_draw(gpimhip_ctx* h, const DrawFamily& F, gpimhip_ctx* sp, const double* Xq, int64_t Nq, double* Pb,
                            int32_t* info, const double* Zb, int S, double* mean_ws, double* Cb) {
    const int64_t npq = sp->np, ldq = sp->ld;
    {
        StageTimer tm(h, 4);
        GP_TRY(F.kmat_refl(F, sp, Xq, Nq, false, Pb, ldq, npq));
    }
    { StageTimer tm(h, 0); GP_TRY(launch_potrf(sp, Pb, npq, ldq, info)); }
    for (int s0 = 0; s0 < S; s0 += sample_draw_group(S - s0)) {
        StageTimer tm(h, 5);
        GP_TRY(launch_sample_draws(sp, Pb, ldq, 0, Nq, nullptr, Zb, S, s0, sp->theta, 1, 0.0, mean_ws, nullptr, nullptr, Cb));
    }
    return GPIMHIP_OK;
}

// (stage timers of the model handle: 4 covariance builds, 0 factorisations, 5 the sweeps L_b z_p, 2 gathers and the
// basis change U^T, 1 the vector solves, 3 cross_apply_kernel with its epilogue)
static int sample_pathwise_impl(gpimhip_ctx* h, const DrawFamily& F, PwGrid gd, const double* twoc, const double* G,
                                int64_t M, const int64_t* idx, const double* y, int64_t N, const double* Z,
                                int S, int noiseless, double jitter_s, double* mean_out, double* samples_out) {
    HIP_TRY(hipSetDevice(h->device));
    SampleWs* w = sws(h);
    int64_t Nq = 1;
    for (int k = 0; k < gd.d; ++k) Nq *= gd.f[k];
    const int B = 1 << __builtin_popcount(gd.mask);
    GP_TRY(draw_sub(h, &w->subp, Nq));
    GP_TRY(draw_sub(h, &w->subt, N));
    gpimhip_ctx *sp = w->subp, *st = w->subt;
    const int64_t npq = sp->np, ldq = sp->ld, npt = st->np, ldt = st->ld;
    const int64_t zw = M + N + (noiseless ? 0 : M), SB = (int64_t)S * B;
    GP_TRY(w->Pb.grow(h, npq * ldq));
    GP_TRY(w->Kt.grow(h, npt * ldt));
    double *Xq, *wts, *Zg, *C, *g, *Xt, *R, *Al, *zf, *t, *piece, *work, *mean_ws;
    auto carve = [&](double* base) {
        Carve a(base);
        Xq = a.take(npq * GPIMHIP_MAX_DIM); wts = a.take(B * Nq); Zg = a.take(SB * Nq); C = a.take(SB * Nq);
        g = a.take((int64_t)S * M); Xt = a.take(npt * GPIMHIP_MAX_DIM); R = a.take((S + 1) * npt); Al = a.take((S + 1) * npt);
        zf = a.take(npt); t = a.take(npt); piece = a.take(4 * NB); work = a.take(4 * NB); mean_ws = a.take(npq);
        return a.used;
    };
    GP_TRY(w->pw.grow(h, carve(nullptr)));
    if (F.reserve) GP_TRY(F.reserve(F, h, npt, npq, pad_to(M, NB), N));
    carve(w->pw);
    // one status word for both factorisations: the training context's
    HIP_TRY(hipMemsetAsync(st->info, 0, sizeof(int32_t), h->stream));
    GP_TRY(F.params(F, sp, jitter_s));
    GP_TRY(launch_pw_set_diag(sp, sp->theta, jitter_s));
    GP_TRY(F.params(F, st, jitter_s));
    {
        StageTimer tm(h, 2);
        GP_TRY(launch_pw_setup(sp, gd, G, M, Nq, B, Xq, wts, idx, N, Xt));
        GP_TRY(launch_pw_gather_z(sp, gd, Z, zw, S, Nq, B, Zg));
    }
    // ---- the prior draw: block b of the grid's covariance, its factor, L_b z_b for every draw
    prior_refl(sp, gd, twoc, M, B);
    for (int b = 0; b < B; ++b) {
        prior_block(sp, b, wts, Nq);
        GP_TRY(prior_block_draw(h, F, sp, Xq, Nq, w->Pb, st->info, Zg + (int64_t)b * S * Nq, S, mean_ws, C + (int64_t)b * S * Nq));
    }
    { StageTimer tm(h, 2); GP_TRY(launch_pw_basis_t(sp, gd, C, S, Nq, B, M, g)); }
    // ---- the training side: K + (noise + jitter) I, its factor, alpha for the S draws and for y
    {
        StageTimer tm(h, 4);
        GP_TRY(F.kmat(F, st, Xt, N, true, w->Kt, ldt, npt));
    }
    { StageTimer tm(h, 0); GP_TRY(launch_potrf(st, w->Kt, npt, ldt, st->info)); }
    {
        StageTimer tm(h, 1);
        const double* yc;
        GP_TRY(centred(F, st, y, N, &yc));
        GP_TRY(launch_pw_rhs(st, g, M, idx, N, Z, zw, S, yc, st->theta, jitter_s, R, npt));
        for (int v = 0; v <= S; ++v)
            GP_TRY(pathwise_solve(st, w->Kt, ldt, R + (int64_t)v * npt, Al + (int64_t)v * npt, zf, t, piece, work));
    }
    {
        StageTimer tm(h, 3);
        for (int s0 = 0; s0 < S; s0 += sample_draw_group(S - s0))
            GP_TRY(F.cross_apply(F, st, G, M, Xt, N, Al, npt, S, s0, g, Z, zw, M + N, noiseless, mean_out, samples_out));
        GP_TRY(launch_pw_scatter(st, idx, N, M, Al, npt, S, jitter_s, samples_out));
    }
    return finish_and_check(st);
}

// ------------------------------------------------------------------------------------------
// draws on a fully observed grid: every step of the recipe above in the reflection basis, block by
// block -- no product with K_GX and no matrix of order N.  Pb holds chol(K_b + d I) until the prior draws c_b exist, then
// K_b + s I and its factor.
// ------------------------------------------------------------------------------------------
// A = (L L^T)^-1 R for ncols (1 .. 8) padded columns, column c at + c * cs: pathwise_solve for a group, the panel and the
// rows below it read once (distops.hip).  Zf: the forward results (columns of cs); t: ncols x np running products;
// part: gemv_t_multi_chunks(np) x 8 x 512.
static int blocks_solve(gpimhip_ctx* sub, const double* L, int64_t ld, const double* R, double* A, double* Zf, int64_t cs,
                        int ncols, double* t, double* part) {
    const int64_t np = sub->np;
    const int nb = (int)(np / NB);
    const int64_t pcs = 4 * NB, pchs = (int64_t)multi_group_width(ncols) * pcs;
    HIP_TRY(hipMemsetAsync(t, 0, (size_t)(ncols * np) * sizeof(double), sub->stream));
    for (int g0 = 0; g0 < nb; g0 += OUTER_W) {
        const int nblk = std::min(OUTER_W, nb - g0), wd = nblk * NB;
        const int64_t r0 = (int64_t)g0 * NB;
        const double* P = L + r0 * ld + r0;
        GP_TRY(launch_dist_trsv_multi(sub, P, ld, sub->dinv + (int64_t)g0 * NB * NB, nblk, 0, R + r0, cs, t + r0, np, 0, 1, ncols,
                                      Zf + r0, cs));
        GP_TRY(launch_dist_rows_acc_multi(sub, P + (int64_t)wd * ld, ld, np - r0 - wd, wd, Zf + r0, cs, ncols, t + r0 + wd, np));
    }
    for (int g0 = ((nb - 1) / OUTER_W) * OUTER_W; g0 >= 0; g0 -= OUTER_W) {
        const int nblk = std::min(OUTER_W, nb - g0), wd = nblk * NB;
        const int64_t r0 = (int64_t)g0 * NB, below = np - r0 - wd;
        const double* P = L + r0 * ld + r0;
        GP_TRY(launch_gemv_t_multi(sub, P + (int64_t)wd * ld, ld, below, wd, A + r0 + wd, cs, ncols, part));
        GP_TRY(launch_dist_trsv_multi(sub, P, ld, sub->dinv + (int64_t)g0 * NB * NB, nblk, 1, Zf + r0, cs, part, pcs, pchs,
                                      below > 0 ? gemv_t_multi_chunks(below) : 0, ncols, A + r0, cs));
    }
    return GPIMHIP_OK;
}

// (stage timers of the model handle, as sample_pathwise_impl: 4 covariance builds, 0 factorisations, 5 the sweeps L_b z_p,
// 2 gathers and both basis changes, 1 the multi-column solves, 3 right-hand sides, combination and epilogue)
// Everything of one call but the closing synchronisation.  theta_src / reset_info: as sample_enqueue; jitter_m: the model's
// own jitter of the diagonal K_b + (noise + jitter_m) I (m->jitter; 0 for a latent block of the multi-output model and for
// the spectral mixture).
static int sample_blocks_enqueue(gpimhip_ctx* h, const DrawFamily& F, PwGrid gd, const double* twoc, const double* G,
                                 int64_t M, const double* y, const double* Z, int S, int noiseless,
                                 double jitter_s, double* mean_out, double* samples_out, const ThetaDev* theta_src,
                                 double jitter_m, bool reset_info) {
    HIP_TRY(hipSetDevice(h->device));
    SampleWs* w = sws(h);
    int64_t Nq = 1;
    for (int k = 0; k < gd.d; ++k) Nq *= gd.f[k];
    const int B = 1 << __builtin_popcount(gd.mask);
    GP_TRY(draw_sub(h, &w->subp, Nq));
    gpimhip_ctx* sp = w->subp;
    const int64_t npq = sp->np, ldq = sp->ld;
    const int64_t zw = 2 * M + (noiseless ? 0 : M), SB = (int64_t)S * B, S1 = S + 1;
    GP_TRY(w->Pb.grow(h, npq * ldq));
    double *Xq, *wts, *Zg, *C, *E, *Cc, *g, *R, *Zf, *Al, *t, *part, *mean_ws;
    auto carve = [&](double* base) {
        Carve a(base);
        Xq = a.take(npq * GPIMHIP_MAX_DIM); wts = a.take(B * Nq); Zg = a.take(SB * Nq); C = a.take(SB * Nq);
        E = a.take(B * S1 * npq); Cc = a.take(B * S1 * Nq); g = a.take(S1 * M); R = a.take(S1 * npq); Zf = a.take(S1 * npq);
        Al = a.take(S1 * npq); t = a.take(8 * npq); part = a.take((int64_t)gemv_t_multi_chunks(npq) * 8 * 4 * NB);
        mean_ws = a.take(npq);
        return a.used;
    };
    GP_TRY(w->pw.grow(h, carve(nullptr)));
    if (F.reserve) GP_TRY(F.reserve(F, h, 0, npq, 0, M));
    carve(w->pw);
    // one status word for the 2 B factorisations
    if (reset_info) HIP_TRY(hipMemsetAsync(sp->info, 0, sizeof(int32_t), h->stream));
    if (theta_src) HIP_TRY(hipMemcpyAsync(sp->theta, theta_src, sizeof(ThetaDev), hipMemcpyDeviceToDevice, h->stream));
    else GP_TRY(F.params(F, sp, jitter_s));
    {
        StageTimer tm(h, 2);
        const double* yc;
        GP_TRY(centred(F, sp, y, M, &yc));
        GP_TRY(launch_pw_setup(sp, gd, G, M, Nq, B, Xq, wts, nullptr, 0, nullptr));
        GP_TRY(launch_pw_gather_z(sp, gd, Z, zw, S, Nq, B, Zg));
        GP_TRY(launch_pw_basis_fwd(sp, gd, Z, zw, M, yc, S, Nq, npq, B, E));
    }
    prior_refl(sp, gd, twoc, M, B);
    for (int b = 0; b < B; ++b) {
        prior_block(sp, b, wts, Nq);
        double *Cb = C + (int64_t)b * S * Nq, *Eb = E + (int64_t)b * S1 * npq;
        // ---- the prior draw c_b = chol(K_b + d I) z_b
        GP_TRY(launch_pw_set_diag(sp, sp->theta, jitter_s));
        GP_TRY(prior_block_draw(h, F, sp, Xq, Nq, w->Pb, sp->info, Zg + (int64_t)b * S * Nq, S, mean_ws, Cb));
        // ---- T_b = K_b + s I in the same buffer, its factor, [alpha_b | alpha_y,b] for the S draws and y
        GP_TRY(launch_pw_reset_diag(sp, sp->theta, jitter_m));
        {
            StageTimer tm(h, 4);
            GP_TRY(F.kmat_refl(F, sp, Xq, Nq, true, w->Pb, ldq, npq));
        }
        { StageTimer tm(h, 0); GP_TRY(launch_potrf(sp, w->Pb, npq, ldq, sp->info)); }
        { StageTimer tm(h, 3); GP_TRY(launch_pw_blocks_rhs(sp, Cb, Eb, S, Nq, npq, sp->theta, jitter_s, R)); }
        {
            StageTimer tm(h, 1);
            for (int c0 = 0; c0 <= S; c0 += sample_draw_group(S + 1 - c0)) {
                const int64_t off = (int64_t)c0 * npq;
                GP_TRY(blocks_solve(sp, w->Pb, ldq, R + off, Al + off, Zf + off, npq, sample_draw_group(S + 1 - c0), t, part));
            }
        }
        {
            StageTimer tm(h, 3);
            GP_TRY(launch_pw_blocks_combine(sp, Al, Eb, S, Nq, npq, sp->theta, jitter_s, Cc + (int64_t)b * S1 * Nq));
        }
    }
    { StageTimer tm(h, 2); GP_TRY(launch_pw_basis_t(sp, gd, Cc, S + 1, Nq, B, M, g)); }
    {
        StageTimer tm(h, 3);
        GP_TRY(launch_pw_blocks_out(sp, g, M, S, Z, zw, 2 * M, noiseless, sp->theta, mean_out, samples_out));
        if (F.shift) {
            if (mean_out) GP_TRY(F.shift(F, sp, mean_out, M));
            GP_TRY(F.shift(F, sp, samples_out, (int64_t)S * M));
        }
    }
    return GPIMHIP_OK;
}
// jitter_m: the model's own jitter (m->jitter; the spectral mixture has none)
static int sample_blocks_impl(gpimhip_ctx* h, const DrawFamily& F, PwGrid gd, const double* twoc, const double* G,
                              int64_t M, const double* y, const double* Z, int S, int noiseless,
                              double jitter_s, double jitter_m, double* mean_out, double* samples_out) {
    GP_TRY(sample_blocks_enqueue(h, F, gd, twoc, G, M, y, Z, S, noiseless, jitter_s, mean_out, samples_out, nullptr, jitter_m,
                                 true));
    return finish_and_check(sws(h)->subp);
}

// ------------------------------------------------------------------------------------------
// joint draws of the multi-output GP.  The reduction of section 9 diagonalises the posterior too: the
// whitened, rotated latent functions h_t = sum_a Q_at s_a^-1/2 f_a are independent GPs with kernel lambda_t K, observed with
// unit noise through z_t, so a joint draw of the T outputs is one single-output draw per latent block, mixed back:
//   f_a = mu_a + s_a^1/2 sum_t Q_at h_t          (vgp.hip: vgp_sample_mix_kernel)
// The blocks run one after the other through the single-output drivers above and the one matrix those own (J, or Pb): the
// large allocation is that of a single-output call at the same sizes.  One status word, one synchronisation.
// (stage timers of the model handle: those of the single-output driver, summed over the T blocks, and 6 = the mix kernel;
// the joint route also records 2 = setup and projection, 3 = the mix of mean and variance)
// ------------------------------------------------------------------------------------------
static int sample_vgp_ws(gpimhip_ctx* h, int T, int64_t N, int64_t M, int S, SampleWs** out) {
    SampleWs* w = sws(h);
    if (!w->vst) GP_TRY(w->vst.alloc(h, 1));
    if (!w->vth) GP_TRY(w->vth.alloc(h, VGP_MAXT));
    GP_TRY(w->vz.grow(h, (int64_t)T * N));
    GP_TRY(w->vH.grow(h, (int64_t)T * S * M));
    GP_TRY(w->vmom.grow(h, 2 * (int64_t)T * M));
    *out = w;
    return GPIMHIP_OK;
}

static int sample_vgp_impl(gpimhip_ctx* h, const gpimhip_model_t* m, const gpimhip_vgp_t* vg, const double* X, const double* Y,
                           int64_t N, const double* u, const double* Xs, int64_t M, const double* Z, int S, int noiseless,
                           double jitter_s, double* mean_out, double* var_out, double* samples_out) {
    HIP_TRY(hipSetDevice(h->device));
    const int T = vg->tasks;
    SampleWs* w = nullptr;
    GP_TRY(sample_vgp_ws(h, T, N, M, S, &w));
    double *mblk = w->vmom, *vblk = w->vmom + (int64_t)T * M;
    {
        StageTimer tm(h, 2);
        GP_TRY(launch_vgp_setup_to(h, m, vg, u, w->vst, w->vth));
        GP_TRY(launch_vgp_project_to(h, Y, N, T, w->vst, w->vz));
    }
    const DrawFamily F = stationary_family(m, nullptr);         // (every block's theta comes from vth)
    for (int t = 0; t < T; ++t)
        GP_TRY(sample_enqueue(h, F, X, w->vz + (int64_t)t * N, N, Xs, M, Z + (int64_t)t * S * M, S, noiseless, jitter_s,
                              mean_out ? mblk + (int64_t)t * M : nullptr, var_out ? vblk + (int64_t)t * M : nullptr,
                              w->vH + (int64_t)t * S * M, w->vth + t, t == 0));
    { StageTimer tm(h, 6); GP_TRY(launch_vgp_sample_mix(h, T, S, M, w->vst, w->vH, samples_out)); }
    if (mean_out || var_out) {
        StageTimer tm(h, 3);
        GP_TRY(launch_vgp_combine(h, T, M, w->vst, mblk, vblk, mean_out, var_out));
    }
    return finish_and_check(w->sub);
}

static int sample_vgp_blocks_impl(gpimhip_ctx* h, const gpimhip_model_t* m, const gpimhip_vgp_t* vg, PwGrid gd,
                                  const double* twoc, const double* G, int64_t M, const double* Y, const double* u,
                                  const double* Z, int S, int noiseless, double jitter_s, double* mean_out,
                                  double* samples_out) {
    HIP_TRY(hipSetDevice(h->device));
    const int T = vg->tasks;
    SampleWs* w = nullptr;
    GP_TRY(sample_vgp_ws(h, T, M, M, S, &w));
    const int64_t zw = 2 * M + (noiseless ? 0 : M);
    GP_TRY(launch_vgp_setup_to(h, m, vg, u, w->vst, w->vth));
    GP_TRY(launch_vgp_project_to(h, Y, M, T, w->vst, w->vz));
    const DrawFamily F = stationary_family(m, nullptr);         // (every block's theta comes from vth)
    for (int t = 0; t < T; ++t)
        GP_TRY(sample_blocks_enqueue(h, F, gd, twoc, G, M, w->vz + (int64_t)t * M, Z + (int64_t)t * S * zw, S, noiseless,
                                     jitter_s, mean_out ? w->vmom + (int64_t)t * M : nullptr, w->vH + (int64_t)t * S * M,
                                     w->vth + t, 0.0, t == 0));
    { StageTimer tm(h, 6); GP_TRY(launch_vgp_sample_mix(h, T, S, M, w->vst, w->vH, samples_out)); }
    if (mean_out) GP_TRY(launch_vgp_combine(h, T, M, w->vst, w->vmom, nullptr, mean_out, nullptr));
    return finish_and_check(w->subp);
}

// ------------------------------------------------------------------------------------------
// draws on a grid with missing points: the recipe of section 17 with the bordered blocks of the model
// in place of a second factorisation per block.  With A = K_GG + s I on the completed grid, V = A^-1 P_m, S = P_m^T V:
//   beta = A^-1 [r~ | y~],  w = S^-1 beta_m,  alpha~ = beta - V w      ((K_oo + s I)^-1 embedded: zero at the missing points)
//   p = (s - d) alpha~ - sqrt(s - d) z_e at the observed points, g + w at the missing ones;  mean = y - s alpha~_y, -w_y
// Everything A^-1, S^-1 and V need is what a prediction leaves: L_b^-1 in h->A, L_S^-1 in the border's sub->A, Y_b = C_b L_S^-T.
// Beyond that state: one np x ld block (SampleWs::Pb, the prior factors one after the other) and vectors.
// (stage timers of the model handle: 4 the prior's covariance builds, 0 factorisations with the inverses their launches
// host, 5 the sweeps L_b z_p, 2 gathers and the basis changes, 1 the multi-column sweeps through L_b^-1 and what is left of
// the triangular inverses, 6 those sweeps alone (intervals inside stage 1's), 3 right-hand sides, the border's vectors,
// combination and epilogue; the model's covariance build, its K^-1 product and the products of border_iter are not timed,
// as in a prediction)
// ------------------------------------------------------------------------------------------
static int sample_border_impl(gpimhip_ctx* h, const gpimhip_model_t* m, const double* X, int64_t x_bs, const double* ys,
                              int64_t Nq, int B, const double* u, PwGrid gd, const double* twoc, const double* G, int64_t M,
                              const int64_t* miss, const double* Z, int S, int noiseless, double jitter_s, double* mean_out,
                              double* samples_out) {
    HIP_TRY(hipSetDevice(h->device));
    SampleWs* w = sws(h);
    GP_TRY(draw_sub(h, &w->subp, Nq));
    gpimhip_ctx* sp = w->subp;
    const int64_t npq = sp->np, ldq = sp->ld;
    const int64_t zw = 2 * M + (noiseless ? 0 : M), SB = (int64_t)S * B, S1 = S + 1;
    const int Mm = bws(h)->M;
    const int64_t mp = pad_to(Mm, NB);
    GP_TRY(w->Pb.grow(h, npq * ldq));
    const int pg = sample_draw_group(S + 1);           // the first group of columns is the largest
    const int64_t n_part = std::max((int64_t)B * tri_bwd_chunks(npq) * pg * npq, (int64_t)tri_bwd_chunks(mp) * pg * mp);
    double *Xq, *wts, *Zg, *C, *g, *mean_ws, *R, *Zf, *Cc, *g2, *tv, *part;
    int32_t* mi;
    auto carve = [&](double* base) {
        Carve a(base);
        Xq = a.take(npq * GPIMHIP_MAX_DIM); wts = a.take(B * Nq); Zg = a.take(SB * Nq); C = a.take(SB * Nq);
        g = a.take((int64_t)S * M); mean_ws = a.take(npq); R = a.take(B * S1 * npq); Zf = a.take(B * S1 * npq);
        Cc = a.take(B * S1 * Nq); g2 = a.take(S1 * M); tv = a.take(3 * S1 * mp); part = a.take(n_part);
        mi = a.take<int32_t>((M + 1) / 2);
        return a.used;
    };
    GP_TRY(w->pw.grow(h, carve(nullptr)));
    carve(w->pw);
    double *vv = tv + S1 * mp, *wv = vv + S1 * mp;
    const DrawFamily F = stationary_family(m, u);
    // ---- the prior draws c_b = chol(K_b + d I) z_b block by block through Pb (sample_blocks_impl), g = U^T c
    HIP_TRY(hipMemsetAsync(sp->info, 0, sizeof(int32_t), h->stream));
    GP_TRY(launch_theta(sp, m, u));
    GP_TRY(launch_pw_set_diag(sp, sp->theta, jitter_s));
    {
        StageTimer tm(h, 2);
        GP_TRY(launch_pw_setup(sp, gd, G, M, Nq, B, Xq, wts, nullptr, 0, nullptr));
        GP_TRY(launch_pw_gather_z(sp, gd, Z, zw, S, Nq, B, Zg));
        GP_TRY(launch_bs_mark(sp, miss, Mm, M, mi));
    }
    prior_refl(sp, gd, twoc, M, B);
    for (int b = 0; b < B; ++b) {
        prior_block(sp, b, wts, Nq);
        GP_TRY(prior_block_draw(h, F, sp, Xq, Nq, w->Pb, sp->info, Zg + (int64_t)b * S * Nq, S, mean_ws, C + (int64_t)b * S * Nq));
    }
    { StageTimer tm(h, 2); GP_TRY(launch_pw_basis_t(sp, gd, C, S, Nq, B, M, g)); }
    // ---- the model's state: L_b^-1, B_b^-1, S, L_S^-1, Y_b (every factorisation reports through h->info)
    GP_TRY(model_state_at_u(h, m, X, x_bs, ys, Nq, B, u));
    GP_TRY(launch_bs_merge_info(h, sp->info, h->info));
    BorderWs* bw = bws(h);
    const int64_t np = h->np, ld = h->ld;
    if (np != npq || sp->stream != h->stream) {         // the vectors above are sized by the prior's context and indexed by the model's
        gpim_set_error("gpimhip_sample_border: the prior's context and the model's workspace disagree on the padded block order "
                       "or on the stream");
        return GPIMHIP_E_BADARG;
    }
    const double *Ls = bw->sub->A;
    const int64_t lds = bw->sub->ld;
    // ---- right-hand sides in the blocks: [U r~ | ys]; what the sweeps leave untouched (padding rows) is zero
    HIP_TRY(hipMemsetAsync(Zf, 0, (size_t)(B * S1 * np) * sizeof(double), h->stream));
    HIP_TRY(hipMemsetAsync(tv, 0, (size_t)(3 * S1 * mp) * sizeof(double), h->stream));
    {
        StageTimer tm(h, 3);
        GP_TRY(launch_bs_rhs_fwd(h, gd, g, Z, zw, M, mi, ys, h->theta, jitter_s, S, Nq, np, B, R));
    }
    // ---- beta_b = L_b^-T (L_b^-1 R_b), a group of columns per pass over the triangles (beta overwrites R)
    {
        StageTimer tm(h, 1);
        for (int c0 = 0; c0 <= S; c0 += sample_draw_group(S + 1 - c0)) {
            const int nc = sample_draw_group(S + 1 - c0);
            const int64_t off = (int64_t)c0 * np;
            StageTimer ts(h, 6);                        // (the two sweeps alone: stage 1 also holds the rest of the inverses)
            GP_TRY(launch_tri_fwd_multi(h, h->A, ld, np * ld, Nq, B, R + off, Zf + off, np, S1 * np, nc));
            GP_TRY(launch_tri_bwd_multi(h, h->A, ld, np * ld, Nq, np, B, Zf + off, R + off, np, S1 * np, nc, part, pg));
        }
    }
    // ---- the border: t = beta_m, v = L_S^-1 t, w = L_S^-T v, alpha~_b = beta_b - Y_b v
    {
        StageTimer tm(h, 3);
        GP_TRY(launch_bs_t(h, R, np, B, (int)S1, bw->q, bw->coef, Mm, mp, tv));
        for (int c0 = 0; c0 <= S; c0 += sample_draw_group(S + 1 - c0)) {
            const int nc = sample_draw_group(S + 1 - c0);
            const int64_t off = (int64_t)c0 * mp;
            GP_TRY(launch_tri_fwd_multi(h, Ls, lds, 0, Mm, 1, tv + off, vv + off, mp, 0, nc));
            GP_TRY(launch_tri_bwd_multi(h, Ls, lds, 0, Mm, mp, 1, vv + off, wv + off, mp, 0, nc, part, pg));
            GP_TRY(launch_bs_yv(h, bw->Y, mp, np, Nq, B, (int)S1, vv, c0, nc, R));
        }
        GP_TRY(launch_bs_combine(h, R, ys, S, Nq, np, B, h->theta, jitter_s, Cc));
    }
    { StageTimer tm(h, 2); GP_TRY(launch_pw_basis_t(h, gd, Cc, S + 1, Nq, B, M, g2)); }
    {
        StageTimer tm(h, 3);
        GP_TRY(launch_bs_out(h, g2, g, wv, mp, mi, M, S, Z, zw, noiseless, h->theta, jitter_s, mean_out, samples_out));
    }
    return finish_and_check(h);
}

// the grid of a pathwise or block draw from its shape and reflected axes; M = its points (0: a bad argument)
static int64_t pw_grid(int dim, const int32_t* shape, int32_t mask, PwGrid* gd) {
    gd->d = dim;
    gd->mask = mask;
    int64_t M = 1;
    for (int k = 0; k < GPIMHIP_MAX_DIM; ++k) {
        gd->n[k] = k < dim ? shape[k] : 1;
        if (gd->n[k] < 1) return 0;
        const bool refl = (mask >> k) & 1;
        if (refl && (k >= dim || gd->n[k] < 2)) return 0;
        gd->f[k] = refl ? (gd->n[k] + 1) / 2 : gd->n[k];
        M *= gd->n[k];
        if (M > ((int64_t)1 << 31)) return 0;
    }
    return M;
}
// the gate of the entries that draw through the reflection blocks of a grid of their own: *M = its points
static int draw_grid(const char* entry, int dim, const int32_t* shape, int32_t mask, PwGrid* gd, int64_t* M) {
    *M = pw_grid(dim, shape, mask, gd);
    if (*M < 1) return GPIMHIP_E_BADARG;
    if (!mask || (mask >> dim)) {
        gpim_set_error(std::string(entry) + ": needs at least one reflected axis of the grid");
        return GPIMHIP_E_BADARG;
    }
    return GPIMHIP_OK;
}

extern "C" {

int gpimhip_sample_blocks(gpimhip_handle h, const gpimhip_model_t* m, const double* G, const int32_t* shape, int32_t mask,
                          const double* twoc, const double* y, const double* u, const double* Z, int32_t S, int32_t noiseless,
                          double jitter, double* mean_out, double* samples_out) {
    FP64_ONLY(h);
    if (!h || !G || !shape || !twoc || !y || !u || !Z || !samples_out || S < 1 || S > 65534 || !(jitter > 0.0))
        return GPIMHIP_E_BADARG;
    GP_TRY(check_model(m));
    if (h->refl.mask) {
        gpim_set_error("gpimhip_sample_blocks: not available in reflection mode (the dense double-precision engine only)");
        return GPIMHIP_E_BADARG;
    }
    PwGrid gd;
    int64_t M;
    GP_TRY(draw_grid("gpimhip_sample_blocks", m->dim, shape, mask, &gd, &M));
    return sample_blocks_impl(h, stationary_family(m, u), gd, twoc, G, M, y, Z, S, noiseless ? 1 : 0, jitter, m->jitter, mean_out,
                              samples_out);
}

int gpimhip_sample_vgp(gpimhip_handle h, const gpimhip_model_t* m, const gpimhip_vgp_t* vg, const double* X, const double* Y,
                       int64_t N, const double* u, const double* Xs, int64_t M, const double* Z, int32_t S, int32_t noiseless,
                       double jitter, double* mean_out, double* var_out, double* samples_out) {
    GP_TRY(vgp_check(h, m, vg, X, Y, N));
    if (!u || !Xs || !Z || !samples_out || M < 1 || S < 1 || S > 65534 || !(jitter > 0.0)) return GPIMHIP_E_BADARG;
    if (h->refl.mask) {
        gpim_set_error("gpimhip_sample_vgp: not available in reflection mode (the observed rows X, Y of the dense model; "
                       "gpimhip_set_reflection(h, 0, ...))");
        return GPIMHIP_E_BADARG;
    }
    return sample_vgp_impl(h, m, vg, X, Y, N, u, Xs, M, Z, S, noiseless ? 1 : 0, jitter, mean_out, var_out, samples_out);
}

int gpimhip_sample_vgp_blocks(gpimhip_handle h, const gpimhip_model_t* m, const gpimhip_vgp_t* vg, const double* G,
                              const int32_t* shape, int32_t mask, const double* twoc, const double* Y, const double* u,
                              const double* Z, int32_t S, int32_t noiseless, double jitter, double* mean_out,
                              double* samples_out) {
    if (!shape || !twoc) return GPIMHIP_E_BADARG;
    GP_TRY(vgp_check(h, m, vg, G, Y, 1));
    if (!u || !Z || !samples_out || S < 1 || S > 65534 || !(jitter > 0.0)) return GPIMHIP_E_BADARG;
    if (jitter > 1.0) {
        gpim_set_error("gpimhip_sample_vgp_blocks: needs 0 < jitter <= 1 (block units: the latent blocks have unit noise)");
        return GPIMHIP_E_BADARG;
    }
    if (h->refl.mask) {
        gpim_set_error("gpimhip_sample_vgp_blocks: not available in reflection mode (the grid G and the rows Y of the dense "
                       "model; gpimhip_set_reflection(h, 0, ...))");
        return GPIMHIP_E_BADARG;
    }
    PwGrid gd;
    int64_t M;
    GP_TRY(draw_grid("gpimhip_sample_vgp_blocks", m->dim, shape, mask, &gd, &M));
    return sample_vgp_blocks_impl(h, m, vg, gd, twoc, G, M, Y, u, Z, S, noiseless ? 1 : 0, jitter, mean_out, samples_out);
}

int gpimhip_sample_border(gpimhip_handle h, const gpimhip_model_t* m, const double* X, int64_t x_stride, const double* y,
                          int64_t N, int32_t B, const double* u, const double* G, const int32_t* shape, int32_t mask,
                          const double* twoc, const int64_t* miss, const double* Z, int32_t S, int32_t noiseless, double jitter,
                          double* mean_out, double* samples_out) {
    FP64_ONLY(h);
    if (!h || !X || !y || !u || !G || !shape || !twoc || !miss || !Z || !samples_out || N < 1 || B < 1 ||
        B > (1 << GPIMHIP_MAX_DIM) || S < 1 || S > 65534 || !(jitter > 0.0))
        return GPIMHIP_E_BADARG;
    GP_TRY(check_model(m));
    if (!h->refl.mask) {
        gpim_set_error("gpimhip_sample_border: needs reflection mode (gpimhip_set_reflection) with a border (gpimhip_set_border)");
        return GPIMHIP_E_BADARG;
    }
    if (!border_on(h)) {
        gpim_set_error("gpimhip_sample_border: no border is set (no missing points: gpimhip_sample_blocks draws on a fully "
                       "observed grid)");
        return GPIMHIP_E_BADARG;
    }
    // (BorderWs::T > 1 can only come from a batch of T 2^r problems: this entry sets one border up, whatever ran before)
    if (mask > 0 && mask < (1 << GPIMHIP_MAX_DIM) && B > (1 << __builtin_popcount(mask)) && B % (1 << __builtin_popcount(mask)) == 0) {
        gpim_set_error("gpimhip_sample_border: a multi-output border (B = T 2^r problems, one border per task) is not built: the "
                       "entry takes the 2^r blocks of one model");
        return GPIMHIP_E_BADARG;
    }
    PwGrid gd;
    const int64_t M = pw_grid(m->dim, shape, mask, &gd);
    int64_t Nq = M < 1 ? 0 : 1;
    for (int k = 0; k < GPIMHIP_MAX_DIM && M >= 1; ++k) Nq *= gd.f[k];
    if (M < 1 || mask != h->refl.mask || (mask >> m->dim) || B != (1 << __builtin_popcount(mask)) || Nq != N ||
        bws(h)->M >= M || h->refl.pb_stride != 1 || h->refl.raw) {
        gpim_set_error("gpimhip_sample_border: the grid (shape, mask) does not describe the handle's reflection blocks (mask, "
                       "B = 2^r, N = the points of the fundamental domain, fewer missing points than grid points, unsharded)");
        return GPIMHIP_E_BADARG;
    }
    return sample_border_impl(h, m, X, x_stride, y, N, B, u, gd, twoc, G, M, miss, Z, S, noiseless ? 1 : 0, jitter, mean_out,
                              samples_out);
}

int gpimhip_sample_pathwise(gpimhip_handle h, const gpimhip_model_t* m, const double* G, const int32_t* shape, int32_t mask,
                            const double* twoc, const int64_t* idx, const double* y, int64_t N, const double* u,
                            const double* Z, int32_t S, int32_t noiseless, double jitter, double* mean_out,
                            double* samples_out) {
    FP64_ONLY(h);
    if (!h || !G || !shape || !twoc || !idx || !y || !u || !Z || !samples_out || N < 1 || S < 1 || S > 65535 || !(jitter > 0.0))
        return GPIMHIP_E_BADARG;
    GP_TRY(check_model(m));
    if (h->refl.mask) {
        gpim_set_error("gpimhip_sample_pathwise: not available in reflection mode (the dense double-precision engine only)");
        return GPIMHIP_E_BADARG;
    }
    PwGrid gd;
    int64_t M;
    GP_TRY(draw_grid("gpimhip_sample_pathwise", m->dim, shape, mask, &gd, &M));
    return sample_pathwise_impl(h, stationary_family(m, u), gd, twoc, G, M, idx, y, N, Z, S, noiseless ? 1 : 0, jitter, mean_out,
                                samples_out);
}

int gpimhip_sample_exact(gpimhip_handle h, const gpimhip_model_t* m, const double* X, const double* y, int64_t N,
                         const double* u, const double* Xs, int64_t M, const double* Z, int32_t S, int32_t noiseless,
                         double jitter, double* mean_out, double* var_out, double* samples_out) {
    FP64_ONLY(h);
    if (!h || !X || !y || !u || !Xs || !Z || !samples_out || N < 1 || M < 1 || S < 1 || !(jitter >= 0.0))
        return GPIMHIP_E_BADARG;
    GP_TRY(check_model(m));
    if (h->refl.mask) {
        gpim_set_error("gpimhip_sample_exact: not available in reflection mode (the dense double-precision engine only)");
        return GPIMHIP_E_BADARG;
    }
    return sample_impl(h, stationary_family(m, u), X, y, N, Xs, M, Z, S, noiseless ? 1 : 0, jitter, mean_out, var_out, samples_out);
}

// ---- the same three draws for the spectral-mixture model: the drivers above with sm_family.  sm_check
// refuses a handle in reflection mode, as the entries above do.
int gpimhip_sample_sm(gpimhip_handle h, const gpimhip_sm_t* sm, const double* X, const double* y, int64_t N, const double* u,
                      const double* Xs, int64_t M, const double* Z, int32_t S, int32_t noiseless, double jitter,
                      double* mean_out, double* var_out, double* samples_out) {
    GP_TRY(sm_check(h, sm, X, N));
    if (!y || !u || !Xs || !Z || !samples_out || M < 1 || S < 1 || !(jitter >= 0.0)) return GPIMHIP_E_BADARG;
    return sample_impl(h, sm_family(h, sm, u), X, y, N, Xs, M, Z, S, noiseless ? 1 : 0, jitter, mean_out, var_out, samples_out);
}

int gpimhip_sample_sm_pathwise(gpimhip_handle h, const gpimhip_sm_t* sm, const double* G, const int32_t* shape, int32_t mask,
                               const double* twoc, const int64_t* idx, const double* y, int64_t N, const double* u,
                               const double* Z, int32_t S, int32_t noiseless, double jitter, double* mean_out,
                               double* samples_out) {
    GP_TRY(sm_check(h, sm, G, N));
    if (!shape || !twoc || !idx || !y || !u || !Z || !samples_out || S < 1 || S > 65535 || !(jitter > 0.0)) return GPIMHIP_E_BADARG;
    PwGrid gd;
    int64_t M;
    GP_TRY(draw_grid("gpimhip_sample_sm_pathwise", sm->dim, shape, mask, &gd, &M));
    return sample_pathwise_impl(h, sm_family(h, sm, u), gd, twoc, G, M, idx, y, N, Z, S, noiseless ? 1 : 0, jitter, mean_out,
                                samples_out);
}

int gpimhip_sample_sm_blocks(gpimhip_handle h, const gpimhip_sm_t* sm, const double* G, const int32_t* shape, int32_t mask,
                             const double* twoc, const double* y, const double* u, const double* Z, int32_t S, int32_t noiseless,
                             double jitter, double* mean_out, double* samples_out) {
    GP_TRY(sm_check(h, sm, G, 1));
    if (!shape || !twoc || !y || !u || !Z || !samples_out || S < 1 || S > 65534 || !(jitter > 0.0)) return GPIMHIP_E_BADARG;
    PwGrid gd;
    int64_t M;
    GP_TRY(draw_grid("gpimhip_sample_sm_blocks", sm->dim, shape, mask, &gd, &M));
    return sample_blocks_impl(h, sm_family(h, sm, u), gd, twoc, G, M, y, Z, S, noiseless ? 1 : 0, jitter, 0.0, mean_out, samples_out);
}

}  // extern "C"
