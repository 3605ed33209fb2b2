// pkrongp.hip -- host drivers of the dense-by-Kronecker blocks (gpimhip_pkron_nll_grad / gpimhip_fit_pkron /
// gpimhip_predict_pkron, DESIGN.md section 22, and the posterior draws gpimhip_sample_pkron, section 23): a grid whose missing
// points are whole columns.  J = prod n_i blocks s2 lambda_j K_s + sigma I of the N_s observed ragged points run in lock-step
// through the batched engine (B = J, shared X_s); the complete axes are a KronAxes set of kron.hip.  Host code only: the
// kernels and their launchers are in pkron.hip, the per-axis drivers in kron.hip, the engine's drivers (workspaces,
// factorisation, tile engine, training loop) in api.hip.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include "common.hpp"
#include "pkron.hpp"
#include "sample.hpp"

void pkron_release(gpimhip_ctx* h) {
    PkronWs* w = (PkronWs*)h->pkron;
    if (!w) return;
    kron_axes_free(h, w->ax);
    dev_release(h, w->th3, w->lamj, w->yt, w->Ks, w->Bp, w->W, w->Z, w->bsum, w->colpart, w->G, w->Q, w->pp, w->cross);
    delete w;
    h->pkron = nullptr;
}
static int pkron_bad(const char* what) {
    gpim_set_error(std::string("dense-by-Kronecker blocks: ") + what);
    return GPIMHIP_E_BADARG;
}
static int pkron_check(gpimhip_ctx* h, const gpimhip_model_t* m, const double* Xs, int64_t Ns, int32_t p, int32_t dc,
                       const int32_t* n_c, const int32_t* perm, const double* axes_c, const double* Y, PkronMap* mp) {
    if (!h || !m || !Xs || !n_c || !axes_c || !Y || Ns < 1) return GPIMHIP_E_BADARG;
    FP64_ONLY(h);
    GP_TRY(check_model(m));
    if (m->kernel != GPIMHIP_KERNEL_RBF) return pkron_bad("only the RBF kernel factorises over the complete axes");
    if (h->refl.mask) return pkron_bad("the handle is in reflection mode (gpimhip_set_reflection(h, 0, ...) first)");
    if (p < 1 || dc < 1 || p + dc != m->dim) return pkron_bad("needs p >= 1 ragged and dc >= 1 complete axes with p + dc = dim");
    memset(mp, 0, sizeof(*mp));
    mp->p = p; mp->dc = dc;
    int64_t J = 1;
    int seen = 0;
    for (int k = 0; k < m->dim; ++k) {
        const int a = perm ? perm[k] : k;
        if (a < 0 || a >= m->dim || (seen >> a & 1)) return pkron_bad("perm is not a permutation of the model's axes");
        seen |= 1 << a;
        mp->perm[k] = a;
    }
    for (int i = 0; i < dc; ++i) {
        if (n_c[i] < 1 || n_c[i] > 4096) return pkron_bad("a complete axis takes 1 .. 4096 points (the eigen-solver's limit)");
        mp->nc[i] = n_c[i];
        J *= n_c[i];
        if (J > 65535) return pkron_bad("more than 65535 blocks (the batched engine's cap)");
    }
    mp->J = (int)J;
    return GPIMHIP_OK;
}
static int pkron_begin(gpimhip_ctx* h, const PkronMap& mp, const int32_t* n_c, const double* axes_c, int64_t Ns, PkronWs** out) {
    HIP_TRY(hipSetDevice(h->device));
    h->nbatch = mp.J;
    HIP_TRY(hipMemsetAsync(h->info, 0, sizeof(int32_t), h->stream));
    GP_TRY(ws_ensure_padded(h, Ns));
    PkronWs* w = (PkronWs*)h->pkron;
    if (!w) {
        w = new PkronWs();
        h->pkron = w;
        GP_TRY(w->th3.alloc(h, 3));
    }
    const int64_t np = h->np, J = mp.J, Jp = pad_to(J, NB);
    GP_TRY(w->lamj.grow(h, J));
    GP_TRY(w->yt.grow(h, 2 * Ns * J));
    GP_TRY(w->Ks.grow(h, np * h->ld));
    GP_TRY(w->Bp.grow(h, Jp * np));
    GP_TRY(w->W.grow(h, Jp * np));
    GP_TRY(w->Z.grow(h, (int64_t)mp.dc * J * np));
    GP_TRY(w->bsum.grow(h, J * PK_SUMS));
    // the rows of the padding of B (a buffer that served a larger J may hold an earlier beta there)
    if (Jp > J) HIP_TRY(hipMemsetAsync(w->Bp + J * np, 0, (size_t)((Jp - J) * np) * sizeof(double), h->stream));
    GP_TRY(kron_axes_load(h, w->ax, mp.dc, n_c, axes_c, true));
    *out = w;
    return GPIMHIP_OK;
}
// the blocks' sub-model: the p ragged columns of X_s (the blocks' theta carry their lengthscales)
static gpimhip_model_t pkron_submodel(const gpimhip_model_t* m, int p) {
    gpimhip_model_t ms = *m;
    ms.dim = p;
    ms.n_ls = p;
    return ms;
}
// C (rows x cols) = Bm (rows x np, rows a multiple of 128: beta, one block per row, or the draws' solutions stacked) x R
// (np x cols, row stride ldr): one rectangle launch of the tile engine on a single problem
static int pkron_rows_times(gpimhip_ctx* h, const double* Bm, int64_t rows, const double* R, int64_t ldr, int64_t cols, double* C,
                            int64_t ldc) {
    const int64_t np = h->np;
    GemmArgs g = gemm_args(Bm, np, R, ldr, C, ldc, 1.0, 0.0, nullptr, 0, 0);
    g.rect_rows = (int)(rows / NB);
    g.rect_cols = (int)(cols / NB);
    g.ntiles = g.rect_rows * g.rect_cols;
    g.kfix0 = 0;
    g.kfix1 = (int)(np / NB);
    g.chunk = deal_chunk(g.ntiles);
    BatchScope one(h, 1);
    return launch_gemm(h, false, true, EPI_STORE, g);
}
// theta, the complete axes' decomposition, the blocks' theta, y~ = Y Q in the padded right-hand sides, and the blocks'
// K, L, L^-1, z, beta (steps 1 - 4 of an iteration without the inverse)
static int pkron_factor(gpimhip_ctx* h, const gpimhip_model_t* m, const gpimhip_model_t* ms, const PkronMap& mp, PkronWs* w,
                        const double* Xs, const double* Y, int64_t Ns, const double* u, bool grad) {
    const KronDev& dv = w->ax.dev;
    GP_TRY(launch_pkron_setup(h, m, mp, u, w->th3));
    GP_TRY(kron_eig_axes(h, w->ax, w->th3 + PK_TH_AXES));
    if (grad) GP_TRY(kron_grad_matrices(h, w->ax));
    GP_TRY(launch_pkron_blocks_theta(h, mp, dv, w->th3, w->lamj));
    const double* mats[KMAXD]; int ld[KMAXD];
    for (int i = 0; i < mp.dc; ++i) { mats[i] = dv.Qt + dv.moff[i]; ld[i] = mp.nc[i]; }
    double* res;
    GP_TRY(tensor_apply(h, mp.dc, mp.nc, mp.nc, mats, ld, 0, 0, Y, w->yt, w->yt + Ns * mp.J, &res, Ns));
    GP_TRY(launch_pkron_scatter(h, res, Ns, mp.J, h->ypad));
    return factor_at_u(h, ms, Xs, 0, Ns, u, true, false);
}
// Loss and gradient at u (and, fit mode, one Adam step).  Every launch reads its iteration-dependent values from the device.
static int pkron_iter(gpimhip_ctx* h, const gpimhip_model_t* m, const PkronMap& mp, PkronWs* w, const double* Xs,
                      const double* Y, int64_t Ns, double* u, int do_adam, double* loss_out, double* grad_out, FinalizeIter fi) {
    const int64_t np = h->np;
    const int J = mp.J;
    const KronDev& dv = w->ax.dev;
    const gpimhip_model_t ms = pkron_submodel(m, mp.p);
    GP_TRY(pkron_factor(h, m, &ms, mp, w, Xs, Y, Ns, u, true));
    { StageTimer t(h, 2); GP_TRY(launch_lauum(h, h->A, h->B, np, h->ld, rag_of(Ns, np))); }
    GP_TRY(launch_grad_reduce(h, &ms, h->B, h->ld, Xs, Ns, (int)(np / NB), h->alpha, 0));
    // W = K_s B: K_s once at variance 1, then one product on the tile engine (rows of W: the blocks)
    {
        BatchScope one(h, 1);
        GP_TRY(launch_kmat(h, &ms, Xs, Ns, nullptr, Ns, w->th3 + PK_TH_UNIT, 0.0, 0, w->Ks, h->ld, np, np, 1, 0, 0, 0, 0));
    }
    GP_TRY(launch_pkron_beta(h, Ns, J, w->Bp));
    GP_TRY(pkron_rows_times(h, w->Bp, pad_to(J, NB), w->Ks, h->ld, np, w->W, np));
    // Z_i = W x_i Mm_i: the mode product along complete axis i of the (n_1, ..., n_dc, np) tensor W
    for (int i = 0; i < mp.dc; ++i) {
        int64_t pre = 1, post = np;
        for (int k = 0; k < i; ++k) pre *= mp.nc[k];
        for (int k = i + 1; k < mp.dc; ++k) post *= mp.nc[k];
        GP_TRY(modeprod(h, w->W, w->Z + (int64_t)i * J * np, dv.Mm + dv.moff[i], mp.nc[i], mp.nc[i], mp.nc[i], 0, 0, pre,
                             post));
    }
    GP_TRY(launch_pkron_block_sums(h, mp, Ns, w->W, w->Z, w->bsum));
    return launch_pkron_finalize(h, m, mp, dv, Ns * (int64_t)J, w->bsum, w->th3, u, do_adam, loss_out, grad_out, fi);
}

// ------------------------------------------------------------------------------------------
// What a prediction and a draw share: the model's side of the call and the test side -- chunks of mc ragged test rows times
// the product grid of the complete test axes.  A draw at z = 0 has predict's bits because its mean is made by the same
// functions: pkron_test_side, pkron_slab, pkron_mix_mean.
// ------------------------------------------------------------------------------------------
struct PkCall {
    gpimhip_ctx* h; PkronWs* w; PkronMap mp; gpimhip_model_t ms;
    const double* Xs; int64_t Ns;
    const double* Xs_test; int64_t Ms; const int32_t* n_test_c;
    // the test grid on the complete axes: Mc = its points, sum_mn = sum m_i n_i (the cross factors), pmax = the largest
    // tensor (per ragged row) the chain of mode products n -> m passes through
    int64_t Mc, sum_mn, pmax;
    int64_t mc, kld;                    // ragged test rows per chunk; row stride of the K*_s slab h->Ks
    const double* bmat[KMAXD];          // b_i = K*_i Q_i (pkron_cross_factors)
};
// False: an axis of the test grid without a coordinate
static bool pkron_test_grid(PkCall& c) {
    c.Mc = 1; c.sum_mn = 0; c.pmax = 1;
    int64_t cur = c.mp.J;
    for (int i = 0; i < c.mp.dc; ++i) {
        if (c.n_test_c[i] < 1) return false;
        c.Mc *= c.n_test_c[i];
        c.sum_mn += (int64_t)c.n_test_c[i] * c.mp.nc[i];
        cur = cur / c.mp.nc[i] * c.n_test_c[i];
        c.pmax = std::max(c.pmax, cur);
    }
    return true;
}
// the chunk (the blocks' partial column sums, J x nb x mc doubles, stay <= ~0.5 GiB), ONE K* slab shared by the J blocks,
// and the buffers of the mean -- with those of the variance where it is wanted
static int pkron_test_side(PkCall& c, bool variance) {
    gpimhip_ctx* h = c.h;
    PkronWs* w = c.w;
    const int64_t np = h->np, J = c.mp.J, nb = np / NB;
    c.mc = std::min(pad_to(c.Ms, NB), std::max<int64_t>(NB, ((int64_t)1 << 26) / (J * nb) / NB * NB));
    {
        BatchScope one(h, 1);
        GP_TRY(ws_ensure_predict(h, np, c.mc));
    }
    c.kld = h->ks_cols + 16;
    if (variance) GP_TRY(w->colpart.grow(h, J * nb * c.mc));
    GP_TRY(w->G.grow(h, pad_to(J, NB) * c.mc));
    if (variance) GP_TRY(w->Q.grow(h, J * c.mc));
    GP_TRY(w->pp.grow(h, 4 * c.pmax * c.mc));
    return w->cross.grow(h, 2 * c.sum_mn);
}
// per complete axis: K*_i and bmat[i] = b_i = K*_i Q_i (eigen-coordinates straight to test points) in w->cross
static int pkron_cross_factors(PkCall& c, const double* axes_test_c) {
    const KronDev& dv = c.w->ax.dev;
    int toff = 0;
    int64_t ko = 0;
    for (int i = 0; i < c.mp.dc; ++i) {
        const int mi = c.n_test_c[i], ni = c.mp.nc[i];
        double* Kc = c.w->cross + ko;
        double* Bc = c.w->cross + c.sum_mn + ko;
        GP_TRY(kron_cross(c.h, dv, c.w->th3 + PK_TH_AXES, axes_test_c, toff, mi, i, Kc));
        GP_TRY(modeprod(c.h, Kc, Bc, dv.Qt + dv.moff[i], ni, ni, ni, 0, 0, mi, 1));
        c.bmat[i] = Bc;
        toff += mi;
        ko += (int64_t)mi * ni;
    }
    return GPIMHIP_OK;
}
// the mode products with b_i (squared entries: square) over `lead` tensors (n_1, ..., n_dc, mc) in src, alternating between
// bufa and bufb; *out = the (lead, m_1, ..., m_dc, mc) result
static int pkron_mode_chain(const PkCall& c, const double* src, double* bufa, double* bufb, int64_t lead, int square,
                            const double** out) {
    const double* cur = src;
    double* dst = bufa;
    for (int i = 0; i < c.mp.dc; ++i) {
        int64_t pre = lead, post = c.mc;
        for (int k = 0; k < i; ++k) pre *= c.n_test_c[k];
        for (int k = i + 1; k < c.mp.dc; ++k) post *= c.mp.nc[k];
        GP_TRY(modeprod(c.h, cur, dst, c.bmat[i], c.n_test_c[i], c.mp.nc[i], c.mp.nc[i], 0, square, pre, post));
        cur = dst;
        dst = (dst == bufa) ? bufb : bufa;
    }
    *out = cur;
    return GPIMHIP_OK;
}
// the ragged test rows [m0, m0 + cnt) of a chunk, cpad = cnt padded to 128
struct PkChunk { int64_t m0, cnt, cpad; };
static PkChunk pkron_chunk_at(const PkCall& c, int64_t m0) {
    const int64_t cnt = std::min(c.mc, c.Ms - m0);
    return PkChunk{m0, cnt, pad_to(cnt, NB)};
}
// K*_s of the chunk at variance 1 into h->Ks and, with `means`, G = B K*_s (Jp x cpad): the blocks' means before the mix
static int pkron_slab(const PkCall& c, const PkChunk& k, bool means) {
    gpimhip_ctx* h = c.h;
    {
        BatchScope one(h, 1);
        GP_TRY(launch_kmat(h, &c.ms, c.Xs, c.Ns, c.Xs_test + k.m0 * c.mp.p, k.cnt, c.w->th3 + PK_TH_UNIT, 0.0, 0, h->Ks, c.kld, h->np,
                           k.cpad, 0, 0, 0, 0, 0));
    }
    if (!means) return GPIMHIP_OK;
    return pkron_rows_times(h, c.w->Bp, pad_to(c.mp.J, NB), h->Ks, c.kld, k.cpad, c.w->G, c.mc);
}
// the mix of the blocks' means: *mraw = G x_i b_i, the mean before its factor s2 (in the first half of w->pp)
static int pkron_mix_mean(const PkCall& c, const double** mraw) {
    return pkron_mode_chain(c, c.w->G, c.w->pp, c.w->pp + c.pmax * c.mc, 1, 0, mraw);
}

// ------------------------------------------------------------------------------------------
// posterior draws: Matheron's rule with the prior drawn through
// L_P = chol(s2 K_s(P, P) + d I) of the union P of the ragged training and test rows and the root rows of the union of the
// complete axes (section 21), the update through the blocks' L_j^-1 for all draws of a group at once on the tile engine.
// Stage timers: 6 the blocks as a whole (theta, eigen-decomposition, factorisation, the mean's beta; inside it the engine's
// own intervals 0 / 1 of the blocks' factorisation and inverse), 4 the prior factor (covariance build, factorisation -- its
// context records no intervals of its own), 2 the prior draws (the union axes' decomposition and root rows, zeta,
// H = L_P zeta, gathers, mode products), 3 the update (cross factors, residual, projection, the blocks' solves, K*_s
// products and mode products, the mean's among them), 5 the epilogue.
// ------------------------------------------------------------------------------------------
// doubles of the buffers that grow with the draws of one group (0.25 GiB): a call of more draws takes them group by group
#define PKS_GROUP_BUDGET ((int64_t)1 << 25)
static int pks_bad(const std::string& what) {
    gpim_set_error("gpimhip_sample_pkron: " + what);
    return GPIMHIP_E_BADARG;
}
// the sizes of a call: the prior factor's order, the draw groups, the tile lists and the arena
struct PksPlan {
    KronUnion un;
    int64_t Us, npU, ldU; int nbU;
    int64_t big;                        // the largest tensor of one draw on the two chains of root rows: U -> J, U -> Mc
    int Sg0;                            // draws per group (the last group may be shorter)
    int64_t cols, Sp, rowsP;            // Sg0 U, Sg0 and Sg0 J padded to 128
    int n_prior, n_solve;
    std::vector<TileDesc> tl;           // H = L_P zeta | T = L_j^-1 R | beta = L_j^-T T
    int64_t th_d, total;
};
// the pieces of the call's arena
struct PksBufs {
    ThetaDev* thp;
    double *LP, *Zg, *Hm, *g0, *g1, *g2, *R0, *R1, *Bst, *Gs, *pa, *pb, *RX, *RT;
    int32_t *iX, *iT, *ic, *it;
    const TileDesc *t_prior, *t_nn, *t_tn;
};
// one call's draw: the shared test side, the plan, the arena, the prior's contexts and the caller's arrays
struct PksDraw : PkCall, PksPlan, PksBufs {
    gpimhip_ctx* sub;                   // factors L_P
    const KronDev* du;                  // the decomposition of the union axes
    const int32_t* n_union;
    const double *rxm[KMAXD], *rtm[KMAXD];          // root rows of the union axes at the training / test coordinates
    const double *Z, *ze, *zn; int64_t zw, NJ;      // z: rows of zw doubles, zeta | z_e | z_n
    int S, noiseless, rag;
    double *mean_out, *samples_out;
};
// Draw groups: the buffers that grow with the draws stay within PKS_GROUP_BUDGET (GPIMHIP_PKRON_DRAW_GROUP, for tests: and
// within that many draws); every draw's arithmetic is its own (one thread per element in the kernels of pkron.hip, one
// k-loop per element in the tile engine and the mode products), so the grouping does not reach the result
static int pks_plan(PksDraw& d) {
    const int64_t np = d.h->np, J = d.mp.J, U = d.un.U;
    const int nb = (int)(np / NB);
    d.npU = d.sub->np; d.ldU = d.sub->ld; d.nbU = (int)(d.npU / NB);
    int64_t cx = U, ct = U, maxX = U, maxT = U;
    for (int i = 0; i < d.mp.dc; ++i) {
        cx = cx / d.n_union[i] * d.mp.nc[i];
        ct = ct / d.n_union[i] * d.n_test_c[i];
        maxX = std::max(maxX, cx);
        maxT = std::max(maxT, ct);
    }
    d.big = std::max(d.Ns * maxX, d.Ms * maxT);
    const int64_t per_draw = 2 * d.npU * U + 3 * d.big + 2 * d.pmax * d.mc + J * (3 * np + d.mc);
    int Sg_max = (int)std::max<int64_t>(1, std::min<int64_t>(d.S, PKS_GROUP_BUDGET / per_draw));
    if (const char* e = getenv("GPIMHIP_PKRON_DRAW_GROUP"))
        if (atoll(e) >= 1) Sg_max = (int)std::min<int64_t>(Sg_max, atoll(e));
    const int ngroups = (d.S + Sg_max - 1) / Sg_max;
    d.Sg0 = (d.S + ngroups - 1) / ngroups;
    d.cols = pad_to(d.Sg0 * U, NB); d.Sp = pad_to(d.Sg0, NB); d.rowsP = pad_to(d.Sg0 * J, NB);
    const int nct = (int)(d.cols / NB), nst = (int)(d.Sp / NB);
    if ((int64_t)d.nbU * nct > (1 << 28) || (int64_t)nb * nst > (1 << 28)) return pks_bad("too many tiles in one launch");
    // tile lists, longest k-ranges first: H = L_P zeta and T = L_j^-1 R stop at the diagonal block, beta = L_j^-T T starts there
    d.tl.reserve((size_t)d.nbU * nct + 2 * (size_t)nb * nst);
    tri_tiles(d.tl, d.nbU, nct, true);
    tri_tiles(d.tl, nb, nst, true);
    tri_tiles(d.tl, nb, nst, false);
    d.n_prior = d.nbU * nct; d.n_solve = nb * nst;
    d.th_d = (int64_t)((sizeof(ThetaDev) + 15) / 16 * 2);
    d.total = d.th_d + d.npU * d.ldU + 2 * d.npU * d.cols + 3 * d.Sg0 * d.big + 2 * J * np * d.Sp + d.rowsP * np + d.rowsP * d.mc +
              2 * d.Sg0 * d.pmax * d.mc + d.un.sum_nu + d.un.sum_mu + (d.Ns + d.Ms + d.un.sum_n + d.un.sum_m) / 2 +
              2 * (int64_t)d.tl.size() + 64;
    return GPIMHIP_OK;
}
// the call's arena, its pieces, and the index maps and tile lists copied in
static int pks_carve(PksDraw& d, DevBuf<double>& ck, const int32_t* irow_train, const int32_t* irow_test, const int32_t* idx_train,
                     const int32_t* idx_test) {
    const int64_t np = d.h->np, J = d.mp.J;
    hipStream_t st = d.h->stream;
    GP_TRY(ck.grow(d.h, d.total));
    Carve a(ck);
    d.thp = a.take<ThetaDev>(d.th_d);
    d.LP = a.take(d.npU * d.ldU);
    d.Zg = a.take(d.npU * d.cols); d.Hm = a.take(d.npU * d.cols);
    d.g0 = a.take(d.Sg0 * d.big); d.g1 = a.take(d.Sg0 * d.big); d.g2 = a.take(d.Sg0 * d.big);
    d.R0 = a.take(J * np * d.Sp); d.R1 = a.take(J * np * d.Sp);
    d.Bst = a.take(d.rowsP * np); d.Gs = a.take(d.rowsP * d.mc);
    d.pa = a.take(d.Sg0 * d.pmax * d.mc); d.pb = a.take(d.Sg0 * d.pmax * d.mc);
    d.RX = a.take(d.un.sum_nu); d.RT = a.take(d.un.sum_mu);
    d.iX = a.take<int32_t>((d.Ns + 1) / 2);
    d.iT = a.take<int32_t>((d.Ms + 1) / 2);
    d.ic = a.take<int32_t>((d.un.sum_n + 1) / 2);
    d.it = a.take<int32_t>((d.un.sum_m + 1) / 2);
    TileDesc* tiles = a.take<TileDesc>(2 * (int64_t)d.tl.size());
    HIP_TRY(hipMemcpyAsync(d.iX, irow_train, (size_t)d.Ns * sizeof(int32_t), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d.iT, irow_test, (size_t)d.Ms * sizeof(int32_t), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d.ic, idx_train, (size_t)d.un.sum_n * sizeof(int32_t), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d.it, idx_test, (size_t)d.un.sum_m * sizeof(int32_t), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(tiles, d.tl.data(), d.tl.size() * sizeof(TileDesc), hipMemcpyHostToDevice, st));
    HIP_TRY(hipStreamSynchronize(st));          // the host arrays are the caller's
    d.t_prior = tiles; d.t_nn = tiles + d.n_prior; d.t_tn = d.t_nn + d.n_solve;
    return GPIMHIP_OK;
}
// L_P = chol(s2 K_s(P, P) + d I); its status goes into the word of the call (NOT_PD at the closing check)
static int pks_prior_factor(const PksDraw& d, const double* P, double jitter) {
    StageTimer t(d.h, 4);
    GP_TRY(launch_pkron_prior_theta(d.h, d.w->th3, d.thp));
    GP_TRY(launch_kmat(d.sub, &d.ms, P, d.Us, nullptr, d.Us, d.thp, jitter, 0, d.LP, d.ldU, d.npU, d.npU, 1, 1, 0, 0, 0));
    GP_TRY(launch_potrf(d.sub, d.LP, d.npU, d.ldU, d.h->info));
    // the factorisation leaves the strict upper triangle of the diagonal blocks as the covariance build wrote it
    return launch_pkron_tril(d.h, d.LP, d.ldU, d.nbU);
}
// H = L_P zeta for the Sg U columns of the group, then *gX = g_X = H[i_X, :] x_i R_i[ic_i, :]
static int pks_group_prior(const PksDraw& d, int s0, int Sg, double** gX) {
    StageTimer t(d.h, 2);
    GP_TRY(launch_pkron_zeta(d.h, d.Z, d.zw, d.Us, d.un.U, s0, Sg, d.npU, d.cols, d.Zg));
    GemmArgs g = gemm_args(d.LP, d.ldU, d.Zg, d.cols, d.Hm, d.cols, 1.0, 0.0, d.t_prior, d.n_prior, 0);
    g.chunk = deal_chunk(g.ntiles);
    GP_TRY(launch_gemm(d.sub, false, true, EPI_STORE, g));
    GP_TRY(launch_pkron_gather(d.h, d.Hm, d.cols, d.iX, d.Ns, d.un.U, Sg, d.g0));
    return tensor_apply(d.h, d.mp.dc, d.n_union, d.mp.nc, d.rxm, d.n_union, 0, 0, d.g0, d.g1, d.g2, gX, (int64_t)Sg * d.Ns);
}
// r = -g_X - sqrt(sigma) z_e, r~ = r x_i Q_i^T, beta_j = L_j^-T (L_j^-1 r~_j) for the J blocks and all draws, stacked in Bst
static int pks_group_solve(const PksDraw& d, int s0, int Sg, double* gX) {
    gpimhip_ctx* h = d.h;
    const KronDev& dv = d.w->ax.dev;
    const int64_t np = h->np, J = d.mp.J;
    const size_t rbytes = (size_t)(J * np * d.Sp) * sizeof(double);
    StageTimer t(h, 3);
    GP_TRY(launch_pkron_resid(h, d.ze, d.zw, s0, d.NJ, Sg, d.w->th3, gX));
    const double* qtm[KMAXD];
    for (int i = 0; i < d.mp.dc; ++i) qtm[i] = dv.Qt + dv.moff[i];
    double *other = gX == d.g1 ? d.g2 : d.g1, *res;
    GP_TRY(tensor_apply(h, d.mp.dc, d.mp.nc, d.mp.nc, qtm, d.mp.nc, 0, 0, gX, other, gX, &res, (int64_t)Sg * d.Ns));
    GP_TRY(launch_pkron_scatter_multi(h, res, d.Ns, J, Sg, d.Sp, d.R0));
    // (a ragged launch stores no row of the padding of the last block: GemmArgs::rag)
    if (d.rag) HIP_TRY(hipMemsetAsync(d.R1, 0, rbytes, h->stream));
    GemmArgs g = gemm_args(h->A, h->ld, d.R0, d.Sp, d.R1, d.Sp, 1.0, 0.0, d.t_nn, d.n_solve, np);
    g.chunk = deal_chunk(g.ntiles);
    g.rag = d.rag;
    GP_TRY(launch_gemm(h, false, true, EPI_STORE, g));
    if (d.rag) HIP_TRY(hipMemsetAsync(d.R0, 0, rbytes, h->stream));
    g = gemm_args(h->A, h->ld, d.R1, d.Sp, d.R0, d.Sp, 1.0, 0.0, d.t_tn, d.n_solve, np);
    g.chunk = deal_chunk(g.ntiles);
    g.krev = 1;
    g.rag = d.rag;
    GP_TRY(launch_gemm(h, true, true, EPI_STORE, g));
    return launch_pkron_beta_stack(h, d.R0, d.Ns, J, Sg, d.Sp, d.rowsP, d.Bst);
}
// *gs = g_* = H[i_*, :] x_i R_i[it_i, :]
static int pks_group_test_prior(const PksDraw& d, int Sg, double** gs) {
    StageTimer t(d.h, 2);
    GP_TRY(launch_pkron_gather(d.h, d.Hm, d.cols, d.iT, d.Ms, d.un.U, Sg, d.g0));
    return tensor_apply(d.h, d.mp.dc, d.n_union, d.n_test_c, d.rtm, d.n_union, 0, 0, d.g0, d.g1, d.g2, gs, (int64_t)Sg * d.Ms);
}
// one chunk of ragged test rows for the draws of a group: the mean (first group), the update and the epilogue
static int pks_chunk(const PksDraw& d, const PkChunk& k, int s0, int Sg, const double* gs) {
    const double* upd;
    {
        StageTimer t(d.h, 3);
        GP_TRY(pkron_slab(d, k, s0 == 0));
        if (s0 == 0) {
            const double* mraw;
            GP_TRY(pkron_mix_mean(d, &mraw));
            GP_TRY(launch_pkron_mean(d.h, d.w->th3, d.Mc, d.mc, k.m0, k.cnt, mraw, d.mean_out));
        }
        // G = B K*_s with the draws' solutions stacked as rows, then the mode products with b_i, batch Sg
        GP_TRY(pkron_rows_times(d.h, d.Bst, d.rowsP, d.h->Ks, d.kld, k.cpad, d.Gs, d.mc));
        GP_TRY(pkron_mode_chain(d, d.Gs, d.pa, d.pb, Sg, 0, &upd));
    }
    StageTimer t(d.h, 5);
    return launch_pkron_draw(d.h, d.w->th3, d.Mc, d.mc, k.m0, k.cnt, d.Ms, s0, Sg, gs, upd, d.mean_out, d.zn, d.zw, d.noiseless,
                             d.samples_out);
}

extern "C" {

int gpimhip_pkron_nll_grad(gpimhip_handle h, const gpimhip_model_t* m, const double* Xs, int64_t Ns, int32_t p, int32_t dc,
                           const int32_t* n_c, const int32_t* perm, const double* axes_c, const double* Y, const double* u,
                           double* loss_out, double* grad_out) {
    PkronMap mp;
    GP_TRY(pkron_check(h, m, Xs, Ns, p, dc, n_c, perm, axes_c, Y, &mp));
    if (!u) return GPIMHIP_E_BADARG;
    PkronWs* w = nullptr;
    GP_TRY(pkron_begin(h, mp, n_c, axes_c, Ns, &w));
    GP_TRY(pkron_iter(h, m, mp, w, Xs, Y, Ns, const_cast<double*>(u), 0, loss_out, grad_out,
                      FinalizeIter{nullptr, nullptr, 0, nullptr, nullptr}));
    return finish_and_check(h);
}

int gpimhip_fit_pkron(gpimhip_handle h, const gpimhip_model_t* m, const double* Xs, int64_t Ns, int32_t p, int32_t dc,
                      const int32_t* n_c, const int32_t* perm, const double* axes_c, const double* Y, double* u_inout, double lr,
                      int32_t T, double* hist_out, double* loss_out) {
    PkronMap mp;
    GP_TRY(pkron_check(h, m, Xs, Ns, p, dc, n_c, perm, axes_c, Y, &mp));
    if (!u_inout || T < 0) return GPIMHIP_E_BADARG;
    PkronWs* w = nullptr;
    GP_TRY(pkron_begin(h, mp, n_c, axes_c, Ns, &w));
    GP_TRY(fit_prologue(h, lr, T, h->adam_m, h->adam_v, MAXP * sizeof(double), h->iter));
    if (T == 0) return finish_and_check(h);
    const FinalizeIter fi{h->iter, h->bc, T, hist_out, loss_out};
    return run_fit_iterations(h, T, FIT_LOOP_DENSE,
                              [&] { return pkron_iter(h, m, mp, w, Xs, Y, Ns, u_inout, 1, nullptr, nullptr, fi); });
}

int gpimhip_predict_pkron(gpimhip_handle h, const gpimhip_model_t* m, const double* Xs, int64_t Ns, int32_t p, int32_t dc,
                          const int32_t* n_c, const int32_t* perm, const double* axes_c, const double* Y, const double* u,
                          const double* Xs_test, int64_t Ms, const int32_t* n_test_c, const double* axes_test_c,
                          double* mean_out, double* var_out) {
    PkCall c;
    GP_TRY(pkron_check(h, m, Xs, Ns, p, dc, n_c, perm, axes_c, Y, &c.mp));
    if (!u || !Xs_test || Ms < 1 || !n_test_c || !axes_test_c || !mean_out || !var_out) return GPIMHIP_E_BADARG;
    c.h = h; c.Xs = Xs; c.Ns = Ns; c.Xs_test = Xs_test; c.Ms = Ms; c.n_test_c = n_test_c;
    c.ms = pkron_submodel(m, p);
    if (!pkron_test_grid(c)) return GPIMHIP_E_BADARG;
    GP_TRY(pkron_begin(h, c.mp, n_c, axes_c, Ns, &c.w));
    PkronWs* w = c.w;
    const int64_t np = h->np;
    const int J = c.mp.J, nb = (int)(np / NB);
    GP_TRY(pkron_test_side(c, true));
    const int64_t mc = c.mc;
    GP_TRY(pkron_factor(h, m, &c.ms, c.mp, w, Xs, Y, Ns, u, false));
    GP_TRY(launch_pkron_beta(h, Ns, J, w->Bp));
    GP_TRY(pkron_cross_factors(c, axes_test_c));
    for (int64_t m0 = 0; m0 < Ms; m0 += mc) {
        const PkChunk k = pkron_chunk_at(c, m0);
        GP_TRY(pkron_slab(c, k, true));
        // q_j = |L_j^-1 k*|^2 from the raw column sums of the batched variance product (K* at variance 1, shared: stride 0)
        GemmArgs g = gemm_args(h->A, h->ld, h->Ks, c.kld, nullptr, 0, 1.0, 0.0, h->pred_tiles, 0, h->np);
        g.sB = 0;
        g.colpart = w->colpart;
        g.ld_colpart = mc;
        g.sColpart = (int64_t)nb * mc;
        g.ntiles = (int)h->pred_ntiles;
        g.chunk = deal_chunk(g.ntiles);
        g.rag = rag_of(Ns, np);
        { StageTimer t(h, 3); GP_TRY(launch_gemm(h, false, true, EPI_COLSUMSQ, g)); }
        GP_TRY(launch_pkron_qsum(h, J, nb, mc, k.cnt, w->colpart, w->Q));
        // mean = s2 G b^T, var = clamp(s2 - s2^2 Q (b o b)^T, 0) + noise: mode products over the (n_1, ..., n_dc, mc) tensors
        const double *mraw, *vraw;
        double* bufv = w->pp + 2 * c.pmax * mc;
        GP_TRY(pkron_mix_mean(c, &mraw));
        GP_TRY(pkron_mode_chain(c, w->Q, bufv, bufv + c.pmax * mc, 1, 1, &vraw));
        GP_TRY(launch_pkron_post(h, w->th3, c.Mc, mc, k.m0, k.cnt, mraw, vraw, mean_out, var_out));
    }
    return finish_and_check(h);
}

int gpimhip_sample_pkron(gpimhip_handle h, const gpimhip_model_t* m, const double* Xs, int64_t Ns, int32_t p, int32_t dc,
                         const int32_t* n_c, const int32_t* perm, const double* axes_c, const double* Y, const double* u,
                         const double* Xs_test, int64_t Ms, const int32_t* n_test_c, const double* axes_test_c,
                         const double* P, int64_t Us, const int32_t* irow_train, const int32_t* irow_test,
                         const int32_t* n_union, const double* axes_union, const int32_t* idx_train, const int32_t* idx_test,
                         const double* Z, int32_t S, int32_t noiseless, double jitter, double* mean_out, double* samples_out) {
    if (!h || !m || !Xs || !n_c || !axes_c || !Y || !u || !Xs_test || !n_test_c || !axes_test_c || !P || !irow_train ||
        !irow_test || !n_union || !axes_union || !idx_train || !idx_test || !Z || !mean_out || !samples_out)
        return pks_bad("a null argument (every pointer but perm is required)");
    if (S < 1) return pks_bad("needs S >= 1");
    if (!(jitter > 0.0) || !(jitter < HUGE_VAL))
        return pks_bad("needs a finite jitter > 0 (the prior factor of the ragged rows is chol(s2 K_s(P, P) + jitter I))");
    PksDraw d;
    GP_TRY(pkron_check(h, m, Xs, Ns, p, dc, n_c, perm, axes_c, Y, &d.mp));
    if (Ms < 1 || Us < 1 || Us > Ns + Ms) return pks_bad("needs Ms >= 1 and 1 <= Us <= Ns + Ms union rows");
    GP_TRY(kron_union_check("gpimhip_sample_pkron", dc, n_c, n_test_c, n_union, idx_train, idx_test, &d.un));
    for (int64_t a = 0; a < Ns; ++a)
        if (irow_train[a] < 0 || irow_train[a] >= Us) return pks_bad("irow_train outside the union rows");
    for (int64_t a = 0; a < Ms; ++a)
        if (irow_test[a] < 0 || irow_test[a] >= Us) return pks_bad("irow_test outside the union rows");
    d.h = h; d.Xs = Xs; d.Ns = Ns; d.Xs_test = Xs_test; d.Ms = Ms; d.n_test_c = n_test_c;
    d.ms = pkron_submodel(m, p);
    (void)pkron_test_grid(d);           // (every axis has a coordinate: checked above)
    GP_TRY(pkron_begin(h, d.mp, n_c, axes_c, Ns, &d.w));
    PkronWs* w = d.w;
    const bool shared = d.un.shared;
    d.n_union = n_union; d.S = S; d.noiseless = noiseless ? 1 : 0; d.rag = rag_of(Ns, h->np);
    d.mean_out = mean_out; d.samples_out = samples_out;
    d.Us = Us; d.NJ = Ns * d.mp.J; d.zw = Us * d.un.U + d.NJ + Ms * d.Mc;
    d.Z = Z; d.ze = Z + Us * d.un.U; d.zn = d.ze + d.NJ;
    GP_TRY(pkron_test_side(d, false));          // the chunks of ragged test rows and the mean's buffers are predict's
    PkronDrawWs sw = sample_pkron_ws(h);
    GP_TRY(draw_sub(h, &sw.sub, Us));
    d.sub = sw.sub;
    if (!shared) GP_TRY(kron_axes_load(h, sw.ck_un, dc, n_union, axes_union, false));
    d.du = shared ? &w->ax.dev : &sw.ck_un.dev;
    GP_TRY(pks_plan(d));
    GP_TRY(pks_carve(d, sw.ck, irow_train, irow_test, idx_train, idx_test));
    {   // the blocks: theta, the complete axes, L_j^-1, and the mean's beta as gpimhip_predict_pkron computes it
        StageTimer t(h, 6);
        GP_TRY(pkron_factor(h, m, &d.ms, d.mp, w, Xs, Y, Ns, u, false));
        GP_TRY(launch_pkron_beta(h, Ns, d.mp.J, w->Bp));
    }
    { StageTimer t(h, 3); GP_TRY(pkron_cross_factors(d, axes_test_c)); }
    {   // the union of the complete axes and the rows of its root at the training and at the test coordinates
        StageTimer t(h, 2);
        if (!shared) GP_TRY(kron_eig_axes(h, sw.ck_un, w->th3 + PK_TH_AXES));
        GP_TRY(kron_union_roots(h, *d.du, dc, n_c, n_test_c, d.ic, d.it, d.RX, d.RT, d.rxm, d.rtm));
    }
    GP_TRY(pks_prior_factor(d, P, jitter));
    for (int s0 = 0; s0 < S; s0 += d.Sg0) {
        const int Sg = std::min(d.Sg0, S - s0);
        double *gX, *gs;
        GP_TRY(pks_group_prior(d, s0, Sg, &gX));
        GP_TRY(pks_group_solve(d, s0, Sg, gX));
        GP_TRY(pks_group_test_prior(d, Sg, &gs));
        for (int64_t m0 = 0; m0 < Ms; m0 += d.mc) GP_TRY(pks_chunk(d, pkron_chunk_at(d, m0), s0, Sg, gs));
    }
    return finish_and_check(h);
}

}  // extern "C"
