// pkron.hpp -- shared declarations of the dense-by-Kronecker blocks (pkron.hip kernels and launchers, pkrongp.hip drivers;
// DESIGN.md sections 22 and 23).
#pragma once
#include "common.hpp"
#include "kron.hpp"

#define PK_SUMS 16          // doubles per block in PkronWs::bsum (pkron_block_sums_kernel)

// the split of the model's axes: ragged columns of Xs first, then the complete axes.  perm[k] = the model's axis (the
// index of its lengthscale) behind ragged column k (k < p) or complete axis k - p.  Passed to the kernels by value.
struct PkronMap {
    int p, dc, J;
    int perm[GPIMHIP_MAX_DIM];
    int nc[GPIMHIP_MAX_DIM];        // orders of the complete axes
};

// theta of one evaluation (device): [0] the model's (original axis order: the chain rule of finalize_step), [1] the
// complete axes' lengthscales in ls[0 .. dc) (kron_eig_axes, kron_cross), [2] the ragged columns' at variance 1 (K_s, K*_s)
#define PK_TH_MODEL 0
#define PK_TH_AXES 1
#define PK_TH_UNIT 2

// the handle's workspace (h->pkron)
struct PkronWs {
    KronAxes ax;                                        // the complete axes: K_i, E_i, Q_i, lambda_i, Mm_i, mdiag_i
    DevBuf<ThetaDev> th3;           // PK_TH_MODEL, PK_TH_AXES, PK_TH_UNIT
    DevBuf<double> lamj;            // J: lambda_j
    DevBuf<double> yt;              // 2 x N_s J: the mode products of the projection
    DevBuf<double> Ks;              // np x ld: K_s at variance 1
    DevBuf<double> Bp;              // Jp x np: beta, zero on the padding (Jp = J padded to 128)
    DevBuf<double> W;               // Jp x np: K_s B
    DevBuf<double> Z;               // dc x J x np: W x_i Mm_i
    DevBuf<double> bsum;            // J x PK_SUMS
    // prediction (chunks of mc ragged test rows)
    DevBuf<double> colpart;         // J x nb x mc
    DevBuf<double> G;               // Jp x mc: K*_s B
    DevBuf<double> Q;               // J x mc: k*^T M_j k*
    DevBuf<double> pp;              // 4 x pmax x mc: the mode products of mean and variance
    DevBuf<double> cross;           // 2 x sum m_i n_i: K*_i and K*_i Q_i
};

// ---- launchers (pkron.hip) ----
int launch_pkron_setup(gpimhip_ctx* h, const gpimhip_model_t* m, const PkronMap& mp, const double* u, ThetaDev* th3);
// lambda_j = prod_i max(lam_i[j_i], 0) into lamj and the J blocks' theta (variance s2 lambda_j, the ragged lengthscales,
// noise, noise + jitter on the diagonal) into h->theta
int launch_pkron_blocks_theta(gpimhip_ctx* h, const PkronMap& mp, const KronDev& dv, const ThetaDev* th3, double* lamj);
// ypad[j * np + n] = yt[n * J + j] (n < Ns), 0 on the padding rows
int launch_pkron_scatter(gpimhip_ctx* h, const double* yt, int64_t Ns, int J, double* ypad);
// B[j * np + n] = beta_j[n] (h->alpha) with zeros on the padding rows n >= Ns
int launch_pkron_beta(gpimhip_ctx* h, int64_t Ns, int J, double* B);
// per block j: the seven gradient sums, |z_j|^2, sum log diag L_j, beta_j . W_j and beta_j . Z_i,j (i < dc) into bsum[j]
int launch_pkron_block_sums(gpimhip_ctx* h, const PkronMap& mp, int64_t Ns, const double* W, const double* Z, double* bsum);
int launch_pkron_finalize(gpimhip_ctx* h, const gpimhip_model_t* m, const PkronMap& mp, const KronDev& dv, int64_t Ntot,
                          const double* bsum, const ThetaDev* th3, double* u, int do_adam, double* loss_out, double* grad_out,
                          FinalizeIter fi);
// q[j * ldq + t] = sum_ci colpart[(j * nb + ci) * ldq + t]: the raw |L_j^-1 k*_s(x_t)|^2 of the batched variance product
int launch_pkron_qsum(gpimhip_ctx* h, int J, int nb, int64_t ldq, int64_t cnt, const double* colpart, double* q);
// mean_out[(m0 + t) * Mc + c] = s2 mraw[c * ldq + t];  var_out = clamp(s2 - s2^2 vraw[c * ldq + t], 0) + noise
int launch_pkron_post(gpimhip_ctx* h, const ThetaDev* th3, int64_t Mc, int64_t ldq, int64_t m0, int64_t cnt, const double* mraw,
                      const double* vraw, double* mean_out, double* var_out);

// ---- posterior draws (gpimhip_sample_pkron): Sg draws s0 .. s0 + Sg of the call per launch ----
// *out = the ragged lengthscales at the model's variance: theta of the prior factor chol(s2 K_s(P, P) + d I)
int launch_pkron_prior_theta(gpimhip_ctx* h, const ThetaDev* th3, ThetaDev* out);
// the strict upper triangle of the nb diagonal blocks of the factor L <- 0
int launch_pkron_tril(gpimhip_ctx* h, double* L, int64_t ld, int nb);
// out (rows x cols, zero padded)[r, s U + c] = zeta_{s0 + s}[r, c]; z: rows of zw doubles, zeta first (Us x U)
int launch_pkron_zeta(gpimhip_ctx* h, const double* z, int64_t zw, int64_t Us, int64_t U, int s0, int Sg, int64_t rows, int64_t cols,
                      double* out);
// out[s, n, c] = H[idx[n], s U + c] (n < rows, c < U)
int launch_pkron_gather(gpimhip_ctx* h, const double* H, int64_t ldh, const int32_t* idx, int64_t rows, int64_t U, int Sg, double* out);
// g[s, e] <- -g[s, e] - sqrt(noise + jitter) ze[(s0 + s) zw + e], e < NJ
int launch_pkron_resid(gpimhip_ctx* h, const double* ze, int64_t zw, int s0, int64_t NJ, int Sg, const ThetaDev* th3, double* g);
// out (J x np x Sp)[j, n, s] = yt[s, n, j], zero for n >= Ns or s >= Sg
int launch_pkron_scatter_multi(gpimhip_ctx* h, const double* yt, int64_t Ns, int64_t J, int Sg, int64_t Sp, double* out);
// out (rows x np)[s J + j, n] = beta (J x np x Sp)[j, n, s], zero for rows >= Sg J or n >= Ns
int launch_pkron_beta_stack(gpimhip_ctx* h, const double* beta, int64_t Ns, int64_t J, int Sg, int64_t Sp, int64_t rows, double* out);
// mean_out[(m0 + t) Mc + c] = s2 mraw[c ldq + t]
int launch_pkron_mean(gpimhip_ctx* h, const ThetaDev* th3, int64_t Mc, int64_t ldq, int64_t m0, int64_t cnt, const double* mraw,
                      double* mean_out);
// out[s0 + s, m0 + t, c] = mean[m0 + t, c] + g*[s, m0 + t, c] + s2 upd[(s Mc + c) ldq + t] + sqrt(c_n) zn[(s0 + s) zw + ...]
int launch_pkron_draw(gpimhip_ctx* h, const ThetaDev* th3, int64_t Mc, int64_t ldq, int64_t m0, int64_t cnt, int64_t Ms, int s0, int Sg,
                      const double* gs, const double* upd, const double* mean, const double* zn, int64_t zw, int noiseless,
                      double* out);
