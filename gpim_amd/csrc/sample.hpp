// sample.hpp -- shared declarations of the joint posterior draws (sample.hip kernels, draws.hip drivers).
#pragma once
#include "common.hpp"

// J[i][i] += jitter + noise(theta) for the n_train leading points, += (noiseless ? 0 : noise(theta)) + jitter_s for the
// n_test points behind them (the identity padding at the end is kmat's)
int launch_sample_diag(gpimhip_ctx* h, double* J, int64_t ld, int64_t n_train, int64_t n_test, const ThetaDev* theta,
                       int noiseless, double jitter_s);
// One sweep of the trapezoid L[N:, :] of the factor of the joint matrix (sample.hip): mean, variance and the draws
// s0 .. s0 + min(S - s0, group) - 1.  mean_ws (M): written when s0 == 0, read by the later groups.
int launch_sample_draws(gpimhip_ctx* h, const double* L, int64_t ld, int64_t N, int64_t M, const double* z, const double* Z,
                        int S, int s0, const ThetaDev* theta, int noiseless, double jitter_s, double* mean_ws,
                        double* mean_out, double* var_out, double* out);
int sample_draw_group(int S);
// a factorisation context of the draws at the given matrix order: created on first use, on the model handle's stream, one
// problem, no matrices (draws.hip: SampleWs)
int draw_sub(gpimhip_ctx* h, gpimhip_ctx** sub, int64_t order);
// what the draws of the dense-by-Kronecker blocks (pkrongp.hip: gpimhip_sample_pkron) keep in the
// handle's draw workspace: `sub` factors L_P, one arena carved per call, and the union of the complete axes when the training
// axes do not serve
struct KronAxes;
struct PkronDrawWs { gpimhip_ctx*& sub; DevBuf<double>& ck; KronAxes& ck_un; };
PkronDrawWs sample_pkron_ws(gpimhip_ctx* h);

// ---- pathwise draws (gpimhip_sample_pathwise) ----
// The complete product grid G of the draw: n[k] points along axis k (row-major, last axis fastest), mask = the reflected
// axes, f[k] = the extent of the fundamental domain ((n[k] + 1) / 2 on a reflected axis, else n[k]).
struct PwGrid { int d, mask; int n[GPIMHIP_MAX_DIM], f[GPIMHIP_MAX_DIM]; };
// Xq (Nq x d): the fundamental domain's coordinates out of G; wts (B x Nq): 1 / sqrt(|stabiliser|), 0 where the point does
// not exist in the block (ReflArgs::wts); Xt (N x d): the training rows G[idx]
int launch_pw_setup(gpimhip_ctx* h, PwGrid gd, const double* G, int64_t M, int64_t Nq, int B, double* Xq, double* wts,
                    const int64_t* idx, int64_t N, double* Xt);
// Zg[b][s][p] = Z[s][flat(gamma_b p)] where p exists in block b (gamma_b: the reflection of the axes whose sign is -1 in
// b -- a bijection of the present (b, p) onto G), else 0
int launch_pw_gather_z(gpimhip_ctx* h, PwGrid gd, const double* Z, int64_t zw, int S, int64_t Nq, int B, double* Zg);
// g = U^T c: g[s][gamma p] = B^-1/2 sqrt(|Stab_p|) sum_b chi_b(gamma) c[b][s][p], b ascending over the blocks that hold p
int launch_pw_basis_t(gpimhip_ctx* h, PwGrid gd, const double* C, int S, int64_t Nq, int B, int64_t M, double* g);
// R (S + 1 rows of npt): row s = g[s][idx] + sqrt(diag_add - jitter_s) Z[s][M + .], row S = y; zero padding
int launch_pw_rhs(gpimhip_ctx* h, const double* g, int64_t M, const int64_t* idx, int64_t N, const double* Z, int64_t zw, int S,
                  const double* y, const ThetaDev* theta, double jitter_s, double* R, int64_t npt);
// theta->diag_add = v (the prior blocks carry the draw's jitter where training carries noise + jitter)
int launch_pw_set_diag(gpimhip_ctx* h, ThetaDev* theta, double v);
// One sweep of K(G, X) for the draws s0 .. s0 + group - 1 and the mean column (row S of Al):
//   out[s][i] = mean_i + g[s][i] - sum_j k(G_i, X_j) Al[s][j]  (+ sqrt(noise) Z[s][zn_off + i] unless noiseless)
int launch_pw_cross_apply(gpimhip_ctx* h, const gpimhip_model_t* m, const double* G, int64_t M, const double* Xt, int64_t N,
                          const ThetaDev* theta, const double* Al, int64_t npt, int S, int s0, const double* g, const double* Z,
                          int64_t zw, int64_t zn_off, int noiseless, double* mean_out, double* out);
// out[s][idx[j]] -= jitter_s Al[s][j]  (idx distinct)
int launch_pw_scatter(gpimhip_ctx* h, const int64_t* idx, int64_t N, int64_t M, const double* Al, int64_t npt, int S,
                      double jitter_s, double* out);

// ---- draws on a fully observed grid through the reflection blocks (gpimhip_sample_blocks) ----
// E[b][s][p] (S + 1 rows of npq per block) = (U v_s)_{b,p}, v_s = Z[s][ze_off + .] (s < S) or y (s == S); zero in the rows of
// points absent from block b and in the padding
int launch_pw_basis_fwd(gpimhip_ctx* h, PwGrid gd, const double* Z, int64_t zw, int64_t ze_off, const double* y, int S,
                        int64_t Nq, int64_t npq, int B, double* E);
// theta->diag_add = jitter_m + noise(theta) again, after launch_pw_set_diag
int launch_pw_reset_diag(gpimhip_ctx* h, ThetaDev* theta, double jitter_m);
// R (S + 1 rows of npq) of one block: row s = Cb[s] + sqrt(diag_add - jitter_s) Eb[s], row S = Eb[S]
int launch_pw_blocks_rhs(gpimhip_ctx* h, const double* Cb, const double* Eb, int S, int64_t Nq, int64_t npq,
                         const ThetaDev* theta, double jitter_s, double* R);
// Cc (S + 1 rows of Nq) of one block from its solutions Al (rows of npq): mean = Eb[S] - diag_add Al[S];
// row v < S = mean + ((diag_add - jitter_s) Al[v] - sqrt(diag_add - jitter_s) Eb[v]), row S = mean
int launch_pw_blocks_combine(gpimhip_ctx* h, const double* Al, const double* Eb, int S, int64_t Nq, int64_t npq,
                             const ThetaDev* theta, double jitter_s, double* Cc);
// out[s] = g[s] (+ sqrt(noise) Z[s][zn_off + .] unless noiseless), mean_out (optional) = g[S]
int launch_pw_blocks_out(gpimhip_ctx* h, const double* g, int64_t M, int S, const double* Z, int64_t zw, int64_t zn_off,
                         int noiseless, const ThetaDev* theta, double* mean_out, double* out);

// ---- draws on a grid with missing points through the bordered reflection blocks (gpimhip_sample_border) ----
// Vectors are block-major: block b at + b v_bs, column c at + c cs (cs = the padded block order).
// mi (M int32) = -1, then mi[miss[j]] = j
int launch_bs_mark(gpimhip_ctx* h, const int64_t* miss, int Mm, int64_t M, int32_t* mi);
// *into = *from if *into == 0; *from = 0  (two status words, one report)
int launch_bs_merge_info(gpimhip_ctx* h, int32_t* from, int32_t* into);
// R[b][s] = (U (1_o (g_s + sqrt(diag_add - jitter_s) Z[s][M + .])))_b for s < S, R[b][S] = ys[b]; zero padding rows p >= Nq
int launch_bs_rhs_fwd(gpimhip_ctx* h, PwGrid gd, const double* g, const double* Z, int64_t zw, int64_t M, const int32_t* mi,
                      const double* ys, const ThetaDev* theta, double jitter_s, int S, int64_t Nq, int64_t np, int B, double* R);
// Y[c][i] = sum_{j <= i} T[i][j] X[c][j], i < n, for ncols (1 .. 8) columns and B lower-triangular matrices T (t_bs apart)
int launch_tri_fwd_multi(gpimhip_ctx* h, const double* T, int64_t ld, int64_t t_bs, int64_t n, int B, const double* X, double* Y,
                         int64_t cs, int64_t v_bs, int ncols);
// row chunks of the transposed sweep: ~np / 8 rows, a multiple of 256 -- a function of the padded order alone
static inline int tri_bwd_rc(int64_t np) {
    const int64_t rc = ((np / 8 + 255) / 256) * 256;
    return (int)(rc < 256 ? 256 : rc);
}
static inline int tri_bwd_chunks(int64_t np) { return (int)((np + tri_bwd_rc(np) - 1) / tri_bwd_rc(np)); }
// Y[c][j] = sum_{i >= j} T[i][j] X[c][i], j < n (X and Y may not alias); part: B x tri_bwd_chunks(np) x pg x np, pg >= ncols
int launch_tri_bwd_multi(gpimhip_ctx* h, const double* T, int64_t ld, int64_t t_bs, int64_t n, int64_t np, int B, const double* X,
                         double* Y, int64_t cs, int64_t v_bs, int ncols, double* part, int pg);
// t[c][j] = sum_b coef_b(j) beta_b[c][q(j)] (S1 columns of mp, zero padding)
int launch_bs_t(gpimhip_ctx* h, const double* beta, int64_t np, int B, int S1, const int32_t* q, const double* coef, int Mm,
                int64_t mp, double* t);
// Al_b[c] -= Y_b v[c] for the columns c0 .. c0 + ncols - 1, rows p < Nq
int launch_bs_yv(gpimhip_ctx* h, const double* Yb, int64_t mp, int64_t np, int64_t Nq, int B, int S1, const double* v, int c0,
                 int ncols, double* Al);
// Cc[b][c] (rows of Nq): (diag_add - jitter_s) Al_b[c] for c < S, ys_b - diag_add Al_b[S] for c == S
int launch_bs_combine(gpimhip_ctx* h, const double* Al, const double* ys, int S, int64_t Nq, int64_t np, int B,
                      const ThetaDev* theta, double jitter_s, double* Cc);
// the two cases of the combination, chosen by mi, and the z_n epilogue (sample.hip: bs_out_kernel)
int launch_bs_out(gpimhip_ctx* h, const double* g2, const double* g, const double* wv, int64_t mp, const int32_t* mi, int64_t M,
                  int S, const double* Z, int64_t zw, int noiseless, const ThetaDev* theta, double jitter_s, double* mean_out,
                  double* out);
