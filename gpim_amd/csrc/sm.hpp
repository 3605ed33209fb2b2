// sm.hpp -- shared declarations of the spectral-mixture kernel (sm.hip kernels, smgp.hip drivers, draws.hip: sm_family).
#pragma once
#include "common.hpp"

// smgp.hip: the argument check of every spectral-mixture entry.  B = 0: a dense entry point (no reflection mode); B > 0: the
// blocks of a handle in reflection mode.  sm_release: frees the handle's spectral-mixture workspace (gpimhip_destroy)
int sm_check(gpimhip_ctx* h, const gpimhip_sm_t* sm, const double* X, int64_t N, int B = 0);
void sm_release(gpimhip_ctx* h);

#define SM_MAXQ GPIMHIP_SM_MAX_MIXTURES
#define SM_MAXP (2 + SM_MAXQ * (2 * GPIMHIP_MAX_DIM + 1))

// offsets of the raw vector u = [c | r_w (Q) | r_m (Q x D) | r_s (Q x D) | r_n]
struct SmLayout { int Q, D, w, m, s, noise, P; };
__host__ __device__ inline SmLayout sm_layout(const gpimhip_sm_t& sm) {
    SmLayout L;
    L.Q = sm.mixtures;
    L.D = sm.ard ? sm.dim : 1;
    L.w = 1;
    L.m = 1 + L.Q;
    L.s = L.m + L.Q * L.D;
    L.noise = L.s + L.Q * L.D;
    L.P = L.noise + 1;
    return L;
}

// constrained parameters at the current u and their softplus derivatives (sm_setup_kernel, device memory)
struct SmDev {
    double c, noise, dnoise;
    double w[SM_MAXQ], dw[SM_MAXQ];
    double m[SM_MAXQ * GPIMHIP_MAX_DIM], dm[SM_MAXQ * GPIMHIP_MAX_DIM];
    double s[SM_MAXQ * GPIMHIP_MAX_DIM], ds[SM_MAXQ * GPIMHIP_MAX_DIM];
    double kap[SM_MAXQ * GPIMHIP_MAX_DIM];      // 2 pi^2 s^2, per data dimension (isotropic: replicated)
};

// phases: cs[((q * dim + d) * 2 + {0: cos, 1: sin}) * ldc + i] of 2 pi m_qd x_id, zero for n <= i < ldc
int launch_sm_setup(gpimhip_ctx* h, const gpimhip_sm_t* sm, const double* u, const double* P, int64_t n, int64_t ldc,
                    double* cs, const double* y, double* ypad, SmDev* st, ThetaDev* theta);
int launch_sm_kmat(gpimhip_ctx* h, const gpimhip_sm_t* sm, const double* X, int64_t N, const double* csx, int64_t ldx,
                   const double* Z, int64_t M, const double* csz, int64_t ldz, const SmDev* st, double* out, int64_t ld,
                   int64_t rows_pad, int64_t cols_pad, int sym, int lower_only);
int launch_sm_grad(gpimhip_ctx* h, const gpimhip_sm_t* sm, const double* Kinv, int64_t ld, const double* X, int64_t N,
                   const double* csx, int64_t ldx, const double* alpha, const SmDev* st, double* part, double* sums);
int launch_sm_finalize(gpimhip_ctx* h, const gpimhip_sm_t* sm, int64_t N, const double* sums, const SmDev* st, double* u,
                       double* adam_m, double* adam_v, int do_adam, AdamStep ast, double* loss_out, double* grad_out,
                       FinalizeIter fi, const double* ones = nullptr, int64_t n_total = 0, const double* border_scal = nullptr);
int launch_sm_mean(gpimhip_ctx* h, const double* mtmp, int64_t n, const SmDev* st, double* mean_out);

// posterior draws.  st: TWO SmDev -- st[0] the parameters at u (and theta: sum w, noise, diag_add =
// noise), st[1] the same with `other` in place of the noise, for a build with another diagonal term (K_b + d I; none)
int launch_sm_params(gpimhip_ctx* h, const gpimhip_sm_t* sm, const double* u, SmDev* st, ThetaDev* theta, double other);
// out = y - c
int launch_sm_centre(gpimhip_ctx* h, const double* y, int64_t n, const SmDev* st, double* out);
// launch_pw_cross_apply (sample.hpp) for this kernel; csg (leading dimension ldg >= M), csx (ldx >= N): the phases of G and of
// the training rows Xt by launch_sm_setup; the constant mean is added to mean_out and to every draw
int launch_sm_cross_apply(gpimhip_ctx* h, const gpimhip_sm_t* sm, const double* G, int64_t M, const double* csg, int64_t ldg,
                          const double* Xt, int64_t N, const double* csx, int64_t ldx, const SmDev* st, const ThetaDev* theta,
                          const double* Al, int64_t npt, int S, int s0, const double* g, const double* Z, int64_t zw,
                          int64_t zn_off, int noiseless, double* mean_out, double* out);

// reflection blocks (handle in reflection mode, h->nbatch = 2^r blocks on the fundamental domain):
// phases of the centred coordinates, r_b = ys_b - c ones_b (ys, ones: B x n; ypad: B x ldc), the blocks K_s (out_bs apart)
// or K_s(Xq, Z) * scale, the contraction with one record per (block, lower tile), and mean += c
int launch_sm_setup_refl(gpimhip_ctx* h, const gpimhip_sm_t* sm, const double* u, const double* P, int64_t n, int64_t ldc,
                         double* cs, const double* ys, const double* ones, double* ypad, SmDev* st, ThetaDev* theta);
int launch_sm_kmat_refl(gpimhip_ctx* h, const gpimhip_sm_t* sm, const double* X, int64_t N, const double* csx, int64_t ldx,
                        const double* Z, int64_t M, const double* csz, int64_t ldz, const SmDev* st, double* out, int64_t ld,
                        int64_t out_bs, int64_t rows_pad, int64_t cols_pad, int sym, int lower_only, double scale);
int launch_sm_grad_refl(gpimhip_ctx* h, const gpimhip_sm_t* sm, const double* Kinv, int64_t ld, const double* X, int64_t N,
                        const double* csx, int64_t ldx, const double* alpha, const SmDev* st, double* part, double* sums);
int launch_sm_addc(gpimhip_ctx* h, double* mean, int64_t n, const SmDev* st);
