// vgp.hpp -- shared declarations of the multi-output GP (vgp.hip kernels, vgpgp.hip drivers, draws.hip: sample_vgp_*).
#pragma once
#include "common.hpp"

// vgpgp.hip: the argument check of every multi-output entry; vgp_release frees the handle's multi-output workspace
// (gpimhip_destroy)
int vgp_check(gpimhip_ctx* h, const gpimhip_model_t* m, const gpimhip_vgp_t* vg, const double* X, const double* Y, int64_t N);
void vgp_release(gpimhip_ctx* h);

#define VGP_MAXT GPIMHIP_VGP_MAX_TASKS
#define VGP_MAXR GPIMHIP_VGP_MAX_TASKS      // IndexKernel rank <= T
#define VGP_MAXP (4 * VGP_MAXT + GPIMHIP_MAX_DIM + 1 + (VGP_MAXR - 1) * VGP_MAXT)
#define VGP_SWEEPS 12                      // Jacobi sweeps at most (quadratic convergence: T <= 16 needs < 10)

// offsets of the raw vector u = [mu (T) | F (T x R) or r_o (T) | r_v (T, correlated only) | r_l (n_ls) | r_a (T) | r_g]
struct VgpLayout { int mu, scale, diag, ls, noise, P; };
__host__ __device__ inline VgpLayout vgp_layout(const gpimhip_model_t& m, const gpimhip_vgp_t& vg) {
    VgpLayout L;
    const int T = vg.tasks;
    L.mu = 0;
    L.scale = T;
    if (vg.independent) {
        L.diag = T;           // r_o is the diagonal of B
        L.ls = 2 * T;
    } else {
        L.diag = T + T * vg.rank;
        L.ls = L.diag + T;
    }
    L.noise = L.ls + m.n_ls;
    L.P = L.noise + T + 1;
    return L;
}

// state of one evaluation, written by vgp_setup_kernel (device memory)
struct VgpDev {
    double lam[VGP_MAXT];                 // eigenvalues of B~ = the blocks' kernel variances
    double Q[VGP_MAXT * VGP_MAXT];        // eigenvectors, Q[a][t]
    double P[VGP_MAXT * VGP_MAXT];        // S^-1/2 Q
    double B[VGP_MAXT * VGP_MAXT];        // task covariance
    double F[VGP_MAXT * VGP_MAXR];        // IndexKernel factor (correlated model)
    double bdiag[VGP_MAXT], ddiag[VGP_MAXT];   // softplus(r_v or r_o) and its derivative
    double s[VGP_MAXT], sqs[VGP_MAXT];    // noise per task and its square root
    double dsa[VGP_MAXT], dsg;            // d s_a / d r_a, d s_a / d r_g
    double mu[VGP_MAXT];
    double ls[GPIMHIP_MAX_DIM], dls[GPIMHIP_MAX_DIM];
};

// (FinalizeIter::hist_base of launch_vgp_finalize: T x n_ls)
// nrep: the problems per task -- 1 on the dense model, 2^r in reflection mode (h->refl; problem t nrep + b = task t, sign
// pattern b); launch_vgp_finalize takes 0 for the dense model
int launch_vgp_setup(gpimhip_ctx* h, const gpimhip_model_t* m, const gpimhip_vgp_t* vg, const double* u, VgpDev* st, int nrep);
int launch_vgp_project(gpimhip_ctx* h, const double* Y, int64_t N, int T, const VgpDev* st);
// the same two launches with caller-owned results (the multi-output draws, draws.hip: sample_vgp_impl): the T blocks' theta
// into `theta` (T entries) instead of h->theta, and z as plain T x N rows (no padding) instead of h->ypad
int launch_vgp_setup_to(gpimhip_ctx* h, const gpimhip_model_t* m, const gpimhip_vgp_t* vg, const double* u, VgpDev* st,
                        ThetaDev* theta);
int launch_vgp_project_to(gpimhip_ctx* h, const double* Y, int64_t N, int T, const VgpDev* st, double* z);
// uo / border_scal / radd: non-null with a border (BorderWs::uo, scal, rsq)
int launch_vgp_project_refl(gpimhip_ctx* h, const double* Y, int64_t N, int T, int nrep, const double* uo, const VgpDev* st);
int launch_vgp_kbeta(gpimhip_ctx* h, const gpimhip_model_t* m, const double* X, int64_t N, int T, double* kb);
int launch_vgp_kbeta_refl(gpimhip_ctx* h, const gpimhip_model_t* m, const double* X, int64_t N, int T, int nrep, double* kb);
int launch_vgp_finalize(gpimhip_ctx* h, const gpimhip_model_t* m, const gpimhip_vgp_t* vg, int64_t N, const double* kb,
                        const VgpDev* st, double* u, double* adam_m, double* adam_v, int do_adam, AdamStep ast,
                        double* loss_out, double* grad_out, FinalizeIter fi, int nrep, const double* border_scal = nullptr);
// (mean_out or var_out may be null: that half is neither read nor written)
int launch_vgp_combine(gpimhip_ctx* h, int T, int64_t M, const VgpDev* st, const double* mblk, const double* vblk,
                       double* mean_out, double* var_out);
// out[s][i][a] = mu_a + s_a^1/2 sum_t Q_at H[t][s][i]: the latent blocks' draws H (T x S x M) mixed into joint draws of the
// T outputs (S x M x T, task fastest); DESIGN.md section 19
int launch_vgp_sample_mix(gpimhip_ctx* h, int T, int S, int64_t M, const VgpDev* st, const double* H, double* out);
int launch_vgp_group_combine(gpimhip_ctx* h, int T, int nrep, int nb, int64_t ldp, int64_t m0, int64_t mcount, const VgpDev* st,
                             double* mean_out, double* var_out, const double* radd = nullptr, int64_t ldr = 0);
