// vgp.hip -- the exact multi-output (vector-valued) GP of the reference's vreconstructor (gpim/gpreg/vgpr.py), reduced to
// T ordinary single-task GPs that share X and run in lock-step on the batched engine (vgpgp.hip: vgp_iter).
//
// Model (GPyTorch semantics, vgpr.py:286-354): C = B (x) K + S (x) I_N, task-major vec(Y - mu), S = diag(s).
//   B~ = S^-1/2 B S^-1/2 = Q diag(lambda) Q^T,  P = S^-1/2 Q   ->   C = (S^1/2 Q (x) I)(diag(lambda) (x) K + I)(Q^T S^1/2 (x) I)
// so block t is A_t = lambda_t K + I (kernel variance lambda_t, noise 1) with targets z_t = sum_a P_at (y_a - mu_a).
//   vgp_setup_kernel     raw u -> B, s, mu, l; Jacobi eigen-decomposition of B~ (one workgroup); the blocks' theta
//   vgp_project_kernel   z_t into the padded per-problem right-hand sides of the batched engine
//   vgp_kbeta_kernel     (K beta_t)_i for all t (K regenerated, variance 1): the bilinear forms beta_t^T K beta_t'
//   vgp_finalize_kernel  loss, gradient (no eigenvector derivatives), chain rule to u, Adam step, history row
//   vgp_combine_kernel   the T x T mix of the blocks' posterior mean / variance
//   vgp_sample_mix_kernel  the same mix for joint draws: the T latent blocks' draws into S x M x T
// Reflection mode (gpimhip_set_reflection): on a complete grid each block A_t splits further into the
// 2^r reflection blocks A_{t,b} = lambda_t K_b + I of engine.hip's symmetry-reduced model; problem t 2^r + b of the batch is
// task t with sign pattern b, and each task's sums run over its 2^r consecutive problems:
//   vgp_project_refl_kernel   z_{t,b} = sum_a P_at (ys_{a,b} - mu_a u_b), u_b = U 1 (with a border: U 1_o)
//   vgp_kbeta_refl_kernel     K_b beta_{t,b} for all t (K_b regenerated as kmat_refl_kernel builds it, variance 1)
//   vgp_finalize_kernel<1>    the finalize step with the per-task sums over the blocks and the grid's N
//   vgp_group_combine_kernel  the blocks' posterior summed per task, then the mix of vgp_combine_kernel
// With a border (gpimhip_set_border; DESIGN.md section 13: an incomplete grid) the launches of border.hip correct beta and
// the blocks' inverses per task between the K^-1 product and the gradient contraction; here only three things change: the
// task means enter through U 1_o, the finalize step adds -|v_t|^2 and log det S_t per task, and the prediction adds
// |sum_b Y_{t,b}^T k*_{t,b}|^2 to task t's variance before the mix.
// Every reduction has a fixed shape: results are bit-reproducible run to run.
#include "kfun.hpp"
#include "refl.hpp"
#include "vgp.hpp"

// softplus as torch.nn.functional.softplus (beta 1, threshold 20) and its derivative
__device__ __forceinline__ double vgp_softplus(double x) { return x > 20.0 ? x : log1p(exp(x)); }
__device__ __forceinline__ double vgp_sigmoid(double x) { return 1.0 / (1.0 + exp(-x)); }
__device__ __forceinline__ double vgp_dsoftplus(double x) { return x > 20.0 ? 1.0 : vgp_sigmoid(x); }

__device__ __forceinline__ void vgp_lengthscale(const gpimhip_model_t& m, int ls_softplus, int k, double r, double& l, double& dl) {
    if (ls_softplus) {
        l = vgp_softplus(r);
        dl = vgp_dsoftplus(r);
    } else {      // gpytorch.constraints.Interval: sigmoid(r) * (hi - lo) + lo
        const double s = vgp_sigmoid(r);
        l = s * (m.ls_hi[k] - m.ls_lo[k]) + m.ls_lo[k];
        dl = (m.ls_hi[k] - m.ls_lo[k]) * s * (1.0 - s);
    }
}

// ------------------------------------------------------------------------------------------
// setup: one workgroup of 64 threads
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void vgp_setup_kernel(gpimhip_model_t m, gpimhip_vgp_t vg, const double* __restrict__ u,
                                                       VgpDev* __restrict__ st, ThetaDev* __restrict__ theta, int nrep) {
    __shared__ double A[VGP_MAXT][VGP_MAXT + 1];
    __shared__ double V[VGP_MAXT][VGP_MAXT + 1];
    __shared__ double cs[2];
    __shared__ int done;
    const int tid = threadIdx.x, T = vg.tasks;
    const VgpLayout L = vgp_layout(m, vg);
    if (tid < T) {
        const int a = tid;
        st->mu[a] = u[L.mu + a];
        double sa = 0.0;
        {
            const double ra = u[L.noise + a], rg = u[L.noise + T];
            sa = (1e-4 + vgp_softplus(ra)) + (1e-4 + vgp_softplus(rg));
            st->dsa[a] = vgp_dsoftplus(ra);
            if (a == 0) st->dsg = vgp_dsoftplus(rg);
        }
        st->s[a] = sa;
        st->sqs[a] = sqrt(sa);
        const double rd = u[(vg.independent ? L.scale : L.diag) + a];
        st->ddiag[a] = vgp_dsoftplus(rd);
        st->bdiag[a] = vgp_softplus(rd);
        for (int r = 0; r < (vg.independent ? 0 : vg.rank); ++r) st->F[a * VGP_MAXR + r] = u[L.scale + a * vg.rank + r];
    }
    if (tid < m.n_ls) {
        double l, dl;
        vgp_lengthscale(m, vg.ls_softplus, tid, u[L.ls + tid], l, dl);
        st->ls[tid] = l;
        st->dls[tid] = dl;
    }
    __syncthreads();
    // B and B~ (lane a owns row a)
    if (tid < T) {
        const int a = tid;
        for (int b = 0; b < T; ++b) {
            double bab = 0.0;
            if (!vg.independent)
                for (int r = 0; r < vg.rank; ++r) bab = fma(st->F[a * VGP_MAXR + r], st->F[b * VGP_MAXR + r], bab);
            if (a == b) bab += st->bdiag[a];
            st->B[a * VGP_MAXT + b] = bab;
            A[a][b] = bab / (st->sqs[a] * st->sqs[b]);
            V[a][b] = (a == b) ? 1.0 : 0.0;
        }
    }
    __syncthreads();
    // cyclic Jacobi, pairs (p, q) in row order, at most VGP_SWEEPS sweeps; a sweep starts only while the off-diagonal part
    // is above 1e-40 of the diagonal's (relative to double precision: exactly converged) -- a function of the input alone
    for (int sweep = 0; sweep < VGP_SWEEPS; ++sweep) {
        if (tid == 0) {
            double off = 0.0, dia = 0.0;
            for (int p = 0; p < T; ++p) {
                dia += A[p][p] * A[p][p];
                for (int q = p + 1; q < T; ++q) off += A[p][q] * A[p][q];
            }
            done = !(off > 1e-40 * dia);
        }
        __syncthreads();
        if (done) break;
        for (int p = 0; p < T - 1; ++p)
            for (int q = p + 1; q < T; ++q) {
                if (tid == 0) {
                    const double apq = A[p][q];
                    double c = 1.0, s = 0.0;
                    if (apq != 0.0) {
                        const double th = (A[q][q] - A[p][p]) / (2.0 * apq);
                        const double at = fabs(th);
                        double t = at > 1e150 ? 0.5 / at : 1.0 / (at + sqrt(fma(th, th, 1.0)));
                        if (th < 0.0) t = -t;
                        c = 1.0 / sqrt(fma(t, t, 1.0));
                        s = t * c;
                    }
                    cs[0] = c;
                    cs[1] = s;
                }
                __syncthreads();
                const double c = cs[0], s = cs[1];
                if (s != 0.0 && tid < T) {
                    const int k = tid;
                    const double t = s / c;
                    if (k == p) {
                        const double apq = A[p][q];
                        A[p][p] = A[p][p] - t * apq;
                        A[q][q] = A[q][q] + t * apq;
                        A[p][q] = 0.0;
                        A[q][p] = 0.0;
                    } else if (k != q) {
                        const double akp = A[k][p], akq = A[k][q];
                        const double nkp = c * akp - s * akq, nkq = s * akp + c * akq;
                        A[k][p] = nkp; A[p][k] = nkp;
                        A[k][q] = nkq; A[q][k] = nkq;
                    }
                    const double vkp = V[k][p], vkq = V[k][q];
                    V[k][p] = c * vkp - s * vkq;
                    V[k][q] = s * vkp + c * vkq;
                }
                __syncthreads();
            }
    }
    // lambda, Q, P; the blocks' theta (variance lambda_t, the shared lengthscales, noise 1, no jitter)
    if (tid < T) {
        const int t = tid;
        const double lam = A[t][t];
        st->lam[t] = lam;
        for (int a = 0; a < T; ++a) {
            st->Q[a * VGP_MAXT + t] = V[a][t];
            st->P[a * VGP_MAXT + t] = V[a][t] / st->sqs[a];
        }
        ThetaDev th;
        th.var = lam;
        for (int k = 0; k < GPIMHIP_MAX_DIM; ++k) {
            th.ls[k] = (k < m.dim) ? st->ls[(m.n_ls == 1) ? 0 : k] : 1.0;
            th.inv_ls[k] = 1.0 / th.ls[k];
            th.dls_du[k] = 0.0;
        }
        th.noise = 1.0;
        th.alpha = 1.0;
        th.diag_add = 1.0;
        th.dvar_du = th.dnoise_du = th.dalpha_du = 0.0;
        for (int b = 0; b < nrep; ++b) theta[t * nrep + b] = th;      // (reflection mode: one problem per sign pattern)
    }
}

// z_t = sum_a P_at (y_a - mu_a), zero on the padding rows.  grid (np / 256, T); Y: T x N (task-major)
__global__ __launch_bounds__(256) void vgp_project_kernel(const double* __restrict__ Y, int64_t N, int64_t np, int T,
                                                          const VgpDev* __restrict__ st, double* __restrict__ z) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int t = blockIdx.y;
    if (i >= np) return;
    double v = 0.0;
    if (i < N)
        for (int a = 0; a < T; ++a) v = fma(st->P[a * VGP_MAXT + t], Y[(int64_t)a * N + i] - st->mu[a], v);
    z[(int64_t)t * np + i] = v;
}

// kb[t][i] = sum_j k(x_i, x_j) beta_t[j] (variance 1) for i < N.  One workgroup: 64 rows; the columns go through LDS 256 at
// a time, wave w taking the fourth w of them; the four waves' sums are added in wave order.
template <int KIND>
__global__ __launch_bounds__(256) void vgp_kbeta_kernel(const double* __restrict__ X, int64_t N, int d, int64_t np, int T,
                                                        const ThetaDev* __restrict__ th, const double* __restrict__ beta,
                                                        double* __restrict__ kb) {
    __shared__ double xs[256][5];
    __shared__ double bs[VGP_MAXT][256];
    double (*red)[VGP_MAXT][64] = reinterpret_cast<double (*)[VGP_MAXT][64]>(&bs[0][0]);     // after the column loop
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const ThetaDev t0 = th[0];
    const int64_t i = (int64_t)blockIdx.x * 64 + lane;
    double a[GPIMHIP_MAX_DIM], an = 0.0;
#pragma unroll
    for (int k = 0; k < GPIMHIP_MAX_DIM; ++k) {
        a[k] = (k < d && i < N) ? X[i * d + k] / t0.ls[k] : 0.0;
        an += a[k] * a[k];
    }
    double acc[VGP_MAXT];
#pragma unroll
    for (int t = 0; t < VGP_MAXT; ++t) acc[t] = 0.0;
    for (int64_t j0 = 0; j0 < N; j0 += 256) {
        __syncthreads();
        {
            const int64_t j = j0 + tid;
            double s2 = 0.0;
            for (int k = 0; k < GPIMHIP_MAX_DIM; ++k) {
                const double v = (k < d && j < N) ? X[j * d + k] / t0.ls[k] : 0.0;
                xs[tid][k] = v;
                s2 += v * v;
            }
            xs[tid][4] = s2;
            for (int t = 0; t < T; ++t) bs[t][tid] = (j < N) ? beta[(int64_t)t * np + j] : 0.0;
        }
        __syncthreads();
        const int jn = (int)((N - j0 < 256) ? (N - j0) : 256);
        for (int jj = wave * 64; jj < wave * 64 + 64 && jj < jn; ++jj) {
            double dot = a[0] * xs[jj][0];
            dot = fma(a[1], xs[jj][1], dot);
            dot = fma(a[2], xs[jj][2], dot);
            dot = fma(a[3], xs[jj][3], dot);
            const double r2 = clamp0_nan((an - 2.0 * dot) + xs[jj][4]);
            const double k = kfun_value<KIND>(r2, 1.0);
#pragma unroll
            for (int t = 0; t < VGP_MAXT; ++t)
                if (t < T) acc[t] = fma(k, bs[t][jj], acc[t]);
        }
    }
    __syncthreads();
#pragma unroll
    for (int t = 0; t < VGP_MAXT; ++t)
        if (t < T) red[wave][t][lane] = acc[t];
    __syncthreads();
    if (wave == 0 && i < N)
        for (int t = 0; t < T; ++t) kb[(int64_t)t * np + i] = (red[0][t][lane] + red[1][t][lane]) + (red[2][t][lane] + red[3][t][lane]);
}

// reflection mode: z_{t,b} = sum_a P_at (ys_{a,b} - mu_a u_b) with u_b = U 1 = sqrt(B) w_0 in block 0 and 0 in the others;
// zero on the padding rows and where the point does not exist in the block (w_b = 0: an identity row of A_{t,b}).
// grid (np / 256, T nrep); Y: T x nrep x N (task-major, then sign pattern); wts: the weights of block b at b N (or null: all 1)
// uo (nrep x N, or null): with a border, u_b = (U 1_o)_b -- the means enter at the observed points only
__global__ __launch_bounds__(256) void vgp_project_refl_kernel(const double* __restrict__ Y, int64_t N, int64_t np, int T,
                                                               int nrep, const double* __restrict__ wts,
                                                               const double* __restrict__ uo,
                                                               const VgpDev* __restrict__ st, double* __restrict__ z) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int p = blockIdx.y, t = p / nrep, b = p % nrep;
    if (i >= np) return;
    double v = 0.0;
    if (i < N) {
        const double wb = wts ? wts[(int64_t)b * N + i] : 1.0;
        const double ub = uo ? uo[(int64_t)b * N + i] : (b == 0) ? sqrt((double)nrep) * wb : 0.0;
        if (wb != 0.0)
            for (int a = 0; a < T; ++a)
                v = fma(st->P[a * VGP_MAXT + t], Y[((int64_t)a * nrep + b) * N + i] - st->mu[a] * ub, v);
    }
    z[(int64_t)p * np + i] = v;
}

// reflection mode: kb[p][i] = sum_j K_b[i, j] beta_p[j] for the T problems p = t nrep + b of block b (grid.y), i < N, with
// K_b[i, j] = w_b,i w_b,j sum_g chi_b(g) k(x_i, g x_j) at variance 1 -- regenerated the way kmat_refl_kernel builds it (the
// rows of absent points come out 0; their beta is 0).  N^2 kernel evaluations over all blocks, as vgp_kbeta_kernel does
// on the dense model.  One workgroup: 64 rows; the columns go through LDS 256 at a time, wave w taking the fourth w of
// them; the four waves' sums are added in wave order.
template <int KIND>
__global__ __launch_bounds__(256) void vgp_kbeta_refl_kernel(const double* __restrict__ X, int64_t N, int d, int64_t np, int T,
                                                             int nrep, ReflArgs refl, const ThetaDev* __restrict__ th,
                                                             const double* __restrict__ beta, double* __restrict__ kb) {
    __shared__ double xs[256][GPIMHIP_MAX_DIM];
    __shared__ double ws[256];
    __shared__ double bs[VGP_MAXT][256];
    double (*red)[VGP_MAXT][64] = reinterpret_cast<double (*)[VGP_MAXT][64]>(&bs[0][0]);     // after the column loop
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.y;
    const int sg = refl_sign_dims(refl.mask, b);
    const double* wts = refl.wts ? refl.wts + (int64_t)b * N : nullptr;
    const ThetaDev t0 = th[0];
    const int64_t i = (int64_t)blockIdx.x * 64 + lane;
    double a[GPIMHIP_MAX_DIM], cz[GPIMHIP_MAX_DIM];
#pragma unroll
    for (int k = 0; k < GPIMHIP_MAX_DIM; ++k) {
        a[k] = (k < d && i < N) ? X[i * d + k] / t0.ls[k] : 0.0;
        cz[k] = (k < d) ? refl.twoc[k] / t0.ls[k] : 0.0;
    }
    const double wi = (wts && i < N) ? wts[i] : 1.0;
    double acc[VGP_MAXT];
#pragma unroll
    for (int t = 0; t < VGP_MAXT; ++t) acc[t] = 0.0;
    for (int64_t j0 = 0; j0 < N; j0 += 256) {
        __syncthreads();
        {
            const int64_t j = j0 + tid;
#pragma unroll
            for (int k = 0; k < GPIMHIP_MAX_DIM; ++k) xs[tid][k] = (k < d && j < N) ? X[j * d + k] / t0.ls[k] : 0.0;
            ws[tid] = (wts && j < N) ? wts[j] : 1.0;
            for (int t = 0; t < T; ++t) bs[t][tid] = (j < N) ? beta[((int64_t)t * nrep + b) * np + j] : 0.0;
        }
        __syncthreads();
        const int jn = (int)((N - j0 < 256) ? (N - j0) : 256);
        for (int jj = wave * 64; jj < wave * 64 + 64 && jj < jn; ++jj) {
            ReflPair p;
#pragma unroll
            for (int k = 0; k < GPIMHIP_MAX_DIM; ++k) {
                const double dm = a[k] - xs[jj][k], dp = (a[k] + xs[jj][k]) - cz[k];
                p.dm2[k] = dm * dm;
                p.dp2[k] = dp * dp;
            }
            double s = 0.0;
            refl_for_each(p, refl.mask, sg, [&](int, double chi, double r2) { s = fma(chi, kfun_value<KIND>(r2, 1.0), s); });
            const double k = s * ws[jj];
#pragma unroll
            for (int t = 0; t < VGP_MAXT; ++t)
                if (t < T) acc[t] = fma(k, bs[t][jj], acc[t]);
        }
    }
    __syncthreads();
#pragma unroll
    for (int t = 0; t < VGP_MAXT; ++t)
        if (t < T) red[wave][t][lane] = acc[t];
    __syncthreads();
    if (wave == 0 && i < N)
        for (int t = 0; t < T; ++t)
            kb[((int64_t)t * nrep + b) * np + i] = wi * ((red[0][t][lane] + red[1][t][lane]) + (red[2][t][lane] + red[3][t][lane]));
}

// NQ block sums of 256 threads at once (fixed tree); arr: NQ x 256 doubles of LDS; results in out[0 .. NQ)
template <int NQ>
__device__ __forceinline__ void vgp_sum_multi(const double* v, double* arr, double* out) {
    const int tid = threadIdx.x;
    __syncthreads();
#pragma unroll
    for (int q = 0; q < NQ; ++q) arr[q * 256 + tid] = v[q];
    __syncthreads();
    if (tid < 64) {
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            const double* p = arr + q * 256;
            double x = (p[tid] + p[tid + 128]) + (p[tid + 64] + p[tid + 192]);
            x += __shfl_down(x, 32);
            x += __shfl_down(x, 16);
            x += __shfl_down(x, 8);
            x += __shfl_down(x, 4);
            x += __shfl_down(x, 2);
            x += __shfl_down(x, 1);
            if (tid == 0) out[q] = x;
        }
    }
    __syncthreads();
}

// ------------------------------------------------------------------------------------------
// finalize: one workgroup of 256 threads
//   per block t:  Sg_t[0..6] = the gradient contraction of grad_reduce_kernel (variance-1 kernel: Sg_t[0] = tr(M_t K) -
//                 beta_t^T K beta_t, Sg_t[5] = tr(M_t) - |beta_t|^2, Sg_t[1+k] the lengthscale sums), q_t = |L_t^-1 z_t|^2,
//                 lg_t = sum log diag L_t, sig_t = sum_i beta_t,i;  pairs: H_tt' = beta_t^T beta_t', G_tt' = beta_t^T K beta_t'
//   dL/dB_ab = 1/2 [sum_t P_at P_bt tr(M_t K) - (P G P^T)_ab],  dL/ds_a = 1/2 [sum_t P_at^2 tr(M_t) - (P H P^T)_aa]
//   dL/dl_k  = 1/2 sum_t lambda_t Sg_t[1+k] / l_k,            dL/dmu_a = -sum_t P_at sig_t
// REFL (reflection mode): task t is the nrep problems t nrep .. t nrep + nrep - 1; every per-task quantity is the sum over
// them (each thread runs through the blocks in order before the fixed tree), sig_t = sum_b u_b^T beta_{t,b} =
// sqrt(nrep) w_0^T beta_{t,0}; ntot = the grid's N (the dense model: ntot = N)
// bscal (T x 2, or null): with a border, |v_t|^2 and sum log diag chol(S_t) -- q_t loses the first, lg_t gains the second
// (beta is the corrected one, zero at the missing points in the original basis: sig_t, H and G need nothing else)
// ------------------------------------------------------------------------------------------
template <bool REFL>
__global__ __launch_bounds__(256) void vgp_finalize_kernel(gpimhip_model_t m, gpimhip_vgp_t vg, int64_t N, int64_t ntot,
                                                           int64_t np, int nb, int ntile, int nrep, const double* __restrict__ wts,
                                                           const double* __restrict__ bscal,
                                                           const double* __restrict__ grad_part,
                                                           const double* __restrict__ z, const double* __restrict__ logdet_part,
                                                           const double* __restrict__ beta, const double* __restrict__ kb,
                                                           const VgpDev* __restrict__ st, double* __restrict__ u,
                                                           double* __restrict__ adam_m, double* __restrict__ adam_v, int do_adam,
                                                           AdamStep ast, double* __restrict__ loss_out,
                                                           double* __restrict__ grad_out, double* __restrict__ hist_row,
                                                           FinalizeIter fi, int32_t* __restrict__ info) {
    __shared__ double arr[8 * 256];
    __shared__ double Sg[VGP_MAXT][8];           // [0..6] contraction, [7] q_t
    __shared__ double lgs[VGP_MAXT][2];          // lg_t, sig_t
    __shared__ double H[VGP_MAXT][VGP_MAXT], G[VGP_MAXT][VGP_MAXT];
    __shared__ double Xg[VGP_MAXT][VGP_MAXT], Xh[VGP_MAXT][VGP_MAXT];
    __shared__ double GB[VGP_MAXT][VGP_MAXT], Gs[VGP_MAXT];
    __shared__ double gsh[VGP_MAXP];
    __shared__ int skip;
    const int tid = threadIdx.x, T = vg.tasks;
    const VgpLayout L = vgp_layout(m, vg);
    for (int t = 0; t < T; ++t) {
        double v[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        double w[2] = {0, 0};
        if (REFL) {
            for (int b = 0; b < nrep; ++b) {
                const int64_t p = (int64_t)t * nrep + b;
                const double* gp = grad_part + p * ntile * 8;
                for (int q = tid; q < ntile; q += 256)
                    for (int k = 0; k < 7; ++k) v[k] += gp[(int64_t)q * 8 + k];
                const double* zt = z + p * np;
                for (int64_t i = tid; i < np; i += 256) v[7] = fma(zt[i], zt[i], v[7]);
                for (int k = tid; k < nb; k += 256) w[0] += logdet_part[p * nb + k];
            }
            const double* bt = beta + (int64_t)t * nrep * np;
            const double sq = sqrt((double)nrep);
            for (int64_t i = tid; i < N; i += 256) w[1] = fma(sq * (wts ? wts[i] : 1.0), bt[i], w[1]);
            vgp_sum_multi<8>(v, arr, &Sg[t][0]);
            vgp_sum_multi<2>(w, arr, &lgs[t][0]);
            continue;
        }
        const double* gp = grad_part + (int64_t)t * ntile * 8;
        for (int q = tid; q < ntile; q += 256)
            for (int k = 0; k < 7; ++k) v[k] += gp[(int64_t)q * 8 + k];
        const double* zt = z + (int64_t)t * np;
        for (int64_t i = tid; i < np; i += 256) v[7] = fma(zt[i], zt[i], v[7]);
        vgp_sum_multi<8>(v, arr, &Sg[t][0]);
        for (int k = tid; k < nb; k += 256) w[0] += logdet_part[(int64_t)t * nb + k];
        const double* bt = beta + (int64_t)t * np;
        for (int64_t i = tid; i < N; i += 256) w[1] += bt[i];
        vgp_sum_multi<2>(w, arr, &lgs[t][0]);
    }
    // pairs t <= t', four at a time: H and G
    {
        const int npair = T * (T + 1) / 2;
        for (int p0 = 0; p0 < npair; p0 += 4) {
            double v[8] = {0, 0, 0, 0, 0, 0, 0, 0};
            int pt[4], pu[4];
            for (int e = 0; e < 4; ++e) {
                int q = p0 + e, t = 0;
                if (q >= npair) { pt[e] = -1; pu[e] = -1; continue; }
                while (q >= T - t) { q -= T - t; ++t; }
                pt[e] = t; pu[e] = t + q;
                double h = 0.0, g = 0.0;
                if (REFL) {          // H_tt' = sum_b beta_{t,b}^T beta_{t',b}, G_tt' = sum_b beta_{t,b}^T K_b beta_{t',b}
                    for (int b = 0; b < nrep; ++b) {
                        const double* bt = beta + ((int64_t)t * nrep + b) * np;
                        const double* bu = beta + ((int64_t)(t + q) * nrep + b) * np;
                        const double* ku = kb + ((int64_t)(t + q) * nrep + b) * np;
                        for (int64_t i = tid; i < N; i += 256) {
                            h = fma(bt[i], bu[i], h);
                            g = fma(bt[i], ku[i], g);
                        }
                    }
                } else {
                    const double* bt = beta + (int64_t)t * np;
                    const double* bu = beta + (int64_t)(t + q) * np;
                    const double* ku = kb + (int64_t)(t + q) * np;
                    for (int64_t i = tid; i < N; i += 256) {
                        h = fma(bt[i], bu[i], h);
                        g = fma(bt[i], ku[i], g);
                    }
                }
                v[2 * e] = h;
                v[2 * e + 1] = g;
            }
            double out[8];
            __shared__ double outs[8];
            vgp_sum_multi<8>(v, arr, outs);
            for (int e = 0; e < 8; ++e) out[e] = outs[e];
            if (tid == 0)
                for (int e = 0; e < 4; ++e) {
                    if (pt[e] < 0) continue;
                    H[pt[e]][pu[e]] = H[pu[e]][pt[e]] = out[2 * e];
                    G[pt[e]][pu[e]] = G[pu[e]][pt[e]] = out[2 * e + 1];
                }
            __syncthreads();
        }
    }
    if (fi.iter) {       // (every thread reads the counter here; thread 0 advances it after the last barrier below)
        const int it = *fi.iter;
        ast.lr_over_bc1 = fi.bc[it];
        ast.bc2_sqrt = fi.bc[fi.T + it];
        if (tid == 0) {
            // a factorisation of this training loop failed: u, the Adam state and the history stay as the previous
            // iteration left them (the reference raises inside torch.linalg.cholesky there)
            skip = *info != 0;
            if (skip) atomicMin(info + 1, it);
        }
    } else if (tid == 0) {
        skip = 0;
    }
    __syncthreads();
    if (skip) return;
    const double inv_nt = 1.0 / ((double)ntot * (double)T);
    // (P G)_{a t'} -> X, then dL/dB and dL/ds
    if (tid < T * T) {
        const int a = tid / T, c = tid % T;
        double xg = 0.0, xh = 0.0;
        for (int t = 0; t < T; ++t) {
            xg = fma(st->P[a * VGP_MAXT + t], G[t][c], xg);
            xh = fma(st->P[a * VGP_MAXT + t], H[t][c], xh);
        }
        Xg[a][c] = xg;
        Xh[a][c] = xh;
    }
    __syncthreads();
    if (tid < T * T) {
        const int a = tid / T, b = tid % T;
        double tr = 0.0, pg = 0.0;
        for (int t = 0; t < T; ++t) {
            const double pat = st->P[a * VGP_MAXT + t], pbt = st->P[b * VGP_MAXT + t];
            tr = fma(pat * pbt, Sg[t][0] + G[t][t], tr);
            pg = fma(Xg[a][t], pbt, pg);
        }
        GB[a][b] = 0.5 * (tr - pg);
        if (a == b) {
            double trm = 0.0, ph = 0.0;
            for (int t = 0; t < T; ++t) {
                const double pat = st->P[a * VGP_MAXT + t];
                trm = fma(pat * pat, Sg[t][5] + H[t][t], trm);
                ph = fma(Xh[a][t], pat, ph);
            }
            Gs[a] = 0.5 * (trm - ph);
        }
    }
    __syncthreads();
    // gradient entry per thread (u layout: vgp_layout)
    if (tid < L.P) {
        const int p = tid;
        double g = 0.0;
        if (p < L.mu + T) {
            const int a = p - L.mu;
            for (int t = 0; t < T; ++t) g = fma(st->P[a * VGP_MAXT + t], lgs[t][1], g);
            g = -g;
        } else if (vg.independent && p < L.scale + T) {
            const int a = p - L.scale;
            g = GB[a][a] * st->ddiag[a];
        } else if (!vg.independent && p < L.scale + T * vg.rank) {
            const int a = (p - L.scale) / vg.rank, r = (p - L.scale) % vg.rank;
            for (int b = 0; b < T; ++b) g = fma(GB[a][b] + GB[b][a], st->F[b * VGP_MAXR + r], g);
        } else if (!vg.independent && p < L.diag + T) {
            const int a = p - L.diag;
            g = GB[a][a] * st->ddiag[a];
        } else if (p < L.ls + m.n_ls) {
            const int k = p - L.ls;
            double s = 0.0;
            for (int t = 0; t < T; ++t) {
                double sk = Sg[t][1 + k];
                if (m.n_ls == 1) {
                    sk = 0.0;
                    for (int q = 0; q < m.dim; ++q) sk += Sg[t][1 + q];
                }
                s = fma(st->lam[t], sk, s);
            }
            g = 0.5 * s / st->ls[k] * st->dls[k];
        } else if (p < L.noise + T) {
            const int a = p - L.noise;
            g = Gs[a] * st->dsa[a];
        } else {
            double s = 0.0;
            for (int a = 0; a < T; ++a) s += Gs[a];
            g = s * st->dsg;
        }
        g *= inv_nt;
        gsh[p] = g;
        if (grad_out) grad_out[p] = g;
        if (do_adam) {       // torch.optim.Adam, the expressions of theta.hpp: finalize_step_ws
            double mm = adam_m[p], vv = adam_v[p];
            mm = mm + (g - mm) * (1.0 - ast.beta1);
            vv = vv * ast.beta2 + (1.0 - ast.beta2) * g * g;
            const double denom = sqrt(vv) / ast.bc2_sqrt + ast.eps;
            u[p] = u[p] + (-ast.lr_over_bc1) * (mm / denom);
            adam_m[p] = mm;
            adam_v[p] = vv;
        }
    }
    __syncthreads();
    if (tid != 0) return;
    double slog = 0.0, lg = 0.0, q2 = 0.0;
    for (int a = 0; a < T; ++a) slog += log(st->s[a]);
    for (int t = 0; t < T; ++t) {
        lg += lgs[t][0];
        q2 += Sg[t][7];
        if (REFL && bscal) {
            lg += bscal[2 * t + 1];
            q2 -= bscal[2 * t];
        }
    }
    const double loss = (0.5 * (double)ntot * slog + lg + 0.5 * q2) * inv_nt + 0.5 * 1.8378770664093453;
    int it = 0;
    if (fi.iter) {
        it = *fi.iter;
        loss_out = fi.loss_base ? fi.loss_base + it : nullptr;
        hist_row = fi.hist_base ? fi.hist_base + (int64_t)it * m.n_ls : nullptr;
        *fi.iter = it + 1;
    }
    if (loss_out) *loss_out = loss;
    if (do_adam && hist_row)
        for (int k = 0; k < m.n_ls; ++k) {
            double l, dl;
            vgp_lengthscale(m, vg.ls_softplus, k, u[L.ls + k], l, dl);
            hist_row[k] = l;
        }
}

// mean[j][a] = mu_a + s_a^1/2 sum_t Q_at mean_t[j];  var[j][a] = s_a sum_t Q_at^2 var_t[j]  (var_t: the block's predictive
// variance, noise 1 included; sum_t Q_at^2 = 1 turns B_aa + s_a - s_a sum_t Q_at^2 q_t into this form).  Outputs M x T.
__global__ __launch_bounds__(256) void vgp_combine_kernel(int T, int64_t M, const VgpDev* __restrict__ st,
                                                          const double* __restrict__ mblk, const double* __restrict__ vblk,
                                                          double* __restrict__ mean_out, double* __restrict__ var_out) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= M) return;
    double mb[VGP_MAXT], vb[VGP_MAXT];
#pragma unroll
    for (int t = 0; t < VGP_MAXT; ++t) {
        mb[t] = (t < T && mean_out) ? mblk[(int64_t)t * M + j] : 0.0;
        vb[t] = (t < T && var_out) ? vblk[(int64_t)t * M + j] : 0.0;
    }
    for (int a = 0; a < T; ++a) {
        double mu = 0.0, v = 0.0;
#pragma unroll
        for (int t = 0; t < VGP_MAXT; ++t)
            if (t < T) {
                const double q = st->Q[a * VGP_MAXT + t];
                mu = fma(q, mb[t], mu);
                v = fma(q * q, vb[t], v);
            }
        if (mean_out) mean_out[j * T + a] = st->mu[a] + st->sqs[a] * mu;
        if (var_out) var_out[j * T + a] = st->s[a] * v;
    }
}

// ------------------------------------------------------------------------------------------
// vgp_sample_mix_kernel: out[s][i][a] = mu_a + s_a^1/2 sum_t Q_at H[t][s][i].  HBM-bound: every entry
// of H is read once and every entry of out written once, 16 T S M bytes.  One workgroup = VM_PTS consecutive points of one
// draw: lane i reads its T latent values along i (coalesced, 512 bytes per wave and block), forms the T outputs with t
// ascending (the bits depend on the inputs alone) and parks them in LDS as tile[a][i]; the workgroup then writes its
// VM_PTS * T contiguous doubles of `out` lane by lane -- without the LDS pass a lane would store T doubles of its own, T * 8
// bytes apart from its neighbour's.  Row stride VM_PTS + 1 doubles: the transposed read walks a * (VM_PTS + 1) + i with a
// fastest, two banks apart per lane.
// ------------------------------------------------------------------------------------------
#define VM_PTS 256
__global__ __launch_bounds__(256) void vgp_sample_mix_kernel(int T, int S, int64_t M, const VgpDev* __restrict__ st,
                                                             const double* __restrict__ H, double* __restrict__ out) {
    __shared__ double tile[VGP_MAXT][VM_PTS + 1];
    __shared__ double qs[VGP_MAXT][VGP_MAXT], mus[VGP_MAXT], sq[VGP_MAXT];
    const int tid = threadIdx.x, s = blockIdx.y;
    const int64_t i0 = (int64_t)blockIdx.x * VM_PTS, i = i0 + tid;
    if (tid < T * T) qs[tid / T][tid % T] = st->Q[(tid / T) * VGP_MAXT + tid % T];
    if (tid < T) {
        mus[tid] = st->mu[tid];
        sq[tid] = st->sqs[tid];
    }
    double hv[VGP_MAXT];
#pragma unroll
    for (int t = 0; t < VGP_MAXT; ++t) hv[t] = (t < T && i < M) ? H[((int64_t)t * S + s) * M + i] : 0.0;
    __syncthreads();
    for (int a = 0; a < T; ++a) {
        double acc = 0.0;
#pragma unroll
        for (int t = 0; t < VGP_MAXT; ++t)
            if (t < T) acc = fma(qs[a][t], hv[t], acc);
        tile[a][tid] = mus[a] + sq[a] * acc;
    }
    __syncthreads();
    const int64_t left = M - i0;
    const int cnt = (int)(left < VM_PTS ? left : VM_PTS) * T;
    double* dst = out + ((int64_t)s * M + i0) * T;
    for (int e = tid; e < cnt; e += 256) dst[e] = tile[e % T][e / T];
}

// reflection mode, one chunk of test points: the blocks' posterior summed per task (mean_t = sum_b k*_{t,b}^T beta_{t,b},
// var_t = lambda_t + 1 - sum_b |L_{t,b}^-1 k*_{t,b}|^2 over the nrep consecutive problems of task t; mean_tmp: ldp per
// problem, colpart: nb x ldp per problem), then the mix of vgp_combine_kernel into rows m0 .. m0 + mcount of the M x T outputs
// radd (T x ldr, or null): with a border, |sum_b Y_{t,b}^T k*_{t,b}|^2, which the missing points give back to var_t
__global__ __launch_bounds__(256) void vgp_group_combine_kernel(int T, int nrep, int nb, int64_t ldp, int64_t m0, int64_t mcount,
                                                                const double* __restrict__ colpart,
                                                                const double* __restrict__ mean_tmp,
                                                                const double* __restrict__ radd, int64_t ldr,
                                                                const ThetaDev* __restrict__ th, const VgpDev* __restrict__ st,
                                                                double* __restrict__ mean_out, double* __restrict__ var_out) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= mcount) return;
    double mb[VGP_MAXT], vb[VGP_MAXT];
#pragma unroll
    for (int t = 0; t < VGP_MAXT; ++t) {
        mb[t] = vb[t] = 0.0;
        if (t < T) {
            double mu = 0.0, q = 0.0;
            for (int b = 0; b < nrep; ++b) {
                const int64_t p = (int64_t)t * nrep + b;
                for (int ci = 0; ci < nb; ++ci) q += colpart[(p * nb + ci) * ldp + j];
                mu += mean_tmp[p * ldp + j];
            }
            const ThetaDev& tt = th[t * nrep];
            mb[t] = mu;
            if (radd) q -= radd[(int64_t)t * ldr + j];
            vb[t] = clamp0_nan(tt.var - q) + tt.noise;
        }
    }
    for (int a = 0; a < T; ++a) {
        double mu = 0.0, v = 0.0;
#pragma unroll
        for (int t = 0; t < VGP_MAXT; ++t)
            if (t < T) {
                const double q = st->Q[a * VGP_MAXT + t];
                mu = fma(q, mb[t], mu);
                v = fma(q * q, vb[t], v);
            }
        mean_out[(m0 + j) * T + a] = st->mu[a] + st->sqs[a] * mu;
        var_out[(m0 + j) * T + a] = st->s[a] * v;
    }
}

// ------------------------------------------------------------------------------------------
// launchers
// ------------------------------------------------------------------------------------------
int launch_vgp_setup(gpimhip_ctx* h, const gpimhip_model_t* m, const gpimhip_vgp_t* vg, const double* u, VgpDev* st, int nrep) {
    hipLaunchKernelGGL(vgp_setup_kernel, dim3(1), dim3(64), 0, h->stream, *m, *vg, u, st, h->theta, nrep);
    HIP_TRY(hipGetLastError());
    return GPIMHIP_OK;
}
int launch_vgp_setup_to(gpimhip_ctx* h, const gpimhip_model_t* m, const gpimhip_vgp_t* vg, const double* u, VgpDev* st,
                        ThetaDev* theta) {
    hipLaunchKernelGGL(vgp_setup_kernel, dim3(1), dim3(64), 0, h->stream, *m, *vg, u, st, theta, 1);
    HIP_TRY(hipGetLastError());
    return GPIMHIP_OK;
}
int launch_vgp_project_to(gpimhip_ctx* h, const double* Y, int64_t N, int T, const VgpDev* st, double* z) {
    hipLaunchKernelGGL(vgp_project_kernel, dim3((unsigned)((N + 255) / 256), T), dim3(256), 0, h->stream, Y, N, N, T, st, z);
    HIP_TRY(hipGetLastError());
    return GPIMHIP_OK;
}
int launch_vgp_sample_mix(gpimhip_ctx* h, int T, int S, int64_t M, const VgpDev* st, const double* H, double* out) {
    hipLaunchKernelGGL(vgp_sample_mix_kernel, dim3((unsigned)((M + VM_PTS - 1) / VM_PTS), S), dim3(256), 0, h->stream, T, S, M, st,
                       H, out);
    HIP_TRY(hipGetLastError());
    return GPIMHIP_OK;
}
int launch_vgp_project(gpimhip_ctx* h, const double* Y, int64_t N, int T, const VgpDev* st) {
    hipLaunchKernelGGL(vgp_project_kernel, dim3((unsigned)((h->np + 255) / 256), T), dim3(256), 0, h->stream, Y, N, h->np, T, st,
                       h->ypad);
    HIP_TRY(hipGetLastError());
    return GPIMHIP_OK;
}
int launch_vgp_project_refl(gpimhip_ctx* h, const double* Y, int64_t N, int T, int nrep, const double* uo, const VgpDev* st) {
    hipLaunchKernelGGL(vgp_project_refl_kernel, dim3((unsigned)((h->np + 255) / 256), T * nrep), dim3(256), 0, h->stream, Y, N,
                       h->np, T, nrep, h->refl.wts, uo, st, h->ypad);
    HIP_TRY(hipGetLastError());
    return GPIMHIP_OK;
}
int launch_vgp_kbeta_refl(gpimhip_ctx* h, const gpimhip_model_t* m, const double* X, int64_t N, int T, int nrep, double* kb) {
    const dim3 grid((unsigned)((N + 63) / 64), nrep);
    if (m->kernel == GPIMHIP_KERNEL_RBF)
        hipLaunchKernelGGL(vgp_kbeta_refl_kernel<GPIMHIP_KERNEL_RBF>, grid, dim3(256), 0, h->stream, X, N, m->dim, h->np, T, nrep,
                           h->refl, h->theta, h->alpha, kb);
    else
        hipLaunchKernelGGL(vgp_kbeta_refl_kernel<GPIMHIP_KERNEL_MATERN52>, grid, dim3(256), 0, h->stream, X, N, m->dim, h->np, T,
                           nrep, h->refl, h->theta, h->alpha, kb);
    HIP_TRY(hipGetLastError());
    return GPIMHIP_OK;
}
int launch_vgp_kbeta(gpimhip_ctx* h, const gpimhip_model_t* m, const double* X, int64_t N, int T, double* kb) {
    const dim3 grid((unsigned)((N + 63) / 64));
    if (m->kernel == GPIMHIP_KERNEL_RBF)
        hipLaunchKernelGGL(vgp_kbeta_kernel<GPIMHIP_KERNEL_RBF>, grid, dim3(256), 0, h->stream, X, N, m->dim, h->np, T, h->theta,
                           h->alpha, kb);
    else
        hipLaunchKernelGGL(vgp_kbeta_kernel<GPIMHIP_KERNEL_MATERN52>, grid, dim3(256), 0, h->stream, X, N, m->dim, h->np, T,
                           h->theta, h->alpha, kb);
    HIP_TRY(hipGetLastError());
    return GPIMHIP_OK;
}
int launch_vgp_finalize(gpimhip_ctx* h, const gpimhip_model_t* m, const gpimhip_vgp_t* vg, int64_t N, const double* kb,
                        const VgpDev* st, double* u, double* adam_m, double* adam_v, int do_adam, AdamStep ast,
                        double* loss_out, double* grad_out, FinalizeIter fi, int nrep, const double* border_scal) {
    const int nb = (int)(h->np / NB);
    if (nrep > 0)
        hipLaunchKernelGGL(vgp_finalize_kernel<true>, dim3(1), dim3(256), 0, h->stream, *m, *vg, N, h->refl.n_total, h->np, nb,
                           nb * (nb + 1) / 2, nrep, h->refl.wts, border_scal, h->grad_part, h->z, h->logdet_part, h->alpha, kb, st, u, adam_m,
                           adam_v, do_adam, ast, loss_out, grad_out, (double*)nullptr, fi, h->info);
    else
        hipLaunchKernelGGL(vgp_finalize_kernel<false>, dim3(1), dim3(256), 0, h->stream, *m, *vg, N, N, h->np, nb,
                           nb * (nb + 1) / 2, 1, (const double*)nullptr, (const double*)nullptr, h->grad_part, h->z, h->logdet_part, h->alpha, kb, st, u,
                           adam_m, adam_v, do_adam, ast, loss_out, grad_out, (double*)nullptr, fi, h->info);
    HIP_TRY(hipGetLastError());
    return GPIMHIP_OK;
}
int launch_vgp_combine(gpimhip_ctx* h, int T, int64_t M, const VgpDev* st, const double* mblk, const double* vblk,
                       double* mean_out, double* var_out) {
    hipLaunchKernelGGL(vgp_combine_kernel, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, h->stream, T, M, st, mblk, vblk,
                       mean_out, var_out);
    HIP_TRY(hipGetLastError());
    return GPIMHIP_OK;
}
int launch_vgp_group_combine(gpimhip_ctx* h, int T, int nrep, int nb, int64_t ldp, int64_t m0, int64_t mcount, const VgpDev* st,
                             double* mean_out, double* var_out, const double* radd, int64_t ldr) {
    hipLaunchKernelGGL(vgp_group_combine_kernel, dim3((unsigned)((mcount + 255) / 256)), dim3(256), 0, h->stream, T, nrep, nb, ldp,
                       m0, mcount, h->colpart, h->mean_tmp, radd, ldr, h->theta, st, mean_out, var_out);
    HIP_TRY(hipGetLastError());
    return GPIMHIP_OK;
}
