// pkron.hip -- exact GP on a grid whose missing points are whole columns (a hyperspectral cube measured at a sparse set of
// pixels, an image with whole rows missing): dense-by-Kronecker blocks.
//
// The observed set is (the N_s observed points X_s of the p "ragged" axes) x (the complete product of the other axes), so
// for the RBF kernel
//     K = s2 K_s(X_s, X_s) (x) K_c,     K_c = (x) K_i = Q Lam Q^T   (Q = (x) Q_i, lambda_j = prod_i lambda_i[j_i])
//     K + sigma I = (I (x) Q) blockdiag_j( s2 lambda_j K_s + sigma I ) (I (x) Q^T),     sigma = noise + jitter
// i.e. J = prod n_i ordinary exact-GP blocks A_j of order N_s that share X_s: block j has kernel variance s2 max(lambda_j, 0)
// and targets y~_j = column j of Y Q.  The blocks run in lock-step through the batched engine (pkrongp.hip: pkron_iter) the way
// the multi-output GP's do (vgp.hip); the complete axes are a KronAxes set of kron.hip.  Here:
//   pkron_setup_kernel        u -> the model's theta, the complete axes' lengthscales, the ragged ones at variance 1
//   pkron_blocks_theta_kernel lambda_j (each factor clamped at 0) and the J blocks' theta
//   pkron_scatter_kernel      y~ (N_s x J, from the mode products) into the padded per-problem right-hand sides
//   pkron_block_sums_kernel   per block: the gradient contraction's sums, |L_j^-1 y~_j|^2, sum log diag L_j, beta_j . (K_s beta_j)
//                             and, per complete axis i, beta_j . Z_i,j with Z_i = W x_i Mm_i (W = K_s B on the tile engine)
//   pkron_finalize_kernel     the sums over the blocks in a fixed order -> the reduced sums S[] of the model on all N = N_s J
//                             observations -> the shared finalize_step (chain rule, Adam, history row)
//   pkron_qsum_kernel / pkron_post_kernel   prediction: the blocks' raw quadratic forms, the epilogue
//   posterior draws (gpimhip_sample_pkron), all draws of a group per launch: pkron_prior_theta_kernel,
//   pkron_tril_kernel (the prior factor), pkron_zeta_kernel, pkron_gather_kernel (the prior draws), pkron_resid_kernel,
//   pkron_scatter_multi_kernel, pkron_beta_stack_kernel (the update), pkron_mean_kernel, pkron_draw_kernel (the epilogue)
// With F_i = Mm_i at axis i and diag(lambda_k) on the other complete axes (Mm_i = Q_i^T E_i Q_i, E_i = l_i dK_i / dl_i):
//   d/d s2            1/2 sum_j lambda_j S_j[0]                         (S_j[]: grad_reduce_kernel's sums of block j)
//   l_k d/d l_k       1/2 s2 sum_j lambda_j S_j[1 + k]                  ragged column k
//   d/d noise         1/2 sum_j S_j[5]
//   l_i d/d l_i       1/2 s2 [ sum_j mdiag_i[j_i] prod_{k != i} lambda_k[j_k] tr(M_j K_s) - <B, W F_i^T> ]   complete axis i
// with tr(M_j K_s) = S_j[0] + beta_j^T K_s beta_j.  No eigenvector derivative appears: repeated lambda are harmless.
// Every reduction has a fixed shape: results are bit-reproducible run to run.
#include "kfun.hpp"
#include "theta.hpp"
#include "pkron.hpp"

// NQ sums over the 256 threads of a workgroup at once (fixed tree); arr: NQ x 256 doubles of LDS; results in out[0 .. NQ)
template <int NQ>
__device__ __forceinline__ void pk_sum_multi(const double* v, double* arr, double* out) {
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

__global__ __launch_bounds__(64) void pkron_setup_kernel(gpimhip_model_t m, PkronMap mp, const double* __restrict__ u,
                                                         ThetaDev* __restrict__ th3) {
    if (threadIdx.x != 0) return;
    ThetaDev t;
    theta_from_u(m, u, t);
    th3[PK_TH_MODEL] = t;
    ThetaDev a = t, r = t;
    for (int k = 0; k < GPIMHIP_MAX_DIM; ++k) {
        a.ls[k] = (k < mp.dc) ? t.ls[mp.perm[mp.p + k]] : 1.0;
        r.ls[k] = (k < mp.p) ? t.ls[mp.perm[k]] : 1.0;
        a.inv_ls[k] = 1.0 / a.ls[k];
        r.inv_ls[k] = 1.0 / r.ls[k];
        a.dls_du[k] = r.dls_du[k] = 0.0;
    }
    r.var = 1.0;
    r.diag_add = 0.0;
    r.dvar_du = r.dnoise_du = r.dalpha_du = 0.0;
    a.dvar_du = a.dnoise_du = a.dalpha_du = 0.0;
    th3[PK_TH_AXES] = a;
    th3[PK_TH_UNIT] = r;
}

// the factor of lambda_j that belongs to axis i, clamped at 0 (K_i is positive semi-definite: a negative value is rounding)
__device__ __forceinline__ double pk_lam(const KronDev& dv, int i, int ji) {
    const double l = dv.lam[dv.off[i] + ji];
    return l > 0.0 ? l : 0.0;
}

__global__ __launch_bounds__(256) void pkron_blocks_theta_kernel(PkronMap mp, KronDev dv, const ThetaDev* __restrict__ th3,
                                                                 ThetaDev* __restrict__ theta, double* __restrict__ lamj) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= mp.J) return;
    int r = j;
    int idx[GPIMHIP_MAX_DIM];
    for (int i = mp.dc - 1; i >= 0; --i) { idx[i] = r % mp.nc[i]; r /= mp.nc[i]; }
    double lam = 1.0;
    for (int i = 0; i < mp.dc; ++i) lam *= pk_lam(dv, i, idx[i]);
    lamj[j] = lam;
    ThetaDev t = th3[PK_TH_UNIT];
    const ThetaDev tm = th3[PK_TH_MODEL];
    t.var = tm.var * lam;
    t.noise = tm.noise;
    t.alpha = 1.0;
    t.diag_add = tm.diag_add;
    theta[j] = t;
}

__global__ __launch_bounds__(256) void pkron_scatter_kernel(const double* __restrict__ yt, int64_t Ns, int J, int64_t np,
                                                            double* __restrict__ ypad) {
    const int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int j = blockIdx.y;
    if (n >= np) return;
    ypad[(int64_t)j * np + n] = (n < Ns) ? yt[n * J + j] : 0.0;
}

// B[j * np + n] = beta_j[n] for n < Ns, 0 on the padding rows: the A operand of the two products with B (rows j >= J of the
// buffer stay zero from its allocation)
__global__ __launch_bounds__(256) void pkron_beta_kernel(const double* __restrict__ beta, int64_t Ns, int64_t np,
                                                         double* __restrict__ B) {
    const int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t j = blockIdx.y;
    if (n >= np) return;
    B[j * np + n] = (n < Ns) ? beta[j * np + n] : 0.0;
}

__global__ __launch_bounds__(256) void pkron_block_sums_kernel(PkronMap mp, int64_t Ns, int64_t np, int nb, int ntile,
                                                               const double* __restrict__ grad_part, const double* __restrict__ z,
                                                               const double* __restrict__ logdet_part,
                                                               const double* __restrict__ beta, const double* __restrict__ W,
                                                               const double* __restrict__ Z, double* __restrict__ bsum) {
    __shared__ double arr[13 * 256];
    __shared__ double out[13];
    const int tid = threadIdx.x;
    const int64_t j = blockIdx.x;
    double v[13] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    const double* gp = grad_part + j * ntile * 8;
    for (int q = tid; q < ntile; q += 256)
        for (int k = 0; k < 7; ++k) v[k] += gp[(int64_t)q * 8 + k];
    const double* zj = z + j * np;
    for (int64_t i = tid; i < np; i += 256) v[7] = fma(zj[i], zj[i], v[7]);
    for (int k = tid; k < nb; k += 256) v[8] += logdet_part[j * nb + k];
    const double* bj = beta + j * np;
    const double* wj = W + j * np;
    for (int64_t i = tid; i < Ns; i += 256) {
        const double b = bj[i];
        v[9] = fma(b, wj[i], v[9]);
        for (int a = 0; a < mp.dc; ++a) v[10 + a] = fma(b, Z[((int64_t)a * mp.J + j) * np + i], v[10 + a]);
    }
    pk_sum_multi<13>(v, arr, out);
    if (tid < PK_SUMS) bsum[j * PK_SUMS + tid] = tid < 13 ? out[tid] : 0.0;
}

// E[0] = sum_j lambda_j S_j[0], E[1 + k] = sum_j lambda_j S_j[1 + k] (ragged column k), E[5] = sum_j S_j[5],
// E[6] = sum |z|^2, E[7] = sum log diag L, E[8 + i] = sum_j po_i(j) [mdiag_i[j_i] (S_j[0] + beta_j . W_j) - beta_j . Z_i,j]
__global__ __launch_bounds__(256) void pkron_finalize_kernel(gpimhip_model_t m, PkronMap mp, KronDev dv, int64_t Ntot,
                                                             const double* __restrict__ bsum, const ThetaDev* __restrict__ th3,
                                                             double* __restrict__ u, double* __restrict__ adam_m,
                                                             double* __restrict__ adam_v, int do_adam, double* loss_out,
                                                             double* grad_out, FinalizeIter fi, int32_t* __restrict__ info) {
    __shared__ double arr[11 * 256];
    __shared__ double E[11];
    const int tid = threadIdx.x;
    double v[11] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int j = tid; j < mp.J; j += 256) {
        const double* b = bsum + (int64_t)j * PK_SUMS;
        int r = j;
        int idx[GPIMHIP_MAX_DIM];
        double l[GPIMHIP_MAX_DIM];
        for (int i = mp.dc - 1; i >= 0; --i) { idx[i] = r % mp.nc[i]; r /= mp.nc[i]; }
        double lam = 1.0;
        for (int i = 0; i < mp.dc; ++i) { l[i] = pk_lam(dv, i, idx[i]); lam *= l[i]; }
        v[0] = fma(lam, b[0], v[0]);
        for (int k = 0; k < mp.p; ++k) v[1 + k] = fma(lam, b[1 + k], v[1 + k]);
        v[5] += b[5];
        v[6] += b[7];
        v[7] += b[8];
        const double trmk = b[0] + b[9];
        for (int i = 0; i < mp.dc; ++i) {
            double po = 1.0;
            for (int k = 0; k < mp.dc; ++k)
                if (k != i) po *= l[k];
            v[8 + i] = fma(po, dv.mdiag[dv.off[i] + idx[i]] * trmk - b[10 + i], v[8 + i]);
        }
    }
    pk_sum_multi<11>(v, arr, E);
    if (tid != 0) return;
    const ThetaDev t = th3[PK_TH_MODEL];
    double S[7] = {0, 0, 0, 0, 0, 0, 0};
    S[0] = E[0];
    for (int k = 0; k < mp.p; ++k) S[1 + mp.perm[k]] = E[1 + k];
    for (int i = 0; i < mp.dc; ++i) S[1 + mp.perm[mp.p + i]] = E[8 + i];
    S[5] = E[5];
    // NaN sums (NaN inputs, a garbage spectrum) count as a failed factorisation
    if (!(E[7] == E[7]) && *info == 0) *info = 1;
    AdamStep st;
    st.beta1 = 0.9; st.beta2 = 0.999; st.eps = 1e-8; st.lr_over_bc1 = 0.0; st.bc2_sqrt = 1.0;
    double* hist_row = nullptr;
    if (!finalize_iter_begin(fi, info, 2 + m.n_ls, st, loss_out, hist_row)) return;
    finalize_step(m, Ntot, S, E[6], E[7], t, u, adam_m, adam_v, do_adam, st, loss_out, grad_out, hist_row, prior_constant(m));
}

__global__ __launch_bounds__(256) void pkron_qsum_kernel(int nb, int64_t ldq, int64_t cnt, const double* __restrict__ colpart,
                                                         double* __restrict__ q) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t j = blockIdx.y;
    if (t >= cnt) return;
    double s = 0.0;
    for (int ci = 0; ci < nb; ++ci) s += colpart[(j * nb + ci) * ldq + t];
    q[j * ldq + t] = s;
}

__global__ __launch_bounds__(256) void pkron_post_kernel(const ThetaDev* __restrict__ th3, int64_t Mc, int64_t ldq, int64_t m0,
                                                         int64_t cnt, const double* __restrict__ mraw,
                                                         const double* __restrict__ vraw, double* __restrict__ mean_out,
                                                         double* __restrict__ var_out) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= cnt * Mc) return;
    const int64_t t = e / Mc, c = e % Mc;
    const double s2 = th3[PK_TH_MODEL].var, noise = th3[PK_TH_MODEL].noise;
    mean_out[(m0 + t) * Mc + c] = s2 * mraw[c * ldq + t];
    var_out[(m0 + t) * Mc + c] = clamp0_nan(s2 - s2 * s2 * vraw[c * ldq + t]) + noise;
}

// ------------------------------------------------------------------------------------------
// posterior draws (gpimhip_sample_pkron); every kernel handles all draws of a group in one launch, one
// thread per output element, no reduction
// ------------------------------------------------------------------------------------------
// theta of the prior factor of the ragged part: the ragged lengthscales (PK_TH_UNIT) at the model's variance
__global__ __launch_bounds__(64) void pkron_prior_theta_kernel(const ThetaDev* __restrict__ th3, ThetaDev* __restrict__ out) {
    if (threadIdx.x != 0) return;
    ThetaDev t = th3[PK_TH_UNIT];
    t.var = th3[PK_TH_MODEL].var;
    *out = t;
}
// the strict upper triangle of the nb diagonal blocks of a factor <- 0 (the factorisation leaves what the covariance build
// wrote there, and a product on the tile engine reads diagonal tiles whole)
__global__ __launch_bounds__(256) void pkron_tril_kernel(double* __restrict__ L, int64_t ld) {
    double* D = L + (int64_t)blockIdx.x * NB * (ld + 1);
    for (int e = threadIdx.x; e < NB * NB; e += 256) {
        const int r = e / NB, c = e % NB;
        if (c > r) D[(int64_t)r * ld + c] = 0.0;
    }
}
// zeta of the draws s0 .. s0 + Sg as the right-hand operand of H = L_P zeta: out[r, s * U + c] = zeta_{s0 + s}[r, c] for
// r < Us, zero on the padding rows and columns (out: rows x cols, both multiples of 128)
__global__ __launch_bounds__(256) void pkron_zeta_kernel(const double* __restrict__ z, int64_t zw, int64_t Us, int64_t U, int s0,
                                                         int Sg, int64_t rows, int64_t cols, double* __restrict__ out) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= rows * cols) return;
    const int64_t r = e / cols, q = e % cols;
    double v = 0.0;
    if (r < Us && q < Sg * U) v = z[(s0 + q / U) * zw + r * U + q % U];
    out[e] = v;
}
// out[s, n, c] = H[idx[n], s * U + c]: the rows of the prior draw at the training (or the test) ragged rows
__global__ __launch_bounds__(256) void pkron_gather_kernel(const double* __restrict__ H, int64_t ldh, const int32_t* __restrict__ idx,
                                                           int64_t rows, int64_t U, int Sg, double* __restrict__ out) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= Sg * rows * U) return;
    const int64_t c = e % U, n = (e / U) % rows, s = e / (U * rows);
    out[e] = H[(int64_t)idx[n] * ldh + s * U + c];
}
// g[s, e] <- -g[s, e] - sqrt(sigma) z_e[s0 + s, e] over the NJ = N_s J observations: what the draw adds to the targets
// (Y's own share of the update is the mean)
__global__ __launch_bounds__(256) void pkron_resid_kernel(const double* __restrict__ ze, int64_t zw, int s0, int64_t NJ, int Sg,
                                                          const ThetaDev* __restrict__ th3, double* __restrict__ g) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= Sg * NJ) return;
    const int64_t s = e / NJ, k = e % NJ;
    g[e] = -g[e] - sqrt(th3[PK_TH_MODEL].diag_add) * ze[(s0 + s) * zw + k];
}
// the projected targets of the group (Sg, N_s, J) as the J blocks' right-hand sides: out[j, n, s] = yt[s, n, j], zero on the
// padding rows n >= Ns and columns s >= Sg (out: J x np x Sp)
__global__ __launch_bounds__(256) void pkron_scatter_multi_kernel(const double* __restrict__ yt, int64_t Ns, int64_t J, int64_t np,
                                                                  int Sg, int64_t Sp, double* __restrict__ out) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= J * np * Sp) return;
    const int64_t s = e % Sp, n = (e / Sp) % np, j = e / (Sp * np);
    out[e] = (n < Ns && s < Sg) ? yt[(s * Ns + n) * J + j] : 0.0;
}
// the blocks' solutions (J x np x Sp) as the rows of one left operand: out[s * J + j, n] = beta[j, n, s], zero on the padding
// rows of the operand (>= Sg J) and of the blocks (n >= Ns)
__global__ __launch_bounds__(256) void pkron_beta_stack_kernel(const double* __restrict__ beta, int64_t Ns, int64_t J, int64_t np,
                                                               int Sg, int64_t Sp, int64_t rows, double* __restrict__ out) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= rows * np) return;
    const int64_t n = e % np, r = e / np;
    out[e] = (r < Sg * J && n < Ns) ? beta[((r % J) * np + n) * Sp + r / J] : 0.0;
}
// mean_out[(m0 + t) Mc + c] = s2 mraw[c ldq + t]: the arithmetic of pkron_post_kernel's mean
__global__ __launch_bounds__(256) void pkron_mean_kernel(const ThetaDev* __restrict__ th3, int64_t Mc, int64_t ldq, int64_t m0,
                                                         int64_t cnt, const double* __restrict__ mraw, double* __restrict__ mean_out) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= cnt * Mc) return;
    const int64_t t = e / Mc, c = e % Mc;
    mean_out[(m0 + t) * Mc + c] = th3[PK_TH_MODEL].var * mraw[c * ldq + t];
}
// out[s0 + s, m0 + t, c] = mean[m0 + t, c] + (g*[s, m0 + t, c] + s2 upd[s, c, t]) + sqrt(c_n) z_n[s0 + s, m0 + t, c]; at
// z = 0 the bracket is 0 and the draw is the mean, bit for bit.  z_n is not read when c_n = 0.
__global__ __launch_bounds__(256) void pkron_draw_kernel(const ThetaDev* __restrict__ th3, int64_t Mc, int64_t ldq, int64_t m0,
                                                         int64_t cnt, int64_t Ms, int s0, int Sg, const double* __restrict__ gs,
                                                         const double* __restrict__ upd, const double* __restrict__ mean,
                                                         const double* __restrict__ zn, int64_t zw, int noiseless,
                                                         double* __restrict__ out) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= Sg * cnt * Mc) return;
    const int64_t c = e % Mc, t = (e / Mc) % cnt, s = e / (Mc * cnt);
    const int64_t pos = (m0 + t) * Mc + c;
    const double cn = noiseless ? 0.0 : th3[PK_TH_MODEL].noise;
    double v = fma(th3[PK_TH_MODEL].var, upd[(s * Mc + c) * ldq + t], gs[s * Ms * Mc + pos]);
    if (cn > 0.0) v = fma(sqrt(cn), zn[(s0 + s) * zw + pos], v);
    out[(s0 + s) * Ms * Mc + pos] = mean[pos] + v;
}

// ------------------------------------------------------------------------------------------
// launchers
// ------------------------------------------------------------------------------------------
#define PK_GRID(total) dim3((unsigned)(((total) + 255) / 256))
int launch_pkron_prior_theta(gpimhip_ctx* h, const ThetaDev* th3, ThetaDev* out) {
    hipLaunchKernelGGL(pkron_prior_theta_kernel, dim3(1), dim3(64), 0, h->stream, th3, out);
    HIP_TRY(hipGetLastError());
    return GPIMHIP_OK;
}
int launch_pkron_tril(gpimhip_ctx* h, double* L, int64_t ld, int nb) {
    hipLaunchKernelGGL(pkron_tril_kernel, dim3(nb), dim3(256), 0, h->stream, L, ld);
    HIP_TRY(hipGetLastError());
    return GPIMHIP_OK;
}
int launch_pkron_zeta(gpimhip_ctx* h, const double* z, int64_t zw, int64_t Us, int64_t U, int s0, int Sg, int64_t rows, int64_t cols,
                      double* out) {
    hipLaunchKernelGGL(pkron_zeta_kernel, PK_GRID(rows * cols), dim3(256), 0, h->stream, z, zw, Us, U, s0, Sg, rows, cols, out);
    HIP_TRY(hipGetLastError());
    return GPIMHIP_OK;
}
int launch_pkron_gather(gpimhip_ctx* h, const double* H, int64_t ldh, const int32_t* idx, int64_t rows, int64_t U, int Sg, double* out) {
    hipLaunchKernelGGL(pkron_gather_kernel, PK_GRID(Sg * rows * U), dim3(256), 0, h->stream, H, ldh, idx, rows, U, Sg, out);
    HIP_TRY(hipGetLastError());
    return GPIMHIP_OK;
}
int launch_pkron_resid(gpimhip_ctx* h, const double* ze, int64_t zw, int s0, int64_t NJ, int Sg, const ThetaDev* th3, double* g) {
    hipLaunchKernelGGL(pkron_resid_kernel, PK_GRID(Sg * NJ), dim3(256), 0, h->stream, ze, zw, s0, NJ, Sg, th3, g);
    HIP_TRY(hipGetLastError());
    return GPIMHIP_OK;
}
int launch_pkron_scatter_multi(gpimhip_ctx* h, const double* yt, int64_t Ns, int64_t J, int Sg, int64_t Sp, double* out) {
    hipLaunchKernelGGL(pkron_scatter_multi_kernel, PK_GRID(J * h->np * Sp), dim3(256), 0, h->stream, yt, Ns, J, h->np, Sg, Sp, out);
    HIP_TRY(hipGetLastError());
    return GPIMHIP_OK;
}
int launch_pkron_beta_stack(gpimhip_ctx* h, const double* beta, int64_t Ns, int64_t J, int Sg, int64_t Sp, int64_t rows, double* out) {
    hipLaunchKernelGGL(pkron_beta_stack_kernel, PK_GRID(rows * h->np), dim3(256), 0, h->stream, beta, Ns, J, h->np, Sg, Sp, rows, out);
    HIP_TRY(hipGetLastError());
    return GPIMHIP_OK;
}
int launch_pkron_mean(gpimhip_ctx* h, const ThetaDev* th3, int64_t Mc, int64_t ldq, int64_t m0, int64_t cnt, const double* mraw,
                      double* mean_out) {
    hipLaunchKernelGGL(pkron_mean_kernel, PK_GRID(cnt * Mc), dim3(256), 0, h->stream, th3, Mc, ldq, m0, cnt, mraw, mean_out);
    HIP_TRY(hipGetLastError());
    return GPIMHIP_OK;
}
int launch_pkron_draw(gpimhip_ctx* h, const ThetaDev* th3, int64_t Mc, int64_t ldq, int64_t m0, int64_t cnt, int64_t Ms, int s0, int Sg,
                      const double* gs, const double* upd, const double* mean, const double* zn, int64_t zw, int noiseless,
                      double* out) {
    hipLaunchKernelGGL(pkron_draw_kernel, PK_GRID(Sg * cnt * Mc), dim3(256), 0, h->stream, th3, Mc, ldq, m0, cnt, Ms, s0, Sg, gs, upd,
                       mean, zn, zw, noiseless, out);
    HIP_TRY(hipGetLastError());
    return GPIMHIP_OK;
}
int launch_pkron_setup(gpimhip_ctx* h, const gpimhip_model_t* m, const PkronMap& mp, const double* u, ThetaDev* th3) {
    hipLaunchKernelGGL(pkron_setup_kernel, dim3(1), dim3(64), 0, h->stream, *m, mp, u, th3);
    HIP_TRY(hipGetLastError());
    return GPIMHIP_OK;
}
int launch_pkron_blocks_theta(gpimhip_ctx* h, const PkronMap& mp, const KronDev& dv, const ThetaDev* th3, double* lamj) {
    hipLaunchKernelGGL(pkron_blocks_theta_kernel, dim3((unsigned)((mp.J + 255) / 256)), dim3(256), 0, h->stream, mp, dv, th3,
                       h->theta, lamj);
    HIP_TRY(hipGetLastError());
    return GPIMHIP_OK;
}
int launch_pkron_scatter(gpimhip_ctx* h, const double* yt, int64_t Ns, int J, double* ypad) {
    hipLaunchKernelGGL(pkron_scatter_kernel, dim3((unsigned)((h->np + 255) / 256), J), dim3(256), 0, h->stream, yt, Ns, J, h->np,
                       ypad);
    HIP_TRY(hipGetLastError());
    return GPIMHIP_OK;
}
int launch_pkron_beta(gpimhip_ctx* h, int64_t Ns, int J, double* B) {
    hipLaunchKernelGGL(pkron_beta_kernel, dim3((unsigned)((h->np + 255) / 256), J), dim3(256), 0, h->stream, h->alpha, Ns, h->np, B);
    HIP_TRY(hipGetLastError());
    return GPIMHIP_OK;
}
int launch_pkron_block_sums(gpimhip_ctx* h, const PkronMap& mp, int64_t Ns, const double* W, const double* Z, double* bsum) {
    const int nb = (int)(h->np / NB);
    hipLaunchKernelGGL(pkron_block_sums_kernel, dim3(mp.J), dim3(256), 0, h->stream, mp, Ns, h->np, nb, nb * (nb + 1) / 2,
                       h->grad_part, h->z, h->logdet_part, h->alpha, W, Z, bsum);
    HIP_TRY(hipGetLastError());
    return GPIMHIP_OK;
}
int launch_pkron_finalize(gpimhip_ctx* h, const gpimhip_model_t* m, const PkronMap& mp, const KronDev& dv, int64_t Ntot,
                          const double* bsum, const ThetaDev* th3, double* u, int do_adam, double* loss_out, double* grad_out,
                          FinalizeIter fi) {
    hipLaunchKernelGGL(pkron_finalize_kernel, dim3(1), dim3(256), 0, h->stream, *m, mp, dv, Ntot, bsum, th3, u, h->adam_m,
                       h->adam_v, do_adam, loss_out, grad_out, fi, h->info);
    HIP_TRY(hipGetLastError());
    return GPIMHIP_OK;
}
int launch_pkron_qsum(gpimhip_ctx* h, int J, int nb, int64_t ldq, int64_t cnt, const double* colpart, double* q) {
    hipLaunchKernelGGL(pkron_qsum_kernel, dim3((unsigned)((cnt + 255) / 256), J), dim3(256), 0, h->stream, nb, ldq, cnt, colpart, q);
    HIP_TRY(hipGetLastError());
    return GPIMHIP_OK;
}
int launch_pkron_post(gpimhip_ctx* h, const ThetaDev* th3, int64_t Mc, int64_t ldq, int64_t m0, int64_t cnt, const double* mraw,
                      const double* vraw, double* mean_out, double* var_out) {
    hipLaunchKernelGGL(pkron_post_kernel, dim3((unsigned)((cnt * Mc + 255) / 256)), dim3(256), 0, h->stream, th3, Mc, ldq, m0, cnt,
                       mraw, vraw, mean_out, var_out);
    HIP_TRY(hipGetLastError());
    return GPIMHIP_OK;
}
