// sm.hip -- the spectral-mixture (SM) kernel of the reference's skreconstructor(kernel='Spectral') (gpim/gpreg/skgpr.py,
// GPyTorch SpectralMixtureKernel) on the exact-GP engine: the factorisation, K^-1, the solves and the variance product are
// the engine's own (smgp.hip: sm_iter); this file has the covariance-specific pieces.
//
//   k_q(tau) = E_q C_q,  E_q = exp(-2 pi^2 sum_d tau_d^2 s_qd^2),  C_q = prod_d cos(2 pi tau_d m_qd),  K = sum_q w_q k_q + noise I
//
//   sm_setup_kernel     raw u -> w, m, s, noise (softplus) and their derivatives; r = y - c into the padded right-hand side;
//                       the per-point phases cos / sin(2 pi m_qd x_d), O(N Q d) -- the entries then need no cos / sin of
//                       their own: cos(2 pi tau m) = cos a cos b + sin a sin b (angle addition, 2 FMAs)
//   sm_kmat_kernel      K(X, X) lower tiles (noise on the diagonal, identity padding) or K(X, Z); one 128 x 128 tile per
//                       workgroup, 16 entries per thread, mixtures one after another through LDS
//   sm_grad_kernel      the contraction of G = K^-1 - alpha alpha^T against dK/dw_q, dK/dm_qd, dK/ds_qd (and tr G for the
//                       noise): per lower tile one fixed-shape record of Q (2 D + 1) + 1 partial sums
//   sm_sum_kernel       the records added up per component (one workgroup per component, fixed tree)
//   sm_finalize_kernel  loss, gradient (c through sum alpha), chain rule, Adam step, history row
//   sm_*_refl_kernel    the same pieces for the 2^r reflection blocks of a grid (one lock-step batch, one parameter vector)
// Every reduction has a fixed shape: results are bit-reproducible run to run.  Nothing is combined across workgroups inside
// a launch.
#include "kfun.hpp"
#include "refl.hpp"
#include "sm.hpp"

#define SM_TWO_PI 6.283185307179586
#define SM_PI2 9.869604401089358          // pi^2
#define SM_NREC (SM_MAXQ * (2 * GPIMHIP_MAX_DIM + 1) + 1)
// tile kernels: 1024 threads per 128 x 128 tile, thread (ty, tx) = (tid / 16, tid % 16) owns rows ty + 64 rr (rr < 2) and
// columns tx * 2 + 32 h + e (h < 4, e < 2): 16 entries, so that the per-entry registers stay well inside the budget
#define SM_RPT 2
#define SM_EPT (SM_RPT * 8)

__device__ __forceinline__ double sm_softplus(double x) { return x > 20.0 ? x : log1p(exp(x)); }
__device__ __forceinline__ double sm_dsoftplus(double x) { return x > 20.0 ? 1.0 : 1.0 / (1.0 + exp(-x)); }

__device__ __forceinline__ double sm_wave_sum(double v) {
    v += __shfl_xor(v, 32);
    v += __shfl_xor(v, 16);
    v += __shfl_xor(v, 8);
    v += __shfl_xor(v, 4);
    v += __shfl_xor(v, 2);
    v += __shfl_xor(v, 1);
    return v;
}

// sum over the 256 threads of a workgroup in a fixed tree; red: 256 doubles of LDS; the result is valid in every thread
__device__ __forceinline__ double sm_block_sum(double v, double* red) {
    const int tid = threadIdx.x;
    __syncthreads();
    red[tid] = v;
    __syncthreads();
    if (tid < 64) {
        double x = (red[tid] + red[tid + 128]) + (red[tid + 64] + red[tid + 192]);
        x = sm_wave_sum(x);
        if (tid == 0) red[0] = x;
    }
    __syncthreads();
    return red[0];
}

__device__ __forceinline__ void sm_lower_tile(int q, int& i, int& j) {
    i = (int)((sqrt(8.0 * (double)q + 1.0) - 1.0) * 0.5);
    while ((int64_t)i * (i + 1) / 2 > q) --i;
    while ((int64_t)(i + 1) * (i + 2) / 2 <= q) ++i;
    j = q - (int)((int64_t)i * (i + 1) / 2);
}

// the constrained parameters at u and what the engine's variance epilogue reads (one thread)
__device__ void sm_setup_params(const gpimhip_sm_t& sm, const SmLayout& L, const double* __restrict__ u, SmDev* __restrict__ st,
                                ThetaDev* __restrict__ theta) {
    const int dim = sm.dim;
    double sw = 0.0;
    st->c = u[0];
    for (int q = 0; q < L.Q; ++q) {
        st->w[q] = sm_softplus(u[L.w + q]);
        st->dw[q] = sm_dsoftplus(u[L.w + q]);
        sw += st->w[q];
        for (int k = 0; k < L.D; ++k) {
            const int j = q * L.D + k;
            st->m[j] = sm_softplus(u[L.m + j]);
            st->dm[j] = sm_dsoftplus(u[L.m + j]);
            st->s[j] = sm_softplus(u[L.s + j]);
            st->ds[j] = sm_dsoftplus(u[L.s + j]);
        }
        for (int d = 0; d < GPIMHIP_MAX_DIM; ++d) {
            const double sv = (d < dim) ? st->s[q * L.D + (sm.ard ? d : 0)] : 0.0;
            st->kap[q * GPIMHIP_MAX_DIM + d] = 2.0 * SM_PI2 * sv * sv;
        }
    }
    st->noise = 1e-4 + sm_softplus(u[L.noise]);
    st->dnoise = sm_dsoftplus(u[L.noise]);
    if (theta) {       // what the engine's variance epilogue reads (predict_var_kernel): prior variance and noise
        ThetaDev th;
        th.var = sw;
        for (int k = 0; k < GPIMHIP_MAX_DIM; ++k) {
            th.ls[k] = 1.0;
            th.inv_ls[k] = 1.0;
            th.dls_du[k] = 0.0;
        }
        th.noise = st->noise;
        th.alpha = 1.0;
        th.diag_add = st->noise;
        th.dvar_du = th.dnoise_du = th.dalpha_du = 0.0;
        *theta = th;
    }
}

// ------------------------------------------------------------------------------------------
// setup: grid over the ldc phase slots; block 0 also writes the constrained parameters
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void sm_setup_kernel(gpimhip_sm_t sm, const double* __restrict__ u, const double* __restrict__ P,
                                                       int64_t n, int64_t ldc, double* __restrict__ cs,
                                                       const double* __restrict__ y, double* __restrict__ ypad,
                                                       SmDev* __restrict__ st, ThetaDev* __restrict__ theta) {
    const SmLayout L = sm_layout(sm);
    const int dim = sm.dim;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < ldc) {
        if (y) ypad[i] = (i < n) ? y[i] - u[0] : 0.0;
        for (int q = 0; q < L.Q; ++q)
            for (int d = 0; d < dim; ++d) {
                const double tpm = SM_TWO_PI * sm_softplus(u[L.m + q * L.D + (sm.ard ? d : 0)]);
                double sv = 0.0, cv = 0.0;
                if (i < n) sincos(tpm * P[i * dim + d], &sv, &cv);
                cs[((int64_t)(q * dim + d) * 2 + 0) * ldc + i] = cv;
                cs[((int64_t)(q * dim + d) * 2 + 1) * ldc + i] = sv;
            }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0 && st) sm_setup_params(sm, L, u, st, theta);
}

// ------------------------------------------------------------------------------------------
// covariance build.  Tile (ci, cj): rows from X (ci), columns from Z (cj); threads 0 .. 255 stage the tile's 128 + 128
// points, every thread's 16 entries are stored as 16-byte pairs like the engine's kmat_kernel.
// ------------------------------------------------------------------------------------------
template <int DIM>
__global__ __launch_bounds__(1024) void sm_kmat_kernel(const double* __restrict__ X, int64_t N, const double* __restrict__ csx,
                                                      int64_t ldx, const double* __restrict__ Z, int64_t M,
                                                      const double* __restrict__ csz, int64_t ldz, int Q,
                                                      const SmDev* __restrict__ st, double* __restrict__ out, int64_t ld, int ntc,
                                                      int sym, int lower_only) {
    __shared__ double xr[128][DIM], xc[128][DIM];
    __shared__ double pr[128][2 * DIM], pc[128][2 * DIM];       // cos, sin per dimension of the current mixture
    const int tid = threadIdx.x, ty = tid >> 4, tx = tid & 15;
    int ci, cj;
    if (lower_only) sm_lower_tile(blockIdx.x, ci, cj);
    else { ci = blockIdx.x / ntc; cj = blockIdx.x % ntc; }
    const bool isrow = tid < 128;
    const int loc = tid & 127;
    const int64_t g = (int64_t)(isrow ? ci : cj) * 128 + loc;
    const int64_t lim = isrow ? N : M;
    const double* src = isrow ? X : Z;
    const double* csrc = isrow ? csx : csz;
    const int64_t lds_ = isrow ? ldx : ldz;
    const bool stager = tid < 256;
    if (stager)
#pragma unroll
        for (int d = 0; d < DIM; ++d) (isrow ? xr : xc)[loc][d] = (g < lim) ? src[g * DIM + d] : 0.0;
    double acc[SM_EPT];
#pragma unroll
    for (int e = 0; e < SM_EPT; ++e) acc[e] = 0.0;
    for (int q = 0; q < Q; ++q) {
        __syncthreads();
        if (stager)
#pragma unroll
            for (int k = 0; k < 2 * DIM; ++k) (isrow ? pr : pc)[loc][k] = (g < lim) ? csrc[((int64_t)q * 2 * DIM + k) * lds_ + g] : 0.0;
        __syncthreads();
        const double wq = st->w[q];
        double kap[DIM];
#pragma unroll
        for (int d = 0; d < DIM; ++d) kap[d] = st->kap[q * GPIMHIP_MAX_DIM + d];
#pragma unroll
        for (int rr = 0; rr < SM_RPT; ++rr) {
            const int r = ty + 64 * rr;
            double a[DIM], ac[DIM], as[DIM];
#pragma unroll
            for (int d = 0; d < DIM; ++d) {
                a[d] = xr[r][d];
                ac[d] = pr[r][2 * d];
                as[d] = pr[r][2 * d + 1];
            }
#pragma unroll
            for (int cc = 0; cc < 8; ++cc) {
                const int c = tx * 2 + 32 * (cc >> 1) + (cc & 1);
                double arg = 0.0, cp = 1.0;
#pragma unroll
                for (int d = 0; d < DIM; ++d) {
                    const double t = a[d] - xc[c][d];
                    arg = fma(t * t, kap[d], arg);
                    cp *= fma(ac[d], pc[c][2 * d], as[d] * pc[c][2 * d + 1]);
                }
                acc[rr * 8 + cc] = fma(wq, cp * kf_exp_neg(-arg), acc[rr * 8 + cc]);
                __builtin_amdgcn_sched_barrier(0);      // one entry at a time: bounded registers (no spills at DIM 4)
            }
        }
    }
    const double noise = st->noise;
    const bool interior = (int64_t)ci * 128 + 128 <= N && (int64_t)cj * 128 + 128 <= M && !(sym && ci == cj);
#pragma unroll
    for (int rr = 0; rr < SM_RPT; ++rr) {
        const int64_t gi = (int64_t)ci * 128 + ty + 64 * rr;
#pragma unroll
        for (int h = 0; h < 4; ++h) {
            double2 v;
            v.x = acc[rr * 8 + 2 * h];
            v.y = acc[rr * 8 + 2 * h + 1];
            if (!interior) {
#pragma unroll
                for (int e = 0; e < 2; ++e) {
                    const int64_t gj = (int64_t)cj * 128 + tx * 2 + 32 * h + e;
                    double& k = e ? v.y : v.x;
                    if (gi >= N || gj >= M) k = (sym && gi == gj) ? 1.0 : 0.0;
                    else if (sym && gi == gj) k += noise;
                }
            }
            *reinterpret_cast<double2*>(out + gi * ld + (int64_t)cj * 128 + tx * 2 + 32 * h) = v;
        }
    }
}

// ------------------------------------------------------------------------------------------
// gradient contraction over the lower tiles of K^-1 (G = K^-1 - alpha alpha^T, off-diagonal entries counted twice):
//   rec[q]                  += sum G E_q C_q                                   (d/dw_q = this)
//   rec[Q + q D + k]        += sum G tau_d sin_qd E_q prod_{e != d} cos_qe     (d/dm_qk: times -2 pi w_q)
//   rec[Q + Q D + q D + k]  += sum G tau_d^2 E_q C_q                           (d/ds_qk: times -4 pi^2 s_qk w_q)
//   rec[Q (2 D + 1)]        += sum_i G_ii                                      (d/dnoise)
// (isotropic, D = 1: the per-dimension terms are added into k = 0).  part: component-major, part[k * ntile + tile].
// ------------------------------------------------------------------------------------------
template <int DIM>
__global__ __launch_bounds__(1024) void sm_grad_kernel(const double* __restrict__ Kinv, int64_t ld, const double* __restrict__ X,
                                                      int64_t N, const double* __restrict__ csx, int64_t ldx,
                                                      const double* __restrict__ alpha, int Q, int ard,
                                                      const SmDev* __restrict__ st, double* __restrict__ part) {
    __shared__ double xr[128][DIM], xc[128][DIM];
    __shared__ double pr[128][2 * DIM], pc[128][2 * DIM];
    __shared__ double al_r[128], al_c[128];
    __shared__ double red[16][SM_NREC];
    const int tid = threadIdx.x, ty = tid >> 4, tx = tid & 15, lane = tid & 63, wave = tid >> 6;
    const int D = ard ? DIM : 1;
    const int nrec = Q * (2 * D + 1) + 1;
    const int ntile = gridDim.x;
    int ci, cj;
    sm_lower_tile(blockIdx.x, ci, cj);
    const bool isrow = tid < 128;
    const int loc = tid & 127;
    const int64_t g = (int64_t)(isrow ? ci : cj) * 128 + loc;
    const bool stager = tid < 256;
    if (stager) {
#pragma unroll
        for (int d = 0; d < DIM; ++d) (isrow ? xr : xc)[loc][d] = (g < N) ? X[g * DIM + d] : 0.0;
        (isrow ? al_r : al_c)[loc] = (g < N) ? alpha[g] : 0.0;
    }
    __syncthreads();
    // G of this thread's entries is re-read from K^-1 for every mixture (the tile stays in the caches between mixtures): no
    // per-entry value lives across the mixture loop, so the registers are bounded by one entry pair's temporaries
    const bool interior = ci > cj && (int64_t)ci * 128 + 128 <= N;
    double sdiag = 0.0;
    for (int q = 0; q < Q; ++q) {
        __syncthreads();
        if (stager)
#pragma unroll
            for (int k = 0; k < 2 * DIM; ++k) (isrow ? pr : pc)[loc][k] = (g < N) ? csx[((int64_t)q * 2 * DIM + k) * ldx + g] : 0.0;
        __syncthreads();
        double kap[DIM];
#pragma unroll
        for (int d = 0; d < DIM; ++d) kap[d] = st->kap[q * GPIMHIP_MAX_DIM + d];
        double s0 = 0.0, sm_[DIM], ss[DIM];
#pragma unroll
        for (int d = 0; d < DIM; ++d) sm_[d] = ss[d] = 0.0;
#pragma unroll 1
        for (int p = 0; p < SM_EPT / 2; ++p) {       // entry pairs: row ty + 64 (p / 4), columns tx * 2 + 32 (p % 4) + {0, 1}
            const int r = ty + 64 * (p >> 2), c0 = tx * 2 + 32 * (p & 3);
            const int64_t gi = (int64_t)ci * 128 + r;
            const double2 kv = *reinterpret_cast<const double2*>(Kinv + gi * ld + (int64_t)cj * 128 + c0);
            double a[DIM], ac[DIM], as[DIM];
#pragma unroll
            for (int d = 0; d < DIM; ++d) {
                a[d] = xr[r][d];
                ac[d] = pr[r][2 * d];
                as[d] = pr[r][2 * d + 1];
            }
            const double alr = al_r[r];
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                const int c = c0 + e;
                const int64_t gj = (int64_t)cj * 128 + c;
                const double gv = (e ? kv.y : kv.x) - alr * al_c[c];
                double wg = 2.0 * gv;
                if (!interior) {
                    if (gi >= N || gj > gi) wg = 0.0;
                    else if (gi == gj) {
                        wg = gv;
                        if (q == 0) sdiag += gv;
                    }
                }
                double t[DIM], t2[DIM], co[DIM], si[DIM];
                double arg = 0.0;
#pragma unroll
                for (int d = 0; d < DIM; ++d) {
                    t[d] = a[d] - xc[c][d];
                    t2[d] = t[d] * t[d];
                    arg = fma(t2[d], kap[d], arg);
                    const double bc = pc[c][2 * d], bs = pc[c][2 * d + 1];
                    co[d] = fma(ac[d], bc, as[d] * bs);
                    si[d] = fma(as[d], bc, -(ac[d] * bs));
                }
                const double aw = wg * kf_exp_neg(-arg);
                // products of the other dimensions' cosines (prefix x suffix)
                double oth[DIM], pre = 1.0;
#pragma unroll
                for (int d = 0; d < DIM; ++d) {
                    oth[d] = pre;
                    pre *= co[d];
                }
                double suf = 1.0;
#pragma unroll
                for (int d = DIM - 1; d >= 0; --d) {
                    oth[d] *= suf;
                    suf *= co[d];
                }
                const double kc = aw * pre;
                s0 += kc;
#pragma unroll
                for (int d = 0; d < DIM; ++d) {
                    ss[d] = fma(kc, t2[d], ss[d]);
                    sm_[d] = fma(aw * t[d], si[d] * oth[d], sm_[d]);
                }
            }
        }
        if (!ard) {
#pragma unroll
            for (int d = 1; d < DIM; ++d) {
                sm_[0] += sm_[d];
                ss[0] += ss[d];
            }
        }
        {
            const double v = sm_wave_sum(s0);
            if (lane == 0) red[wave][q] = v;
        }
        for (int k = 0; k < D; ++k) {        // (D is DIM or 1: the register index stays static after unrolling by the compiler)
            double vm = 0.0, vs = 0.0;
#pragma unroll
            for (int d = 0; d < DIM; ++d)
                if (d == k) { vm = sm_[d]; vs = ss[d]; }
            vm = sm_wave_sum(vm);
            vs = sm_wave_sum(vs);
            if (lane == 0) {
                red[wave][Q + q * D + k] = vm;
                red[wave][Q + Q * D + q * D + k] = vs;
            }
        }
    }
    {
        const double v = sm_wave_sum(sdiag);
        if (lane == 0) red[wave][nrec - 1] = v;
    }
    __syncthreads();
    for (int k = tid; k < nrec; k += 1024) {
        double v[16];
#pragma unroll
        for (int w = 0; w < 16; ++w) v[w] = red[w][k];
#pragma unroll
        for (int s = 8; s > 0; s >>= 1)
#pragma unroll
            for (int w = 0; w < s; ++w) v[w] += v[w + s];
        part[(int64_t)k * ntile + blockIdx.x] = v[0];
    }
}

// sums[k] = sum over the tiles of component k: one workgroup per component
__global__ __launch_bounds__(256) void sm_sum_kernel(const double* __restrict__ part, int ntile, double* __restrict__ sums) {
    __shared__ double red[256];
    const int k = blockIdx.x;
    double v = 0.0;
    for (int t = threadIdx.x; t < ntile; t += 256) v += part[(int64_t)k * ntile + t];
    v = sm_block_sum(v, red);
    if (threadIdx.x == 0) sums[k] = v;
}

// ------------------------------------------------------------------------------------------
// finalize: one workgroup of 256 threads.  loss = (|L^-1 r|^2 / 2 + sum log L_ii) / n + log(2 pi) / 2
// B > 1: the reflection blocks of one model (z, alpha: B x np; logdet_part: B x nb; sums: over all blocks' tiles), added in
// the fixed order of the stacked buffers; ones (B x N): U 1, through which c enters the blocks (null: 1); n = n_total;
// border_scal (border.hip): |L_S^-1 t|^2 leaves the quadratic form, sum log (L_S)_ii joins the log-determinant
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void sm_finalize_kernel(gpimhip_sm_t sm, int64_t N, int64_t np, int nb, int B,
                                                          const double* __restrict__ ones, int64_t n_total,
                                                          const double* __restrict__ border_scal,
                                                          const double* __restrict__ sums, const double* __restrict__ z,
                                                          const double* __restrict__ logdet_part,
                                                          const double* __restrict__ alpha, const SmDev* __restrict__ st,
                                                          double* __restrict__ u, double* __restrict__ adam_m,
                                                          double* __restrict__ adam_v, int do_adam, AdamStep ast,
                                                          double* __restrict__ loss_out, double* __restrict__ grad_out,
                                                          FinalizeIter fi, int32_t* __restrict__ info) {
    __shared__ double red[256];
    __shared__ int skip;
    const int tid = threadIdx.x;
    const SmLayout L = sm_layout(sm);
    double q2 = 0.0, lg = 0.0, sa = 0.0;
    for (int64_t i = tid; i < B * np; i += 256) q2 = fma(z[i], z[i], q2);
    for (int k = tid; k < B * nb; k += 256) lg += logdet_part[k];
    if (!ones) {
        for (int64_t i = tid; i < N; i += 256) sa += alpha[i];
    } else {
        for (int b = 0; b < B; ++b)
            for (int64_t i = tid; i < N; i += 256) sa = fma(ones[b * N + i], alpha[b * np + i], sa);
    }
    q2 = sm_block_sum(q2, red);
    lg = sm_block_sum(lg, red);
    sa = sm_block_sum(sa, red);
    int it = 0;
    double* hist_row = nullptr;
    if (fi.iter) {       // (every thread reads the counter here; thread 0 advances it after the last barrier below)
        it = *fi.iter;
        ast.lr_over_bc1 = fi.bc[it];
        ast.bc2_sqrt = fi.bc[fi.T + it];
        loss_out = fi.loss_base ? fi.loss_base + it : nullptr;
        hist_row = fi.hist_base ? fi.hist_base + (int64_t)it * L.P : nullptr;
        if (tid == 0) {
            // a factorisation of this training loop failed: u, the Adam state and the history stay as the previous
            // iteration left them (the reference raises inside the Cholesky there)
            skip = *info != 0;
            if (skip) atomicMin(info + 1, it);
        }
    } else if (tid == 0) {
        skip = 0;
    }
    __syncthreads();
    if (skip) return;
    const double h2n = 0.5 / (double)n_total;
    if (tid < L.P) {
        const int p = tid;
        double g;
        if (p == 0) {
            g = -sa / (double)n_total;
        } else if (p < L.m) {
            const int q = p - L.w;
            g = h2n * sums[q] * st->dw[q];
        } else if (p < L.s) {
            const int j = p - L.m, q = j / L.D;
            g = h2n * (-SM_TWO_PI * st->w[q]) * sums[L.Q + j] * st->dm[j];
        } else if (p < L.noise) {
            const int j = p - L.s, q = j / L.D;
            g = h2n * (-4.0 * SM_PI2 * st->s[j] * st->w[q]) * sums[L.Q + L.Q * L.D + j] * st->ds[j];
        } else {
            g = h2n * sums[L.Q * (2 * L.D + 1)] * st->dnoise;
        }
        if (grad_out) grad_out[p] = g;
        if (do_adam) {       // torch.optim.Adam, the expressions of theta.hpp: finalize_step_ws
            double mm = adam_m[p], vv = adam_v[p];
            mm = mm + (g - mm) * (1.0 - ast.beta1);
            vv = vv * ast.beta2 + (1.0 - ast.beta2) * g * g;
            const double denom = sqrt(vv) / ast.bc2_sqrt + ast.eps;
            const double un = u[p] + (-ast.lr_over_bc1) * (mm / denom);
            u[p] = un;
            adam_m[p] = mm;
            adam_v[p] = vv;
            if (hist_row) hist_row[p] = (p == 0) ? un : (p == L.noise ? 1e-4 + sm_softplus(un) : sm_softplus(un));
        }
    }
    __syncthreads();
    if (tid != 0) return;
    if (border_scal) {
        q2 -= border_scal[0];
        lg += border_scal[1];
    }
    const double loss = (0.5 * q2 + lg) / (double)n_total + 0.5 * 1.8378770664093453;
    if (loss_out) *loss_out = loss;
    if (fi.iter) *fi.iter = it + 1;
}

__global__ void sm_mean_kernel(const double* __restrict__ mtmp, int64_t n, const SmDev* __restrict__ st,
                               double* __restrict__ mean_out) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j < n) mean_out[j] = mtmp[j] + st->c;
}

// ------------------------------------------------------------------------------------------
// reflection blocks.  The kernel is stationary and even in every coordinate difference, so on a
// grid with reflected axes (ReflArgs::mask) the model is the B = 2^r blocks of engine.hip: kmat_refl_kernel, all on the
// points Xq of the fundamental domain, and the sum over the 2^r reflections factorises over the axes:
//   K_s[p, p'] = w_p w_p' sum_q w_q prod_d F_qd,   F_qd = f_qd(a_d - b_d) + sigma_d f_qd(a_d + b_d - 2 c_d)
//   f_qd(t) = exp(-2 pi^2 t^2 s_qd^2) cos(2 pi t m_qd),   sigma_d = the block's sign on a reflected axis (else no mirror term)
// Phases are those of the centred coordinates x_d - c_d (one set for all blocks): with cc = cos A cos B, ss = sin A sin B
// the plain term's cosine is cc + ss and the mirror term's cc - ss; the sines of the gradient are sc -+ cs likewise.
// ------------------------------------------------------------------------------------------
struct SmCentre { double c[GPIMHIP_MAX_DIM]; };

// setup in reflection mode: the phases of P - c (ldc slots); r_b = ys_b - c ones_b into the B padded right-hand sides
__global__ __launch_bounds__(256) void sm_setup_refl_kernel(gpimhip_sm_t sm, const double* __restrict__ u, const double* __restrict__ P,
                                                            int64_t n, int64_t ldc, double* __restrict__ cs,
                                                            const double* __restrict__ ys, const double* __restrict__ ones, int B,
                                                            double* __restrict__ ypad, SmCentre cen, SmDev* __restrict__ st,
                                                            ThetaDev* __restrict__ theta) {
    const SmLayout L = sm_layout(sm);
    const int dim = sm.dim;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < ldc) {
        if (ys)
            for (int b = 0; b < B; ++b) ypad[b * ldc + i] = (i < n) ? ys[b * n + i] - u[0] * ones[b * n + i] : 0.0;
        for (int q = 0; q < L.Q; ++q)
            for (int d = 0; d < dim; ++d) {
                const double tpm = SM_TWO_PI * sm_softplus(u[L.m + q * L.D + (sm.ard ? d : 0)]);
                double sv = 0.0, cv = 0.0;
                if (i < n) sincos(tpm * (P[i * dim + d] - cen.c[d]), &sv, &cv);
                cs[((int64_t)(q * dim + d) * 2 + 0) * ldc + i] = cv;
                cs[((int64_t)(q * dim + d) * 2 + 1) * ldc + i] = sv;
            }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0 && st) sm_setup_params(sm, L, u, st, theta);
}

// K_s (sym; lower_only: the lower tiles; noise on the diagonal of the present points, identity rows for absent points and padding) or
// K_s(Xq, Z) * scale; blockIdx.y: the block.  Tile layout and staging of sm_kmat_kernel; the staged coordinates are centred.
template <int DIM>
__global__ __launch_bounds__(1024) void sm_kmat_refl_kernel(const double* __restrict__ X, int64_t N, const double* __restrict__ csx,
                                                           int64_t ldx, const double* __restrict__ Z, int64_t M,
                                                           const double* __restrict__ csz, int64_t ldz, int Q,
                                                           const SmDev* __restrict__ st, double* __restrict__ out, int64_t ld,
                                                           int64_t out_bs, int ntc, int sym, int lower_only, ReflArgs refl,
                                                           SmCentre cen, double scale) {
    __shared__ double xr[128][DIM], xc[128][DIM];
    __shared__ double pr[128][2 * DIM], pc[128][2 * DIM];
    __shared__ double wr_s[128], wc_s[128];
    const int tid = threadIdx.x, ty = tid >> 4, tx = tid & 15;
    const int sg = refl_sign_dims(refl.mask, refl.pb_off + (int)blockIdx.y * refl.pb_stride);
    const double* wts = refl.wts ? refl.wts + (int64_t)blockIdx.y * N : nullptr;
    out += blockIdx.y * out_bs;
    int ci, cj;
    if (lower_only) sm_lower_tile(blockIdx.x, ci, cj);
    else { ci = blockIdx.x / ntc; cj = blockIdx.x % ntc; }
    const bool isrow = tid < 128;
    const int loc = tid & 127;
    const int64_t g = (int64_t)(isrow ? ci : cj) * 128 + loc;
    const int64_t lim = isrow ? N : M;
    const double* src = isrow ? X : Z;
    const double* csrc = isrow ? csx : csz;
    const int64_t lds_ = isrow ? ldx : ldz;
    const bool stager = tid < 256;
    if (stager) {
#pragma unroll
        for (int d = 0; d < DIM; ++d) (isrow ? xr : xc)[loc][d] = (g < lim) ? src[g * DIM + d] - cen.c[d] : 0.0;
        (isrow ? wr_s : wc_s)[loc] = (wts && (isrow || sym) && g < lim) ? wts[g] : 1.0;
    }
    double sgn[DIM];
#pragma unroll
    for (int d = 0; d < DIM; ++d) sgn[d] = ((refl.mask >> d) & 1) ? (((sg >> d) & 1) ? -1.0 : 1.0) : 0.0;
    double acc[SM_EPT];
#pragma unroll
    for (int e = 0; e < SM_EPT; ++e) acc[e] = 0.0;
    for (int q = 0; q < Q; ++q) {
        __syncthreads();
        if (stager)
#pragma unroll
            for (int k = 0; k < 2 * DIM; ++k) (isrow ? pr : pc)[loc][k] = (g < lim) ? csrc[((int64_t)q * 2 * DIM + k) * lds_ + g] : 0.0;
        __syncthreads();
        const double wq = st->w[q];
        double kap[DIM];
#pragma unroll
        for (int d = 0; d < DIM; ++d) kap[d] = st->kap[q * GPIMHIP_MAX_DIM + d];
#pragma unroll
        for (int rr = 0; rr < SM_RPT; ++rr) {
            const int r = ty + 64 * rr;
            double a[DIM], ac[DIM], as[DIM];
#pragma unroll
            for (int d = 0; d < DIM; ++d) {
                a[d] = xr[r][d];
                ac[d] = pr[r][2 * d];
                as[d] = pr[r][2 * d + 1];
            }
#pragma unroll
            for (int cc = 0; cc < 8; ++cc) {
                const int c = tx * 2 + 32 * (cc >> 1) + (cc & 1);
                double prod = 1.0;
#pragma unroll
                for (int d = 0; d < DIM; ++d) {
                    const double b = xc[c][d];
                    const double tm = a[d] - b;
                    const double cb = ac[d] * pc[c][2 * d], sb = as[d] * pc[c][2 * d + 1];
                    const double tp = a[d] + b;
                    double f = kf_exp_neg(-(tm * tm) * kap[d]) * (cb + sb);
                    f = fma(sgn[d] * kf_exp_neg(-(tp * tp) * kap[d]), cb - sb, f);      // (sgn 0: an axis without mirror)
                    prod *= f;
                    __builtin_amdgcn_sched_barrier(0);      // one axis at a time: its two exponentials do not overlap the next's
                }
                acc[rr * 8 + cc] = fma(wq, prod, acc[rr * 8 + cc]);
                __builtin_amdgcn_sched_barrier(0);      // one entry at a time: bounded registers
            }
        }
    }
    const double noise = st->noise;
#pragma unroll
    for (int rr = 0; rr < SM_RPT; ++rr) {
        const int r = ty + 64 * rr;
        const int64_t gi = (int64_t)ci * 128 + r;
#pragma unroll
        for (int h = 0; h < 4; ++h) {
            double2 v;
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                const int c = tx * 2 + 32 * h + e;
                const int64_t gj = (int64_t)cj * 128 + c;
                const double ww = wr_s[r] * wc_s[c];
                double k = scale * acc[rr * 8 + 2 * h + e] * ww;
                if (gi >= N || gj >= M || (sym && ww == 0.0)) k = (sym && gi == gj) ? 1.0 : 0.0;      // padding / absent points
                else if (sym && gi == gj) k += noise;
                (e ? v.y : v.x) = k;
            }
            *reinterpret_cast<double2*>(out + gi * ld + (int64_t)cj * 128 + tx * 2 + 32 * h) = v;
        }
    }
}

// the contraction of sm_grad_kernel for the blocks: G_s = B_s^-1 - alpha_s alpha_s^T (weights w_p w_p' included) against
//   rec[q]                  += sum G prod_d F_qd
//   rec[Q + q D + k]        += sum G (t- sin- E- + sigma t+ sin+ E+)_k prod_{e != k} F_qe          (times -2 pi w_q)
//   rec[Q + Q D + q D + k]  += sum G (t-^2 E- cos- + sigma t+^2 E+ cos+)_k prod_{e != k} F_qe      (times -4 pi^2 s_qk w_q)
//   rec[Q (2 D + 1)]        += sum_i G_ii over the present points
// with t- = a - b, t+ = a + b - 2 c.  One record per (block, lower tile): part[k * (B ntile) + block * ntile + tile].
template <int DIM>
__global__ __launch_bounds__(1024) void sm_grad_refl_kernel(const double* __restrict__ Kinv, int64_t ld, const double* __restrict__ X,
                                                           int64_t N, int64_t np, const double* __restrict__ csx, int64_t ldx,
                                                           const double* __restrict__ alpha, int Q, int ard,
                                                           const SmDev* __restrict__ st, double* __restrict__ part,
                                                           ReflArgs refl, SmCentre cen) {
    __shared__ double xr[128][DIM], xc[128][DIM];
    __shared__ double pr[128][2 * DIM], pc[128][2 * DIM];
    __shared__ double al_r[128], al_c[128];
    __shared__ double wr_s[128], wc_s[128];
    __shared__ double red[16][SM_NREC];
    const int tid = threadIdx.x, ty = tid >> 4, tx = tid & 15, lane = tid & 63, wave = tid >> 6;
    const int D = ard ? DIM : 1;
    const int nrec = Q * (2 * D + 1) + 1;
    const int ntile = gridDim.x;
    const int sg = refl_sign_dims(refl.mask, refl.pb_off + (int)blockIdx.y * refl.pb_stride);
    const double* wts = refl.wts ? refl.wts + (int64_t)blockIdx.y * N : nullptr;
    Kinv += blockIdx.y * np * ld;
    alpha += blockIdx.y * np;
    int ci, cj;
    sm_lower_tile(blockIdx.x, ci, cj);
    const bool isrow = tid < 128;
    const int loc = tid & 127;
    const int64_t g = (int64_t)(isrow ? ci : cj) * 128 + loc;
    const bool stager = tid < 256;
    if (stager) {
#pragma unroll
        for (int d = 0; d < DIM; ++d) (isrow ? xr : xc)[loc][d] = (g < N) ? X[g * DIM + d] - cen.c[d] : 0.0;
        (isrow ? al_r : al_c)[loc] = (g < N) ? alpha[g] : 0.0;
        (isrow ? wr_s : wc_s)[loc] = (wts && g < N) ? wts[g] : 1.0;
    }
    double sgn[DIM];
#pragma unroll
    for (int d = 0; d < DIM; ++d) sgn[d] = ((sg >> d) & 1) ? -1.0 : 1.0;
    __syncthreads();
    double sdiag = 0.0;
    for (int q = 0; q < Q; ++q) {
        __syncthreads();
        if (stager)
#pragma unroll
            for (int k = 0; k < 2 * DIM; ++k) (isrow ? pr : pc)[loc][k] = (g < N) ? csx[((int64_t)q * 2 * DIM + k) * ldx + g] : 0.0;
        __syncthreads();
        double kap[DIM];
#pragma unroll
        for (int d = 0; d < DIM; ++d) kap[d] = st->kap[q * GPIMHIP_MAX_DIM + d];
        double s0 = 0.0, sm_[DIM], ss[DIM];
#pragma unroll
        for (int d = 0; d < DIM; ++d) sm_[d] = ss[d] = 0.0;
#pragma unroll 1
        for (int p = 0; p < SM_EPT / 2; ++p) {       // entry pairs, as sm_grad_kernel
            const int r = ty + 64 * (p >> 2), c0 = tx * 2 + 32 * (p & 3);
            const int64_t gi = (int64_t)ci * 128 + r;
            const double2 kv = *reinterpret_cast<const double2*>(Kinv + gi * ld + (int64_t)cj * 128 + c0);
            double a[DIM], ac[DIM], as[DIM];
#pragma unroll
            for (int d = 0; d < DIM; ++d) {
                a[d] = xr[r][d];
                ac[d] = pr[r][2 * d];
                as[d] = pr[r][2 * d + 1];
            }
            const double alr = al_r[r], wrr = wr_s[r];
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                const int c = c0 + e;
                const int64_t gj = (int64_t)cj * 128 + c;
                const double gv = (e ? kv.y : kv.x) - alr * al_c[c];
                const double ww = wrr * wc_s[c];
                double wg = 2.0 * gv * ww;
                if (gi >= N || gj > gi) wg = 0.0;                  // padding, the upper triangle of a diagonal tile
                else if (gi == gj) {
                    wg = gv * ww;
                    if (q == 0 && ww != 0.0) sdiag += gv;          // (an absent point's identity row is not in the trace)
                }
                double F[DIM], Fm[DIM], Fs[DIM];
#pragma unroll
                for (int d = 0; d < DIM; ++d) {
                    const double b = xc[c][d];
                    const double bc = pc[c][2 * d], bs = pc[c][2 * d + 1];
                    const double cb = ac[d] * bc, sb = as[d] * bs, scb = as[d] * bc, csb = ac[d] * bs;
                    const double tm = a[d] - b, tm2 = tm * tm;
                    const double em = kf_exp_neg(-tm2 * kap[d]);
                    const double fm = em * (cb + sb);
                    F[d] = fm;
                    Fm[d] = tm * em * (scb - csb);
                    Fs[d] = tm2 * fm;
                    if ((refl.mask >> d) & 1) {       // (wave-uniform)
                        const double tp = a[d] + b, tp2 = tp * tp;
                        const double ep = sgn[d] * kf_exp_neg(-tp2 * kap[d]);
                        const double fp = ep * (cb - sb);
                        F[d] += fp;
                        Fm[d] = fma(tp * ep, scb + csb, Fm[d]);
                        Fs[d] = fma(tp2, fp, Fs[d]);
                    }
                }
                // products of the other dimensions' factors (prefix x suffix)
                double oth[DIM], pre = 1.0;
#pragma unroll
                for (int d = 0; d < DIM; ++d) {
                    oth[d] = pre;
                    pre *= F[d];
                }
                double suf = 1.0;
#pragma unroll
                for (int d = DIM - 1; d >= 0; --d) {
                    oth[d] *= suf;
                    suf *= F[d];
                }
                s0 = fma(wg, pre, s0);
#pragma unroll
                for (int d = 0; d < DIM; ++d) {
                    const double wo = wg * oth[d];
                    ss[d] = fma(wo, Fs[d], ss[d]);
                    sm_[d] = fma(wo, Fm[d], sm_[d]);
                }
            }
        }
        if (!ard) {
#pragma unroll
            for (int d = 1; d < DIM; ++d) {
                sm_[0] += sm_[d];
                ss[0] += ss[d];
            }
        }
        {
            const double v = sm_wave_sum(s0);
            if (lane == 0) red[wave][q] = v;
        }
        for (int k = 0; k < D; ++k) {
            double vm = 0.0, vs = 0.0;
#pragma unroll
            for (int d = 0; d < DIM; ++d)
                if (d == k) { vm = sm_[d]; vs = ss[d]; }
            vm = sm_wave_sum(vm);
            vs = sm_wave_sum(vs);
            if (lane == 0) {
                red[wave][Q + q * D + k] = vm;
                red[wave][Q + Q * D + q * D + k] = vs;
            }
        }
    }
    {
        const double v = sm_wave_sum(sdiag);
        if (lane == 0) red[wave][nrec - 1] = v;
    }
    __syncthreads();
    for (int k = tid; k < nrec; k += 1024) {
        double v[16];
#pragma unroll
        for (int w = 0; w < 16; ++w) v[w] = red[w][k];
#pragma unroll
        for (int s = 8; s > 0; s >>= 1)
#pragma unroll
            for (int w = 0; w < s; ++w) v[w] += v[w + s];
        part[((int64_t)k * gridDim.y + blockIdx.y) * ntile + blockIdx.x] = v[0];
    }
}

// mean += c in place (the blocks' summed means of predict_coupled_kernel)
__global__ void sm_addc_kernel(double* mean, int64_t n, const SmDev* __restrict__ st) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j < n) mean[j] += st->c;
}

// ------------------------------------------------------------------------------------------
// posterior draws (draws.hip: sm_family, the spectral-mixture side of the draw drivers)
// ------------------------------------------------------------------------------------------
// the constrained parameters at u into st[0] and theta (one thread), and st[1] = st[0] with `other` as its diagonal term: the
// covariance builders put st->noise on the diagonal, and a draw also builds K_b + d I (prior blocks) and the joint matrix
// with no diagonal term (launch_sample_diag adds its two)
__global__ void sm_params_kernel(gpimhip_sm_t sm, const double* __restrict__ u, SmDev* __restrict__ st,
                                 ThetaDev* __restrict__ theta, double other) {
    sm_setup_params(sm, sm_layout(sm), u, st, theta);
    st[1] = st[0];
    st[1].noise = other;
}

// out = y - c (the right-hand side of a model with a constant mean)
__global__ void sm_centre_kernel(const double* __restrict__ y, int64_t n, const SmDev* __restrict__ st, double* __restrict__ out) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j < n) out[j] = y[j] - st->c;
}

// ------------------------------------------------------------------------------------------
// sm_cross_apply_kernel: cross_apply_kernel (sample.hip) for this kernel -- K(G, X) applied to the solved right-hand sides
// without ever being written:
//   out[s][i] = c + mean_i + g[s][i] - sum_j k(G_i, X_j) Al[s][j]  (+ sqrt(noise) z_n unless noiseless),  mean_i = sum_j k Al[S][j]
// ALU-bound on the fp64 vector pipe: M N Q exponentials.  One grid point per lane.  Neither a lane's registers nor the LDS
// hold the phases of all Q <= 16 mixtures (128 doubles per point at d = 4), so the mixtures go by in chunks of SCA_QC: a lane
// keeps its own phases of the chunk (2 d SCA_QC doubles), the workgroup stages SCA_TJ training rows with their phases of the
// chunk and the SG + 1 entries of Al, and every lane reads them at the same address (a broadcast).  Per (chunk, row) the
// chunk's share of the kernel value is completed in a register -- cosine of the difference from the phases as in
// sm_kmat_kernel, no sincos here -- and then takes SG + 1 FMAs: with Q <= SCA_QC (the default Q = 4) that is the whole kernel
// value, and SG + 1 FMAs per (mixture, row) would cost a quarter of an entry's ~35 instructions at SG = 8.  Each accumulator
// runs over (chunk, j) in that order, by itself: a draw's bits do not depend on S, on s0, on the group it falls into or on
// the other draws.
// ------------------------------------------------------------------------------------------
#define SCA_TJ 128

template <int DIM, int SG>
__global__ __launch_bounds__(256) void sm_cross_apply_kernel(const double* __restrict__ G, int64_t M, const double* __restrict__ csg,
                                                             int64_t ldg, const double* __restrict__ Xt, int64_t N,
                                                             const double* __restrict__ csx, int64_t ldx, int Q,
                                                             const SmDev* __restrict__ st, const ThetaDev* __restrict__ th,
                                                             const double* __restrict__ Al, int64_t npt, int S, int s0,
                                                             const double* __restrict__ g, const double* __restrict__ Z,
                                                             int64_t zw, int64_t zn_off, int noiseless,
                                                             double* __restrict__ mean_out, double* __restrict__ out) {
    constexpr int SCA_QC = DIM <= 2 ? 4 : 2;                    // mixtures per chunk: 2 d SCA_QC <= 16 phases in a lane's registers
    __shared__ __attribute__((aligned(16))) double xs[SCA_TJ][DIM];
    __shared__ __attribute__((aligned(16))) double as[SCA_TJ][SG + 1];
    __shared__ __attribute__((aligned(16))) double ph[SCA_TJ][SCA_QC][2 * DIM];     // cos, sin per dimension
    const int tid = threadIdx.x;
    const int64_t i = (int64_t)blockIdx.x * 256 + tid;
    double a[DIM];
#pragma unroll
    for (int d = 0; d < DIM; ++d) a[d] = (i < M) ? G[i * DIM + d] : 0.0;
    double acc[SG + 1];
#pragma unroll
    for (int c = 0; c <= SG; ++c) acc[c] = 0.0;
    for (int q0 = 0; q0 < Q; q0 += SCA_QC) {
        const int qn = Q - q0 < SCA_QC ? Q - q0 : SCA_QC;
        double gp[SCA_QC][2 * DIM];
#pragma unroll
        for (int qq = 0; qq < SCA_QC; ++qq)
#pragma unroll
            for (int k = 0; k < 2 * DIM; ++k)
                gp[qq][k] = (qq < qn && i < M) ? csg[((int64_t)(q0 + qq) * 2 * DIM + k) * ldg + i] : 0.0;
        double wq[SCA_QC], kap[SCA_QC][DIM];                    // (wave-uniform: scalar registers)
#pragma unroll
        for (int qq = 0; qq < SCA_QC; ++qq) {
            const int q = qq < qn ? q0 + qq : q0;
            wq[qq] = st->w[q];
#pragma unroll
            for (int d = 0; d < DIM; ++d) kap[qq][d] = st->kap[q * GPIMHIP_MAX_DIM + d];
        }
        for (int64_t j0 = 0; j0 < N; j0 += SCA_TJ) {
            __syncthreads();                                    // the previous tile has been read
            {
                const int r = tid & (SCA_TJ - 1), hf = tid >> 7;
                const int64_t j = j0 + r;
                if (hf == 0)
#pragma unroll
                    for (int d = 0; d < DIM; ++d) xs[r][d] = (j < N) ? Xt[j * DIM + d] : 0.0;
#pragma unroll 1
                for (int c = hf; c <= SG; c += 2) {             // the two halves of the workgroup take alternate columns
                    const int64_t row = c == SG ? S : s0 + c;
                    as[r][c] = (j < N && (c == SG || s0 + c < S)) ? Al[row * npt + j] : 0.0;
                }
#pragma unroll 1
                for (int e = hf; e < SCA_QC * 2 * DIM; e += 2)  // and alternate phases of the chunk's mixtures
                    (&ph[r][0][0])[e] = (e / (2 * DIM) < qn && j < N) ? csx[((int64_t)q0 * 2 * DIM + e) * ldx + j] : 0.0;
            }
            __syncthreads();
            const int jn = (int)(N - j0 < SCA_TJ ? N - j0 : SCA_TJ);
            for (int r = 0; r < jn; ++r) {
                double t2[DIM];
#pragma unroll
                for (int d = 0; d < DIM; ++d) {
                    const double t = a[d] - xs[r][d];
                    t2[d] = t * t;
                }
                double kv = 0.0;
#pragma unroll
                for (int qq = 0; qq < SCA_QC; ++qq) {
                    if (qq >= qn) break;                        // (wave-uniform)
                    double arg = 0.0, cp = 1.0;
#pragma unroll
                    for (int d = 0; d < DIM; ++d) {
                        arg = fma(t2[d], kap[qq][d], arg);
                        cp *= fma(gp[qq][2 * d], ph[r][qq][2 * d], gp[qq][2 * d + 1] * ph[r][qq][2 * d + 1]);
                    }
                    kv = fma(wq[qq], cp * kf_exp_neg(-arg), kv);
                }
#pragma unroll
                for (int c = 0; c <= SG; ++c) acc[c] = fma(kv, as[r][c], acc[c]);
            }
        }
    }
    if (i >= M) return;
    const double mu = st->c + acc[SG];
    if (s0 == 0 && mean_out) mean_out[i] = mu;
    const double sn = noiseless ? 0.0 : sqrt(th->noise);
#pragma unroll
    for (int c = 0; c < SG; ++c) {
        if (s0 + c >= S) continue;
        const int64_t o = (int64_t)(s0 + c) * M + i;
        double v = mu + (g[o] - acc[c]);
        if (!noiseless) v = fma(sn, Z[(int64_t)(s0 + c) * zw + zn_off + i], v);
        out[o] = v;
    }
}

// ------------------------------------------------------------------------------------------
// launchers
// ------------------------------------------------------------------------------------------
int launch_sm_params(gpimhip_ctx* h, const gpimhip_sm_t* sm, const double* u, SmDev* st, ThetaDev* theta, double other) {
    hipLaunchKernelGGL(sm_params_kernel, dim3(1), dim3(1), 0, h->stream, *sm, u, st, theta, other);
    HIP_TRY(hipGetLastError());
    return GPIMHIP_OK;
}

int launch_sm_centre(gpimhip_ctx* h, const double* y, int64_t n, const SmDev* st, double* out) {
    hipLaunchKernelGGL(sm_centre_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, y, n, st, out);
    HIP_TRY(hipGetLastError());
    return GPIMHIP_OK;
}

int launch_sm_cross_apply(gpimhip_ctx* h, const gpimhip_sm_t* sm, const double* G, int64_t M, const double* csg, int64_t ldg,
                          const double* Xt, int64_t N, const double* csx, int64_t ldx, const SmDev* st, const ThetaDev* theta,
                          const double* Al, int64_t npt, int S, int s0, const double* g, const double* Z, int64_t zw,
                          int64_t zn_off, int noiseless, double* mean_out, double* out) {
    const dim3 grid((unsigned)((M + 255) / 256)), block(256);
    const int rem = S - s0;
#define SCA_LAUNCH(DIM, SG)                                                                                                 \
    hipLaunchKernelGGL((sm_cross_apply_kernel<DIM, SG>), grid, block, 0, h->stream, G, M, csg, ldg, Xt, N, csx, ldx, sm->mixtures, \
                       st, theta, Al, npt, S, s0, g, Z, zw, zn_off, noiseless, mean_out, out)
#define SCA_DIM(DIM)                            \
    do {                                        \
        if (rem >= 5) SCA_LAUNCH(DIM, 8);       \
        else if (rem >= 3) SCA_LAUNCH(DIM, 4);  \
        else if (rem == 2) SCA_LAUNCH(DIM, 2);  \
        else SCA_LAUNCH(DIM, 1);                \
    } while (0)
    switch (sm->dim) {
        case 1: SCA_DIM(1); break;
        case 2: SCA_DIM(2); break;
        case 3: SCA_DIM(3); break;
        default: SCA_DIM(4); break;
    }
#undef SCA_DIM
#undef SCA_LAUNCH
    HIP_TRY(hipGetLastError());
    return GPIMHIP_OK;
}

int launch_sm_setup(gpimhip_ctx* h, const gpimhip_sm_t* sm, const double* u, const double* P, int64_t n, int64_t ldc,
                    double* cs, const double* y, double* ypad, SmDev* st, ThetaDev* theta) {
    hipLaunchKernelGGL(sm_setup_kernel, dim3((unsigned)((ldc + 255) / 256)), dim3(256), 0, h->stream, *sm, u, P, n, ldc, cs, y,
                       ypad, st, theta);
    HIP_TRY(hipGetLastError());
    return GPIMHIP_OK;
}

int launch_sm_kmat(gpimhip_ctx* h, const gpimhip_sm_t* sm, const double* X, int64_t N, const double* csx, int64_t ldx,
                   const double* Z, int64_t M, const double* csz, int64_t ldz, const SmDev* st, double* out, int64_t ld,
                   int64_t rows_pad, int64_t cols_pad, int sym, int lower_only) {
    const int ntr = (int)(rows_pad / 128), ntc = (int)(cols_pad / 128);
    const int64_t nblk = lower_only ? (int64_t)ntr * (ntr + 1) / 2 : (int64_t)ntr * ntc;
    if (nblk <= 0) return GPIMHIP_OK;
    if (sym) { Z = X; M = N; csz = csx; ldz = ldx; }
#define SMK(DIM) hipLaunchKernelGGL(sm_kmat_kernel<DIM>, dim3((unsigned)nblk), dim3(1024), 0, h->stream, X, N, csx, ldx, Z, M, csz, \
                                    ldz, sm->mixtures, st, out, ld, ntc, sym, lower_only)
    switch (sm->dim) {
        case 1: SMK(1); break;
        case 2: SMK(2); break;
        case 3: SMK(3); break;
        default: SMK(4); break;
    }
#undef SMK
    HIP_TRY(hipGetLastError());
    return GPIMHIP_OK;
}

int launch_sm_grad(gpimhip_ctx* h, const gpimhip_sm_t* sm, const double* Kinv, int64_t ld, const double* X, int64_t N,
                   const double* csx, int64_t ldx, const double* alpha, const SmDev* st, double* part, double* sums) {
    const int nb = (int)(h->np / NB), ntile = nb * (nb + 1) / 2;
    const SmLayout L = sm_layout(*sm);
    const int nrec = L.Q * (2 * L.D + 1) + 1;
#define SMG(DIM) hipLaunchKernelGGL(sm_grad_kernel<DIM>, dim3((unsigned)ntile), dim3(1024), 0, h->stream, Kinv, ld, X, N, csx, ldx, \
                                    alpha, sm->mixtures, sm->ard, st, part)
    switch (sm->dim) {
        case 1: SMG(1); break;
        case 2: SMG(2); break;
        case 3: SMG(3); break;
        default: SMG(4); break;
    }
#undef SMG
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(sm_sum_kernel, dim3((unsigned)nrec), dim3(256), 0, h->stream, part, ntile, sums);
    HIP_TRY(hipGetLastError());
    return GPIMHIP_OK;
}

int launch_sm_finalize(gpimhip_ctx* h, const gpimhip_sm_t* sm, int64_t N, const double* sums, const SmDev* st, double* u,
                       double* adam_m, double* adam_v, int do_adam, AdamStep ast, double* loss_out, double* grad_out,
                       FinalizeIter fi, const double* ones, int64_t n_total, const double* border_scal) {
    hipLaunchKernelGGL(sm_finalize_kernel, dim3(1), dim3(256), 0, h->stream, *sm, N, h->np, (int)(h->np / NB), h->nbatch, ones,
                       n_total > 0 ? n_total : N, border_scal, sums, h->z,
                       h->logdet_part, h->alpha, st, u, adam_m, adam_v, do_adam, ast, loss_out, grad_out, fi, h->info);
    HIP_TRY(hipGetLastError());
    return GPIMHIP_OK;
}

int launch_sm_mean(gpimhip_ctx* h, const double* mtmp, int64_t n, const SmDev* st, double* mean_out) {
    hipLaunchKernelGGL(sm_mean_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, mtmp, n, st, mean_out);
    HIP_TRY(hipGetLastError());
    return GPIMHIP_OK;
}

// ---- reflection blocks: the batch is h->nbatch blocks, the centres are half of ReflArgs::twoc (0 on an axis without mirror)
static SmCentre sm_centre(const gpimhip_ctx* h) {
    SmCentre cen;
    for (int d = 0; d < GPIMHIP_MAX_DIM; ++d) cen.c[d] = ((h->refl.mask >> d) & 1) ? 0.5 * h->refl.twoc[d] : 0.0;
    return cen;
}

int launch_sm_setup_refl(gpimhip_ctx* h, const gpimhip_sm_t* sm, const double* u, const double* P, int64_t n, int64_t ldc,
                         double* cs, const double* ys, const double* ones, double* ypad, SmDev* st, ThetaDev* theta) {
    hipLaunchKernelGGL(sm_setup_refl_kernel, dim3((unsigned)((ldc + 255) / 256)), dim3(256), 0, h->stream, *sm, u, P, n, ldc, cs,
                       ys, ones, h->nbatch, ypad, sm_centre(h), st, theta);
    HIP_TRY(hipGetLastError());
    return GPIMHIP_OK;
}

int launch_sm_kmat_refl(gpimhip_ctx* h, const gpimhip_sm_t* sm, const double* X, int64_t N, const double* csx, int64_t ldx,
                        const double* Z, int64_t M, const double* csz, int64_t ldz, const SmDev* st, double* out, int64_t ld,
                        int64_t out_bs, int64_t rows_pad, int64_t cols_pad, int sym, int lower_only, double scale) {
    const int ntr = (int)(rows_pad / 128), ntc = (int)(cols_pad / 128);
    const int64_t nblk = lower_only ? (int64_t)ntr * (ntr + 1) / 2 : (int64_t)ntr * ntc;
    if (nblk <= 0) return GPIMHIP_OK;
    if (sym) { Z = X; M = N; csz = csx; ldz = ldx; }
    const dim3 grid((unsigned)nblk, (unsigned)h->nbatch);
#define SMK(DIM) hipLaunchKernelGGL(sm_kmat_refl_kernel<DIM>, grid, dim3(1024), 0, h->stream, X, N, csx, ldx, Z, M, csz, ldz, \
                                    sm->mixtures, st, out, ld, out_bs, ntc, sym, lower_only, h->refl, sm_centre(h), scale)
    switch (sm->dim) {
        case 1: SMK(1); break;
        case 2: SMK(2); break;
        case 3: SMK(3); break;
        default: SMK(4); break;
    }
#undef SMK
    HIP_TRY(hipGetLastError());
    return GPIMHIP_OK;
}

int launch_sm_grad_refl(gpimhip_ctx* h, const gpimhip_sm_t* sm, const double* Kinv, int64_t ld, const double* X, int64_t N,
                        const double* csx, int64_t ldx, const double* alpha, const SmDev* st, double* part, double* sums) {
    const int nb = (int)(h->np / NB), ntile = nb * (nb + 1) / 2;
    const SmLayout L = sm_layout(*sm);
    const int nrec = L.Q * (2 * L.D + 1) + 1;
    const dim3 grid((unsigned)ntile, (unsigned)h->nbatch);
#define SMG(DIM) hipLaunchKernelGGL(sm_grad_refl_kernel<DIM>, grid, dim3(1024), 0, h->stream, Kinv, ld, X, N, h->np, csx, ldx, alpha, \
                                    sm->mixtures, sm->ard, st, part, h->refl, sm_centre(h))
    switch (sm->dim) {
        case 1: SMG(1); break;
        case 2: SMG(2); break;
        case 3: SMG(3); break;
        default: SMG(4); break;
    }
#undef SMG
    HIP_TRY(hipGetLastError());
    // the records of all blocks' tiles per component, in the fixed order of the stacked buffer
    hipLaunchKernelGGL(sm_sum_kernel, dim3((unsigned)nrec), dim3(256), 0, h->stream, part, ntile * h->nbatch, sums);
    HIP_TRY(hipGetLastError());
    return GPIMHIP_OK;
}

int launch_sm_addc(gpimhip_ctx* h, double* mean, int64_t n, const SmDev* st) {
    hipLaunchKernelGGL(sm_addc_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, mean, n, st);
    HIP_TRY(hipGetLastError());
    return GPIMHIP_OK;
}
