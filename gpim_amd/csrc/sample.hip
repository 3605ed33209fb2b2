// sample.hip -- joint draws from the posterior of the exact GP (gpimhip_sample_exact).
//
// The joint covariance J of the stacked points [X; Xs] is factored once by the engine's Cholesky (api.hip:
// sample_impl).  In chol(J) = [[L11, 0], [L21, L22]] the right-looking factorisation has formed the Schur complement on
// its way: L21 = (L11^-1 K*)^T and L22 = chol(K** - K*^T K^-1 K* + d I), so with z = L11^-1 y and one row
// [z; z_s] per draw everything the caller wants is a product with the trapezoid L[N:, :]:
//   mean_i = L[N+i, :N] z        var_i = sum_k L22[i,k]^2 - d + noise        f_s,i = mean_i + L22[i, :i+1] z_s[:i+1]
// sample_draws_kernel reads the trapezoid once per group of up to eight draws and produces all three.
#include "sample.hpp"
#include "kfun.hpp"
#include "refl.hpp"

__global__ void sample_diag_kernel(double* __restrict__ J, int64_t ld, int64_t n_train, int64_t n_test,
                                   const ThetaDev* __restrict__ th, int noiseless, double jitter_s) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_train + n_test) return;
    const double add = i < n_train ? th->diag_add : (noiseless ? 0.0 : th->noise) + jitter_s;
    J[i * ld + i] += add;
}
int launch_sample_diag(gpimhip_ctx* h, double* J, int64_t ld, int64_t n_train, int64_t n_test, const ThetaDev* theta,
                       int noiseless, double jitter_s) {
    const int64_t n = n_train + n_test;
    hipLaunchKernelGGL(sample_diag_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, J, ld, n_train, n_test,
                       theta, noiseless, jitter_s);
    HIP_TRY(hipGetLastError());
    return GPIMHIP_OK;
}

// ------------------------------------------------------------------------------------------
// The draws kernel.  HBM-bound: every element of the trapezoid is read once per launch, 16 bytes per lane and load.
// One workgroup = SD_ROWS consecutive test points, two per wave (a wave owns its rows: the only cross-lane step is the
// xor-shuffle reduction at the end, in a fixed order).  Columns go by in chunks of SD_CW:
//   chunks left of the K / K* boundary carry the mean only (z straight from L2);
//   from the chunk that holds column N on, the workgroup stages the chunk's slice of [z; Z_s0 .. Z_s0+SG-1] in LDS once
//   and its eight rows share it (both rows of a wave from the same registers) -- without that every row would pull
//   SG x its own length through L2;
//   the strict upper triangle of L22 (what the factorisation left of K**) is never loaded.
// SG draws are accumulated in registers; the host sweeps again for the next group (launch_sample_draws).
// ------------------------------------------------------------------------------------------
#define SD_ROWS 8
#define SD_CW 256

template <int SG>
__global__ __launch_bounds__(256) void sample_draws_kernel(const double* __restrict__ L, int64_t ld, int64_t N, int64_t M,
                                                           const double* __restrict__ z, const double* __restrict__ Z, int S,
                                                           int s0, const ThetaDev* __restrict__ th, int noiseless,
                                                           double jitter_s, double* __restrict__ mean_ws,
                                                           double* __restrict__ mean_out, double* __restrict__ var_out,
                                                           double* __restrict__ out) {
    __shared__ __attribute__((aligned(16))) double zs[SD_CW];
    __shared__ __attribute__((aligned(16))) double Zs[SG][SD_CW];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t i0 = (int64_t)blockIdx.x * SD_ROWS;
    const int64_t iw = i0 + 2 * wave;                       // this wave's test points iw, iw + 1
    const bool first = s0 == 0;                             // the first group also carries mean and variance
    const double* row[2];
    int64_t lim[2];                                         // last column of the row (-1: no such test point)
    bool rv[2];
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        rv[r] = iw + r < M;
        row[r] = L + (N + (rv[r] ? iw + r : 0)) * ld;
        lim[r] = rv[r] ? N + iw + r : -1;
    }
    double mean[2] = {0.0, 0.0}, ssq[2] = {0.0, 0.0}, acc[2][SG];
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int s = 0; s < SG; ++s) acc[r][s] = 0.0;

    const int64_t cgen = (N / SD_CW) * SD_CW;               // the chunk that holds column N
    if (first) {
        for (int64_t c0 = 0; c0 < cgen; c0 += SD_CW) {
#pragma unroll
            for (int hh = 0; hh < 2; ++hh) {
                const int64_t c = c0 + hh * 128 + lane * 2;
                const double2 zz = *reinterpret_cast<const double2*>(z + c);
#pragma unroll
                for (int r = 0; r < 2; ++r) {
                    if (!rv[r]) continue;
                    const double2 l = *reinterpret_cast<const double2*>(row[r] + c);
                    mean[r] = fma(l.x, zz.x, mean[r]);
                    mean[r] = fma(l.y, zz.y, mean[r]);
                }
            }
        }
    }
    const int64_t cend = N + (i0 + SD_ROWS < M ? i0 + SD_ROWS : M);     // one past the workgroup's last column
    const bool rows_full = i0 + SD_ROWS <= M;
    for (int64_t c0 = cgen; c0 < cend; c0 += SD_CW) {
        __syncthreads();                                    // the previous chunk has been read
        {
            const int64_t c = c0 + tid, k = c - N;
            zs[tid] = (first && c < N) ? z[c] : 0.0;
#pragma unroll
            for (int s = 0; s < SG; ++s)
                Zs[s][tid] = (k >= 0 && k < M && s0 + s < S) ? Z[(int64_t)(s0 + s) * M + k] : 0.0;
        }
        __syncthreads();
        // a chunk right of the boundary and left of every row's diagonal needs no per-entry tests
        const bool interior = rows_full && c0 >= N && c0 + SD_CW - 1 <= N + i0;
        auto body = [&](auto INTERIOR) {
#pragma unroll
            for (int hh = 0; hh < 2; ++hh) {
                const int e = hh * 128 + lane * 2;
                const int64_t c = c0 + e;
                const double2 zz = *reinterpret_cast<const double2*>(&zs[e]);
                double2 zv[SG];
#pragma unroll
                for (int s = 0; s < SG; ++s) zv[s] = *reinterpret_cast<const double2*>(&Zs[s][e]);
#pragma unroll
                for (int r = 0; r < 2; ++r) {
                    double2 l, q;
                    if (decltype(INTERIOR)::value) {
                        l = *reinterpret_cast<const double2*>(row[r] + c);
                        q = l;
                    } else {
                        l.x = l.y = 0.0;
                        if (c + 1 <= lim[r]) l = *reinterpret_cast<const double2*>(row[r] + c);
                        else if (c <= lim[r]) l.x = row[r][c];
                        q.x = c >= N ? l.x : 0.0;
                        q.y = c + 1 >= N ? l.y : 0.0;
                        mean[r] = fma(l.x, zz.x, mean[r]);
                        mean[r] = fma(l.y, zz.y, mean[r]);
                    }
                    ssq[r] = fma(q.x, q.x, ssq[r]);
                    ssq[r] = fma(q.y, q.y, ssq[r]);
#pragma unroll
                    for (int s = 0; s < SG; ++s) {
                        acc[r][s] = fma(l.x, zv[s].x, acc[r][s]);
                        acc[r][s] = fma(l.y, zv[s].y, acc[r][s]);
                    }
                }
            }
        };
        if (interior) body(std::true_type{});
        else body(std::false_type{});
    }
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        for (int o = 32; o > 0; o >>= 1) {
            mean[r] += __shfl_xor(mean[r], o);
            ssq[r] += __shfl_xor(ssq[r], o);
#pragma unroll
            for (int s = 0; s < SG; ++s) acc[r][s] += __shfl_xor(acc[r][s], o);
        }
    }
    if (lane != 0) return;
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        if (!rv[r]) continue;
        const int64_t i = iw + r;
        double mu;
        if (first) {
            mu = mean[r];
            mean_ws[i] = mu;
            if (mean_out) mean_out[i] = mu;
            // the definition of gpimhip_predict_exact: noise included, jitter excluded
            if (var_out) var_out[i] = (ssq[r] - ((noiseless ? 0.0 : th->noise) + jitter_s)) + th->noise;
        } else {
            mu = mean_ws[i];
        }
#pragma unroll
        for (int s = 0; s < SG; ++s)
            if (s0 + s < S) out[(int64_t)(s0 + s) * M + i] = mu + acc[r][s];
    }
}

// draws handled by the sweep that starts at a group of `rem` remaining ones
int sample_draw_group(int rem) { return rem >= 5 ? (rem < 8 ? rem : 8) : rem; }

int launch_sample_draws(gpimhip_ctx* h, const double* L, int64_t ld, int64_t N, int64_t M, const double* z, const double* Z,
                        int S, int s0, const ThetaDev* theta, int noiseless, double jitter_s, double* mean_ws,
                        double* mean_out, double* var_out, double* out) {
    const dim3 grid((unsigned)((M + SD_ROWS - 1) / SD_ROWS)), block(256);
    const int rem = S - s0;
#define SD_LAUNCH(SG)                                                                                                   \
    hipLaunchKernelGGL(sample_draws_kernel<SG>, grid, block, 0, h->stream, L, ld, N, M, z, Z, S, s0, theta, noiseless, \
                       jitter_s, mean_ws, mean_out, var_out, out)
    if (rem >= 5) SD_LAUNCH(8);
    else if (rem >= 3) SD_LAUNCH(4);
    else if (rem == 2) SD_LAUNCH(2);
    else SD_LAUNCH(1);
#undef SD_LAUNCH
    HIP_TRY(hipGetLastError());
    return GPIMHIP_OK;
}

// ==========================================================================================
// Pathwise draws (gpimhip_sample_pathwise): a prior draw on the complete grid G through its
// reflection blocks, then one mean-type update against the training factor.  api.hip: sample_pathwise_impl.
// ==========================================================================================
// multi-index of a row-major linear index over the extents ext[0 .. d)
__device__ __forceinline__ void pw_unravel(int64_t p, const int* ext, int d, int* ix) {
#pragma unroll
    for (int k = GPIMHIP_MAX_DIM - 1; k >= 0; --k) {
        if (k < d) {
            ix[k] = (int)(p % ext[k]);
            p /= ext[k];
        } else {
            ix[k] = 0;
        }
    }
}
__device__ __forceinline__ int64_t pw_ravel(const int* ix, const int* ext, int d) {
    int64_t p = 0;
#pragma unroll
    for (int k = 0; k < GPIMHIP_MAX_DIM; ++k)
        if (k < d) p = p * ext[k] + ix[k];
    return p;
}
// the reflected axes (bit k) on whose mirror plane the point of the fundamental domain lies (axes of odd length)
__device__ __forceinline__ int pw_planes(const PwGrid& gd, const int* ix) {
    int pl = 0;
#pragma unroll
    for (int k = 0; k < GPIMHIP_MAX_DIM; ++k)
        if (k < gd.d && ((gd.mask >> k) & 1) && (gd.n[k] & 1) && ix[k] == gd.n[k] / 2) pl |= 1 << k;
    return pl;
}

__global__ __launch_bounds__(256) void pw_setup_kernel(PwGrid gd, const double* __restrict__ G, int64_t M, int64_t Nq, int B,
                                                       double* __restrict__ Xq, double* __restrict__ wts,
                                                       const int64_t* __restrict__ idx, int64_t N, double* __restrict__ Xt) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p < Nq) {
        int ix[GPIMHIP_MAX_DIM];
        pw_unravel(p, gd.f, gd.d, ix);
        const int64_t flat = pw_ravel(ix, gd.n, gd.d);
        for (int k = 0; k < gd.d; ++k) Xq[p * gd.d + k] = G[flat * gd.d + k];
        const int pl = pw_planes(gd, ix), cnt = __popc(pl);
        const double w = ldexp((cnt & 1) ? 0.70710678118654752440 : 1.0, -(cnt >> 1));
        for (int b = 0; b < B; ++b) wts[(int64_t)b * Nq + p] = (refl_sign_dims(gd.mask, b) & pl) ? 0.0 : w;
    }
    if (p < N) {
        int64_t ii = idx[p];
        ii = ii < 0 ? 0 : (ii >= M ? M - 1 : ii);
        for (int k = 0; k < gd.d; ++k) Xt[p * gd.d + k] = G[ii * gd.d + k];
    }
}
int launch_pw_setup(gpimhip_ctx* h, PwGrid gd, const double* G, int64_t M, int64_t Nq, int B, double* Xq, double* wts,
                    const int64_t* idx, int64_t N, double* Xt) {
    const int64_t n = Nq > N ? Nq : N;
    hipLaunchKernelGGL(pw_setup_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, gd, G, M, Nq, B, Xq, wts, idx,
                       N, Xt);
    HIP_TRY(hipGetLastError());
    return GPIMHIP_OK;
}

__global__ __launch_bounds__(256) void pw_gather_z_kernel(PwGrid gd, const double* __restrict__ Z, int64_t zw, int S, int64_t Nq,
                                                          double* __restrict__ Zg) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int s = blockIdx.y, b = blockIdx.z;
    if (p >= Nq) return;
    int ix[GPIMHIP_MAX_DIM];
    pw_unravel(p, gd.f, gd.d, ix);
    const int sg = refl_sign_dims(gd.mask, b);
    double v = 0.0;
    if (!(sg & pw_planes(gd, ix))) {
#pragma unroll
        for (int k = 0; k < GPIMHIP_MAX_DIM; ++k)
            if ((sg >> k) & 1) ix[k] = gd.n[k] - 1 - ix[k];
        v = Z[(int64_t)s * zw + pw_ravel(ix, gd.n, gd.d)];
    }
    Zg[((int64_t)b * S + s) * Nq + p] = v;
}
int launch_pw_gather_z(gpimhip_ctx* h, PwGrid gd, const double* Z, int64_t zw, int S, int64_t Nq, int B, double* Zg) {
    hipLaunchKernelGGL(pw_gather_z_kernel, dim3((unsigned)((Nq + 255) / 256), S, B), dim3(256), 0, h->stream, gd, Z, zw, S, Nq, Zg);
    HIP_TRY(hipGetLastError());
    return GPIMHIP_OK;
}

__global__ __launch_bounds__(256) void pw_basis_t_kernel(PwGrid gd, const double* __restrict__ C, int S, int64_t Nq, int B,
                                                         int64_t M, double rsqrt_b, double* __restrict__ g) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int s = blockIdx.y;
    if (i >= M) return;
    int ix[GPIMHIP_MAX_DIM];
    pw_unravel(i, gd.n, gd.d, ix);
    int gam = 0;                                            // the reflection that takes the representative to the point
#pragma unroll
    for (int k = 0; k < GPIMHIP_MAX_DIM; ++k)
        if (k < gd.d && ((gd.mask >> k) & 1) && ix[k] > (gd.n[k] - 1) / 2) {
            gam |= 1 << k;
            ix[k] = gd.n[k] - 1 - ix[k];
        }
    const int pl = pw_planes(gd, ix), cnt = __popc(pl);
    const int64_t p = pw_ravel(ix, gd.f, gd.d);
    double acc = 0.0;
    for (int b = 0; b < B; ++b) {
        const int sg = refl_sign_dims(gd.mask, b);
        if (sg & pl) continue;
        const double c = C[((int64_t)b * S + s) * Nq + p];
        acc += (__popc(sg & gam) & 1) ? -c : c;
    }
    g[(int64_t)s * M + i] = acc * (ldexp((cnt & 1) ? 1.41421356237309504880 : 1.0, cnt >> 1) * rsqrt_b);
}
int launch_pw_basis_t(gpimhip_ctx* h, PwGrid gd, const double* C, int S, int64_t Nq, int B, int64_t M, double* g) {
    hipLaunchKernelGGL(pw_basis_t_kernel, dim3((unsigned)((M + 255) / 256), S), dim3(256), 0, h->stream, gd, C, S, Nq, B, M,
                       1.0 / sqrt((double)B), g);
    HIP_TRY(hipGetLastError());
    return GPIMHIP_OK;
}

__global__ __launch_bounds__(256) void pw_rhs_kernel(const double* __restrict__ g, int64_t M, const int64_t* __restrict__ idx,
                                                     int64_t N, const double* __restrict__ Z, int64_t zw, int S,
                                                     const double* __restrict__ y, const ThetaDev* __restrict__ th,
                                                     double jitter_s, double* __restrict__ R, int64_t npt) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int s = blockIdx.y;
    if (j >= npt) return;
    double v = 0.0;
    if (j < N) {
        if (s < S) {
            const int64_t ii = idx[j];
            const double e = th->diag_add - jitter_s;
            v = ((ii >= 0 && ii < M) ? g[(int64_t)s * M + ii] : 0.0) + sqrt(e > 0.0 ? e : 0.0) * Z[(int64_t)s * zw + M + j];
        } else {
            v = y[j];
        }
    }
    R[(int64_t)s * npt + j] = v;
}
int launch_pw_rhs(gpimhip_ctx* h, const double* g, int64_t M, const int64_t* idx, int64_t N, const double* Z, int64_t zw, int S,
                  const double* y, const ThetaDev* theta, double jitter_s, double* R, int64_t npt) {
    hipLaunchKernelGGL(pw_rhs_kernel, dim3((unsigned)((npt + 255) / 256), S + 1), dim3(256), 0, h->stream, g, M, idx, N, Z, zw, S,
                       y, theta, jitter_s, R, npt);
    HIP_TRY(hipGetLastError());
    return GPIMHIP_OK;
}

__global__ void pw_set_diag_kernel(ThetaDev* th, double v) { th->diag_add = v; }
int launch_pw_set_diag(gpimhip_ctx* h, ThetaDev* theta, double v) {
    hipLaunchKernelGGL(pw_set_diag_kernel, dim3(1), dim3(1), 0, h->stream, theta, v);
    HIP_TRY(hipGetLastError());
    return GPIMHIP_OK;
}

// ------------------------------------------------------------------------------------------
// cross_apply_kernel: K(G, X) applied to the solved right-hand sides without ever being written.  ALU-bound on the fp64
// vector pipe (M N covariance evaluations of kfun.hpp, SG + 1 FMAs each).  One grid point per lane; the workgroup stages
// CA_TJ training rows (scaled by the lengthscales) and the matching SG + 1 entries of Al in LDS once and every lane reads
// them at the same address (a broadcast).  Each accumulator runs over j = 0 .. N-1 in order, by itself: a draw's bits do
// not depend on S, on the group it falls into or on the other draws.  The last column is alpha_y: the posterior mean.
// ------------------------------------------------------------------------------------------
#define CA_TJ 128

template <int KIND, int SG>
__global__ __launch_bounds__(256) void cross_apply_kernel(const double* __restrict__ G, int64_t M, const double* __restrict__ Xt,
                                                          int64_t N, int d, const ThetaDev* __restrict__ th,
                                                          const double* __restrict__ Al, int64_t npt, int S, int s0,
                                                          const double* __restrict__ g, const double* __restrict__ Z, int64_t zw,
                                                          int64_t zn_off, int noiseless, double* __restrict__ mean_out,
                                                          double* __restrict__ out) {
    __shared__ __attribute__((aligned(16))) double xs[CA_TJ][GPIMHIP_MAX_DIM];
    __shared__ __attribute__((aligned(16))) double as[CA_TJ][SG + 1];
    const int tid = threadIdx.x;
    // (the few fields needed, not a private copy of the struct: that would live in scratch memory)
    const double t_var = th->var, t_alpha = th->alpha, t_noise = th->noise;
    const double ls0 = th->ls[0], ls1 = th->ls[1], ls2 = th->ls[2], ls3 = th->ls[3];
    const double ls[GPIMHIP_MAX_DIM] = {ls0, ls1, ls2, ls3};
    const int64_t i = (int64_t)blockIdx.x * 256 + tid;
    double a[GPIMHIP_MAX_DIM];
#pragma unroll
    for (int k = 0; k < GPIMHIP_MAX_DIM; ++k) a[k] = (k < d && i < M) ? G[i * d + k] / ls[k] : 0.0;
    double acc[SG + 1];
#pragma unroll
    for (int c = 0; c <= SG; ++c) acc[c] = 0.0;
    for (int64_t j0 = 0; j0 < N; j0 += CA_TJ) {
        __syncthreads();                                    // the previous tile has been read
        {
            const int r = tid & (CA_TJ - 1), hf = tid >> 7;
            const int64_t j = j0 + r;
#pragma unroll
            for (int k = hf * 2; k < hf * 2 + 2; ++k) xs[r][k] = (k < d && j < N) ? Xt[j * d + k] / ls[k] : 0.0;
#pragma unroll
            for (int c = 0; c <= SG; ++c) {
                if ((c & 1) != hf) continue;                // the two halves of the workgroup take alternate columns
                const int64_t row = c == SG ? S : s0 + c;
                as[r][c] = (j < N && (c == SG || s0 + c < S)) ? Al[row * npt + j] : 0.0;
            }
        }
        __syncthreads();
        const int jn = (int)(N - j0 < CA_TJ ? N - j0 : CA_TJ);
        for (int r = 0; r < jn; ++r) {
            double r2 = 0.0;
#pragma unroll
            for (int k = 0; k < GPIMHIP_MAX_DIM; ++k) {
                const double df = a[k] - xs[r][k];
                r2 = fma(df, df, r2);
            }
            const double kv = kfun_value<KIND>(r2, t_alpha);
#pragma unroll
            for (int c = 0; c <= SG; ++c) acc[c] = fma(kv, as[r][c], acc[c]);
        }
    }
    if (i >= M) return;
    const double mu = t_var * acc[SG];
    if (s0 == 0 && mean_out) mean_out[i] = mu;
    const double sn = noiseless ? 0.0 : sqrt(t_noise);
#pragma unroll
    for (int c = 0; c < SG; ++c) {
        if (s0 + c >= S) continue;
        const int64_t o = (int64_t)(s0 + c) * M + i;
        double v = mu + (g[o] - t_var * acc[c]);
        if (!noiseless) v = fma(sn, Z[(int64_t)(s0 + c) * zw + zn_off + i], v);
        out[o] = v;
    }
}

int launch_pw_cross_apply(gpimhip_ctx* h, const gpimhip_model_t* m, const double* G, int64_t M, const double* Xt, int64_t N,
                          const ThetaDev* theta, const double* Al, int64_t npt, int S, int s0, const double* g, const double* Z,
                          int64_t zw, int64_t zn_off, int noiseless, double* mean_out, double* out) {
    const dim3 grid((unsigned)((M + 255) / 256)), block(256);
    const int rem = S - s0;
#define CA_LAUNCH(KIND, SG)                                                                                              \
    hipLaunchKernelGGL((cross_apply_kernel<KIND, SG>), grid, block, 0, h->stream, G, M, Xt, N, m->dim, theta, Al, npt, S, s0, g, \
                       Z, zw, zn_off, noiseless, mean_out, out)
#define CA_KIND(KIND)                    \
    do {                                 \
        if (rem >= 5) CA_LAUNCH(KIND, 8); \
        else if (rem >= 3) CA_LAUNCH(KIND, 4); \
        else if (rem == 2) CA_LAUNCH(KIND, 2); \
        else CA_LAUNCH(KIND, 1);         \
    } while (0)
    switch (m->kernel) {
        case GPIMHIP_KERNEL_RBF: CA_KIND(GPIMHIP_KERNEL_RBF); break;
        case GPIMHIP_KERNEL_MATERN52: CA_KIND(GPIMHIP_KERNEL_MATERN52); break;
        case GPIMHIP_KERNEL_RQ: CA_KIND(GPIMHIP_KERNEL_RQ); break;
        default: gpim_set_error("unknown kernel kind"); return GPIMHIP_E_BADARG;
    }
#undef CA_KIND
#undef CA_LAUNCH
    HIP_TRY(hipGetLastError());
    return GPIMHIP_OK;
}

__global__ __launch_bounds__(256) void pw_scatter_kernel(const int64_t* __restrict__ idx, int64_t N, int64_t M,
                                                         const double* __restrict__ Al, int64_t npt, double jitter_s,
                                                         double* __restrict__ out) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int s = blockIdx.y;
    if (j >= N) return;
    const int64_t ii = idx[j];
    if (ii < 0 || ii >= M) return;
    out[(int64_t)s * M + ii] -= jitter_s * Al[(int64_t)s * npt + j];
}
int launch_pw_scatter(gpimhip_ctx* h, const int64_t* idx, int64_t N, int64_t M, const double* Al, int64_t npt, int S,
                      double jitter_s, double* out) {
    hipLaunchKernelGGL(pw_scatter_kernel, dim3((unsigned)((N + 255) / 256), S), dim3(256), 0, h->stream, idx, N, M, Al, npt,
                       jitter_s, out);
    HIP_TRY(hipGetLastError());
    return GPIMHIP_OK;
}

// ==========================================================================================
// Draws on a fully observed grid through its reflection blocks alone (gpimhip_sample_blocks): with
// observations on every grid point the whole recipe above is block diagonal in the basis U.  api.hip: sample_blocks_impl.
// ==========================================================================================
// E[b][s][p] = (U v_s)_{b,p}: v_s = Z[s][ze_off + .] for s < S, y for s == S -- the transpose of pw_basis_t_kernel.  The
// distinct mirror images of p are added in the order of the reflections; rows of points absent from block b and the padding
// p >= Nq (rows of npq) are zero.
__global__ __launch_bounds__(256) void pw_basis_fwd_kernel(PwGrid gd, const double* __restrict__ Z, int64_t zw, int64_t ze_off,
                                                           const double* __restrict__ y, int S, int64_t Nq, int64_t npq, int B,
                                                           double rsqrt_b, double* __restrict__ E) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int s = blockIdx.y, b = blockIdx.z;
    if (p >= npq) return;
    double v = 0.0;
    if (p < Nq) {
        int ix[GPIMHIP_MAX_DIM];
        pw_unravel(p, gd.f, gd.d, ix);
        const int pl = pw_planes(gd, ix), cnt = __popc(pl), sb = refl_sign_dims(gd.mask, b);
        if (!(sb & pl)) {
            const double* src = s < S ? Z + (int64_t)s * zw + ze_off : y;
            double acc = 0.0;
            for (int g = 0; g < B; ++g) {
                const int sg = refl_sign_dims(gd.mask, g);
                if (sg & pl) continue;                      // the image of a point on the mirror plane is the point itself
                int jx[GPIMHIP_MAX_DIM];
#pragma unroll
                for (int k = 0; k < GPIMHIP_MAX_DIM; ++k) jx[k] = ((sg >> k) & 1) ? gd.n[k] - 1 - ix[k] : ix[k];
                const double c = src[pw_ravel(jx, gd.n, gd.d)];
                acc += (__popc(sb & sg) & 1) ? -c : c;
            }
            v = acc * (ldexp((cnt & 1) ? 1.41421356237309504880 : 1.0, cnt >> 1) * rsqrt_b);
        }
    }
    E[((int64_t)b * (S + 1) + s) * npq + p] = v;
}
int launch_pw_basis_fwd(gpimhip_ctx* h, PwGrid gd, const double* Z, int64_t zw, int64_t ze_off, const double* y, int S,
                        int64_t Nq, int64_t npq, int B, double* E) {
    hipLaunchKernelGGL(pw_basis_fwd_kernel, dim3((unsigned)((npq + 255) / 256), S + 1, B), dim3(256), 0, h->stream, gd, Z, zw,
                       ze_off, y, S, Nq, npq, B, 1.0 / sqrt((double)B), E);
    HIP_TRY(hipGetLastError());
    return GPIMHIP_OK;
}

// theta->diag_add = jitter_m + noise: what launch_theta left there before launch_pw_set_diag (theta.hpp: theta_from_u)
__global__ void pw_reset_diag_kernel(ThetaDev* th, double jitter_m) { th->diag_add = jitter_m + th->noise; }
int launch_pw_reset_diag(gpimhip_ctx* h, ThetaDev* theta, double jitter_m) {
    hipLaunchKernelGGL(pw_reset_diag_kernel, dim3(1), dim3(1), 0, h->stream, theta, jitter_m);
    HIP_TRY(hipGetLastError());
    return GPIMHIP_OK;
}

// one block's right-hand sides R (S + 1 rows of npq): row s = c[s] + sqrt(diag_add - jitter_s) e[s], row S = ys (Eb: the
// block's S + 1 rows of pw_basis_fwd_kernel; Cb: its S rows of Nq prior draws); theta->diag_add = s
__global__ __launch_bounds__(256) void pw_blocks_rhs_kernel(const double* __restrict__ Cb, const double* __restrict__ Eb, int S,
                                                            int64_t Nq, int64_t npq, const ThetaDev* __restrict__ th,
                                                            double jitter_s, double* __restrict__ R) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int s = blockIdx.y;
    if (p >= npq) return;
    double v = Eb[(int64_t)s * npq + p];
    if (s < S) {
        const double e = th->diag_add - jitter_s;
        v = (p < Nq ? Cb[(int64_t)s * Nq + p] : 0.0) + sqrt(e > 0.0 ? e : 0.0) * v;
    }
    R[(int64_t)s * npq + p] = v;
}
int launch_pw_blocks_rhs(gpimhip_ctx* h, const double* Cb, const double* Eb, int S, int64_t Nq, int64_t npq,
                         const ThetaDev* theta, double jitter_s, double* R) {
    hipLaunchKernelGGL(pw_blocks_rhs_kernel, dim3((unsigned)((npq + 255) / 256), S + 1), dim3(256), 0, h->stream, Cb, Eb, S, Nq,
                       npq, theta, jitter_s, R);
    HIP_TRY(hipGetLastError());
    return GPIMHIP_OK;
}

// one block's rows of the result in the basis U (S + 1 rows of Nq): with mean = ys - s alpha_y,
// row v < S = mean + ((s - d) alpha_v - sqrt(s - d) e_v), row S = mean
__global__ __launch_bounds__(256) void pw_blocks_combine_kernel(const double* __restrict__ Al, const double* __restrict__ Eb,
                                                                int S, int64_t Nq, int64_t npq,
                                                                const ThetaDev* __restrict__ th, double jitter_s,
                                                                double* __restrict__ Cc) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int v = blockIdx.y;
    if (p >= Nq) return;
    const double sd = th->diag_add;
    const double mean = Eb[(int64_t)S * npq + p] - sd * Al[(int64_t)S * npq + p];
    double o = mean;
    if (v < S) {
        double e = sd - jitter_s;
        e = e > 0.0 ? e : 0.0;
        o = mean + (e * Al[(int64_t)v * npq + p] - sqrt(e) * Eb[(int64_t)v * npq + p]);
    }
    Cc[(int64_t)v * Nq + p] = o;
}
int launch_pw_blocks_combine(gpimhip_ctx* h, const double* Al, const double* Eb, int S, int64_t Nq, int64_t npq,
                             const ThetaDev* theta, double jitter_s, double* Cc) {
    hipLaunchKernelGGL(pw_blocks_combine_kernel, dim3((unsigned)((Nq + 255) / 256), S + 1), dim3(256), 0, h->stream, Al, Eb, S,
                       Nq, npq, theta, jitter_s, Cc);
    HIP_TRY(hipGetLastError());
    return GPIMHIP_OK;
}

// out[s] = g[s] (+ sqrt(noise) Z[s][zn_off + .] unless noiseless) for s < S; mean_out = g[S]
__global__ __launch_bounds__(256) void pw_blocks_out_kernel(const double* __restrict__ g, int64_t M, int S,
                                                            const double* __restrict__ Z, int64_t zw, int64_t zn_off,
                                                            int noiseless, const ThetaDev* __restrict__ th,
                                                            double* __restrict__ mean_out, double* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int s = blockIdx.y;
    if (i >= M) return;
    double v = g[(int64_t)s * M + i];
    if (s == S) {
        if (mean_out) mean_out[i] = v;
        return;
    }
    if (!noiseless) v = fma(sqrt(th->noise), Z[(int64_t)s * zw + zn_off + i], v);
    out[(int64_t)s * M + i] = v;
}
int launch_pw_blocks_out(gpimhip_ctx* h, const double* g, int64_t M, int S, const double* Z, int64_t zw, int64_t zn_off,
                         int noiseless, const ThetaDev* theta, double* mean_out, double* out) {
    hipLaunchKernelGGL(pw_blocks_out_kernel, dim3((unsigned)((M + 255) / 256), S + 1), dim3(256), 0, h->stream, g, M, S, Z, zw,
                       zn_off, noiseless, theta, mean_out, out);
    HIP_TRY(hipGetLastError());
    return GPIMHIP_OK;
}
