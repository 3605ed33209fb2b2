// sample.hip -- joint draws from the posterior of the exact GP (gpimhip_sample_exact).
//
// The joint covariance J of the stacked points [X; Xs] is factored once by the engine's Cholesky (draws.hip:
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
// reflection blocks, then one mean-type update against the training factor.  draws.hip: sample_pathwise_impl.
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
    return with_kind(m->kernel, [&](auto K) {
        constexpr int KIND = decltype(K)::value;
        auto launch = [&](auto SG) {
            hipLaunchKernelGGL((cross_apply_kernel<KIND, decltype(SG)::value>), grid, block, 0, h->stream, G, M, Xt, N, m->dim, theta,
                               Al, npt, S, s0, g, Z, zw, zn_off, noiseless, mean_out, out);
        };
        if (rem >= 5) launch(std::integral_constant<int, 8>{});
        else if (rem >= 3) launch(std::integral_constant<int, 4>{});
        else if (rem == 2) launch(std::integral_constant<int, 2>{});
        else launch(std::integral_constant<int, 1>{});
        HIP_TRY(hipGetLastError());
        return GPIMHIP_OK;
    });
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
// observations on every grid point the whole recipe above is block diagonal in the basis U.  draws.hip: sample_blocks_impl.
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

// ==========================================================================================
// Draws on a grid with MISSING points through the bordered reflection blocks (gpimhip_sample_border).
// The model's prediction state is all there is to solve against: the explicit inverse factors L_b^-1 of the completed grid's
// blocks, and S, L_S^-1, Y_b of the border.  draws.hip: sample_border_impl.  Vectors are stored block-major, S + 1 columns of
// np per block (column S: y); every reduction below has a fixed order and every column accumulates by itself.
// ==========================================================================================
__device__ __forceinline__ double bs_wave_sum(double v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// mi[miss[j]] = j (mi preset to -1): the grid point's place among the missing ones
__global__ __launch_bounds__(256) void bs_mark_kernel(const int64_t* __restrict__ miss, int Mm, int64_t M, int32_t* __restrict__ mi) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= Mm) return;
    const int64_t ii = miss[j];
    if (ii >= 0 && ii < M) mi[ii] = j;
}
int launch_bs_mark(gpimhip_ctx* h, const int64_t* miss, int Mm, int64_t M, int32_t* mi) {
    HIP_TRY(hipMemsetAsync(mi, 0xff, (size_t)M * sizeof(int32_t), h->stream));
    hipLaunchKernelGGL(bs_mark_kernel, dim3((unsigned)((Mm + 255) / 256)), dim3(256), 0, h->stream, miss, Mm, M, mi);
    HIP_TRY(hipGetLastError());
    return GPIMHIP_OK;
}
__global__ void bs_merge_info_kernel(int32_t* __restrict__ from, int32_t* __restrict__ into) {
    const int32_t s = *from;
    if (s != 0 && *into == 0) *into = s;
    *from = 0;
}
int launch_bs_merge_info(gpimhip_ctx* h, int32_t* from, int32_t* into) {
    hipLaunchKernelGGL(bs_merge_info_kernel, dim3(1), dim3(1), 0, h->stream, from, into);
    HIP_TRY(hipGetLastError());
    return GPIMHIP_OK;
}

// R[b][s][p] = (U r~_s)_{b,p} for s < S, r~_s = g_s + sqrt(diag_add - jitter_s) Z[s][M + .] at the observed points and 0 at
// the missing ones; R[b][S] = ys[b] (y~ comes in the adapted basis).  pw_basis_fwd_kernel with the right-hand side formed on
// the way: the same order over the mirror images, zero rows for absent points and for the padding p >= Nq.
__global__ __launch_bounds__(256) void bs_rhs_fwd_kernel(PwGrid gd, const double* __restrict__ g, const double* __restrict__ Z,
                                                         int64_t zw, int64_t M, const int32_t* __restrict__ mi,
                                                         const double* __restrict__ ys, const ThetaDev* __restrict__ th,
                                                         double jitter_s, int S, int64_t Nq, int64_t np, int B, double rsqrt_b,
                                                         double* __restrict__ R) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int s = blockIdx.y, b = blockIdx.z;
    if (p >= np) return;
    double v = 0.0;
    if (p < Nq) {
        if (s == S) {
            v = ys[(int64_t)b * Nq + p];
        } else {
            int ix[GPIMHIP_MAX_DIM];
            pw_unravel(p, gd.f, gd.d, ix);
            const int pl = pw_planes(gd, ix), cnt = __popc(pl), sb = refl_sign_dims(gd.mask, b);
            if (!(sb & pl)) {
                const double e = th->diag_add - jitter_s, sq = sqrt(e > 0.0 ? e : 0.0);
                double acc = 0.0;
                for (int gm = 0; gm < B; ++gm) {
                    const int sg = refl_sign_dims(gd.mask, gm);
                    if (sg & pl) continue;
                    int jx[GPIMHIP_MAX_DIM];
#pragma unroll
                    for (int k = 0; k < GPIMHIP_MAX_DIM; ++k) jx[k] = ((sg >> k) & 1) ? gd.n[k] - 1 - ix[k] : ix[k];
                    const int64_t i = pw_ravel(jx, gd.n, gd.d);
                    const double c = mi[i] >= 0 ? 0.0 : fma(sq, Z[(int64_t)s * zw + M + i], g[(int64_t)s * M + i]);
                    acc += (__popc(sb & sg) & 1) ? -c : c;
                }
                v = acc * (ldexp((cnt & 1) ? 1.41421356237309504880 : 1.0, cnt >> 1) * rsqrt_b);
            }
        }
    }
    R[((int64_t)b * (S + 1) + s) * np + p] = v;
}
int launch_bs_rhs_fwd(gpimhip_ctx* h, PwGrid gd, const double* g, const double* Z, int64_t zw, int64_t M, const int32_t* mi,
                      const double* ys, const ThetaDev* theta, double jitter_s, int S, int64_t Nq, int64_t np, int B, double* R) {
    hipLaunchKernelGGL(bs_rhs_fwd_kernel, dim3((unsigned)((np + 255) / 256), S + 1, B), dim3(256), 0, h->stream, gd, g, Z, zw, M, mi,
                       ys, theta, jitter_s, S, Nq, np, B, 1.0 / sqrt((double)B), R);
    HIP_TRY(hipGetLastError());
    return GPIMHIP_OK;
}

// ------------------------------------------------------------------------------------------
// The two triangular sweeps with an EXPLICIT lower-triangular inverse factor T (L_b^-1 of the blocks, batched over
// blockIdx.y; L_S^-1 with one block): HBM-bound, the triangle is read once per group of SG columns, 16 bytes per lane along
// the rows.  Only entries T[i][j], j <= i < n are used (what lies above the diagonal or in the padding is never relied on).
//
// tri_fwd_multi_kernel: Y[c][i] = sum_{j <= i} T[i][j] X[c][j].  sample_draws_kernel without its mean / variance half: a
// workgroup owns TF_ROWS rows, two per wave; the columns go by in chunks of TF_CW whose slice of the SG vectors is staged in
// LDS once for the eight rows.  A lane adds its entries in increasing j, the wave's sum is the xor butterfly: the order of a
// column's sum depends on nothing but i.
// ------------------------------------------------------------------------------------------
#define TF_ROWS 8
#define TF_CW 256

template <int SG>
__global__ __launch_bounds__(256) void tri_fwd_multi_kernel(const double* __restrict__ T, int64_t ld, int64_t t_bs, int64_t n,
                                                            const double* __restrict__ X, double* __restrict__ Y, int64_t cs,
                                                            int64_t v_bs, int ncols) {
    __shared__ __attribute__((aligned(16))) double Xs[SG][TF_CW];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    T += (int64_t)blockIdx.y * t_bs;
    X += (int64_t)blockIdx.y * v_bs;
    Y += (int64_t)blockIdx.y * v_bs;
    const int64_t i0 = (int64_t)blockIdx.x * TF_ROWS, iw = i0 + 2 * wave;
    const double* row[2];
    int64_t lim[2];
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const bool rv = iw + r < n;
        row[r] = T + (rv ? iw + r : 0) * ld;
        lim[r] = rv ? iw + r : -1;
    }
    double acc[2][SG];
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int s = 0; s < SG; ++s) acc[r][s] = 0.0;
    const int64_t cend = i0 + TF_ROWS < n ? i0 + TF_ROWS : n;          // one past the workgroup's last column
    const bool rows_full = i0 + TF_ROWS <= n;
    for (int64_t c0 = 0; c0 < cend; c0 += TF_CW) {
        __syncthreads();                                    // the previous chunk has been read
        {
            const int64_t c = c0 + tid;
#pragma unroll
            for (int s = 0; s < SG; ++s) Xs[s][tid] = (c < n && s < ncols) ? X[(int64_t)s * cs + c] : 0.0;
        }
        __syncthreads();
        const bool interior = rows_full && c0 + TF_CW - 1 <= i0;
        auto body = [&](auto INTERIOR) {
#pragma unroll
            for (int hh = 0; hh < 2; ++hh) {
                const int e = hh * 128 + lane * 2;
                const int64_t c = c0 + e;
                double2 xv[SG];
#pragma unroll
                for (int s = 0; s < SG; ++s) xv[s] = *reinterpret_cast<const double2*>(&Xs[s][e]);
#pragma unroll
                for (int r = 0; r < 2; ++r) {
                    double2 l;
                    if (decltype(INTERIOR)::value) {
                        l = *reinterpret_cast<const double2*>(row[r] + c);
                    } else {
                        l.x = l.y = 0.0;
                        if (c + 1 <= lim[r]) l = *reinterpret_cast<const double2*>(row[r] + c);
                        else if (c <= lim[r]) l.x = row[r][c];
                    }
#pragma unroll
                    for (int s = 0; s < SG; ++s) {
                        acc[r][s] = fma(l.x, xv[s].x, acc[r][s]);
                        acc[r][s] = fma(l.y, xv[s].y, acc[r][s]);
                    }
                }
            }
        };
        if (interior) body(std::true_type{});
        else body(std::false_type{});
    }
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int s = 0; s < SG; ++s) acc[r][s] = bs_wave_sum(acc[r][s]);
    if (lane != 0) return;
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        if (lim[r] < 0) continue;
#pragma unroll
        for (int s = 0; s < SG; ++s)
            if (s < ncols) Y[(int64_t)s * cs + iw + r] = acc[r][s];
    }
}
// X, Y: the group's first column (column c at + c cs, block b at + b v_bs); ncols = sample_draw_group(columns left)
int launch_tri_fwd_multi(gpimhip_ctx* h, const double* T, int64_t ld, int64_t t_bs, int64_t n, int B, const double* X, double* Y,
                         int64_t cs, int64_t v_bs, int ncols) {
    if (n < 1) return GPIMHIP_OK;
    const dim3 grid((unsigned)((n + TF_ROWS - 1) / TF_ROWS), B), block(256);
#define TF_LAUNCH(SG) hipLaunchKernelGGL(tri_fwd_multi_kernel<SG>, grid, block, 0, h->stream, T, ld, t_bs, n, X, Y, cs, v_bs, ncols)
    if (ncols >= 5) TF_LAUNCH(8);
    else if (ncols >= 3) TF_LAUNCH(4);
    else if (ncols == 2) TF_LAUNCH(2);
    else TF_LAUNCH(1);
#undef TF_LAUNCH
    HIP_TRY(hipGetLastError());
    return GPIMHIP_OK;
}

// ------------------------------------------------------------------------------------------
// tri_bwd_multi_kernel: Y[c][j] = sum_{i >= j} T[i][j] X[c][i], the transposed sweep.  gemv_t_tri_kernel for SG columns: the
// ROWS are cut into chunks of rc (tri_bwd_rc: a function of the padded order alone), workgroup (64-column strip, chunk)
// handles what lies at or below the strip's first row and writes 64 partial sums per column to part[chunk][column][j] (pg columns per chunk: the call's largest group); a
// wave reads two rows x 512 bytes per load (lane: row parity, column pair), four loads in flight, the chunk's slice of the
// SG vectors staged in LDS 256 rows at a time.  Y[c][j] = the chunks' partial sums from the first chunk that holds a row
// >= 64 (j / 64) on, in increasing order (tri_bwd_sum_kernel).
// ------------------------------------------------------------------------------------------
#define TB_XR 256

template <int SG>
__global__ __launch_bounds__(256) void tri_bwd_multi_kernel(const double* __restrict__ T, int64_t ld, int64_t t_bs, int64_t n,
                                                            const double* __restrict__ X, int64_t cs, int64_t v_bs, int ncols,
                                                            double* __restrict__ part, int64_t np, int rc, int nR, int pg) {
    __shared__ __attribute__((aligned(16))) double xs[TB_XR][SG];
    __shared__ double2 red[4][SG][32];
    const int cb = blockIdx.x / nR, r = blockIdx.x % nR;
    const int64_t strip0 = (int64_t)cb * 64;
    int64_t i0 = (int64_t)r * rc, i1 = i0 + rc < n ? i0 + rc : n;
    if (i1 <= strip0) return;                               // above the strip: never read by the sum
    if (i0 < strip0) i0 = strip0;
    T += (int64_t)blockIdx.y * t_bs;
    X += (int64_t)blockIdx.y * v_bs;
    part += (((int64_t)blockIdx.y * nR + r) * pg) * np;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, cp = lane & 31, rp = lane >> 5;
    const int64_t j0 = strip0 + 2 * cp;
    const double* col = T + j0;
    double2 acc[SG];
#pragma unroll
    for (int s = 0; s < SG; ++s) acc[s].x = acc[s].y = 0.0;
    for (int64_t b0 = i0; b0 < i1; b0 += TB_XR) {
        __syncthreads();                                    // the previous slice has been read
        {
            const int64_t i = b0 + tid;
#pragma unroll
            for (int s = 0; s < SG; ++s) xs[tid][s] = (i < i1 && s < ncols) ? X[(int64_t)s * cs + i] : 0.0;
        }
        __syncthreads();
        const int cnt = (int)(i1 - b0 < TB_XR ? i1 - b0 : TB_XR);
        auto row_step = [&](int il, double2 a) {
            const int64_t i = b0 + il;
            a.x = i >= j0 ? a.x : 0.0;                      // (the strict upper triangle is not relied on)
            a.y = i >= j0 + 1 ? a.y : 0.0;
#pragma unroll
            for (int s = 0; s < SG; ++s) {
                const double x = xs[il][s];
                acc[s].x = fma(a.x, x, acc[s].x);
                acc[s].y = fma(a.y, x, acc[s].y);
            }
        };
        int il = 2 * wave + rp;                             // rows il, il + 8, ... (8 = 4 waves x 2 rows)
        for (; il + 24 < cnt; il += 32) {
            const double2 a0 = *reinterpret_cast<const double2*>(col + (b0 + il) * ld);
            const double2 a1 = *reinterpret_cast<const double2*>(col + (b0 + il + 8) * ld);
            const double2 a2 = *reinterpret_cast<const double2*>(col + (b0 + il + 16) * ld);
            const double2 a3 = *reinterpret_cast<const double2*>(col + (b0 + il + 24) * ld);
            row_step(il, a0);
            row_step(il + 8, a1);
            row_step(il + 16, a2);
            row_step(il + 24, a3);
        }
        for (; il < cnt; il += 8) row_step(il, *reinterpret_cast<const double2*>(col + (b0 + il) * ld));
    }
#pragma unroll
    for (int s = 0; s < SG; ++s) {
        acc[s].x += __shfl_xor(acc[s].x, 32);               // the two row parities
        acc[s].y += __shfl_xor(acc[s].y, 32);
        if (rp == 0) red[wave][s][cp] = acc[s];
    }
    __syncthreads();
    if (tid < 32) {
#pragma unroll
        for (int s = 0; s < SG; ++s) {
            if (s >= ncols) continue;
            double2 t = red[0][s][cp];
            t.x = ((t.x + red[1][s][cp].x) + red[2][s][cp].x) + red[3][s][cp].x;
            t.y = ((t.y + red[1][s][cp].y) + red[2][s][cp].y) + red[3][s][cp].y;
            *reinterpret_cast<double2*>(part + (int64_t)s * np + j0) = t;
        }
    }
}
__global__ __launch_bounds__(256) void tri_bwd_sum_kernel(const double* __restrict__ part, int64_t np, int64_t n, int rc, int nR,
                                                          int pg, double* __restrict__ Y, int64_t cs, int64_t v_bs) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int s = blockIdx.y, b = blockIdx.z;
    if (j >= n) return;
    const int rl = (int)((n + rc - 1) / rc);                // chunks that hold a row < n
    double t = 0.0;
    for (int r = (int)(((j / 64) * 64) / rc); r < rl; ++r) t += part[((((int64_t)b * nR + r) * pg) + s) * np + j];
    Y[(int64_t)b * v_bs + (int64_t)s * cs + j] = t;
}
// part: B x tri_bwd_chunks(np) x pg x np, pg >= ncols (the largest group of the call)
int launch_tri_bwd_multi(gpimhip_ctx* h, const double* T, int64_t ld, int64_t t_bs, int64_t n, int64_t np, int B, const double* X,
                         double* Y, int64_t cs, int64_t v_bs, int ncols, double* part, int pg) {
    if (n < 1) return GPIMHIP_OK;
    if (pg < ncols) return GPIMHIP_E_BADARG;
    const int rc = tri_bwd_rc(np), nR = tri_bwd_chunks(np);
    const dim3 grid((unsigned)(((n + 63) / 64) * nR), B), block(256);
#define TB_LAUNCH(SG) \
    hipLaunchKernelGGL(tri_bwd_multi_kernel<SG>, grid, block, 0, h->stream, T, ld, t_bs, n, X, cs, v_bs, ncols, part, np, rc, nR, pg)
    if (ncols >= 5) TB_LAUNCH(8);
    else if (ncols >= 3) TB_LAUNCH(4);
    else if (ncols == 2) TB_LAUNCH(2);
    else TB_LAUNCH(1);
#undef TB_LAUNCH
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(tri_bwd_sum_kernel, dim3((unsigned)((n + 255) / 256), ncols, B), dim3(256), 0, h->stream,
                       (const double*)part, np, n, rc, nR, pg, Y, cs, v_bs);
    HIP_TRY(hipGetLastError());
    return GPIMHIP_OK;
}

// t[c][j] = sum_b coef_b(j) beta_b[c][q(j)] for the S1 columns (border_t_kernel's sum, b ascending); 0 on the padding j >= Mm
__global__ __launch_bounds__(256) void bs_t_kernel(const double* __restrict__ beta, int64_t np, int B, int S1,
                                                   const int32_t* __restrict__ q, const double* __restrict__ coef, int Mm,
                                                   int64_t mp, double* __restrict__ t) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int c = blockIdx.y;
    if (j >= mp) return;
    double v = 0.0;
    if (j < Mm)
        for (int b = 0; b < B; ++b) v = fma(coef[(int64_t)b * Mm + j], beta[((int64_t)b * S1 + c) * np + q[j]], v);
    t[(int64_t)c * mp + j] = v;
}
int launch_bs_t(gpimhip_ctx* h, const double* beta, int64_t np, int B, int S1, const int32_t* q, const double* coef, int Mm,
                int64_t mp, double* t) {
    hipLaunchKernelGGL(bs_t_kernel, dim3((unsigned)((mp + 255) / 256), S1), dim3(256), 0, h->stream, beta, np, B, S1, q, coef, Mm,
                       mp, t);
    HIP_TRY(hipGetLastError());
    return GPIMHIP_OK;
}

// alpha~_b[c] = beta_b[c] - Y_b v[c] in place, for the rows p < Nq of every block: the skinny product over the stacked
// (B np) x mp matrix Y, read once per group of SG columns.  Two rows per wave share the loads of v; a lane adds its entries
// in increasing k, the wave's sum is the butterfly.  v is zero on its padding (and so are Y's padding columns).
template <int SG>
__global__ __launch_bounds__(256) void bs_yv_kernel(const double* __restrict__ Yb, int64_t mp, int64_t np, int64_t Nq, int S1,
                                                    const double* __restrict__ v, int c0, int ncols, double* __restrict__ Al) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, b = blockIdx.y;
    const int64_t p0 = (int64_t)blockIdx.x * 8 + 2 * wave;
    if (p0 >= Nq) return;
    const bool two = p0 + 1 < Nq;
    const double* y0 = Yb + ((int64_t)b * np + p0) * mp;
    const double* y1 = y0 + (two ? mp : 0);
    double acc[2][SG];
#pragma unroll
    for (int s = 0; s < SG; ++s) acc[0][s] = acc[1][s] = 0.0;
    for (int64_t k = lane * 2; k < mp; k += 128) {
        const double2 a0 = *reinterpret_cast<const double2*>(y0 + k), a1 = *reinterpret_cast<const double2*>(y1 + k);
#pragma unroll
        for (int s = 0; s < SG; ++s) {
            double2 x;
            x.x = x.y = 0.0;
            if (s < ncols) x = *reinterpret_cast<const double2*>(v + (int64_t)(c0 + s) * mp + k);
            acc[0][s] = fma(a0.x, x.x, acc[0][s]);
            acc[0][s] = fma(a0.y, x.y, acc[0][s]);
            acc[1][s] = fma(a1.x, x.x, acc[1][s]);
            acc[1][s] = fma(a1.y, x.y, acc[1][s]);
        }
    }
#pragma unroll
    for (int s = 0; s < SG; ++s) {
        acc[0][s] = bs_wave_sum(acc[0][s]);
        acc[1][s] = bs_wave_sum(acc[1][s]);
    }
    if (lane != 0) return;
#pragma unroll
    for (int s = 0; s < SG; ++s) {
        if (s >= ncols) continue;
        double* a = Al + ((int64_t)b * S1 + c0 + s) * np + p0;
        a[0] -= acc[0][s];
        if (two) a[1] -= acc[1][s];
    }
}
int launch_bs_yv(gpimhip_ctx* h, const double* Yb, int64_t mp, int64_t np, int64_t Nq, int B, int S1, const double* v, int c0,
                 int ncols, double* Al) {
    const dim3 grid((unsigned)((Nq + 7) / 8), B), block(256);
#define YV_LAUNCH(SG) hipLaunchKernelGGL(bs_yv_kernel<SG>, grid, block, 0, h->stream, Yb, mp, np, Nq, S1, v, c0, ncols, Al)
    if (ncols >= 5) YV_LAUNCH(8);
    else if (ncols >= 3) YV_LAUNCH(4);
    else if (ncols == 2) YV_LAUNCH(2);
    else YV_LAUNCH(1);
#undef YV_LAUNCH
    HIP_TRY(hipGetLastError());
    return GPIMHIP_OK;
}

// Cc[b][c][p] (rows of Nq, the layout of pw_basis_t_kernel): c < S: (s - d) alpha~_b[c];  c == S: ys_b - s alpha~_y,b
__global__ __launch_bounds__(256) void bs_combine_kernel(const double* __restrict__ Al, const double* __restrict__ ys, int S,
                                                         int64_t Nq, int64_t np, const ThetaDev* __restrict__ th,
                                                         double jitter_s, double* __restrict__ Cc) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int c = blockIdx.y, b = blockIdx.z;
    if (p >= Nq) return;
    const double sd = th->diag_add, a = Al[((int64_t)b * (S + 1) + c) * np + p];
    double e = sd - jitter_s;
    e = e > 0.0 ? e : 0.0;
    Cc[((int64_t)b * (S + 1) + c) * Nq + p] = c < S ? e * a : ys[(int64_t)b * Nq + p] - sd * a;
}
int launch_bs_combine(gpimhip_ctx* h, const double* Al, const double* ys, int S, int64_t Nq, int64_t np, int B,
                      const ThetaDev* theta, double jitter_s, double* Cc) {
    hipLaunchKernelGGL(bs_combine_kernel, dim3((unsigned)((Nq + 255) / 256), S + 1, B), dim3(256), 0, h->stream, Al, ys, S, Nq, np,
                       theta, jitter_s, Cc);
    HIP_TRY(hipGetLastError());
    return GPIMHIP_OK;
}

// g2 = U^T Cc (S + 1 rows of M).  Observed point i: mean = g2[S][i], draw c = mean + (g2[c][i] - sqrt(s - d) Z[c][M + i]);
// missing point j at i: mean = -w[S][j], draw c = mean + (g[c][i] + w[c][j]).  (+ sqrt(noise) Z[c][2 M + i] unless noiseless)
__global__ __launch_bounds__(256) void bs_out_kernel(const double* __restrict__ g2, const double* __restrict__ g,
                                                     const double* __restrict__ wv, int64_t mp, const int32_t* __restrict__ mi,
                                                     int64_t M, int S, const double* __restrict__ Z, int64_t zw, int noiseless,
                                                     const ThetaDev* __restrict__ th, double jitter_s,
                                                     double* __restrict__ mean_out, double* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int c = blockIdx.y;
    if (i >= M) return;
    const int j = mi[i];
    const double mean = j >= 0 ? -wv[(int64_t)S * mp + j] : g2[(int64_t)S * M + i];
    if (c == S) {
        if (mean_out) mean_out[i] = mean;
        return;
    }
    double v;
    if (j >= 0) {
        v = mean + (g[(int64_t)c * M + i] + wv[(int64_t)c * mp + j]);
    } else {
        const double e = th->diag_add - jitter_s;
        v = mean + (g2[(int64_t)c * M + i] - sqrt(e > 0.0 ? e : 0.0) * Z[(int64_t)c * zw + M + i]);
    }
    if (!noiseless) v = fma(sqrt(th->noise), Z[(int64_t)c * zw + 2 * M + i], v);
    out[(int64_t)c * M + i] = v;
}
int launch_bs_out(gpimhip_ctx* h, const double* g2, const double* g, const double* wv, int64_t mp, const int32_t* mi, int64_t M,
                  int S, const double* Z, int64_t zw, int noiseless, const ThetaDev* theta, double jitter_s, double* mean_out,
                  double* out) {
    hipLaunchKernelGGL(bs_out_kernel, dim3((unsigned)((M + 255) / 256), S + 1), dim3(256), 0, h->stream, g2, g, wv, mp, mi, M, S, Z,
                       zw, noiseless, theta, jitter_s, mean_out, out);
    HIP_TRY(hipGetLastError());
    return GPIMHIP_OK;
}
