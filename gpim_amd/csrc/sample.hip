// sample.hip -- joint draws from the posterior of the exact GP (gpimhip_sample_exact).
//
// The joint covariance J of the stacked points [X; Xs] is factored once by the engine's Cholesky (api.hip:
// sample_impl).  In chol(J) = [[L11, 0], [L21, L22]] the right-looking factorisation has formed the Schur complement on
// its way: L21 = (L11^-1 K*)^T and L22 = chol(K** - K*^T K^-1 K* + d I), so with z = L11^-1 y and one row
// [z; z_s] per draw everything the caller wants is a product with the trapezoid L[N:, :]:
//   mean_i = L[N+i, :N] z        var_i = sum_k L22[i,k]^2 - d + noise        f_s,i = mean_i + L22[i, :i+1] z_s[:i+1]
// sample_draws_kernel reads the trapezoid once per group of up to eight draws and produces all three.
#include "sample.hpp"

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
