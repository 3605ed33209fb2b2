// engine.hip -- the non-GEMM device kernels that build and apply the covariance on the exact-GP hot path:
//   theta_kernel        u -> constrained hyper-parameters + chain-rule factors       (row a4)
//   kmat_kernel         LDS-tiled pairwise-distance + covariance build               (row a5)
//   kmat_refl_kernel    the same for the reflection blocks of a complete grid
//   pad / copy          matrices and vectors into and out of the padded workspace
//   trmv / gemv_t*      z = L^-1 y, alpha = L^-T z, mean = K*^T alpha                 (rows a7, a11)
//   kres                y - K alpha in double: the refinement step of single-precision handles
// What follows K^-1 in a training iteration is grad.hip; the prediction epilogues and leave-one-out are predict.hip, the
// acquisition sweep and ranking select.hip.  Row labels refer to SURVEY.md section 8(a).  All reductions use fixed-shape
// trees so results are bit-reproducible run to run.
#include "kfun.hpp"
#include <type_traits>
#include "theta.hpp"
#include "refl.hpp"
#include "tile128.hpp"

// ------------------------------------------------------------------------------------------
// u -> theta   (torch.distributions transform_to(interval) = Affine o Sigmoid with clipping;
//               transform_to(positive) = exp.  SURVEY App. A.2)
// ------------------------------------------------------------------------------------------
// Batch convention of this file: blockIdx.y = problem index b; every per-problem pointer advances by
// b times the stride passed next to it (workspace buffers of the B problems are stacked).
__global__ void theta_kernel(gpimhip_model_t m, const double* __restrict__ u, int ustride,
                             ThetaDev* __restrict__ out) {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        ThetaDev t;
        theta_from_u(m, u + (int64_t)blockIdx.y * ustride, t);
        out[blockIdx.y] = t;
    }
}

// raw = [s2, l_0.., alpha]  (operator-level gpimhip_kmat)
__global__ void theta_raw_kernel(gpimhip_model_t m, const double* __restrict__ raw, ThetaDev* __restrict__ out) {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        ThetaDev t;
        t.var = raw[0];
        for (int k = 0; k < GPIMHIP_MAX_DIM; ++k) {
            t.ls[k] = (k < m.dim) ? raw[1 + ((m.n_ls == 1) ? 0 : k)] : 1.0;
            t.inv_ls[k] = 1.0 / t.ls[k];
            t.dls_du[k] = 0.0;
        }
        t.alpha = (m.kernel == GPIMHIP_KERNEL_RQ) ? raw[1 + m.n_ls] : 1.0;
        t.noise = 0.0;
        t.diag_add = 0.0;
        t.dvar_du = t.dnoise_du = t.dalpha_du = 0.0;
        *out = t;
    }
}

int launch_theta(gpimhip_ctx* h, const gpimhip_model_t* m, const double* u) {
    const int P = 2 + m->n_ls + (m->kernel == GPIMHIP_KERNEL_RQ ? 1 : 0);
    hipLaunchKernelGGL(theta_kernel, dim3(1, h->nbatch), dim3(64), 0, h->stream, *m, u, P, h->theta);
    HIP_TRY(hipGetLastError());
    return GPIMHIP_OK;
}
int launch_theta_raw(gpimhip_ctx* h, const gpimhip_model_t* m, const double* raw) {
    hipLaunchKernelGGL(theta_raw_kernel, dim3(1), dim3(64), 0, h->stream, *m, raw, h->theta1);
    HIP_TRY(hipGetLastError());
    return GPIMHIP_OK;
}

// ------------------------------------------------------------------------------------------
// covariance build.  One workgroup = one 128x128 tile; the 128 + 128 scaled coordinate rows are
// staged once in LDS, every thread produces an 8x8 patch and stores 16-byte pairs so that each
// wave writes 4 rows x 256 contiguous bytes.
// ------------------------------------------------------------------------------------------
template <int KIND, typename R>
__global__ __launch_bounds__(256) void kmat_kernel(const double* __restrict__ X, int64_t N,
                                                   const double* __restrict__ Z, int64_t M, int d,
                                                   const ThetaDev* __restrict__ th, double diag_add,
                                                   int use_theta_diag, R* __restrict__ out, int64_t ld,
                                                   int ntc, int sym, int lower_only, int64_t x_bs, int64_t z_bs,
                                                   int64_t out_bs) {
    __shared__ double xa[128][5];
    __shared__ double xz[128][5];
    const int tid = threadIdx.x;
    X += blockIdx.y * x_bs;
    Z += blockIdx.y * z_bs;
    th += blockIdx.y;
    out += blockIdx.y * out_bs;
    int ci, cj;
    tile_from_linear(blockIdx.x, ntc, lower_only, ci, cj);
    const ThetaDev t = *th;
    tile_stage<5>(X, N, Z, M, d, t, ci, cj, xa, xz);
    __syncthreads();
    const double dadd = use_theta_diag ? t.diag_add : diag_add;
    const int ty = tid >> 4, tx = tid & 15;
    // a tile that lies inside the matrix and off its diagonal (all but 2 nb - 1 of the nb (nb + 1) / 2 lower tiles) needs
    // no per-entry bounds / diagonal tests (64-bit compares: a tenth of the entry's instructions)
    const bool interior = (int64_t)ci * 128 + 128 <= N && (int64_t)cj * 128 + 128 <= M && !(sym && ci == cj);
    auto body = [&](auto INTERIOR) {
#pragma unroll 2
        for (int rr = 0; rr < 8; ++rr) {
            const int r = ty + 16 * rr;
            const int64_t gi = (int64_t)ci * 128 + r;
            const double a0 = xa[r][0], a1 = xa[r][1], a2 = xa[r][2], a3 = xa[r][3], an = xa[r][4];
#pragma unroll
            for (int cc = 0; cc < 4; ++cc) {
                typename Vec2<R>::T v;
#pragma unroll
                for (int e = 0; e < 2; ++e) {
                    const int c = tx * 2 + 32 * cc + e;
                    const int64_t gj = (int64_t)cj * 128 + c;
                    double dot = a0 * xz[c][0];
                    dot = fma(a1, xz[c][1], dot);
                    dot = fma(a2, xz[c][2], dot);
                    dot = fma(a3, xz[c][3], dot);
                    double r2 = (an - 2.0 * dot) + xz[c][4];
                    r2 = clamp0_nan(r2);
                    double k = t.var * kfun_value<KIND>(r2, t.alpha);
                    if (!decltype(INTERIOR)::value) {
                        if (gi >= N || gj >= M) k = (sym && gi == gj) ? 1.0 : 0.0;
                        else if (sym && gi == gj) k += dadd;
                    }
                    v[e] = (R)k;
                }
                *reinterpret_cast<typename Vec2<R>::T*>(out + gi * ld + (int64_t)cj * 128 + tx * 2 + 32 * cc) = v;
            }
        }
    };
    if (interior) body(std::true_type{});
    else body(std::false_type{});
}

int launch_kmat(gpimhip_ctx* h, const gpimhip_model_t* m, const double* X, int64_t N, const double* Z,
                int64_t M, const ThetaDev* theta, double diag_add, int use_theta_diag, double* out,
                int64_t ld, int64_t rows_pad, int64_t cols_pad, int sym, int lower_only, int64_t x_bs,
                int64_t z_bs, int64_t out_bs) {
    const int ntr = (int)(rows_pad / 128), ntc = (int)(cols_pad / 128);
    const int64_t nblk = lower_only ? (int64_t)ntr * (ntr + 1) / 2 : (int64_t)ntr * ntc;
    if (nblk <= 0) return GPIMHIP_OK;
    const double* Zp = Z ? Z : X;
    const dim3 grid((unsigned)nblk, h->nbatch), block(256);
    if (!Z) z_bs = x_bs;
    return with_kind(m->kernel, [&](auto K) {
        constexpr int KIND = decltype(K)::value;
        auto launch = [&](auto* o) {
            typedef std::remove_pointer_t<decltype(o)> R;
            hipLaunchKernelGGL((kmat_kernel<KIND, R>), grid, block, 0, h->stream, X, N, Zp, M, m->dim, theta, diag_add,
                               use_theta_diag, o, ld, ntc, sym, lower_only, x_bs, z_bs, out_bs);
        };
        if (h->fp32) launch(reinterpret_cast<float*>(out));
        else launch(out);
        HIP_TRY(hipGetLastError());
        return GPIMHIP_OK;
    });
}

// ------------------------------------------------------------------------------------------
// small utilities
// ------------------------------------------------------------------------------------------
__global__ void pad_copy_kernel(const double* __restrict__ src, int64_t n, double* __restrict__ dst, int64_t np) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    src += blockIdx.y * n;
    dst += blockIdx.y * np;
    if (i < np) dst[i] = (i < n) ? src[i] : 0.0;
}
int launch_pad_copy(gpimhip_ctx* h, const double* src, int64_t n, double* dst, int64_t np) {
    hipLaunchKernelGGL(pad_copy_kernel, dim3((unsigned)((np + 255) / 256), h->nbatch), dim3(256), 0, h->stream, src,
                       n, dst, np);
    HIP_TRY(hipGetLastError());
    return GPIMHIP_OK;
}

// A[k,k] <- dinv[k] for every diagonal block (leaves of the triangular inversion)
template <typename R>
__global__ __launch_bounds__(256) void diag_inv_copy_kernel(R* __restrict__ A, int64_t ld,
                                                            const R* __restrict__ dinv, int64_t a_bs,
                                                            int64_t d_bs) {
    typedef typename Vec2<R>::T R2;
    const int k = blockIdx.x;
    A += blockIdx.y * a_bs;
    dinv += blockIdx.y * d_bs;
    R* dst = A + ((int64_t)k * NB) * ld + (int64_t)k * NB;
    const R* src = dinv + (int64_t)k * NB * NB;
    for (int e = threadIdx.x; e < NB * NB / 2; e += 256) {
        const int r = e >> 6, c2 = (e & 63) * 2;
        *reinterpret_cast<R2*>(dst + (int64_t)r * ld + c2) = *reinterpret_cast<const R2*>(src + r * NB + c2);
    }
}
int launch_diag_inv_copy(gpimhip_ctx* h, double* A, int64_t ld, int nb) {
    if (h->fp32)
        hipLaunchKernelGGL(diag_inv_copy_kernel<float>, dim3(nb, h->nbatch), dim3(256), 0, h->stream,
                           reinterpret_cast<float*>(A), ld, reinterpret_cast<const float*>(h->dinv.p), (int64_t)nb * NB * ld,
                           (int64_t)nb * NB * NB);
    else
        hipLaunchKernelGGL(diag_inv_copy_kernel<double>, dim3(nb, h->nbatch), dim3(256), 0, h->stream, A, ld, h->dinv,
                       (int64_t)nb * NB * ld, (int64_t)nb * NB * NB);
    HIP_TRY(hipGetLastError());
    return GPIMHIP_OK;
}

// copy an n x n user matrix into / out of the padded workspace (identity padding)
__global__ void pad_matrix_in_kernel(const double* __restrict__ src, int64_t n, int64_t lds_,
                                     double* __restrict__ dst, int64_t np) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= np * np) return;
    const int64_t r = idx / np, c = idx % np;
    double v;
    if (r < n && c < n) v = src[r * lds_ + c];
    else v = (r == c) ? 1.0 : 0.0;
    dst[idx] = v;
}
__global__ void pad_matrix_out_lower_kernel(const double* __restrict__ src, int64_t np,
                                            double* __restrict__ dst, int64_t n, int64_t ldd) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n * n) return;
    const int64_t r = idx / n, c = idx % n;
    if (c <= r) dst[r * ldd + c] = src[r * np + c];
}
int launch_pad_matrix_in(gpimhip_ctx* h, const double* src, int64_t n, int64_t ld, double* dst, int64_t np) {
    hipLaunchKernelGGL(pad_matrix_in_kernel, dim3((unsigned)((np * np + 255) / 256)), dim3(256), 0, h->stream,
                       src, n, ld, dst, np);
    HIP_TRY(hipGetLastError());
    return GPIMHIP_OK;
}
int launch_pad_matrix_out_lower(gpimhip_ctx* h, const double* src, int64_t np, double* dst, int64_t n, int64_t ld) {
    hipLaunchKernelGGL(pad_matrix_out_lower_kernel, dim3((unsigned)((n * n + 255) / 256)), dim3(256), 0,
                       h->stream, src, np, dst, n, ld);
    HIP_TRY(hipGetLastError());
    return GPIMHIP_OK;
}

// ------------------------------------------------------------------------------------------
// triangular matrix-vector products with L^-1 (lower, zeros above the diagonal inside blocks)
// ------------------------------------------------------------------------------------------

// z[i] = sum_{j < jend(i)} L[i][j] * y[j];  one wave per row, 4 rows per workgroup
template <typename R>
__global__ __launch_bounds__(256) void trmv_lower_kernel(const R* __restrict__ L, int64_t ld, int64_t np,
                                                         const double* __restrict__ y, double* __restrict__ z) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t i = (int64_t)blockIdx.x * 4 + wave;
    L += blockIdx.y * np * ld;
    y += blockIdx.y * np;
    z += blockIdx.y * np;
    if (i >= np) return;
    const int64_t jend = (i / NB + 1) * NB;
    const R* row = L + i * ld;
    double s = 0.0;
    for (int64_t j = lane * 2; j < jend; j += 128) {
        const typename Vec2<R>::T l = *reinterpret_cast<const typename Vec2<R>::T*>(row + j);
        const d2 v = *reinterpret_cast<const d2*>(y + j);
        s = fma((double)l[0], v[0], s);
        s = fma((double)l[1], v[1], s);
    }
    s = wave_sum(s);
    if (lane == 0) z[i] = s;
}

// out[j] = sum_{i >= i0(j)} A[i][j] * x[i] for 64 columns per workgroup; tri != 0 starts at the
// diagonal block of the column (A lower triangular), else at row 0.  HBM-bound (8 B per entry of
// A): 16 waves per workgroup, each with four 512-byte row segments in flight; fixed summation order.
#define GEMVT_WAVES 16
// (one workgroup per 64-column strip; the row-chunked form that alpha = L^-T z used until round 5 is gemv_t_tri_kernel below)
template <typename R>
__global__ __launch_bounds__(GEMVT_WAVES * 64) void gemv_t_kernel(const R* __restrict__ A, int64_t ld,
                                                                 int64_t nrows, const double* __restrict__ x,
                                                                 double* __restrict__ out, int tri, int64_t a_bs,
                                                                 int64_t x_bs, int64_t o_bs) {
    __shared__ double red[GEMVT_WAVES][64];
    A += blockIdx.y * a_bs;
    x += blockIdx.y * x_bs;
    out += blockIdx.y * o_bs;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t j = (int64_t)blockIdx.x * 64 + lane;
    const int64_t i0 = tri ? ((int64_t)blockIdx.x * 64 / NB) * NB : 0, i1 = nrows;
    const R* col = A + j;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
    int64_t i = i0 + wave;
    for (; i + 3 * GEMVT_WAVES < i1; i += 4 * GEMVT_WAVES) {
        const double a0 = (double)col[i * ld], a1 = (double)col[(i + GEMVT_WAVES) * ld];
        const double a2 = (double)col[(i + 2 * GEMVT_WAVES) * ld], a3 = (double)col[(i + 3 * GEMVT_WAVES) * ld];
        s0 = fma(a0, x[i], s0);
        s1 = fma(a1, x[i + GEMVT_WAVES], s1);
        s2 = fma(a2, x[i + 2 * GEMVT_WAVES], s2);
        s3 = fma(a3, x[i + 3 * GEMVT_WAVES], s3);
    }
    for (; i < i1; i += GEMVT_WAVES) s0 = fma((double)col[i * ld], x[i], s0);
    red[wave][lane] = (s0 + s1) + (s2 + s3);
    __syncthreads();
    if (wave == 0) {
        double t = 0.0;
#pragma unroll
        for (int w = 0; w < GEMVT_WAVES; ++w) t += red[w][lane];
        out[j] = t;
    }
}

int launch_trmv_lower(gpimhip_ctx* h, const double* L, int64_t ld, int64_t np, const double* y, double* z) {
    if (h->fp32)
        hipLaunchKernelGGL(trmv_lower_kernel<float>, dim3((unsigned)((np + 3) / 4), h->nbatch), dim3(256), 0, h->stream,
                           reinterpret_cast<const float*>(L), ld, np, y, z);
    else
        hipLaunchKernelGGL(trmv_lower_kernel<double>, dim3((unsigned)((np + 3) / 4), h->nbatch), dim3(256), 0, h->stream, L, ld,
                       np, y, z);
    HIP_TRY(hipGetLastError());
    return GPIMHIP_OK;
}
int launch_gemv_t(gpimhip_ctx* h, const double* A, int64_t ld, int64_t nrows, int64_t ncols, const double* x,
                  double* out, int tri, int64_t a_bs, int64_t x_bs, int64_t o_bs) {
    const dim3 grid((unsigned)(ncols / 64), h->nbatch);
    if (h->fp32)
        hipLaunchKernelGGL(gemv_t_kernel<float>, grid, dim3(GEMVT_WAVES * 64), 0, h->stream,
                           reinterpret_cast<const float*>(A), ld, nrows, x, out, tri, a_bs, x_bs, o_bs);
    else
        hipLaunchKernelGGL(gemv_t_kernel<double>, grid, dim3(GEMVT_WAVES * 64), 0, h->stream, A, ld, nrows,
                       x, out, tri, a_bs, x_bs, o_bs);
    HIP_TRY(hipGetLastError());
    return GPIMHIP_OK;
}

// ------------------------------------------------------------------------------------------
// alpha = L^-T z over the lower-triangular L^-1 (round 6).  The strip of a 64-column block starts at its diagonal
// block, so strips run from np rows down to 128: cutting every strip into the SAME number of chunks (round 5's form of the kernel above)
// leaves the launch waiting for the first strips' workgroups -- 1.5 TB/s at np = 16384.  Here the ROWS are cut into
// chunks of rc (gemv_tri_rc: ~np / 32, a multiple of 128, 128 ... 1024): workgroup (column block, chunk) handles what
// lies at or below the block's diagonal block -- equal work per workgroup, thousands of workgroups of four waves --
// and writes 64 partial sums to part[chunk][column].  A wave reads two rows x 512 bytes per instruction (lane: row
// parity, column pair), four instructions in flight.  alpha_j = sum over the chunks r >= r0(j) in increasing order:
// gemv_tri_sum_kernel, or the consumer itself (grad_reduce_kernel sums the 256 entries it needs: gemv_tri_alpha).
// ------------------------------------------------------------------------------------------
template <typename R>
__global__ __launch_bounds__(256) void gemv_t_tri_kernel(const R* __restrict__ A, int64_t ld, int64_t np,
                                                         const double* __restrict__ x, double* __restrict__ part, int rc,
                                                         int nR, int64_t a_bs) {
    __shared__ d2 red[4][32];
    const int cb = blockIdx.x / nR, r = blockIdx.x % nR;
    const int64_t diag0 = ((int64_t)cb * 64 / NB) * NB;
    int64_t i0 = (int64_t)r * rc, i1 = i0 + rc < np ? i0 + rc : np;
    if (i1 <= diag0) return;                                   // structurally zero: never read by the sum
    if (i0 < diag0) i0 = diag0;
    A += blockIdx.y * a_bs;
    x += blockIdx.y * np;
    part += ((int64_t)blockIdx.y * nR + r) * np;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, cp = lane & 31, rp = lane >> 5;
    typedef typename Vec2<R>::T RV;
    const R* col = A + (int64_t)cb * 64 + 2 * cp;
    d2 s0 = (d2){0.0, 0.0}, s1 = s0, s2 = s0, s3 = s0;
    int64_t i = i0 + 2 * wave + rp;                             // rows i, i + 8, i + 16, ... (8 = 4 waves x 2 rows)
    for (; i + 24 < i1; i += 32) {
        const RV a0 = *reinterpret_cast<const RV*>(col + i * ld), a1 = *reinterpret_cast<const RV*>(col + (i + 8) * ld);
        const RV a2 = *reinterpret_cast<const RV*>(col + (i + 16) * ld), a3 = *reinterpret_cast<const RV*>(col + (i + 24) * ld);
        const double x0 = x[i], x1 = x[i + 8], x2 = x[i + 16], x3 = x[i + 24];
        s0[0] = fma((double)a0[0], x0, s0[0]); s0[1] = fma((double)a0[1], x0, s0[1]);
        s1[0] = fma((double)a1[0], x1, s1[0]); s1[1] = fma((double)a1[1], x1, s1[1]);
        s2[0] = fma((double)a2[0], x2, s2[0]); s2[1] = fma((double)a2[1], x2, s2[1]);
        s3[0] = fma((double)a3[0], x3, s3[0]); s3[1] = fma((double)a3[1], x3, s3[1]);
    }
    for (; i < i1; i += 8) {
        const RV a0 = *reinterpret_cast<const RV*>(col + i * ld);
        const double x0 = x[i];
        s0[0] = fma((double)a0[0], x0, s0[0]); s0[1] = fma((double)a0[1], x0, s0[1]);
    }
    d2 v;
    v[0] = (s0[0] + s1[0]) + (s2[0] + s3[0]);
    v[1] = (s0[1] + s1[1]) + (s2[1] + s3[1]);
    v[0] += __shfl_xor(v[0], 32);                               // the two row parities (both halves end with the same sum)
    v[1] += __shfl_xor(v[1], 32);
    if (rp == 0) red[wave][cp] = v;
    __syncthreads();
    if (threadIdx.x < 32) {
        d2 t = red[0][cp];
        t[0] = ((t[0] + red[1][cp][0]) + red[2][cp][0]) + red[3][cp][0];
        t[1] = ((t[1] + red[1][cp][1]) + red[2][cp][1]) + red[3][cp][1];
        *reinterpret_cast<d2*>(part + (int64_t)cb * 64 + 2 * cp) = t;
    }
}
__global__ __launch_bounds__(256) void gemv_tri_sum_kernel(const double* __restrict__ part, int nR, int rc, int64_t np,
                                                           double* __restrict__ out) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= np) return;
    out[blockIdx.y * np + j] = gemv_tri_alpha(part + (int64_t)blockIdx.y * nR * np, nR, rc, np, j);
}
// part: gemv_tri_chunks(np) * np doubles per problem (h->gemv_part); out == nullptr: the consumer sums the partials itself
int launch_gemv_t_tri(gpimhip_ctx* h, const double* A, int64_t ld, int64_t np, const double* x, double* part, double* out) {
    const int rc = gemv_tri_rc(np), nR = gemv_tri_chunks(np);
    const dim3 grid((unsigned)((np / 64) * nR), h->nbatch);
    if (h->fp32)
        hipLaunchKernelGGL(gemv_t_tri_kernel<float>, grid, dim3(256), 0, h->stream, reinterpret_cast<const float*>(A), ld, np, x,
                           part, rc, nR, np * ld);
    else
        hipLaunchKernelGGL(gemv_t_tri_kernel<double>, grid, dim3(256), 0, h->stream, A, ld, np, x, part, rc, nR, np * ld);
    HIP_TRY(hipGetLastError());
    if (out) {
        hipLaunchKernelGGL(gemv_tri_sum_kernel, dim3((unsigned)((np + 255) / 256), h->nbatch), dim3(256), 0, h->stream,
                           (const double*)part, nR, rc, np, out);
        HIP_TRY(hipGetLastError());
    }
    return GPIMHIP_OK;
}

// ------------------------------------------------------------------------------------------
// residual r = y - (K + (jitter + noise) I) alpha with K generated on the fly in double (kmat_kernel's
// arithmetic): the iterative-refinement step of single-precision handles.  alpha = K^-1 y through an fp32 factor
// and its explicit fp32 inverse is off by eps32 * cond(K); one pass  alpha += K32^-1 (y - K alpha)  squares that
// factor.  Workgroup = 128 rows x every S-th column block; partial sums in part[s][row], summed in order.
// ------------------------------------------------------------------------------------------
template <int KIND>
__global__ __launch_bounds__(256) void kres_partial_kernel(const double* __restrict__ X, int64_t N, int d,
                                                           const double* __restrict__ alpha,
                                                           const ThetaDev* __restrict__ th, double* __restrict__ part,
                                                           int64_t x_bs, int64_t np, int S) {
    __shared__ double xz[128][5];
    __shared__ double al[128];
    __shared__ double red[128];
    const int tid = threadIdx.x, r = tid & 127, half = tid >> 7;
    const int ci = blockIdx.x / S, s0 = blockIdx.x % S, nb = (int)(np / NB);
    X += blockIdx.y * x_bs;
    alpha += blockIdx.y * np;
    th += blockIdx.y;
    part += (int64_t)blockIdx.y * S * np;
    const ThetaDev t = *th;
    const int64_t gi = (int64_t)ci * 128 + r;
    double a[4], an = 0.0;
#pragma unroll
    for (int k = 0; k < GPIMHIP_MAX_DIM; ++k) {
        a[k] = (k < d && gi < N) ? X[gi * d + k] / t.ls[k] : 0.0;
        an += a[k] * a[k];
    }
    double acc = 0.0;
    for (int cj = s0; cj < nb; cj += S) {
        __syncthreads();
        if (tid < 128) {
            const int64_t g = (int64_t)cj * 128 + tid;
            double s2 = 0.0;
            for (int k = 0; k < GPIMHIP_MAX_DIM; ++k) {
                const double v = (k < d && g < N) ? X[g * d + k] / t.ls[k] : 0.0;
                xz[tid][k] = v;
                s2 += v * v;
            }
            xz[tid][4] = s2;
            al[tid] = (g < N) ? alpha[g] : 0.0;
        }
        __syncthreads();
        for (int c = half * 64; c < half * 64 + 64; ++c) {
            double dot = a[0] * xz[c][0];
            dot = fma(a[1], xz[c][1], dot);
            dot = fma(a[2], xz[c][2], dot);
            dot = fma(a[3], xz[c][3], dot);
            const double r2 = clamp0_nan((an - 2.0 * dot) + xz[c][4]);
            acc = fma(t.var * kfun_value<KIND>(r2, t.alpha), al[c], acc);
        }
    }
    __syncthreads();
    if (half == 1) red[r] = acc;
    __syncthreads();
    if (half == 0) part[(int64_t)s0 * np + gi] = (gi < N) ? acc + red[r] : 0.0;
}
__global__ void kres_final_kernel(const double* __restrict__ y, const double* __restrict__ alpha,
                                  const double* __restrict__ part, const ThetaDev* __restrict__ th, int64_t N,
                                  int64_t np, int S, double* __restrict__ res) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= np) return;
    const int64_t o = (int64_t)blockIdx.y * np;
    double s = 0.0;
    for (int q = 0; q < S; ++q) s += part[((int64_t)blockIdx.y * S + q) * np + i];
    res[o + i] = (i < N) ? (y[o + i] - th[blockIdx.y].diag_add * alpha[o + i]) - s : 0.0;
}
__global__ void axpy_kernel(double* __restrict__ x, const double* __restrict__ d, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) x[i] += d[i];
}
// res <- ypad - K(theta) alpha   (scratch: S * np doubles per problem)
int launch_kres(gpimhip_ctx* h, const gpimhip_model_t* m, const double* X, int64_t x_bs, int64_t N, double* scratch,
                int S, double* res) {
    const int64_t np = h->np;
    const int nb = (int)(np / NB);
    const dim3 grid(nb * S, h->nbatch), block(256);
    GP_TRY(with_kind(m->kernel, [&](auto K) {
        hipLaunchKernelGGL((kres_partial_kernel<decltype(K)::value>), grid, block, 0, h->stream, X, N, m->dim, h->alpha, h->theta,
                           scratch, x_bs, np, S);
        return GPIMHIP_OK;
    }));
    hipLaunchKernelGGL(kres_final_kernel, dim3((unsigned)((np + 255) / 256), h->nbatch), dim3(256), 0, h->stream, h->ypad,
                       h->alpha, scratch, h->theta, N, np, S, res);
    HIP_TRY(hipGetLastError());
    return GPIMHIP_OK;
}
int launch_axpy(gpimhip_ctx* h, double* x, const double* d, int64_t n) {
    hipLaunchKernelGGL(axpy_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, x, d, n);
    HIP_TRY(hipGetLastError());
    return GPIMHIP_OK;
}

// ------------------------------------------------------------------------------------------
// Symmetry-reduced exact GP on a complete uniform grid (reconstructor(structured=True) with a kernel that does not
// factorise over the axes: role of the reference's structured class gpim/gpreg/skgpr.py:399-448, exact instead of SKI).
// A stationary kernel that is even in every coordinate difference commutes with the reflections g of the grid about
// its centre planes; in the basis  v_{s,p} = |G|^-1/2 sum_g chi_s(g) e_{g p}  (p in the fundamental domain: the first
// half of every reflected axis, s a sign pattern, chi_s(g) = prod_{k in g} s_k) the covariance is block diagonal with
//     K_s[p, q] = sum_g chi_s(g) k(p, g q)              (N / |G| points each, |G| = 2^(reflected axes))
// and (noise + jitter) I stays what it is.  The |G| blocks are the problems of ONE lock-step batch (problem b <-> sign
// pattern: bit j of b = the sign of the j-th reflected axis is -1) with ONE set of hyper-parameters: their gradient sums,
// quadratic forms and log-determinants add up (finalize_coupled_kernel).  Cost of the O(N^3) stages: |G|^-2 of the dense
// model -- 1/16 in two dimensions.  Exact up to rounding: an orthogonal change of basis.
// ------------------------------------------------------------------------------------------
// ReflPair, refl_sign_dims, refl_for_each: refl.hpp
template <int KIND>
__global__ __launch_bounds__(256) void kmat_refl_kernel(const double* __restrict__ X, int64_t N, const double* __restrict__ Z,
                                                        int64_t M, int d, const ThetaDev* __restrict__ th, double* __restrict__ out,
                                                        int64_t ld, int ntc, int sym, int64_t x_bs, int64_t z_bs, int64_t out_bs,
                                                        ReflArgs refl, double scale) {
    __shared__ double xa[128][4];
    __shared__ double xz[128][4];
    __shared__ double wr_s[128], wc_s[128];
    const int tid = threadIdx.x;
    const int sg = refl_sign_dims(refl.mask, refl.pb_off + (int)blockIdx.y * refl.pb_stride);
    X += blockIdx.y * x_bs;
    Z += blockIdx.y * z_bs;
    th += blockIdx.y;
    out += blockIdx.y * out_bs;
    const double* wts = refl.wts ? refl.wts + (int64_t)blockIdx.y * N : nullptr;
    int ci, cj;
    tile_from_linear(blockIdx.x, ntc, sym, ci, cj);            // (sym: the factorisation reads the lower tiles only)
    const ThetaDev t = *th;
    {
        const TileSlot s = tile_stage<4>(X, N, Z, M, d, t, ci, cj, xa, xz);
        // weights of the block's points (rows; the columns too when they are the same points)
        tile_put(s, wr_s, wc_s, (wts && (s.isrow || sym) && s.valid) ? wts[s.g] : 1.0);
    }
    __syncthreads();
    double cz[GPIMHIP_MAX_DIM];
#pragma unroll
    for (int k = 0; k < GPIMHIP_MAX_DIM; ++k) cz[k] = (k < d) ? refl.twoc[k] / t.ls[k] : 0.0;
    const int ty = tid >> 4, tx = tid & 15;
    for (int rr = 0; rr < 8; ++rr) {
        const int r = ty + 16 * rr;
        const int64_t gi = (int64_t)ci * 128 + r;
        const double a0 = xa[r][0], a1 = xa[r][1], a2 = xa[r][2], a3 = xa[r][3];
#pragma unroll
        for (int cc = 0; cc < 4; ++cc) {
            d2 v;
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                const int c = tx * 2 + 32 * cc + e;
                const int64_t gj = (int64_t)cj * 128 + c;
                const double av[4] = {a0, a1, a2, a3};
                ReflPair p;
#pragma unroll
                for (int k = 0; k < GPIMHIP_MAX_DIM; ++k) {
                    const double dm = av[k] - xz[c][k], dp = (av[k] + xz[c][k]) - cz[k];
                    p.dm2[k] = dm * dm;
                    p.dp2[k] = dp * dp;
                }
                double acc = 0.0;
                refl_for_each(p, refl.mask, sg, [&](int, double chi, double r2) { acc = fma(chi, kfun_value<KIND>(r2, t.alpha), acc); });
                const double ww = wr_s[r] * wc_s[c];
                double k = scale * t.var * acc * ww;
                if (gi >= N || gj >= M || (sym && ww == 0.0)) k = (sym && gi == gj) ? 1.0 : 0.0;      // padding / absent points
                else if (sym && gi == gj) k += t.diag_add;
                v[e] = k;
            }
            *reinterpret_cast<d2*>(out + gi * ld + (int64_t)cj * 128 + tx * 2 + 32 * cc) = v;
        }
    }
}
int launch_kmat_refl(gpimhip_ctx* h, const gpimhip_model_t* m, const double* X, int64_t N, const double* Z, int64_t M,
                     const ThetaDev* theta, double* out, int64_t ld, int64_t rows_pad, int64_t cols_pad, int sym, int64_t x_bs,
                     int64_t z_bs, int64_t out_bs, double scale) {
    const int ntr = (int)(rows_pad / 128), ntc = (int)(cols_pad / 128);
    if (ntr <= 0 || ntc <= 0) return GPIMHIP_OK;
    const double* Zp = Z ? Z : X;
    if (!Z) z_bs = x_bs;
    const dim3 grid((unsigned)(sym ? ntr * (ntr + 1) / 2 : ntr * ntc), h->nbatch), block(256);
    return with_kind(m->kernel, [&](auto K) {
        hipLaunchKernelGGL((kmat_refl_kernel<decltype(K)::value>), grid, block, 0, h->stream, X, N, Zp, M, m->dim, theta, out, ld,
                           ntc, sym, x_bs, z_bs, out_bs, h->refl, scale);
        HIP_TRY(hipGetLastError());
        return GPIMHIP_OK;
    });
}

// The diagonal of a column slab of the covariance (columns row0 .. row0 + npad - 1 of the padded matrix):
// out[(row0 + j) * ld + j] += jitter + noise(theta) for the n valid columns, = 1 for the padding columns
__global__ void add_diag_theta_kernel(double* __restrict__ out, int64_t ld, int64_t row0, int64_t n, int64_t npad,
                                      const ThetaDev* __restrict__ th) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j < n) out[(row0 + j) * ld + j] += th->diag_add;
    else if (j < npad) out[(row0 + j) * ld + j] = 1.0;
}
int launch_add_diag_theta(gpimhip_ctx* h, double* out, int64_t ld, int64_t row0, int64_t n, int64_t npad) {
    hipLaunchKernelGGL(add_diag_theta_kernel, dim3((unsigned)((npad + 255) / 256)), dim3(256), 0, h->stream, out, ld, row0, n,
                       npad, h->theta);
    HIP_TRY(hipGetLastError());
    return GPIMHIP_OK;
}
