// border.hip -- the exact GP on the observed points of an INCOMPLETE grid, computed from the reflection blocks of the
// completed grid plus a low-rank "border" for its M missing points (gpimhip_set_border).
//
// On the completed grid A = K + (noise + jitter) I is block diagonal in the reflection basis U (blocks B_b, engine.hip:
// kmat_refl_kernel).  With S = (A^-1)_mm (M x M), L_S = chol(S), y~ = y with 0 at the missing points:
//   A_oo^-1 embedded in the grid  =  A^-1 - A^-1 P_m S^-1 P_m^T A^-1
//   log det A_oo = log det A + log det S,   y_o^T A_oo^-1 y_o = y~^T A^-1 y~ - |L_S^-1 t|^2,   t = (A^-1 y~)_m
// Missing point j has ONE representative q(j) in the fundamental domain and coefficient c_b(j) in block b, so
//   S_ij = sum_b c_b(i) c_b(j) (B_b^-1)[q(i), q(j)],   C_b = (U^T A^-1 P_m)_b: column j = c_b(j) (B_b^-1)[:, q(j)]
//   Y_b = C_b L_S^-T,   alpha_b <- alpha_b - Y_b (L_S^-1 t),   B_b^-1 <- B_b^-1 - Y_b Y_b^T
// after which the unchanged gradient contraction (launch_grad_reduce_refl) sees the blocks of the observed model.
// The two products with Y run on the tile engine (api.hip: border_iter); the launches here are the gathers, the
// vector corrections and the prediction's sums of squares.  Every reduction has a fixed order: bit-reproducible.
// Multi-output GP (vgp.hip in reflection mode): the batch is T tasks of nrep = 2^r blocks each, and
// there are T borders S_t, one per task, handled in lock-step: the launches below take the task from blockIdx.y (the
// gather of C: the problem t nrep + b) and advance their per-task buffers by it.  q and coef are shared by the tasks.
#include "border.hpp"

// a wave's sum in a fixed butterfly order (the same bits on every run)
__device__ __forceinline__ double bd_wave_sum(double v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// (B_b^-1)[r, c] from the lower triangle the K^-1 product leaves
__device__ __forceinline__ double bd_sym(const double* __restrict__ Bi, int64_t ld, int64_t r, int64_t c) {
    return r >= c ? Bi[r * ld + c] : Bi[c * ld + r];
}

// S (mp x mp, row-major, every entry written): the lower triangle of sum_b c_b(i) c_b(j) B_b^-1[q(i), q(j)] with
// identity padding, zeros above the diagonal
__global__ __launch_bounds__(256) void border_gather_s_kernel(const double* __restrict__ Binv, int64_t ld, int64_t np, int B,
                                                              const int32_t* __restrict__ q, const double* __restrict__ coef,
                                                              int M, int64_t mp, double* __restrict__ S, int64_t lds, int64_t s_bs) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= mp * mp) return;
    Binv += (int64_t)blockIdx.y * B * np * ld;          // task t: its B blocks, its S
    S += (int64_t)blockIdx.y * s_bs;
    const int64_t i = e / mp, j = e - i * mp;
    double v = (i == j) ? 1.0 : 0.0;
    if (i < M && j <= i) {
        const int64_t qi = q[i], qj = q[j];
        v = 0.0;
        for (int b = 0; b < B; ++b)
            v = fma(coef[(int64_t)b * M + i] * coef[(int64_t)b * M + j], bd_sym(Binv + (int64_t)b * np * ld, ld, qi, qj), v);
    }
    S[i * lds + j] = v;
}
int launch_border_gather_s(gpimhip_ctx* h, const BorderWs* w, const double* Binv, int64_t ld, double* S, int64_t lds) {
    const int64_t n = w->mp * w->mp;
    hipLaunchKernelGGL(border_gather_s_kernel, dim3((unsigned)((n + 255) / 256), w->T), dim3(256), 0, h->stream, Binv, ld, h->np,
                       h->nbatch / w->T, w->q, w->coef, w->M, w->mp, S, lds, w->sub->np * lds);
    HIP_TRY(hipGetLastError());
    return GPIMHIP_OK;
}

// after the factorisation of S: zeros above the diagonal of L_S^-1's diagonal tiles (the products with Y read whole
// tiles), S's status word into the model's (a failed factorisation stops training like a failed block), and the
// former reset for the next iteration
__global__ __launch_bounds__(256) void border_tidy_kernel(double* __restrict__ Linv, int64_t lds, int64_t mp,
                                                          int32_t* __restrict__ sub_info, int32_t* __restrict__ info,
                                                          int64_t s_bs) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    Linv += (int64_t)blockIdx.y * s_bs;
    if (e == 0 && blockIdx.y == 0) {       // (one status word for the T factorisations, as for the model's blocks)
        const int32_t s = *sub_info;
        if (s != 0 && *info == 0) *info = s;
        *sub_info = 0;
    }
    if (e >= mp * NB) return;
    const int64_t i = e / NB, c = e - i * NB, j = (i / NB) * NB + c;
    if (j > i) Linv[i * lds + j] = 0.0;
}
int launch_border_tidy(gpimhip_ctx* h, const BorderWs* w, double* Linv, int64_t lds) {
    const int64_t n = w->mp * NB;
    hipLaunchKernelGGL(border_tidy_kernel, dim3((unsigned)((n + 255) / 256), w->T), dim3(256), 0, h->stream, Linv, lds, w->mp,
                       w->sub->info, h->info, w->sub->np * lds);
    HIP_TRY(hipGetLastError());
    return GPIMHIP_OK;
}

// C_b[p, j] = c_b(j) B_b^-1[p, q(j)] for the nq points of the domain, 0 on padding rows and columns; blockIdx.y: the
// problem (task-major: its block is blockIdx.y % B)
__global__ __launch_bounds__(256) void border_gather_c_kernel(const double* __restrict__ Binv, int64_t ld, int64_t np, int64_t nq,
                                                              int B, const int32_t* __restrict__ q,
                                                              const double* __restrict__ coef, int M, int64_t mp,
                                                              double* __restrict__ C) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= np * mp) return;
    const int pb = blockIdx.y, b = pb % B;
    const int64_t p = e / mp, j = e - p * mp;
    double v = 0.0;
    if (p < nq && j < M) v = coef[(int64_t)b * M + j] * bd_sym(Binv + (int64_t)pb * np * ld, ld, p, q[j]);
    C[(int64_t)pb * np * mp + e] = v;
}
int launch_border_gather_c(gpimhip_ctx* h, const BorderWs* w, const double* Binv, int64_t ld, int64_t nq) {
    const int64_t n = h->np * w->mp;
    hipLaunchKernelGGL(border_gather_c_kernel, dim3((unsigned)((n + 255) / 256), h->nbatch), dim3(256), 0, h->stream, Binv, ld,
                       h->np, nq, h->nbatch / w->T, w->q, w->coef, w->M, w->mp, w->C);
    HIP_TRY(hipGetLastError());
    return GPIMHIP_OK;
}

// t_j = sum_b c_b(j) alpha_b[q(j)]  (= (A^-1 y~)_j)
__global__ __launch_bounds__(256) void border_t_kernel(const double* __restrict__ alpha, int64_t np, int B,
                                                       const int32_t* __restrict__ q, const double* __restrict__ coef, int M,
                                                       int64_t mp, double* __restrict__ t) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= mp) return;
    alpha += (int64_t)blockIdx.y * B * np;
    t += (int64_t)blockIdx.y * 2 * mp;
    double v = 0.0;
    if (j < M)
        for (int b = 0; b < B; ++b) v = fma(coef[(int64_t)b * M + j], alpha[(int64_t)b * np + q[j]], v);
    t[j] = v;
}
// out[r] = sign * sum_k A[r * lda + k] x[k] (+ out[r] when accumulate), k < klim(r): one wave per row; task blockIdx.y
// has its operands a_bs, x_bs and o_bs further on
__global__ __launch_bounds__(256) void border_rowdot_kernel(const double* __restrict__ A, int64_t lda, int64_t rows, int64_t kcols,
                                                            int lower, const double* __restrict__ x, double* __restrict__ out,
                                                            int accumulate, int64_t a_bs, int64_t x_bs, int64_t o_bs) {
    const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (r >= rows) return;
    A += (int64_t)blockIdx.y * a_bs;
    x += (int64_t)blockIdx.y * x_bs;
    out += (int64_t)blockIdx.y * o_bs;
    const int64_t kn = lower ? r + 1 : kcols;
    double s = 0.0;
    for (int64_t k = lane; k < kn; k += 64) s = fma(A[r * lda + k], x[k], s);
    s = bd_wave_sum(s);
    if (lane == 0) out[r] = accumulate ? out[r] - s : s;
}
// scal[0] = |v|^2, scal[1] = sum log (L_S)_ii (the factorisation's per-block partial sums)
__global__ __launch_bounds__(256) void border_scal_kernel(const double* __restrict__ v, int64_t mp,
                                                          const double* __restrict__ logdet_part, int nbs, double* __restrict__ scal) {
    __shared__ double red[4];
    const int tid = threadIdx.x;
    v += (int64_t)blockIdx.x * 2 * mp;                   // task t: v_t, S_t's partial sums, its two scalars
    logdet_part += (int64_t)blockIdx.x * nbs;
    scal += 2 * blockIdx.x;
    double s = 0.0;
    for (int64_t i = tid; i < mp; i += 256) s = fma(v[i], v[i], s);
    s = bd_wave_sum(s);
    if ((tid & 63) == 0) red[tid >> 6] = s;
    __syncthreads();
    if (tid == 0) {
        scal[0] = (red[0] + red[1]) + (red[2] + red[3]);
        double l = 0.0;
        for (int k = 0; k < nbs; ++k) l += logdet_part[k];
        scal[1] = l;
    }
}
int launch_border_vectors(gpimhip_ctx* h, const BorderWs* w, const double* Linv, int64_t lds, const double* logdet_part, int nbs,
                          double* alpha) {
    const int64_t mp = w->mp;
    const int T = w->T, B = h->nbatch / T;
    double *t = w->tv, *v = w->tv + mp;                 // (task t: 2 mp further on)
    hipLaunchKernelGGL(border_t_kernel, dim3((unsigned)((mp + 255) / 256), T), dim3(256), 0, h->stream, alpha, h->np, B, w->q,
                       w->coef, w->M, mp, t);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(border_rowdot_kernel, dim3((unsigned)((mp + 3) / 4), T), dim3(256), 0, h->stream, Linv, lds, mp, mp, 1, t, v,
                       0, w->sub->np * lds, 2 * mp, 2 * mp);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(border_scal_kernel, dim3(T), dim3(256), 0, h->stream, v, mp, logdet_part, nbs, w->scal);
    HIP_TRY(hipGetLastError());
    // alpha_b -= Y_b v: a task's stacked blocks are one (B np) x mp matrix
    const int64_t rows = (int64_t)B * h->np;
    hipLaunchKernelGGL(border_rowdot_kernel, dim3((unsigned)((rows + 3) / 4), T), dim3(256), 0, h->stream, w->Y, mp, rows, mp, 0, v,
                       alpha, 1, rows * mp, 2 * mp, rows);
    HIP_TRY(hipGetLastError());
    return GPIMHIP_OK;
}

// rsq[j] = sum_i R[i, j]^2 for the chunk's cnt test points (fixed order over i)
__global__ __launch_bounds__(256) void border_colsumsq_kernel(const double* __restrict__ R, int64_t ldr, int64_t mp, int64_t cnt,
                                                              double* __restrict__ rsq) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= cnt) return;
    R += (int64_t)blockIdx.y * mp * ldr;                 // task t: R_t, its row of rsq
    rsq += (int64_t)blockIdx.y * ldr;
    double s = 0.0;
    for (int64_t i = 0; i < mp; ++i) s = fma(R[i * ldr + j], R[i * ldr + j], s);
    rsq[j] = s;
}
int launch_border_colsumsq(gpimhip_ctx* h, const BorderWs* w, int64_t cnt) {
    hipLaunchKernelGGL(border_colsumsq_kernel, dim3((unsigned)((cnt + 255) / 256), w->T), dim3(256), 0, h->stream, w->R, w->r_cols,
                       w->mp, cnt, w->rsq);
    HIP_TRY(hipGetLastError());
    return GPIMHIP_OK;
}

// uo (B x N) = U 1_o, the indicator of the observed points in the adapted basis: (U 1)_b = sqrt(B) w_0 in block 0 and 0 in
// the others, minus c_b(j) at q(j) for every missing point j -- in the order of j (several can share a representative)
__global__ __launch_bounds__(256) void border_ones_kernel(int64_t N, int B, const double* __restrict__ wts,
                                                          const int32_t* __restrict__ q, const double* __restrict__ coef, int M,
                                                          double* __restrict__ uo) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int b = blockIdx.y;
    if (i >= N) return;
    double v = (b == 0) ? sqrt((double)B) * (wts ? wts[i] : 1.0) : 0.0;
    for (int j = 0; j < M; ++j)
        if (q[j] == i) v -= coef[(int64_t)b * M + j];
    uo[(int64_t)b * N + i] = v;
}
int launch_border_ones(gpimhip_ctx* h, const BorderWs* w, int64_t N, int B, double* uo) {
    hipLaunchKernelGGL(border_ones_kernel, dim3((unsigned)((N + 255) / 256), B), dim3(256), 0, h->stream, N, B, h->refl.wts, w->q,
                       w->coef, w->M, uo);
    HIP_TRY(hipGetLastError());
    return GPIMHIP_OK;
}
