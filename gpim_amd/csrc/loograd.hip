// loograd.hip -- the leave-one-out objective (gpimhip_loo_grad, gpimhip_fit_exact_loo): from L^-1,
// alpha and the lower tiles of S^-1 to what the gradient contraction and the finalize step of a training iteration read.
// With d = diag(S^-1), q = alpha / d, r = S^-1 q, omega = 1 / d + alpha^2 / d^2 and G2 = S^-1 diag(omega) S^-1
//     loss = sum_i [ -1/2 log d_i + alpha_i^2 / (2 d_i) ] + N/2 log 2 pi + prior constant
//     d loss / d theta = 1/2 sum_ij dS_ij/d theta (G2_ij - (r_i alpha_j + alpha_i r_j))
// -- the marginal-likelihood gradient with G2 for S^-1 and the symmetric pair for alpha alpha^T.
//   loo_points_kernel   d from the row-chunk sums of colsq_tri_kernel, q, sqrt(omega), the block sums of -1/2 log d
//   loo_mirror_kernel   C = S^-1 diag(sqrt(omega)) as a full matrix from the lower tiles of S^-1
//   loo_grad_at_u       the schedule: ... -> lower(G2) = C C^T on the tile engine -> grad_reduce_kernel<LOO> -> finalize_kernel
// No atomics: every sum has one fixed order, two calls give the same bits.
#include "tile128.hpp"

// Block k of 128 threads: the points 128 k .. 128 k + 127.  Rows >= N (the identity padding) get q = sqrt(omega) = 0 and add
// nothing to the block's sum; their d is never read (colsq_tri_kernel leaves whole padding column blocks unwritten).
// lg_part[k] = -1/2 sum log d_i, the place of sum log L_ii in the finalize step (loss = 1/2 quad + lg + ...): the two waves'
// sums in the order (wave 0 + wave 1).
__global__ __launch_bounds__(128) void loo_points_kernel(const double* __restrict__ diag_part, int nR, int rc, int64_t np, int64_t N,
                                                         const double* __restrict__ alpha, double* __restrict__ q,
                                                         double* __restrict__ sw, double* __restrict__ lg_part) {
    __shared__ double red[2];
    const int64_t i = (int64_t)blockIdx.x * 128 + threadIdx.x;
    double qi = 0.0, si = 0.0, lg = 0.0;
    if (i < N) {
        const double d = gemv_tri_alpha(diag_part, nR, rc, np, i), a = alpha[i];
        qi = a / d;
        si = sqrt(1.0 / d + qi * qi);
        lg = -0.5 * log(d);
    }
    q[i] = qi;
    sw[i] = si;
    lg = wave_sum(lg);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = lg;
    __syncthreads();
    if (threadIdx.x == 0) lg_part[blockIdx.x] = red[0] + red[1];
}

// One workgroup per lower 64 x 64 tile (ti >= tj) of S^-1 (Sinv: its lower 128-tiles, what launch_lauum left).  The tile
// goes through LDS: written back scaled by the column's sqrt(omega) as tile (ti, tj) of C, and transposed, scaled by what
// is then the column's, as tile (tj, ti); a diagonal tile is completed from its lower half first.  Entries with a row or a
// column >= N are never read (a ragged factorisation leaves stale padding there) and are written as zeros, so C is defined
// on all np x np entries.  8 np^2 bytes written, 4 np^2 read: HBM-bound.
#define LOO_MT 64
__global__ __launch_bounds__(256) void loo_mirror_kernel(const double* __restrict__ Sinv, int64_t ld, int64_t N,
                                                         const double* __restrict__ sw, double* __restrict__ C) {
    __shared__ double t[LOO_MT][LOO_MT + 1];
    int ti, tj;
    lower_tile_from_linear(blockIdx.x, ti, tj);
    const int tid = threadIdx.x, cx = (tid & 31) * 2, ry = tid >> 5;      // a thread: two columns of eight rows
    const int64_t i0 = (int64_t)ti * LOO_MT, j0 = (int64_t)tj * LOO_MT;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int r = ry + 8 * k;
        const int64_t gi = i0 + r, gj = j0 + cx;
        d2 v = (d2){0.0, 0.0};
        if (gi < N && gj <= gi) {                                         // (gj even, gj + 1 may be past the diagonal or N)
            v = *reinterpret_cast<const d2*>(Sinv + gi * ld + gj);
            if (gj + 1 > gi) v[1] = 0.0;
        }
        t[r][cx] = v[0];
        t[r][cx + 1] = v[1];
    }
    __syncthreads();
    const bool diag = ti == tj;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int r = ry + 8 * k;
        const int64_t gi = i0 + r, gj = j0 + cx;
        d2 v;
        v[0] = (diag && cx > r) ? t[cx][r] : t[r][cx];
        v[1] = (diag && cx + 1 > r) ? t[cx + 1][r] : t[r][cx + 1];
        const d2 s = *reinterpret_cast<const d2*>(sw + gj);              // (0 for columns >= N)
        v[0] *= s[0];
        v[1] *= s[1];
        *reinterpret_cast<d2*>(C + gi * ld + gj) = v;
    }
    if (diag) return;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int r = ry + 8 * k;                                         // row j0 + r of C, columns i0 + cx, i0 + cx + 1
        const d2 s = *reinterpret_cast<const d2*>(sw + i0 + cx);
        d2 v;
        v[0] = t[cx][r] * s[0];
        v[1] = t[cx + 1][r] * s[1];
        *reinterpret_cast<d2*>(C + (j0 + r) * ld + i0 + cx) = v;
    }
}

// The workspace of the objective beyond the training workspace: three vectors of np (q, sqrt(omega), r) and the tile list of
// the product C C^T (every lower tile, the whole k-range).  Built outside any capture: both synchronise.
int loo_obj_ensure(gpimhip_ctx* h) {
    const int nb = (int)(h->np / NB);
    GP_TRY(h->loo_vec.grow(h, 3 * h->np));
    if (h->loo_tiles_nb == nb && h->loo_tiles) return GPIMHIP_OK;
    std::vector<TileDesc> tl;
    lower_patch_order(tl, 0, nb, 0, nb);
    HIP_TRY(hipStreamSynchronize(h->stream));
    h->loo_tiles.release(h);
    h->loo_tiles_nb = 0;
    GP_TRY(h->loo_tiles.alloc(h, (int64_t)tl.size()));
    HIP_TRY(hipMemcpyAsync(h->loo_tiles, tl.data(), tl.size() * sizeof(TileDesc), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    h->loo_tiles_nb = nb;
    return GPIMHIP_OK;
}

// One evaluation of the leave-one-out objective at u (one problem, double precision, the dense engine), after
// loo_obj_ensure.  h->Tm, the temporary of the triangular inverse, is free once L^-1 is in h->A: it holds C.  On return
// h->B holds the lower tiles of G2 (not S^-1), h->z = L^-1 q and h->gemv_part the row-chunk sums of r.
int loo_grad_at_u(gpimhip_ctx* h, const gpimhip_model_t* m, const double* X, int64_t N, double* u, int do_adam, AdamStep st,
                  const FinalizeOut& out, bool theta_carried) {
    const int64_t np = h->np, ld = h->ld;
    const int nb = (int)(np / NB), nt = (int)(np / LOO_MT);
    double *q = h->loo_vec, *sw = q + np, *r = sw + np;
    GP_TRY(factor_at_u(h, m, X, 0, N, u, theta_carried, false));
    { StageTimer t(h, 2); GP_TRY(launch_lauum(h, h->A, h->B, np, ld, rag_of(N, np))); }
    GP_TRY(launch_colsq_tri(h, h->A, ld, np, N, h->gemv_part));
    hipLaunchKernelGGL(loo_points_kernel, dim3(nb), dim3(128), 0, h->stream, (const double*)h->gemv_part, gemv_tri_chunks(np),
                       gemv_tri_rc(np), np, N, (const double*)h->alpha, q, sw, h->logdet_part.p);
    HIP_TRY(hipGetLastError());
    GP_TRY(launch_trmv_lower(h, h->A, ld, np, q, h->z));                  // r = L^-T (L^-1 q)
    GP_TRY(launch_gemv_t_tri(h, h->A, ld, np, h->z, h->gemv_part, r));
    hipLaunchKernelGGL(loo_mirror_kernel, dim3(nt * (nt + 1) / 2), dim3(256), 0, h->stream, (const double*)h->B, ld, N,
                       (const double*)sw, h->Tm.p);
    HIP_TRY(hipGetLastError());
    {
        // lower(G2) = C C^T (NT, A = B = C): N^3 flop, every tile the whole k-range
        GemmArgs g = gemm_args(h->Tm, ld, h->Tm, ld, h->B, ld, 1.0, 0.0, h->loo_tiles, (int)h->loo_tiles.cap, np);
        g.chunk = deal_chunk(g.ntiles);
        GP_TRY(launch_gemm(h, false, false, EPI_STORE, g));
    }
    GP_TRY(launch_grad_reduce_loo(h, m, h->B, ld, X, N, nb, h->alpha, r));
    return launch_finalize_vec(h, m, N, np, u, do_adam, st, out, theta_carried ? 1 : 0, h->alpha, q);
}
