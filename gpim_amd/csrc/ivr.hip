// ivr.hip -- integrated variance reduction (ALC) of the exact GP: gpimhip_ivr_exact.
//
// With S = K + (noise + jitter) I, W = L^-1 K(X, G) and C = K(G, G) - W^T W (the latent posterior covariance on the M rows
// of the test grid G) measuring candidate j lowers the latent variance at grid point m by C_mj^2 / (C_jj + noise + jitter):
//     a_j = sum_m w_m C_mj^2 / (max(C_jj, 0) + noise + jitter)
// The entry runs the model's state at u, W through the tile engine's NN store layout (the launch of predict_cols with
// EPI_STORE), the mean on predict_cols' path, the LOWER tiles of C (symmetric build, then one TN launch with alpha = -1,
// beta = 1 over the lower tile list), and two kernels of its own:
//   colsq_sym_kernel   s_j = sum_m w_m C_mj^2 from lower-stored C, every stored entry read once
//   ivr_finish_kernel  the partial sums added in their order, the quotient, sd and the mask
// W, C and the partial sums belong to this entry (IvrWs; grow-only, charged to h->bytes).
#include <algorithm>
#include "common.hpp"
#include "border.hpp"
#include "kfun.hpp"

typedef double d2 __attribute__((ext_vector_type(2)));

struct IvrWs {
    DevBuf<double> W;               // np x ldm: L^-1 K(X, G), rows >= N zero
    DevBuf<double> C;               // mp x ldm: lower tiles of the latent posterior covariance
    DevBuf<double> part;            // (mp / 128) x mp: part[k][j] = sum over the rows m of block k of w_m C_mj^2
    DevBuf<TileDesc> tiles;         // lower tiles of an nt x nt block matrix
    int nt = 0;
};
static IvrWs* iws(gpimhip_ctx* h) {
    if (!h->ivr) h->ivr = new IvrWs();
    return (IvrWs*)h->ivr;
}
void ivr_release(gpimhip_ctx* h) {
    IvrWs* w = (IvrWs*)h->ivr;
    if (!w) return;
    dev_release(h, w->W, w->C, w->part, w->tiles);
    delete w;
    h->ivr = nullptr;
}

// ------------------------------------------------------------------------------------------
// Symmetric squared column sums.  One workgroup = one stored 128 x 128 tile (ti, tj), ti >= tj, of C (rows of ld doubles).
// Threads as in kmat_kernel: thread (ty, tx) of 16 x 16 holds rows ty + 16 rr and the column pairs 2 tx + 32 cc, so a wave
// reads 4 rows x 256 contiguous bytes per instruction; every entry is loaded once and serves both sums it belongs to:
//   the column walk   part[ti][tj * 128 + c] = sum_r w_(ti, r) C(r, c)^2      (C_mj, m in block ti, for the columns of block tj)
//   the row walk      part[tj][ti * 128 + r] = sum_c w_(tj, c) C(r, c)^2      (C_jm read as C_mj, m in block tj, for block ti)
// The diagonal tile is read below and on its diagonal only and mirrored: the column walk takes r >= c, the row walk r > c,
// and both land in part[ti][ti * 128 + .].  So slot k of column j holds the contribution of the rows of block k, every
// (k, block) slot is written by exactly one workgroup on every call, and the finisher adds the slots in increasing k: no
// atomics, the same bits on every call.  Rows and columns >= M (the padding of C and W) are never added.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void colsq_sym_kernel(const double* __restrict__ C, int64_t ld, int64_t M, int64_t mp,
                                                        const double* __restrict__ wts, double* __restrict__ part) {
    __shared__ double wr[128], wc[128];
    __shared__ double cred[16][128 + 1], rred[16][128 + 1];
    int ti, tj;
    {
        // lower tile from the linear index (exact in double up to 2^26 tiles)
        const int q = blockIdx.x;
        ti = (int)((sqrt(8.0 * (double)q + 1.0) - 1.0) * 0.5);
        while ((int64_t)ti * (ti + 1) / 2 > q) --ti;
        while ((int64_t)(ti + 1) * (ti + 2) / 2 <= q) ++ti;
        tj = q - (int)((int64_t)ti * (ti + 1) / 2);
    }
    const int tid = threadIdx.x, ty = tid >> 4, tx = tid & 15;
    const int64_t r0 = (int64_t)ti * 128, c0 = (int64_t)tj * 128;
    {
        const int loc = tid & 127;
        const int64_t g = (tid < 128 ? r0 : c0) + loc;
        const double v = g < M ? (wts ? wts[g] : 1.0) : 0.0;
        (tid < 128 ? wr : wc)[loc] = v;
    }
    __syncthreads();
    const bool diag = ti == tj;
    const bool interior = r0 + 128 <= M && !diag;       // (c0 <= r0)
    double cs[8], rs[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) cs[k] = rs[k] = 0.0;
    const double* base = C + r0 * ld + c0 + 2 * tx;
#pragma unroll
    for (int rr = 0; rr < 8; ++rr) {
        const int r = ty + 16 * rr;
        const double wrow = wr[r];
#pragma unroll
        for (int cc = 0; cc < 4; ++cc) {
            if (diag && 16 * rr + 15 < 32 * cc) continue;               // wholly above the diagonal (the whole workgroup)
            const d2 v = *reinterpret_cast<const d2*>(base + (int64_t)r * ld + 32 * cc);
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                const int c = 2 * tx + 32 * cc + e;
                double x = v[e];
                bool col_on = true, row_on = true;
                if (!interior) {
                    if (r0 + r >= M || c0 + c >= M) x = 0.0;            // padding: never added, whatever it holds
                    if (diag) { col_on = r >= c; row_on = r > c; }
                }
                const double x2 = x * x;
                if (col_on) cs[2 * cc + e] = fma(wrow, x2, cs[2 * cc + e]);
                if (row_on) rs[rr] = fma(wc[c], x2, rs[rr]);
            }
        }
    }
#pragma unroll
    for (int cc = 0; cc < 4; ++cc) {
        cred[ty][2 * tx + 32 * cc] = cs[2 * cc];
        cred[ty][2 * tx + 32 * cc + 1] = cs[2 * cc + 1];
    }
#pragma unroll
    for (int rr = 0; rr < 8; ++rr) rred[tx][ty + 16 * rr] = rs[rr];
    __syncthreads();
    // threads 0 .. 127: column c of the tile; 128 .. 255: row r.  Sixteen partial sums each, in their order.
    const int loc = tid & 127;
    double s;
    if (tid < 128) {
        s = cred[0][loc];
#pragma unroll
        for (int k = 1; k < 16; ++k) s += cred[k][loc];
    } else {
        s = rred[0][loc];
#pragma unroll
        for (int k = 1; k < 16; ++k) s += rred[k][loc];
    }
    if (diag) {
        // column walk and mirrored row walk of the same block: one slot
        __syncthreads();
        if (tid >= 128) rred[0][loc] = s;
        __syncthreads();
        if (tid < 128) part[(int64_t)ti * mp + r0 + loc] = s + rred[0][loc];
    } else if (tid < 128) {
        part[(int64_t)ti * mp + c0 + loc] = s;
    } else {
        part[(int64_t)tj * mp + r0 + loc] = s;
    }
}

// s_j = the nt slots of column j in increasing order; acq = s_j / (max(C_jj, 0) + noise + jitter) (times the mask),
// sd = sqrt(max(C_jj, 0) + noise): predict's convention, the jitter is not part of the reported variance
__global__ __launch_bounds__(256) void ivr_finish_kernel(const double* __restrict__ part, int nt, int64_t mp,
                                                         const double* __restrict__ C, int64_t ld, int64_t M,
                                                         const ThetaDev* __restrict__ th, const double* __restrict__ mask,
                                                         double* __restrict__ sd_out, double* __restrict__ acq_out) {
    const double noise = th->noise, dadd = th->diag_add;
    for (int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x; j < M; j += (int64_t)gridDim.x * 256) {
        double s = part[j];
        for (int k = 1; k < nt; ++k) s += part[(int64_t)k * mp + j];
        const double cjj = clamp0_nan(C[j * ld + j]);
        double a = s / (cjj + dadd);
        if (mask) a = mask[j] * a;
        acq_out[j] = a;
        if (sd_out) sd_out[j] = sqrt(cjj + noise);
    }
}

// the lower tiles of an nt x nt block matrix in 8 x 8 patches (operand panels of the TN product shared in L2), every tile
// with the k-range the launch fixes (kfix0 / kfix1)
static int ivr_tiles_ensure(gpimhip_ctx* h, IvrWs* w, int nt) {
    if (w->nt == nt) return GPIMHIP_OK;
    std::vector<TileDesc> tl;
    tl.reserve((size_t)nt * (nt + 1) / 2);
    for (int ig = 0; ig <= (nt - 1) / 8; ++ig)
        for (int jg = 0; jg <= ig; ++jg)
            for (int i = ig * 8; i < std::min(nt, ig * 8 + 8); ++i)
                for (int j = jg * 8; j < std::min(nt, jg * 8 + 8); ++j)
                    if (j <= i) tl.push_back({i, j, 0, 0});
    w->nt = 0;
    GP_TRY(w->tiles.grow(h, (int64_t)tl.size()));
    HIP_TRY(hipMemcpyAsync(w->tiles, tl.data(), tl.size() * sizeof(TileDesc), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    w->nt = nt;
    return GPIMHIP_OK;
}

static int ivr_impl(gpimhip_ctx* h, const gpimhip_model_t* m, const double* X, const double* y, int64_t N, const double* u,
                    const double* Xs, int64_t M, const double* weights, const double* mask, double* mean_out, double* sd_out,
                    double* acq_out) {
    HIP_TRY(hipSetDevice(h->device));
    IvrWs* w = iws(h);
    const int64_t npn = pad_to(N, NB), mp = pad_to(M, NB), ldm = mp + 16;       // (no power-of-two row stride)
    const int nt = (int)(mp / NB);
    // the entry's own buffers first: the model's state is not enqueued when they do not fit
    GP_TRY(w->W.grow(h, npn * ldm));
    GP_TRY(w->C.grow(h, mp * ldm));
    GP_TRY(w->part.grow(h, (int64_t)nt * mp));
    GP_TRY(ivr_tiles_ensure(h, w, nt));
    GP_TRY(model_state_at_u(h, m, X, 0, y, N, 1, u));
    const int64_t np = h->np;
    const int nb = (int)(np / NB);
    if (np != npn) {                            // (W was sized for the padded order the workspace is expected to have)
        gpim_set_error("gpimhip_ivr_exact: the workspace's padded order is not pad(N, 128)");
        return GPIMHIP_E_BADARG;
    }
    // W = L^-1 K* chunk by chunk of the K* slab, and the mean K*^T alpha (predict_cols' launches, EPI_STORE for EPI_COLSUMSQ)
    const int64_t mc = predict_chunk_cols(np, 1, M);
    GP_TRY(ws_ensure_predict(h, np, mc));
    for (int64_t m0 = 0; m0 < M; m0 += mc) {
        const int64_t cnt = std::min(mc, M - m0), cpad = pad_to(cnt, NB);
        const int64_t mcap = h->ks_cols, kld = mcap + 16;                       // buffer strides follow the capacity
        GP_TRY(launch_kmat(h, m, X, N, Xs + m0 * m->dim, cnt, h->theta, 0.0, 0, h->Ks, kld, np, cpad, 0, 0, 0, 0, np * kld));
        if (mean_out) {
            GP_TRY(launch_gemv_t(h, h->Ks, kld, np, cpad, h->alpha, h->mean_tmp, 0, np * kld, np, mcap));
            GP_TRY(launch_copy_slice(h, h->mean_tmp, mean_out + m0, cnt, mcap, M));
        }
        GP_TRY(ws_ensure_predict(h, np, cpad));                                 // (the tile list of this chunk's column blocks)
        GemmArgs g = gemm_args(h->A, h->ld, h->Ks, kld, w->W, ldm, 1.0, 0.0, h->pred_tiles, (int)h->pred_ntiles, np);
        g.c_coff = (int)(m0 / NB);
        g.chunk = deal_chunk(g.ntiles);
        g.rag = rag_of(N, np);
        { StageTimer t(h, 3); GP_TRY(launch_gemm(h, false, true, EPI_STORE, g)); }
    }
    // rows >= N of W: the identity padding of L^-1 gives zeros, but a ragged launch skips the rows >= 64 of the last block
    // row (GemmArgs::rag) and W may hold what an earlier call left there
    if (np > N) HIP_TRY(hipMemsetAsync(w->W + N * ldm, 0, (size_t)((np - N) * ldm) * sizeof(double), h->stream));
    // lower tiles of K(G, G), then C -= W^T W on them (TN; the product is not done for the upper half)
    GP_TRY(launch_kmat(h, m, Xs, M, nullptr, M, h->theta, 0.0, 0, w->C, ldm, mp, mp, 1, 1, 0, 0, 0));
    {
        GemmArgs g = gemm_args(w->W, ldm, w->W, ldm, w->C, ldm, -1.0, 1.0, w->tiles, nt * (nt + 1) / 2, 0);
        g.kfix0 = 0;
        g.kfix1 = nb;
        g.chunk = deal_chunk(g.ntiles);
        GP_TRY(launch_gemm(h, true, true, EPI_STORE, g));
    }
    hipLaunchKernelGGL(colsq_sym_kernel, dim3((unsigned)(nt * (nt + 1) / 2)), dim3(256), 0, h->stream, (const double*)w->C, ldm,
                       M, mp, weights, (double*)w->part);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(ivr_finish_kernel, dim3((unsigned)std::min<int64_t>((M + 255) / 256, 1024)), dim3(256), 0, h->stream,
                       (const double*)w->part, nt, mp, (const double*)w->C, ldm, M, (const ThetaDev*)h->theta, mask, sd_out,
                       acq_out);
    HIP_TRY(hipGetLastError());
    return finish_and_check(h);
}

extern "C" int gpimhip_ivr_exact(gpimhip_handle h, const gpimhip_model_t* m, const double* X, const double* y, int64_t N,
                                 const double* u, const double* Xs, int64_t M, const double* weights, const double* mask,
                                 double* mean_out, double* sd_out, double* acq_out) {
    if (!h || !X || !y || !u || !Xs || !acq_out || N < 1 || M < 1) {
        gpim_set_error("gpimhip_ivr_exact: null argument, N < 1 or M < 1");
        return GPIMHIP_E_BADARG;
    }
    GP_TRY(check_model(m));
    if (h->fp32) {
        gpim_set_error("gpimhip_ivr_exact: C = K** - W^T W cancels to the posterior variance; needs a double-precision handle "
                       "(gpimhip_set_precision(h, 64))");
        return GPIMHIP_E_BADARG;
    }
    if (h->refl.mask || border_on(h)) {
        gpim_set_error("gpimhip_ivr_exact: not available in reflection, border or shard mode (the cross-covariance of arbitrary "
                       "grid points is not block-structured; the dense double-precision engine only)");
        return GPIMHIP_E_BADARG;
    }
    if (M > ((int64_t)1 << 20)) {
        gpim_set_error("gpimhip_ivr_exact: M > 2^20 (C is M x M doubles)");
        return GPIMHIP_E_BADARG;
    }
    return ivr_impl(h, m, X, y, N, u, Xs, M, weights, mask, mean_out, sd_out, acq_out);
}
