// ivr.hip -- integrated variance reduction (ALC) of the exact GP: gpimhip_ivr_exact, its greedy
// batch, gpimhip_ivr_greedy (section 27), and both without the M x M covariance, gpimhip_ivr_*_banded (section 30).
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
//
// The greedy batch conditions C on each pick p: C <- C - g g^T with g = C[:, p] / sqrt(max(C_pp, 0) + noise + jitter) -- a
// GP's variance does not depend on the measured value -- and takes the next map from the new C.  Per round:
//   ivr_pick_kernel      arg-max of the round's map (NaN never, ties to the larger index), the pick leaves the live vector
//   ivr_gather_kernel    g from lower-stored C, a launch of its own: the pass rewrites the entries it reads
//   colsq_sym_kernel<true>   the downdate fused into the squared column sums: every stored entry read once, written once
//   ivr_finish_kernel    with the live vector as its mask
// All rounds are enqueued up front: the pick travels through device memory, no grid depends on it.
//
// The banded entries, gpimhip_ivr_exact_banded and gpimhip_ivr_greedy_banded (section 30), never hold C: it is built,
// summed by colsq_sym_kernel<false, true> and thrown away one band of block columns at a time (ivr_band_pass), the slots
// of the partial sums being filled by the same tiles in the same order.  Their greedy batch conditions by appending
// g^(r) to W as one more row (C^(r+1) = K(G, G) - W_aug^T W_aug: every s_j stays a sum of squares), so a further pick
// costs a whole M^2 N product where the stored batch pays one M^2 pass: the price of the memory.
#include <algorithm>
#include <type_traits>
#include "common.hpp"
#include "border.hpp"
#include "kfun.hpp"
#include "ivr.hpp"

typedef double d2 __attribute__((ext_vector_type(2)));

IvrWs* ivr_ws(gpimhip_ctx* h) {
    if (!h->ivr) h->ivr = new IvrWs();
    return (IvrWs*)h->ivr;
}
void ivr_release(gpimhip_ctx* h) {
    IvrWs* w = (IvrWs*)h->ivr;
    if (!w) return;
    dev_release(h, w->W, w->C, w->part, w->tiles, w->g, w->live, w->row, w->bpart, w->v, w->gs, w->inc, w->band, w->btiles);
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
// DOWNDATE: the entry becomes fma(-g_r, g_c, C(r, c)) before it is squared and is stored back where it was loaded from
// (gvec: mp doubles, zero at rows >= M, so the identity padding of C survives).  Each stored entry belongs to one thread of
// one workgroup: no race.  Of the diagonal tile the 32-column groups wholly above the diagonal stay unread and unwritten;
// the entries above the diagonal inside the other groups are downdated with the rest and, as before, never added.
// ------------------------------------------------------------------------------------------
// BAND (the banded pass): C is the band buffer of one band of block columns starting at column
// band.col0 -- entry (r, c) of the matrix lies at C[r * ld + c - col0], rows >= col0 -- and workgroup q takes tile
// band.tiles[q] (ci >= cj, cj inside the band: the list of the TN launch that made the tiles).  A tile owns the same slots
// of part as in the stored pass and adds in the same order, so a slot holds the same bits whatever the band width.  The
// workgroup of a diagonal tile also saves C_jj of its 128 columns to band.diag[j * ld]: the first padding column of row j
// of the band buffer, which nothing else writes, so the diagonal outlives its band.
struct ColsqBand {
    const TileDesc* tiles;
    int64_t col0;
    double* diag;
};
template <bool DOWNDATE, bool BAND = false>
__global__ __launch_bounds__(256) void colsq_sym_kernel(std::conditional_t<DOWNDATE, double*, const double*> __restrict__ C,
                                                        int64_t ld, int64_t M, int64_t mp, const double* __restrict__ wts,
                                                        double* __restrict__ part, const double* __restrict__ gvec,
                                                        std::conditional_t<BAND, ColsqBand, std::false_type> band = {}) {
    static_assert(!(BAND && DOWNDATE), "a band is thrown away after its pass: there is nothing to downdate");
    __shared__ double wr[128], wc[128];
    __shared__ double gr[DOWNDATE ? 128 : 1], gc[DOWNDATE ? 128 : 1];   // (not allocated where they are not used)
    __shared__ double cred[16][128 + 1], rred[16][128 + 1];
    int ti, tj;
    if constexpr (BAND) {
        const TileDesc t = band.tiles[blockIdx.x];
        ti = t.ci;
        tj = t.cj;
        C -= band.col0;
    } else {
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
        if constexpr (DOWNDATE) (tid < 128 ? gr : gc)[loc] = gvec[g];   // (g < mp: the tile lies inside the padded order)
    }
    __syncthreads();
    const bool diag = ti == tj;
    const bool interior = r0 + 128 <= M && !diag;       // (c0 <= r0)
    double cs[8], rs[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) cs[k] = rs[k] = 0.0;
    const auto base = C + r0 * ld + c0 + 2 * tx;
#pragma unroll
    for (int rr = 0; rr < 8; ++rr) {
        const int r = ty + 16 * rr;
        const double wrow = wr[r];
#pragma unroll
        for (int cc = 0; cc < 4; ++cc) {
            if (diag && 16 * rr + 15 < 32 * cc) continue;               // wholly above the diagonal (the whole workgroup)
            d2 v = *reinterpret_cast<const d2*>(base + (int64_t)r * ld + 32 * cc);
            if constexpr (DOWNDATE) {
                // the 16-byte store that matches the load; g = 0 on the padding, which so keeps what it holds
                const double mg = -gr[r];
                v[0] = fma(mg, gc[2 * tx + 32 * cc], v[0]);
                v[1] = fma(mg, gc[2 * tx + 32 * cc + 1], v[1]);
                *reinterpret_cast<d2*>(base + (int64_t)r * ld + 32 * cc) = v;
            }
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
    if constexpr (BAND) {
        // (r0 + loc < mp: the tile lies inside the padded order)
        if (diag && tid < 128) band.diag[(r0 + loc) * ld] = C[(r0 + loc) * ld + r0 + loc];
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

// ------------------------------------------------------------------------------------------
// The greedy batch's three small kernels (gpimhip_ivr_greedy).
// ------------------------------------------------------------------------------------------
// live[j] = the user's mask, or 1
__global__ __launch_bounds__(256) void ivr_live_init_kernel(const double* __restrict__ mask, int64_t M, double* __restrict__ live) {
    for (int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x; j < M; j += (int64_t)gridDim.x * 256) live[j] = mask ? mask[j] : 1.0;
}

// Pick r: the largest entry of the round's map that is not NaN, ties to the larger flat index (gpimhip_topk's order).  One
// workgroup; every thread scans its strided share in increasing index, the 1024 candidates are merged by the same rule, so the
// result does not depend on the merge order.  idx_out[r] = the pick or -1, gain_out[r] = its value or NaN; a pick leaves the
// live vector and sets count = r + 1 (round 0 always writes the count).  The later launches read the pick from idx_out[r].
__global__ __launch_bounds__(1024) void ivr_pick_kernel(const double* __restrict__ map, int64_t M, int r, double* __restrict__ live,
                                                        int64_t* __restrict__ idx_out, double* __restrict__ gain_out,
                                                        int64_t* __restrict__ count_out) {
    __shared__ double bv[1024];
    __shared__ int64_t bi[1024];
    const int tid = threadIdx.x;
    double v = 0.0;
    int64_t at = -1;
    for (int64_t j = tid; j < M; j += 1024) {
        const double a = map[j];
        if (a == a && (at < 0 || a >= v)) { v = a; at = j; }
    }
    bv[tid] = v;
    bi[tid] = at;
    __syncthreads();
    for (int s = 512; s > 0; s >>= 1) {
        if (tid < s) {
            const double v2 = bv[tid + s];
            const int64_t i2 = bi[tid + s], i1 = bi[tid];
            if (i2 >= 0 && (i1 < 0 || v2 > bv[tid] || (v2 == bv[tid] && i2 > i1))) { bv[tid] = v2; bi[tid] = i2; }
        }
        __syncthreads();
    }
    if (tid == 0) {
        const int64_t p = bi[0];
        idx_out[r] = p;
        gain_out[r] = p >= 0 ? bv[0] : __builtin_nan("");
        if (p >= 0) {
            live[p] = __builtin_nan("");
            *count_out = r + 1;
        } else if (r == 0) {
            *count_out = 0;
        }
    }
}

int launch_ivr_live_init(gpimhip_ctx* h, const double* mask, int64_t M, double* live) {
    hipLaunchKernelGGL(ivr_live_init_kernel, ivr_grid(M), dim3(256), 0, h->stream, mask, M, live);
    HIP_TRY(hipGetLastError());
    return GPIMHIP_OK;
}
int launch_ivr_pick(gpimhip_ctx* h, const double* map, int64_t M, int r, double* live, int64_t* idx_out, double* val_out,
                    int64_t* count_out) {
    hipLaunchKernelGGL(ivr_pick_kernel, dim3(1), dim3(1024), 0, h->stream, map, M, r, live, idx_out, val_out, count_out);
    HIP_TRY(hipGetLastError());
    return GPIMHIP_OK;
}

// g_m = C_mp / sqrt(max(C_pp, 0) + noise + jitter) for m < M from lower-stored C (C[m][p] for m >= p, C[p][m] for m < p),
// 0 for M <= m < mp and everywhere when there was no pick (p < 0: the pass then leaves C as it is)
__global__ __launch_bounds__(256) void ivr_gather_kernel(const double* __restrict__ C, int64_t ld, int64_t M, int64_t mp,
                                                         const ThetaDev* __restrict__ th, const int64_t* __restrict__ pick,
                                                         double* __restrict__ g) {
    const int64_t p = *pick;
    const bool on = p >= 0 && p < M;
    const double den = on ? sqrt(clamp0_nan(C[p * ld + p]) + th->diag_add) : 1.0;
    for (int64_t m = (int64_t)blockIdx.x * 256 + threadIdx.x; m < mp; m += (int64_t)gridDim.x * 256)
        g[m] = on && m < M ? (m >= p ? C[m * ld + p] : C[p * ld + m]) / den : 0.0;
}

// after the last pick no pass is needed: sd_after_j = sqrt(max(C_jj - g_j^2, 0) + noise), the diagonal the pass would store
__global__ __launch_bounds__(256) void ivr_sd_after_kernel(const double* __restrict__ C, int64_t ld, int64_t M,
                                                           const ThetaDev* __restrict__ th, const double* __restrict__ g,
                                                           double* __restrict__ sd_after) {
    const double noise = th->noise;
    for (int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x; j < M; j += (int64_t)gridDim.x * 256)
        sd_after[j] = sqrt(clamp0_nan(fma(-g[j], g[j], C[j * ld + j])) + noise);
}

// The banded batch keeps no C to gather from: the conditioned column of pick p is c = k(G, g_p) - W_aug^T W_aug[:, p]
// (section 28's identity over the rows of W and the g rows behind them; part: launch_believer_col's nR chunks, added in
// increasing order), and g = c / sqrt(max(c_p, 0) + noise + jitter) becomes the next row of W_aug: out[m], m < mp, zero at
// m >= M and everywhere when there was no pick.  c_p is computed by thread 0 of every workgroup with the code of every
// other entry.
template <int KIND>
__global__ __launch_bounds__(256) void ivr_gcol_kernel(const double* __restrict__ part, int nR, int64_t mp, int64_t M,
                                                       const double* __restrict__ Xs, int d, const ThetaDev* __restrict__ th,
                                                       const int64_t* __restrict__ pick, double* __restrict__ out) {
    __shared__ double sh_cp;
    const ThetaDev t = *th;
    int64_t p = *pick;
    const bool on = p >= 0 && p < M;
    if (!on) p = 0;                                     // (addresses stay inside; nothing read through them is used)
    double xp[GPIMHIP_MAX_DIM], pn;
    bel_point(Xs, p, d, t, xp, pn);
    auto column = [&](int64_t j) {
        double xj[GPIMHIP_MAX_DIM], jn;
        bel_point(Xs, j, d, t, xj, jn);
        double dot = xj[0] * xp[0];
#pragma unroll
        for (int k = 1; k < GPIMHIP_MAX_DIM; ++k) dot = fma(xj[k], xp[k], dot);
        const double r2 = clamp0_nan((jn - 2.0 * dot) + pn);
        double s = part[j];
        for (int k = 1; k < nR; ++k) s += part[(int64_t)k * mp + j];
        return t.var * kfun_value<KIND>(r2, t.alpha) - s;
    };
    if (threadIdx.x == 0) sh_cp = on ? column(p) : 0.0;
    __syncthreads();
    const double den = sqrt(clamp0_nan(sh_cp) + t.diag_add);
    for (int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x; j < mp; j += (int64_t)gridDim.x * 256)
        out[j] = on && j < M ? column(j) / den : 0.0;
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

// the same tiles band by band of bw block columns (band b: block columns [b bw, min(nt, (b + 1) bw)), block rows from its
// first column down), 8 x 8 patches inside a band
static int ivr_band_tiles_ensure(gpimhip_ctx* h, IvrWs* w, int nt, int bw) {
    if (w->bnt == nt && w->bbw == bw) return GPIMHIP_OK;
    std::vector<TileDesc> tl;
    std::vector<int> off;
    tl.reserve((size_t)nt * (nt + 1) / 2);
    for (int c0 = 0; c0 < nt; c0 += bw) {
        const int c1 = std::min(nt, c0 + bw);
        off.push_back((int)tl.size());
        for (int i8 = c0; i8 < nt; i8 += 8)
            for (int j8 = c0; j8 < c1; j8 += 8)
                for (int i = i8; i < std::min(nt, i8 + 8); ++i)
                    for (int j = j8; j < std::min(c1, j8 + 8); ++j)
                        if (j <= i) tl.push_back({i, j, 0, 0});
    }
    off.push_back((int)tl.size());
    w->bnt = 0;
    GP_TRY(w->btiles.grow(h, (int64_t)tl.size()));
    HIP_TRY(hipMemcpyAsync(w->btiles, tl.data(), tl.size() * sizeof(TileDesc), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    w->boff.swap(off);
    w->bnt = nt;
    w->bbw = bw;
    return GPIMHIP_OK;
}

// W = L^-1 K* chunk by chunk of the K* slab, and the mean K*^T alpha (predict_cols' launches, EPI_STORE for EPI_COLSUMSQ)
int ivr_build_w(gpimhip_ctx* h, const gpimhip_model_t* m, const double* X, int64_t N, const double* Xs, int64_t M, double* W,
                int64_t ldm, double* mean_out) {
    const int64_t np = h->np;
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
        GemmArgs g = gemm_args(h->A, h->ld, h->Ks, kld, W, ldm, 1.0, 0.0, h->pred_tiles, (int)h->pred_ntiles, np);
        g.c_coff = (int)(m0 / NB);
        g.chunk = deal_chunk(g.ntiles);
        g.rag = rag_of(N, np);
        { StageTimer t(h, 3); GP_TRY(launch_gemm(h, false, true, EPI_STORE, g)); }
    }
    // rows >= N of W: the identity padding of L^-1 gives zeros, but a ragged launch skips the rows >= 64 of the last block
    // row (GemmArgs::rag) and W may hold what an earlier call left there
    if (np > N) HIP_TRY(hipMemsetAsync(W + N * ldm, 0, (size_t)((np - N) * ldm) * sizeof(double), h->stream));
    return GPIMHIP_OK;
}

// what gpimhip_ivr_greedy adds to the map of round 0 (q picks; the outputs of the entry, device pointers)
struct IvrGreedy {
    int32_t q;
    double *maps, *sd_after, *gain;
    int64_t *idx, *count;
};

// One banded pass (section 30): for each band of bw block columns the band's tiles of K(G, G), minus W_aug^T W_aug over the
// first kb k-blocks of W on exactly the band's lower tiles, the squared sums into the slots those tiles own, the diagonal
// into the padding column.  The band buffer is overwritten by the next band: one stream, so every launch has finished
// with it before.  Tiles strictly above the diagonal inside a band are built and never read.
static int ivr_band_pass(gpimhip_ctx* h, IvrWs* w, const gpimhip_model_t* m, const double* Xs, int64_t M, int64_t ldm, int bw,
                         int kb, const double* weights) {
    const int64_t mp = pad_to(M, NB), ldb = (int64_t)NB * bw + 16;
    const int nt = (int)(mp / NB);
    double* B = w->band;
    for (int b = 0, c0 = 0; c0 < nt; ++b, c0 += bw) {
        const int c1 = std::min(nt, c0 + bw), n = w->boff[b + 1] - w->boff[b];
        const int64_t col0 = (int64_t)c0 * NB, cols = (int64_t)(c1 - c0) * NB;
        const double* G0 = Xs + col0 * m->dim;
        const TileDesc* tiles = w->btiles + w->boff[b];
        // (a rectangle at an offset: kmat_kernel computes an entry from its own row and column point, so these are the
        // entries of the symmetric build.  sym = 1 -- rows and columns start at the same point, so the rectangle's diagonal
        // is the matrix's: a diagonal tile then takes the kernel's bounds-checked loop as in the stored build, not the
        // interior one, whose schedule of the same arithmetic rounds a few entries differently, and the padding is C's)
        GP_TRY(launch_kmat(h, m, G0, M - col0, G0, std::min(cols, M - col0), h->theta, 0.0, 0, B + col0 * ldb, ldb, mp - col0,
                           cols, 1, 0, 0, 0, 0));
        GemmArgs g = gemm_args(w->W, ldm, w->W, ldm, B, ldb, -1.0, 1.0, tiles, n, 0);
        g.c_coff = -c0;                                 // block column cj of C is block column cj - c0 of the band buffer
        g.kfix0 = 0;
        g.kfix1 = kb;
        g.chunk = deal_chunk(g.ntiles);
        GP_TRY(launch_gemm(h, true, true, EPI_STORE, g));
        hipLaunchKernelGGL((colsq_sym_kernel<false, true>), dim3((unsigned)n), dim3(256), 0, h->stream, (const double*)B, ldb, M,
                           mp, weights, (double*)w->part, (const double*)nullptr, ColsqBand{tiles, col0, B + (int64_t)NB * bw});
        HIP_TRY(hipGetLastError());
    }
    return GPIMHIP_OK;
}

// The map of round 0 into acq_out (gpimhip_ivr_exact: greedy == nullptr, the mask multiplied in), then for a greedy batch
// the q - 1 conditioned rounds, every launch enqueued before the one synchronisation at the end.  band > 0: the banded
// entries -- C exists one band of block columns at a time, and conditioning on pick r appends g^(r) to W as row np + r
// (C^(r+1) = K(G, G) - W_aug^T W_aug), so a round is the banded pass over a k-range one block longer per 128 picks.
static int ivr_impl(gpimhip_ctx* h, const char* who, const gpimhip_model_t* m, const double* X, const double* y, int64_t N,
                    const double* u, const double* Xs, int64_t M, const double* weights, const double* mask, double* mean_out,
                    double* sd_out, double* acq_out, const IvrGreedy* greedy, int band) {
    HIP_TRY(hipSetDevice(h->device));
    IvrWs* w = ivr_ws(h);
    const int64_t npn = pad_to(N, NB), mp = pad_to(M, NB), ldm = mp + 16;       // (no power-of-two row stride)
    const int nt = (int)(mp / NB);
    const int bw = std::min(band, nt);                                          // block columns per band; 0: C is stored
    const int64_t ldb = (int64_t)NB * bw + 16;
    const int64_t gpad = bw && greedy ? pad_to(greedy->q, NB) : 0;              // the g rows behind W
    // the entry's own buffers first: the model's state is not enqueued when they do not fit
    GP_TRY(w->W.grow(h, (npn + gpad) * ldm));
    if (bw) GP_TRY(w->band.grow(h, mp * ldb));
    else GP_TRY(w->C.grow(h, mp * ldm));
    GP_TRY(w->part.grow(h, (int64_t)nt * mp));
    if (greedy) {
        if (bw) {
            // the column pass runs over np + pad(r, 128) rows in round r; the chunk count is not monotone in the rows
            int nR = 0;
            for (int64_t rows = npn; rows <= npn + gpad; rows += NB) nR = std::max(nR, gemv_tri_chunks(rows));
            GP_TRY(w->bpart.grow(h, (int64_t)nR * mp));
        } else {
            GP_TRY(w->g.grow(h, mp));
        }
        GP_TRY(w->live.grow(h, M));
        if (!greedy->maps) {
            GP_TRY(w->row.grow(h, M));
            acq_out = w->row;
        }
    }
    if (bw) GP_TRY(ivr_band_tiles_ensure(h, w, nt, bw));
    else GP_TRY(ivr_tiles_ensure(h, w, nt));
    GP_TRY(model_state_at_u(h, m, X, 0, y, N, 1, u));
    const int64_t np = h->np;
    const int nb = (int)(np / NB);
    if (np != npn) {                            // (W was sized for the padded order the workspace is expected to have)
        gpim_set_error(std::string(who) + ": the workspace's padded order is not pad(N, 128)");
        return GPIMHIP_E_BADARG;
    }
    GP_TRY(ivr_build_w(h, m, X, N, Xs, M, w->W, ldm, mean_out));
    // the g rows of this call: W is grow-only and an earlier, longer batch has left its rows behind
    if (gpad) HIP_TRY(hipMemsetAsync(w->W + np * ldm, 0, (size_t)(gpad * ldm) * sizeof(double), h->stream));
    const dim3 tiles((unsigned)(nt * (nt + 1) / 2));
    const ThetaDev* th = h->theta;
    // where the finisher finds C_jj as Cc[j * ldc + j]: in C, or in the padding column of the band buffer (row j, column
    // 128 bw: the "matrix" that starts there with rows of ldb - 1 doubles has it on its diagonal)
    const double* Cc = bw ? w->band + (int64_t)NB * bw : w->C;
    const int64_t ldc = bw ? ldb - 1 : ldm;
    if (bw) {
        GP_TRY(ivr_band_pass(h, w, m, Xs, M, ldm, bw, nb, weights));
    } else {
        // lower tiles of K(G, G), then C -= W^T W on them (TN; the product is not done for the upper half)
        GP_TRY(launch_kmat(h, m, Xs, M, nullptr, M, h->theta, 0.0, 0, w->C, ldm, mp, mp, 1, 1, 0, 0, 0));
        GemmArgs g = gemm_args(w->W, ldm, w->W, ldm, w->C, ldm, -1.0, 1.0, w->tiles, nt * (nt + 1) / 2, 0);
        g.kfix0 = 0;
        g.kfix1 = nb;
        g.chunk = deal_chunk(g.ntiles);
        GP_TRY(launch_gemm(h, true, true, EPI_STORE, g));
        hipLaunchKernelGGL(colsq_sym_kernel<false>, tiles, dim3(256), 0, h->stream, Cc, ldm, M, mp, weights, (double*)w->part,
                           (const double*)nullptr);
        HIP_TRY(hipGetLastError());
    }
    if (greedy) {
        // the live vector stands in for the mask from round 0 on: 1 * a is a
        GP_TRY(launch_ivr_live_init(h, mask, M, w->live));
        mask = w->live;
    }
    hipLaunchKernelGGL(ivr_finish_kernel, ivr_grid(M), dim3(256), 0, h->stream, (const double*)w->part, nt, mp, Cc, ldc, M, th,
                       mask, sd_out, acq_out);
    HIP_TRY(hipGetLastError());
    // banded: g^(r) of pick r from W_aug (its rows np .. np + r - 1 hold the picks before) into row np + r
    auto append_g = [&](int r) -> int {
        const int64_t rows = np + pad_to(r, NB);
        GP_TRY(launch_believer_col(h, w->W, ldm, rows, M, mp, greedy->idx + r, w->bpart));
        return with_kind(m->kernel, [&](auto K) {
            hipLaunchKernelGGL(ivr_gcol_kernel<decltype(K)::value>, ivr_grid(mp), dim3(256), 0, h->stream,
                               (const double*)w->bpart, gemv_tri_chunks(rows), mp, M, Xs, (int)m->dim, th,
                               (const int64_t*)(greedy->idx + r), w->W + (np + r) * ldm);
            HIP_TRY(hipGetLastError());
            return GPIMHIP_OK;
        });
    };
    for (int r = 0; greedy && r < greedy->q; ++r) {
        double* map = greedy->maps ? greedy->maps + (int64_t)r * M : (double*)w->row;       // (round 0: acq_out)
        if (r > 0) {
            if (bw) {
                GP_TRY(append_g(r - 1));
                GP_TRY(ivr_band_pass(h, w, m, Xs, M, ldm, bw, nb + (int)(pad_to(r, NB) / NB), weights));
            } else {
                // the column of pick r - 1 before the pass that rewrites it, the downdate fused into the sums
                hipLaunchKernelGGL(ivr_gather_kernel, ivr_grid(mp), dim3(256), 0, h->stream, Cc, ldm, M, mp, th,
                                   (const int64_t*)(greedy->idx + r - 1), (double*)w->g);
                HIP_TRY(hipGetLastError());
                hipLaunchKernelGGL(colsq_sym_kernel<true>, tiles, dim3(256), 0, h->stream, (double*)w->C, ldm, M, mp, weights,
                                   (double*)w->part, (const double*)w->g);
                HIP_TRY(hipGetLastError());
            }
            // the new map
            hipLaunchKernelGGL(ivr_finish_kernel, ivr_grid(M), dim3(256), 0, h->stream, (const double*)w->part, nt, mp, Cc, ldc,
                               M, th, mask, (double*)nullptr, map);
            HIP_TRY(hipGetLastError());
        }
        GP_TRY(launch_ivr_pick(h, map, M, r, w->live, greedy->idx, greedy->gain, greedy->count));
    }
    if (greedy && greedy->sd_after) {
        // no pass after the last pick: the diagonal of the last pass and the last g
        const double* glast = bw ? w->W + (np + greedy->q - 1) * ldm : w->g;
        if (bw) {
            GP_TRY(append_g(greedy->q - 1));
        } else {
            hipLaunchKernelGGL(ivr_gather_kernel, ivr_grid(mp), dim3(256), 0, h->stream, Cc, ldm, M, mp, th,
                               (const int64_t*)(greedy->idx + greedy->q - 1), (double*)w->g);
            HIP_TRY(hipGetLastError());
        }
        hipLaunchKernelGGL(ivr_sd_after_kernel, ivr_grid(M), dim3(256), 0, h->stream, Cc, ldc, M, th, glast, greedy->sd_after);
        HIP_TRY(hipGetLastError());
    }
    return finish_and_check(h);
}

// what both entries refuse, with the reason
int ivr_check(gpimhip_ctx* h, const char* who, const gpimhip_model_t* m, bool pointers, int64_t N, int64_t M,
              const char* why_m) {
    if (!h || !pointers || N < 1 || M < 1) {
        gpim_set_error(std::string(who) + ": null argument, N < 1 or M < 1");
        return GPIMHIP_E_BADARG;
    }
    GP_TRY(check_model(m));
    if (h->fp32) {
        gpim_set_error(std::string(who) + ": C = K** - W^T W cancels to the posterior variance; needs a double-precision handle "
                       "(gpimhip_set_precision(h, 64))");
        return GPIMHIP_E_BADARG;
    }
    if (h->refl.mask || border_on(h)) {
        gpim_set_error(std::string(who) + ": not available in reflection, border or shard mode (the cross-covariance of "
                       "arbitrary grid points is not block-structured; the dense double-precision engine only)");
        return GPIMHIP_E_BADARG;
    }
    if (M > ((int64_t)1 << 20)) {
        gpim_set_error(std::string(who) + ": M > 2^20 (" + why_m + ")");
        return GPIMHIP_E_BADARG;
    }
    return GPIMHIP_OK;
}

// the two exact entries (band == 0: C is stored) and the two greedy ones: the checks, then ivr_impl
static const char* const IVR_WHY_PART = "the partial sums are M^2 / 128 doubles";
static int ivr_band_check(const char* who, int32_t band) {
    if (band >= 1) return GPIMHIP_OK;
    gpim_set_error(std::string(who) + ": band = " + std::to_string(band) + " block columns per band (band >= 1)");
    return GPIMHIP_E_BADARG;
}

extern "C" int gpimhip_ivr_exact(gpimhip_handle h, const gpimhip_model_t* m, const double* X, const double* y, int64_t N,
                                 const double* u, const double* Xs, int64_t M, const double* weights, const double* mask,
                                 double* mean_out, double* sd_out, double* acq_out) {
    GP_TRY(ivr_check(h, "gpimhip_ivr_exact", m, X && y && u && Xs && acq_out, N, M));
    return ivr_impl(h, "gpimhip_ivr_exact", m, X, y, N, u, Xs, M, weights, mask, mean_out, sd_out, acq_out, nullptr, 0);
}

extern "C" int gpimhip_ivr_exact_banded(gpimhip_handle h, const gpimhip_model_t* m, const double* X, const double* y, int64_t N,
                                        const double* u, const double* Xs, int64_t M, int32_t band, const double* weights,
                                        const double* mask, double* mean_out, double* sd_out, double* acq_out) {
    const char* who = "gpimhip_ivr_exact_banded";
    GP_TRY(ivr_check(h, who, m, X && y && u && Xs && acq_out, N, M, IVR_WHY_PART));
    GP_TRY(ivr_band_check(who, band));
    return ivr_impl(h, who, m, X, y, N, u, Xs, M, weights, mask, mean_out, sd_out, acq_out, nullptr, band);
}

static int ivr_greedy_entry(gpimhip_ctx* h, const char* who, const gpimhip_model_t* m, const double* X, const double* y,
                            int64_t N, const double* u, const double* Xs, int64_t M, int32_t band, const double* weights,
                            const double* mask, int32_t q, double* mean_out, double* sd_out, double* maps_out,
                            double* sd_after_out, int64_t* idx_out, double* gain_out, int64_t* count_out) {
    if (q < 1 || q > M) {
        gpim_set_error(std::string(who) + ": q = " + std::to_string(q) + " picks of M = " + std::to_string(M) +
                       " candidates (1 <= q <= M)");
        return GPIMHIP_E_BADARG;
    }
    if (!idx_out || !gain_out || !count_out) {
        gpim_set_error(std::string(who) + ": idx_out, gain_out and count_out are not optional");
        return GPIMHIP_E_BADARG;
    }
    const IvrGreedy greedy = {q, maps_out, sd_after_out, gain_out, idx_out, count_out};
    return ivr_impl(h, who, m, X, y, N, u, Xs, M, weights, mask, mean_out, sd_out, maps_out, &greedy, band);   // (round 0: row 0)
}

extern "C" int gpimhip_ivr_greedy(gpimhip_handle h, const gpimhip_model_t* m, const double* X, const double* y, int64_t N,
                                  const double* u, const double* Xs, int64_t M, const double* weights, const double* mask,
                                  int32_t q, double* mean_out, double* sd_out, double* maps_out, double* sd_after_out,
                                  int64_t* idx_out, double* gain_out, int64_t* count_out) {
    const char* who = "gpimhip_ivr_greedy";
    GP_TRY(ivr_check(h, who, m, X && y && u && Xs, N, M));
    return ivr_greedy_entry(h, who, m, X, y, N, u, Xs, M, 0, weights, mask, q, mean_out, sd_out, maps_out, sd_after_out, idx_out,
                            gain_out, count_out);
}

extern "C" int gpimhip_ivr_greedy_banded(gpimhip_handle h, const gpimhip_model_t* m, const double* X, const double* y,
                                         int64_t N, const double* u, const double* Xs, int64_t M, int32_t band,
                                         const double* weights, const double* mask, int32_t q, double* mean_out, double* sd_out,
                                         double* maps_out, double* sd_after_out, int64_t* idx_out, double* gain_out,
                                         int64_t* count_out) {
    const char* who = "gpimhip_ivr_greedy_banded";
    GP_TRY(ivr_check(h, who, m, X && y && u && Xs, N, M, IVR_WHY_PART));
    GP_TRY(ivr_band_check(who, band));
    return ivr_greedy_entry(h, who, m, X, y, N, u, Xs, M, band, weights, mask, q, mean_out, sd_out, maps_out, sd_after_out,
                            idx_out, gain_out, count_out);
}
