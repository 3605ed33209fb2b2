// ivr.hpp -- what ivr.hip (integrated variance reduction, DESIGN.md sections 26 / 27 / 30) shares with believer.hip (believer
// batches of CB / EI / POI, section 28): the workspace both keep W = L^-1 K(X, G) in, the loop that builds W and the mean,
// the argument checks, the launchers of the live vector, of the pick and of the pass W^T W[:, p] over W, and a candidate's
// scaled coordinates.  The kernels stay in their files.
#pragma once
#include <algorithm>
#include <vector>
#include "common.hpp"

struct IvrWs {
    DevBuf<double> W;               // np x ldm: L^-1 K(X, G), rows >= N zero; the banded greedy batch: pad(q, 128) more rows,
                                    // row np + r the scaled conditioned column g^(r) of pick r, the rest zero
    DevBuf<double> C;               // mp x ldm: lower tiles of the latent posterior covariance
    DevBuf<double> part;            // (mp / 128) x mp: part[k][j] = sum over the rows m of block k of w_m C_mj^2
    DevBuf<TileDesc> tiles;         // lower tiles of an nt x nt block matrix
    DevBuf<double> g;               // mp: the scaled column of the last pick, zero at rows >= M (gpimhip_ivr_greedy)
    DevBuf<double> live;            // M: the user's mask or ones, NaN at the picks made so far
    DevBuf<double> row;             // M: a round's map when the caller does not want the maps
    int nt = 0;
    // the banded entries (section 30)
    DevBuf<double> band;            // mp x (128 * bw + 16): one band of bw block columns of C at a time; the first padding
                                    // column of row j keeps C_jj once j's band is gone
    DevBuf<TileDesc> btiles;        // the lower tiles of an bnt x bnt block matrix, band by band
    std::vector<int> boff;          // the tiles of band b: [boff[b], boff[b + 1])
    int bnt = 0, bbw = 0;
    // gpimhip_acquire_batch (believer.hip)
    DevBuf<double> bpart;           // nR x mp: part[chunk][j] = sum over the rows k of the chunk of W_kj W_kp (or W_kj^2)
    DevBuf<double> v;               // 2 x M: the latent variance, read from one half and written to the other (round parity)
    DevBuf<double> gs;              // q x mp: the scaled conditioned columns g^(s) of the picks made so far
    DevBuf<double> inc;             // q + 1: the incumbent b_r of round r in slot r (EI / POI)
};
IvrWs* ivr_ws(gpimhip_ctx* h);

// what the entries of both files refuse, with the reason: null arguments, fp32, reflection / border / shard mode, M > 2^20
// (why_m: what grows with M^2 in the entry that asks)
int ivr_check(gpimhip_ctx* h, const char* who, const gpimhip_model_t* m, bool pointers, int64_t N, int64_t M,
              const char* why_m = "C is M x M doubles");

// W = L^-1 K* (np x ldm, rows >= N zeroed) chunk by chunk of the K* slab and, with mean_out, the mean K*^T alpha, from the
// model's state in the workspace (model_state_at_u): predict_cols' launches with EPI_STORE in place of EPI_COLSUMSQ
int ivr_build_w(gpimhip_ctx* h, const gpimhip_model_t* m, const double* X, int64_t N, const double* Xs, int64_t M, double* W,
                int64_t ldm, double* mean_out);

static inline dim3 ivr_grid(int64_t n) { return dim3((unsigned)std::min<int64_t>((n + 255) / 256, 1024)); }
// live[j] = mask[j], or 1 without a mask
int launch_ivr_live_init(gpimhip_ctx* h, const double* mask, int64_t M, double* live);
// pick r of a round's map (ivr_pick_kernel): idx_out[r], val_out[r], the pick leaves the live vector, *count_out = r + 1
int launch_ivr_pick(gpimhip_ctx* h, const double* map, int64_t M, int r, double* live, int64_t* idx_out, double* val_out,
                    int64_t* count_out);
// believer_col_kernel (believer.hip) over the first `rows` rows of W (a multiple of 128): part[chunk][j] = sum over the rows k
// of the chunk of W_kj W_kp, p = *pick (zeros when there is no pick); gemv_tri_chunks(rows) chunks of mp doubles
int launch_believer_col(gpimhip_ctx* h, const double* W, int64_t ldm, int64_t rows, int64_t M, int64_t mp, const int64_t* pick,
                        double* part);

// the candidate's coordinates over the lengthscales and their squared norm (tile_stage's arithmetic, the norm in the
// order of the dot product of the callers: a point against itself gives r2 = 0 exactly)
__device__ __forceinline__ void bel_point(const double* __restrict__ Xs, int64_t j, int d, const ThetaDev& t, double* a, double& n2) {
#pragma unroll
    for (int k = 0; k < GPIMHIP_MAX_DIM; ++k) a[k] = k < d ? Xs[j * d + k] / t.ls[k] : 0.0;
    n2 = a[0] * a[0];
#pragma unroll
    for (int k = 1; k < GPIMHIP_MAX_DIM; ++k) n2 = fma(a[k], a[k], n2);
}
