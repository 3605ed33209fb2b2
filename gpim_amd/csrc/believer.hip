// believer.hip -- believer batches of the three classical acquisition functions: gpimhip_acquire_batch.
//
// A batch of q picks for CB / EI / POI by the kriging believer (Ginsbourger et al.; for CB this is GP-BUCB, Desautels et
// al.): after picking p, pretend that p was measured and gave its posterior mean.  The mean map then does not change and
// the latent variance drops by section 27's identity, of which only the diagonal and the q picked columns are needed:
// with S = K + (noise + jitter) I, W = L^-1 K(X, G) and the candidates' latent variance v_j = s2 - sum_k W_kj^2,
//     c     = k(G, g_p) - W^T W[:, p] - sum_{s < r} g^(s) g^(s)[p]       the conditioned column of pick r
//     g^(r) = c / sqrt(max(c_p, 0) + noise + jitter),   v <- v - g^(r) o g^(r)
// i.e. a pivoted partial Cholesky of the posterior covariance C taken from W alone: C is never formed, there is no M x M
// matrix and no M^2 N product, so the entry also runs where gpimhip_ivr_greedy cannot.  The next pick maximises the
// acquisition function of (mean, sqrt(max(v, 0) + noise)); for EI / POI the believed value joins the observations the
// incumbent is the maximum of.  Kernels:
//   wcolsq_kernel            part[chunk][j] = sum over the rows k of the chunk of W_kj^2, one pass over W
//   believer_init_kernel     v, sd and the map of round 0 (the partial sums added in increasing chunk order)
//   believer_col_kernel      part[chunk][j] = sum over the rows k of the chunk of W_kj W_kp, one pass over W per pick
//   believer_finish_kernel   c, g^(r), v, the next incumbent and the next map
// with ivr.hip's live vector and pick (ivr.hpp).  All rounds are enqueued up front: the pick travels through device
// memory (idx_out[r]), no grid depends on it; one synchronisation at the end.
//
// Hazards.
//   g^(s)[p], s < r, is read by every workgroup of believer_finish_kernel while row r of the same buffer is being written:
//     different rows, no overlap.
//   v: believer_finish_kernel needs v[p] in every workgroup (the sd of the believed value, POI's incumbent) and updates
//     v[j] in the thread that owns j; it therefore reads one half of a two-row buffer and writes the other (round parity),
//     so that no workgroup can see v[p] half-updated.
//   The incumbent: slot r holds b_r.  A kernel of round r reads slot r (written by an earlier launch) and workgroup 0 alone
//     writes slot r + 1; the other workgroups derive b_(r+1) themselves from what they have read.
//   No pick (p < 0, no live candidate left): believer_col_kernel writes zeros, believer_finish_kernel stores g^(r) = 0,
//     copies v and the incumbent, and the next map is NaN everywhere because the live vector is.
//   Padding columns j >= M of W are summed into part (they are zeros of the K* slab) but never read from it: the
//     finishers stop at M, the pick scans M entries.  Rows >= N of W are zero (ivr_build_w).
//   Every sum has one fixed order and there are no atomics: two calls return identical bits.
#include <algorithm>
#include "common.hpp"
#include "kfun.hpp"
#include "ivr.hpp"
#include "acq.hpp"

typedef double d2 __attribute__((ext_vector_type(2)));

#define BEL_STRIP 128       // columns of W per workgroup
#define BEL_RC_MAX 1024     // rows per workgroup at most (gemv_tri_rc): the picked column's share in LDS

// ------------------------------------------------------------------------------------------
// One pass over W (np x ldm, rows contiguous).  Workgroup (strip, chunk) = 128 columns x rc rows, four waves: wave w takes
// the column half w & 1 and the row pairs 2 (w >> 1) + {0, 1} + 4 n, so a wave instruction reads two rows x 512 contiguous
// bytes with 16-byte loads (gemv_t_tri_kernel's pattern), four in flight per lane.  SQ: sum of squares; else the product
// with the chunk's share of column p of W, gathered by the workgroup itself into LDS (rc strided loads, tiny next to the
// strip).  part[chunk][column]: the two row parities (one shuffle), then the two waves of a column half, in that order.
// np and rc are multiples of 128, so every chunk holds a multiple of 16 rows.
// ------------------------------------------------------------------------------------------
template <bool SQ>
__device__ __forceinline__ void bel_pass(const double* __restrict__ W, int64_t ldm, int64_t np, int64_t mp, int rc, int64_t p,
                                         double* __restrict__ part, double* colp, d2 (*red)[32]) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, cp = lane & 31, rp = lane >> 5;
    const int half = wave & 1, rw = wave >> 1;
    const int64_t i0 = (int64_t)blockIdx.y * rc, c0 = (int64_t)blockIdx.x * BEL_STRIP;
    const int rows = (int)(np - i0 < rc ? np - i0 : rc);
    double* out = part + (int64_t)blockIdx.y * mp + c0;
    if (!SQ) {
        if (p < 0) {                                    // no pick (the whole grid takes this branch)
            if (tid < BEL_STRIP) out[tid] = 0.0;
            return;
        }
        for (int t = tid; t < rows; t += 256) colp[t] = W[(i0 + t) * ldm + p];
        __syncthreads();
    }
    const double* col = W + i0 * ldm + c0 + 64 * half + 2 * cp;
    d2 s0 = (d2){0.0, 0.0}, s1 = s0, s2 = s0, s3 = s0;
    int i = 2 * rw + rp;                                // rows i, i + 4, i + 8, ... of the chunk
    for (; i + 12 < rows; i += 16) {
        const d2 a0 = *reinterpret_cast<const d2*>(col + (int64_t)i * ldm);
        const d2 a1 = *reinterpret_cast<const d2*>(col + (int64_t)(i + 4) * ldm);
        const d2 a2 = *reinterpret_cast<const d2*>(col + (int64_t)(i + 8) * ldm);
        const d2 a3 = *reinterpret_cast<const d2*>(col + (int64_t)(i + 12) * ldm);
        if (SQ) {
            s0[0] = fma(a0[0], a0[0], s0[0]); s0[1] = fma(a0[1], a0[1], s0[1]);
            s1[0] = fma(a1[0], a1[0], s1[0]); s1[1] = fma(a1[1], a1[1], s1[1]);
            s2[0] = fma(a2[0], a2[0], s2[0]); s2[1] = fma(a2[1], a2[1], s2[1]);
            s3[0] = fma(a3[0], a3[0], s3[0]); s3[1] = fma(a3[1], a3[1], s3[1]);
        } else {
            const double x0 = colp[i], x1 = colp[i + 4], x2 = colp[i + 8], x3 = colp[i + 12];
            s0[0] = fma(a0[0], x0, s0[0]); s0[1] = fma(a0[1], x0, s0[1]);
            s1[0] = fma(a1[0], x1, s1[0]); s1[1] = fma(a1[1], x1, s1[1]);
            s2[0] = fma(a2[0], x2, s2[0]); s2[1] = fma(a2[1], x2, s2[1]);
            s3[0] = fma(a3[0], x3, s3[0]); s3[1] = fma(a3[1], x3, s3[1]);
        }
    }
    for (; i < rows; i += 4) {
        const d2 a0 = *reinterpret_cast<const d2*>(col + (int64_t)i * ldm);
        const double x0 = SQ ? 0.0 : colp[i];
        s0[0] = fma(a0[0], SQ ? a0[0] : x0, s0[0]);
        s0[1] = fma(a0[1], SQ ? a0[1] : x0, s0[1]);
    }
    d2 v;
    v[0] = (s0[0] + s1[0]) + (s2[0] + s3[0]);
    v[1] = (s0[1] + s1[1]) + (s2[1] + s3[1]);
    v[0] += __shfl_xor(v[0], 32);                       // the two row parities (both halves end with the same sum)
    v[1] += __shfl_xor(v[1], 32);
    if (rp == 0) red[wave][cp] = v;
    __syncthreads();
    if (tid < 64) {
        const int hf = tid >> 5, c = tid & 31;
        d2 t = red[hf][c];
        t[0] += red[hf + 2][c][0];
        t[1] += red[hf + 2][c][1];
        *reinterpret_cast<d2*>(out + 64 * hf + 2 * c) = t;
    }
}

__global__ __launch_bounds__(256) void wcolsq_kernel(const double* __restrict__ W, int64_t ldm, int64_t np, int64_t mp, int rc,
                                                     double* __restrict__ part) {
    __shared__ d2 red[4][32];
    bel_pass<true>(W, ldm, np, mp, rc, 0, part, nullptr, red);
}

// (the pick of the round from device memory; p outside 0 .. M - 1 counts as no pick)
__global__ __launch_bounds__(256) void believer_col_kernel(const double* __restrict__ W, int64_t ldm, int64_t np, int64_t M,
                                                           int64_t mp, int rc, const int64_t* __restrict__ pick,
                                                           double* __restrict__ part) {
    __shared__ d2 red[4][32];
    __shared__ double colp[BEL_RC_MAX];
    int64_t p = *pick;
    if (p >= M) p = -1;
    bel_pass<false>(W, ldm, np, mp, rc, p, part, colp, red);
}

// (ivr.hpp: the same pass for the banded greedy IVR, over W and the g rows behind it)
int launch_believer_col(gpimhip_ctx* h, const double* W, int64_t ldm, int64_t rows, int64_t M, int64_t mp, const int64_t* pick,
                        double* part) {
    const dim3 pass((unsigned)(mp / BEL_STRIP), (unsigned)gemv_tri_chunks(rows));
    hipLaunchKernelGGL(believer_col_kernel, pass, dim3(256), 0, h->stream, W, ldm, rows, M, mp, gemv_tri_rc(rows), pick, part);
    HIP_TRY(hipGetLastError());
    return GPIMHIP_OK;
}

// Round 0: v_j = s2 - sum of the chunks' squared column sums in increasing chunk order (predict_var_kernel's prior variance
// and order of operations), sd = sqrt(max(v, 0) + noise), map_0 = live * acq.  inc: slot 0 of the incumbents (EI / POI).
__global__ __launch_bounds__(256) void believer_init_kernel(const double* __restrict__ part, int nR, int64_t mp, int64_t M,
                                                            const ThetaDev* __restrict__ th, int kind, double p0, double p1,
                                                            const double* __restrict__ inc, const double* __restrict__ mean,
                                                            const double* __restrict__ live, double* __restrict__ v_out,
                                                            double* __restrict__ sd_out, double* __restrict__ map0) {
    const double s2 = th->var, noise = th->noise;
    const double a = kind == GPIMHIP_ACQ_CB ? p0 : inc[0];
    for (int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x; j < M; j += (int64_t)gridDim.x * 256) {
        double s = part[j];
        for (int k = 1; k < nR; ++k) s += part[(int64_t)k * mp + j];
        const double v = s2 - s;
        v_out[j] = v;
        const double sd = sqrt(clamp0_nan(v) + noise);
        sd_out[j] = sd;
        map0[j] = live[j] * acq_value(kind, mean[j], sd, a, p1);
    }
}

struct BelFinish {
    const double* part; int nR; int64_t mp, M;          // believer_col_kernel's partial sums for pick r
    const double* Xs; int d; const ThetaDev* th;        // the candidates (M x d) and the hyper-parameters
    const int64_t* pick; int r;                         // idx_out + r
    double* gs;                                         // q x mp: rows < r read, row r written
    const double* v_in; double* v_out;                  // the two halves of the variance buffer
    const double* mean; const double* live;
    int kind; double p0, p1;
    double* inc;                                        // slot r read, slot r + 1 written by workgroup 0 (EI / POI)
    double* map_next;                                   // row r + 1 of the maps, or null after the last pick
    double* sd_after;                                   // M, or null: the sd after this (the last) pick
};

// After pick r = p: the conditioned column c_j = k(g_j, g_p) - sum of the chunks (increasing) - sum_{s < r} g^(s)_j g^(s)_p
// (increasing s), g^(r)_j = c_j / sqrt(max(c_p, 0) + noise + jitter), v_j -= g_j^2, the incumbent with the believed value
// (mean[p], and for POI its sd after the update: the reference's tuple quirk), and the map of round r + 1.  c_p is
// computed by thread 0 of every workgroup with the code of every other entry.  Grid-stride over M.
template <int KIND>
__global__ __launch_bounds__(256) void believer_finish_kernel(const BelFinish a) {
    __shared__ double sh_cp;
    const ThetaDev t = *a.th;
    const int64_t M = a.M, mp = a.mp;
    int64_t p = *a.pick;
    const bool on = p >= 0 && p < M;
    if (!on) p = 0;                                     // (addresses stay inside; nothing read through them is used)
    double xp[GPIMHIP_MAX_DIM], pn;
    bel_point(a.Xs, p, a.d, t, xp, pn);
    const double* grow = a.gs + p;                      // g^(s)_p = grow[s * mp]
    auto column = [&](int64_t j) {
        double xj[GPIMHIP_MAX_DIM], jn;
        bel_point(a.Xs, j, a.d, t, xj, jn);
        double dot = xj[0] * xp[0];
#pragma unroll
        for (int k = 1; k < GPIMHIP_MAX_DIM; ++k) dot = fma(xj[k], xp[k], dot);
        const double r2 = clamp0_nan((jn - 2.0 * dot) + pn);
        double s = a.part[j];
        for (int k = 1; k < a.nR; ++k) s += a.part[(int64_t)k * mp + j];
        double c = t.var * kfun_value<KIND>(r2, t.alpha) - s;
        for (int q = 0; q < a.r; ++q) c = fma(-a.gs[(int64_t)q * mp + j], grow[(int64_t)q * mp], c);
        return c;
    };
    if (threadIdx.x == 0) sh_cp = on ? column(p) : 0.0;
    __syncthreads();
    const double cpp = sh_cp;
    const double den = sqrt(clamp0_nan(cpp) + t.diag_add);
    double b = 0.0;
    if (a.kind != GPIMHIP_ACQ_CB) {
        b = a.inc[a.r];
        if (on) {
            const double gp = cpp / den;
            b = fmax(b, a.mean[p]);
            if (a.kind == GPIMHIP_ACQ_POI) b = fmax(b, sqrt(clamp0_nan(fma(-gp, gp, a.v_in[p])) + t.noise));
        }
        if (blockIdx.x == 0 && threadIdx.x == 0) a.inc[a.r + 1] = b;
    }
    const double acq_a = a.kind == GPIMHIP_ACQ_CB ? a.p0 : b;
    double* gout = a.gs + (int64_t)a.r * mp;
    for (int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x; j < M; j += (int64_t)gridDim.x * 256) {
        double v = a.v_in[j], g = 0.0;
        if (on) {
            g = column(j) / den;
            v = fma(-g, g, v);
        }
        gout[j] = g;
        a.v_out[j] = v;
        const double sd = sqrt(clamp0_nan(v) + t.noise);
        if (a.sd_after) a.sd_after[j] = sd;
        if (a.map_next) a.map_next[j] = a.live[j] * acq_value(a.kind, a.mean[j], sd, acq_a, a.p1);
    }
}

extern "C" int gpimhip_acquire_batch(gpimhip_handle h, const gpimhip_model_t* m, const double* X, const double* y, int64_t N,
                                     const double* u, const double* Xs, int64_t M, const double* Xobs, int64_t Mobs,
                                     int32_t kind, double p0, double p1, const double* mask, int32_t q, double* mean_out,
                                     double* sd_out, double* maps_out, double* sd_after_out, int64_t* idx_out, double* val_out,
                                     int64_t* count_out) {
    const std::string who = "gpimhip_acquire_batch";
    GP_TRY(ivr_check(h, who.c_str(), m, X && y && u && Xs, N, M));
    if (q < 1 || q > M) {
        gpim_set_error(who + ": q = " + std::to_string(q) + " picks of M = " + std::to_string(M) + " candidates (1 <= q <= M)");
        return GPIMHIP_E_BADARG;
    }
    if (kind != GPIMHIP_ACQ_CB && kind != GPIMHIP_ACQ_EI && kind != GPIMHIP_ACQ_POI) {
        gpim_set_error(who + ": kind = " + std::to_string(kind) + " is none of GPIMHIP_ACQ_CB, GPIMHIP_ACQ_EI, GPIMHIP_ACQ_POI");
        return GPIMHIP_E_BADARG;
    }
    if (kind != GPIMHIP_ACQ_CB && (!Xobs || Mobs < 1)) {
        gpim_set_error(who + ": EI and POI need the observed rows Xobs (Mobs >= 1): their incumbent is the maximum of the "
                       "posterior there");
        return GPIMHIP_E_BADARG;
    }
    if (!idx_out || !val_out || !count_out || !mean_out || !sd_out) {
        gpim_set_error(who + ": idx_out, val_out, count_out, mean_out and sd_out are not optional");
        return GPIMHIP_E_BADARG;
    }
    HIP_TRY(hipSetDevice(h->device));
    IvrWs* w = ivr_ws(h);
    const int64_t npn = pad_to(N, NB), mp = pad_to(M, NB), ldm = mp + 16;       // (W as gpimhip_ivr_exact lays it out)
    const int rc = gemv_tri_rc(npn), nR = gemv_tri_chunks(npn);
    // every buffer before anything is enqueued
    GP_TRY(w->W.grow(h, npn * ldm));
    GP_TRY(w->bpart.grow(h, (int64_t)nR * mp));
    GP_TRY(w->v.grow(h, 2 * M));
    GP_TRY(w->gs.grow(h, (int64_t)q * mp));
    GP_TRY(w->live.grow(h, M));
    GP_TRY(w->inc.grow(h, (int64_t)q + 1));
    if (!maps_out) GP_TRY(w->row.grow(h, M));
    const bool has_inc = kind != GPIMHIP_ACQ_CB;
    if (has_inc) GP_TRY(acq_incumbent_reserve(h, kind, Mobs));
    GP_TRY(model_state_at_u(h, m, X, 0, y, N, 1, u));
    const int64_t np = h->np;
    if (np != npn) {
        gpim_set_error(who + ": the workspace's padded order is not pad(N, 128)");
        return GPIMHIP_E_BADARG;
    }
    double* inc = w->inc;
    // b_0: gpimhip_acquire_exact's incumbent, always on the slab path
    if (has_inc) GP_TRY(acq_incumbent(h, m, X, N, Xobs, Mobs, kind, false, inc));
    GP_TRY(ivr_build_w(h, m, X, N, Xs, M, w->W, ldm, mean_out));
    GP_TRY(launch_ivr_live_init(h, mask, M, w->live));
    const dim3 pass((unsigned)(mp / BEL_STRIP), (unsigned)nR);
    const double *W = w->W, *live = w->live;
    double *part = w->bpart, *v0 = w->v, *v1 = w->v + M;
    double* map = maps_out ? maps_out : (double*)w->row;
    hipLaunchKernelGGL(wcolsq_kernel, pass, dim3(256), 0, h->stream, W, ldm, np, mp, rc, part);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(believer_init_kernel, ivr_grid(M), dim3(256), 0, h->stream, (const double*)part, nR, mp, M,
                       (const ThetaDev*)h->theta, (int)kind, p0, p1, (const double*)inc, (const double*)mean_out, live, v0,
                       sd_out, map);
    HIP_TRY(hipGetLastError());
    for (int r = 0; r < q; ++r) {
        GP_TRY(launch_ivr_pick(h, map, M, r, w->live, idx_out, val_out, count_out));
        const bool last = r == q - 1;
        if (last && !sd_after_out) break;               // nothing reads the variance after the last pick
        hipLaunchKernelGGL(believer_col_kernel, pass, dim3(256), 0, h->stream, W, ldm, np, M, mp, rc,
                           (const int64_t*)(idx_out + r), part);
        HIP_TRY(hipGetLastError());
        if (!last && maps_out) map = maps_out + (int64_t)(r + 1) * M;
        BelFinish a;
        a.part = part; a.nR = nR; a.mp = mp; a.M = M;
        a.Xs = Xs; a.d = m->dim; a.th = h->theta;
        a.pick = idx_out + r; a.r = r;
        a.gs = w->gs;
        a.v_in = (r & 1) ? v1 : v0; a.v_out = (r & 1) ? v0 : v1;
        a.mean = mean_out; a.live = live;
        a.kind = kind; a.p0 = p0; a.p1 = p1;
        a.inc = inc;
        a.map_next = last ? nullptr : map;
        a.sd_after = last ? sd_after_out : nullptr;
        GP_TRY(with_kind(m->kernel, [&](auto K) {
            hipLaunchKernelGGL(believer_finish_kernel<decltype(K)::value>, ivr_grid(M), dim3(256), 0, h->stream, a);
            HIP_TRY(hipGetLastError());
            return GPIMHIP_OK;
        }));
    }
    return finish_and_check(h);
}
