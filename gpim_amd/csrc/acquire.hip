// acquire.hip -- the acquisition, ranking and thinning entries of the C ABI: gpimhip_acq, gpimhip_acquire_exact,
// gpimhip_nanmax, gpimhip_topk, gpimhip_thin_batch, and the incumbent of EI / POI that gpimhip_acquire_exact shares with
// gpimhip_acquire_batch (believer.hip).  Host code only: the kernels they launch are in select.hip and predict.hip
// (DESIGN.md section 29).
#include <stdlib.h>
#include "acq.hpp"

int sel_scratch_ensure(gpimhip_ctx* h) {
    if (h->sel_scratch) return GPIMHIP_OK;
    return h->sel_scratch.alloc(h, (int64_t)sel_scratch_bytes());
}

// what the nanmax runs over in h->acq_tmp = [means | sds | ...]: the means (EI) or both (POI)
static int64_t incumbent_count(int kind, int64_t Mobs) { return kind == GPIMHIP_ACQ_EI ? Mobs : 2 * Mobs; }

int acq_incumbent_reserve(gpimhip_ctx* h, int kind, int64_t Mobs) {
    GP_TRY(h->acq_tmp.grow(h, 2 * Mobs + 2));
    if (incumbent_count(kind, Mobs) > 4096) GP_TRY(sel_scratch_ensure(h));
    return GPIMHIP_OK;
}

int acq_incumbent(gpimhip_ctx* h, const gpimhip_model_t* m, const double* X, int64_t N, const double* Xobs, int64_t Mobs,
                  int kind, bool allow_fused, double* best_out) {
    double *mo = h->acq_tmp, *so = h->acq_tmp + Mobs;
    const AcqOut sd_only{{-1, 0.0, nullptr, 0.0, nullptr}, so, nullptr};
    if (allow_fused && !h->fp32 && fused_predict_fits(h->np)) {
        GP_TRY(launch_predict_fused(h, m, X, 0, N, Xobs, Mobs, mo, nullptr, &sd_only));
    } else {
        PredictFamily f = stationary_family(h, m, X, 0, N, 1, Xobs, Mobs, mo, so);
        f.fused = nullptr;
        GP_TRY(predict_cols(h, f, N, 1));
        GP_TRY(launch_acq_from_var(h, mo, so, Mobs, sd_only));
    }
    const int64_t nmax = incumbent_count(kind, Mobs);
    if (nmax <= 4096) return launch_nanmax(h, mo, nmax, best_out);
    return launch_nanmax_two_stage(h, mo, nmax, best_out);
}

extern "C" {

int gpimhip_acq(gpimhip_handle h, int32_t kind, const double* mean, const double* sd, int64_t M, double p0,
                double p1, const double* mask, double* acq_out) {
    if (!h || !mean || !sd || !acq_out || M < 1 || kind < 0 || kind > GPIMHIP_ACQ_POI) return GPIMHIP_E_BADARG;
    HIP_TRY(hipSetDevice(h->device));
    return launch_acq(h, kind, mean, sd, M, p0, p1, mask, acq_out);
}

int gpimhip_acquire_exact(gpimhip_handle h, const gpimhip_model_t* m, const double* X, const double* y, int64_t N,
                          const double* u, const double* Xs, int64_t M, const double* Xobs, int64_t Mobs, int32_t kind,
                          double p0, double p1, const double* mask, double* mean_out, double* sd_out, double* acq_out) {
    if (!h || !X || !y || !u || !Xs || M < 1 || N < 1 || !mean_out || !sd_out || !acq_out || kind < 0 ||
        kind > GPIMHIP_ACQ_POI || (kind != GPIMHIP_ACQ_CB && (!Xobs || Mobs < 1)))
        return GPIMHIP_E_BADARG;
    GP_TRY(check_model(m));
    HIP_TRY(hipSetDevice(h->device));
    h->nbatch = 1;
    GP_TRY(ws_ensure_padded(h, N));
    const int64_t np = h->np;
    const bool has_inc = kind != GPIMHIP_ACQ_CB;
    if (has_inc) GP_TRY(acq_incumbent_reserve(h, kind, Mobs));
    HIP_TRY(hipMemsetAsync(h->info, 0, sizeof(int32_t), h->stream));
    GP_TRY(launch_pad_copy(h, y, N, h->ypad, np));
    GP_TRY(factor_at_u(h, m, X, 0, N, u));
    // the incumbent stays on the device: slot 2 Mobs of acq_tmp, behind the observed rows' means and sds
    double* inc = has_inc ? h->acq_tmp + 2 * Mobs : nullptr;
    if (has_inc) GP_TRY(acq_incumbent(h, m, X, N, Xobs, Mobs, kind, true, inc));
    const AcqOut out{{kind, p0, inc, p1, mask}, sd_out, acq_out};
    if (!h->fp32 && fused_predict_fits(np)) {
        GP_TRY(launch_predict_fused(h, m, X, 0, N, Xs, M, mean_out, nullptr, &out));
    } else {
        // sd_out doubles as the variance buffer of the slab path
        GP_TRY(predict_cols(h, stationary_family(h, m, X, 0, N, 1, Xs, M, mean_out, sd_out), N, 1));
        GP_TRY(launch_acq_from_var(h, mean_out, sd_out, M, out));
    }
    return finish_and_check(h);
}

int gpimhip_nanmax(gpimhip_handle h, const double* x, int64_t n, double* out) {
    if (!h || !x || !out || n < 1) return GPIMHIP_E_BADARG;
    HIP_TRY(hipSetDevice(h->device));
    if (n <= 4096) return launch_nanmax(h, x, n, out);
    GP_TRY(sel_scratch_ensure(h));
    return launch_nanmax_two_stage(h, x, n, out);
}

int gpimhip_topk(gpimhip_handle h, const double* acq, int64_t M, int32_t k, int32_t keep_nan, double* vals_out,
                 int64_t* idx_out, int64_t* count_out) {
    if (!h || !acq || !vals_out || !idx_out || !count_out || M < 1 || k < 1) return GPIMHIP_E_BADARG;
    HIP_TRY(hipSetDevice(h->device));
    GP_TRY(h->keys.grow(h, M));
    // large grids: multi-block radix selection (15 launches, O(M) each); small ones: k arg-max passes of one
    // workgroup (2 launches)
    if (M > 2048 && k <= 1024 && M < ((int64_t)1 << 32) && !getenv("GPIMHIP_NO_RADIX_TOPK")) {
        GP_TRY(sel_scratch_ensure(h));
        return launch_topk_radix(h, acq, M, k, keep_nan, vals_out, idx_out, count_out);
    }
    return launch_topk(h, acq, M, k, keep_nan, vals_out, idx_out, count_out);
}

int gpimhip_thin_batch(gpimhip_handle h, const double* vals, const int64_t* flat_idx, int32_t n, int32_t d,
                       const int64_t* shape, double dscale, int32_t max_out, int32_t* keep_out, int32_t* nkeep_out) {
    if (!h || !vals || !flat_idx || !shape || !keep_out || !nkeep_out || n < 1 || n > 1024 || d < 1 ||
        d > GPIMHIP_MAX_DIM || max_out < 1)
        return GPIMHIP_E_BADARG;
    HIP_TRY(hipSetDevice(h->device));
    return launch_thin_batch(h, vals, flat_idx, n, d, shape, dscale, max_out, keep_out, nkeep_out);
}

}  // extern "C"
