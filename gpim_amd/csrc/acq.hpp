// acq.hpp -- what the acquisition layer shares: the CB / EI / POI formula (acq_value), how a sweep is specified (AcqSpec) and
// where it goes (AcqOut), the two launchers of predict.hip that take them, and the incumbent of EI / POI (acquire.hip).
// DESIGN.md section 29 says which file holds what.
#pragma once
#include "common.hpp"

// The acquisition functions of acqfunc.py:11-92 (Phi / phi as scipy.stats.norm: ndtr(z) = erfc(-z / sqrt2) / 2), pinned to
// the reference's goldens through acq_kernel (select.hip).  a = alpha (CB) or the incumbent (EI / POI), b = beta or xi.
// The product with a mask or a live vector stays with the caller.
__device__ __forceinline__ double acq_value(int kind, double mu, double s, double a, double b) {
    if (kind == GPIMHIP_ACQ_CB) return a * mu + b * s;
    const double imp = mu - a - b;
    const double zz = imp / s;
    const double cdf = 0.5 * erfc(-zz * 0.7071067811865476);
    if (kind == GPIMHIP_ACQ_POI) return cdf;
    const double pdf = exp(-0.5 * zz * zz) * 0.3989422804014327;
    return imp * cdf + s * pdf;
}

// kind < 0: no acquisition.  p0_dev non-null: the incumbent comes from device memory (no host round trip between the
// observed-rows prediction, its nanmax and the sweep), else p0.  mask: M doubles of 1 / NaN or null.
struct AcqSpec { int kind; double p0; const double* p0_dev; double p1; const double* mask; };
// sd_out = sqrt(var) and acq_out = mask * acq_value(mean, sd), M doubles each, either may be null
struct AcqOut { AcqSpec spec; double* sd_out; double* acq_out; };

// predict.hip.  The fused launch: mean / var (and with acq: sd, the sweep; single problem only) at M test points from the
// factorised model held in the workspace (theta, L^-1 in A, alpha); var_out may be null when acq->sd_out is given.
int launch_predict_fused(gpimhip_ctx* h, const gpimhip_model_t* m, const double* X, int64_t x_bs, int64_t N, const double* Xs,
                         int64_t M, double* mean_out, double* var_out, const AcqOut* acq = nullptr);
// the same outputs behind the slab path, from its mean and variance (sd_out may be var)
int launch_acq_from_var(gpimhip_ctx* h, const double* mean, const double* var, int64_t M, const AcqOut& acq);

// acquire.hip.  The incumbent of EI / POI: nanmax of the posterior at the observed rows (EI: means; POI: means and sds -- the
// reference's tuple quirk), on device.  reserve grows h->acq_tmp and, where the two-stage nanmax will run, h->sel_scratch;
// acq_incumbent enqueues the prediction (the fused launch where allowed and fused_predict_fits, else the slab path), the
// sd and the nanmax into *best_out, from the model's state in the workspace.
int acq_incumbent_reserve(gpimhip_ctx* h, int kind, int64_t Mobs);
int acq_incumbent(gpimhip_ctx* h, const gpimhip_model_t* m, const double* X, int64_t N, const double* Xobs, int64_t Mobs,
                  int kind, bool allow_fused, double* best_out);
