// predict.hip -- fused posterior (+ acquisition) kernel for models with few observations
// (the "K* never written to HBM" design; replaces gpmodel.predict inside
// the acquisition functions, gpim/gpbayes/acqfunc.py:27-29,58-60,86-88, and GPRegression.forward,
// gpim/gpreg/gpr.py:243-250, when N <= 384).
//
// One workgroup owns CT = 32 test points.  It
//   1. builds its K(X, X*) panel (np x 32) in LDS with the arithmetic of kmat_kernel (same bits as the slab
//      the large-N path writes to HBM),
//   2. mean_c = sum_k K*[k][c] alpha[k]                         (fixed-shape 8-way split, LDS reduce),
//   3. W = L^-1 K* on v_mfma_f64_16x16x4_f64: every wave takes 16-row tiles of L^-1 (fragments straight
//      from L2 -- L^-1 is at most 1.2 MB and shared by all workgroups), both 16-column tiles of the panel;
//      only the column sums of squares of W are kept,
//   4. var_c = clamp(s2 - sum_i W[i][c]^2, 0) + noise, and optionally sd, CB / EI / POI (incumbent read
//      from device memory, so the observed-rows prediction -> nanmax -> grid sweep chain needs no host
//      round trip) and the NaN mask.
// The large-N path keeps the slab: there every 128-row tile of L^-1 K* would have to regenerate the K*
// operand of its whole k-range (N/256 times the exp() work per element on average) inside a loop that is
// MFMA-bound, while writing and re-reading the slab costs 1.5 % of the product's time.
//
// Behind it: the epilogues of that slab path (predict_var, copy_slice, predict_coupled) and the leave-one-out predictions
// from one factorisation (colsq_tri, loo_finish, loo_score).
#include "kfun.hpp"
#include "tile128.hpp"
#include "acq.hpp"

typedef double d4 __attribute__((ext_vector_type(4)));

#define PF_CT 32
#define PF_LDK (PF_CT + 16)     // row stride of the K* panel in LDS: 4 k-rows of a B fragment hit distinct banks

struct FusedPredictArgs {
    const double* X; int64_t N; int64_t x_bs; int d;
    const double* Xs; int64_t M;
    const ThetaDev* th;
    const double* Linv; int64_t ld; int64_t np;
    const double* alpha;
    double* mean_out; double* var_out;           // M each (per problem), var_out may be null when acq.sd_out is given
    AcqOut acq;                                  // optional outputs (single problem only)
};

template <int KIND>
__global__ __launch_bounds__(256, 2) void predict_fused_kernel(FusedPredictArgs a) {
    extern __shared__ __attribute__((aligned(16))) double smem[];
    const int np = (int)a.np;
    double* Ks = smem;                                  // [np][PF_LDK]
    double* xa = smem + (size_t)np * PF_LDK;            // [np][5], later red[4][32] + part[8][32]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t c0 = (int64_t)blockIdx.x * PF_CT;
    const int b = blockIdx.y;
    const double* X = a.X + b * a.x_bs;
    const ThetaDev t = a.th[b];
    const double* Linv = a.Linv + (int64_t)b * a.np * a.ld;
    const double* alpha = a.alpha + (int64_t)b * a.np;

    // scaled training coordinates (as kmat_kernel: division by the lengthscale, |a|^2 in slot 4)
    for (int g = tid; g < np; g += 256) {
        double s2 = 0.0;
#pragma unroll
        for (int k = 0; k < GPIMHIP_MAX_DIM; ++k) {
            double v = 0.0;
            if (k < a.d && g < a.N) v = X[(int64_t)g * a.d + k] / t.ls[k];
            xa[g * 5 + k] = v;
            s2 += v * v;
        }
        xa[g * 5 + 4] = s2;
    }
    // this thread's test point (column c) in scaled coordinates
    const int c = tid & (PF_CT - 1), part = tid >> 5;       // 8 row groups
    const int64_t gj = c0 + c;
    double z[GPIMHIP_MAX_DIM], zn = 0.0;
#pragma unroll
    for (int k = 0; k < GPIMHIP_MAX_DIM; ++k) {
        double v = 0.0;
        if (k < a.d && gj < a.M) v = a.Xs[gj * a.d + k] / t.ls[k];
        z[k] = v;
        zn += v * v;
    }
    __syncthreads();
    double msum = 0.0;
    for (int g = part; g < np; g += 8) {
        double dot = xa[g * 5 + 0] * z[0];
        dot = fma(xa[g * 5 + 1], z[1], dot);
        dot = fma(xa[g * 5 + 2], z[2], dot);
        dot = fma(xa[g * 5 + 3], z[3], dot);
        double r2 = (xa[g * 5 + 4] - 2.0 * dot) + zn;
        r2 = clamp0_nan(r2);
        double k = t.var * kfun_value<KIND>(r2, t.alpha);
        if (g >= a.N || gj >= a.M) k = 0.0;
        Ks[g * PF_LDK + c] = k;
        msum = fma(k, alpha[g], msum);
    }
    __syncthreads();                                    // K* panel complete; xa is free
    double* red = xa;                                   // [4][32]
    double* mpart = xa + 4 * PF_CT;                     // [8][32]
    mpart[part * PF_CT + c] = msum;

    // W = L^-1 K*: wave w takes row tiles w, w+4, ...; accumulators for the two 16-column tiles
    double ssq0 = 0.0, ssq1 = 0.0;
    const int nrt = np >> 4;
    const int ar = lane & 15, ak = lane >> 4;
    for (int rt = wave; rt < nrt; rt += 4) {
        d4 acc0 = (d4){0.0, 0.0, 0.0, 0.0}, acc1 = acc0;
        const double* arow = Linv + (int64_t)(rt * 16 + ar) * a.ld + ak;
        double av[4], an[4];
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) av[kk] = arow[kk * 4];
        for (int kb = 0; kb <= rt; ++kb) {
            if (kb < rt) {
#pragma unroll
                for (int kk = 0; kk < 4; ++kk) an[kk] = arow[(kb + 1) * 16 + kk * 4];
            }
            const double* bp = Ks + (kb * 16 + ak) * PF_LDK + ar;
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) {
                const double b0 = bp[kk * 4 * PF_LDK], b1 = bp[kk * 4 * PF_LDK + 16];
                acc0 = __builtin_amdgcn_mfma_f64_16x16x4f64(av[kk], b0, acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f64_16x16x4f64(av[kk], b1, acc1, 0, 0, 0);
            }
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) av[kk] = an[kk];
        }
#pragma unroll
        for (int rg = 0; rg < 4; ++rg) {
            ssq0 = fma(acc0[rg], acc0[rg], ssq0);
            ssq1 = fma(acc1[rg], acc1[rg], ssq1);
        }
    }
    // D layout: column = lane & 15 -> add the four lane groups, then the four waves (fixed order)
    ssq0 += __shfl_xor(ssq0, 16);
    ssq0 += __shfl_xor(ssq0, 32);
    ssq1 += __shfl_xor(ssq1, 16);
    ssq1 += __shfl_xor(ssq1, 32);
    if (lane < 16) {
        red[wave * PF_CT + lane] = ssq0;
        red[wave * PF_CT + 16 + lane] = ssq1;
    }
    __syncthreads();
    if (tid < PF_CT && c0 + tid < a.M) {
        const int64_t j = c0 + tid;
        double q = red[tid];
        q += red[PF_CT + tid];
        q += red[2 * PF_CT + tid];
        q += red[3 * PF_CT + tid];
        double mu = mpart[tid];
#pragma unroll
        for (int p = 1; p < 8; ++p) mu += mpart[p * PF_CT + tid];
        const double var = clamp0_nan(t.var - q) + t.noise;
        a.mean_out[(int64_t)b * a.M + j] = mu;
        if (a.var_out) a.var_out[(int64_t)b * a.M + j] = var;
        const AcqOut& o = a.acq;
        if (o.sd_out || o.acq_out) {
            const double s = sqrt(var);
            if (o.sd_out) o.sd_out[j] = s;
            if (o.acq_out) {
                double v = acq_value(o.spec.kind, mu, s, o.spec.p0_dev ? *o.spec.p0_dev : o.spec.p0, o.spec.p1);
                if (o.spec.mask) v = o.spec.mask[j] * v;
                o.acq_out[j] = v;
            }
        }
    }
}

// sd = sqrt(var) and the acquisition sweep for the slab path (N > 384), incumbent from device memory
__global__ void acq_from_var_kernel(const double* __restrict__ mean, const double* __restrict__ var, int64_t M, AcqOut o) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= M) return;
    const double mu = mean[j], s = sqrt(var[j]);
    if (o.sd_out) o.sd_out[j] = s;
    if (!o.acq_out) return;
    double v = acq_value(o.spec.kind, mu, s, o.spec.p0_dev ? *o.spec.p0_dev : o.spec.p0, o.spec.p1);
    if (o.spec.mask) v = o.spec.mask[j] * v;
    o.acq_out[j] = v;
}
int launch_acq_from_var(gpimhip_ctx* h, const double* mean, const double* var, int64_t M, const AcqOut& acq) {
    hipLaunchKernelGGL(acq_from_var_kernel, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, h->stream, mean, var, M, acq);
    HIP_TRY(hipGetLastError());
    return GPIMHIP_OK;
}

bool fused_predict_fits(int64_t np) {
    return np <= 384 && !getenv("GPIMHIP_NO_FUSED_PREDICT");
}

// (acq.hpp) no acq: mean and var only
int launch_predict_fused(gpimhip_ctx* h, const gpimhip_model_t* m, const double* X, int64_t x_bs, int64_t N, const double* Xs,
                         int64_t M, double* mean_out, double* var_out, const AcqOut* acq) {
    FusedPredictArgs a;
    a.X = X; a.N = N; a.x_bs = x_bs; a.d = m->dim;
    a.Xs = Xs; a.M = M; a.th = h->theta;
    a.Linv = h->A; a.ld = h->ld; a.np = h->np; a.alpha = h->alpha;
    a.mean_out = mean_out; a.var_out = var_out;
    a.acq = acq ? *acq : AcqOut{{-1, 0.0, nullptr, 0.0, nullptr}, nullptr, nullptr};
    const size_t lds = ((size_t)h->np * PF_LDK + std::max<size_t>((size_t)h->np * 5, 12 * PF_CT)) * sizeof(double);
    const dim3 grid((unsigned)((M + PF_CT - 1) / PF_CT), h->nbatch);
    return with_kind(m->kernel, [&](auto K) {
        constexpr int KIND = decltype(K)::value;
        // once per process and kernel; several host threads may predict at the same time (dist.reconstruct_slices)
        static const hipError_t attr_rc = hipFuncSetAttribute((const void*)predict_fused_kernel<KIND>,
                                                              hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        HIP_TRY(attr_rc);
        hipLaunchKernelGGL(predict_fused_kernel<KIND>, grid, dim3(256), lds, h->stream, a);
        HIP_TRY(hipGetLastError());
        return GPIMHIP_OK;
    });
}

// ------------------------------------------------------------------------------------------
// epilogues of the slab path (api.hip: predict_cols): var_j = clamp(s2 - sum_ci colpart[ci][j], 0) + noise
// ------------------------------------------------------------------------------------------
__global__ void predict_var_kernel(const double* __restrict__ colpart, int64_t ldp, int nb, int64_t m0,
                                   int64_t mcount, const ThetaDev* __restrict__ th, double* __restrict__ var_out,
                                   int64_t M) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    colpart += blockIdx.y * nb * ldp;
    th += blockIdx.y;
    var_out += blockIdx.y * M;
    if (j >= mcount) return;
    double q = 0.0;
    for (int ci = 0; ci < nb; ++ci) q += colpart[(int64_t)ci * ldp + j];
    const double v = clamp0_nan(th->var - q);
    var_out[m0 + j] = v + th->noise;
}
__global__ void copy_slice_kernel(const double* __restrict__ src, double* __restrict__ dst, int64_t n,
                                  int64_t s_bs, int64_t d_bs) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j < n) dst[blockIdx.y * d_bs + j] = src[blockIdx.y * s_bs + j];
}
int launch_predict_var(gpimhip_ctx* h, int64_t ldp, int nb, int64_t m0, int64_t mcount, double* var_out, int64_t M) {
    hipLaunchKernelGGL(predict_var_kernel, dim3((unsigned)((mcount + 255) / 256), h->nbatch), dim3(256), 0, h->stream,
                       h->colpart, ldp, nb, m0, mcount, h->theta, var_out, M);
    HIP_TRY(hipGetLastError());
    return GPIMHIP_OK;
}
int launch_copy_slice(gpimhip_ctx* h, const double* src, double* dst, int64_t n, int64_t s_bs, int64_t d_bs) {
    hipLaunchKernelGGL(copy_slice_kernel, dim3((unsigned)((n + 255) / 256), h->nbatch), dim3(256), 0, h->stream, src,
                       dst, n, s_bs, d_bs);
    HIP_TRY(hipGetLastError());
    return GPIMHIP_OK;
}
// posterior of the coupled reflection blocks: mean_j = sum_b mean_b[j], var_j = clamp(s2 - sum_b sum_ci colpart_b[ci][j], 0)
// + noise (the variance only for the chunk's first nvar test points: ReflArgs::var_count)
__global__ void predict_coupled_kernel(const double* __restrict__ colpart, int64_t ldp, int nb, int B, int64_t m0, int64_t mcount,
                                       int64_t nvar, const double* __restrict__ mean_tmp, int64_t mean_bs,
                                       const ThetaDev* __restrict__ th, double* __restrict__ mean_out, double* __restrict__ var_out,
                                       int raw, const double* __restrict__ radd) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= mcount) return;
    double q = 0.0, mu = 0.0;
    for (int b = 0; b < B; ++b) {
        if (j < nvar)
            for (int ci = 0; ci < nb; ++ci) q += colpart[((int64_t)b * nb + ci) * ldp + j];
        mu += mean_tmp[b * mean_bs + j];
    }
    mean_out[m0 + j] = mu;
    // radd (border of the missing points): + |sum_b Y_b^T k*_b|^2
    if (j < nvar) var_out[m0 + j] = raw ? q : (radd ? clamp0_nan((th->var - q) + radd[j]) : clamp0_nan(th->var - q)) + th->noise;
}
int launch_predict_coupled(gpimhip_ctx* h, int64_t ldp, int nb, int64_t m0, int64_t mcount, int64_t nvar, int64_t mean_bs,
                           double* mean_out, double* var_out, const double* radd) {
    hipLaunchKernelGGL(predict_coupled_kernel, dim3((unsigned)((mcount + 255) / 256)), dim3(256), 0, h->stream, h->colpart, ldp,
                       nb, h->nbatch, m0, mcount, nvar, h->mean_tmp, mean_bs, h->theta, mean_out, var_out, h->refl.raw, radd);
    HIP_TRY(hipGetLastError());
    return GPIMHIP_OK;
}

// ------------------------------------------------------------------------------------------
// Leave-one-out cross-validation from one factorisation (gpimhip_loo_*).  With S = K + (noise +
// jitter) I, alpha = S^-1 y and d_i = [S^-1]_ii the prediction of y_i from the other N - 1 observations is
//     mu_i = y_i - alpha_i / d_i,    var_i = max(1 / d_i - (noise + jitter), 0) + noise      (predict()'s convention)
// and d_i = sum_{k >= i} (L^-1)_ki^2: the column sums of squares of the triangular inverse that every model state already
// holds in h->A -- one HBM-bound pass over N^2 / 2 entries, no O(N^3) product.
// colsq_tri_kernel is gemv_t_tri_kernel (engine.hip) with a * a in place of a * x: the same (column block, row chunk)
// workgroups, the same two-rows-per-instruction loads, double accumulation, per-chunk partial sums that the consumer adds in
// increasing chunk order (gemv_tri_alpha).  Rows >= N (the identity padding, which a ragged factorisation never writes) are
// not read: a chunk that lies wholly in the padding writes zeros.
// ------------------------------------------------------------------------------------------
template <typename R>
__global__ __launch_bounds__(256) void colsq_tri_kernel(const R* __restrict__ A, int64_t ld, int64_t np, int64_t N,
                                                        double* __restrict__ part, int rc, int nR, int64_t a_bs) {
    __shared__ d2 red[4][32];
    const int cb = blockIdx.x / nR, r = blockIdx.x % nR;
    const int64_t diag0 = ((int64_t)cb * 64 / NB) * NB;
    int64_t i0 = (int64_t)r * rc, i1 = i0 + rc < np ? i0 + rc : np;
    if (i1 <= diag0 || (int64_t)cb * 64 >= N) return;          // structurally zero / padding columns: never read by the sum
    if (i0 < diag0) i0 = diag0;
    if (i1 > N) i1 = N;
    A += blockIdx.y * a_bs;
    part += ((int64_t)blockIdx.y * nR + r) * np;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, cp = lane & 31, rp = lane >> 5;
    typedef typename Vec2<R>::T RV;
    const R* col = A + (int64_t)cb * 64 + 2 * cp;
    d2 s0 = (d2){0.0, 0.0}, s1 = s0, s2 = s0, s3 = s0;
    int64_t i = i0 + 2 * wave + rp;                             // rows i, i + 8, i + 16, ... (8 = 4 waves x 2 rows)
    for (; i + 24 < i1; i += 32) {
        const RV a0 = *reinterpret_cast<const RV*>(col + i * ld), a1 = *reinterpret_cast<const RV*>(col + (i + 8) * ld);
        const RV a2 = *reinterpret_cast<const RV*>(col + (i + 16) * ld), a3 = *reinterpret_cast<const RV*>(col + (i + 24) * ld);
        s0[0] = fma((double)a0[0], (double)a0[0], s0[0]); s0[1] = fma((double)a0[1], (double)a0[1], s0[1]);
        s1[0] = fma((double)a1[0], (double)a1[0], s1[0]); s1[1] = fma((double)a1[1], (double)a1[1], s1[1]);
        s2[0] = fma((double)a2[0], (double)a2[0], s2[0]); s2[1] = fma((double)a2[1], (double)a2[1], s2[1]);
        s3[0] = fma((double)a3[0], (double)a3[0], s3[0]); s3[1] = fma((double)a3[1], (double)a3[1], s3[1]);
    }
    for (; i < i1; i += 8) {
        const RV a0 = *reinterpret_cast<const RV*>(col + i * ld);
        s0[0] = fma((double)a0[0], (double)a0[0], s0[0]); s0[1] = fma((double)a0[1], (double)a0[1], s0[1]);
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
// part: gemv_tri_chunks(np) * np doubles per problem, as launch_gemv_t_tri's (h->gemv_part once alpha has been summed);
// all h->nbatch problems in one launch
int launch_colsq_tri(gpimhip_ctx* h, const double* A, int64_t ld, int64_t np, int64_t N, double* part) {
    const int rc = gemv_tri_rc(np), nR = gemv_tri_chunks(np);
    const dim3 grid((unsigned)((np / 64) * nR), h->nbatch);
    if (h->fp32)
        hipLaunchKernelGGL(colsq_tri_kernel<float>, grid, dim3(256), 0, h->stream, reinterpret_cast<const float*>(A), ld, np, N,
                           part, rc, nR, np * ld);
    else
        hipLaunchKernelGGL(colsq_tri_kernel<double>, grid, dim3(256), 0, h->stream, A, ld, np, N, part, rc, nR, np * ld);
    HIP_TRY(hipGetLastError());
    return GPIMHIP_OK;
}

// The held-out predictions of the n points of s (common.hpp: LooSrc) and their score.  Thread by thread over the points
// (grid stride): d_i and alpha_i -- the point's own entries, or in reflection mode the sums over the blocks that hold its
// representative p,  d_i = sum_s (|Stab_p| / B) [S_s^-1]_pp  and  alpha_i = sum_s chi_s(g_i) sqrt(|Stab_p| / B) alpha_s[p]
// with |Stab_p| = wts^-2 -- then mu, var, the squared residual and log N(y_i | mu, var).  The last two are summed per
// workgroup (block_sum_256) into part[2 * workgroup ..]; loo_score_kernel adds the workgroups' sums in their order: no
// atomics, the same bits on every call.  Only the n points are written.
__global__ __launch_bounds__(256) void loo_finish_kernel(LooSrc s, int64_t n, const ThetaDev* __restrict__ th,
                                                         double* __restrict__ mean_out, double* __restrict__ var_out,
                                                         double* __restrict__ part) {
    __shared__ double red[256];
    const double noise = th->noise, dadd = th->diag_add;
    double elpd = 0.0, sse = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        double d = 0.0, a = 0.0;
        if (s.B == 0) {
            d = gemv_tri_alpha(s.diag_part, s.nR, s.rc, s.np, i);
            a = s.alpha[i];
        } else {
            const int64_t p = s.rep[i];
            const int g = s.sgn[i];
            const double sb = sqrt((double)s.B);
            for (int b = 0; b < s.B; ++b) {
                const double w = s.wts ? s.wts[(int64_t)b * s.Nq + p] : 1.0;
                if (w == 0.0) continue;                         // the point does not exist in this block (an identity row)
                const double c = 1.0 / (w * sb);                // sqrt(|Stab_p| / B)
                d = fma(c * c, gemv_tri_alpha(s.diag_part + (int64_t)b * s.nR * s.np, s.nR, s.rc, s.np, p), d);
                const double t = c * s.alpha[(int64_t)b * s.np + p];
                a += (__popc(b & g) & 1) ? -t : t;
            }
        }
        const double yi = s.y[i];
        const double mu = yi - a / d, v = clamp0_nan(1.0 / d - dadd) + noise;
        const double res = yi - mu;
        mean_out[i] = mu;
        var_out[i] = v;
        elpd -= 0.5 * (log(6.283185307179586476925 * v) + res * res / v);
        sse = fma(res, res, sse);
    }
    elpd = block_sum_256(elpd, red);
    sse = block_sum_256(sse, red);
    if (threadIdx.x == 0) {
        part[2 * blockIdx.x] = elpd;
        part[2 * blockIdx.x + 1] = sse;
    }
}
__global__ __launch_bounds__(256) void loo_score_kernel(const double* __restrict__ part, int nblk, double* __restrict__ score) {
    __shared__ double red[256];
    double elpd = 0.0, sse = 0.0;
    for (int k = threadIdx.x; k < nblk; k += 256) {
        elpd += part[2 * k];
        sse += part[2 * k + 1];
    }
    elpd = block_sum_256(elpd, red);
    sse = block_sum_256(sse, red);
    if (threadIdx.x == 0) {
        score[0] = elpd;
        score[1] = sse;
    }
}
// part: 2 * loo_blocks(n) doubles of scratch; theta: the (first) problem's; score_out = [elpd, sse]
int launch_loo_finish(gpimhip_ctx* h, const LooSrc& s, int64_t n, const ThetaDev* theta, double* part, double* mean_out,
                      double* var_out, double* score_out) {
    const int nblk = loo_blocks(n);
    hipLaunchKernelGGL(loo_finish_kernel, dim3(nblk), dim3(256), 0, h->stream, s, n, theta, mean_out, var_out, part);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(loo_score_kernel, dim3(1), dim3(256), 0, h->stream, (const double*)part, nblk, score_out);
    HIP_TRY(hipGetLastError());
    return GPIMHIP_OK;
}
