// kron.hip -- exact GP on a FULLY OBSERVED regular grid through the Kronecker structure of the
// covariance (the role of the reference's structured-kernel reconstructor,
// gpim/gpreg/skgpr.py:399-448 -- there GPyTorch's interpolated SKI approximation, here exact).
//
// For the ARD (or isotropic) RBF kernel on a product grid X = c_1 x c_2 x ... x c_d
//     K = s2 * K_1 (x) K_2 (x) ... (x) K_d,     K_i[a,b] = exp(-((c_i[a] - c_i[b]) / l_i)^2 / 2),
// so with K_i = Q_i diag(lam_i) Q_i^T (n_i x n_i symmetric eigenproblems)
//     K + (jitter + noise) I = Q diag(D) Q^T,   Q = (x) Q_i,   D = s2 * prod_i lam_i[j_i] + jitter + noise.
// Everything the dense path gets from the N x N Cholesky factor and K^-1 -- the loss, the SAME reduced
// gradient sums S[] that csrc/grad.hip:grad_reduce_kernel produces (so the chain rule, the Adam step and
// the history row are the shared finalize_step of theta.hpp), the posterior mean and variance -- follows
// from mode products with the small matrices: O(sum n_i^3 + N sum n_i) instead of O(N^3) work and
// O(N + sum n_i^2) instead of O(N^2) memory.  Same model, same parameterisation, same results as
// gpimhip_fit_exact / gpimhip_predict_exact up to rounding (tests/test_gpu_kron.py checks against the
// dense oracle).
//
// Kernels (all HBM/latency-bound; the work is tiny next to the dense path's):
//   kron_axis_kernel     K_i, E_i = K_i o ((c_a - c_b)/l_i)^2 (= l_i dK_i/dl_i), identity for the rotations
//   kron_reduce_kernel   axes with centro-symmetric coordinates (uniform grids): K_i splits into a symmetric and a
//                        skew-symmetric eigen-problem of half the order
//   kron_eigh_kernel     one-sided (Hestenes) Jacobi, one 16-wave workgroup per eigen-problem, round-robin ordering
//   kron_assemble_kernel eigenvectors of K_i from the rotations of its eigen-problems
//   kron_modeprod_kernel out[p,a,q] = sum_b M[a,b] in[p,b,q]   (tensor-times-matrix along one mode)
//   kron_dvec_kernel     D, alpha~ = y~ / D, first reduction pass;  kron_quad_kernel second pass
//   kron_finalize_kernel sums -> finalize_step;  kron_cross_kernel / kron_var_kernel for the posterior
//   posterior draws on any product test grid (gpimhip_sample_kron), all S draws per launch:
//   kron_root_rows_kernel rows of the prior root of a union axis;  kron_zeta_kernel zeta out of z;  kron_resid_kernel the
//   residual;  kron_dscale_kernel the 1 / D scaling;  kron_draw_kernel the epilogue
// Host drivers: the five entries gpimhip_*_kron (gpimhip_loo_kron: leave-one-out) and the diagnostic gpimhip_kron_eigh, and what the dense-by-Kronecker blocks
// (pkrongp.hip) build on (kron.hpp): the per-axis drivers and the union-axis steps the two draws share (kron_axes_load,
// kron_union_check, kron_union_roots).
#include <limits.h>
#include <math.h>
#include <stdio.h>
#include <string.h>
#include <algorithm>
#include "common.hpp"
#include "kfun.hpp"
#include "theta.hpp"
#include "blocklds.hpp"      // wave_sum: DPP / readlane reduction (no LDS crossbar round trips)

#include "kron.hpp"      // KronDev, KronAxes and the per-axis drivers shared with the dense-by-Kronecker blocks

struct KronWs {
    int d = 0;
    int n[KMAXD] = {0, 0, 0, 0};
    int64_t N = 0;
    KronAxes tr;                 // the training grid's axes
    DevBuf<double> arena;        // the N-sized vectors
    double *yt = nullptr, *at = nullptr, *t1 = nullptr, *t2 = nullptr, *Z = nullptr, *part = nullptr;
    int nblk = 0;
    // prediction
    int m[KMAXD] = {0, 0, 0, 0};
    int64_t M = 0, pmax = 0;
    DevBuf<double> parena;
    double *Ks = nullptr, *Bs = nullptr, *p1 = nullptr, *p2 = nullptr, *tcoords = nullptr;
    int64_t koff[KMAXD] = {0, 0, 0, 0};
    // posterior draws (gpimhip_sample_kron)
    KronAxes un;                 // the union axes, when they differ from the training axes
    DevBuf<double> sarena;
    int64_t s_key[3 + 3 * KMAXD] = {0};      // S, d, buffer size, n_union, n, n_test the workspace was carved for
    double *RG = nullptr, *RT = nullptr, *Zc = nullptr, *sa = nullptr, *sb = nullptr;
    int32_t *ic = nullptr, *it = nullptr;
    // the axis set of the diagnostic gpimhip_kron_eigh (its own: the rotations it leaves in Vr are no fit's warm start)
    KronAxes dg;
    bool dg_ready = false;       // dg holds the rotations of a completed call (what warm = 1 continues from)
};

void kron_release(gpimhip_ctx* h) {
    KronWs* w = static_cast<KronWs*>(h->kron);
    if (!w) return;
    dev_release(h, w->arena, w->tr.arena, w->un.arena, w->dg.arena, w->parena, w->sarena);
    delete w;
    h->kron = nullptr;
}

// the per-axis state for axes of the orders n[]; grad: with E, Mm and mdiag (training)
int kron_axes_ensure(gpimhip_ctx* h, KronAxes& a, int d, const int32_t* n, bool grad) {
    bool same = a.d == d && a.arena && a.grad == grad;
    for (int i = 0; i < d && same; ++i) same = a.n[i] == n[i];
    if (same) return GPIMHIP_OK;
    HIP_TRY(hipStreamSynchronize(h->stream));
    a.arena.release(h);
    a.d = d; a.grad = grad;
    a.sum_n = 0; a.sum_n2 = 0;
    int64_t N = 1;
    for (int i = 0; i < KMAXD; ++i) a.n[i] = i < d ? n[i] : 1;
    for (int i = 0; i < d; ++i) { N *= n[i]; a.sum_n += n[i]; a.sum_n2 += (int64_t)n[i] * n[i]; }
    const int64_t count = (grad ? 3 : 2) * a.sum_n + (grad ? 7 : 5) * a.sum_n2 + 32;
    GP_TRY(a.arena.alloc(h, count, "hipMalloc failed (structured-GP axis workspace)"));
    Carve c(a.arena);
    KronDev& dv = a.dev;
    memset(&dv, 0, sizeof(dv));
    dv.d = d; dv.N = N;
    int off = 0; int64_t moff = 0;
    for (int i = 0; i < KMAXD; ++i) {
        dv.n[i] = a.n[i]; dv.off[i] = off; dv.moff[i] = moff;
        if (i < d) { off += n[i]; moff += (int64_t)n[i] * n[i]; }
    }
    dv.coords = c.take(a.sum_n); dv.lam = c.take(a.sum_n);
    dv.K = c.take(a.sum_n2); dv.W = c.take(a.sum_n2); dv.Qt = c.take(a.sum_n2); dv.Tt = c.take(a.sum_n2); dv.Vr = c.take(a.sum_n2);
    if (grad) { dv.mdiag = c.take(a.sum_n); dv.E = c.take(a.sum_n2); dv.Mm = c.take(a.sum_n2); }
    dv.stat = c.take(2 * 2 * KMAXD);      // out of the 32 spare entries (the ten pieces above round up by at most one each)
    return GPIMHIP_OK;
}

// the handle's workspace with the N-sized vectors of a grid of the orders n[]
static int kron_ensure(gpimhip_ctx* h, int d, const int32_t* n, KronWs** out) {
    if (!h->kron) h->kron = new KronWs();
    KronWs& w = *static_cast<KronWs*>(h->kron);
    *out = &w;
    bool same = w.d == d && w.arena;
    for (int i = 0; i < d && same; ++i) same = w.n[i] == n[i];
    if (same) return GPIMHIP_OK;
    HIP_TRY(hipStreamSynchronize(h->stream));
    w.arena.release(h);
    w.d = d;
    w.N = 1;
    for (int i = 0; i < KMAXD; ++i) w.n[i] = i < d ? n[i] : 1;
    for (int i = 0; i < d; ++i) w.N *= n[i];
    w.nblk = (int)std::min<int64_t>(1024, (w.N + 255) / 256);
    const int64_t count = (4 + d) * w.N + (int64_t)w.nblk * 16 + 32;
    GP_TRY(w.arena.alloc(h, count, "hipMalloc failed (structured-GP workspace)"));
    Carve c(w.arena);
    w.yt = c.take(w.N); w.at = c.take(w.N); w.t1 = c.take(w.N); w.t2 = c.take(w.N);
    w.Z = c.take((int64_t)d * w.N);
    w.part = c.take((int64_t)w.nblk * 16);
    return GPIMHIP_OK;
}

// ------------------------------------------------------------------------------------------
// per-axis matrices
// ------------------------------------------------------------------------------------------
__global__ void kron_axis_kernel(KronDev dv, const ThetaDev* __restrict__ th) {
    const int ax = blockIdx.y;
    const int n = dv.n[ax];
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (int64_t)n * n) return;
    const int a = (int)(e / n), b = (int)(e % n);
    const double* c = dv.coords + dv.off[ax];
    const double il = 1.0 / th->ls[ax];
    const double dl = c[a] * il - c[b] * il;
    const double r2 = dl * dl;
    const double k = exp(-0.5 * r2);
    const int64_t o = dv.moff[ax] + e;
    dv.K[o] = k;
    if (dv.E) dv.E[o] = k * r2;      // (an axis set without the gradient matrices: the union axes of the draws)
}

// Vr <- I for every eigen-problem (cold start of the rotations)
__global__ void kron_eye_kernel(KronDev dv) {
    const int pr = blockIdx.y;
    const int n = dv.pn[pr];
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (int64_t)n * n) return;
    dv.Vr[dv.moff[dv.pax[pr]] + dv.poff[pr] + e] = (e / n == e % n) ? 1.0 : 0.0;
}

// The matrix of each eigen-problem (into Tt): K_i itself, or its restriction to the symmetric / skew-symmetric
// vectors.  With n = 2m (+1), basis (e_a +- e_{n-1-a}) / sqrt2 (and e_m):
//   symmetric  S[a][b] = K[a][b] + K[a][n-1-b],  S[a][m] = S[m][a] = sqrt2 K[a][m],  S[m][m] = K[m][m]
//   skew       D[a][b] = K[a][b] - K[a][n-1-b]
__global__ void kron_reduce_kernel(KronDev dv) {
    const int pr = blockIdx.y;
    const int ax = dv.pax[pr], part = dv.ppart[pr], np_ = dv.pn[pr], n = dv.n[ax], m = n / 2;
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (int64_t)np_ * np_) return;
    const int a = (int)(e / np_), b = (int)(e % np_);
    const double* K = dv.K + dv.moff[ax];
    double v;
    if (part == 0) v = K[(int64_t)a * n + b];
    else if (part == 2) v = K[(int64_t)a * n + b] - K[(int64_t)a * n + (n - 1 - b)];
    else if (a < m && b < m) v = K[(int64_t)a * n + b] + K[(int64_t)a * n + (n - 1 - b)];
    else if (a == m && b == m) v = K[(int64_t)m * n + m];
    else v = 1.4142135623730951 * K[(int64_t)(a < m ? a : b) * n + m];
    dv.Tt[dv.moff[ax] + dv.poff[pr] + e] = v;
}

// Qt rows (eigenvectors of K_i, length n) from the rotations of the eigen-problems
__global__ void kron_assemble_kernel(KronDev dv) {
    const int pr = blockIdx.y;
    const int ax = dv.pax[pr], part = dv.ppart[pr], np_ = dv.pn[pr], n = dv.n[ax], m = n / 2;
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (int64_t)np_ * n) return;
    const int j = (int)(e / n), a = (int)(e % n);
    const double* V = dv.Vr + dv.moff[ax] + dv.poff[pr] + (int64_t)j * np_;
    double v;
    if (part == 0) v = V[a];
    else {
        const int lo = a < m ? a : n - 1 - a;            // mirrored index; a == m only when n is odd
        if ((n & 1) && a == m) v = (part == 1) ? V[m] : 0.0;
        else v = 0.7071067811865476 * V[lo] * ((part == 2 && a >= n - m) ? -1.0 : 1.0);
    }
    dv.Qt[dv.moff[ax] + (int64_t)(dv.plam[pr] + j) * n + a] = v;
}

__device__ __forceinline__ double kwave_sum(double v) { return wave_sum(v); }

// One-sided Jacobi on the rows of the symmetric positive semi-definite W (= its columns): plane rotations
// make the rows mutually orthogonal, W = V K; for symmetric K the accumulated V holds the eigenvectors
// (row j = eigenvector j).  Round-robin (circle) ordering: n/2 disjoint pairs per step, the pairs of a step
// dealt to the 16 waves; per step every wave first forms the rotations of all its pairs (independent
// loads, several pairs in flight), then applies them.
// Stopping rule per pair (i, j) with a = |w_i|^2, b = |w_j|^2, c = w_i . w_j:
//   |c| <= 1e-15 sqrt(a b)                          rows orthogonal to working precision, or
//   |c| <= 2e-15 lmax sqrt(a + b)                   the coupling (V K V^T)_ij ~ c / (lam_i + lam_j) is below
//                                                   ~10 eps * lmax: RBF Gram matrices have most of their
//                                                   spectrum below eps * lmax, and rows that are pure
//                                                   rounding noise never get orthogonal in the relative sense
// Eigenvalue j = (row j of W) . (row j of V) -- keeps the sign of numerically negative ones.
#define EIGH_WAVES 16

// 1/x and 1/sqrt(x) from the hardware seeds (v_rcp_f64 / v_rsq_f64) + two Newton steps: a tenth of the
// instructions of an IEEE divide / square root.  tools/jacobi_prof.hip: with 16 waves on 4 SIMDs the
// rotation arithmetic -- 3 divides and 4 square roots per pair, ~1500 issue cycles -- was what a step waited
// for, not the row loads.
__device__ __forceinline__ double fast_rcp(double x) {
    double y = __builtin_amdgcn_rcp(x);
    y = fma(y, fma(-x, y, 1.0), y);
    return fma(y, fma(-x, y, 1.0), y);
}
__device__ __forceinline__ double fast_rsqrt(double x) {
    double y = __builtin_amdgcn_rsq(x);
    y = y * fma(-0.5 * x * y, y, 1.5);
    return y * fma(-0.5 * x * y, y, 1.5);
}

// rotation that makes rows i, j orthogonal (a = |w_i|^2, b = |w_j|^2, c = w_i . w_j), or false when the pair
// passes the stopping rule above.  With d = b - a, e = 2c:  tan = sign(d e) |e| / (|d| + sqrt(d^2 + e^2)).
// The tests are on squares ((sqrt a + sqrt b)^2 <= 2 (a + b)), so nothing here divides or takes a root the
// slow way; cos = 1/sqrt(1 + tan^2) is accurate to rounding, which is what keeps V orthogonal.
__device__ __forceinline__ bool jacobi_rotation(double a, double b, double c, double lmax, double& cs, double& sn) {
    const double c2 = c * c;
    if (!(c2 > 1e-30 * (a * b) && c2 > (4e-30 * lmax * lmax) * (a + b))) return false;
    const double d = b - a, e = 2.0 * c;
    const double h2 = fma(d, d, e * e);
    const double h = h2 * fast_rsqrt(h2);
    double t = fabs(e) * fast_rcp(fabs(d) + h);
    t = ((d >= 0.0) == (e >= 0.0)) ? t : -t;
    cs = fast_rsqrt(fma(t, t, 1.0));
    sn = cs * t;
    return true;
}

// One step of the round-robin ordering for rows of at most 64 * NPL elements: every wave takes G of its
// pairs at a time, with the four rows of each pair (w_i, w_j, v_i, v_j) held in registers -- one memory
// round trip per G pairs instead of two per pair (the kernel is bound by the latency of these trips).
template <int NPL, int G>
__device__ __forceinline__ double jacobi_step_regs(double* W, double* V, int n, int half, int ring, int step, int wave,
                                                   int lane, double lmax) {
    double any = 0.0;          // largest |sin| applied
    for (int k0 = wave; k0 < half; k0 += EIGH_WAVES * G) {
        double wi[G][NPL], wj[G][NPL], vi[G][NPL], vj[G][NPL];
        int ri[G], rj[G];
        double a[G], b[G], c[G];
#pragma unroll
        for (int g = 0; g < G; ++g) {
            const int k = k0 + g * EIGH_WAVES;
            const int i = (k == 0) ? ring : (step + k) % ring;
            const int j = (step + ring - k) % ring;
            const bool ok = k < half && i < n && j < n;
            ri[g] = ok ? i : -1;
            rj[g] = j;
            a[g] = b[g] = c[g] = 0.0;
#pragma unroll
            for (int q = 0; q < NPL; ++q) {
                const int e = lane + 64 * q;
                const bool in = ok && e < n;
                wi[g][q] = in ? W[(int64_t)i * n + e] : 0.0;
                wj[g][q] = in ? W[(int64_t)j * n + e] : 0.0;
                vi[g][q] = in ? V[(int64_t)i * n + e] : 0.0;
                vj[g][q] = in ? V[(int64_t)j * n + e] : 0.0;
            }
        }
#pragma unroll
        for (int g = 0; g < G; ++g)
#pragma unroll
            for (int q = 0; q < NPL; ++q) {
                a[g] = fma(wi[g][q], wi[g][q], a[g]);
                b[g] = fma(wj[g][q], wj[g][q], b[g]);
                c[g] = fma(wi[g][q], wj[g][q], c[g]);
            }
#pragma unroll
        for (int g = 0; g < G; ++g) { a[g] = kwave_sum(a[g]); b[g] = kwave_sum(b[g]); c[g] = kwave_sum(c[g]); }
#pragma unroll
        for (int g = 0; g < G; ++g) {
            double cs, sn;
            if (ri[g] < 0 || !jacobi_rotation(a[g], b[g], c[g], lmax, cs, sn)) continue;
            any = fmax(any, fabs(sn));
            const int i = ri[g], j = rj[g];
#pragma unroll
            for (int q = 0; q < NPL; ++q) {
                const int e = lane + 64 * q;
                if (e < n) {
                    W[(int64_t)i * n + e] = cs * wi[g][q] - sn * wj[g][q];
                    W[(int64_t)j * n + e] = sn * wi[g][q] + cs * wj[g][q];
                    V[(int64_t)i * n + e] = cs * vi[g][q] - sn * vj[g][q];
                    V[(int64_t)j * n + e] = sn * vi[g][q] + cs * vj[g][q];
                }
            }
        }
    }
    return any;
}

// any row length: rows streamed from memory twice (dot products, then the update)
__device__ __forceinline__ double jacobi_step_stream(double* W, double* V, int n, int half, int ring, int step,
                                                     int wave, int lane, double lmax) {
    double any = 0.0;
    for (int k = wave; k < half; k += EIGH_WAVES) {
        const int i = (k == 0) ? ring : (step + k) % ring;
        const int j = (step + ring - k) % ring;
        if (i >= n || j >= n) continue;
        double* wi = W + (int64_t)i * n;
        double* wj = W + (int64_t)j * n;
        double a = 0.0, b = 0.0, c = 0.0;
        for (int e = lane; e < n; e += 64) {
            const double x = wi[e], y = wj[e];
            a = fma(x, x, a); b = fma(y, y, b); c = fma(x, y, c);
        }
        a = kwave_sum(a); b = kwave_sum(b); c = kwave_sum(c);
        double cs, sn;
        if (!jacobi_rotation(a, b, c, lmax, cs, sn)) continue;
        any = fmax(any, fabs(sn));
        double* vi = V + (int64_t)i * n;
        double* vj = V + (int64_t)j * n;
        for (int e = lane; e < n; e += 64) {
            const double x = wi[e], y = wj[e], p = vi[e], q = vj[e];
            wi[e] = cs * x - sn * y;
            wj[e] = sn * x + cs * y;
            vi[e] = cs * p - sn * q;
            vj[e] = sn * p + cs * q;
        }
    }
    return any;
}

// NPL = row elements per lane held in registers (rows of at most 64 * NPL entries), G = pairs in flight
// per wave; NPL = 0: rows streamed from memory (any length).  One instantiation per size class, so the
// small ones do not inherit the register footprint of the large ones.
template <int NPL, int G>
__global__ __launch_bounds__(EIGH_WAVES * 64) void kron_eigh_kernel(KronDev dv) {
    __shared__ double s_max[EIGH_WAVES];
    const int pr = blockIdx.x;
    const int ax = dv.pax[pr];
    const int n = dv.pn[pr];
    double* W = dv.W + dv.moff[ax] + dv.poff[pr];
    double* V = dv.Vr + dv.moff[ax] + dv.poff[pr];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n2 = n + (n & 1), half = n2 / 2, ring = n2 - 1;
    // lmax: the largest absolute row sum of K (Gershgorin: an upper bound of the largest eigenvalue, tight
    // within a small factor for these non-negative matrices)
    {
        double mx = 0.0;
        for (int r = wave; r < n; r += EIGH_WAVES) {
            double a = 0.0;
            for (int e = lane; e < n; e += 64) a += fabs(W[(int64_t)r * n + e]);
            mx = fmax(mx, kwave_sum(a));
        }
        if (lane == 0) s_max[wave] = mx;
        __syncthreads();
    }
    double lmax = 0.0;
    for (int w = 0; w < EIGH_WAVES; ++w) lmax = fmax(lmax, s_max[w]);
    // Sweeps until the largest rotation of a sweep is below 1e-8: the method converges quadratically, so
    // what is left after such a sweep is at rounding level (no rotation-free sweep needed to confirm).  The
    // rotations continue from the V the caller left in Vr -- the identity, or the eigenvectors of the
    // previous Adam iteration, whose K differs by a small change of the lengthscale: W = V K then starts
    // almost orthogonal and two or three sweeps are enough instead of 8 ... 18.
    // The cap: measured on the MI355X through gpimhip_kron_eigh (tests/test_gpu_kron_eigh.py), cold starts of order 64 ... 520
    // end by the rule above in 11 ... 30 sweeps.  The two halves of a uniform 1300-point axis at lengthscale 3 (order 650
    // each) run into the cap with rotations of |sin| 0.29 and 0.71 still being applied in sweep 40 -- and are converged all
    // the same: eigenvalues within 0.8 n eps lmax of LAPACK's, orthogonality 1.1 n eps, as good as the problems that stop
    // by themselves.  (Not traced, but consistent with it: what still rotates are rows inside the eps * lmax cluster, whose
    // mutual rotations change nothing that is resolved.)  Nothing above order 650 has been measured.
    int nsweep = 0;
    double all = 0.0;
    for (int sweep = 0; sweep < EIGH_MAX_SWEEPS; ++sweep) {
        ++nsweep;
        if (tid < EIGH_WAVES) s_max[tid] = 0.0;
        __syncthreads();
        double big = 0.0;
        for (int step = 0; step < ring; ++step) {
            double r;
            if (NPL > 0) r = jacobi_step_regs<(NPL > 0 ? NPL : 1), G>(W, V, n, half, ring, step, wave, lane, lmax);
            else r = jacobi_step_stream(W, V, n, half, ring, step, wave, lane, lmax);
            big = fmax(big, r);
            __syncthreads();
        }
        if (lane == 0) s_max[wave] = big;
        __syncthreads();
        all = 0.0;
        for (int w = 0; w < EIGH_WAVES; ++w) all = fmax(all, s_max[w]);
        __syncthreads();
        if (all < 1e-8) break;
    }
    if (tid == 0 && dv.stat) { dv.stat[2 * pr] = (double)nsweep; dv.stat[2 * pr + 1] = all; }
#ifdef KRON_DEBUG
    if (tid == 0) printf("eigh axis %d part %d n %d: %d sweeps, lmax %.3f\n", ax, dv.ppart[pr], n, nsweep, lmax);
#endif
    double* lam = dv.lam + dv.off[ax] + dv.plam[pr];
    for (int j = wave; j < n; j += EIGH_WAVES) {
        double s = 0.0;
        for (int e = lane; e < n; e += 64) s = fma(W[(int64_t)j * n + e], V[(int64_t)j * n + e], s);
        s = kwave_sum(s);
        if (lane == 0) lam[j] = s;
    }
}

// ------------------------------------------------------------------------------------------
// tensor-times-matrix along one mode: out[p, a, q] = sum_b Mx(a, b) in[p, b, q]
//   Mx(a, b) = M[a * ldm + b]  (trans == 0)  or  M[b * ldm + a]  (trans != 0);  sq != 0 squares the entries
// ------------------------------------------------------------------------------------------
__global__ void kron_modeprod_kernel(const double* __restrict__ in, double* __restrict__ out,
                                     const double* __restrict__ M, int ma, int nbk, int ldm, int trans, int sq,
                                     int64_t pre, int64_t post) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= pre * ma * post) return;
    const int64_t q = idx % post, a = (idx / post) % ma, p = idx / (post * ma);
    const double* src = in + p * nbk * post + q;
    double s = 0.0;
    for (int b = 0; b < nbk; ++b) {
        double mv = trans ? M[(int64_t)b * ldm + a] : M[(int64_t)a * ldm + b];
        if (sq) mv *= mv;
        s = fma(mv, src[(int64_t)b * post], s);
    }
    out[idx] = s;
}

int modeprod(gpimhip_ctx* h, const double* in, double* out, const double* M, int ma, int nbk, int ldm,
             int trans, int sq, int64_t pre, int64_t post) {
    const int64_t total = pre * ma * post;
    hipLaunchKernelGGL(kron_modeprod_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, h->stream, in, out, M,
                       ma, nbk, ldm, trans, sq, pre, post);
    HIP_TRY(hipGetLastError());
    return GPIMHIP_OK;
}

// applies, for every axis i, the matrix mats[i] (ma[i] x nb[i]) along mode i of `src` (shape nb[]);
// ping-pongs between bufa/bufb and returns the buffer that holds the result (shape ma[]).  batch > 1: src is `batch`
// contiguous tensors (batch, nb[]) -- the batch index folds into `pre`, so a mode is still one launch.  src may be bufb
// (it is read by the first mode only, which writes bufa), never bufa.
int tensor_apply(gpimhip_ctx* h, int d, const int* nbv, const int* mav, const double* const* mats,
                 const int* ldm, int trans, int sq, const double* src, double* bufa, double* bufb,
                 double** result, int64_t batch) {
    const double* cur = src;
    double* dst = bufa;
    int shape[KMAXD];
    for (int i = 0; i < d; ++i) shape[i] = nbv[i];
    for (int i = 0; i < d; ++i) {
        int64_t pre = batch, post = 1;
        for (int k = 0; k < i; ++k) pre *= shape[k];
        for (int k = i + 1; k < d; ++k) post *= shape[k];
        GP_TRY(modeprod(h, cur, dst, mats[i], mav[i], nbv[i], ldm[i], trans, sq, pre, post));
        shape[i] = mav[i];
        cur = dst;
        dst = (dst == bufa) ? bufb : bufa;
    }
    *result = const_cast<double*>(cur);
    return GPIMHIP_OK;
}

// ------------------------------------------------------------------------------------------
// reductions.  part[blk][0..15]: 0 lg = sum log D / 2, 1 q2 = sum yt^2/D, 2 sum lam/D, 3 sum lam yt^2/D^2,
// 4 sum 1/D, 5 sum yt^2/D^2, 6+i trace part of axis i, 10+i quadratic part of axis i
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ void kron_block_reduce(double* vals, int nv, double* part) {
    __shared__ double red[4][16];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int k = 0; k < nv; ++k) {
        const double v = kwave_sum(vals[k]);
        if (lane == 0) red[wave][k] = v;
    }
    __syncthreads();
    if (threadIdx.x < nv)
        part[(int64_t)blockIdx.x * 16 + threadIdx.x] =
            (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
}

__global__ __launch_bounds__(256) void kron_dvec_kernel(KronDev dv, const ThetaDev* __restrict__ th,
                                                        const double* __restrict__ yt, double* __restrict__ at,
                                                        double* __restrict__ part) {
    const ThetaDev t = *th;
    double v[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x; j < dv.N; j += (int64_t)gridDim.x * 256) {
        int idx[KMAXD];
        int64_t r = j;
        for (int i = dv.d - 1; i >= 0; --i) { idx[i] = (int)(r % dv.n[i]); r /= dv.n[i]; }
        double lam = t.var, l[KMAXD];
        for (int i = 0; i < dv.d; ++i) { l[i] = dv.lam[dv.off[i] + idx[i]]; lam *= l[i]; }
        const double D = lam + t.diag_add;
        const double y = yt[j], a = y / D;
        at[j] = a;
        v[0] += 0.5 * log(D);
        v[1] = fma(y, a, v[1]);
        v[2] += lam / D;
        v[3] = fma(lam * a, a, v[3]);
        v[4] += 1.0 / D;
        v[5] = fma(a, a, v[5]);
        for (int i = 0; i < dv.d; ++i) {
            double po = 1.0;
            for (int k = 0; k < dv.d; ++k) if (k != i) po *= l[k];
            v[6 + i] += dv.mdiag[dv.off[i] + idx[i]] * po / D;
        }
    }
    kron_block_reduce(v, 10, part);
}

// quadratic parts: sum_j at_j * Z_i[j] * prod_{k != i} lam_k[j_k]
__global__ __launch_bounds__(256) void kron_quad_kernel(KronDev dv, const double* __restrict__ at,
                                                        const double* __restrict__ Z, double* __restrict__ part) {
    double v[4] = {0, 0, 0, 0};
    for (int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x; j < dv.N; j += (int64_t)gridDim.x * 256) {
        int idx[KMAXD];
        int64_t r = j;
        for (int i = dv.d - 1; i >= 0; --i) { idx[i] = (int)(r % dv.n[i]); r /= dv.n[i]; }
        double l[KMAXD];
        for (int i = 0; i < dv.d; ++i) l[i] = dv.lam[dv.off[i] + idx[i]];
        const double a = at[j];
        for (int i = 0; i < dv.d; ++i) {
            double po = 1.0;
            for (int k = 0; k < dv.d; ++k) if (k != i) po *= l[k];
            v[i] = fma(a * po, Z[(int64_t)i * dv.N + j], v[i]);
        }
    }
    kron_block_reduce(v, 4, part + 10);
}

__global__ void kron_mdiag_kernel(KronDev dv) {
    const int ax = blockIdx.y, n = dv.n[ax];
    const int a = blockIdx.x * blockDim.x + threadIdx.x;
    if (a < n) dv.mdiag[dv.off[ax] + a] = dv.Mm[dv.moff[ax] + (int64_t)a * n + a];
}

__global__ __launch_bounds__(256) void kron_finalize_kernel(gpimhip_model_t m, KronDev dv, int nblk,
                                                            const double* __restrict__ part,
                                                            const ThetaDev* __restrict__ th, double* __restrict__ u,
                                                            double* __restrict__ adam_m, double* __restrict__ adam_v,
                                                            int do_adam, double* __restrict__ loss_out,
                                                            double* __restrict__ grad_out, FinalizeIter fi,
                                                            int32_t* __restrict__ info) {
    __shared__ double red[256];
    __shared__ double tot[16];
    const int tid = threadIdx.x;
    for (int k = 0; k < 14; ++k) {
        double v = 0.0;
        for (int b = tid; b < nblk; b += 256) v += part[(int64_t)b * 16 + k];
        red[tid] = v;
        __syncthreads();
        for (int s = 128; s > 0; s >>= 1) {
            if (tid < s) red[tid] += red[tid + s];
            __syncthreads();
        }
        if (tid == 0) tot[k] = red[0];
        __syncthreads();
    }
    if (tid != 0) return;
    const ThetaDev t = *th;
    double S[7] = {0, 0, 0, 0, 0, 0, 0};
    S[0] = (tot[2] - tot[3]) / t.var;
    S[5] = tot[4] - tot[5];
    for (int i = 0; i < dv.d; ++i) S[1 + i] = tot[6 + i] - tot[10 + i];
    // a structurally indefinite spectrum (D <= 0) cannot happen with jitter + noise > 0 unless the
    // eigenvalues are garbage (NaN inputs): flag it like a failed factorisation
    if (!(tot[0] == tot[0]) && *info == 0) *info = 1;
    AdamStep st;
    st.beta1 = 0.9; st.beta2 = 0.999; st.eps = 1e-8; st.lr_over_bc1 = 0.0; st.bc2_sqrt = 1.0;
    double* hist_row = nullptr;
    if (!finalize_iter_begin(fi, info, 2 + m.n_ls, st, loss_out, hist_row)) return;
    finalize_step(m, dv.N, S, tot[1], tot[0], t, u, adam_m, adam_v, do_adam, st, loss_out, grad_out, hist_row,
                  prior_constant(m));
}

// ------------------------------------------------------------------------------------------
// posterior
// ------------------------------------------------------------------------------------------
// Ks_i[t, a] = exp(-((ct[t] - c[a]) / l_i)^2 / 2)
__global__ void kron_cross_kernel(KronDev dv, const ThetaDev* __restrict__ th, const double* __restrict__ tcoords,
                                  int toff, int mi, int ax, double* __restrict__ Ks) {
    const int n = dv.n[ax];
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (int64_t)mi * n) return;
    const int t = (int)(e / n), a = (int)(e % n);
    const double il = 1.0 / th->ls[ax];
    const double dl = tcoords[toff + t] * il - dv.coords[dv.off[ax] + a] * il;
    Ks[e] = exp(-0.5 * dl * dl);
}
__global__ void kron_invd_kernel(KronDev dv, const ThetaDev* __restrict__ th, double* __restrict__ out) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= dv.N) return;
    int64_t r = j;
    double lam = th->var;
    for (int i = dv.d - 1; i >= 0; --i) { lam *= dv.lam[dv.off[i] + (int)(r % dv.n[i])]; r /= dv.n[i]; }
    out[j] = 1.0 / (lam + th->diag_add);
}
// (mean_raw may alias mean_out: element j is read before it is written, by the same thread)
__global__ void kron_post_kernel(const double* mean_raw, const double* __restrict__ q, int64_t M,
                                 const ThetaDev* __restrict__ th, double* mean_out, double* __restrict__ var_out) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= M) return;
    const double s2 = th->var;
    mean_out[j] = s2 * mean_raw[j];
    var_out[j] = clamp0_nan(s2 - s2 * s2 * q[j]) + th->noise;
}

// ------------------------------------------------------------------------------------------
// posterior draws (gpimhip_sample_kron); every kernel handles all S draws in one launch
// ------------------------------------------------------------------------------------------
// rows of the prior root R_i = Q_i diag(sqrt(max(lam_i, 0))) of axis ax:  out[r, j] = Q_i[idx[r], j] sqrt(max(lam_i[j], 0))
// (Qt holds Q_i^T; idx was checked against the axis by the host side of the entry point)
__global__ void kron_root_rows_kernel(KronDev dv, int ax, const int32_t* __restrict__ idx, int rows,
                                      double* __restrict__ out) {
    const int n = dv.n[ax];
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (int64_t)rows * n) return;
    const int r = (int)(e / n), j = (int)(e % n);
    const double lam = dv.lam[dv.off[ax] + j];
    out[e] = dv.Qt[dv.moff[ax] + (int64_t)j * n + idx[r]] * sqrt(lam > 0.0 ? lam : 0.0);
}
// zeta of every draw, the first PU entries of its row of z, as one contiguous (S, PU) tensor
__global__ void kron_zeta_kernel(const double* __restrict__ z, int64_t zw, int64_t PU, int64_t total,
                                 double* __restrict__ out) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= total) return;
    out[e] = z[(e / PU) * zw + e % PU];
}
// g[s, j] <- y[j] - sqrt(s2) g[s, j] - sqrt(sigma) z_e[s, j]     (ze: the z_e part of draw 0; rows zw apart)
__global__ void kron_resid_kernel(const double* __restrict__ y, const double* __restrict__ ze, int64_t zw, int64_t N,
                                  int64_t total, const ThetaDev* __restrict__ th, double* __restrict__ g) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= total) return;
    const int64_t s = e / N, j = e % N;
    g[e] = y[j] - sqrt(th->var) * g[e] - sqrt(th->diag_add) * ze[s * zw + j];
}
// v[s, j] <- v[s, j] / D[j] in the eigenbasis of the training grid (the D of kron_dvec_kernel, none of its sums);
// blockIdx.y strides the draws
__global__ void kron_dscale_kernel(KronDev dv, const ThetaDev* __restrict__ th, int64_t S, double* __restrict__ v) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= dv.N) return;
    int idx[KMAXD];
    int64_t r = j;
    for (int i = dv.d - 1; i >= 0; --i) { idx[i] = (int)(r % dv.n[i]); r /= dv.n[i]; }
    double lam = th->var;           // the product in kron_dvec_kernel's order: a draw at z = 0 is the mean, bit for bit
    for (int i = 0; i < dv.d; ++i) lam *= dv.lam[dv.off[i] + idx[i]];
    const double D = lam + th->diag_add;
    for (int64_t s = blockIdx.y; s < S; s += gridDim.y) v[s * dv.N + j] = v[s * dv.N + j] / D;
}
// out[s, j] <- sqrt(s2) g*[s, j] + s2 out[s, j] + sqrt(c) z_n[s, j],  c = (0 if noiseless else noise) + jitter;
// mean[j] <- s2 mean[j] (the arithmetic of kron_post_kernel), by the threads of draw 0
__global__ void kron_draw_kernel(const double* __restrict__ gs, const double* __restrict__ zn, int64_t zw, int64_t M,
                                 int64_t total, const ThetaDev* __restrict__ th, int noiseless, double jitter,
                                 double* __restrict__ mean, double* __restrict__ out) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= total) return;
    const int64_t s = e / M, j = e % M;
    const double s2 = th->var;
    const double c = (noiseless ? 0.0 : th->noise) + jitter;
    double v = fma(sqrt(s2), gs[e], s2 * out[e]);
    if (c > 0.0) v = fma(sqrt(c), zn[s * zw + j], v);
    out[e] = v;
    if (s == 0) mean[j] = s2 * mean[j];
}

// ------------------------------------------------------------------------------------------
// drivers
// ------------------------------------------------------------------------------------------
int kron_cold_start(gpimhip_ctx* h, const KronDev& dv) {
    int nmax = 1;
    for (int pr = 0; pr < dv.nprob; ++pr) nmax = std::max(nmax, dv.pn[pr]);
    hipLaunchKernelGGL(kron_eye_kernel, dim3((unsigned)(((int64_t)nmax * nmax + 255) / 256), dv.nprob), dim3(256), 0,
                       h->stream, dv);
    HIP_TRY(hipGetLastError());
    return GPIMHIP_OK;
}

// Splits every axis whose coordinates are centro-symmetric (c_a + c_{n-1-a} constant: any uniform grid) into a
// symmetric and a skew-symmetric eigen-problem.  Needs the coordinates on the host: one small copy + sync per call.
int kron_plan_problems(gpimhip_ctx* h, KronAxes& ax) {
    std::vector<double> c((size_t)ax.sum_n);
    HIP_TRY(hipMemcpyAsync(c.data(), ax.dev.coords, c.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    KronDev& dv = ax.dev;
    dv.nprob = 0;
    const bool allow = true;
    for (int i = 0; i < ax.d; ++i) {
        const int n = ax.n[i];
        const double* ci = c.data() + dv.off[i];
        bool sym = allow && n >= 8;
        double scale = 1.0;
        for (int a = 0; a < n; ++a) scale = std::max(scale, fabs(ci[a]));
        for (int a = 0; a < n && sym; ++a)
            sym = fabs((ci[a] + ci[n - 1 - a]) - (ci[0] + ci[n - 1])) <= 1e-12 * scale;
        auto add = [&](int part, int order, int64_t off, int lam0) {
            const int pr = dv.nprob++;
            dv.pax[pr] = i; dv.ppart[pr] = part; dv.pn[pr] = order; dv.poff[pr] = off; dv.plam[pr] = lam0;
        };
        if (sym) {
            const int ns = (n + 1) / 2, nd = n / 2;
            add(1, ns, 0, 0);
            add(2, nd, (int64_t)ns * ns, ns);
        } else {
            add(0, n, 0, 0);
        }
    }
    return GPIMHIP_OK;
}

// K_i at the lengthscales in h->theta and its eigen-decomposition (Qt, lam), continued from the rotations in Vr
// (kron_cold_start() resets them), for every axis of the set
int kron_eig_axes(gpimhip_ctx* h, const KronAxes& ax, const ThetaDev* th) {
    const KronDev& dv = ax.dev;
    if (!th) th = h->theta;
    int nmax = 1, pmax = 1;
    for (int i = 0; i < ax.d; ++i) nmax = std::max(nmax, ax.n[i]);
    for (int pr = 0; pr < dv.nprob; ++pr) pmax = std::max(pmax, dv.pn[pr]);
    hipLaunchKernelGGL(kron_axis_kernel, dim3((unsigned)(((int64_t)nmax * nmax + 255) / 256), ax.d), dim3(256), 0, h->stream,
                       dv, th);
    hipLaunchKernelGGL(kron_reduce_kernel, dim3((unsigned)(((int64_t)pmax * pmax + 255) / 256), dv.nprob), dim3(256), 0,
                       h->stream, dv);
    for (int pr = 0; pr < dv.nprob; ++pr) {      // W = V * (matrix of the problem)
        const int64_t o = dv.moff[dv.pax[pr]] + dv.poff[pr];
        const int np_ = dv.pn[pr];
        GP_TRY(modeprod(h, dv.Tt + o, dv.W + o, dv.Vr + o, np_, np_, np_, 0, 0, 1, np_));
    }
    if (pmax <= 64) hipLaunchKernelGGL((kron_eigh_kernel<1, 4>), dim3(dv.nprob), dim3(EIGH_WAVES * 64), 0, h->stream, dv);
    else if (pmax <= 128) hipLaunchKernelGGL((kron_eigh_kernel<2, 4>), dim3(dv.nprob), dim3(EIGH_WAVES * 64), 0, h->stream, dv);
    else if (pmax <= 256) hipLaunchKernelGGL((kron_eigh_kernel<4, 2>), dim3(dv.nprob), dim3(EIGH_WAVES * 64), 0, h->stream, dv);
    else if (pmax <= 512) hipLaunchKernelGGL((kron_eigh_kernel<8, 1>), dim3(dv.nprob), dim3(EIGH_WAVES * 64), 0, h->stream, dv);
    else hipLaunchKernelGGL((kron_eigh_kernel<0, 1>), dim3(dv.nprob), dim3(EIGH_WAVES * 64), 0, h->stream, dv);
    hipLaunchKernelGGL(kron_assemble_kernel, dim3((unsigned)(((int64_t)pmax * nmax + 255) / 256), dv.nprob), dim3(256), 0,
                       h->stream, dv);
    HIP_TRY(hipGetLastError());
    return GPIMHIP_OK;
}

// M_i = Q_i^T E_i Q_i  (two mode products on the n_i x n_i "tensor") and its diagonal
int kron_grad_matrices(gpimhip_ctx* h, const KronAxes& ax) {
    const KronDev& dv = ax.dev;
    int nmax = 1;
    for (int i = 0; i < ax.d; ++i) {
        const int n = ax.n[i];
        nmax = std::max(nmax, n);
        GP_TRY(modeprod(h, dv.E + dv.moff[i], dv.Tt + dv.moff[i], dv.Qt + dv.moff[i], n, n, n, 0, 0, 1, n));
        GP_TRY(modeprod(h, dv.Tt + dv.moff[i], dv.Mm + dv.moff[i], dv.Qt + dv.moff[i], n, n, n, 0, 0, n, 1));
    }
    hipLaunchKernelGGL(kron_mdiag_kernel, dim3((nmax + 63) / 64, ax.d), dim3(64), 0, h->stream, dv);
    HIP_TRY(hipGetLastError());
    return GPIMHIP_OK;
}

int kron_root_rows(gpimhip_ctx* h, const KronDev& dv, int ax, const int32_t* idx, int rows, double* out) {
    hipLaunchKernelGGL(kron_root_rows_kernel, dim3((unsigned)(((int64_t)rows * dv.n[ax] + 255) / 256)), dim3(256), 0, h->stream, dv,
                       ax, idx, rows, out);
    HIP_TRY(hipGetLastError());
    return GPIMHIP_OK;
}

int kron_axes_load(gpimhip_ctx* h, KronAxes& a, int d, const int32_t* n, const double* coords_dev, bool grad) {
    GP_TRY(kron_axes_ensure(h, a, d, n, grad));
    HIP_TRY(hipMemcpyAsync(const_cast<double*>(a.dev.coords), coords_dev, (size_t)a.sum_n * sizeof(double), hipMemcpyDeviceToDevice,
                           h->stream));
    GP_TRY(kron_plan_problems(h, a));
    return kron_cold_start(h, a.dev);
}

int kron_union_check(const char* entry, int d, const int32_t* n, const int32_t* n_test, const int32_t* n_union,
                     const int32_t* idx_train, const int32_t* idx_test, KronUnion* out) {
    auto bad = [&](const char* what) {
        gpim_set_error(std::string(entry) + ": " + what);
        return GPIMHIP_E_BADARG;
    };
    KronUnion un = {true, 0, 0, 0, 0, 0, 1};
    for (int i = 0, oc = 0, ot = 0; i < d; ++i) {
        if (n[i] < 1 || n_test[i] < 1) return bad("every axis of the training and of the test grid needs at least one coordinate");
        if (n_union[i] > 4096) {
            char msg[200];
            snprintf(msg, sizeof(msg), "the union of the training and the test coordinates of axis %d has %d entries; the "
                     "eigen-solver takes at most 4096", i, (int)n_union[i]);
            return bad(msg);
        }
        if (n_union[i] < n[i] || (int64_t)n_union[i] > (int64_t)n[i] + n_test[i])
            return bad("n_union[i] must lie between n[i] and n[i] + n_test[i]");
        for (int a = 0; a < n[i]; ++a) {
            const int32_t v = idx_train[oc + a];
            if (v < 0 || v >= n_union[i]) return bad("idx_train outside its union axis");
            un.shared = un.shared && v == a;
        }
        for (int a = 0; a < n_test[i]; ++a) {
            const int32_t v = idx_test[ot + a];
            if (v < 0 || v >= n_union[i]) return bad("idx_test outside its union axis");
        }
        un.shared = un.shared && n_union[i] == n[i];
        oc += n[i]; ot += n_test[i];
        un.sum_n += n[i]; un.sum_m += n_test[i]; un.sum_u += n_union[i];
        un.sum_nu += (int64_t)n[i] * n_union[i];
        un.sum_mu += (int64_t)n_test[i] * n_union[i];
        un.U *= n_union[i];
    }
    *out = un;
    return GPIMHIP_OK;
}

int kron_union_roots(gpimhip_ctx* h, const KronDev& du, int d, const int32_t* n, const int32_t* n_test, const int32_t* ic,
                     const int32_t* it, double* RX, double* RT, const double** rx, const double** rt) {
    for (int i = 0; i < d; ++i) {
        GP_TRY(kron_root_rows(h, du, i, ic, n[i], RX));
        GP_TRY(kron_root_rows(h, du, i, it, n_test[i], RT));
        rx[i] = RX; rt[i] = RT;
        RX += (int64_t)n[i] * du.n[i]; RT += (int64_t)n_test[i] * du.n[i];
        ic += n[i]; it += n_test[i];
    }
    return GPIMHIP_OK;
}

void kron_axes_free(gpimhip_ctx* h, KronAxes& a) {
    a.arena.release(h);
    a.d = 0;
}
int kron_cross(gpimhip_ctx* h, const KronDev& dv, const ThetaDev* th, const double* tcoords, int toff, int mi, int ax, double* Ks) {
    const int64_t cnt = (int64_t)mi * dv.n[ax];
    hipLaunchKernelGGL(kron_cross_kernel, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, h->stream, dv, th, tcoords, toff, mi, ax,
                       Ks);
    HIP_TRY(hipGetLastError());
    return GPIMHIP_OK;
}

// theta(u), the eigen-decomposition of the training axes, y~
static int kron_decompose(gpimhip_ctx* h, KronWs& w, const gpimhip_model_t* m, const double* u, const double* y) {
    const KronDev& dv = w.tr.dev;
    GP_TRY(launch_theta(h, m, u));
    GP_TRY(kron_eig_axes(h, w.tr));
    // y~ = (Q_1^T (x) ... (x) Q_d^T) y
    const double* mats[KMAXD]; int ld[KMAXD];
    for (int i = 0; i < w.d; ++i) { mats[i] = dv.Qt + dv.moff[i]; ld[i] = w.n[i]; }
    double* res;
    GP_TRY(tensor_apply(h, w.d, w.n, w.n, mats, ld, 0, 0, y, w.t1, w.t2, &res));
    HIP_TRY(hipMemcpyAsync(w.yt, res, (size_t)w.N * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
    return GPIMHIP_OK;
}

static int kron_loss_grad(gpimhip_ctx* h, KronWs& w, const gpimhip_model_t* m, const double* y, double* u, int do_adam,
                          double* loss_out, double* grad_out, const FinalizeIter* it) {
    const KronDev& dv = w.tr.dev;
    GP_TRY(kron_decompose(h, w, m, u, y));
    GP_TRY(kron_grad_matrices(h, w.tr));
    hipLaunchKernelGGL(kron_dvec_kernel, dim3(w.nblk), dim3(256), 0, h->stream, dv, h->theta, w.yt, w.at, w.part);
    for (int i = 0; i < w.d; ++i) {
        int64_t pre = 1, post = 1;
        for (int k = 0; k < i; ++k) pre *= w.n[k];
        for (int k = i + 1; k < w.d; ++k) post *= w.n[k];
        GP_TRY(modeprod(h, w.at, w.Z + (int64_t)i * w.N, dv.Mm + dv.moff[i], w.n[i], w.n[i], w.n[i], 0, 0, pre, post));
    }
    hipLaunchKernelGGL(kron_quad_kernel, dim3(w.nblk), dim3(256), 0, h->stream, dv, w.at, w.Z, w.part);
    FinalizeIter fi{nullptr, nullptr, 0, nullptr, nullptr};
    if (it) fi = *it;
    hipLaunchKernelGGL(kron_finalize_kernel, dim3(1), dim3(256), 0, h->stream, *m, dv, w.nblk, w.part, h->theta, u,
                       h->adam_m, h->adam_v, do_adam, loss_out, grad_out, fi, h->info);
    HIP_TRY(hipGetLastError());
    return GPIMHIP_OK;
}

static int kron_prepare(gpimhip_ctx* h, const gpimhip_model_t* m, int32_t d, const int32_t* n, const double* axes,
                        KronWs** w) {
    GP_TRY(check_model(m));
    if (m->kernel != GPIMHIP_KERNEL_RBF) {
        gpim_set_error("structured (Kronecker) solver: only the RBF kernel factorises over the grid axes");
        return GPIMHIP_E_BADARG;
    }
    if (d != m->dim || !n || !axes) return GPIMHIP_E_BADARG;
    for (int i = 0; i < d; ++i)
        if (n[i] < 1 || n[i] > 4096) return GPIMHIP_E_BADARG;
    HIP_TRY(hipSetDevice(h->device));
    h->nbatch = 1;
    GP_TRY(ws_ensure(h, 1));                   // theta, Adam state, iteration counter
    GP_TRY(kron_ensure(h, d, n, w));
    HIP_TRY(hipMemsetAsync(h->info, 0, sizeof(int32_t), h->stream));
    return kron_axes_load(h, (*w)->tr, d, n, axes, true);
}

// the prediction workspace for the test grid of the orders n_test[] and its coordinates
static int kron_predict_ws(gpimhip_ctx* h, KronWs& w, int d, const int32_t* n_test, const double* axes_test) {
    int64_t M = 1, sum_m = 0, sum_mn = 0, pmax = w.N;
    {
        int64_t cur = w.N;
        for (int i = 0; i < d; ++i) {
            if (n_test[i] < 1) return GPIMHIP_E_BADARG;
            M *= n_test[i]; sum_m += n_test[i]; sum_mn += (int64_t)n_test[i] * w.n[i];
            cur = cur / w.n[i] * n_test[i];
            pmax = std::max(pmax, cur);
        }
    }
    bool same = w.parena && w.M == M && w.pmax == pmax;
    for (int i = 0; i < d && same; ++i) same = w.m[i] == n_test[i];
    if (!same) {
        HIP_TRY(hipStreamSynchronize(h->stream));
        w.parena.release(h);
        const int64_t count = sum_m + 2 * sum_mn + 2 * pmax + 64;
        GP_TRY(w.parena.alloc(h, count, "hipMalloc failed (structured-GP prediction workspace)"));
        Carve c(w.parena);
        w.tcoords = c.take(sum_m); w.Ks = c.take(sum_mn); w.Bs = c.take(sum_mn); w.p1 = c.take(pmax); w.p2 = c.take(pmax);
        int64_t ko = 0;
        for (int i = 0; i < KMAXD; ++i) {
            w.m[i] = i < d ? n_test[i] : 1;
            w.koff[i] = ko;
            if (i < d) ko += (int64_t)n_test[i] * w.n[i];
        }
        w.M = M; w.pmax = pmax;
    }
    HIP_TRY(hipMemcpyAsync(w.tcoords, axes_test, (size_t)sum_m * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
    return GPIMHIP_OK;
}

// cross-covariances per axis and B_i = Ks_i Q_i
static int kron_cross_factors(gpimhip_ctx* h, KronWs& w) {
    const KronDev& dv = w.tr.dev;
    int toff = 0;
    for (int i = 0; i < w.d; ++i) {
        GP_TRY(kron_cross(h, dv, h->theta, w.tcoords, toff, w.m[i], i, w.Ks + w.koff[i]));
        GP_TRY(modeprod(h, w.Ks + w.koff[i], w.Bs + w.koff[i], dv.Qt + dv.moff[i], w.n[i], w.n[i], w.n[i], 0, 0, w.m[i], 1));
        toff += w.m[i];
    }
    return GPIMHIP_OK;
}

// mean_out = ((x) B_i) alpha~, the posterior mean before its factor s2 (B_i = Ks_i Q_i maps eigen-coordinates straight to
// test points); mats / ld: the B_i as tensor_apply takes them.  The mean of a prediction and of a draw
static int kron_mean_raw(gpimhip_ctx* h, KronWs& w, const double** mats, int* ld, double* mean_out) {
    for (int i = 0; i < w.d; ++i) { mats[i] = w.Bs + w.koff[i]; ld[i] = w.n[i]; }
    double* res;
    GP_TRY(tensor_apply(h, w.d, w.n, w.m, mats, ld, 0, 0, w.at, w.p1, w.p2, &res));
    HIP_TRY(hipMemcpyAsync(mean_out, res, (size_t)w.M * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
    return GPIMHIP_OK;
}

// the workspace of gpimhip_sample_kron: the gathered root rows, the index maps, zeta of every draw and two buffers of
// S * smax doubles for the mode products (smax: the largest tensor any of the four chains U -> n, n -> n, n -> m, U -> m
// passes through)
static int kron_sample_ws(gpimhip_ctx* h, KronWs& w, int d, const int32_t* nu, const KronUnion& un, int64_t S) {
    const int32_t* lo[2] = {w.n, w.m};
    int64_t smax = std::max(w.N, w.M);
    for (int c = 0; c < 2; ++c) {
        int64_t cur = un.U;
        for (int i = 0; i < d; ++i) { cur = cur / nu[i] * lo[c][i]; smax = std::max(smax, cur); }
    }
    {
        int64_t cur = w.N;
        for (int i = 0; i < d; ++i) { cur = cur / w.n[i] * w.m[i]; smax = std::max(smax, cur); }
    }
    int64_t key[3 + 3 * KMAXD] = {S, d, smax};
    for (int i = 0; i < d; ++i) { key[3 + i] = nu[i]; key[3 + KMAXD + i] = w.n[i]; key[3 + 2 * KMAXD + i] = w.m[i]; }
    if (w.sarena && memcmp(key, w.s_key, sizeof(key)) == 0) return GPIMHIP_OK;
    HIP_TRY(hipStreamSynchronize(h->stream));
    w.sarena.release(h);
    const int64_t count = un.sum_nu + un.sum_mu + (un.sum_n + un.sum_m + 4) / 2 + S * un.U + 2 * S * smax + 32;
    GP_TRY(w.sarena.alloc(h, count, "hipMalloc failed (structured-GP posterior-draw workspace)"));
    Carve c(w.sarena);
    w.RG = c.take(un.sum_nu); w.RT = c.take(un.sum_mu);
    w.ic = c.take<int32_t>((un.sum_n + 1) / 2); w.it = c.take<int32_t>((un.sum_m + 1) / 2);
    w.Zc = c.take(S * un.U); w.sa = c.take(S * smax); w.sb = c.take(S * smax);
    memcpy(w.s_key, key, sizeof(key));
    return GPIMHIP_OK;
}

extern "C" {

int gpimhip_kron_nll_grad(gpimhip_handle h, const gpimhip_model_t* m, int32_t d, const int32_t* n, const double* axes,
                          const double* y, const double* u, double* loss_out, double* grad_out) {
    if (!h || !m || !y || !u) return GPIMHIP_E_BADARG;
    KronWs* w;
    GP_TRY(kron_prepare(h, m, d, n, axes, &w));
    GP_TRY(kron_loss_grad(h, *w, m, y, const_cast<double*>(u), 0, loss_out, grad_out, nullptr));
    return finish_and_check(h);
}

int gpimhip_fit_kron(gpimhip_handle h, const gpimhip_model_t* m, int32_t d, const int32_t* n, const double* axes,
                     const double* y, double* u_inout, double lr, int32_t T, double* hist_out, double* loss_out) {
    if (!h || !m || !y || !u_inout || T < 0) return GPIMHIP_E_BADARG;
    KronWs* w;
    GP_TRY(kron_prepare(h, m, d, n, axes, &w));
    GP_TRY(fit_prologue(h, lr, T, h->adam_m, h->adam_v, MAXP * sizeof(double), h->iter));
    if (T == 0) return GPIMHIP_OK;
    const FinalizeIter it{h->iter, h->bc, T, hist_out, loss_out};
    // every iteration is the same ~4d + 8 small launches
    return run_fit_iterations(h, T, FIT_LOOP_PLAIN,
                              [&] { return kron_loss_grad(h, *w, m, y, u_inout, 1, nullptr, nullptr, &it); });
}

int gpimhip_predict_kron(gpimhip_handle h, const gpimhip_model_t* m, int32_t d, const int32_t* n, const double* axes,
                         const double* y, const double* u, const int32_t* n_test, const double* axes_test,
                         double* mean_out, double* var_out) {
    if (!h || !m || !y || !u || !n_test || !axes_test || !mean_out || !var_out) return GPIMHIP_E_BADARG;
    KronWs* wp;
    GP_TRY(kron_prepare(h, m, d, n, axes, &wp));
    KronWs& w = *wp;
    const KronDev& dv = w.tr.dev;
    GP_TRY(kron_predict_ws(h, w, d, n_test, axes_test));
    const int64_t M = w.M;
    GP_TRY(kron_decompose(h, w, m, u, y));
    hipLaunchKernelGGL(kron_dvec_kernel, dim3(w.nblk), dim3(256), 0, h->stream, dv, h->theta, w.yt, w.at, w.part);
    GP_TRY(kron_cross_factors(h, w));
    // mean = s2 * ((x) B_i) alpha~
    const double* mats[KMAXD]; int ld[KMAXD];
    GP_TRY(kron_mean_raw(h, w, mats, ld, mean_out));
    double* res;
    // var = s2 - s2^2 * ((x) B_i o B_i) (1 / D)
    hipLaunchKernelGGL(kron_invd_kernel, dim3((unsigned)((w.N + 255) / 256)), dim3(256), 0, h->stream, dv, h->theta, w.t1);
    GP_TRY(tensor_apply(h, d, w.n, w.m, mats, ld, 0, 1, w.t1, w.p1, w.p2, &res));
    hipLaunchKernelGGL(kron_post_kernel, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, h->stream, mean_out, res, M,
                       h->theta, mean_out, var_out);
    HIP_TRY(hipGetLastError());
    return finish_and_check(h);
}

// Leave-one-out cross-validation in the eigenbasis: alpha = Q (y~ / D) and diag(S^-1) = ((x) Q_i o Q_i)
// (1 / D), the mode products of the squared eigenvector matrices with what kron_invd_kernel leaves; then the dense
// model's finisher (predict.hip: loo_finish_kernel).  alpha waits in w.Z while 1 / D takes the place of alpha~.
int gpimhip_loo_kron(gpimhip_handle h, const gpimhip_model_t* m, int32_t d, const int32_t* n, const double* axes,
                     const double* y, const double* u, double* mean_out, double* var_out, double* score_out) {
    if (!h || !m || !y || !u || !mean_out || !var_out || !score_out) return GPIMHIP_E_BADARG;
    FP64_ONLY(h);
    KronWs* wp;
    GP_TRY(kron_prepare(h, m, d, n, axes, &wp));
    KronWs& w = *wp;
    const KronDev& dv = w.tr.dev;
    GP_TRY(kron_decompose(h, w, m, u, y));
    hipLaunchKernelGGL(kron_dvec_kernel, dim3(w.nblk), dim3(256), 0, h->stream, dv, h->theta, w.yt, w.at, w.part);
    // Qt holds Q_i^T: transposed, the mode products map eigen-coordinates back to grid points
    const double* mats[KMAXD]; int ld[KMAXD];
    for (int i = 0; i < w.d; ++i) { mats[i] = dv.Qt + dv.moff[i]; ld[i] = w.n[i]; }
    double* res;
    GP_TRY(tensor_apply(h, w.d, w.n, w.n, mats, ld, 1, 0, w.at, w.t1, w.t2, &res));
    HIP_TRY(hipMemcpyAsync(w.Z, res, (size_t)w.N * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
    hipLaunchKernelGGL(kron_invd_kernel, dim3((unsigned)((w.N + 255) / 256)), dim3(256), 0, h->stream, dv, h->theta, w.at);
    GP_TRY(tensor_apply(h, w.d, w.n, w.n, mats, ld, 1, 1, w.at, w.t1, w.t2, &res));
    const LooSrc s{y, res, 1, INT_MAX, w.N, w.Z, 0, nullptr, nullptr, nullptr, 0};
    GP_TRY(launch_loo_finish(h, s, w.N, h->theta, w.part, mean_out, var_out, score_out));
    return finish_and_check(h);
}

// Joint posterior draws on the product test grid by Matheron's rule with every factor a Kronecker product (DESIGN.md
// section 21).  Stage timers: 0 the union axes' eigen-decomposition, 1 the training axes' (with y~), 2 the prior's root
// rows and mode products, 3 the update's factors and mode products (the mean's among them), 5 the epilogue.
// One call: the workspace, the union axes (the training axes where they serve), the caller's z (rows of zw doubles: zeta of
// PU entries | z_e | z_n) and where every union axis' root rows at the training / test coordinates start
struct KronDraw {
    KronWs& w; const KronAxes& ua;
    const double* z; int64_t PU, zw, S;
    const double *rg[KMAXD], *rt[KMAXD];
};
// the prior on the training grid: *gG = g_G / sqrt(s2) = ((x) R_i[ic_i, :]) zeta
static int kron_draw_prior_train(gpimhip_ctx* h, KronDraw& D, double** gG) {
    KronWs& w = D.w;
    StageTimer t(h, 2);
    GP_TRY(kron_union_roots(h, D.ua.dev, w.d, w.n, w.m, w.ic, w.it, w.RG, w.RT, D.rg, D.rt));
    hipLaunchKernelGGL(kron_zeta_kernel, dim3((unsigned)((D.S * D.PU + 255) / 256)), dim3(256), 0, h->stream, D.z, D.zw, D.PU,
                       D.S * D.PU, w.Zc);
    HIP_TRY(hipGetLastError());
    return tensor_apply(h, w.d, D.ua.n, w.n, D.rg, D.ua.n, 0, 0, w.Zc, w.sa, w.sb, gG, D.S);
}
// the update: out <- ((x) Ks_i Q_i) D^-1 ((x) Q_i^T) (y - sqrt(s2) g_G - sqrt(sigma) z_e), and the mean as predict computes it
static int kron_draw_update(gpimhip_ctx* h, KronDraw& D, const double* y, double* gG, double* mean_out, double* out) {
    KronWs& w = D.w;
    const KronDev& dv = w.tr.dev;
    const int64_t N = w.N, S = D.S;
    const double* mats[KMAXD]; int ld[KMAXD];
    double *res, *upd;
    StageTimer t(h, 3);
    GP_TRY(kron_cross_factors(h, w));
    hipLaunchKernelGGL(kron_resid_kernel, dim3((unsigned)((S * N + 255) / 256)), dim3(256), 0, h->stream, y, D.z + D.PU, D.zw, N,
                       S * N, h->theta, gG);
    double* other = gG == w.sa ? w.sb : w.sa;
    for (int i = 0; i < w.d; ++i) { mats[i] = dv.Qt + dv.moff[i]; ld[i] = w.n[i]; }
    GP_TRY(tensor_apply(h, w.d, w.n, w.n, mats, ld, 0, 0, gG, other, gG, &res, S));
    hipLaunchKernelGGL(kron_dscale_kernel, dim3((unsigned)((N + 255) / 256), (unsigned)std::min<int64_t>(S, 64)), dim3(256), 0,
                       h->stream, dv, h->theta, S, res);
    HIP_TRY(hipGetLastError());
    other = res == w.sa ? w.sb : w.sa;
    for (int i = 0; i < w.d; ++i) { mats[i] = w.Bs + w.koff[i]; ld[i] = w.n[i]; }
    GP_TRY(tensor_apply(h, w.d, w.n, w.m, mats, ld, 0, 0, res, other, res, &upd, S));
    HIP_TRY(hipMemcpyAsync(out, upd, (size_t)(S * w.M) * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
    return kron_mean_raw(h, w, mats, ld, mean_out);
}
// the prior on the test grid, from the same zeta
static int kron_draw_prior_test(gpimhip_ctx* h, KronDraw& D, double** gs) {
    KronWs& w = D.w;
    StageTimer t(h, 2);
    return tensor_apply(h, w.d, D.ua.n, w.m, D.rt, D.ua.n, 0, 0, w.Zc, w.sa, w.sb, gs, D.S);
}

int gpimhip_sample_kron(gpimhip_handle h, const gpimhip_model_t* m, int32_t d, const int32_t* n, const double* axes,
                        const double* y, const double* u, const int32_t* n_test, const double* axes_test,
                        const int32_t* n_union, const double* axes_union, const int32_t* idx_train, const int32_t* idx_test,
                        const double* z, int32_t S, int32_t noiseless, double jitter, double* mean_out, double* out) {
    auto bad = [](const char* what) { gpim_set_error(what); return (int)GPIMHIP_E_BADARG; };
    if (!h || !m || !y || !u || !n || !n_test || !axes_test || !n_union || !axes_union || !idx_train || !idx_test || !z ||
        !mean_out || !out)
        return bad("gpimhip_sample_kron: a null argument (every pointer of the entry point is required)");
    if (S < 1 || !(jitter >= 0.0) || !(jitter < HUGE_VAL)) return bad("gpimhip_sample_kron: needs S >= 1 and a finite jitter >= 0");
    if (d < 1 || d > KMAXD) return bad("gpimhip_sample_kron: d must be between 1 and 4");
    KronUnion un;
    GP_TRY(kron_union_check("gpimhip_sample_kron", d, n, n_test, n_union, idx_train, idx_test, &un));
    KronWs* wp;
    GP_TRY(kron_prepare(h, m, d, n, axes, &wp));
    KronWs& w = *wp;
    GP_TRY(kron_predict_ws(h, w, d, n_test, axes_test));
    if (!un.shared) GP_TRY(kron_axes_load(h, w.un, d, n_union, axes_union, false));
    GP_TRY(kron_sample_ws(h, w, d, n_union, un, S));
    HIP_TRY(hipMemcpyAsync(w.ic, idx_train, (size_t)un.sum_n * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(w.it, idx_test, (size_t)un.sum_m * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));          // the host arrays are the caller's
    const int64_t N = w.N, M = w.M;
    KronDraw D = {w, un.shared ? w.tr : w.un, z, un.U, un.U + N + M, S, {}, {}};
    {
        StageTimer t(h, 1);
        GP_TRY(kron_decompose(h, w, m, u, y));
        hipLaunchKernelGGL(kron_dvec_kernel, dim3(w.nblk), dim3(256), 0, h->stream, w.tr.dev, h->theta, w.yt, w.at, w.part);
    }
    if (!un.shared) {
        StageTimer t(h, 0);
        GP_TRY(kron_eig_axes(h, w.un));
    }
    double *gG, *gs;
    GP_TRY(kron_draw_prior_train(h, D, &gG));
    GP_TRY(kron_draw_update(h, D, y, gG, mean_out, out));
    GP_TRY(kron_draw_prior_test(h, D, &gs));
    {
        StageTimer t(h, 5);
        hipLaunchKernelGGL(kron_draw_kernel, dim3((unsigned)((S * M + 255) / 256)), dim3(256), 0, h->stream, gs, z + D.PU + N, D.zw,
                           M, (int64_t)S * M, h->theta, noiseless, jitter, mean_out, out);
        HIP_TRY(hipGetLastError());
    }
    return finish_and_check(h);
}

static int kron_eigh_bad(const char* what) {
    gpim_set_error(std::string("gpimhip_kron_eigh: ") + what);
    return GPIMHIP_E_BADARG;
}

// DIAGNOSTIC (tests/test_gpu_kron_eigh.py): the axis eigen-decomposition by the product's own chain -- kron_axes_ensure,
// kron_plan_problems, kron_cold_start (unless warm), kron_eig_axes -- on an axis set of its own, and what the sweep loop of
// every eigen-problem did.
int gpimhip_kron_eigh(gpimhip_handle h, int32_t d, const int32_t* n, const double* axes, const double* ls, int32_t warm,
                      double* lam_out, double* Qt_out, int32_t* nprob_out, int32_t* plan_out, double* rot_out,
                      int32_t* cap_out) {
    if (!h) return kron_eigh_bad("null handle");
    FP64_ONLY(h);
    if (!n || !axes || !ls || !lam_out || !Qt_out || !nprob_out || !plan_out || !rot_out) return kron_eigh_bad("null argument");
    if (d < 1 || d > KMAXD) return kron_eigh_bad("d must be between 1 and 4");
    ThetaDev th;
    memset(&th, 0, sizeof(th));
    th.var = 1.0;
    for (int i = 0; i < KMAXD; ++i) th.ls[i] = th.inv_ls[i] = 1.0;
    for (int i = 0; i < d; ++i) {
        if (n[i] < 1 || n[i] > 4096) return kron_eigh_bad("every axis needs between 1 and 4096 points");
        if (!(ls[i] > 0.0) || !(ls[i] < HUGE_VAL)) return kron_eigh_bad("lengthscales must be positive and finite");
        th.ls[i] = ls[i]; th.inv_ls[i] = 1.0 / ls[i];
    }
    HIP_TRY(hipSetDevice(h->device));
    GP_TRY(ws_ensure(h, 1));                   // theta
    if (!h->kron) h->kron = new KronWs();
    KronWs& w = *static_cast<KronWs*>(h->kron);
    KronAxes& ax = w.dg;
    bool same = w.dg_ready && ax.arena && ax.d == d;
    for (int i = 0; i < d && same; ++i) same = ax.n[i] == n[i];
    if (warm && !same) return kron_eigh_bad("warm = 1 continues the previous call: it needs one, on axes of the same orders");
    w.dg_ready = false;
    KronDev prev;
    memset(&prev, 0, sizeof(prev));
    if (warm) prev = ax.dev;
    GP_TRY(kron_axes_ensure(h, ax, d, n, false));
    HIP_TRY(hipMemcpyAsync(const_cast<double*>(ax.dev.coords), axes, (size_t)ax.sum_n * sizeof(double), hipMemcpyDeviceToDevice,
                           h->stream));
    GP_TRY(kron_plan_problems(h, ax));
    const KronDev& dv = ax.dev;
    if (warm) {
        bool plan_same = prev.nprob == dv.nprob;
        for (int pr = 0; pr < dv.nprob && plan_same; ++pr) plan_same = prev.pn[pr] == dv.pn[pr] && prev.pax[pr] == dv.pax[pr];
        if (!plan_same) return kron_eigh_bad("warm = 1 on coordinates that split into other eigen-problems than the previous call's");
    } else {
        GP_TRY(kron_cold_start(h, dv));
    }
    HIP_TRY(hipMemcpyAsync(h->theta.p, &th, sizeof(th), hipMemcpyHostToDevice, h->stream));
    GP_TRY(kron_eig_axes(h, ax, h->theta));
    double stat[2 * 2 * KMAXD];
    HIP_TRY(hipMemcpyAsync(stat, dv.stat, sizeof(stat), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipMemcpyAsync(lam_out, dv.lam, (size_t)ax.sum_n * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(Qt_out, dv.Qt, (size_t)ax.sum_n2 * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    *nprob_out = dv.nprob;
    for (int pr = 0; pr < dv.nprob; ++pr) {
        plan_out[4 * pr] = dv.pax[pr]; plan_out[4 * pr + 1] = dv.ppart[pr]; plan_out[4 * pr + 2] = dv.pn[pr];
        plan_out[4 * pr + 3] = (int32_t)stat[2 * pr];
        rot_out[pr] = stat[2 * pr + 1];
    }
    if (cap_out) *cap_out = EIGH_MAX_SWEEPS;
    w.dg_ready = true;
    return GPIMHIP_OK;
}

}  // extern "C"
