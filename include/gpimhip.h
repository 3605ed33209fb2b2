/*
 * gpimhip.h -- C ABI of libgpimhip.so, the MI355X (gfx950) engine behind
 * gpim_amd.reconstructor / gpim_amd.boptimizer.
 *
 * The reference (ziatdinovmax/GPim, /root/reference) has no native boundary: its hot
 * path is Python calling pyro.contrib.gp / torch.  Each entry point below replaces the
 * group of third-party calls made at the cited reference call site; the Python host
 * code in gpim_amd/ binds them with ctypes.
 *
 * Conventions
 *   - every data pointer is a DEVICE pointer (HBM) borrowed for the duration of the
 *     call; outputs are caller-allocated; the library owns only its workspace.
 *   - all work is enqueued on the handle's HIP stream; calls return without
 *     synchronising unless stated.  Nothing here allocates per call once the
 *     workspace for a problem size exists.
 *   - matrices are row-major doubles; "lower" means the i >= j part is meaningful.
 *   - return value: 0 = ok, <0 = error (see GPIMHIP_E_*), message via
 *     gpimhip_last_error().  Non-positive-definite detection is asynchronous: the
 *     factorisation records the first failing column in a device word that
 *     gpimhip_fit_exact / gpimhip_predict_exact read back at their final sync and
 *     report as GPIMHIP_E_NOT_PD (torch.linalg.cholesky raises at gpr.py:192,248).  Training loops stop
 *     updating on the device at the failing iteration and stop being enqueued a bounded number of
 *     iterations later (see gpimhip_fit_completed).
 *   - parameter vector u (unconstrained, the thing Adam updates), length
 *     P = 2 + n_ls (+1 for RationalQuadratic):
 *         u[0]            variance      sigma^2 = amp_lo + (amp_hi-amp_lo)*sigmoid(u)
 *         u[1..n_ls]      lengthscale   l_k     = ls_lo_k + (ls_hi_k-ls_lo_k)*sigmoid(u)
 *         u[1+n_ls]       noise         s_n^2   = exp(u)
 *         u[2+n_ls]       scale_mixture alpha   = exp(u)      (RationalQuadratic only)
 *     (pyro_kernels.py:81-94 Uniform priors -> interval constraints)
 *   - three regimes behind gpimhip_fit_exact, same arithmetic: N <= 128 one fused launch per
 *     training (one workgroup, K/L/L^-1 resident in LDS); mid N the blocked path with one iteration
 *     captured in a hipGraph and replayed; N >= 6144 the blocked path with a look-ahead panel
 *     stream (side streams are created on first use).  Environment switches for A/B testing:
 *     GPIMHIP_NO_SMALLN, GPIMHIP_NO_GRAPH, GPIMHIP_NO_CUMASK (any value disables the respective
 *     mechanism), GPIMHIP_LOOKAHEAD_MIN_PANELS, GPIMHIP_RESERVED_CUS.
 */
#ifndef GPIMHIP_H
#define GPIMHIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GPIMHIP_OK            0
#define GPIMHIP_E_BADARG     -1
#define GPIMHIP_E_HIP        -2
#define GPIMHIP_E_NOT_PD     -3
#define GPIMHIP_E_NOMEM      -4

#define GPIMHIP_KERNEL_RBF       0
#define GPIMHIP_KERNEL_MATERN52  1
#define GPIMHIP_KERNEL_RQ        2

#define GPIMHIP_ACQ_CB   0
#define GPIMHIP_ACQ_EI   1
#define GPIMHIP_ACQ_POI  2

#define GPIMHIP_MAX_DIM  4
#define GPIMHIP_MAX_PARAMS 8

typedef struct gpimhip_ctx* gpimhip_handle;

/* Model description: kernel family + parameterisation.
 * Replaces gpim/kernels/pyro_kernels.py:14-96 (get_kernel) and the jitter argument of
 * gp.models.GPRegression at gpim/gpreg/gpr.py:141-144. */
typedef struct {
    int32_t kernel;                     /* GPIMHIP_KERNEL_*                                  */
    int32_t dim;                        /* d, 1..4                                           */
    int32_t n_ls;                       /* 1 (isotropic) or dim                              */
    int32_t reserved;
    double  amp_lo, amp_hi;             /* variance prior bounds (default 1e-4, 10)          */
    double  ls_lo[GPIMHIP_MAX_DIM];     /* lengthscale prior bounds                          */
    double  ls_hi[GPIMHIP_MAX_DIM];
    double  jitter;                     /* added to diag(K) with the noise (gpr.py:141)      */
} gpimhip_model_t;

/* ---- lifetime ------------------------------------------------------------------- */
/* hip_stream: the hipStream_t every call is enqueued on; NULL selects the device's default
 * (null) stream, so work is ordered with the caller's own default-stream work. */
int  gpimhip_create(gpimhip_handle* out, int device, void* hip_stream);
int  gpimhip_destroy(gpimhip_handle h);
const char* gpimhip_last_error(void);
int  gpimhip_version(void);
/* bytes of device workspace currently held by the handle */
int64_t gpimhip_workspace_bytes(gpimhip_handle h);

/* ---- operator-level entry points (parity hooks; each is also a stage of fit/predict) -- */

/* K = k(X, Z) (+ diag_add on the diagonal when Z == NULL, i.e. the symmetric case).
 * Replaces the Pyro kernel forward called from GPRegression.model/forward
 * (call sites gpim/gpreg/gpr.py:192,248; formulas SURVEY App. A.3).
 * theta (device, doubles): [sigma^2, l_0..l_{n_ls-1}, alpha_rq].  out: (N x M) row-major,
 * leading dimension ld >= M.  Symmetric case writes the full square. */
int gpimhip_kmat(gpimhip_handle h, const gpimhip_model_t* m,
                 const double* X, int64_t N, const double* Z, int64_t M,
                 const double* theta, double diag_add, double* out, int64_t ld);

/* Arithmetic of the exact-GP path (gpimhip_nll_grad, gpimhip_fit_exact*, gpimhip_predict_exact*,
 * gpimhip_acquire_exact): bits = 64 (default) or 32 = the reconstructor's precision='single'
 * (gpim/gpreg/gpr.py:104-113: float32 tensors end to end).  With 32 the N x N matrices (covariance, factor,
 * inverse, K* slab) are float and every O(N^3) product runs on v_mfma_f32_16x16x4_f32 (twice the fp64 matrix
 * rate, half the HBM bytes); diagonal blocks are factored in double and all O(N) vectors, reductions, the
 * loss, the gradient and Adam stay double (wider than the reference's float32, never narrower).  Inputs and
 * outputs of the C ABI remain double.  The fused trainer for N <= 128 computes in double on either setting.
 * Entry points outside that path (kmat, potrf, vfe, dist) require bits = 64.  Switching releases the workspace. */
int gpimhip_set_precision(gpimhip_handle h, int32_t bits);

/* In-place lower Cholesky of the n x n matrix A (row-major, ld), n any size >= 1;
 * the strict upper triangle is left untouched.  info (device int32): 0, or 1 + first
 * failing column.  Replaces torch.linalg.cholesky inside Pyro (gpr.py:192,248). */
int gpimhip_potrf(gpimhip_handle h, double* A, int64_t n, int64_t ld, int32_t* info);

/* loss (negative log marginal likelihood + prior constant) and d loss / d u at u.
 * Replaces Trace_ELBO().differentiable_loss + loss.backward() (gpr.py:186,192-193).
 * loss_out: 1 double, grad_out: P doubles (device). */
int gpimhip_nll_grad(gpimhip_handle h, const gpimhip_model_t* m,
                     const double* X, const double* y, int64_t N,
                     const double* u, double* loss_out, double* grad_out);

/* ---- the hot path ------------------------------------------------------------------ */

/* T Adam iterations on u, entirely on device (no host sync inside the loop).
 * Replaces the training loop reconstructor.train (gpr.py:185-199): fresh Adam state
 * (t=0, m=v=0), lr, betas (0.9, 0.999), eps 1e-8.
 *   u_inout   P doubles (device), updated in place
 *   hist_out  T x (P) doubles (device): constrained values AFTER each step, in the
 *             order [sigma^2, l_*, s_n^2(, alpha)]  (what gpr.py:195-197 appends)
 *   loss_out  T doubles (device) or NULL: loss evaluated BEFORE each step
 * Synchronises the stream once at the end; returns GPIMHIP_E_NOT_PD if any
 * factorisation failed (info of the first failure via gpimhip_last_error). */
int gpimhip_fit_exact(gpimhip_handle h, const gpimhip_model_t* m,
                      const double* X, const double* y, int64_t N,
                      double* u_inout, double lr, int32_t T,
                      double* hist_out, double* loss_out);

/* Posterior mean and variance (full_cov=False, noiseless=False) at Xs (M x d), NaN rows
 * allowed (they produce NaN outputs).  Replaces GPRegression.forward -> conditional
 * (gpr.py:247-248): K and L are recomputed at u.
 *   mean_out, var_out: M doubles (device); var includes the noise, excludes jitter.
 * Synchronises at the end (to report NOT_PD). */
int gpimhip_predict_exact(gpimhip_handle h, const gpimhip_model_t* m,
                          const double* X, const double* y, int64_t N,
                          const double* u, const double* Xs, int64_t M,
                          double* mean_out, double* var_out);

/* S joint draws from the posterior at Xs (M x d, finite), with the posterior mean and variance from the same pass.
 * The reference draws through pyro / gpytorch rsample (its multi-output predictor, gpim/gpreg/vgpr.py:213-221); its
 * exact GP exposes full_cov only.  draw s = mean + chol(Sigma) Z[s],  Sigma = K** - K*^T (K + (s_n^2 + jitter) I)^-1 K* + d I,
 * d = (noiseless ? 0 : s_n^2) + jitter (the argument below; the model's own jitter stays on the training block).
 * One Cholesky of the joint covariance of [X; Xs] (order N + M) on a matrix that belongs to this entry point
 * (grow-only, counted by gpimhip_workspace_bytes, released by gpimhip_destroy / gpimhip_set_precision): the workspace
 * of fit / predict is not touched.  DESIGN.md section 15.
 *   Z            S x M standard normals (device), draw s contiguous
 *   mean_out, var_out   M doubles each or NULL; var as gpimhip_predict_exact (noise included, jitter excluded)
 *   samples_out  S x M
 * Double-precision handles outside reflection mode only; NULL arguments, S < 1, M < 1 or jitter < 0 -> GPIMHIP_E_BADARG.
 * Synchronises at the end (to report NOT_PD). */
int gpimhip_sample_exact(gpimhip_handle h, const gpimhip_model_t* m,
                         const double* X, const double* y, int64_t N, const double* u,
                         const double* Xs, int64_t M,
                         const double* Z, int32_t S,
                         int32_t noiseless, double jitter,
                         double* mean_out, double* var_out,
                         double* samples_out);

/* S pathwise draws from the posterior on a complete product grid G (Matheron's rule):
 *   g = U^T blockdiag_b(chol(K_b + d I)) z_p        a prior draw on G through its 2^r reflection blocks, ~ N(0, K_GG + d I)
 *   r = g[idx] + sqrt(s - d) z_e                    s = s_n^2 + the model's jitter, d = `jitter` below, 0 < d <= s
 *   draw = mean + g - (K_GX + d P)(K + s I)^-1 r  (+ s_n z_n unless noiseless),   mean = K_GX (K + s I)^-1 y
 * Two factorisations, of order M / 2^r (2^r times, through one buffer) and of order N, instead of one of order N + M.
 *   G        M x d coordinates of the grid, row-major over `shape` (device)
 *   shape    d grid extents (host), their product M <= 2^31
 *   mask     bit k: axis k is symmetric about its centre and reflected (at least one); twoc: 4 doubles (host), first + last
 *            coordinate of each reflected axis
 *   idx      N DISTINCT flat indices into G, each IN RANGE [0, M) (device, int64): the training rows are G[idx].  Neither
 *            property is checked on the device: an index out of range is clamped where the training rows are gathered and
 *            skipped elsewhere, a repeated one races in the scatter -- the result is then meaningless, no error is reported
 *   Z        S x (M + N [+ M]) standard normals (device), row s = [z_p | z_e | z_n]; z_n only unless noiseless.  z_p is
 *            indexed by the grid point: row p of block b takes z_p[flat(gamma_b p)], gamma_b the reflection of the axes
 *            whose sign is -1 in b
 *   mean_out M doubles or NULL (the posterior mean of gpimhip_predict_exact);  samples_out  S x M
 * Matrices and vectors belong to this entry point (grow-only, counted by gpimhip_workspace_bytes).  Double-precision handles
 * outside reflection mode only; NULL arguments, S < 1, S > 65535 or jitter <= 0 -> GPIMHIP_E_BADARG (d <= s is the caller's
 * to check: s lives on the device).  Synchronises once, at the end (to report NOT_PD of a prior block or of K + s I). */
int gpimhip_sample_pathwise(gpimhip_handle h, const gpimhip_model_t* m,
                            const double* G, const int32_t* shape, int32_t mask, const double* twoc,
                            const int64_t* idx, const double* y, int64_t N, const double* u,
                            const double* Z, int32_t S,
                            int32_t noiseless, double jitter,
                            double* mean_out, double* samples_out);

/* S pathwise draws on a FULLY OBSERVED product grid G -- an observation y on every grid point -- computed in the grid's
 * reflection basis alone.  Per reflection block b, with e_b = (U z_e)_b and ys_b = (U y)_b:
 *   c_b = chol(K_b + d I) z_b                          the prior draw of gpimhip_sample_pathwise
 *   [alpha_b | alpha_y,b] = (K_b + s I)^-1 [c_b + sqrt(s - d) e_b | ys_b]
 *   draw = U^T [ys_b - s alpha_y,b + (s - d) alpha_b - sqrt(s - d) e_b]  (+ s_n z_n unless noiseless)
 * the draws of gpimhip_sample_pathwise with idx = 0 .. M-1 up to rounding, at 2 x 2^r factorisations of order M / 2^r through
 * one buffer: no matrix of order M and no product with K_GX.
 *   G, shape, mask, twoc, u, noiseless, jitter, mean_out, samples_out   as for gpimhip_sample_pathwise
 *   y        M observations in the row-major order of the grid (device)
 *   Z        S x (2 M [+ M]) standard normals (device), row s = [z_p | z_e | z_n] -- the layout of gpimhip_sample_pathwise
 *            with N = M
 * Matrices and vectors are those of gpimhip_sample_pathwise (grow-only, counted by gpimhip_workspace_bytes).
 * Double-precision handles outside reflection mode only; NULL arguments, S < 1, S > 65534 or jitter <= 0 ->
 * GPIMHIP_E_BADARG.  Synchronises once, at the end (to report NOT_PD of any of the 2 x 2^r factorisations, through one status
 * word; the handle stays usable). */
int gpimhip_sample_blocks(gpimhip_handle h, const gpimhip_model_t* m,
                          const double* G, const int32_t* shape, int32_t mask, const double* twoc,
                          const double* y, const double* u,
                          const double* Z, int32_t S,
                          int32_t noiseless, double jitter,
                          double* mean_out, double* samples_out);

/* S pathwise draws on a product grid G with MISSING points, through the bordered reflection blocks of the model (DESIGN.md
 * section 18): the handle is in reflection mode with a border (gpimhip_set_reflection, gpimhip_set_border), and X, x_stride,
 * y, N, B, u are those of gpimhip_predict_exact_batched for that model -- the fundamental domain, y with 0 at the missing
 * points in the adapted basis (gpim_amd.gprutils.border_blocks), B = 2^r copies of the parameter vector.
 * With A = K_GG + s I on the completed grid, V = A^-1 P_m, S = P_m^T V and g the prior draw of gpimhip_sample_pathwise:
 *   r~ = 1_o (g + sqrt(s - d) z_e),   beta = A^-1 [r~ | y~],   w = S^-1 beta_m,   alpha~ = beta - V w
 *   draw = y - s alpha~_y + (s - d) alpha~ - sqrt(s - d) z_e   at the observed points
 *        = -w_y + g + w                                        at the missing points      (+ s_n z_n unless noiseless)
 * the draws of gpimhip_sample_pathwise with idx = the observed points up to rounding.  A^-1, S^-1 and V are applied through
 * what a prediction of the model leaves (the explicit factors L_b^-1, L_S^-1 and Y_b): no matrix of the order of the grid,
 * no product with K_GX.
 *   G, shape, mask, twoc   the completed grid as for gpimhip_sample_pathwise; mask and B must be the handle's
 *   miss     the flat (row-major) grid indices of the M_m missing points of gpimhip_set_border, in its order (device int64)
 *   Z        S x (2 M [+ M]) standard normals (device), row s = [z_p | z_e | z_n], each indexed by the grid point; entries
 *            of z_e at missing points are ignored
 *   mean_out (M, may be NULL), samples_out (S x M)
 * Beyond the prediction state of the model: one block of the prior (shared with gpimhip_sample_blocks) and vectors, grow-only,
 * counted by gpimhip_workspace_bytes.  Double-precision handles only; no reflection mode, no border, a multi-output batch
 * (B = T 2^r problems with T > 1: one border per task is not built; what the handle ran before does not matter, the entry
 * sets its one border up itself), a grid that does not match the handle's blocks, NULL arguments, S < 1, S > 65534 or
 * jitter <= 0 -> GPIMHIP_E_BADARG.  Synchronises once, at the end (NOT_PD of any factorisation -- prior blocks, model blocks, S -- through the
 * model's status word; the handle stays usable). */
int gpimhip_sample_border(gpimhip_handle h, const gpimhip_model_t* m,
                          const double* X, int64_t x_stride, const double* y, int64_t N, int32_t B, const double* u,
                          const double* G, const int32_t* shape, int32_t mask, const double* twoc,
                          const int64_t* miss,
                          const double* Z, int32_t S,
                          int32_t noiseless, double jitter,
                          double* mean_out, double* samples_out);

/* Batched forms: B independent problems with the SAME N (and the same model description), advanced in
 * lock-step by every launch (grid.y = problem index) -- B spectral slices of a cube share each
 * latency-bound step of the blocked factorisation instead of paying for it B times.
 *   X         problem b reads X + b*x_stride (N x d); x_stride = 0 shares one X between all problems
 *   y         B x N,  u_inout / u  B x P,  hist_out  B x T x P,  loss_out  B x T
 *   Xs        M x d test points shared by all problems;  mean_out / var_out  B x M
 * The reference has no such loop (it fits one GP per call, gpr.py:257-283); a caller that loops
 * reconstructor(...).run() over slices gets identical per-slice results from one batched call. */
int gpimhip_fit_exact_batched(gpimhip_handle h, const gpimhip_model_t* m,
                              const double* X, int64_t x_stride, const double* y, int64_t N, int32_t B,
                              double* u_inout, double lr, int32_t T,
                              double* hist_out, double* loss_out);
int gpimhip_predict_exact_batched(gpimhip_handle h, const gpimhip_model_t* m,
                                  const double* X, int64_t x_stride, const double* y, int64_t N, int32_t B,
                                  const double* u, const double* Xs, int64_t M,
                                  double* mean_out, double* var_out);

/* ---- exact multi-output GP (vector-valued functions) ---------------------------------------
 * Replaces GPyTorch's ExactGP with MultitaskKernel / MultitaskGaussianLikelihood as the reference's vreconstructor builds
 * it (gpim/gpreg/vgpr.py:286-317 correlated, 320-354 independent).  T tasks share the N inputs X (vgpr.py:103-104: rows
 * with any NaN output are dropped); Y is T x N, task-major (block a = the N values of task a).
 *   C = B (x) K + diag(s) (x) I_N,   K = the RBF / Matern52 kernel at lengthscales l (no output scale of its own)
 *   correlated:  B = F F^T + diag(softplus(r_v)), F: T x rank (gpytorch IndexKernel; the reference uses rank 1)
 *   independent: B = diag(softplus(r_o))  (ScaleKernel(batch_shape=T); the lengthscales stay shared, vgpr.py:341-343)
 *   s_a = (1e-4 + softplus(r_a)) + (1e-4 + softplus(r_g))   (rank-0 likelihood: per-task plus global noise)
 *   l_k = ls_lo_k + (ls_hi_k - ls_lo_k) sigmoid(r_l,k)  (gpytorch Interval), or softplus(r_l,k) with ls_softplus != 0
 *   mean: a constant mu_a per task
 * Parameter vector (unconstrained, what Adam updates), P doubles:
 *   u = [mu (T) | F (T x rank, row-major) or r_o (T) | r_v (T, correlated only) | r_l (n_ls) | r_a (T) | r_g]
 * loss = -log N(vec Y | mu (x) 1, C) / (N T)  (gpytorch ExactMarginalLogLikelihood divides by the number of targets).
 * The model's kernel field is GPIMHIP_KERNEL_RBF or GPIMHIP_KERNEL_MATERN52, dim / n_ls / ls_lo / ls_hi as for the
 * single-task GP; amp_lo, amp_hi and jitter are not used (GPyTorch adds no jitter here).  More than 16 tasks, another
 * kernel, or P > 256 -> GPIMHIP_E_BADARG.  Double-precision handles only.
 * The engine splits C exactly into T single-task blocks lambda_t K + I and runs them in lock-step
 * through the batched exact-GP path; the handle's batched workspace is sized for T problems of N points.
 *   gpimhip_vgp_nll_grad   loss (1 double) and d loss / du (P doubles) at u     (vgpr.py:163-166: loss and backward)
 *   gpimhip_fit_vgp        T_iter Adam iterations on u, no host synchronisation inside the loop (vgpr.py:155-176): fresh
 *                          Adam state, lr, betas (0.9, 0.999), eps 1e-8; hist_out: T_iter x n_ls lengthscales AFTER each
 *                          step (vgpr.py:169-174), loss_out: T_iter losses BEFORE each step (either may be NULL)
 *   gpimhip_predict_vgp    the exact predictive mean and variance of likelihood(model(Xs)) (noise included) at M test
 *                          points (NaN rows give NaN), M x T each (task fastest).  Replaces the 100-sample Monte-Carlo
 *                          estimate of vgpr.py:213-221 by the quantities it estimates.
 * Reflection mode (gpimhip_set_reflection(h, mask, twoc, wts, n_total, 0) on a complete grid): each
 * task block splits into the B = 2^popcount(mask) reflection blocks, T B problems in all, problem t B + b = task t with sign
 * pattern b.  Then X is the fundamental domain (N = its N_q points), Y is T x B x N_q (task-major, then sign pattern:
 * y_a in the adapted basis, gpim_amd.gprutils.reflection_blocks_multi), wts (or NULL) is T B x N_q -- the B x N_q weights
 * repeated once per task -- and n_total the grid's N.  u, the loss, the gradient, hist_out / loss_out, Xs, mean_out and
 * var_out (M x T) are as in dense mode.  A sharded handle (gpimhip_set_reflection_shard) gives BADARG.
 * With a border (gpimhip_set_border; an incomplete grid) the three entry points compute the model of
 * the OBSERVED rows: Y holds every task with 0 at the M missing points (gpim_amd.gprutils.border_blocks_multi), n_total is
 * the number of observed rows, q and coef are shared by the tasks; the T borders S_t = (A_t^-1)_mm are handled in
 * lock-step, and a border that is not positive definite ends training like a failed block. */
#define GPIMHIP_VGP_MAX_TASKS 16
typedef struct {
    int32_t tasks;          /* T, 1 .. GPIMHIP_VGP_MAX_TASKS                                        */
    int32_t rank;           /* IndexKernel rank (correlated model), 1 .. T; ignored when independent */
    int32_t independent;    /* 0: MultitaskKernel (vgprmodel), 1: per-task ScaleKernel (ivgprmodel)  */
    int32_t ls_softplus;    /* 0: Interval(ls_lo, ls_hi) lengthscales, 1: unbounded (softplus)       */
} gpimhip_vgp_t;
int gpimhip_vgp_nll_grad(gpimhip_handle h, const gpimhip_model_t* m, const gpimhip_vgp_t* vg, const double* X,
                         const double* Y, int64_t N, const double* u, double* loss_out, double* grad_out);
int gpimhip_fit_vgp(gpimhip_handle h, const gpimhip_model_t* m, const gpimhip_vgp_t* vg, const double* X, const double* Y,
                    int64_t N, double* u_inout, double lr, int32_t T_iter, double* hist_out, double* loss_out);
int gpimhip_predict_vgp(gpimhip_handle h, const gpimhip_model_t* m, const gpimhip_vgp_t* vg, const double* X,
                        const double* Y, int64_t N, const double* u, const double* Xs, int64_t M, double* mean_out,
                        double* var_out);

/* Joint posterior draws of the T outputs (gpim_amd extension: vreconstructor.sample; the reference's only use of draws is
 * the Monte-Carlo estimate of vgpr.py:218-224).  The block reduction diagonalises the posterior as well: the latent
 * functions h_t = sum_a Q_at s_a^-1/2 f_a are independent GPs with kernel lambda_t K, unit noise and targets z_t, so the
 * call is T single-output draws -- gpimhip_sample_exact, or gpimhip_sample_blocks on a fully observed grid -- run one after
 * the other through the one matrix of those entries, and one mix f_a = mu_a + s_a^1/2 sum_t Q_at h_t.  DESIGN.md section 19.
 *   X (N x d), Y (T x N, task-major), u      the observed rows and the raw vector, as gpimhip_predict_vgp on the dense model
 *   Z            block-major standard normals (device): (T, S, M) for gpimhip_sample_vgp, (T, S, 2 M [+ M unless noiseless])
 *                for gpimhip_sample_vgp_blocks; block t's slice means what the single-output entry gives it
 *   jitter       > 0, in block units, i.e. relative to each task's noise: task a's draws carry s_a * jitter on the diagonal
 *                of their covariance; gpimhip_sample_vgp_blocks also needs jitter <= 1 (section 17's d <= s with s = 1)
 *   noiseless    0: the draws include the observation noise s_a of each task (the blocks' unit noise, mixed)
 *   mean_out, var_out   M x T each (task fastest) or NULL: the posterior of gpimhip_predict_vgp (noise included, jitter
 *                excluded); gpimhip_sample_vgp_blocks has no var_out
 *   samples_out  S x M x T (task fastest)
 *   G, shape, mask, twoc   the fully observed grid as for gpimhip_sample_blocks; Y (T x M) in grid order
 * The training workspace of the handle is not touched; the state of the reduction, the blocks' draws (T S M doubles) and
 * moments are grow-only and counted by gpimhip_workspace_bytes.  Double-precision handles outside reflection mode only; NULL
 * arguments, S < 1, S > 65534, jitter <= 0, more than GPIMHIP_VGP_MAX_TASKS tasks -> GPIMHIP_E_BADARG.  Synchronises once,
 * at the end (NOT_PD of any block's factorisation through one status word; the handle stays usable).
 * Stage timers: those of the single-output entry summed over the T blocks, and 6 = the mix kernel; gpimhip_sample_vgp also
 * records 2 = setup and projection, 3 = the mix of mean and variance. */
int gpimhip_sample_vgp(gpimhip_handle h, const gpimhip_model_t* m, const gpimhip_vgp_t* vg,
                       const double* X, const double* Y, int64_t N, const double* u,
                       const double* Xs, int64_t M,
                       const double* Z, int32_t S,
                       int32_t noiseless, double jitter,
                       double* mean_out, double* var_out,
                       double* samples_out);
int gpimhip_sample_vgp_blocks(gpimhip_handle h, const gpimhip_model_t* m, const gpimhip_vgp_t* vg,
                              const double* G, const int32_t* shape, int32_t mask, const double* twoc,
                              const double* Y, const double* u,
                              const double* Z, int32_t S,
                              int32_t noiseless, double jitter,
                              double* mean_out, double* samples_out);

/* ---- exact GP with the spectral-mixture kernel ---------------------------------------------
 * Replaces GPyTorch's ExactGP with a SpectralMixtureKernel, a ConstantMean and a GaussianLikelihood as the reference's
 * skreconstructor(kernel='Spectral') builds it (gpim/gpreg/skgpr.py:122-123: no SKI; gpim/kernels/gpytorch_kernels.py:65-70).
 * Q mixtures, D = dim (ard != 0) or 1 (one mean / scale per mixture shared by all dimensions), tau = x_i - x_j:
 *   k_q(tau) = exp(-2 pi^2 sum_d tau_d^2 s_qd^2) prod_d cos(2 pi tau_d m_qd);  K = sum_q w_q k_q + noise I
 *   w = softplus(r_w), m = softplus(r_m), s = softplus(r_s), noise = 1e-4 + softplus(r_n), mean: a constant c
 * Parameter vector (unconstrained, what Adam updates), P = 2 + Q (2 D + 1) doubles:
 *   u = [c | r_w (Q) | r_m (Q x D, row-major) | r_s (Q x D) | r_n]
 * loss = -log N(y | c 1, K) / N  (gpytorch ExactMarginalLogLikelihood).  Double-precision handles only; a handle in
 * reflection mode runs the _batched entries below.  Q > GPIMHIP_SM_MAX_MIXTURES or dim outside 1 .. GPIMHIP_MAX_DIM -> GPIMHIP_E_BADARG.
 *   gpimhip_sm_kmat      K(X, Z) (N x M) at u into out (leading dimension ld); Z == NULL: K(X, X) + noise I (N x N)
 *   gpimhip_sm_nll_grad  loss (1 double) and d loss / du (P doubles) at u
 *   gpimhip_fit_sm       T Adam iterations on u (skgpr.py:196-220), no host synchronisation inside the loop: fresh Adam
 *                        state, lr, betas (0.9, 0.999), eps 1e-8; hist_out: T x P constrained values [c, w, m, s, noise]
 *                        AFTER each step, loss_out: T losses BEFORE each step (either may be NULL)
 *   gpimhip_predict_sm   the exact predictive mean (c included) and variance of likelihood(model(Xs)) (noise included) at M
 *                        test points; NaN rows give NaN */
#define GPIMHIP_SM_MAX_MIXTURES 16
typedef struct {
    int32_t dim;            /* input dimensions, 1 .. GPIMHIP_MAX_DIM                             */
    int32_t mixtures;       /* Q, 1 .. GPIMHIP_SM_MAX_MIXTURES                                      */
    int32_t ard;            /* 1: a mean and a scale per mixture and dimension; 0: per mixture      */
    int32_t reserved;
} gpimhip_sm_t;
int gpimhip_sm_kmat(gpimhip_handle h, const gpimhip_sm_t* sm, const double* X, int64_t N, const double* Z, int64_t M,
                    const double* u, double* out, int64_t ld);
int gpimhip_sm_nll_grad(gpimhip_handle h, const gpimhip_sm_t* sm, const double* X, const double* y, int64_t N,
                        const double* u, double* loss_out, double* grad_out);
int gpimhip_fit_sm(gpimhip_handle h, const gpimhip_sm_t* sm, const double* X, const double* y, int64_t N, double* u_inout,
                   double lr, int32_t T, double* hist_out, double* loss_out);
int gpimhip_predict_sm(gpimhip_handle h, const gpimhip_sm_t* sm, const double* X, const double* y, int64_t N,
                       const double* u, const double* Xs, int64_t M, double* mean_out, double* var_out);
/* Posterior draws of this model: gpimhip_sample_exact, gpimhip_sample_pathwise and gpimhip_sample_blocks
 * with the spectral-mixture covariance and its constant mean.  Arguments, the layout of Z, workspaces and error rules are
 * those of the three entries above with `sm` in place of the model struct; what differs:
 *   - the right-hand sides are y - c, and c is added to mean_out and to every draw;
 *   - the training diagonal is the model's noise alone (it has no jitter of its own), so s = noise: jitter >= 0 for
 *     gpimhip_sample_sm, 0 < jitter <= noise (the caller's to check: the noise lives on the device) for the other two;
 *   - var_out of gpimhip_sample_sm is gpimhip_predict_sm's (noise included, jitter excluded).
 * The entries depend on the observed rows and u only: they serve a model whose training ran on reflection blocks as well,
 * called outside reflection mode (a handle in reflection mode -> GPIMHIP_E_BADARG). */
int gpimhip_sample_sm(gpimhip_handle h, const gpimhip_sm_t* sm,
                      const double* X, const double* y, int64_t N, const double* u,
                      const double* Xs, int64_t M,
                      const double* Z, int32_t S,
                      int32_t noiseless, double jitter,
                      double* mean_out, double* var_out,
                      double* samples_out);
int gpimhip_sample_sm_pathwise(gpimhip_handle h, const gpimhip_sm_t* sm,
                               const double* G, const int32_t* shape, int32_t mask, const double* twoc,
                               const int64_t* idx, const double* y, int64_t N, const double* u,
                               const double* Z, int32_t S,
                               int32_t noiseless, double jitter,
                               double* mean_out, double* samples_out);
int gpimhip_sample_sm_blocks(gpimhip_handle h, const gpimhip_sm_t* sm,
                             const double* G, const int32_t* shape, int32_t mask, const double* twoc,
                             const double* y, const double* u,
                             const double* Z, int32_t S,
                             int32_t noiseless, double jitter,
                             double* mean_out, double* samples_out);
/* The same model on the reflection blocks of a grid: the handle is in reflection mode (gpimhip_set_reflection; with
 * gpimhip_set_border for an incomplete grid), X the N points of the fundamental domain, B = 2^r the blocks of the r reflected
 * axes, ys (B x N) the targets and ones (B x N) the constant 1 (with a border: the indicator of the observed points) in the
 * adapted basis, u ONE parameter vector of P doubles shared by the blocks.  The kernel is even in every coordinate difference:
 *   K_s[p, p'] = w_p w_p' sum_q w_q prod_d ( f_qd(a_d - b_d) + sigma_d f_qd(a_d + b_d - 2 c_d) ),
 *   f_qd(t) = exp(-2 pi^2 t^2 s_qd^2) cos(2 pi t m_qd),  sigma_d = +-1 the block's sign on a reflected axis (else no mirror term)
 * loss, gradient, history and posterior are those of the dense model on the n_total points up to rounding.  Outputs as the
 * dense entries (hist_out T x P, loss_out T); predictions honour var_count of gpimhip_set_reflection.
 * gpimhip_sm_kmat on a handle in reflection mode returns the B blocks stacked (B N rows): K_s with the noise on the
 * diagonal of the present points and identity rows for absent ones, or K_s(X, Z) / sqrt(B). */
int gpimhip_sm_nll_grad_batched(gpimhip_handle h, const gpimhip_sm_t* sm, const double* X, const double* ys, const double* ones,
                                int64_t N, int32_t B, const double* u, double* loss_out, double* grad_out);
int gpimhip_fit_sm_batched(gpimhip_handle h, const gpimhip_sm_t* sm, const double* X, const double* ys, const double* ones,
                           int64_t N, int32_t B, double* u_inout, double lr, int32_t T, double* hist_out, double* loss_out);
int gpimhip_predict_sm_batched(gpimhip_handle h, const gpimhip_sm_t* sm, const double* X, const double* ys, const double* ones,
                               int64_t N, int32_t B, const double* u, const double* Xs, int64_t M, double* mean_out,
                               double* var_out);

/* ---- sparse (inducing-point) GP, variational free energy ---------------------------------
 * Replaces pyro.contrib.gp.models.SparseGPRegression(approx="VFE") as constructed by
 * reconstructor(sparse=True) (gpim/gpreg/gpr.py:145-155; formulas SURVEY App. A.7).
 * The parameter vector is u = [ P kernel/noise entries as above | Mu x d inducing inputs Xu,
 * row-major, unconstrained ]; both parts are trained by Adam (the reference trains Xu too and
 * records it every iteration, gpr.py:198-199).
 *   gpimhip_vfe_nll_grad   loss (1 double) and gradient (P + Mu*d doubles) at u
 *   gpimhip_fit_vfe        T Adam iterations; hist_theta T x P, hist_xu T x Mu x d (either may be
 *                          NULL), loss_out T or NULL; synchronises at the end
 *   gpimhip_predict_vfe    posterior mean / variance (full_cov=False, noiseless=False) at Xs */
int gpimhip_vfe_nll_grad(gpimhip_handle h, const gpimhip_model_t* m,
                         const double* X, const double* y, int64_t N, int64_t Mu,
                         const double* u, double* loss_out, double* grad_out);
int gpimhip_fit_vfe(gpimhip_handle h, const gpimhip_model_t* m,
                    const double* X, const double* y, int64_t N, int64_t Mu,
                    double* u_inout, double lr, int32_t T,
                    double* hist_theta, double* hist_xu, double* loss_out);
int gpimhip_predict_vfe(gpimhip_handle h, const gpimhip_model_t* m,
                        const double* X, const double* y, int64_t N, int64_t Mu,
                        const double* u, const double* Xs, int64_t M,
                        double* mean_out, double* var_out);
/* B sparse models of equal N and Mu in lock-step (the slices of a 4D cube, gpim/gpreg/gpr.py:145-155 once per slice):
 * every launch of the training loop carries all of them (blockIdx.y = model); each model's arithmetic is that of its own
 * gpimhip_fit_vfe / gpimhip_predict_vfe call.  X: B x N x d with x_stride doubles between models (0: shared inputs),
 * y: B x N, u: B x (P + Mu*d), hist_theta: B x T x P, hist_xu: B x T x Mu x d, loss_out: B x T (each may be NULL);
 * Xs: test points, xs_stride doubles between models (0: shared); mean_out / var_out: B x M.  A factorisation that fails in
 * any model freezes the whole batch at that iteration (GPIMHIP_E_NOT_PD, gpimhip_fit_completed). */
int gpimhip_fit_vfe_batched(gpimhip_handle h, const gpimhip_model_t* m,
                            const double* X, int64_t x_stride, const double* y, int64_t N, int64_t Mu, int32_t B,
                            double* u_inout, double lr, int32_t T,
                            double* hist_theta, double* hist_xu, double* loss_out);
int gpimhip_predict_vfe_batched(gpimhip_handle h, const gpimhip_model_t* m,
                                const double* X, int64_t x_stride, const double* y, int64_t N, int64_t Mu, int32_t B,
                                const double* u, const double* Xs, int64_t xs_stride, int64_t M,
                                double* mean_out, double* var_out);

/* ---- exact GP on a fully observed regular grid (Kronecker-structured covariance) ---------------
 * Takes the role of the reference's structured-kernel reconstructor (gpim/gpreg/skgpr.py:399-448, there
 * GPyTorch's interpolated SKI approximation): the SAME model and parameterisation as
 * gpimhip_fit_exact / gpimhip_predict_exact (RBF kernel, ARD or isotropic), but for observations on a
 * complete product grid c_1 x ... x c_d the covariance is s2 K_1 (x) ... (x) K_d and loss, gradient,
 * Adam loop and posterior follow from the n_i x n_i eigen-decompositions: O(sum n_i^3 + N sum n_i) work,
 * O(N + sum n_i^2) memory, results equal to the dense path's up to rounding.
 *   d, n[d]      grid shape (HOST array; N = prod n_i observations in C order, last axis fastest)
 *   axes         device, sum n_i doubles: the coordinate vectors c_1, ..., c_d, concatenated
 *   y            device, N doubles (no NaN: the grid must be fully observed)
 *   n_test / axes_test   the prediction grid, the same way (M = prod n_test_i outputs, C order)
 * Only GPIMHIP_KERNEL_RBF factorises over the axes; other kernels return GPIMHIP_E_BADARG. */
int gpimhip_kron_nll_grad(gpimhip_handle h, const gpimhip_model_t* m, int32_t d, const int32_t* n,
                          const double* axes, const double* y, const double* u,
                          double* loss_out, double* grad_out);
int gpimhip_fit_kron(gpimhip_handle h, const gpimhip_model_t* m, int32_t d, const int32_t* n,
                     const double* axes, const double* y, double* u_inout, double lr, int32_t T,
                     double* hist_out, double* loss_out);
int gpimhip_predict_kron(gpimhip_handle h, const gpimhip_model_t* m, int32_t d, const int32_t* n,
                         const double* axes, const double* y, const double* u,
                         const int32_t* n_test, const double* axes_test,
                         double* mean_out, double* var_out);

/* Joint posterior draws of the structured model on ANY finite product test grid (the training grid, a finer or shifted
 * one, a crop), by Matheron's rule with every factor a Kronecker product: nothing of the order of
 * N or M is factored; measured, one draw costs 1.1 - 5 predictions and each of 16 draws 0.2 - 0.8.
 *   out[s]   = g*_s + s2 ((x) Ks_i) Q D^-1 Q^T (y - g_G,s - sqrt(sigma) z_e,s) + sqrt(c) z_n,s
 *   mean_out = the same with zeta, z_e, z_n = 0: the mean of gpimhip_predict_kron (same launches, same bits)
 * with sigma = noise + m->jitter, c = (noiseless ? 0 : noise) + jitter, Ks_i, Q, D those of gpimhip_predict_kron, and the
 * prior draw (g_G, g*) = sqrt(s2) ((x) R_i[idx_train_i, :], (x) R_i[idx_test_i, :]) zeta on the two grids from one zeta over
 * the UNION axes u_i = sorted union of the training and the test coordinates of axis i:
 * R_i = Q_i^U diag(sqrt(max(lam_i^U, 0))), K_i(u_i, u_i) = Q_i^U diag(lam_i^U) Q_i^U^T.  Cov(out[s]) = Sigma_post + c I.
 *   d, n, axes, y, u, n_test, axes_test   as for gpimhip_predict_kron
 *   n_union[d]   HOST: the orders U_i of the union axes, n[i] <= U_i <= min(n[i] + n_test[i], 4096)
 *   axes_union   device, sum U_i doubles: the union axes, concatenated
 *   idx_train, idx_test   HOST, sum n_i and sum n_test_i int32: the position of every training / test coordinate in its
 *                union axis.  When idx_train is the identity on every axis and U_i = n[i] (the test grid is the training
 *                grid or a crop of it) the training decomposition serves as the union one and axes_union is not read.
 *   z            device, S x (prod U_i + N + M) doubles, each row [zeta | z_e | z_n]: zeta row-major over the union axes,
 *                z_e in training-grid order, z_n in test-grid order (read only when c > 0)
 *   S >= 1, jitter >= 0;  mean_out: M doubles, out: S x M doubles (device)
 * A draw is a pure function of its z on this library; the root R_i is fixed only up to an orthogonal change of zeta, so
 * draws for one z are not comparable with another implementation of the root -- their distribution is. */
int gpimhip_sample_kron(gpimhip_handle h, const gpimhip_model_t* m, int32_t d, const int32_t* n,
                        const double* axes, const double* y, const double* u,
                        const int32_t* n_test, const double* axes_test,
                        const int32_t* n_union, const double* axes_union,
                        const int32_t* idx_train, const int32_t* idx_test,
                        const double* z, int32_t S, int32_t noiseless, double jitter,
                        double* mean_out, double* out);

/* ---- exact GP on a grid whose missing points are whole columns (dense-by-Kronecker blocks) ----------
 * The reference's hyperspectral use case (gpim/gpreg/gpr.py:30-43): a cube measured at a sparse set of pixels, each with
 * its whole spectrum -- or an image with whole rows missing.  The observations are (the N_s observed points X_s of the p
 * "ragged" axes) x (the complete product grid of the other dc axes), so the RBF covariance is s2 K_s (x) K_c and, with the
 * eigen-decompositions K_i = Q_i diag(lambda_i) Q_i^T of the complete axes, K + sigma I splits exactly into J = prod n_i
 * ordinary exact-GP blocks s2 lambda_j K_s + sigma I of order N_s.  They share X_s and run in lock-step through the batched
 * engine: J N_s^3 work and J N_s^2 memory instead of (J N_s)^3 and (J N_s)^2.  The SAME model,
 * parameterisation, u, loss, gradient, history rows and posterior as gpimhip_nll_grad / gpimhip_fit_exact /
 * gpimhip_predict_exact on the N = N_s J observations, up to rounding.
 *   m          the model of all dim = p + dc axes (RBF; ARD or isotropic); lengthscales in the model's own axis order
 *   Xs         device, N_s x p: the observed ragged points (column k = model axis perm[k])
 *   n_c        HOST, dc ints: the orders of the complete axes (each <= 4096, J = prod n_c <= 65535)
 *   perm       HOST, dim ints, or NULL for the identity: the model's axis behind ragged column k (k < p) and behind
 *              complete axis k - p (k >= p)
 *   axes_c     device, sum n_c doubles: the coordinate vectors of the complete axes, concatenated
 *   Y          device, N_s x J: row n = the observations at ragged point n over the complete grid in C order
 *   Xs_test    device, M_s x p ragged test rows (NaN rows give NaN); n_test_c (HOST) / axes_test_c (device): the test
 *              coordinates of the complete axes; mean_out / var_out: M_s x prod n_test_c (ragged row major), var with
 *              the noise as gpimhip_predict_exact
 * Double-precision handles outside reflection mode; another kernel, p < 1, dc < 1, p + dc != dim, an axis longer than
 * 4096, J > 65535 or an invalid perm -> GPIMHIP_E_BADARG.  The workspace is grow-only and counted by
 * gpimhip_workspace_bytes.  A block that is not positive definite ends training like any failed factorisation
 * (GPIMHIP_E_NOT_PD, gpimhip_fit_completed).  Stage timers: 0 / 1 the blocks' factorisation and inverse, 2 their K^-1
 * products, 3 the variance product. */
int gpimhip_pkron_nll_grad(gpimhip_handle h, const gpimhip_model_t* m, const double* Xs, int64_t Ns, int32_t p, int32_t dc,
                           const int32_t* n_c, const int32_t* perm, const double* axes_c, const double* Y, const double* u,
                           double* loss_out, double* grad_out);
int gpimhip_fit_pkron(gpimhip_handle h, const gpimhip_model_t* m, const double* Xs, int64_t Ns, int32_t p, int32_t dc,
                      const int32_t* n_c, const int32_t* perm, const double* axes_c, const double* Y, double* u_inout,
                      double lr, int32_t T, double* hist_out, double* loss_out);
int gpimhip_predict_pkron(gpimhip_handle h, const gpimhip_model_t* m, const double* Xs, int64_t Ns, int32_t p, int32_t dc,
                          const int32_t* n_c, const int32_t* perm, const double* axes_c, const double* Y, const double* u,
                          const double* Xs_test, int64_t Ms, const int32_t* n_test_c, const double* axes_test_c,
                          double* mean_out, double* var_out);

/* Joint posterior draws of the dense-by-Kronecker blocks on (M_s ragged test rows) x (any product of test coordinates for
 * the complete axes), by Matheron's rule.  With P the union of the ragged training and test rows
 * (U_s rows), L_P = chol(s2 K_s(P, P) + jitter I), u_i / R_i the union axes and root rows of gpimhip_sample_kron for the
 * complete axes (U = prod U_i), sigma = noise + m->jitter and c_n = noiseless ? 0 : noise:
 *   H = L_P zeta,   g_X = H[irow_train, :] x_i R_i[idx_train_i, :],   g_* = H[irow_test, :] x_i R_i[idx_test_i, :]
 *   out[s]   = mean + g_* - K_*X (K_XX + sigma I)^-1 (g_X + sqrt(sigma) z_e) + sqrt(c_n) z_n
 *   mean_out = the mean of gpimhip_predict_pkron, by its launches (same bits); a draw at z = 0 is mean_out bit for bit
 * The draws are exactly N(mean, Sigma_post + c_n I + jitter T (I (x) K_c(u, u)) T^T), T = S_* - K_*X (K_XX + sigma I)^-1 S_X
 * (S_X, S_* select the training / test points out of P x u): the last term, positive semi-definite and of the size of
 * jitter, is the price of factoring K_s(P, P), which is numerically singular on a pixel grid.
 *   Xs .. axes_test_c   as for gpimhip_predict_pkron (test rows must be finite)
 *   P            device, U_s x p: the union rows, 1 <= U_s <= N_s + M_s
 *   irow_train, irow_test   HOST, N_s and M_s int32: the position of every training / test ragged row in P
 *   n_union, axes_union, idx_train, idx_test   as for gpimhip_sample_kron, for the dc complete axes (U_i <= 4096)
 *   z            device, S x (U_s U + N_s J + M_s M_c) doubles, each row [zeta | z_e | z_n]: zeta row-major over
 *                (U_s, U_1, .., U_dc), z_e in the layout of Y, z_n in the layout of the output (read only when c_n > 0)
 *   S >= 1, jitter > 0 (finite);  mean_out: M_s x M_c, samples_out: S x M_s x M_c doubles (device)
 * Every limit is checked before anything is allocated or launched (GPIMHIP_E_BADARG with a message; the handle stays
 * usable); a prior factor that is not positive definite -> GPIMHIP_E_NOT_PD at the closing check.  The draws are taken in
 * groups whose buffers stay within 0.25 GiB; the result does not depend on the grouping, and two calls with the same z give
 * the same bits (no atomics, fixed reduction shapes).  Workspace: grow-only, counted by gpimhip_workspace_bytes.
 * Stage timers: see gpimhip_timing_enable. */
int gpimhip_sample_pkron(gpimhip_handle h, const gpimhip_model_t* m, const double* Xs, int64_t Ns, int32_t p, int32_t dc,
                         const int32_t* n_c, const int32_t* perm, const double* axes_c, const double* Y, const double* u,
                         const double* Xs_test, int64_t Ms, const int32_t* n_test_c, const double* axes_test_c,
                         const double* P, int64_t Us, const int32_t* irow_train, const int32_t* irow_test,
                         const int32_t* n_union, const double* axes_union, const int32_t* idx_train, const int32_t* idx_test,
                         const double* z, int32_t S, int32_t noiseless, double jitter, double* mean_out, double* samples_out);

/* Acquisition sweep over the dense grid (gpim/gpbayes/acqfunc.py:11-92):
 *   CB : p0*mean + p1*sd                                  (alpha, beta)
 *   EI : imp*Phi(imp/sd) + sd*phi(imp/sd), imp = mean - p0 - p1     (best, xi)
 *   POI: Phi((mean - p0 - p1)/sd)
 * mask (M doubles of 1/NaN, or NULL) is multiplied in as boptim.py:307-308 does.
 * mean, sd, acq_out: M doubles (device). */
int gpimhip_acq(gpimhip_handle h, int32_t kind, const double* mean, const double* sd,
                int64_t M, double p0, double p1, const double* mask, double* acq_out);

/* One acquisition evaluation of boptimizer for an exact-GP surrogate, without leaving the device and with
 * ONE factorisation (replaces the predict / predict / nanmax / sweep sequence of gpim/gpbayes/acqfunc.py:27-29,
 * 52-62, 80-91 and boptim.py:303-308):
 *   posterior at the observed rows Xobs (Mobs x dim; EI, POI only) -> incumbent = nanmax of the means (EI) or
 *   of the means and standard deviations (POI: the reference's tuple quirk, acqfunc.py:86-88), kept on the device;
 *   posterior at the grid Xs (M x dim) -> mean_out, sd_out; acq_out = CB(p0 = alpha, p1 = beta) or
 *   EI / POI(incumbent, p1 = xi), times mask (M doubles of 1 / NaN, or NULL).
 * For N <= 384 every prediction is one fused launch whose K(X, X*) panel never leaves LDS (csrc/predict.hip). */
int gpimhip_acquire_exact(gpimhip_handle h, const gpimhip_model_t* m, const double* X, const double* y,
                          int64_t N, const double* u, const double* Xs, int64_t M, const double* Xobs,
                          int64_t Mobs, int32_t kind, double p0, double p1, const double* mask,
                          double* mean_out, double* sd_out, double* acq_out);

/* nanmax over n doubles (device) -> out (1 double, device): the incumbent
 * "np.nanmax(mean_sample)" of acqfunc.py:59,88. */
int gpimhip_nanmax(gpimhip_handle h, const double* x, int64_t n, double* out);

/* Descending top-k of acq (NaNs ranked first when keep_nan != 0, exactly like
 * np.argsort(...)[::-1] at boptim.py:303-306; dropped otherwise, boptim.py:310-315).
 * vals_out: k doubles, idx_out: k int64 flat indices (device).  count_out (device
 * int64): number of valid entries written (< k when fewer non-NaN values exist).
 * Ties rank the larger flat index first.  Grids of more than 2048 points use a multi-block radix
 * selection (O(M) per pass, no host round trip), smaller ones k arg-max passes of one workgroup. */
int gpimhip_topk(gpimhip_handle h, const double* acq, int64_t M, int32_t k, int32_t keep_nan,
                 double* vals_out, int64_t* idx_out, int64_t* count_out);

/* ---- one exact GP across several GPUs: building blocks of a block-column-cyclic Cholesky ----------
 * (SURVEY 8(f) rank 1.  The reference treats a cube as ONE d-dimensional GP, gpim/gpreg/gpr.py:30-43,
 * 115-126; its covariance does not fit one device beyond N ~ 10^5.)  The matrix is dealt to the P ranks
 * of a process group by 512-column panels (panel p -> rank p mod P, the 1 x P case of a 2-D block-cyclic
 * layout); each rank keeps its panels, all rows, side by side in ONE caller-owned row-major array
 *     Aloc : np x (512 * owned panels), leading dimension ldloc,   np = N padded to 128.
 * The host driver (gpim_amd/dist_chol.py, torch.distributed / RCCL) runs, for p = 0, 1, ...:
 *     owner(p):  gpimhip_dist_panel_factor   -> L(:, panel p) in place   (on a side stream: look-ahead)
 *                gpimhip_dist_panel_pack     -> broadcast buffer: rows of the panel + its diagonal-block inverses
 *     all     :  broadcast of the buffer ((np + 128) x 512 doubles, src = owner)
 *     each    :  gpimhip_dist_update for its owned panels right of p (panel p+1 first, the rest in one launch)
 *   gpimhip_dist_setup            per-handle set-up for order n on rank `rank` of `world`: diagonal-block workspace
 *                                 and the launch plans of this rank's share -- none of the n x n buffers of the
 *                                 single-GPU path.  gpimhip_dist_begin(h, n) = gpimhip_dist_setup(h, n, 1, 0).
 *   gpimhip_dist_panel_factor     loc_blk0: block column (128-wide) where the panel starts inside Aloc;
 *                                 glob_blk0: its global block index (a multiple of 4); logdet_out: up to 4 doubles
 *                                 (device), the sums of log L_ii of the panel's 128-blocks, or NULL; info as
 *                                 gpimhip_potrf.  The step kernels of the single-GPU factorisation (cholstep.hip)
 *                                 with the left-looking window restricted to the panel.
 *   gpimhip_dist_panel_pack       buf (ldbuf >= 512, np + 128 rows): rows [128 glob_blk0, np) <- the panel, rows
 *                                 [np, np + 128) <- the inverses of its diagonal blocks side by side
 *   gpimhip_dist_update           buf: a packed panel with global block index panel_glob_blk0; updates the OWNED
 *                                 panels c with panel_first <= c < panel_last (global panel indices) in Aloc
 *                                 (this rank's panels side by side):  C -= P_rows P_cols^T on tiles i >= j.
 *                                 One launch whatever the number of panels.
 *   gpimhip_dist_solve_update     one panel step of the forward substitution W = L^-1 B for this rank's own
 *                                 right-hand sides B (np x mpad row-major, mpad a multiple of 128, destroyed):
 *                                 W rows of the panel -> Wt (512 x mpad), B rows below -= L W, and
 *                                 q[j] += sum_r W[r][j]^2 (q may be NULL).  col_tiles > 0: only the first col_tiles
 *                                 128-column tiles of B take part (the others are known to be zero).  Replaces the
 *                                 solve_triangular /
 *                                 GEMM pair of `conditional` (gpim/gpreg/gpr.py:247-248) for a factor that is
 *                                 streamed through the ranks panel by panel. */
int gpimhip_dist_setup(gpimhip_handle h, int64_t n, int32_t world, int32_t rank);
int gpimhip_dist_begin(gpimhip_handle h, int64_t n);
int gpimhip_dist_panel_factor(gpimhip_handle h, double* Aloc, int64_t ldloc, int32_t loc_blk0,
                              int32_t glob_blk0, double* logdet_out, int32_t* info);
int gpimhip_dist_panel_pack(gpimhip_handle h, const double* Aloc, int64_t ldloc, int32_t loc_blk0,
                            int32_t glob_blk0, double* buf, int64_t ldbuf);
int gpimhip_dist_update(gpimhip_handle h, const double* buf, int64_t ldbuf, int32_t panel_glob_blk0,
                        double* Aloc, int64_t ldloc, int32_t panel_first, int32_t panel_last);
int gpimhip_dist_solve_update(gpimhip_handle h, const double* buf, int64_t ldbuf, int32_t panel_glob_blk0,
                              double* B, int64_t ldb, int64_t mpad, double* Wt, int64_t ldw, double* q,
                              int32_t col_tiles);
/* ... for two panels held side by side in a buffer of 1024 columns (gpim_amd.dist_chol._stream_pairs): the first panel of
 * a pair (second = 0) updates the second panel's block rows only; after the second panel's own solves (second = 1) the
 * rows below receive both panels in ONE pass of k-depth 1024 -- half the read-modify-write traffic over the rank's
 * right-hand sides.  wide: first panel in columns [0, 512), second in [512, 1024), each packed by gpimhip_dist_panel_pack
 * with ldbuf >= 1024; Wt2: 1024 rows.  The arithmetic per element is that of two consecutive gpimhip_dist_solve_update
 * calls with the two subtractions of a row below the pair summed in one accumulation. */
int gpimhip_dist_solve_update2(gpimhip_handle h, const double* wide, int64_t ldbuf, int32_t panel_glob_blk0, double* Bm,
                               int64_t ldb, int64_t mpad, double* Wt2, int64_t ldw, double* q, int32_t col_tiles,
                               int32_t second);

/* Distributed TRAINING of that one exact GP (gpim/gpreg/gpr.py:170-217 for a covariance that does not fit one
 * device; driver: gpim_amd/dist_chol.py exact_gp_fit).  Per Adam iteration, at the unconstrained parameters u:
 *   gpimhip_dist_kmat_cols    columns [col0, col0 + ncols_pad) of K(u) + (jitter + noise) I into out (np rows; identity
 *                             on the padding diagonal) -- every rank builds its own panels
 *   (factorisation as above, then X = L^-1 by streaming the factor once more through gpimhip_dist_solve_update with
 *    B = this rank's identity columns, Wt = the panel's rows of the rank's X share, col_tiles = the block columns that
 *    are not structurally zero yet)
 *   gpimhip_dist_kinv_update  xbuf: the broadcast block-column panel of X with global block index panel_glob_blk0
 *                             (all np rows x 512); rows of that panel of K^-1 = X^T X for the OWNED columns
 *                             (tiles i >= j) -> Kinv (np x owned columns, like Aloc)
 *   gpimhip_dist_grad_sums    the rank's share of  sum_ij (K^-1 - alpha alpha^T)_ij dK_ij/dtheta  reduced to 8
 *                             doubles S_out (device); the ranks all-reduce (sum) them
 *   gpimhip_dist_finalize     loss (given quad = y^T alpha and half_logdet = sum log L_ii), d loss / du, and -- for
 *                             t >= 1, the 1-based Adam iteration -- torch.optim.Adam's step on u (state in the handle,
 *                             reset at t = 1) and the constrained values of the stepped u in hist_row; t = 0:
 *                             loss and gradient only.  Identical inputs on every rank -> identical u.
 *   gpimhip_dist_finalize_dev the same with the scalars read from DEVICE memory, so that the training loop of
 *                             gpim_amd.dist_chol.exact_gp_fit enqueues an iteration without reading anything back:
 *                             red[0..7] = the all-reduced sums, red[8] = sum log L_ii over all ranks, red[9] = number of
 *                             ranks whose factorisation met a non-positive pivot (if not 0: *loss_out = NaN, nothing else
 *                             is written), quad[0] = y^T alpha. */
int gpimhip_dist_kmat_cols(gpimhip_handle h, const gpimhip_model_t* m, const double* X, int64_t N, const double* u,
                           int64_t col0, int64_t ncols_pad, double* out, int64_t ld);
/* The O(N^2) vector solves of alpha = K^-1 y of the distributed model (torch.linalg.solve_triangular over the whole
 * factor in the reference, gpr.py:192-193 through pyro), panel by panel on the OWNER of panel [glob_blk0, glob_blk0 + 4)
 * with the handle that factored it (the inverses of its diagonal blocks live there):
 *   gpimhip_dist_vec_forward   piece (<= 512) = Lpp^-1 (y_p - t)  (t may be NULL);  acc[rows below the panel] +=
 *                              L(below, p) piece   (acc: full-length np vector of this rank's partial sums)
 *   gpimhip_dist_vec_backward  piece = Lpp^-T (z_p - L(below, p)^T a[below])  (a: full-length np vector; work: 512 doubles)
 *   gpimhip_matvec_t           out (ncols) = A^T x, A row-major nrows x ncols (ncols % 64 == 0): K*^T alpha */
int gpimhip_dist_vec_forward(gpimhip_handle h, const double* Aloc, int64_t ldloc, int32_t loc_blk0, int32_t glob_blk0,
                             const double* y_p, const double* t, double* piece, double* acc);
int gpimhip_dist_vec_backward(gpimhip_handle h, const double* Aloc, int64_t ldloc, int32_t loc_blk0, int32_t glob_blk0,
                              const double* z_p, const double* a, double* work, double* piece);
int gpimhip_matvec_t(gpimhip_handle h, const double* A, int64_t ld, int64_t nrows, int64_t ncols, const double* x,
                     double* out);
int gpimhip_dist_kinv_update(gpimhip_handle h, const double* xbuf, int64_t ldx, int32_t panel_glob_blk0,
                             const double* Xloc, int64_t ldloc, double* Kinv, int64_t ldk);
/* ... for `npanels` consecutive panels in ONE launch: xbuf holds them side by side (np rows x 512 * npanels, the first one
 * with global block index panel_glob_blk0).  Early panels have few tiles, each as deep as the whole matrix: one at a time
 * they leave most of the chip idle (round 6: the Python driver groups 8 per launch, GPIM_DIST_KINV_GROUP).  npanels is
 * clamped to the panels that remain behind panel_glob_blk0: a last group may ask for more than there are. */
int gpimhip_dist_kinv_update_n(gpimhip_handle h, const double* xbuf, int64_t ldx, int32_t panel_glob_blk0, int32_t npanels,
                               const double* Xloc, int64_t ldloc, double* Kinv, int64_t ldk);
int gpimhip_dist_grad_sums(gpimhip_handle h, const gpimhip_model_t* m, const double* X, int64_t N, const double* u,
                           const double* Kinv, int64_t ldk, const double* alpha, double* S_out);
int gpimhip_dist_finalize(gpimhip_handle h, const gpimhip_model_t* m, int64_t N, double* u, const double* S,
                          double quad, double half_logdet, double lr, int32_t t, double* loss_out, double* grad_out,
                          double* hist_row);
int gpimhip_dist_finalize_dev(gpimhip_handle h, const gpimhip_model_t* m, int64_t N, double* u, const double* red,
                              const double* quad, double lr, int32_t t, double* loss_out, double* grad_out,
                              double* hist_row);

/* Symmetry-reduced exact GP on a COMPLETE uniform grid, for kernels that do not factorise over the axes (Matern52,
 * RationalQuadratic; RBF works too): the role of the reference's structured class (gpim/gpreg/skgpr.py:399-448 with
 * gpim/kernels/gpytorch_kernels.py:65), exact instead of interpolated.  mask: bit k = dimension k of the grid is
 * reflection-symmetric (its coordinates are symmetric about their centre); twoc[k] = first + last.
 * With a mask set, gpimhip_fit_exact_batched / gpimhip_predict_exact_batched / gpimhip_nll_grad-style calls treat the
 * B = 2^popcount(mask) problems of a batch as the diagonal blocks of ONE model in the reflection-adapted basis:
 *   X         the fundamental domain (the first half of every reflected axis): N / B points, shared (x_stride 0)
 *   y         B stacked vectors  y_s[p] = B^-1/2 sum_g chi_s(g) y[g p]   (sign pattern s = problem index, bit j = the
 *             j-th reflected dimension in ascending order carries sign -1)
 *   u         B copies of ONE parameter vector (all updated alike); hist_out / loss_out: the slots of problem 0
 *   predict   mean_out, var_out: M doubles (NOT B x M) -- the posterior of the full model at Xs
 * Axes of ODD length: the fundamental domain includes the mirror plane; wts (device, B x (N / B rounded up to the domain's
 * size), or NULL when every reflected axis is even) holds per block and point 2^(-m/2), m = the number of mirror planes the
 * point lies on, and 0 for a point that does not exist in the block (it lies on the mirror plane of an axis whose sign is
 * -1: its combination vanishes) -- such rows are identity rows of the block, and y of the block is 0 there.  n_total = the
 * number of observations of the full model (0: B x N).
 * var_count > 0: predictions compute the variance for the first var_count test points only (var_out keeps M entries; the
 * others are not written) -- the posterior variance is invariant under the reflections, so a caller predicting on the
 * training grid orders the fundamental domain first and mirrors the result (gpim_amd/gpr.py).
 * The multi-output GP (gpimhip_vgp_nll_grad / gpimhip_fit_vgp / gpimhip_predict_vgp) honours the mode too: see there.
 * mask = 0 switches back.  Double precision only. */
int gpimhip_set_reflection(gpimhip_handle h, int32_t mask, const double* twoc, const double* wts, int64_t n_total,
                           int64_t var_count);

/* The blocks of the symmetry-reduced model dealt to the ranks of a job (gpim_amd/dist_symm.py): no data-path collective at
 * all -- the blocks only share the hyper-parameters, so the ranks exchange eleven doubles per Adam iteration.
 *   gpimhip_set_reflection_shard  problem b of this handle's batches is the block of sign pattern pb_off + b * pb_stride out
 *                                 of nblocks_total = 2^r; raw != 0: gpimhip_predict_exact_batched returns in var_out the
 *                                 local blocks' summed quadratic form instead of the variance (the ranks add theirs up:
 *                                 var = max(sigma^2 - sum, 0) + noise) and in mean_out their share of the mean.  Reset by
 *                                 gpimhip_set_reflection(h, 0, ...).
 *   gpimhip_refl_sums             one evaluation of the local blocks at u (B copies of the parameter vector): kernel
 *                                 matrices, factorisations, inverses, gradient contraction; sums_out (device, 11 doubles):
 *                                 [0..7] gradient sums, [8] sum log L_ii, [9] 1 if a factorisation failed, [10] sum
 *                                 |L^-1 y|^2.  After the all-reduce, gpimhip_dist_finalize_dev takes [0..9] and [10]. */
int gpimhip_set_reflection_shard(gpimhip_handle h, int32_t pb_off, int32_t pb_stride, int32_t nblocks_total, int32_t raw);

/* Border of the reflection blocks: the exact GP on the OBSERVED points of an incomplete grid (gpim_amd/skgpr.py; DESIGN.md
 * section 11).  The blocks are those of the completed grid (y = 0 at the M missing points, n_total of
 * gpimhip_set_reflection = the number of observations); missing point j has the representative q[j] (a point of the
 * fundamental domain, device int32, M) and in block b the coefficient coef[b * M + j] (device, B x M) -- both as
 * gpim_amd.gprutils.border_blocks returns them.  Valid only in reflection mode, double precision, unsharded; honoured by
 * gpimhip_fit_exact_batched, gpimhip_predict_exact_batched, gpimhip_nll_grad_batched and, in reflection mode, by
 * gpimhip_vgp_nll_grad, gpimhip_fit_vgp and gpimhip_predict_vgp (one border per task; see there).  M = 0, or
 * gpimhip_set_reflection(h, 0, ...), switches it off.  q and coef must stay valid while it is on.
 *   gpimhip_nll_grad_batched  one loss / gradient evaluation of the coupled blocks in reflection mode (with the border when
 *                             it is set) at u (B copies of the parameter vector); loss_out, grad_out: device. */
int gpimhip_set_border(gpimhip_handle h, int32_t M, const int32_t* q, const double* coef);
int gpimhip_nll_grad_batched(gpimhip_handle h, const gpimhip_model_t* m, const double* X, int64_t x_stride, const double* y,
                             int64_t N, int32_t B, const double* u, double* loss_out, double* grad_out);
int gpimhip_refl_sums(gpimhip_handle h, const gpimhip_model_t* m, const double* X, const double* y, int64_t N, int32_t B,
                      const double* u, double* sums_out);

/* Leave-one-out cross-validation from one factorisation.  With S = K + (noise + jitter) I,
 * alpha = S^-1 y and d_i = [S^-1]_ii, the prediction of observation i from the other N - 1 is
 *   mean_out[i] = y_i - alpha_i / d_i        var_out[i] = max(1 / d_i - (noise + jitter), 0) + noise
 * (the convention of the predict entries: the jitter belongs to the training matrix, not to the reported variance) and
 *   score_out = [ sum_i log N(y_i | mean_i, var_i),  sum_i (y_i - mean_i)^2 ].
 * One factorisation and triangular inverse -- the state a prediction starts from -- then d = the column sums of squares of
 * L^-1: one pass over N^2 / 2 entries.  No K^-1 product, no gradient contraction: less than one training iteration.  Fixed
 * summation order: two calls give the same bits.  mean_out, var_out (N doubles) and score_out (2 doubles): device.
 *   gpimhip_loo_exact           the dense model (arguments of gpimhip_predict_exact) on double- and single-precision
 *                               handles, through the general engine at every N; not in reflection mode (E_BADARG)
 *   gpimhip_loo_exact_batched   the reflection blocks (arguments of gpimhip_predict_exact_batched; reflection mode with
 *                               n_total set): the blocks' diagonals in one launch, combined in grid space.  rep[i] (device
 *                               int32, n_total): the row of grid point i's representative in the fundamental domain; sgn[i]:
 *                               the reflections that take the representative to i, bit j = the j-th reflected dimension in
 *                               ascending order (0 for a point on that mirror plane); y_grid: the n_total observations in
 *                               grid order.  Outputs: n_total doubles.  With a border set (the missing points couple the
 *                               blocks), a shard, or on a single-precision handle: E_BADARG with a message.
 *   gpimhip_loo_kron            the Kronecker model (arguments of gpimhip_predict_kron without the test grid):
 *                               diag(S^-1) = ((x) Q_i o Q_i) (1 / D) by mode products.  Double-precision handles.
 * A matrix that is not positive definite: GPIMHIP_E_NOT_PD, as the predict entries. */
int gpimhip_loo_exact(gpimhip_handle h, const gpimhip_model_t* m, const double* X, const double* y, int64_t N,
                      const double* u, double* mean_out, double* var_out, double* score_out);
int gpimhip_loo_exact_batched(gpimhip_handle h, const gpimhip_model_t* m, const double* X, int64_t x_stride, const double* y,
                              int64_t N, int32_t B, const double* u, const int32_t* rep, const int32_t* sgn,
                              const double* y_grid, double* mean_out, double* var_out, double* score_out);
int gpimhip_loo_kron(gpimhip_handle h, const gpimhip_model_t* m, int32_t d, const int32_t* n, const double* axes,
                     const double* y, const double* u, double* mean_out, double* var_out, double* score_out);

/* The leave-one-out pseudo-likelihood as a training objective (Rasmussen & Williams 5.4.2).  With
 * S = K + (noise + jitter) I, alpha = S^-1 y and d_i = [S^-1]_ii
 *   loss = sum_i [ -1/2 log d_i + alpha_i^2 / (2 d_i) ] + N/2 log 2 pi + prior constant
 *        = - sum_i log N(y_i | y_i - alpha_i / d_i, 1 / d_i) + prior constant
 * The held-out variance is 1 / d_i, that of the matrix that is trained: gpimhip_loo_exact's var_out plus the jitter wherever
 * that entry did not clamp.  The prior constant is the one gpimhip_nll_grad carries.  The gradient takes the form of the
 * marginal likelihood's, 1/2 sum_ij dS_ij/dtheta (G2_ij - (r_i alpha_j + alpha_i r_j)) with q = alpha / d, r = S^-1 q,
 * omega = 1 / d + q^2 and G2 = S^-1 diag(omega) S^-1: one more N^3 product on the tile engine for all hyper-parameters
 * together, about twice the cost of an iteration on the marginal likelihood.  Through the general engine at every N; fixed
 * summation order: two calls give the same bits.
 *   gpimhip_loo_grad        loss and d loss / d u at u: the arguments of gpimhip_nll_grad
 *   gpimhip_fit_exact_loo   T Adam iterations on it: the arguments, outputs and failure report of gpimhip_fit_exact
 * One problem per call on a double-precision handle of the dense model (there is no batched form): a single-precision
 * handle, reflection mode, a border or a shard return GPIMHIP_E_BADARG with a message. */
int gpimhip_loo_grad(gpimhip_handle h, const gpimhip_model_t* m, const double* X, const double* y, int64_t N,
                     const double* u, double* loss_out, double* grad_out);
int gpimhip_fit_exact_loo(gpimhip_handle h, const gpimhip_model_t* m, const double* X, const double* y, int64_t N,
                          double* u_inout, double lr, int32_t T, double* hist_out, double* loss_out);

/* Integrated variance reduction (ALC, the active-learning criterion of Cohn) over the M rows of a test grid Xs (M x d,
 * finite: the caller's contract, as for gpimhip_sample_exact) -- DESIGN.md section 26.  With S = K + (noise + jitter) I,
 * W = L^-1 K(X, Xs) and C = K(Xs, Xs) - W^T W, the latent posterior covariance on the grid,
 *   acq_out[j] = sum_m w_m C_mj^2 / (max(C_jj, 0) + noise + jitter)
 * = sum_m w_m (latent variance at m before - after measuring candidate j): a refit puts the jitter on the new point's
 * diagonal too, so the identity is exact.  The model's state at u through the general engine at every N, W with the tile
 * engine's NN store layout, the lower tiles of C by one TN launch (M^2 N flop, not done for the upper half), then one
 * pass that reads every stored entry of C once.  Fixed summation order, no atomics: two calls give the same bits.
 *   weights   M doubles >= 0 (device) or NULL (all 1): the integral's weight of grid point m
 *   mask      M doubles of 1 / NaN (device) or NULL, multiplied in as gpimhip_acq does: excludes candidates only
 *   mean_out, sd_out   M doubles each or NULL: the posterior of gpimhip_predict_exact at Xs (sd includes the noise,
 *                      excludes the jitter)
 *   acq_out   M doubles (device)
 * W (N x M), C (M x M) and the partial sums belong to this entry point (grow-only, counted by gpimhip_workspace_bytes,
 * released by gpimhip_destroy / gpimhip_set_precision); the matrices of fit / predict are not resized.  An allocation
 * that fails: GPIMHIP_E_NOMEM, nothing enqueued.  Double-precision handles outside reflection, border and shard modes
 * only; these, NULL arguments, N < 1 or M < 1 -> GPIMHIP_E_BADARG with a reason in gpimhip_last_error().
 * Synchronises at the end (to report NOT_PD). */
int gpimhip_ivr_exact(gpimhip_handle h, const gpimhip_model_t* m, const double* X, const double* y, int64_t N,
                      const double* u, const double* Xs, int64_t M, const double* weights, const double* mask,
                      double* mean_out, double* sd_out, double* acq_out);

/* Greedy batch of q picks by integrated variance reduction -- DESIGN.md section 27.  A GP's variance does not depend on the
 * measured values, so after picking p the latent covariance of the grid is C - g g^T with
 *   g = C[:, p] / sqrt(max(C_pp, 0) + noise + jitter)
 * and the next map is gpimhip_ivr_exact's formula on the new C.  Round 0 is exactly that entry's map (mean_out, sd_out and
 * row 0 of maps_out hold its bits); pick r is the largest entry of round r's map among the live candidates -- those the mask
 * does not make NaN and no earlier round picked -- ties to the larger flat index, as gpimhip_topk, NaN never.  Between
 * rounds one pass over the stored lower tiles of C applies the downdate and takes the squared column sums: every stored
 * entry read once and written once, q - 1 passes for q picks, all launches enqueued up front (the pick travels through
 * device memory), one synchronisation at the end.  Fixed summation order, no atomics: two calls give the same bits.
 *   weights, mask      as gpimhip_ivr_exact: the weights weight the integral only, the mask excludes candidates only
 *   q                  1 <= q <= M
 *   mean_out, sd_out   M doubles each or NULL: as gpimhip_ivr_exact (the posterior BEFORE the batch)
 *   maps_out           q x M doubles or NULL: row r = the map pick r was taken from, NaN at masked and earlier picks
 *   sd_after_out       M doubles or NULL: sqrt(max(C_jj, 0) + noise) after all picks, the error bar once the batch is measured
 *   idx_out, gain_out  q each (device): the flat index of pick r and its map value = the drop of the weighted total latent
 *                      variance caused by pick r given picks 0 .. r - 1 (the gains add up to the batch's total drop)
 *   count_out          1 int64 (device): picks made; < q when the live candidates ran out, then the remaining idx_out are -1
 *                      and the remaining gain_out NaN
 * The scaled column, the live vector and a scratch map row (O(M)) join gpimhip_ivr_exact's buffers under the same rules.
 * Refuses what gpimhip_ivr_exact refuses, q < 1, q > M and NULL idx_out / gain_out / count_out: GPIMHIP_E_BADARG with a
 * reason in gpimhip_last_error(). */
int gpimhip_ivr_greedy(gpimhip_handle h, const gpimhip_model_t* m, const double* X, const double* y, int64_t N,
                       const double* u, const double* Xs, int64_t M, const double* weights, const double* mask, int32_t q,
                       double* mean_out, double* sd_out, double* maps_out, double* sd_after_out, int64_t* idx_out,
                       double* gain_out, int64_t* count_out);

/* The same two without the M x M covariance -- DESIGN.md section 30.  C is built, summed and thrown away one band of
 * `band` block columns (of 128 columns) at a time: a band buffer of M_pad x (128 band + 16) doubles, M_pad = M rounded up
 * to 128, takes the place of C; W and the partial sums (M_pad^2 / 128 doubles) stay.  The launches are those of the
 * stored entries over the band's tiles, every partial sum is written by the same tile's walk and added in the same
 * order: gpimhip_ivr_exact_banded returns the bits of gpimhip_ivr_exact for every band.
 *   band   block columns per band, >= 1, clipped to M_pad / 128 (one band: the whole lower half at once)
 * gpimhip_ivr_greedy_banded conditions on pick r by appending g^(r) = c / sqrt(max(c_p, 0) + noise + jitter), c the
 * conditioned column of the pick, to W as one more row (W holds pad(q, 128) more rows; C^(r+1) = K(Xs, Xs) - W_aug^T W_aug,
 * every squared sum stays a sum of squares), so round r + 1 is the banded pass again: a further pick costs a whole
 * M^2 N product where gpimhip_ivr_greedy pays one M^2 pass -- the price of the memory.  Its picks are those of
 * gpimhip_ivr_greedy up to rounding (other operations, not other mathematics); q = 1 returns gpimhip_ivr_exact_banded's bits.
 * Every other argument, the buffers' rules and the refusals as in the stored entries (M > 2^20: the partial sums are
 * M^2 / 128 doubles); band < 1 -> GPIMHIP_E_BADARG with a reason, nothing allocated. */
int gpimhip_ivr_exact_banded(gpimhip_handle h, const gpimhip_model_t* m, const double* X, const double* y, int64_t N,
                             const double* u, const double* Xs, int64_t M, int32_t band, const double* weights,
                             const double* mask, double* mean_out, double* sd_out, double* acq_out);
int gpimhip_ivr_greedy_banded(gpimhip_handle h, const gpimhip_model_t* m, const double* X, const double* y, int64_t N,
                              const double* u, const double* Xs, int64_t M, int32_t band, const double* weights,
                              const double* mask, int32_t q, double* mean_out, double* sd_out, double* maps_out,
                              double* sd_after_out, int64_t* idx_out, double* gain_out, int64_t* count_out);

/* Believer batch of q picks for the acquisition functions CB / EI / POI (kriging believer; for CB: GP-BUCB) -- DESIGN.md
 * section 28.  After picking p the model is conditioned on p having been measured at its posterior mean: the mean map does
 * not change, the latent variance v drops as in gpimhip_ivr_greedy,
 *   c = k(Xs, x_p) - W^T W[:, p] - sum_{s < r} g^(s) g^(s)[p],   g^(r) = c / sqrt(max(c_p, 0) + noise + jitter),   v -= g^(r) o g^(r)
 * (W = L^-1 K(X, Xs); a pivoted partial Cholesky of the posterior covariance: no M x M matrix is formed), and the next
 * pick maximises the acquisition function of (mean, sqrt(max(v, 0) + noise)).  Round 0 is gpimhip_acquire_exact's map on the
 * general engine; the incumbent of EI / POI is that entry's (nanmax of the posterior at Xobs: means for EI, means and sds
 * for POI) and takes in every believed value: b <- max(b, mean[p]) for EI, max(b, mean[p], sd[p] after the update) for POI.
 * Pick r is the largest entry of round r's map among the live candidates, ties to the larger flat index, NaN never, as
 * gpimhip_ivr_greedy.  One pass over W per pick, all launches enqueued up front, one synchronisation at the end; fixed
 * summation order, no atomics: two calls give the same bits.
 *   Xobs, Mobs         the observed rows (EI / POI; NULL / 0 for CB)
 *   kind, p0, p1       GPIMHIP_ACQ_CB: p0 * mean + p1 * sd; GPIMHIP_ACQ_EI / _POI: p1 = xi, p0 is not read
 *   mask               M doubles of 1 / NaN (device) or NULL: excludes candidates
 *   q                  1 <= q <= M
 *   mean_out, sd_out   M doubles each: the posterior BEFORE the batch (sd includes the noise, excludes the jitter)
 *   maps_out           q x M doubles or NULL: row r = the map pick r was taken from, NaN at masked and earlier picks
 *   sd_after_out       M doubles or NULL: sqrt(max(v, 0) + noise) after all picks
 *   idx_out, val_out   q each (device): the flat index of pick r and its map value; -1 / NaN once no live candidate is left
 *   count_out          1 int64 (device): picks made
 * W is gpimhip_ivr_exact's buffer; the partial sums, v, the q x M scaled columns, the live vector, the incumbents and a
 * scratch map row join it under the same rules (grow-only, counted, released with the handle, allocated before anything
 * is enqueued).  Refuses what gpimhip_ivr_exact refuses, q < 1, q > M, a kind outside CB / EI / POI, EI / POI without
 * Xobs, and NULL idx_out / val_out / count_out / mean_out / sd_out: GPIMHIP_E_BADARG with a reason in gpimhip_last_error(). */
int gpimhip_acquire_batch(gpimhip_handle h, const gpimhip_model_t* m, const double* X, const double* y, int64_t N,
                          const double* u, const double* Xs, int64_t M, const double* Xobs, int64_t Mobs, int32_t kind,
                          double p0, double p1, const double* mask, int32_t q, double* mean_out, double* sd_out,
                          double* maps_out, double* sd_after_out, int64_t* idx_out, double* val_out, int64_t* count_out);

/* Batch thinning of boptimizer.update_points (gpim/gpbayes/boptim.py:326-376): among n <= 1024 ranked
 * candidates (vals, flat grid indices into a d-dimensional grid of the given shape) repeatedly keep the
 * largest remaining value and drop every candidate within Euclidean index distance <= dscale of it
 * (scipy.spatial.cKDTree.query_ball_point semantics), until none is left or max_out are kept.
 *   shape      d int64 (device);  keep_out  max_out int32 (device): kept positions 0..n-1, in order;
 *   nkeep_out  1 int32 (device).  The random padding of short batches stays with the caller (np.random). */
int gpimhip_thin_batch(gpimhip_handle h, const double* vals, const int64_t* flat_idx, int32_t n, int32_t d,
                       const int64_t* shape, double dscale, int32_t max_out, int32_t* keep_out,
                       int32_t* nkeep_out);

/* The launch plan of the factorisation (and of the triangular inverse riding in its launches, with_inverse != 0) for a
 * double-precision matrix of nb block columns, as HOST data -- no device involved; for tests that replay the schedule
 * on small blocks (tests/test_step_plan.py).  Records of six int32 in `out` (capacity `cap` records): launch index
 * (< nb: the step launch that factors that block column; >= nb: the launches after the last step), ci, cj, kb0, kb1,
 * kind (0: A[ci,cj] -= sum_k L[ci,k] L[cj,k]^T; 1 / 2: Tm[ci,cj] (=|+=) sum_k A[ci,k] A[k,cj]; 3 / 4: A[ci,cj] (=|-=)
 * -sum_k A[ci,k] Tm[k,cj]; k over block columns [kb0, kb1)).  *n_out = number of records of the plan. */
int gpimhip_step_plan_host(int32_t nb, int32_t with_inverse, int32_t* out, int64_t cap, int64_t* n_out);

/* The plan with the inverse as it RUNS for at most four problems: from nb = 68 the step launches of the bulk regime factor
 * two block columns each (a pair's hosted operations are recorded under its first column); below nb = 68 the records of
 * gpimhip_step_plan_host(nb, 1, ...).  pair_out (nb int32, may be NULL): 1 = the launch of this column factors the next one
 * too, 2 = second column of a pair (no launch of its own), 0 = one column per launch.  After the records of the launches,
 * records of kind 5 under a pair's first column j list the update terms the launch AFTER its step launch applies besides
 * solving both columns: k-block j to the tiles (i, j+1), i >= j+2, and k-blocks [j, j+2) to the tiles (j+2,j+2), (j+3,j+2),
 * (j+3,j+3).  GPIMHIP_NO_PAIR_STEPS=1 (read when a handle builds its plans) runs the per-column schedule instead. */
int gpimhip_step_plan_host_paired(int32_t nb, int32_t* out, int64_t cap, int64_t* n_out, int32_t* pair_out);

/* The same for a single-precision handle (cholstep32.hip: hosted fill capped from 88 block columns, pair mode from 160),
 * records in the order of the tile list the handle uploads.  What the float schedule adds: launch index -(p + 1) = the
 * tile-engine launch before the first step of outer panel p (four block columns; the part of the panel's bulk update
 * that exceeds the cap), and diag_out (nb int32, may be NULL): diag_out[j] = how many diagonal tiles, (j+1, j+1)
 * onwards, the launch after the panel solve of block column j updates with column j. */
int gpimhip_step_plan_host_f32(int32_t nb, int32_t with_inverse, int32_t* out, int64_t cap, int64_t* n_out,
                               int32_t* diag_out);

/* The work plan of the Cholesky-with-inverse of an LDS-resident block of npan 16-column panels (blocklds.hpp:
 * lds_factor_inv -- the fused trainer for N <= 128 at npan = ceil(N / 16), the diagonal blocks of the blocked Cholesky at
 * npan = 8), as HOST data: out[0..6] = the plan words of step p for workers 0-5 (waves 1, 2, 3, 5, 6, 7) and worker 6
 * (wave 0), from the function the device table is initialised from.  A word: bits 0-3 / 4-7 the tiles j of row p of the
 * inverse the worker forms (15 = none), bits 8-11 its number of trailing items, then 12 bits per item
 * (rtA << 9) | (ctA << 6) | (rtB << 3) | ctB (rtB = 0: one tile).  tests/test_fi_plan_host.py replays it on small blocks.
 * GPIMHIP_E_BADARG outside 1 <= npan <= 8, 0 <= p < npan. */
int gpimhip_fi_plan_host(int32_t npan, int32_t p, uint64_t* out);

/* DIAGNOSTIC: the MFMA tile engine behind every O(N^3) stage, by itself (tests/test_gemm_host.py, tests/test_gpu_gemm.py).
 * Nothing in the product path calls these four.
 *
 * A launch covers a list of 128 x 128 output tiles, for `batch` problems in lock-step:
 *   C[ci + c_roff, cj + c_coff] = alpha * sum_{kb in [kb0, kb1)} A-block(ci, kb) * B-block(kb, cj) + beta * C[...]
 * on row-major matrices in blocks of 128.  A-block(ci, kb) is block (ci + a_roff, kb + a_coff) of A when a_km = 0 (rows
 * of A are rows of the product, k contiguous) and the transpose of block (kb + a_roff, ci + a_coff) when a_km = 1;
 * B-block(kb, cj) is the transpose of block (cj + b_roff, kb + b_coff) of B when b_km = 0 and block (kb + b_roff,
 * cj + b_coff) when b_km = 1.  Layout pairs: NT (0, 0), NN (0, 1), TN (1, 1).  epi = 1 (NN only) stores, instead of C,
 * the column sums of squares of each product tile: colpart[ci * ld_colpart + (cj + c_coff) * 128 + col], in double for
 * either precision.  Problem p of the batch reads A + p * sA, B + (p >> bshift) * sB and writes C + p * sC (colpart +
 * p * sColpart), strides in elements.  Switches, as GemmArgs (csrc/common.hpp) documents them: krev (walk each k-range
 * from its end), chunk (dealing of the list to the XCDs), kfix0 < kfix1 (one k-range for every tile), rect_rows x
 * rect_cols (no list: the tiles of a rectangle, ntiles = their product; needs kfix), cj_max (> 0: tiles with cj >= cj_max
 * are skipped), cmap (the output block column is the tile's kb0; needs kfix), rag (> 0: rows >= 64 of block row rag - 1
 * are not computed and the last 64 k of a range ending at block rag are not read), inplace (row-half workgroups),
 * shape_div (the shape is chosen for ntiles * batch / shape_div tiles).  A single-precision handle
 * (gpimhip_set_precision) reads A, B, C as float and refuses rect_cols, cj_max, cmap, rag and shape_div, which its
 * engine does not implement.
 *   gpimhip_gemm_tiles          copies the HOST list `tiles` (ntiles quadruples ci, cj, kb0, kb1; NULL with rect_cols > 0)
 *                               to the device, runs the production dispatch (launch_gemm) once and synchronises.
 *                               A, B, C, colpart: device.  The caller answers for the extents: every block a tile names
 *                               must lie inside the matrices.
 *   gpimhip_gemm_shape_host     the workgroup shape the dispatch chooses (GPIMHIP_GEMM_SHAPE_*), or -1 when there is
 *                               nothing to launch or the engine has no such layout / switch.  No device involved.
 *   gpimhip_gemm_tile_pos_host  the map workgroup index -> (position in the tile list, part of the tile) of a launch of
 *                               n tiles in `quads` (1, 2, 4) workgroups per tile, for bx = bx0 .. bx0 + count - 1; fp32 != 0:
 *                               the copy of the map that the single-precision kernels compile.
 *   gpimhip_gemm_rect_tile_host the map position -> (ci, cj) of a rectangle launch, for p = p0 .. p0 + count - 1. */
#define GPIMHIP_GEMM_SHAPE_QUAD 0     /* 4 waves on a 64 x 64 quadrant */
#define GPIMHIP_GEMM_SHAPE_ROWHALF 1  /* 8 waves on a 64 x 128 row half */
#define GPIMHIP_GEMM_SHAPE_8W_LDS 2   /* 8 waves on a tile, one workgroup per CU (24 KB of dynamic LDS) */
#define GPIMHIP_GEMM_SHAPE_8W 3       /* 8 waves on a tile */
#define GPIMHIP_GEMM_SHAPE_4W 4       /* 4 waves on a tile */
typedef struct {
    const void* A; int64_t lda; int32_t a_roff, a_coff;
    const void* B; int64_t ldb; int32_t b_roff, b_coff;
    void* C; int64_t ldc; int32_t c_roff, c_coff;
    double* colpart; int64_t ld_colpart;
    double alpha, beta;
    const int32_t* tiles; int32_t ntiles;
    int32_t a_km, b_km, epi;
    int32_t krev, chunk, kfix0, kfix1, rect_rows, rect_cols, cj_max, cmap, rag, inplace, bshift, shape_div;
    int64_t sA, sB, sC, sColpart;
    int32_t batch;
} gpimhip_gemm_test_t;
int gpimhip_gemm_tiles(gpimhip_handle h, const gpimhip_gemm_test_t* d);
int gpimhip_gemm_shape_host(int32_t fp32, int32_t a_km, int32_t b_km, int32_t epi, int64_t ntiles, int64_t batch,
                            int32_t shape_div, int32_t inplace);
int gpimhip_gemm_tile_pos_host(int32_t fp32, int32_t n, int32_t chunk, int32_t quads, int32_t bx0, int32_t count,
                               int32_t* p_out, int32_t* quad_out);
int gpimhip_gemm_rect_tile_host(int32_t rect_rows, int32_t rect_cols, int32_t p0, int32_t count, int32_t* ci_out,
                                int32_t* cj_out);

/* DIAGNOSTIC: the eigen-solver under the structured (Kronecker) paths by itself (tests/test_gpu_kron_eigh.py).  Nothing in
 * the product path calls it.  Runs the product's own chain -- the axis workspace, the eigen-problem plan (a centro-symmetric
 * axis of n >= 8 points splits into a symmetric problem of order ceil(n/2) and a skew one of order floor(n/2)), the cold
 * start of the rotations unless warm != 0, then K_i[a,b] = exp(-((c_a - c_b) / ls[i])^2 / 2) and its one-sided Jacobi
 * eigen-decomposition -- on an axis set of its own, and synchronises.
 *   d, n (HOST, d orders, each 1 .. 4096), axes (device, sum n_i coordinates), ls (HOST, d lengthscales > 0)
 *   warm      != 0: the rotations continue from those the previous call on this handle left behind, as an Adam iteration's
 *             do (needs such a call, on axes of the same orders that split the same way); 0: from the identity
 *   lam_out   device, sum n_i: the eigenvalues, axis by axis, in the solver's own (unsorted) order
 *   Qt_out    device, sum n_i^2: row j of axis i's n_i x n_i block is the eigenvector of lam_out[off_i + j]
 *   nprob_out HOST: the number of eigen-problems (at most 2 d)
 *   plan_out  HOST, 4 int32 per problem: axis, part (0 whole, 1 symmetric, 2 skew), order, sweeps run
 *   rot_out   HOST, one double per problem: the largest |sin| of a rotation applied in the last sweep
 *   cap_out   HOST (may be NULL): the cap of the sweep loop; a problem whose sweeps reach it did not end by its own rule */
int gpimhip_kron_eigh(gpimhip_handle h, int32_t d, const int32_t* n, const double* axes, const double* ls, int32_t warm,
                      double* lam_out, double* Qt_out, int32_t* nprob_out, int32_t* plan_out, double* rot_out,
                      int32_t* cap_out);

/* Stage timing for bench.py (HIP events on the handle's stream, recorded only while enabled).
 * stage: 0 = Cholesky (all launches of one factorisation, including the tile operations of the triangular inverse
 *            they host), 1 = what is left of the triangular inverse after the last step,
 *        2 = K^-1 = L^-T L^-1 (exactly one gemm_tiles_kernel<true,true,0> launch, N^3/3 flop),
 *        3 = predictive-variance product L^-1 K(X,X*) (one launch per test-point slab),
 *        4 = spectral-mixture covariance build K(X, X) (gpimhip_sm_*: one launch per evaluation),
 *        5 = spectral-mixture gradient contraction (its tile launch and the record sum).
 * gpimhip_sample_exact: 4 = build of the joint covariance, 0 = its factorisation, 1 = the forward substitution z = L11^-1 y,
 *        5 = the draws kernel (one interval per sweep of the trapezoid).
 * gpimhip_sample_pathwise: 4 = covariance builds (2^r prior blocks, K), 0 = their factorisations, 5 = the sweeps L_b z_p,
 *        2 = gathers and the basis change U^T, 1 = the vector solves, 3 = cross_apply_kernel and its epilogue.
 * gpimhip_sample_blocks: 4 = covariance builds (2 x 2^r), 0 = their factorisations, 5 = the sweeps L_b z_p, 2 = gathers and the
 *        basis changes U and U^T, 1 = the multi-column solves, 3 = right-hand sides, combination and epilogue.
 * gpimhip_sample_sm / _sm_pathwise / _sm_blocks: the stages of gpimhip_sample_exact / _pathwise / _blocks (the phases belong
 *        to the covariance builds and to the cross apply, y - c and + c to the stage they sit in).
 * gpimhip_sample_border: 4 = covariance builds of the 2^r prior blocks, 0 = factorisations (prior blocks, model blocks, S,
 *        with the inverses the launches host), 5 = the sweeps L_b z_p, 2 = gathers and basis changes, 1 = the multi-column
 *        sweeps through L_b^-1 (and the rest of the triangular inverses), 6 = those two sweeps alone (one interval per group
 *        of columns, inside stage 1's; no other entry point records stage 6), 3 = right-hand sides, the border's vectors,
 *        combination and epilogue; the model's covariance build, K^-1 product and border products are not timed.
 * gpimhip_sample_kron: 0 = eigen-decomposition of the union axes (absent when the training one serves), 1 = that of the
 *        training axes with y~ and alpha~, 2 = the prior: root rows, zeta, both chains of mode products, 3 = the update:
 *        cross factors, residual, its three chains of mode products (the mean's among them), 5 = the epilogue.
 * gpimhip_sample_pkron: 6 = the blocks as a whole (theta, eigen-decomposition of the complete axes, factorisation with the
 *        inverse, the mean's beta; inside it the intervals 0 / 1 of the blocks' factorisation and inverse), 4 = the prior
 *        factor (covariance build of the union rows and its factorisation), 2 = the prior draws (the union axes'
 *        eigen-decomposition and root rows, zeta, H = L_P zeta on the tile engine, gathers, mode products), 3 = the update
 *        (cross factors, residual, projection, the blocks' two solve launches, K*_s products and mode products, the mean's
 *        among them), 5 = the epilogue.
 * gpimhip_timing_read synchronises, returns the summed milliseconds and the number of timed
 * intervals since the last read, and clears them. */
int gpimhip_timing_enable(gpimhip_handle h, int enable);
int gpimhip_timing_read(gpimhip_handle h, int stage, double* total_ms, int64_t* count);

/* Number of Adam iterations the last gpimhip_fit_exact[_batched] / gpimhip_fit_vfe call completed: T,
 * or -- when that call returned GPIMHIP_E_NOT_PD -- the index of the iteration whose covariance was not
 * positive-definite.  The device loop freezes u, the optimiser state and the history rows at that
 * iteration (the reference raises there, gpr.py:192, with the parameters of the previous step), so
 * u_inout and the first gpimhip_fit_completed() rows of hist_out / loss_out are valid after the error. */
int gpimhip_fit_completed(gpimhip_handle h);

/* Releases the process-wide helper streams of the library (created on first use, shared by all handles).  Call once,
 * after the last handle has been destroyed and before the process exits; the Python binding registers it with
 * atexit.  Handles created afterwards recreate what they need. */
int gpimhip_shutdown(void);

/* Block until everything enqueued on the handle's stream has finished. */
int gpimhip_sync(gpimhip_handle h);

#ifdef __cplusplus
}
#endif
#endif /* GPIMHIP_H */
