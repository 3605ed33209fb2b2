// common.hpp -- shared declarations of libgpimhip (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <functional>
#include <string>
#include <type_traits>
#include <vector>
#include <utility>
#include "../../include/gpimhip.h"

#define NB 128            // block size of every blocked algorithm (rows/cols of one tile)
#define GEMM_BK 16        // k-depth of one LDS stage of the MFMA GEMM
#define MAXP GPIMHIP_MAX_PARAMS

void gpim_set_error(const std::string& s);

#define HIP_TRY(expr)                                                              \
    do {                                                                           \
        hipError_t _e = (expr);                                                    \
        if (_e != hipSuccess) {                                                    \
            gpim_set_error(std::string(#expr) + ": " + hipGetErrorString(_e));     \
            return GPIMHIP_E_HIP;                                                  \
        }                                                                          \
    } while (0)

#define GP_TRY(expr)                      \
    do {                                  \
        int _r = (expr);                  \
        if (_r != GPIMHIP_OK) return _r;  \
    } while (0)

// The one dispatch on the covariance function: f(std::integral_constant<int, KIND>{}) for the model's kind -- the launchers
// instantiate their kernel templates on decltype(K)::value -- and f's return code; any other kind is a bad argument.
template <typename F> static inline int with_kind(int kind, F&& f) {
    switch (kind) {
        case GPIMHIP_KERNEL_RBF: return f(std::integral_constant<int, GPIMHIP_KERNEL_RBF>{});
        case GPIMHIP_KERNEL_MATERN52: return f(std::integral_constant<int, GPIMHIP_KERNEL_MATERN52>{});
        case GPIMHIP_KERNEL_RQ: return f(std::integral_constant<int, GPIMHIP_KERNEL_RQ>{});
        default: gpim_set_error("unknown kernel kind"); return GPIMHIP_E_BADARG;
    }
}

// A device buffer that knows its own size: cap elements, charged to h->bytes by alloc / grow and credited by release (the
// members are defined below gpimhip_ctx).  Reads as a plain pointer wherever one is expected.
struct gpimhip_ctx;
template <typename T> struct DevBuf {
    T* p = nullptr;
    int64_t cap = 0;                          // elements allocated (what h->bytes was charged for)
    // exactly count elements into an empty buffer; what: the error text of a failed hipMalloc (default: HIP's own)
    int alloc(gpimhip_ctx* h, int64_t count, const char* what = nullptr);
    // grow-only, to exactly want elements.  The stream is synchronised before the free: earlier launches may still read the buffer.
    int grow(gpimhip_ctx* h, int64_t want);
    void release(gpimhip_ctx* h);
    operator T*() const { return p; }
};

// One output tile of a blocked GEMM-like launch: C[ci,cj] (op)= sum_{kb in [kb0,kb1)} A(ci,kb) B(kb,cj)
struct TileDesc {
    int32_t ci, cj, kb0, kb1;
};

// Device-resident constants of one model instance, refreshed from u each iteration.
// Layout shared by host and device code.
struct ThetaDev {
    double var;                     // sigma^2
    double ls[GPIMHIP_MAX_DIM];     // lengthscale per input dim (isotropic: replicated)
    double inv_ls[GPIMHIP_MAX_DIM];
    double noise;                   // sigma_n^2
    double alpha;                   // RationalQuadratic scale_mixture
    double diag_add;                // jitter + noise
    // chain-rule factors d theta / d u (0 where the clipped sigmoid saturates)
    double dvar_du;
    double dls_du[GPIMHIP_MAX_DIM];
    double dnoise_du;
    double dalpha_du;
};

struct AdamStep {
    double lr_over_bc1;     // lr / (1 - beta1^t)
    double bc2_sqrt;        // sqrt(1 - beta2^t)
    double beta1, beta2, eps;
};
// Adam's constants with a neutral step (do_adam = 0, or the finalize step looks lr_over_bc1 / bc2_sqrt up by iteration)
static inline AdamStep adam_step_init() {
    AdamStep st;
    st.beta1 = 0.9; st.beta2 = 0.999; st.eps = 1e-8; st.lr_over_bc1 = 0.0; st.bc2_sqrt = 1.0;
    return st;
}

// Iteration-indexed form of a finalize kernel (grad.hip, vgp.hip, sm.hip, kron.hip): when `iter` is given the Adam bias
// corrections, the history row and the loss slot are looked up by the device-resident iteration counter, which the kernel
// advances.  All T iterations then enqueue byte-identical launches, i.e. one captured hipGraph can be replayed
// (run_fit_iterations).  Passed to the kernels by value: the members are the kernel-argument layout.
struct FinalizeIter {
    int32_t* iter;              // device counter (null: one evaluation with the by-value arguments)
    const double* bc;           // [2*T]: lr/(1-beta1^t) then sqrt(1-beta2^t)
    int32_t T;
    double* hist_base;          // T x (parameters of a history row) or null
    double* loss_base;          // T or null
};

// Where a finalize launch leaves its results.  One evaluation (gpimhip_nll_grad): the three by-value pointers, no table.  A
// training loop: the table alone -- loss slot and history row are looked up by the iteration (theta.hpp: finalize_iter_begin).
struct FinalizeOut {
    double* loss_out; double* grad_out; double* hist_row;
    FinalizeIter fi;
    FinalizeOut(const FinalizeIter& tab) : loss_out(nullptr), grad_out(nullptr), hist_row(nullptr), fi(tab) {}
    FinalizeOut(double* loss, double* grad, double* hist) : loss_out(loss), grad_out(grad), hist_row(hist), fi{nullptr, nullptr, 0, nullptr, nullptr} {}
};

// A cached launch plan: tile lists of the level-by-level triangular inverse and of the K^-1 product at a given nb.
struct PlanRange { int64_t off; int32_t n; };

struct LinalgPlan {
    int nb = 0;
    TileDesc* d_tiles = nullptr;          // device copy of all tile lists
    int64_t n_tiles = 0;
    // trtri: per level two launches
    std::vector<PlanRange> tri_t, tri_x;
    // lauum
    PlanRange lauum{0, 0};
};

// Launch plan of the step schedule of the Cholesky (cholstep.hip): per block column the tiles hosted by the launch
// that factors its diagonal block and the diagonal tiles updated after its panel solve; per outer panel what is
// left of the previous panel's bulk update.
struct StepPlan {
    int nb = 0;
    int fp32 = 0;                       // hosting policy the lists were built for (cholstep.hip)
    TileDesc* d_tiles = nullptr;
    int64_t n_tiles = 0;
    std::vector<PlanRange> fill;        // per block column: what its step launch hosts
    std::vector<PlanRange> diag;        // per block column: .n = diagonal tiles updated after its panel solve
    std::vector<PlanRange> bulk_rest;   // per outer panel: bulk update launched before its first step (float handles)
    std::vector<PlanRange> post;        // fused inverse: what is left of it after the last step, launch by launch
    std::vector<int32_t> n_update;      // per block column: k-blocks of trailing update among fill[] (sets the hosted shape)
    std::vector<int32_t> n_all;         // per block column: all hosted k-blocks (shape of the launches of a large batch)
    std::vector<uint8_t> pair;          // per block column: its step launch runs hosted quadrants two per CU (cholstep.hip)
    std::vector<uint8_t> copy;          // per block column: its step launch leaves a copy of A[j+1, j] (TILE_COPY): F_j and D_j fuse
    std::vector<uint8_t> lead;          // per block column: 1 = its step launch factors columns j and j+1 (paired schedule), 2 = column
                                        // j+1 of such a pair (no launch of its own), 0 = one column per launch
};

// Launch plans of the distributed (block-column-cyclic, 1 x P) factorisation for one rank (distgp.hip: gpimhip_dist_*)
struct DistPlan {
    int nb = 0, world = 0, rank = 0;
    TileDesc* d_tiles = nullptr;
    int64_t n_tiles = 0;
    std::vector<PlanRange> colfill;     // per global block column j: the in-panel left-looking column update
    std::vector<PlanRange> upd_panel;   // per global panel c: the tiles of its trailing update (empty when not owned)
    std::vector<PlanRange> kinv_panel;  // per global panel c: tiles of K^-1 rows of panel c x owned columns (training)
    PlanRange grad_tiles{0, 0};         // the owned lower tiles of K^-1 for the gradient contraction
    int rect_cols = 0;                  // column-tile count the rectangle list below was built for
    TileDesc* d_rect = nullptr;         // tiles (r, c), r = 0 .. nb-1, c = 0 .. rect_cols-1, row-major
    int64_t n_rect = 0;
};

// Reflection symmetry of a complete, uniform grid under a stationary kernel that is even in every coordinate difference
// (gpimhip_set_reflection; engine.hip: kmat_refl_kernel): mask = the reflected dimensions (bit k), twoc[k] = first + last
// coordinate of dimension k, so that the mirror image of z_k is twoc[k] - z_k.
// wts (optional, device, B x N): per block and point 1 / sqrt(|stabiliser|) -- 1 off the mirror planes, 2^-1/2 on one
// plane (axes of odd length), ... -- and 0 where the point does not exist in that block (a point on the mirror plane of
// an axis whose sign is -1): such rows are identity rows of K_s.  n_total: the number of observations of the full model.
struct ReflArgs {
    int mask;
    double twoc[GPIMHIP_MAX_DIM];
    const double* wts;
    int64_t n_total;
    int64_t var_count;      // > 0: predictions compute the variance for the first var_count test points only
    // blocks dealt to the ranks of a job (gpimhip_set_reflection_shard): problem b of the local batch is the block of sign
    // pattern pb_off + b * pb_stride; |G| = nblocks_total (the K* scale).  raw: predictions return, instead of the variance,
    // the blocks' summed quadratic form  sum_s |L_s^-1 K*_s|^2  (the ranks add theirs up before subtracting from sigma^2)
    int pb_off, pb_stride, nblocks_total, raw;
};
struct gpimhip_ctx {
    ReflArgs refl = {0, {0, 0, 0, 0}, nullptr, 0, 0, 0, 1, 0, 0};
    int device = 0;
    hipStream_t stream = nullptr;
    hipStream_t capture_stream = nullptr; // internal stream used only to capture one iteration into a hipGraph
    bool capture_stream_tried = false;    // the capture stream is created on first use
    int side_generation = 0;              // generation of the process-wide capture stream the pointer below belongs to (api.hip)
    // workspace (sized for np = padded N)
    int64_t np = 0;                 // padded matrix order the buffers are sized for
    int64_t ld = 0;                 // leading dimension (doubles) of A, B, Tm: np, or np + 16 (see ws_ensure_b)
    int nbatch = 1;                 // problems processed in lock-step by the current call (grid.y)
    int ws_batch = 0;               // number of problems the workspace is sized for
    DevBuf<double> A;               // np x np : K -> L -> L^-1
    DevBuf<double> B;               // np x np : K^-1 (lower)
    DevBuf<double> Tm;              // np x np : trtri temporary
    DevBuf<double> dinv;            // nb x 128 x 128 inverses of diagonal blocks
    DevBuf<double> dinvB;           // the same in MFMA B-operand order (panel solve of cholstep.hip); fp64 handles
    DevBuf<double> pcopy;           // B x 128 x 128: A[j+1, j] as the step launch of column j left it (cholstep.hip: panel_solve_diag_kernel)
    DevBuf<double> ypad;            // np
    DevBuf<double> z;               // np  (L^-1 y)
    DevBuf<double> alpha;           // np  (K^-1 y)
    DevBuf<double> logdet_part;     // nb
    DevBuf<double> grad_part;       // ntiles_lower x 8
    DevBuf<double> gemv_part;       // gemv_tri_chunks(np) x np: row-chunk partial sums of alpha = L^-T z (engine.hip: gemv_t_tri_kernel)
    DevBuf<uint32_t> fin_counter;      // per problem: workgroups of grad_reduce_kernel that have finished (grad.hip: FinFused; the last
                                       // one runs the finalize step and resets it)
    DevBuf<ThetaDev> theta;         // [ws_batch]
    DevBuf<ThetaDev> theta1;        // single struct for the operator-level gpimhip_kmat
    DevBuf<int32_t> iter;           // [ws_batch] device-side iteration counters
    DevBuf<double> adam_m;          // MAXP
    DevBuf<double> adam_v;          // MAXP
    DevBuf<int32_t> info;           // potrf status word
    // prediction workspace
    int64_t ks_rows = 0, ks_cols = 0, ks_batch = 0;   // ks_cols = CAPACITY in test-point columns (grow-only)
    struct PredList { int nc; DevBuf<TileDesc> tiles; };
    std::vector<PredList> pred_lists;                // variance-product tile lists by number of column blocks
    DevBuf<double> Ks;              // np x mc chunk of K(X, X*)
    DevBuf<double> colpart;         // nb x mc partial column sums of squares
    DevBuf<double> mean_tmp;        // mc
    TileDesc* pred_tiles = nullptr; // tile list of the variance product
    int64_t pred_ntiles = 0;
    int64_t bytes = 0;
    LinalgPlan plan;
    StepPlan splan, splan_inv;      // factorisation alone / with the triangular inverse riding in its launches
    StepPlan splan_pair;            // splan_inv with two block columns per step launch in the bulk regime (nb >= 68, <= 4 problems)
    DistPlan dplan;
    // optional stage timing (bench.py): HIP event pairs on the handle's stream
    bool timing = false;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> ev[7];
    // Adam bias-correction table for the fused small-N trainer
    DevBuf<double> bc;
    std::vector<double> bc_host;
    // top-k scratch
    DevBuf<unsigned long long> keys;
    DevBuf<double> acq_tmp;         // observed-rows posterior + incumbent (gpimhip_acquire_exact)
    DevBuf<char> sel_scratch;       // radix-select state, candidates, nanmax partials (select.hip)
    // training-loop bookkeeping: iterations completed by the last fit call, pinned copy of the status
    // word + events of the bounded run-ahead check (api.hip: RunAhead)
    int fit_completed = 0;
    int32_t* pinned_info = nullptr;
    hipEvent_t ra_ev[2] = {nullptr, nullptr};
    // sparse (VFE) workspace, owned by vfe.hip (VfeWs*); released by vfe_release()
    void* vfe = nullptr;
    // structured (Kronecker) workspace, owned by kron.hip (KronWs*); released by kron_release()
    void* kron = nullptr;
    // multi-output GP workspace, owned by vgpgp.hip (VgpWs); released by vgp_release()
    void* vgp = nullptr;
    // dense-by-Kronecker blocks (a grid whose missing points are whole columns), owned by pkrongp.hip (PkronWs); pkron_release()
    void* pkron = nullptr;
    // spectral-mixture workspace, owned by smgp.hip (SmWs); released by sm_release()
    void* sm = nullptr;
    // border of the reflection blocks (missing points of an incomplete grid), owned by api.hip (BorderWs); border_release()
    void* border = nullptr;
    // joint posterior draws: the (N + M)^2 matrix and its factorisation context, owned by draws.hip (SampleWs); sample_release()
    void* sample = nullptr;
    // integrated variance reduction: W = L^-1 K*, the lower tiles of the posterior covariance on the test grid and the partial
    // column sums, owned by ivr.hip (IvrWs); ivr_release()
    void* ivr = nullptr;
    DevBuf<double> refine;          // residual, correction and partial sums of the refinement (fp32 handles)
    // leave-one-out objective (loograd.hip: loo_obj_ensure): q, sqrt(omega), r -- 3 x np, released with the matrices -- and the
    // tile list of C C^T for loo_tiles_nb block rows
    DevBuf<double> loo_vec;
    DevBuf<TileDesc> loo_tiles;
    int loo_tiles_nb = 0;
    int fp32 = 0;                   // 1: the N x N matrices of the exact-GP path are float (gpimhip_set_precision)
    // GPIMHIP_NO_FUSED_FINALIZE as the current public call found it (api.hip: read_finalize_knob, at the top of every entry that
    // reaches loss_grad_at_u): theta carry, fused finalize and deferred alpha all derive from this one read
    bool no_fused_finalize = false;
};

template <typename T> int DevBuf<T>::alloc(gpimhip_ctx* h, int64_t count, const char* what) {
    void* q = nullptr;
    hipError_t e = hipMalloc(&q, (size_t)count * sizeof(T));
    if (e != hipSuccess) {
        if (what) (void)hipGetLastError();
        gpim_set_error(what ? std::string(what) : std::string("hipMalloc failed: ") + hipGetErrorString(e));
        return GPIMHIP_E_NOMEM;
    }
    p = (T*)q;
    cap = count;
    h->bytes += cap * (int64_t)sizeof(T);
    return GPIMHIP_OK;
}
template <typename T> void DevBuf<T>::release(gpimhip_ctx* h) {
    if (p) {
        (void)hipFree(p);
        h->bytes -= cap * (int64_t)sizeof(T);
    }
    p = nullptr;
    cap = 0;
}
template <typename T> int DevBuf<T>::grow(gpimhip_ctx* h, int64_t want) {
    if (cap >= want) return GPIMHIP_OK;
    HIP_TRY(hipStreamSynchronize(h->stream));
    release(h);
    return alloc(h, want);
}
template <typename... Bufs> static inline void dev_release(gpimhip_ctx* h, Bufs&... bufs) { (bufs.release(h), ...); }

// h->nbatch = nbatch until the end of the scope, then what it was before (a launch of ONE problem in a call on a batch)
struct BatchScope {
    gpimhip_ctx* h; int prev;
    BatchScope(gpimhip_ctx* h_, int nbatch) : h(h_), prev(h_->nbatch) { h->nbatch = nbatch; }
    ~BatchScope() { h->nbatch = prev; }
};

// entry points outside the exact-GP path keep their matrices in double
#define FP64_ONLY(h)                                                                                      \
    do {                                                                                                  \
        if ((h) && (h)->fp32) {                                                                           \
            gpim_set_error("this entry point needs a double-precision handle (gpimhip_set_precision(h, 64))"); \
            return GPIMHIP_E_BADARG;                                                                      \
        }                                                                                                 \
    } while (0)

static inline int64_t pad_to(int64_t n, int64_t m) { return (n + m - 1) / m * m; }
// Carves pieces off one arena of doubles.  Every piece starts at an even offset (16-byte alignment), i.e. the piece before
// it is rounded up to an even count; `used` is the total once the last piece is taken.  With base == nullptr take() only
// counts -- the sizing pass, before the buffer exists; the same list of takes with the buffer then hands out the pointers.
struct Carve {
    double* base;
    int64_t used = 0;
    explicit Carve(double* b) : base(b) {}
    template <typename T = double> T* take(int64_t doubles) {
        const int64_t off = (used + 1) & ~(int64_t)1;
        used = off + doubles;
        return base ? (T*)(base + off) : nullptr;
    }
};
// GemmArgs::rag for an exact-GP matrix of N valid rows padded to np with the identity
static inline int rag_of(int64_t N, int64_t np) {
    const int64_t last = N - (np - NB);
    return (np >= 2 * NB && last > 0 && last <= 64) ? (int)(np / NB) : 0;
}

// stage timers (bench.py): 0 factorisation (with the part of the inverse its launches host), 1 rest of the triangular
// inverse, 2 K^-1 product (one tile-engine launch), 3 predictive-variance product
struct StageTimer {
    gpimhip_ctx* h; int stage; hipEvent_t e1 = nullptr;
    StageTimer(gpimhip_ctx* h_, int s) : h(h_), stage(s) {
        if (!h->timing) return;
        hipEvent_t e0;
        if (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess) { e1 = nullptr; return; }
        (void)hipEventRecord(e0, h->stream);
        h->ev[stage].push_back({e0, e1});
    }
    ~StageTimer() { if (e1) (void)hipEventRecord(e1, h->stream); }
};

// ---- drivers shared between translation units ----
// row chunks of the triangular transposed mat-vec alpha = L^-T z (engine.hip: gemv_t_tri_kernel): ~np / 32 rows, a multiple
// of 128 between 128 and 1024; a function of the matrix order alone (a problem gives the same bits alone and in a batch)
static inline int gemv_tri_rc(int64_t np) {
    const int64_t rc = ((np / 32 + NB - 1) / NB) * NB;
    return (int)(rc < NB ? NB : (rc > 1024 ? 1024 : rc));
}
static inline int gemv_tri_chunks(int64_t np) { return (int)((np + gemv_tri_rc(np) - 1) / gemv_tri_rc(np)); }
// api.hip
#define OUTER_W 4    // outer Cholesky panel = 4 x 128 columns
int ws_ensure(gpimhip_ctx* h, int64_t N);
int ws_ensure_b(gpimhip_ctx* h, int64_t N, int B, int padded, bool matrices = true);
int ws_ensure_padded(gpimhip_ctx* h, int64_t N);
int ws_ensure_predict(gpimhip_ctx* h, int64_t np, int64_t mc);
int deal_chunk(int ntiles = 1 << 30);
void tri_tiles(std::vector<TileDesc>& tl, int nbr, int nc, bool lower);     // (with the tile-list builders of api.hip)
void lower_patch_order(std::vector<TileDesc>& out, int lo, int hi, int kb0, int kb1);
int model_state_at_u(gpimhip_ctx* h, const gpimhip_model_t* m, const double* X, int64_t x_bs, const double* y, int64_t N,
                     int B, const double* u);
// z = L^-1 ypad and alpha = L^-T z from L^-1 in h->A; K(u) -> L^-1 in h->A, then the two (api.hip has the details)
int solve_vectors(gpimhip_ctx* h, const gpimhip_model_t* m, const double* X, int64_t x_bs, int64_t N, bool defer_alpha = false);
int factor_at_u(gpimhip_ctx* h, const gpimhip_model_t* m, const double* X, int64_t x_bs, int64_t N, const double* u,
                bool theta_current = false, bool defer_alpha = false);
// One chunk of predict_cols: test points [m0, m0 + cnt) starting at Z, cpad = cnt padded to 128.  The slab h->Ks has the
// leading dimension kld (np * kld between problems); mean_tmp and colpart have the stride mcap.  For the finisher: the
// variance is wanted for the first nvar points of the chunk (colpart holds no more; 0: none), and with a border radd holds
// the column sums of squares to add back (BorderWs::rsq)
struct PredictChunk { const double* Z; int64_t m0, cnt, cpad, mcap, kld, nvar; const double* radd; };
// What a model family supplies to predict_cols: its M test points Xs of `dim` coordinates, and per chunk
//   slab     K* of the chunk into h->Ks, for all problems of the batch
//   mean     (optional) runs once mean_tmp = K*^T alpha is there, before the variance product is launched: the dense
//            finishers write their mean here
//   finish   the chunk's mean and variance into the caller's outputs from mean_tmp / colpart / radd
// fused (optional): the family may take the single launch of predict.hip where it fits, this is it.  var_on_domain: the
// finisher sums reflection blocks and honours ReflArgs::var_count
struct PredictFamily {
    int dim; const double* Xs; int64_t M;
    bool var_on_domain = false;
    std::function<int()> fused;
    std::function<int(const PredictChunk&)> slab, mean, finish;
};
int64_t predict_chunk_cols(int64_t np, int B, int64_t M);
int predict_cols(gpimhip_ctx* h, const PredictFamily& f, int64_t N, int B);
PredictFamily stationary_family(gpimhip_ctx* h, const gpimhip_model_t* m, const double* X, int64_t x_bs, int64_t N, int B,
                                const double* Xs, int64_t M, double* mean_out, double* var_out);
// draws.hip
void sample_release(gpimhip_ctx* h);
int64_t sample_bytes(const gpimhip_ctx* h);
// ivr.hip
void ivr_release(gpimhip_ctx* h);
// The preamble of a fit call: info[1] = "completed" = huge until a failure, fit_completed = T and, for T > 0, the
// bias-correction table, then the Adam state (adam_bytes at adam_m and, where the two halves are buffers of their own, at
// adam_v) and the iteration counter zeroed.  What a fit of T == 0 returns is the caller's business.
int fit_prologue(gpimhip_ctx* h, double lr, int T, double* adam_m, double* adam_v, size_t adam_bytes, int32_t* iter);
int plan_ensure(gpimhip_ctx* h, int nb);
int check_model(const gpimhip_model_t* m);
int launch_potrf(gpimhip_ctx* h, double* A, int64_t np, int64_t ld, int32_t* info);
int launch_trtri(gpimhip_ctx* h, double* A, double* Tm, int64_t np, int64_t ld);
int launch_potrf_inv(gpimhip_ctx* h, double* A, double* Tm, int64_t np, int64_t ld, int32_t* info, int rag);
int launch_lauum(gpimhip_ctx* h, const double* A, double* B, int64_t np, int64_t ld, int rag);
int upload_bc_table(gpimhip_ctx* h, double lr, int T);
int finish_and_check(gpimhip_ctx* h);
// The two ways in which the training loops differ (run_fit_iterations).  Both are observable -- they decide which launches
// and copies a fit enqueues -- so each trainer keeps the row it had:
//   dense_gates  the dense engine (exact / batched, multi-output, spectral mixture) replays a graph only with stage timing
//                off (the timers record events around single launches) and below EAGER_MIN_PANELS outer panels (beyond,
//                launch cost no longer matters).  The Kronecker and sparse trainers have neither stage timers nor a large-N
//                regime of many long launches: any fit of T >= 8 is replayed.
//   run_ahead    bounded run-ahead (api.hip: RunAhead) relies on the finalize kernel freezing u, the Adam state and the
//                history at a failed factorisation; the Kronecker and sparse finalize kernels have not been checked for
//                that, so their loops enqueue all T iterations.
struct FitLoop { bool dense_gates, run_ahead; };
static const FitLoop FIT_LOOP_DENSE = {true, true}, FIT_LOOP_PLAIN = {false, false};
// Runs `iteration` (which enqueues one Adam iteration on h->stream and returns a GPIMHIP_* code) T times -- as one captured
// hipGraph replayed T times where FitLoop allows, else launch by launch -- and returns finish_and_check().  During the
// capture h->stream is the capture stream: the body must not synchronise, allocate or touch the legacy stream.
int run_fit_iterations(gpimhip_ctx* h, int T, FitLoop loop, const std::function<int()>& iteration);
// vfe.hip, kron.hip, pkrongp.hip
void vfe_release(gpimhip_ctx* h);
void kron_release(gpimhip_ctx* h);
void pkron_release(gpimhip_ctx* h);
// cholstep.hip, cholstep32.hip
int launch_potrf_steps(gpimhip_ctx* h, double* A, int64_t np, int64_t ld, int32_t* info, double* Tm = nullptr, int rag = 0);
int launch_potrf_steps_f32(gpimhip_ctx* h, double* A, int64_t np, int64_t ld, int32_t* info);
void step_plan_release(gpimhip_ctx* h);
int step_plan_ensure(gpimhip_ctx* h, int nb);
int step_plan_ensure_inv(gpimhip_ctx* h, int nb);
int step_plan_ensure_pair(gpimhip_ctx* h, int nb);      // (nothing to do where the paired schedule does not apply)
int launch_panel_chain(gpimhip_ctx* h, double* A, int64_t ld, int p0, int p1, int nb, const TileDesc* tiles,
                       const PlanRange* colfill, int32_t* info);
// distgp.hip
void dist_plan_release(gpimhip_ctx* h);
// distops.hip
int launch_dist_pack(gpimhip_ctx* h, const double* P, int64_t ldp, int64_t r0, int64_t np, int w, const double* dinv,
                     int nblk, double* buf, int64_t ldb);
int launch_colsumsq_acc(gpimhip_ctx* h, const double* W, int64_t ldw, int rows, int64_t m, double* q);
int launch_dist_trsv(gpimhip_ctx* h, const double* P, int64_t ld, const double* D, int nblk, int backward, const double* r0,
                     const double* r1, double* out);
int launch_dist_rows_acc(gpimhip_ctx* h, const double* A, int64_t ld, int64_t rows, int w, const double* x, double* acc);
// the same for a group of ncols (1 .. 8) columns per sweep, column c at its pointer + c * (its column stride): draws.hip
// blocks_solve.  r1: nch chunks (stride r1_chs) of partial sums, added in their order and taken off r0; part of
// launch_gemv_t_multi: gemv_t_multi_chunks(nrows) x multi_group_width(ncols) x 512 doubles.
#define GEMV_T_MULTI_RC 1024
static inline int gemv_t_multi_chunks(int64_t nrows) { return (int)((nrows + GEMV_T_MULTI_RC - 1) / GEMV_T_MULTI_RC); }
int multi_group_width(int ncols);
int launch_dist_trsv_multi(gpimhip_ctx* h, const double* P, int64_t ld, const double* D, int nblk, int backward, const double* r0,
                           int64_t r0_cs, const double* r1, int64_t r1_cs, int64_t r1_chs, int nch, int ncols, double* out,
                           int64_t out_cs);
int launch_dist_rows_acc_multi(gpimhip_ctx* h, const double* A, int64_t ld, int64_t rows, int w, const double* x, int64_t x_cs,
                               int ncols, double* acc, int64_t acc_cs);
int launch_gemv_t_multi(gpimhip_ctx* h, const double* A, int64_t ld, int64_t nrows, int w, const double* x, int64_t x_cs,
                        int ncols, double* part);
// engine.hip
int launch_theta_raw(gpimhip_ctx* h, const gpimhip_model_t* m, const double* raw);
int launch_kmat(gpimhip_ctx* h, const gpimhip_model_t* m, const double* X, int64_t N, const double* Z,
                int64_t M, const ThetaDev* theta, double diag_add, int use_theta_diag, double* out,
                int64_t ld, int64_t rows_pad, int64_t cols_pad, int sym, int lower_only, int64_t x_bs,
                int64_t z_bs, int64_t out_bs);
int launch_pad_copy(gpimhip_ctx* h, const double* src, int64_t n, double* dst, int64_t np);
int launch_diag_inv_copy(gpimhip_ctx* h, double* A, int64_t ld, int nb);
int launch_pad_matrix_in(gpimhip_ctx* h, const double* src, int64_t n, int64_t ld, double* dst, int64_t np);
int launch_pad_matrix_out_lower(gpimhip_ctx* h, const double* src, int64_t np, double* dst, int64_t n, int64_t ld);
int launch_trmv_lower(gpimhip_ctx* h, const double* L, int64_t ld, int64_t np, const double* y, double* z);
int launch_gemv_t(gpimhip_ctx* h, const double* A, int64_t ld, int64_t nrows, int64_t ncols, const double* x,
                  double* out, int tri, int64_t a_bs, int64_t x_bs, int64_t o_bs);
int launch_kres(gpimhip_ctx* h, const gpimhip_model_t* m, const double* X, int64_t x_bs, int64_t N, double* scratch,
                int S, double* res);
int launch_axpy(gpimhip_ctx* h, double* x, const double* d, int64_t n);
int launch_gemv_t_tri(gpimhip_ctx* h, const double* A, int64_t ld, int64_t np, const double* x, double* part, double* out);
int launch_kmat_refl(gpimhip_ctx* h, const gpimhip_model_t* m, const double* X, int64_t N, const double* Z, int64_t M,
                     const ThetaDev* theta, double* out, int64_t ld, int64_t rows_pad, int64_t cols_pad, int sym, int64_t x_bs,
                     int64_t z_bs, int64_t out_bs, double scale);
int launch_add_diag_theta(gpimhip_ctx* h, double* out, int64_t ld, int64_t row0, int64_t n, int64_t npad);
int launch_theta(gpimhip_ctx* h, const gpimhip_model_t* m, const double* u);
// grad.hip
int launch_grad_reduce(gpimhip_ctx* h, const gpimhip_model_t* m, const double* Kinv, int64_t ld,
                       const double* X, int64_t N, int nb, const double* alpha, int64_t x_bs);
// the gradient contraction with the finalize step in its last workgroup (grad.hip: FinFused), and the step as a launch of
// its own.  carry_theta: the theta of the stepped parameters replaces h->theta (the next iteration skips its theta launch).
// The fused form contracts K^-1 in h->B with alpha from h->alpha, or (alpha_deferred) from the row-chunk sums in h->gemv_part.
int launch_grad_reduce_fin(gpimhip_ctx* h, const gpimhip_model_t* m, const double* X, int64_t x_bs, int64_t N,
                           bool alpha_deferred, double* u, int do_adam, AdamStep st, const FinalizeOut& out, int carry_theta);
int launch_finalize(gpimhip_ctx* h, const gpimhip_model_t* m, int64_t N, int64_t np, double* u, int do_adam,
                    AdamStep st, const FinalizeOut& out, int carry_theta = 0);
int launch_finalize_vec(gpimhip_ctx* h, const gpimhip_model_t* m, int64_t N, int64_t np, double* u, int do_adam, AdamStep st,
                        const FinalizeOut& out, int carry_theta, const double* z, const double* zb);
// grad.hip, loograd.hip (the leave-one-out objective: one double-precision problem of the dense engine)
int launch_grad_reduce_loo(gpimhip_ctx* h, const gpimhip_model_t* m, const double* Kinv, int64_t ld, const double* X, int64_t N,
                           int nb, const double* alpha, const double* rvec);
int loo_obj_ensure(gpimhip_ctx* h);
int loo_grad_at_u(gpimhip_ctx* h, const gpimhip_model_t* m, const double* X, int64_t N, double* u, int do_adam, AdamStep st,
                  const FinalizeOut& out, bool theta_carried);
// grad.hip (distributed training, reflection blocks)
int launch_grad_reduce_tiles(gpimhip_ctx* h, const gpimhip_model_t* m, const double* Kinv, int64_t ld, const double* X,
                             int64_t N, int64_t np, const double* alpha, const TileDesc* tiles, int ntile, double* part);
int launch_sum7(gpimhip_ctx* h, const double* part, int ntile, double* S);
int launch_grad_reduce_refl(gpimhip_ctx* h, const gpimhip_model_t* m, const double* Kinv, int64_t ld, const double* X,
                            int64_t N, int nb, const double* alpha, int64_t x_bs);
int launch_finalize_coupled(gpimhip_ctx* h, const gpimhip_model_t* m, int64_t N, int64_t np, double* u, int do_adam,
                            AdamStep st, const FinalizeOut& out, const double* border_scal = nullptr);
int launch_coupled_sums(gpimhip_ctx* h, int64_t np, double* out11);
int launch_dist_finalize_dev(gpimhip_ctx* h, const gpimhip_model_t* m, int64_t N, const double* red, const double* quad,
                             double* u, int do_adam, AdamStep st, double* loss_out, double* grad_out, double* hist_row);
int launch_dist_finalize(gpimhip_ctx* h, const gpimhip_model_t* m, int64_t N, const double* S, double q2, double lg,
                         double* u, int do_adam, AdamStep st, double* loss_out, double* grad_out, double* hist_row);
// predict.hip (epilogues of the slab path)
int launch_predict_var(gpimhip_ctx* h, int64_t ldp, int nb, int64_t m0, int64_t mcount, double* var_out, int64_t M);
int launch_copy_slice(gpimhip_ctx* h, const double* src, double* dst, int64_t n, int64_t s_bs, int64_t d_bs);
int launch_predict_coupled(gpimhip_ctx* h, int64_t ldp, int nb, int64_t m0, int64_t mcount, int64_t nvar, int64_t mean_bs,
                           double* mean_out, double* var_out, const double* radd = nullptr);
// predict.hip (leave-one-out cross-validation).  What loo_finish_kernel reads for its n points: the observations y, and
// per problem d = diag(S^-1) as the row-chunk partial sums of launch_colsq_tri (nR chunks of rc rows of a matrix of order
// np; nR = 1 with rc = INT_MAX: d itself, np apart) and alpha (np apart).  B == 0: one problem, point i is its row i.
// B > 0: the B reflection blocks of Nq points -- wts (B x Nq, or null), rep[i] the row of point i's representative and
// sgn[i] the reflections that take the representative to i (bit j: the j-th reflected axis, the numbering of the blocks)
struct LooSrc {
    const double* y; const double* diag_part; int nR, rc; int64_t np; const double* alpha;
    int B; const double* wts; const int32_t* rep; const int32_t* sgn; int64_t Nq;
};
static inline int loo_blocks(int64_t n) { return n > 1024 * 256 ? 1024 : (int)((n + 255) / 256); }
int launch_colsq_tri(gpimhip_ctx* h, const double* A, int64_t ld, int64_t np, int64_t N, double* part);
int launch_loo_finish(gpimhip_ctx* h, const LooSrc& s, int64_t n, const ThetaDev* theta, double* part, double* mean_out,
                      double* var_out, double* score_out);
// select.hip
int launch_acq(gpimhip_ctx* h, int kind, const double* mean, const double* sd, int64_t M, double p0, double p1,
               const double* mask, double* out);
int launch_nanmax(gpimhip_ctx* h, const double* x, int64_t n, double* out);
int launch_topk(gpimhip_ctx* h, const double* x, int64_t M, int k, int keep_nan, double* vals, int64_t* idx,
                int64_t* count);
int launch_topk_radix(gpimhip_ctx* h, const double* x, int64_t M, int k, int keep_nan, double* vals, int64_t* idx,
                      int64_t* count);
int launch_nanmax_two_stage(gpimhip_ctx* h, const double* x, int64_t n, double* out);
int launch_thin_batch(gpimhip_ctx* h, const double* vals, const int64_t* flat, int n, int d, const int64_t* shape,
                      double dscale, int max_out, int32_t* keep_out, int32_t* nkeep_out);
size_t sel_scratch_bytes();
int sel_scratch_ensure(gpimhip_ctx* h);         // (acquire.hip) h->sel_scratch, allocated once
// smalln.hip
int launch_fit_small(gpimhip_ctx* h, const gpimhip_model_t* m, const double* X, int64_t x_bs, const double* y,
                     int N, double* u, const double* lr_over_bc1, const double* bc2_sqrt, int T, double* hist,
                     double* loss, double* grad);
// predict.hip (its fused launch and the sweep behind the slab path: acq.hpp)
bool fused_predict_fits(int64_t np);


enum GemmEpi { EPI_STORE = 0, EPI_COLSUMSQ = 1 };
struct GemmArgs {
    const double* A; int64_t lda; int a_roff, a_coff;
    const double* B; int64_t ldb; int b_roff, b_coff;
    double* C; int64_t ldc; int c_roff, c_coff;
    double alpha, beta;
    const TileDesc* tiles; int ntiles;
    int cj_max;                            // > 0: tiles with cj >= cj_max are skipped (structurally zero columns)
    int cmap;                              // C's block column is the tile's kb0 field (operand columns stay cj): output
                                           // stored at local columns (distributed layouts); needs kfix0 / kfix1
    int chunk;                             // XCD dealing: 0 = contiguous slices, >0 = round-robin chunks
    int inplace;                           // C aliases an operand tile (panel solve): one workgroup must own the whole tile
    // INVARIANT of ragged launches: the padding rows of the last block row of Tm and B (workspace matrices) are zeroed at
    // allocation only and never written by a rag launch; every reader of Tm / B under rag skips them too (X phase with
    // kb1 == nb, lauum with krev, the COLSUMSQ predict path).  Non-rag fits and the sparse model on the same handle write
    // those rows fully, so after them they hold stale data: a NEW consumer of Tm or B (a full-np reduction over K^-1, say)
    // must either skip the padding rows or zero them first.
    int rag;                               // > 0: block rag - 1 (the LAST block of the matrix order) holds at most 64 valid
                                           // rows / columns, the rest is identity padding: output rows >= 64 of block row
                                           // rag - 1 and the k-steps >= 64 of a range ending with that block are structurally
                                           // zero and skipped (exact GP with (N - 1) % 128 < 64: rag_of())
    int krev;                              // walk each tile's k-range from its end (ranges sharing their upper end)
    int kfix0, kfix1;                      // when kfix1 > kfix0: every tile uses this k-block range (its own is ignored)
    int rect_rows, rect_cols;              // rect_cols > 0: no list -- the launch covers the rect_rows x rect_cols tiles of a
                                           // rectangle (ntiles = their product) in strips of eight rows, column by column
                                           // inside a strip: 64 consecutive tiles are an 8 x 8 patch (with chunk = 64 one
                                           // patch per XCD at a time: 8 + 8 operand panels for 64 tiles); needs kfix0 / kfix1
    double* colpart; int64_t ld_colpart;   // EPI_COLSUMSQ: colpart[ci*ld + cj*128 + col]
    double* C2;                            // != nullptr: the output tile is ALSO stored here as a dense 128 x 128 block (set per tile by
                                           // the Cholesky step kernel: the copy of A[j+1, j] that the fused panel-solve / diagonal-update launch reads)
    int shape_div;                         // > 1: the launch shape is chosen for ntiles * batch / shape_div tiles (the sparse model's
                                           // lock-step batches: every model gets the tile shapes -- hence the bits -- of its own launch)
    int64_t sA, sB, sC, sColpart;          // per-problem (blockIdx.y) strides in elements
    int bshift;                            // operand B of problem p is that of p >> bshift (double-precision engine: the 2^r blocks
                                           // of one task of the multi-output GP share their border's L_S^-1; api.hip: border_iter)
};
int launch_gemm(gpimhip_ctx* h, bool a_km, bool b_km, int epi, const GemmArgs& g);
int launch_gemm_f32(gpimhip_ctx* h, bool a_km, bool b_km, int epi, const GemmArgs& g);   // gemm32.hip
GemmArgs gemm_args(const double* A, int64_t lda, const double* B, int64_t ldb, double* C, int64_t ldc, double alpha, double beta,
                   const TileDesc* tiles, int n, int64_t rows);                           // api.hip

// The workgroup shape of a tile-engine launch (NW waves on a TSM x TSN part of each 128 x 128 tile; gemm_body.hpp), chosen
// from the launch's tile count by gemm_shape_f64 (gemm.hip) / gemm_shape_f32 (gemm_kernel.hpp, gemm32.hip); the values are
// the GPIMHIP_GEMM_SHAPE_* of gpimhip.h.  -1: nothing to launch (no tiles) or an operand layout the engine does not have.
enum GemmShape {
    GEMM_SHAPE_QUAD = GPIMHIP_GEMM_SHAPE_QUAD,          // (4,  64,  64)
    GEMM_SHAPE_ROWHALF = GPIMHIP_GEMM_SHAPE_ROWHALF,    // (8,  64, 128)
    GEMM_SHAPE_8W_LDS = GPIMHIP_GEMM_SHAPE_8W_LDS,      // (8, 128, 128) + 24 KB of dynamic LDS: one tile per CU
    GEMM_SHAPE_8W = GPIMHIP_GEMM_SHAPE_8W,              // (8, 128, 128)
    GEMM_SHAPE_4W = GPIMHIP_GEMM_SHAPE_4W               // (4, 128, 128)
};
static inline bool gemm_layout_ok(bool a_km, bool b_km, int epi) {
    if (epi == EPI_STORE) return !a_km || b_km;         // NT, NN, TN
    return epi == EPI_COLSUMSQ && !a_km && b_km;        // NN
}
int gemm_shape_f64(bool a_km, bool b_km, int epi, int64_t ntiles, int64_t batch, int shape_div, int inplace);   // gemm.hip
int gemm_shape_f32(bool a_km, bool b_km, int epi, int64_t ntiles, int64_t batch, int shape_div, int inplace);   // gemm32.hip
int gemm_tile_pos_f32(int n, int chunk, int quads, int bx, int& quad);      // gemm32.hip: the float engine's copy of gemm_tile_pos

// XCD-aware bijective remap of a launch's workgroup index to a position of its tile list (block b runs on XCD
// b % 8, in order b / 8 on that XCD).
//  chunk == 0: every XCD gets one contiguous slice of the tile list -- best L2 reuse when all
//              tiles cost the same (SYRK-shaped trailing updates).
//  chunk  > 0: the list is dealt to the XCDs in chunks of that many tiles (one 8x8 patch), back
//              and forth, so lists sorted by decreasing k-range stay balanced across XCDs.
// Host-callable for the tests of the map itself (gpimhip_gemm_tile_pos_host).  The float engine keeps a copy of its own
// (gemm_kernel.hpp: GEMM_TILE_POS_T).
template <int TSM, int TSN>
__host__ __device__ __forceinline__ int gemm_tile_pos(int n, int chunk, int bx, int& quad) {
    constexpr int QUADS = (128 / TSM) * (128 / TSN);    // workgroups per 128x128 tile
    const int b = bx / QUADS;
    quad = bx % QUADS;
    if (QUADS > 1) return b;
    if (chunk == 0) {
        const int q = n >> 3, r = n & 7, x = b & 7, yy = b >> 3;
        return (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + yy;
    }
    const int C = chunk, full = (n / (8 * C)) * (8 * C);
    if (b < full) {
        // serpentine: odd rounds deal in reverse, so that on a list sorted by cost no XCD always
        // gets the most expensive chunk of the round (16 % spread between XCD 0 and 7 otherwise)
        const int x = b & 7, y = b >> 3, round = y / C;
        return (round * 8 + ((round & 1) ? 7 - x : x)) * C + (y % C);
    }
    return b;
}
// Position p of a rectangle launch (GemmArgs::rect_rows / rect_cols) -> its tile: strips of eight rows, column by column
// inside a strip (the last strip may be lower).
__host__ __device__ __forceinline__ void gemm_rect_tile(int rect_rows, int rect_cols, int p, int& ci, int& cj) {
    const int per = 8 * rect_cols, s = p / per, q = p - s * per, left = rect_rows - 8 * s, rows_here = left < 8 ? left : 8;
    ci = 8 * s + q % rows_here;
    cj = q / rows_here;
}
