// api.hip -- host side of libgpimhip: workspace, launch plans, blocked-algorithm drivers and the
// extern "C" entry points declared in include/gpimhip.h.  The posterior draws (gpimhip_sample_*) have their drivers and entries
// in draws.hip, the spectral-mixture GP (gpimhip_*_sm*) in smgp.hip, the multi-output GP (gpimhip_*_vgp*) in vgpgp.hip, the
// Kronecker model (gpimhip_*_kron) in kron.hip, the dense-by-Kronecker blocks (gpimhip_*_pkron) in pkrongp.hip and the
// multi-GPU panel drivers (gpimhip_dist_*, gpimhip_matvec_t) in distgp.hip; the iteration of the leave-one-out objective
// (loo_grad_at_u, behind loss_grad_at_u) is in loograd.hip.
#include <math.h>
#include <stdio.h>
#include <string.h>
#include <stdlib.h>
#include <algorithm>
#include <chrono>
#include <atomic>
#include <mutex>
#include "common.hpp"
#include "border.hpp"
#include "vgp.hpp"
#include "sm.hpp"
#include "sample.hpp"
#include "acq.hpp"

static thread_local std::string g_err;
void gpim_set_error(const std::string& s) { g_err = s; }

// XCD dealing chunk for lists sorted by decreasing cost: 64-tile chunks keep neighbouring tiles (shared operand
// panels) on one XCD's L2, but a list of a few hundred tiles dealt 64 at a time puts all the longest tiles on
// XCD 0 (N = 4206: K^-1 product 0.92 -> 0.72 ms with single-tile dealing); grow the chunk with the list.
int deal_chunk(int ntiles) { return std::max(1, std::min(64, ntiles / 512)); }
// "large N": from 12 outer panels (6144 unknowns) on an iteration is enqueued launch by launch on the caller's stream
// (below: one captured iteration is replayed; its ~100 launches are then one host call)
#define EAGER_MIN_PANELS 12

// ------------------------------------------------------------------------------------------
// workspace
// ------------------------------------------------------------------------------------------

// the N x N matrices hold floats on a single-precision handle: same element counts, half the doubles
static inline int64_t mat_doubles(const gpimhip_ctx* h, int64_t elements) { return h->fp32 ? (elements + 1) / 2 : elements; }

static void ws_release_matrix(gpimhip_ctx* h) {
    dev_release(h, h->A, h->B, h->Tm, h->dinv, h->dinvB, h->pcopy, h->ypad, h->z, h->alpha, h->logdet_part, h->grad_part,
                h->gemv_part, h->fin_counter, h->theta, h->adam_m, h->adam_v, h->iter, h->loo_vec);
    h->np = 0;
    h->ws_batch = 0;
}

// Workspace for B problems of N observations processed in lock-step (all per-problem buffers are
// stacked: problem b lives at base + b * size).
// padded != 0: rows of the np x np matrices are np + 16 doubles apart.  With ld = np = 2^k every row
// of a 128-column panel maps to the same L2 sets (row stride 2^(k+3) bytes) and tiles that share a
// panel evict each other's lines; one extra cache line per row spreads the rows over the sets.
// matrices == false: only what the diagonal-block kernels and the launch plan need (dinv, log-det partials,
// theta, Adam state) -- the distributed factorisation keeps its share of the matrix in caller-owned storage
// and never needs the three np x np buffers (3 x 32 GiB at N = 65536).
int ws_ensure_b(gpimhip_ctx* h, int64_t N, int B, int padded, bool matrices) {
    const int64_t np = pad_to(std::max<int64_t>(N, 1), NB);
    const int64_t ld = np + ((padded && np >= 1024) ? (h->fp32 ? 32 : 16) : 0);      // one extra 128-byte line per row
    if (np == h->np && B == h->ws_batch && ld == h->ld && (h->A != nullptr || !matrices)) return GPIMHIP_OK;
    HIP_TRY(hipStreamSynchronize(h->stream));
    ws_release_matrix(h);
    const int64_t nb = np / NB;
    // (if an allocation in the middle fails, ws_release_matrix() frees what exists)
    h->np = np;
    h->ws_batch = B;
    h->ld = ld;
    int rc = GPIMHIP_OK;
    if ((matrices && ((rc = h->A.alloc(h, mat_doubles(h, B * np * ld))) ||
                      (rc = h->B.alloc(h, mat_doubles(h, B * np * ld))) ||
                      (rc = h->Tm.alloc(h, mat_doubles(h, B * np * ld))))) ||
        (rc = h->dinv.alloc(h, mat_doubles(h, B * nb * NB * NB))) ||
        (rc = h->dinvB.alloc(h, B * nb * NB * NB)) ||
        (rc = h->pcopy.alloc(h, (int64_t)B * NB * NB)) ||
        (rc = h->ypad.alloc(h, B * np)) || (rc = h->z.alloc(h, B * np)) ||
        (rc = h->alpha.alloc(h, B * np)) || (rc = h->logdet_part.alloc(h, B * nb)) ||
        (rc = h->grad_part.alloc(h, B * nb * (nb + 1) / 2 * 8)) || (rc = h->gemv_part.alloc(h, B * (int64_t)gemv_tri_chunks(np) * np)) || (rc = h->fin_counter.alloc(h, (int64_t)B)) || (rc = h->theta.alloc(h, (int64_t)B)) ||
        (rc = h->adam_m.alloc(h, (int64_t)B * MAXP)) || (rc = h->adam_v.alloc(h, (int64_t)B * MAXP)) ||
        (rc = h->iter.alloc(h, (int64_t)B))) {
        ws_release_matrix(h);
        return rc;
    }
    HIP_TRY(hipMemsetAsync(h->fin_counter, 0, (size_t)B * sizeof(uint32_t), h->stream));   // (the last workgroups reset them)
    if (matrices) {
        // Tm / B: a ragged last block (GemmArgs::rag) never writes the rows of its identity padding
        HIP_TRY(hipMemsetAsync(h->Tm, 0, (size_t)mat_doubles(h, B * np * ld) * sizeof(double), h->stream));
        HIP_TRY(hipMemsetAsync(h->B, 0, (size_t)mat_doubles(h, B * np * ld) * sizeof(double), h->stream));
    }
    if (h->fp32 && h->refine.cap < 10 * (int64_t)B * np) {
        h->refine.release(h);           // (no launch still reads it: the stream was synchronised above)
        if ((rc = h->refine.alloc(h, 10 * (int64_t)B * np))) {
            ws_release_matrix(h);       // the next call with this N must not take the early return without it
            return rc;
        }
    }
    // launch plans of the single-GPU path (built here: building one synchronises the stream, which a graph
    // capture does not allow); the distributed factorisation has its own (gpimhip_dist_setup)
    if (matrices) {
        rc = plan_ensure(h, (int)nb);
        // fit / predict invert the factor in the factorisation's launches (double precision); float matrices and
        // gpimhip_potrf use the plain plan, which is built on first use (never inside a capture)
        if (rc == GPIMHIP_OK) rc = h->fp32 ? step_plan_ensure(h, (int)nb) : step_plan_ensure_inv(h, (int)nb);
        if (rc == GPIMHIP_OK && !h->fp32) rc = step_plan_ensure_pair(h, (int)nb);
        if (rc != GPIMHIP_OK) { ws_release_matrix(h); return rc; }     // (a later call must not find buffers without plans)
    }
    return GPIMHIP_OK;
}
int ws_ensure(gpimhip_ctx* h, int64_t N) { return ws_ensure_b(h, N, h->nbatch, 0); }
int ws_ensure_padded(gpimhip_ctx* h, int64_t N) { return ws_ensure_b(h, N, h->nbatch, 1); }

static void ws_release_predict(gpimhip_ctx* h) {
    dev_release(h, h->Ks, h->colpart, h->mean_tmp);
    for (auto& pl : h->pred_lists) pl.tiles.release(h);
    h->pred_lists.clear();
    h->pred_tiles = nullptr;
    h->pred_ntiles = 0;
    h->ks_rows = h->ks_cols = 0;
    h->ks_batch = 0;
}

// Prediction workspace for slabs of up to mc test points.  Grow-only in mc: a Bayesian-optimisation step
// alternates between the full grid and the handful of observed points, and re-allocating the slab on every
// switch costs more than the prediction itself.  Buffers are laid out for the capacity h->ks_cols (row
// stride of the slab: capacity + 16 doubles -- no power-of-two stride); the tile list of the variance
// product depends on the number of column blocks actually used and is cached per size.
int ws_ensure_predict(gpimhip_ctx* h, int64_t np, int64_t mc) {
    const int B = h->nbatch;
    if (!(h->ks_rows == np && h->ks_batch == B && mc <= h->ks_cols)) {
        HIP_TRY(hipStreamSynchronize(h->stream));
        const int64_t cap = (h->ks_rows == np && h->ks_batch == B) ? std::max(mc, h->ks_cols) : mc;
        ws_release_predict(h);
        h->ks_rows = np;
        h->ks_cols = cap;
        h->ks_batch = B;
        int rc = GPIMHIP_OK;
        if ((rc = h->Ks.alloc(h, mat_doubles(h, B * np * (cap + 16)))) || (rc = h->colpart.alloc(h, B * (np / NB) * cap)) ||
            (rc = h->mean_tmp.alloc(h, B * cap))) {
            ws_release_predict(h);
            return rc;
        }
    }
    const int nb = (int)(np / NB), nc = (int)(mc / NB);
    for (auto& pl : h->pred_lists)
        if (pl.nc == nc) {
            h->pred_tiles = pl.tiles;
            h->pred_ntiles = pl.tiles.cap;
            return GPIMHIP_OK;
        }
    // tile list of the variance product W = L^-1 K*: 8x8 patches, longest k-ranges first
    std::vector<TileDesc> tl;
    tl.reserve((size_t)nb * nc);
    for (int ig = (nb - 1) / 8; ig >= 0; --ig)
        for (int jg = 0; jg <= (nc - 1) / 8; ++jg)
            for (int ci = std::min(nb - 1, ig * 8 + 7); ci >= ig * 8; --ci)
                for (int cj = jg * 8; cj < std::min(nc, jg * 8 + 8); ++cj) tl.push_back({ci, cj, 0, ci + 1});
    gpimhip_ctx::PredList pl{nc, {}};
    GP_TRY(pl.tiles.alloc(h, (int64_t)tl.size()));
    // (async + stream sync rather than hipMemcpy: the latter serialises against the legacy stream and is
    // illegal while another thread captures a graph)
    HIP_TRY(hipMemcpyAsync(pl.tiles, tl.data(), tl.size() * sizeof(TileDesc), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    h->pred_lists.push_back(pl);
    h->pred_tiles = pl.tiles;
    h->pred_ntiles = pl.tiles.cap;
    return GPIMHIP_OK;
}

// ------------------------------------------------------------------------------------------
// launch plans (tile lists) for a matrix of nb x nb blocks
// ------------------------------------------------------------------------------------------
void lower_patch_order(std::vector<TileDesc>& out, int lo, int hi, int kb0, int kb1) {
    // lower-triangular tile set {(i,j): lo <= j <= i < hi} in 8x8 patches (operand-panel reuse in L2)
    for (int ig = lo / 8; ig <= (hi - 1) / 8; ++ig)
        for (int jg = lo / 8; jg <= ig; ++jg)
            for (int i = std::max(lo, ig * 8); i < std::min(hi, ig * 8 + 8); ++i)
                for (int j = std::max(lo, jg * 8); j < std::min(hi, jg * 8 + 8); ++j)
                    if (j <= i) out.push_back({i, j, kb0, kb1});
}

// the nbr x nc tiles of a product with a triangular factor of nbr block rows, longest k-ranges first.  lower: the k-range
// stops at the diagonal block, [0, ci], rows descending; else it starts there, [ci, nbr), rows ascending
void tri_tiles(std::vector<TileDesc>& tl, int nbr, int nc, bool lower) {
    for (int r = 0; r < nbr; ++r) {
        const int ci = lower ? nbr - 1 - r : r;
        for (int cj = 0; cj < nc; ++cj) tl.push_back(lower ? TileDesc{ci, cj, 0, ci + 1} : TileDesc{ci, cj, ci, nbr});
    }
}

// rectangular tile set rows [r0,r1) x cols [c0,c1) in 8x8 patches; krange(ci,cj) -> {kb0,kb1}
template <typename F>
static void rect_patch_order(std::vector<TileDesc>& out, int r0, int r1, int c0, int c1, bool rows_desc,
                             bool col_major, F krange) {
    // col_major: walk patch columns in the outer loop (use when the k-range depends on cj), else
    // patch rows (k-range depends on ci).  Either way consecutive patches cost about the same, so
    // dealing them round-robin to the 8 XCDs stays balanced.
    const int nrg = (r1 - r0 + 7) / 8, ncg = (c1 - c0 + 7) / 8;
    const int nouter = col_major ? ncg : nrg, ninner = col_major ? nrg : ncg;
    for (int a = 0; a < nouter; ++a)
        for (int bq = 0; bq < ninner; ++bq) {
            int ig = col_major ? bq : a, jg = col_major ? a : bq;
            if (rows_desc) ig = nrg - 1 - ig;
            for (int i = r0 + ig * 8; i < std::min(r1, r0 + ig * 8 + 8); ++i)
                for (int j = c0 + jg * 8; j < std::min(c1, c0 + jg * 8 + 8); ++j) {
                    int k0, k1;
                    krange(i, j, k0, k1);
                    out.push_back({i, j, k0, k1});
                }
        }
}

struct TriNode { int lo, mid, hi; };
static int tri_build(int lo, int hi, std::vector<std::vector<TriNode>>& levels) {
    if (hi - lo <= 1) return 0;
    const int mid = lo + (hi - lo + 1) / 2;
    const int hl = tri_build(lo, mid, levels), hr = tri_build(mid, hi, levels);
    const int ht = 1 + std::max(hl, hr);
    if ((int)levels.size() < ht) levels.resize(ht);
    levels[ht - 1].push_back({lo, mid, hi});
    return ht;
}

int plan_ensure(gpimhip_ctx* h, int nb) {
    LinalgPlan& P = h->plan;
    if (P.nb == nb) return GPIMHIP_OK;
    if (P.d_tiles) { (void)hipFree(P.d_tiles); P.d_tiles = nullptr; }
    std::vector<TileDesc> tl;
    auto mark = [&](size_t start) { return PlanRange{(int64_t)start, (int32_t)(tl.size() - start)}; };
    // triangular inversion, bottom-up by subtree height
    std::vector<std::vector<TriNode>> levels;
    tri_build(0, nb, levels);
    P.tri_t.clear();
    P.tri_x.clear();
    // Levels with several nodes: node after node, each longest-first, is a saw-tooth of costs and the
    // launch ends on the long tail of whichever workgroup slots drew the long tiles last (model in
    // tools/sched_model.py: 12 % / 40 % over the ideal makespan for 2 / 4 nodes).  One list sorted by
    // k-length instead: equal lengths are one tile column (T) or row (X) of every node, which still
    // share an operand panel.
    auto sort_longest_first = [&](size_t nnodes, size_t start) {
        // (lists of at most one chip-load of tiles stay node-major: sorted, one XCD would draw all the
        // long tiles of the single round -- 298 vs 218 us for the 8-node level at nb = 128)
        if (nnodes < 2 || tl.size() - start <= 512) return;
        std::stable_sort(tl.begin() + start, tl.end(),
                         [](const TileDesc& a, const TileDesc& b) { return a.kb1 - a.kb0 > b.kb1 - b.kb0; });
    };
    for (auto& lv : levels) {
        size_t s = tl.size();
        // T = L21 * X11: k-range [cj, mid) -- longest for the leftmost columns
        for (auto& nd : lv)
            rect_patch_order(tl, nd.mid, nd.hi, nd.lo, nd.mid, false, true,
                             [&](int, int cj, int& k0, int& k1) { k0 = cj; k1 = nd.mid; });
        sort_longest_first(lv.size(), s);
        P.tri_t.push_back(mark(s));
        s = tl.size();
        // X21 = -X22 * T: k-range [mid, ci] -- longest for the bottom rows
        for (auto& nd : lv)
            rect_patch_order(tl, nd.mid, nd.hi, nd.lo, nd.mid, true, false,
                             [&](int ci, int, int& k0, int& k1) { k0 = nd.mid; k1 = ci + 1; });
        sort_longest_first(lv.size(), s);
        P.tri_x.push_back(mark(s));
    }
    // K^-1 = L^-T L^-1 (lower): k-range [ci, nb), longest first.  Patches are 2 rows x 32 columns:
    // tiles of one row have the same k-length and stay in lock-step (their shared operand panel is
    // read once per XCD), neighbouring rows differ by one block only.
    {
        size_t s = tl.size();
        // (measured at N = 16384: 1x64 / 2x32 / 4x16 22.0-22.2 ms, 8x8 22.7, 16x4 23.2; L2-miss traffic
        // 61-67 GB for all of them)
        const int PR = 2, PC = 32;
        for (int ig = 0; ig <= (nb - 1) / PR; ++ig)
            for (int jg = 0; jg * PC <= std::min(nb - 1, ig * PR + PR - 1); ++jg)
                for (int i = ig * PR; i < std::min(nb, ig * PR + PR); ++i)
                    for (int j = jg * PC; j < std::min(nb, jg * PC + PC); ++j)
                        if (j <= i) tl.push_back({i, j, i, nb});
        P.lauum = mark(s);
    }
    P.n_tiles = (int64_t)tl.size();
    void* q = nullptr;
    HIP_TRY(hipMalloc(&q, std::max<size_t>(tl.size(), 1) * sizeof(TileDesc)));
    P.d_tiles = (TileDesc*)q;
    HIP_TRY(hipMemcpyAsync(P.d_tiles, tl.data(), tl.size() * sizeof(TileDesc), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    P.nb = nb;
    return GPIMHIP_OK;
}

// ------------------------------------------------------------------------------------------
// blocked drivers
// ------------------------------------------------------------------------------------------
GemmArgs gemm_args(const double* A, int64_t lda, const double* B, int64_t ldb, double* C, int64_t ldc,
                   double alpha, double beta, const TileDesc* tiles, int n, int64_t rows) {
    GemmArgs g;
    memset(&g, 0, sizeof(g));
    g.A = A; g.lda = lda; g.B = B; g.ldb = ldb; g.C = C; g.ldc = ldc;
    g.alpha = alpha; g.beta = beta; g.tiles = tiles; g.ntiles = n;
    g.sA = rows * lda; g.sB = rows * ldb; g.sC = rows * ldc;  // stacked np-row workspace matrices
    return g;
}

// The one helper stream of the library: the stream an iteration is CAPTURED on (mid-size N).  It is created on first
// use and shared by every handle of the device for the life of the process.  The training loop itself runs on the
// caller's stream alone.  (Until round 4 large-N iterations ran their two mat-vecs on a high-priority side stream beside
// the K^-1 product and drove the launch chains from a second one.  The side branch was the CAUSE of the "stream
// population" slow-down recorded in DESIGN.md section 6: its wait on the next iteration's event sits in a hardware queue
// of its own for the whole factorisation, and when that queue is the fifth or later the process has created, every
// dependent launch of the main queue starts 30-45 us late -- profiles/r04_queue_sweep.txt.  On the caller's stream the
// mat-vecs cost < 0.1 ms of a 74 ms iteration.)
struct SideStreams {
    hipStream_t capture = nullptr;
    bool capture_tried = false;
};
static std::mutex g_side_mutex;
static SideStreams g_side[64];
// gpimhip_shutdown destroys the shared stream; a handle that outlives it (a C-ABI host that shuts down and goes on)
// must not use the pointer it cached: every shutdown starts a new generation, and a handle of an older one forgets it
static std::atomic<int> g_side_generation{0};
static void side_refresh(gpimhip_ctx* h) {
    const int g = g_side_generation.load();
    if (h->side_generation == g) return;
    h->side_generation = g;
    h->capture_stream = nullptr;
    h->capture_stream_tried = false;
}
// The capture stream is shared by every handle of a device: two threads fitting at the same time must not
// interleave their Begin..EndCapture sections on it (the second BeginCapture would fail and that fit would
// silently run un-graphed).  Capture itself is short (host-side recording of one iteration).
static std::mutex g_capture_mutex[64];
static void capture_lock(gpimhip_ctx* h) { g_capture_mutex[h->device & 63].lock(); }
static void capture_unlock(gpimhip_ctx* h) { g_capture_mutex[h->device & 63].unlock(); }

static hipStream_t ensure_capture_stream(gpimhip_ctx* h) {
    side_refresh(h);
    if (!h->capture_stream && !h->capture_stream_tried) {
        h->capture_stream_tried = true;
        std::lock_guard<std::mutex> lock(g_side_mutex);
        SideStreams& S = g_side[h->device & 63];
        if (!S.capture_tried) {
            S.capture_tried = true;
            if (hipStreamCreateWithFlags(&S.capture, hipStreamNonBlocking) != hipSuccess) S.capture = nullptr;
        }
        h->capture_stream = S.capture;
    }
    return h->capture_stream;
}

// The blocked Cholesky: the step schedule of cholstep.hip (float matrices: cholstep32.hip).
int launch_potrf(gpimhip_ctx* h, double* A, int64_t np, int64_t ld, int32_t* info) {
    return launch_potrf_steps(h, A, np, ld, info, nullptr);
}

// in-place inverse of the lower-triangular factor: recursive halving, all nodes of one subtree
// height in one launch pair:  T = L21 * X11 ;  X21 = -X22 * T.
int launch_trtri(gpimhip_ctx* h, double* A, double* Tm, int64_t np, int64_t ld) {
    const int nb = (int)(np / NB);
    GP_TRY(plan_ensure(h, nb));
    const LinalgPlan& P = h->plan;
    GP_TRY(launch_diag_inv_copy(h, A, ld, nb));
    for (size_t lv = 0; lv < P.tri_t.size(); ++lv) {
        GemmArgs g1 = gemm_args(A, ld, A, ld, Tm, ld, 1.0, 0.0, P.d_tiles + P.tri_t[lv].off, P.tri_t[lv].n, h->np);
        g1.chunk = deal_chunk(g1.ntiles);
        g1.krev = 1;              // ranges [cj, mid) share their end
        GP_TRY(launch_gemm(h, false, true, EPI_STORE, g1));
        GemmArgs g2 = gemm_args(A, ld, Tm, ld, A, ld, -1.0, 0.0, P.d_tiles + P.tri_x[lv].off, P.tri_x[lv].n, h->np);
        g2.chunk = deal_chunk(g2.ntiles);
        GP_TRY(launch_gemm(h, false, true, EPI_STORE, g2));
    }
    return GPIMHIP_OK;
}

// A <- L^-1 for the SPD matrix in A (Tm: np x np temporary).  Double precision: one pass -- the tile operations of the
// inverse ride in the launches of the factorisation (cholstep.hip: plan_inverse); float matrices: factorisation, then
// the level-by-level inverse above.
int launch_potrf_inv(gpimhip_ctx* h, double* A, double* Tm, int64_t np, int64_t ld, int32_t* info, int rag) {
    if (!h->fp32) return launch_potrf_steps(h, A, np, ld, info, Tm, rag);
    { StageTimer t(h, 0); GP_TRY(launch_potrf_steps(h, A, np, ld, info, nullptr)); }
    StageTimer t(h, 1);
    return launch_trtri(h, A, Tm, np, ld);
}

// B(lower) = A^T A for lower-triangular A (= L^-1): K^-1.
int launch_lauum(gpimhip_ctx* h, const double* A, double* B, int64_t np, int64_t ld, int rag) {
    const int nb = (int)(np / NB);
    GP_TRY(plan_ensure(h, nb));
    const LinalgPlan& P = h->plan;
    GemmArgs g = gemm_args(A, ld, A, ld, B, ld, 1.0, 0.0, P.d_tiles + P.lauum.off, P.lauum.n, h->np);
    g.chunk = deal_chunk(g.ntiles);
    g.krev = 1;                   // ranges [ci, nb) share their end
    g.rag = h->fp32 ? 0 : rag;
    return launch_gemm(h, true, true, EPI_STORE, g);
}

// ------------------------------------------------------------------------------------------
// border of the reflection blocks: the exact GP on the observed points of an incomplete grid (border.hip, DESIGN.md
// section 11).  S = (A^-1)_mm has a handle of its own (`sub`: mp x mp workspace, factorisation plans, status word) that
// enqueues on the model handle's stream, so the factorisation of S is the engine's own and rides in the captured iteration.
// ------------------------------------------------------------------------------------------
BorderWs* bws(const gpimhip_ctx* h) { return (BorderWs*)h->border; }
bool border_on(const gpimhip_ctx* h) { return h->refl.mask && h->border && bws(h)->M > 0; }

static void border_free_bufs(gpimhip_ctx* h, BorderWs* w) {
    dev_release(h, w->C, w->Y, w->tv, w->scal, w->uo, w->tiles_y, w->tiles_upd, w->R, w->rsq);
    w->np = 0; w->B = 0; w->n_y = w->n_upd = 0; w->r_cols = 0;
}
static void border_release(gpimhip_ctx* h) {
    BorderWs* w = bws(h);
    if (!w) return;
    border_free_bufs(h, w);
    if (w->sub) gpimhip_destroy(w->sub);
    delete w;
    h->border = nullptr;
}

// buffers for the workspace's np and batch (outside any capture: allocations and tile-list uploads synchronise).
// T: the borders in lock-step (the tasks of the multi-output GP: the batch is T 2^r blocks; otherwise 1)
int border_ensure(gpimhip_ctx* h, int T) {
    BorderWs* w = bws(h);
    const int64_t mp = pad_to(w->M, NB);
    if (!w->sub) GP_TRY(gpimhip_create(&w->sub, h->device, h->stream));
    w->sub->nbatch = T;
    w->sub->stream = h->stream;
    GP_TRY(ws_ensure_b(w->sub, w->M, T, 1));
    if (w->np == h->np && w->B == h->nbatch && w->T == T && w->mp == mp && w->C) return GPIMHIP_OK;
    HIP_TRY(hipStreamSynchronize(h->stream));
    border_free_bufs(h, w);
    w->mp = mp; w->np = h->np; w->B = h->nbatch; w->T = T;
    const int nb = (int)(h->np / NB), nm = (int)(mp / NB);
    std::vector<TileDesc> ty, tu;
    for (int ci = 0; ci < nb; ++ci)
        for (int cj = 0; cj < nm; ++cj) ty.push_back({ci, cj, 0, cj + 1});       // L_S^-1 is lower triangular
    lower_patch_order(tu, 0, nb, 0, nm);
    w->n_y = (int)ty.size();
    w->n_upd = (int)tu.size();
    int rc = GPIMHIP_OK;
    if ((rc = w->C.alloc(h, (int64_t)w->B * w->np * mp)) || (rc = w->Y.alloc(h, (int64_t)w->B * w->np * mp)) ||
        (rc = w->tv.alloc(h, 2 * mp * T)) || (rc = w->scal.alloc(h, 2 * T)) || (rc = w->tiles_y.alloc(h, w->n_y)) ||
        (rc = w->tiles_upd.alloc(h, w->n_upd))) {
        border_free_bufs(h, w);
        return rc;
    }
    HIP_TRY(hipMemcpyAsync(w->tiles_y, ty.data(), ty.size() * sizeof(TileDesc), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(w->tiles_upd, tu.data(), tu.size() * sizeof(TileDesc), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return GPIMHIP_OK;
}
int border_ensure_r(gpimhip_ctx* h, int64_t cols) {
    BorderWs* w = bws(h);
    if (w->r_cols >= cols && w->R) return GPIMHIP_OK;
    HIP_TRY(hipStreamSynchronize(h->stream));
    dev_release(h, w->R, w->rsq);
    w->r_cols = 0;
    int rc = GPIMHIP_OK;
    if ((rc = w->R.alloc(h, w->mp * cols * w->T)) || (rc = w->rsq.alloc(h, cols * w->T))) {
        w->R.release(h);
        return rc;
    }
    w->r_cols = cols;
    return GPIMHIP_OK;
}

// After the blocks' inverses are in h->B (launch_lauum): S, L_S^-1, Y_b = C_b L_S^-T, the corrected alpha, the two loss
// scalars, and (training) B_b^-1 -= Y_b Y_b^T on the lower tiles.  nq: the points of the fundamental domain.
// With T borders (BorderWs::T) all of it runs per task in lock-step: sub factors the T matrices S_t as one batch.
int border_iter(gpimhip_ctx* h, int64_t nq, bool update_inverse) {
    BorderWs* w = bws(h);
    gpimhip_ctx* sub = w->sub;
    sub->stream = h->stream;                // (the capture stream while run_fit_iterations records an iteration)
    const int64_t mp = w->mp;
    GP_TRY(launch_border_gather_s(h, w, h->B, h->ld, sub->A, sub->ld));
    GP_TRY(launch_potrf_inv(sub, sub->A, sub->Tm, mp, sub->ld, sub->info, 0));      // (rag 0: every padding row is written)
    GP_TRY(launch_border_tidy(h, w, sub->A, sub->ld));
    GP_TRY(launch_border_gather_c(h, w, h->B, h->ld, nq));
    {
        // Y = C L_S^-T (NT: operand B is L_S^-1 of the problem's task, shared by the task's blocks)
        GemmArgs g = gemm_args(w->C, mp, sub->A, sub->ld, w->Y, mp, 1.0, 0.0, w->tiles_y, w->n_y, h->np);
        g.sB = sub->np * sub->ld;
        g.bshift = __builtin_ctz((unsigned)(h->nbatch / w->T));         // (2^r blocks per task)
        g.chunk = deal_chunk(g.ntiles);
        GP_TRY(launch_gemm(h, false, false, EPI_STORE, g));
    }
    GP_TRY(launch_border_vectors(h, w, sub->A, sub->ld, sub->logdet_part, (int)(mp / NB), h->alpha));
    if (update_inverse) {
        // B_b^-1 -= Y_b Y_b^T (NT, subtracting epilogue: alpha = -1, beta = 1) on the tiles the gradient contraction reads
        GemmArgs g = gemm_args(w->Y, mp, w->Y, mp, h->B, h->ld, -1.0, 1.0, w->tiles_upd, w->n_upd, h->np);
        g.sA = g.sB = h->np * mp;
        g.kfix0 = 0;
        g.kfix1 = (int)(mp / NB);
        g.chunk = deal_chunk(g.ntiles);
        GP_TRY(launch_gemm(h, false, false, EPI_STORE, g));
    }
    return GPIMHIP_OK;
}

// N <= 128: the fused single-workgroup trainer (smalln.hip) replaces the blocked path
static bool use_small_path(int64_t N) { return N <= NB && !getenv("GPIMHIP_NO_SMALLN"); }

int check_model(const gpimhip_model_t* m) {
    if (!m || m->dim < 1 || m->dim > GPIMHIP_MAX_DIM || (m->n_ls != 1 && m->n_ls != m->dim) ||
        m->kernel < 0 || m->kernel > GPIMHIP_KERNEL_RQ) {
        gpim_set_error("invalid gpimhip_model_t");
        return GPIMHIP_E_BADARG;
    }
    return GPIMHIP_OK;
}

// Everything needed at the current u: theta, K, L, L^-1, z, alpha.  (Shared by fit and predict.)
// x_bs: per-problem stride of X in elements (0 when all problems of a batch share one X).
// z = L^-1 y, alpha = L^-T z (two HBM-bound passes over L^-1).
// Single-precision handles refine alpha against the covariance regenerated in double (launch_kres): the fp32
// factor and its explicit fp32 inverse leave an error of eps32 * cond(K) in alpha, every pass
// alpha += K32^-1 (y - K alpha) multiplies it by that factor again (one pass by default; measured at cond = 1e5,
// N = 2300, RBF: posterior-mean error 6e-4 -> 1.2e-4, a float32 LAPACK run: 1.3e-3; loss 0.95 -> 0.06 of 4129;
// a second pass changes nothing -- what is left comes from log det and K^-1 themselves).  The loss then takes its
// quadratic term as y^T alpha (launch_finalize).
static int refine_passes() {
    static const int v = 1;
    return v;
}
// defer_alpha (double precision only): alpha stays as the row-chunk partial sums in h->gemv_part -- the gradient
// contraction adds up the entries it needs itself (launch_grad_reduce_fin), one launch less per iteration; h->alpha is
// then NOT valid.
static bool alpha_deferrable(const gpimhip_ctx* h) { return !h->fp32 && !h->refl.mask && h->np <= 8192 && !h->no_fused_finalize; }
// GPIMHIP_NO_FUSED_FINALIZE (run-time knob: the finalize step as a launch of its own, theta launched every iteration -- the
// same reductions in the same order, the same bits), read ONCE per public call, at the top of every entry that reaches
// loss_grad_at_u; carry (fit_impl), modern / fused (loss_grad_at_u) and alpha_deferrable all follow this one read, so they
// cannot disagree inside a call.  Per call, not per handle: the tests flip the knob on a live handle.
static void read_finalize_knob(gpimhip_ctx* h) { h->no_fused_finalize = getenv("GPIMHIP_NO_FUSED_FINALIZE") != nullptr; }
int solve_vectors(gpimhip_ctx* h, const gpimhip_model_t* m, const double* X, int64_t x_bs, int64_t N, bool defer_alpha) {
    const int64_t np = h->np, ld = h->ld;
    GP_TRY(launch_trmv_lower(h, h->A, ld, np, h->ypad, h->z));
    GP_TRY(launch_gemv_t_tri(h, h->A, ld, np, h->z, h->gemv_part, defer_alpha && !h->fp32 ? nullptr : h->alpha));
    if (!h->fp32) return GPIMHIP_OK;
    const int B = h->nbatch, nb = (int)(np / NB);
    // >= ~512 workgroups per launch of ONE problem.  S sets the order in which the residual's partial sums are added, so it
    // must not depend on the batch: a problem of a lock-step batch keeps the bits of its stand-alone run (it used to be
    // 512 / (nb * B): from 17 block columns a batch of four summed in another order than the same problem alone).
    const int S = std::max(1, std::min(8, 512 / std::max(1, nb)));
    double *res = h->refine, *delta = res + (int64_t)B * np, *scratch = delta + (int64_t)B * np;
    for (int pass = 0; pass < refine_passes(); ++pass) {
        GP_TRY(launch_kres(h, m, X, x_bs, N, scratch, S, res));
        GP_TRY(launch_trmv_lower(h, h->A, ld, np, res, h->z));
        GP_TRY(launch_gemv_t_tri(h, h->A, ld, np, h->z, h->gemv_part, delta));
        GP_TRY(launch_axpy(h, h->alpha, delta, (int64_t)B * np));
    }
    return GPIMHIP_OK;
}

// K(u) -> L -> L^-1 (in h->A), then z = L^-1 y and alpha = L^-T z
// theta_current: h->theta already holds theta(u) -- the previous iteration's finalize step wrote it (fit_impl)
int factor_at_u(gpimhip_ctx* h, const gpimhip_model_t* m, const double* X, int64_t x_bs, int64_t N, const double* u,
                bool theta_current, bool defer_alpha) {
    const int64_t np = h->np, ld = h->ld;
    if (!theta_current) GP_TRY(launch_theta(h, m, u));
    if (h->refl.mask)      // symmetry-reduced model: problem b of the batch is the block of sign pattern b (engine.hip)
        GP_TRY(launch_kmat_refl(h, m, X, N, nullptr, N, h->theta, h->A, ld, np, np, 1, x_bs, x_bs, np * ld, 1.0));
    else
        GP_TRY(launch_kmat(h, m, X, N, nullptr, N, h->theta, 0.0, 1, h->A, ld, np, np, 1, 1, x_bs, x_bs, np * ld));
    GP_TRY(launch_potrf_inv(h, h->A, h->Tm, np, ld, h->info, rag_of(N, np)));
    return solve_vectors(h, m, X, x_bs, N, defer_alpha);
}

// theta_carried: the training loop launched theta(u) once before its first iteration; every finalize step then leaves the
// theta of the stepped parameters in h->theta (no theta launch inside the loop)
struct IterTable : FinalizeIter { bool theta_carried; };
// what a training iteration minimises: the negative log marginal likelihood, or the leave-one-out pseudo-likelihood
// (loograd.hip; one double-precision problem of the dense engine: loo_objective_refused)
enum Objective { OBJ_NLL = 0, OBJ_LOO = 1 };

static int loss_grad_at_u(gpimhip_ctx* h, const gpimhip_model_t* m, const double* X, int64_t x_bs, int64_t N,
                          double* u, int do_adam, AdamStep st, double* loss_out, double* grad_out,
                          double* hist_row, const IterTable* tab = nullptr, Objective obj = OBJ_NLL) {
    const int64_t np = h->np;
    if (obj == OBJ_LOO)     // (its finalize step is always a launch of its own; theta is carried as for the other objective)
        return loo_grad_at_u(h, m, X, N, u, do_adam, st, tab ? FinalizeOut(*tab) : FinalizeOut(loss_out, grad_out, hist_row),
                             !h->no_fused_finalize && tab && tab->theta_carried);
    // One launch for the gradient contraction and the finalize step (unless the knob asks for the two launches: see
    // read_finalize_knob)
    // ... up to np = 8192; beyond, the finalize step is a launch of its own again (the tail's device-scope loads of 8256 tiles'
    // sums take longer than a launch boundary costs: 530 us against 400 + 20 at N = 16384) -- it still leaves the next theta
    const bool modern = !h->refl.mask && !h->no_fused_finalize;
    const bool fused = modern && np <= 8192;
    const bool carried = modern && tab && tab->theta_carried;
    const bool defer = fused && alpha_deferrable(h);
    // a training loop leaves its results by the table, one evaluation where the caller said
    const FinalizeOut out = tab ? FinalizeOut(*tab) : FinalizeOut(loss_out, grad_out, hist_row);
    GP_TRY(factor_at_u(h, m, X, x_bs, N, u, carried, defer));
    { StageTimer t(h, 2); GP_TRY(launch_lauum(h, h->A, h->B, np, h->ld, rag_of(N, np))); }
    if (h->refl.mask) {
        const bool bd = border_on(h);
        if (bd) GP_TRY(border_iter(h, N, true));
        GP_TRY(launch_grad_reduce_refl(h, m, h->B, h->ld, X, N, (int)(np / NB), h->alpha, x_bs));
        return launch_finalize_coupled(h, m, N, np, u, do_adam, st, out, bd ? bws(h)->scal.p : nullptr);
    }
    if (fused) return launch_grad_reduce_fin(h, m, X, x_bs, N, defer, u, do_adam, st, out, carried ? 1 : 0);
    GP_TRY(launch_grad_reduce(h, m, h->B, h->ld, X, N, (int)(np / NB), h->alpha, x_bs));
    return launch_finalize(h, m, N, np, u, do_adam, st, out, carried ? 1 : 0);
}

// Fill the device table of Adam bias corrections (same libm pow() values for every path).
int upload_bc_table(gpimhip_ctx* h, double lr, int T) {
    GP_TRY(h->bc.grow(h, 2 * (int64_t)T));
    h->bc_host.resize(2 * (size_t)T);
    for (int t = 1; t <= T; ++t) {
        h->bc_host[t - 1] = lr / (1.0 - pow(0.9, (double)t));
        h->bc_host[T + t - 1] = sqrt(1.0 - pow(0.999, (double)t));
    }
    HIP_TRY(hipMemcpyAsync(h->bc, h->bc_host.data(), 2 * (size_t)T * sizeof(double), hipMemcpyHostToDevice,
                           h->stream));
    return GPIMHIP_OK;
}

int fit_prologue(gpimhip_ctx* h, double lr, int T, double* adam_m, double* adam_v, size_t adam_bytes, int32_t* iter) {
    HIP_TRY(hipMemsetAsync(h->info + 1, 0x7f, sizeof(int32_t), h->stream));   // "completed" = huge until a failure
    h->fit_completed = T;
    if (T == 0) return GPIMHIP_OK;
    GP_TRY(upload_bc_table(h, lr, T));
    HIP_TRY(hipMemsetAsync(adam_m, 0, adam_bytes, h->stream));
    if (adam_v) HIP_TRY(hipMemsetAsync(adam_v, 0, adam_bytes, h->stream));
    HIP_TRY(hipMemsetAsync(iter, 0, sizeof(int32_t), h->stream));
    return GPIMHIP_OK;
}

// info[0]: 0 or 1 + first failing column; info[1]: the number of Adam iterations that had completed
// when a training loop first met a non-PD matrix (min over the problems of a batch; only meaningful
// when info[0] != 0 -- fit_impl presets it to a large value).
int finish_and_check(gpimhip_ctx* h) {
    int32_t info[2] = {0, 0};
    HIP_TRY(hipMemcpyAsync(info, h->info, 2 * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    if (info[0] != 0) {
        h->fit_completed = std::max(0, std::min(h->fit_completed, info[1]));
        gpim_set_error("cholesky: the input is not positive-definite (leading minor of order " +
                       std::to_string(info[0]) + ")");
        return GPIMHIP_E_NOT_PD;
    }
    return GPIMHIP_OK;
}

// Bounded run-ahead for training loops: every `period` iterations the status word is copied to pinned
// host memory behind an event; before enqueueing more work the host looks at the copy made two periods
// ago (already complete unless the queue is that short), so a failed factorisation stops the loop
// within 2 * period iterations while the device queue never drains.  The device side freezes u, the
// Adam state and the history at the failing iteration on its own (finalize_kernel), so where exactly
// the host stops enqueueing does not change any result.
struct RunAhead {
    gpimhip_ctx* h;
    int period;
    bool armed[2] = {false, false};
    RunAhead(gpimhip_ctx* h_, int64_t np, bool enabled) : h(h_), period(enabled ? (np >= 4096 ? 4 : 32) : 0) {
        if (enabled && !h->pinned_info) {
            void* q = nullptr;
            if (hipHostMalloc(&q, 2 * sizeof(int32_t), hipHostMallocDefault) == hipSuccess) h->pinned_info = (int32_t*)q;
            for (auto& e : h->ra_ev)
                if (!e && hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) e = nullptr;
        }
    }
    // call before enqueueing iteration t; returns true when the loop should stop
    bool stop(int t) {
        if (!period || !h->pinned_info || !h->ra_ev[0] || !h->ra_ev[1] || t == 0 || t % period) return false;
        const int slot = (t / period) & 1;
        if (armed[slot]) {
            (void)hipEventSynchronize(h->ra_ev[slot]);
            if (h->pinned_info[slot] != 0) return true;
        }
        (void)hipMemcpyAsync(h->pinned_info + slot, h->info, sizeof(int32_t), hipMemcpyDeviceToHost, h->stream);
        (void)hipEventRecord(h->ra_ev[slot], h->stream);
        armed[slot] = true;
        return false;
    }
};

// The training loop of every fit entry point (common.hpp).  Every iteration enqueues the same launches (the iteration
// index lives on the device: FinalizeIter), so one iteration is captured into a hipGraph and replayed: ~10 us of host work
// per iteration instead of one launch call per kernel.  Not used for very short fits, and for the dense engine
// (FitLoop::dense_gates) neither while stage timing is on nor at large N, where the launch cost no longer matters and the
// iteration is enqueued launch by launch on the caller's stream (ONE in-order stream: factor_at_u, loss_grad_at_u).
// The capture lock is held from begin to end capture only, not during replay.
int run_fit_iterations(gpimhip_ctx* h, int T, FitLoop loop, const std::function<int()>& iteration) {
    bool use_graph = T >= 8 && !getenv("GPIMHIP_NO_GRAPH");
    if (loop.dense_gates) {
        const int npanel = (int)((h->np / NB + OUTER_W - 1) / OUTER_W);
        use_graph = use_graph && !h->timing && npanel < EAGER_MIN_PANELS;
    }
    hipGraph_t graph = nullptr;
    hipGraphExec_t exec = nullptr;
    if (use_graph && ensure_capture_stream(h)) {
        hipStream_t main_s = h->stream;
        h->stream = h->capture_stream;
        capture_lock(h);
        hipError_t e = hipStreamBeginCapture(h->capture_stream, hipStreamCaptureModeRelaxed);
        int rc = GPIMHIP_OK;
        if (e == hipSuccess) {
            rc = iteration();
            e = hipStreamEndCapture(h->capture_stream, &graph);
        }
        capture_unlock(h);
        h->stream = main_s;
        if (rc != GPIMHIP_OK) { if (graph) (void)hipGraphDestroy(graph); return rc; }
        if (e != hipSuccess || !graph || hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0) != hipSuccess) {
            if (graph) (void)hipGraphDestroy(graph);
            graph = nullptr;
            exec = nullptr;
            (void)hipGetLastError();                        // capture unavailable: plain launches below
        }
    }
    RunAhead ra(h, h->np, loop.run_ahead);
    if (!exec) {
        for (int t = 0; t < T && !ra.stop(t); ++t) GP_TRY(iteration());
        return finish_and_check(h);
    }
    hipError_t le = hipSuccess;
    for (int t = 0; t < T && le == hipSuccess && !ra.stop(t); ++t) le = hipGraphLaunch(exec, h->stream);
    const int rc = finish_and_check(h);
    (void)hipGraphExecDestroy(exec);
    (void)hipGraphDestroy(graph);
    HIP_TRY(le);
    return rc;
}

// ------------------------------------------------------------------------------------------
// C ABI
// ------------------------------------------------------------------------------------------
extern "C" {

const char* gpimhip_last_error(void) { return g_err.c_str(); }

// Destroys the process-wide capture stream (ensure_capture_stream).  Called by the Python binding at interpreter exit,
// while the HIP runtime is still up.
int gpimhip_shutdown(void) {
    std::lock_guard<std::mutex> lock(g_side_mutex);
    for (auto& S : g_side) {
        if (S.capture) (void)hipStreamDestroy(S.capture);
        S = SideStreams();
    }
    g_side_generation.fetch_add(1);
    return GPIMHIP_OK;
}
int gpimhip_version(void) { return 100; }

int gpimhip_create(gpimhip_handle* out, int device, void* hip_stream) {
    if (!out) return GPIMHIP_E_BADARG;
    HIP_TRY(hipSetDevice(device));
    gpimhip_ctx* h = new gpimhip_ctx();
    h->device = device;
    h->stream = (hipStream_t)hip_stream;     // NULL = the device's default (null) stream
    int rc = GPIMHIP_OK;
    if ((rc = h->theta1.alloc(h, 1)) || (rc = h->info.alloc(h, 4))) {
        delete h;
        return rc;
    }
    (void)hipMemsetAsync(h->info, 0, 4 * sizeof(int32_t), h->stream);
    *out = h;
    return GPIMHIP_OK;
}

int gpimhip_set_precision(gpimhip_handle h, int32_t bits) {
    if (!h || (bits != 32 && bits != 64)) return GPIMHIP_E_BADARG;
    const int want = bits == 32 ? 1 : 0;
    if (want == h->fp32) return GPIMHIP_OK;
    if (want && h->refl.mask) {     // (the other order is refused by gpimhip_set_reflection)
        gpim_set_error("the symmetry-reduced model computes in double precision: leave reflection mode (gpimhip_set_reflection(h, 0, ...)) first");
        return GPIMHIP_E_BADARG;
    }
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipStreamSynchronize(h->stream));
    ws_release_matrix(h);               // sized by the element type
    ws_release_predict(h);
    sample_release(h);
    ivr_release(h);
    h->fp32 = want;
    return GPIMHIP_OK;
}

int gpimhip_destroy(gpimhip_handle h) {
    if (!h) return GPIMHIP_OK;
    (void)hipSetDevice(h->device);
    (void)hipStreamSynchronize(h->stream);
    vfe_release(h);
    kron_release(h);
    vgp_release(h);
    pkron_release(h);
    sm_release(h);
    border_release(h);
    sample_release(h);
    ivr_release(h);
    ws_release_matrix(h);
    ws_release_predict(h);
    dev_release(h, h->keys, h->sel_scratch, h->acq_tmp, h->refine, h->bc, h->theta1, h->info, h->loo_tiles);
    if (h->plan.d_tiles) (void)hipFree(h->plan.d_tiles);
    step_plan_release(h);
    dist_plan_release(h);
    for (auto e : h->ra_ev)
        if (e) (void)hipEventDestroy(e);
    if (h->pinned_info) (void)hipHostFree(h->pinned_info);
    // (the capture stream belongs to the process, not to the handle)
    delete h;
    return GPIMHIP_OK;
}

// (with a border: the handle of S is part of the model's workspace; so is the factorisation context of the draws)
int64_t gpimhip_workspace_bytes(gpimhip_handle h) {
    if (!h) return 0;
    const BorderWs* w = bws(h);
    return h->bytes + (w && w->sub ? w->sub->bytes : 0) + sample_bytes(h);
}

int gpimhip_timing_enable(gpimhip_handle h, int enable) {
    if (!h) return GPIMHIP_E_BADARG;
    h->timing = enable != 0;
    return GPIMHIP_OK;
}

int gpimhip_timing_read(gpimhip_handle h, int stage, double* total_ms, int64_t* count) {
    if (!h || stage < 0 || stage > 6 || !total_ms || !count) return GPIMHIP_E_BADARG;
    HIP_TRY(hipStreamSynchronize(h->stream));
    double tot = 0.0;
    for (auto& pr : h->ev[stage]) {
        float ms = 0.f;
        (void)hipEventElapsedTime(&ms, pr.first, pr.second);
        tot += ms;
        (void)hipEventDestroy(pr.first);
        (void)hipEventDestroy(pr.second);
    }
    *total_ms = tot;
    *count = (int64_t)h->ev[stage].size();
    h->ev[stage].clear();
    return GPIMHIP_OK;
}

int gpimhip_fit_completed(gpimhip_handle h) { return h ? h->fit_completed : 0; }

int gpimhip_sync(gpimhip_handle h) {
    if (!h) return GPIMHIP_E_BADARG;
    HIP_TRY(hipStreamSynchronize(h->stream));
    return GPIMHIP_OK;
}

int gpimhip_kmat(gpimhip_handle h, const gpimhip_model_t* m, const double* X, int64_t N, const double* Z,
                 int64_t M, const double* theta, double diag_add, double* out, int64_t ld) {
    FP64_ONLY(h);
    if (!h || !X || !theta || !out || N < 1) return GPIMHIP_E_BADARG;
    GP_TRY(check_model(m));
    HIP_TRY(hipSetDevice(h->device));
    const bool sym = (Z == nullptr);
    const int64_t Mv = sym ? N : M;
    if (Mv < 1 || ld < Mv) return GPIMHIP_E_BADARG;
    h->nbatch = 1;
    GP_TRY(launch_theta_raw(h, m, theta));
    // tiles are 128x128: build into a padded scratch and copy out the valid part
    const int64_t rp = pad_to(N, NB), cp = pad_to(Mv, NB);
    GP_TRY(ws_ensure_predict(h, rp, cp));
    const int64_t kld = h->ks_cols + 16;
    GP_TRY(launch_kmat(h, m, X, N, sym ? nullptr : Z, Mv, h->theta1, diag_add, 0, h->Ks, kld, rp, cp, sym ? 1 : 0, 0, 0,
                       0, 0));
    HIP_TRY(hipMemcpy2DAsync(out, (size_t)ld * sizeof(double), h->Ks, (size_t)kld * sizeof(double),
                             (size_t)Mv * sizeof(double), (size_t)N, hipMemcpyDeviceToDevice, h->stream));
    return GPIMHIP_OK;
}

int gpimhip_potrf(gpimhip_handle h, double* A, int64_t n, int64_t ld, int32_t* info) {
    FP64_ONLY(h);
    if (!h || !A || n < 1 || ld < n || !info) return GPIMHIP_E_BADARG;
    HIP_TRY(hipSetDevice(h->device));
    h->nbatch = 1;
    GP_TRY(ws_ensure(h, n));
    const int64_t np = h->np;
    HIP_TRY(hipMemsetAsync(info, 0, sizeof(int32_t), h->stream));
    GP_TRY(launch_pad_matrix_in(h, A, n, ld, h->A, np));
    GP_TRY(launch_potrf(h, h->A, np, np, info));
    GP_TRY(launch_pad_matrix_out_lower(h, h->A, np, A, n, ld));
    return GPIMHIP_OK;
}

static int fit_impl(gpimhip_ctx* h, const gpimhip_model_t* m, const double* X, int64_t x_bs, const double* y,
                    int64_t N, int B, double* u, double lr, int32_t T, double* hist_out, double* loss_out,
                    Objective obj = OBJ_NLL) {
    read_finalize_knob(h);
    HIP_TRY(hipSetDevice(h->device));
    h->nbatch = B;
    HIP_TRY(hipMemsetAsync(h->info, 0, sizeof(int32_t), h->stream));
    HIP_TRY(hipMemsetAsync(h->info + 1, 0x7f, sizeof(int32_t), h->stream));   // "completed" = huge until a failure
    h->fit_completed = T;
    if (T == 0) return GPIMHIP_OK;
    GP_TRY(upload_bc_table(h, lr, T));
    if (use_small_path(N) && !h->refl.mask && obj == OBJ_NLL) {
        // fused single-launch trainer, one workgroup per problem (it knows the marginal likelihood only)
        GP_TRY(launch_fit_small(h, m, X, x_bs, y, (int)N, u, h->bc, h->bc + T, T, hist_out, loss_out, nullptr));
        return finish_and_check(h);
    }
    GP_TRY(ws_ensure_padded(h, N));
    if (obj == OBJ_LOO) GP_TRY(loo_obj_ensure(h));
    if (border_on(h)) GP_TRY(border_ensure(h));
    HIP_TRY(hipMemsetAsync(h->adam_m, 0, (size_t)B * MAXP * sizeof(double), h->stream));
    HIP_TRY(hipMemsetAsync(h->adam_v, 0, (size_t)B * MAXP * sizeof(double), h->stream));
    HIP_TRY(hipMemsetAsync(h->iter, 0, (size_t)B * sizeof(int32_t), h->stream));     // iteration counters
    HIP_TRY(hipMemsetAsync(h->fin_counter, 0, (size_t)B * sizeof(uint32_t), h->stream));   // (zero already, unless a launch was cut short)
    GP_TRY(launch_pad_copy(h, y, N, h->ypad, h->np));
    // theta(u) once; after that every iteration's finalize step leaves the next theta behind (not for the symmetry-reduced
    // model, whose coupled finalize step is a launch of its own)
    const bool carry = !h->refl.mask && !h->no_fused_finalize;
    if (carry) GP_TRY(launch_theta(h, m, u));
    const IterTable tab{{h->iter, h->bc, T, hist_out, loss_out}, carry};
    const AdamStep st = adam_step_init();
    return run_fit_iterations(h, T, FIT_LOOP_DENSE,
                              [&] { return loss_grad_at_u(h, m, X, x_bs, N, u, 1, st, nullptr, nullptr, nullptr, &tab, obj); });
}


// test-point columns per chunk of predict_cols: the K* slabs of all B problems together stay <= ~1 GiB
// (C++ linkage, as model_state_at_u below: this and the next two are declared in common.hpp)
extern "C++" int64_t predict_chunk_cols(int64_t np, int B, int64_t M) {
    int64_t mc = std::min(pad_to(M, NB), std::max<int64_t>(NB, ((int64_t)1 << 27) / np / B / NB * NB));
    // run-time knob for the tests: at most this many columns (rounded down to whole tiles), so that the second and the ragged
    // last pass of the loop run at test sizes
    if (const char* e = getenv("GPIMHIP_PREDICT_CHUNK")) mc = std::min(mc, std::max<int64_t>(NB, atoll(e) / NB * NB));
    return mc;
}

// posterior mean / variance at the family's test points from the factorised model in the workspace (L^-1, alpha; with a
// border Y_b): per chunk the family's K* slab, mean_tmp = K*^T alpha, colpart = column sums of squares of L^-1 K* (and
// rsq = those of R = sum_b Y_b^T K*_b), then the family's finisher
extern "C++" int predict_cols(gpimhip_ctx* h, const PredictFamily& f, int64_t N, int B) {
    const int64_t np = h->np, M = f.M;
    const int nb = (int)(np / NB);
    // few observations: one fused launch, K* stays in LDS (predict.hip)
    if (f.fused && !h->fp32 && fused_predict_fits(np)) return f.fused();
    const int64_t mc = predict_chunk_cols(np, B, M);
    GP_TRY(ws_ensure_predict(h, np, mc));
    const bool bd = border_on(h);
    if (bd) GP_TRY(border_ensure_r(h, h->ks_cols));
    for (int64_t m0 = 0; m0 < M; m0 += mc) {
        const int64_t cnt = std::min(mc, M - m0), mcap = h->ks_cols;       // buffer strides follow the capacity
        PredictChunk c{f.Xs + m0 * f.dim, m0, cnt, pad_to(cnt, NB), mcap, mcap + 16, cnt, nullptr};
        GP_TRY(f.slab(c));
        GP_TRY(launch_gemv_t(h, h->Ks, c.kld, np, c.cpad, h->alpha, h->mean_tmp, 0, np * c.kld, np, c.mcap));
        if (f.mean) GP_TRY(f.mean(c));
        // reflection blocks: the variance may be wanted for the first var_count test points only (it is invariant under
        // the reflections: a caller predicting on the training grid asks for it on the fundamental domain)
        // (not with a border: the missing points break the symmetry of the variance)
        if (f.var_on_domain && h->refl.var_count > 0 && !bd) c.nvar = std::max<int64_t>(0, std::min(cnt, h->refl.var_count - m0));
        if (c.nvar > 0) {
            GemmArgs g = gemm_args(h->A, h->ld, h->Ks, c.kld, nullptr, 0, 1.0, 0.0, h->pred_tiles, 0, h->np);
            if (c.nvar < c.cnt) g.cj_max = (int)((c.nvar + NB - 1) / NB);
            g.sB = np * c.kld;
            g.colpart = h->colpart;
            g.ld_colpart = c.mcap;
            g.sColpart = (int64_t)nb * c.mcap;
            // a ragged last chunk still sweeps all column tiles of the slab (stale columns are ignored)
            g.ntiles = (int)h->pred_ntiles;
            g.chunk = deal_chunk(g.ntiles);
            g.rag = h->fp32 ? 0 : rag_of(N, np);
            { StageTimer t(h, 3); GP_TRY(launch_gemm(h, false, true, EPI_COLSUMSQ, g)); }
            if (bd) {
                // R = sum_b Y_b^T K*_b: the stacked blocks of Y and of the slab are (B np)-row matrices (TN, one problem per
                // border: sub's batch -- the multi-output GP's tasks, each with its 2^r blocks and K* at its own variance)
                BorderWs* w = bws(h);
                w->sub->stream = h->stream;
                const int64_t brows = (int64_t)(B / w->T) * np;
                GemmArgs gr = gemm_args(w->Y, w->mp, h->Ks, c.kld, w->R, w->r_cols, 1.0, 0.0, nullptr, 0, 0);
                gr.sA = brows * w->mp;
                gr.sB = brows * c.kld;
                gr.sC = w->mp * w->r_cols;
                gr.rect_rows = (int)(w->mp / NB);
                gr.rect_cols = (int)(c.cpad / NB);
                gr.ntiles = gr.rect_rows * gr.rect_cols;
                gr.kfix0 = 0;
                gr.kfix1 = (int)(brows / NB);
                gr.chunk = deal_chunk(gr.ntiles);
                GP_TRY(launch_gemm(w->sub, true, true, EPI_STORE, gr));
                GP_TRY(launch_border_colsumsq(h, w, c.cnt));
                c.radd = w->rsq;
            }
        }
        GP_TRY(f.finish(c));
    }
    return GPIMHIP_OK;
}

// The stationary kernels (engine.hip) at the parameters in h->theta.  Dense: the fused launch where it fits, else the mean
// copied out and the variance from colpart.  Reflection mode: V_s^T k(X, x*), the block's rows against the test point and
// its mirror images, |G|^-1/2 each; the coupled finisher sums the blocks.  The test grid is shared by all problems of the
// batch (z stride 0).
extern "C++" PredictFamily stationary_family(gpimhip_ctx* h, const gpimhip_model_t* m, const double* X, int64_t x_bs, int64_t N,
                                             int B, const double* Xs, int64_t M, double* mean_out, double* var_out) {
    PredictFamily f{m->dim, Xs, M};
    if (h->refl.mask) {
        const double scale = 1.0 / sqrt((double)(h->refl.nblocks_total > 0 ? h->refl.nblocks_total : B));
        f.var_on_domain = true;
        f.slab = [=](const PredictChunk& c) {
            return launch_kmat_refl(h, m, X, N, c.Z, c.cnt, h->theta, h->Ks, c.kld, h->np, c.cpad, 0, x_bs, 0, h->np * c.kld, scale);
        };
        f.finish = [=](const PredictChunk& c) {
            return launch_predict_coupled(h, c.mcap, (int)(h->np / NB), c.m0, c.cnt, c.nvar, c.mcap, mean_out, var_out, c.radd);
        };
        return f;
    }
    f.fused = [=] { return launch_predict_fused(h, m, X, x_bs, N, Xs, M, mean_out, var_out); };
    f.slab = [=](const PredictChunk& c) {
        return launch_kmat(h, m, X, N, c.Z, c.cnt, h->theta, 0.0, 0, h->Ks, c.kld, h->np, c.cpad, 0, 0, x_bs, 0, h->np * c.kld);
    };
    f.mean = [=](const PredictChunk& c) { return launch_copy_slice(h, h->mean_tmp, mean_out + c.m0, c.cnt, c.mcap, M); };
    f.finish = [=](const PredictChunk& c) { return launch_predict_var(h, c.mcap, (int)(h->np / NB), c.m0, c.cnt, var_out, M); };
    return f;
}

// The model's state at u, what a prediction and a draw through the border start from: theta, L^-1 (h->A), alpha and, with a
// border, the blocks' inverses (h->B), S, L_S^-1, C_b, Y_b and the corrected alpha
// (C++ linkage: declared in common.hpp for draws.hip; not part of the C ABI this block defines)
extern "C++" int model_state_at_u(gpimhip_ctx* h, const gpimhip_model_t* m, const double* X, int64_t x_bs, const double* y,
                                  int64_t N, int B, const double* u) {
    HIP_TRY(hipSetDevice(h->device));
    h->nbatch = B;
    GP_TRY(ws_ensure_padded(h, N));
    const int64_t np = h->np;
    HIP_TRY(hipMemsetAsync(h->info, 0, sizeof(int32_t), h->stream));
    GP_TRY(launch_pad_copy(h, y, N, h->ypad, np));
    if (border_on(h)) GP_TRY(border_ensure(h));
    GP_TRY(factor_at_u(h, m, X, x_bs, N, u));
    if (border_on(h)) {
        GP_TRY(launch_lauum(h, h->A, h->B, np, h->ld, rag_of(N, np)));
        GP_TRY(border_iter(h, N, false));
    }
    return GPIMHIP_OK;
}

static int predict_impl(gpimhip_ctx* h, const gpimhip_model_t* m, const double* X, int64_t x_bs, const double* y,
                        int64_t N, int B, const double* u, const double* Xs, int64_t M, double* mean_out,
                        double* var_out) {
    GP_TRY(model_state_at_u(h, m, X, x_bs, y, N, B, u));
    GP_TRY(predict_cols(h, stationary_family(h, m, X, x_bs, N, B, Xs, M, mean_out, var_out), N, B));
    return finish_and_check(h);
}

// one evaluation of the objective and its gradient at u (one problem)
static int loss_grad_impl(gpimhip_ctx* h, const gpimhip_model_t* m, const double* X, const double* y, int64_t N, const double* u,
                          double* loss_out, double* grad_out, Objective obj) {
    read_finalize_knob(h);
    HIP_TRY(hipSetDevice(h->device));
    h->nbatch = 1;
    HIP_TRY(hipMemsetAsync(h->info, 0, sizeof(int32_t), h->stream));
    if (use_small_path(N) && obj == OBJ_NLL) {
        GP_TRY(launch_fit_small(h, m, X, 0, y, (int)N, const_cast<double*>(u), nullptr, nullptr, 0, nullptr,
                                loss_out, grad_out));
        return finish_and_check(h);
    }
    GP_TRY(ws_ensure_padded(h, N));
    if (obj == OBJ_LOO) GP_TRY(loo_obj_ensure(h));
    GP_TRY(launch_pad_copy(h, y, N, h->ypad, h->np));
    AdamStep st;
    memset(&st, 0, sizeof(st));
    GP_TRY(loss_grad_at_u(h, m, X, 0, N, const_cast<double*>(u), 0, st, loss_out, grad_out, nullptr, nullptr, obj));
    return finish_and_check(h);
}

int gpimhip_nll_grad(gpimhip_handle h, const gpimhip_model_t* m, const double* X, const double* y, int64_t N,
                     const double* u, double* loss_out, double* grad_out) {
    if (!h || !X || !y || !u || N < 1) return GPIMHIP_E_BADARG;
    GP_TRY(check_model(m));
    return loss_grad_impl(h, m, X, y, N, u, loss_out, grad_out, OBJ_NLL);
}

// The leave-one-out objective is built for ONE double-precision problem of the dense engine
static int loo_objective_refused(const gpimhip_ctx* h, const char* who) {
    const char* why = h->fp32 ? "a single-precision handle (d = diag(S^-1) and the loss's log d cancel in float matrices: gpimhip_set_precision(h, 64))"
                    : border_on(h) ? "a border (the missing points couple the blocks: diag(S^-1) is no sum of the blocks' diagonals)"
                    : (h->refl.pb_off != 0 || h->refl.pb_stride != 1 || h->refl.raw || h->refl.nblocks_total) && h->refl.mask
                        ? "a shard of reflection blocks (the objective is not a sum over the blocks)"
                    : h->refl.mask ? "reflection mode (a lock-step batch of blocks: the held-out terms mix the blocks' diagonals)"
                                   : nullptr;
    if (!why) return GPIMHIP_OK;
    gpim_set_error(std::string(who) + ": the leave-one-out objective is the dense double-precision model's, one problem per call; refused on " + why);
    return GPIMHIP_E_BADARG;
}

int gpimhip_loo_grad(gpimhip_handle h, const gpimhip_model_t* m, const double* X, const double* y, int64_t N, const double* u,
                     double* loss_out, double* grad_out) {
    if (!h || !X || !y || !u || N < 1) return GPIMHIP_E_BADARG;
    GP_TRY(check_model(m));
    GP_TRY(loo_objective_refused(h, "gpimhip_loo_grad"));
    return loss_grad_impl(h, m, X, y, N, u, loss_out, grad_out, OBJ_LOO);
}

int gpimhip_fit_exact_loo(gpimhip_handle h, const gpimhip_model_t* m, const double* X, const double* y, int64_t N,
                          double* u_inout, double lr, int32_t T, double* hist_out, double* loss_out) {
    if (!h || !X || !y || !u_inout || N < 1 || T < 0) return GPIMHIP_E_BADARG;
    GP_TRY(check_model(m));
    GP_TRY(loo_objective_refused(h, "gpimhip_fit_exact_loo"));
    return fit_impl(h, m, X, 0, y, N, 1, u_inout, lr, T, hist_out, loss_out, OBJ_LOO);
}

int gpimhip_fit_exact(gpimhip_handle h, const gpimhip_model_t* m, const double* X, const double* y, int64_t N,
                      double* u_inout, double lr, int32_t T, double* hist_out, double* loss_out) {
    if (!h || !X || !y || !u_inout || N < 1 || T < 0) return GPIMHIP_E_BADARG;
    GP_TRY(check_model(m));
    return fit_impl(h, m, X, 0, y, N, 1, u_inout, lr, T, hist_out, loss_out);
}

int gpimhip_predict_exact(gpimhip_handle h, const gpimhip_model_t* m, const double* X, const double* y, int64_t N,
                          const double* u, const double* Xs, int64_t M, double* mean_out, double* var_out) {
    if (!h || !X || !y || !u || !Xs || M < 1 || N < 1 || !mean_out || !var_out) return GPIMHIP_E_BADARG;
    GP_TRY(check_model(m));
    return predict_impl(h, m, X, 0, y, N, 1, u, Xs, M, mean_out, var_out);
}

int gpimhip_fit_exact_batched(gpimhip_handle h, const gpimhip_model_t* m, const double* X, int64_t x_stride,
                              const double* y, int64_t N, int32_t B, double* u_inout, double lr, int32_t T,
                              double* hist_out, double* loss_out) {
    if (!h || !X || !y || !u_inout || N < 1 || T < 0 || B < 1 || B > 65535 ||
        (x_stride != 0 && x_stride < N * (m ? m->dim : 1)))
        return GPIMHIP_E_BADARG;
    GP_TRY(check_model(m));
    return fit_impl(h, m, X, x_stride, y, N, B, u_inout, lr, T, hist_out, loss_out);
}

int gpimhip_predict_exact_batched(gpimhip_handle h, const gpimhip_model_t* m, const double* X, int64_t x_stride,
                                  const double* y, int64_t N, int32_t B, const double* u, const double* Xs,
                                  int64_t M, double* mean_out, double* var_out) {
    if (!h || !X || !y || !u || !Xs || M < 1 || N < 1 || !mean_out || !var_out || B < 1 || B > 65535)
        return GPIMHIP_E_BADARG;
    GP_TRY(check_model(m));
    return predict_impl(h, m, X, x_stride, y, N, B, u, Xs, M, mean_out, var_out);
}

int gpimhip_nll_grad_batched(gpimhip_handle h, const gpimhip_model_t* m, const double* X, int64_t x_stride, const double* y,
                             int64_t N, int32_t B, const double* u, double* loss_out, double* grad_out) {
    if (!h || !X || !y || !u || N < 1 || B < 1 || B > 65535 || !loss_out || !grad_out || (x_stride != 0 && x_stride < N * (m ? m->dim : 1)))
        return GPIMHIP_E_BADARG;
    GP_TRY(check_model(m));
    if (!h->refl.mask || h->fp32) {
        gpim_set_error("gpimhip_nll_grad_batched evaluates the coupled reflection blocks: needs reflection mode on a double-precision handle");
        return GPIMHIP_E_BADARG;
    }
    read_finalize_knob(h);
    HIP_TRY(hipSetDevice(h->device));
    h->nbatch = B;
    HIP_TRY(hipMemsetAsync(h->info, 0, sizeof(int32_t), h->stream));
    GP_TRY(ws_ensure_padded(h, N));
    if (border_on(h)) GP_TRY(border_ensure(h));
    GP_TRY(launch_pad_copy(h, y, N, h->ypad, h->np));
    AdamStep st;
    memset(&st, 0, sizeof(st));
    GP_TRY(loss_grad_at_u(h, m, X, x_stride, N, const_cast<double*>(u), 0, st, loss_out, grad_out, nullptr));
    return finish_and_check(h);
}

// Leave-one-out cross-validation (predict.hip: colsq_tri_kernel, loo_finish_kernel): the model's state at u, then the column
// sums of squares of L^-1 of every problem in one launch and the finisher.  No K^-1 product, no gradient contraction.  The
// row-chunk partial sums go to h->gemv_part (alpha has been summed out of it) and the score's to h->z (L^-1 y has served).
static int loo_impl(gpimhip_ctx* h, const gpimhip_model_t* m, const double* X, int64_t x_bs, const double* y, int64_t N, int B,
                    const double* u, const int32_t* rep, const int32_t* sgn, const double* y_grid, double* mean_out,
                    double* var_out, double* score_out) {
    GP_TRY(model_state_at_u(h, m, X, x_bs, y, N, B, u));
    const int64_t np = h->np;
    GP_TRY(launch_colsq_tri(h, h->A, h->ld, np, N, h->gemv_part));
    LooSrc s{rep ? y_grid : y, h->gemv_part, gemv_tri_chunks(np), gemv_tri_rc(np), np, h->alpha, rep ? B : 0, h->refl.wts, rep, sgn, N};
    GP_TRY(launch_loo_finish(h, s, rep ? h->refl.n_total : N, h->theta, h->z, mean_out, var_out, score_out));
    return finish_and_check(h);
}

int gpimhip_loo_exact(gpimhip_handle h, const gpimhip_model_t* m, const double* X, const double* y, int64_t N, const double* u,
                      double* mean_out, double* var_out, double* score_out) {
    if (!h || !X || !y || !u || N < 1 || !mean_out || !var_out || !score_out) return GPIMHIP_E_BADARG;
    GP_TRY(check_model(m));
    if (h->refl.mask) {
        gpim_set_error("gpimhip_loo_exact is the dense model's entry: in reflection mode use gpimhip_loo_exact_batched");
        return GPIMHIP_E_BADARG;
    }
    return loo_impl(h, m, X, 0, y, N, 1, u, nullptr, nullptr, nullptr, mean_out, var_out, score_out);
}

int gpimhip_loo_exact_batched(gpimhip_handle h, const gpimhip_model_t* m, const double* X, int64_t x_stride, const double* y,
                              int64_t N, int32_t B, const double* u, const int32_t* rep, const int32_t* sgn,
                              const double* y_grid, double* mean_out, double* var_out, double* score_out) {
    if (!h || !X || !y || !u || N < 1 || B < 1 || B > (1 << GPIMHIP_MAX_DIM) || !rep || !sgn || !y_grid || !mean_out ||
        !var_out || !score_out || (x_stride != 0 && x_stride < N * (m ? m->dim : 1)))
        return GPIMHIP_E_BADARG;
    GP_TRY(check_model(m));
    if (!h->refl.mask || h->fp32 || h->refl.n_total < 1) {
        gpim_set_error("gpimhip_loo_exact_batched combines the reflection blocks: needs reflection mode with n_total set on a double-precision handle");
        return GPIMHIP_E_BADARG;
    }
    if (border_on(h)) {
        gpim_set_error("gpimhip_loo_exact_batched: no leave-one-out through a border (the missing points couple the blocks: "
                       "diag(S^-1) is no longer a weighted sum of the blocks' diagonals)");
        return GPIMHIP_E_BADARG;
    }
    if (h->refl.pb_off != 0 || h->refl.pb_stride != 1 || h->refl.raw || (h->refl.nblocks_total && h->refl.nblocks_total != B)) {
        gpim_set_error("gpimhip_loo_exact_batched needs all blocks of the model on this handle (no shard)");
        return GPIMHIP_E_BADARG;
    }
    return loo_impl(h, m, X, x_stride, y, N, B, u, rep, sgn, y_grid, mean_out, var_out, score_out);
}

int gpimhip_set_reflection(gpimhip_handle h, int32_t mask, const double* twoc, const double* wts, int64_t n_total,
                           int64_t var_count) {
    if (!h || mask < 0 || mask >= (1 << GPIMHIP_MAX_DIM) || (mask && !twoc) || n_total < 0 || var_count < 0) return GPIMHIP_E_BADARG;
    if (mask && h->fp32) {
        gpim_set_error("the symmetry-reduced model computes in double precision");
        return GPIMHIP_E_BADARG;
    }
    h->refl.mask = mask;
    for (int k = 0; k < GPIMHIP_MAX_DIM; ++k) h->refl.twoc[k] = mask ? twoc[k] : 0.0;
    h->refl.wts = mask ? wts : nullptr;
    h->refl.n_total = mask ? n_total : 0;
    h->refl.var_count = mask ? var_count : 0;
    if (!mask) { h->refl.pb_off = 0; h->refl.pb_stride = 1; h->refl.nblocks_total = 0; h->refl.raw = 0; }
    if (!mask && h->border) bws(h)->M = 0;
    return GPIMHIP_OK;
}

int gpimhip_set_border(gpimhip_handle h, int32_t M, const int32_t* q, const double* coef) {
    if (!h || M < 0 || (M > 0 && (!q || !coef))) return GPIMHIP_E_BADARG;
    if (M > 0 && (!h->refl.mask || h->fp32 || h->refl.pb_stride != 1 || h->refl.raw)) {
        gpim_set_error("gpimhip_set_border needs reflection mode (gpimhip_set_reflection) on a double-precision handle, unsharded");
        return GPIMHIP_E_BADARG;
    }
    if (!h->border) {
        if (M == 0) return GPIMHIP_OK;
        h->border = new BorderWs();
    }
    BorderWs* w = bws(h);
    w->M = M;
    w->q = M ? q : nullptr;
    w->coef = M ? coef : nullptr;
    return GPIMHIP_OK;
}

int gpimhip_set_reflection_shard(gpimhip_handle h, int32_t pb_off, int32_t pb_stride, int32_t nblocks_total, int32_t raw) {
    if (!h || pb_off < 0 || pb_stride < 1 || nblocks_total < 0 || nblocks_total > (1 << GPIMHIP_MAX_DIM)) return GPIMHIP_E_BADARG;
    h->refl.pb_off = pb_off;
    h->refl.pb_stride = pb_stride;
    h->refl.nblocks_total = nblocks_total;
    h->refl.raw = raw ? 1 : 0;
    return GPIMHIP_OK;
}

int gpimhip_refl_sums(gpimhip_handle h, const gpimhip_model_t* m, const double* X, const double* y, int64_t N, int32_t B,
                      const double* u, double* sums_out) {
    if (!h || !X || !y || !u || !sums_out || N < 1 || B < 1 || B > (1 << GPIMHIP_MAX_DIM) || !h->refl.mask) return GPIMHIP_E_BADARG;
    FP64_ONLY(h);
    GP_TRY(check_model(m));
    HIP_TRY(hipSetDevice(h->device));
    h->nbatch = B;
    HIP_TRY(hipMemsetAsync(h->info, 0, sizeof(int32_t), h->stream));
    GP_TRY(ws_ensure_padded(h, N));
    const int64_t np = h->np;
    GP_TRY(launch_pad_copy(h, y, N, h->ypad, np));
    GP_TRY(factor_at_u(h, m, X, 0, N, u));
    GP_TRY(launch_lauum(h, h->A, h->B, np, h->ld, rag_of(N, np)));
    GP_TRY(launch_grad_reduce_refl(h, m, h->B, h->ld, X, N, (int)(np / NB), h->alpha, 0));
    return launch_coupled_sums(h, np, sums_out);
}

}  // extern "C"
