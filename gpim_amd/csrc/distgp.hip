// distgp.hip -- host drivers of the multi-GPU exact GP (gpimhip_dist_*, gpimhip_matvec_t; include/gpimhip.h, DESIGN.md
// section 6): the building blocks of the block-column-cyclic (1 x P) factorisation, the panel-wise solves and the distributed
// training passes that gpim_amd/dist_chol.py drives.  Host code only: the kernels and their launchers are in distops.hip,
// cholstep.hip, engine.hip and grad.hip, the engine's drivers (workspaces, tile engine) in api.hip.
#include <math.h>
#include <algorithm>
#include <vector>
#include "common.hpp"

// ---- distributed (block-column-cyclic, 1 x P) exact GP: building blocks (see include/gpimhip.h) ----
void dist_plan_release(gpimhip_ctx* h) {
    DistPlan& D = h->dplan;
    if (D.d_tiles) (void)hipFree(D.d_tiles);
    if (D.d_rect) (void)hipFree(D.d_rect);
    D = DistPlan();
}
// the distributed entry points address the workspace (diagonal-block inverses, batch strides) through the plan's block
// count: a handle whose workspace was re-sized after gpimhip_dist_setup must not be used with the stale plan
static bool dist_plan_ok(const gpimhip_ctx* h) { return h && h->np && h->dplan.nb && h->np == (int64_t)h->dplan.nb * NB; }

extern "C" {

static int upload_tiles(gpimhip_ctx* h, const std::vector<TileDesc>& tl, TileDesc** out) {
    void* q = nullptr;
    HIP_TRY(hipMalloc(&q, std::max<size_t>(tl.size(), 1) * sizeof(TileDesc)));
    *out = (TileDesc*)q;
    HIP_TRY(hipMemcpyAsync(q, tl.data(), tl.size() * sizeof(TileDesc), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return GPIMHIP_OK;
}

int gpimhip_dist_setup(gpimhip_handle h, int64_t n, int32_t world, int32_t rank) {
    FP64_ONLY(h);
    if (!h || n < 1 || world < 1 || rank < 0 || rank >= world) return GPIMHIP_E_BADARG;
    HIP_TRY(hipSetDevice(h->device));
    h->nbatch = 1;
    GP_TRY(ws_ensure_b(h, n, 1, 0, false));
    HIP_TRY(hipMemsetAsync(h->info, 0, sizeof(int32_t), h->stream));
    const int nb = (int)(h->np / NB);
    DistPlan& D = h->dplan;
    if (D.nb == nb && D.world == world && D.rank == rank) return GPIMHIP_OK;
    dist_plan_release(h);
    std::vector<TileDesc> tl;
    auto mark = [&](size_t start) { return PlanRange{(int64_t)start, (int32_t)(tl.size() - start)}; };
    D.colfill.assign(nb, {0, 0});
    const int npanel = (nb + OUTER_W - 1) / OUTER_W;
    D.upd_panel.assign(npanel, {0, 0});
    for (int j = 0; j < nb; ++j) {
        const int p0 = (j / OUTER_W) * OUTER_W;
        size_t s0 = tl.size();
        if (j > p0)
            for (int i = j + 1; i < nb; ++i) tl.push_back({i, j, p0, j});
        D.colfill[j] = mark(s0);
    }
    // trailing-update tiles of the owned panels, ascending: a round updates a contiguous range of them.  kb0 carries
    // the LOCAL block column of the output (GemmArgs::cmap), the k-range comes from kfix.
    int slot = 0;
    for (int c = 0; c < npanel; ++c) {
        if (c % world != rank) continue;
        size_t s0 = tl.size();
        const int j0 = c * OUTER_W, j1 = std::min(j0 + OUTER_W, nb);
        for (int ig = j0 / 8; ig <= (nb - 1) / 8; ++ig)
            for (int i = std::max(j0, ig * 8); i < std::min(nb, ig * 8 + 8); ++i)
                for (int j = j0; j < std::min(j1, i + 1); ++j) tl.push_back({i, j, slot * OUTER_W + (j - j0), 0});
        D.upd_panel[c] = mark(s0);
        ++slot;
    }
    // training: K^-1 = X^T X row panel by row panel (X = L^-1, broadcast panel c) against the owned columns, and the
    // owned lower tiles of K^-1 for the gradient contraction.  Local block lb <-> global block gblk[lb].
    std::vector<int> gblk;
    for (int c = 0; c < npanel; ++c)
        if (c % world == rank)
            for (int j = c * OUTER_W; j < std::min(c * OUTER_W + OUTER_W, nb); ++j) gblk.push_back(j);
    // (a rank's last owned panel may be the ragged one: its local blocks still sit at slot * 4 + offset)
    auto local_of = [&](int lbidx) { return (gblk[lbidx] / OUTER_W / world) * OUTER_W + gblk[lbidx] % OUTER_W; };
    D.kinv_panel.assign(npanel, {0, 0});
    for (int c = 0; c < npanel; ++c) {
        size_t s0 = tl.size();
        // 64 consecutive tiles = the panel's four block rows x 16 owned columns: dealt to the XCDs in chunks of 64
        // (gpimhip_dist_kinv_update) a patch streams 4 + 16 operand panels for 64 tiles (row by row it was 1 + 64, and the
        // pass ran at 56 TFLOP/s at N = 65536)
        const int ci1 = std::min(c * OUTER_W + OUTER_W, nb);
        for (size_t q0 = 0; q0 < gblk.size(); q0 += 16)
            for (int ci = c * OUTER_W; ci < ci1; ++ci)
                for (size_t q = q0; q < std::min(gblk.size(), q0 + 16); ++q)
                    if (gblk[q] <= ci) tl.push_back({ci, local_of((int)q), ci, nb});
        D.kinv_panel[c] = mark(s0);
    }
    {
        size_t s0 = tl.size();
        for (size_t q = 0; q < gblk.size(); ++q)
            for (int ci = gblk[q]; ci < nb; ++ci) tl.push_back({ci, gblk[q], local_of((int)q), 0});
        D.grad_tiles = mark(s0);
    }
    D.n_tiles = (int64_t)tl.size();
    GP_TRY(upload_tiles(h, tl, &D.d_tiles));
    D.nb = nb; D.world = world; D.rank = rank;
    return GPIMHIP_OK;
}

int gpimhip_dist_begin(gpimhip_handle h, int64_t n) { return gpimhip_dist_setup(h, n, 1, 0); }

int gpimhip_dist_panel_factor(gpimhip_handle h, double* Aloc, int64_t ldloc, int32_t loc_blk0, int32_t glob_blk0,
                              double* logdet_out, int32_t* info) {
    FP64_ONLY(h);
    if (!h || !Aloc || !info || loc_blk0 < 0 || glob_blk0 < 0 || !dist_plan_ok(h)) return GPIMHIP_E_BADARG;
    HIP_TRY(hipSetDevice(h->device));
    const int nb = (int)(h->np / NB);
    if (glob_blk0 >= nb || glob_blk0 % OUTER_W || ldloc < (int64_t)(loc_blk0 + std::min(OUTER_W, nb - glob_blk0)) * NB)
        return GPIMHIP_E_BADARG;
    h->nbatch = 1;
    // the panel's columns live at local block offset loc_blk0: shift the base so that GLOBAL column indices
    // address them (the chain only touches columns of this panel)
    double* As = Aloc - (int64_t)(glob_blk0 - loc_blk0) * NB;
    const int p1 = std::min(glob_blk0 + OUTER_W, nb);
    GP_TRY(launch_panel_chain(h, As, ldloc, glob_blk0, p1, nb, h->dplan.d_tiles, h->dplan.colfill.data() + glob_blk0, info));
    if (logdet_out)
        HIP_TRY(hipMemcpyAsync(logdet_out, h->logdet_part + glob_blk0, (size_t)(p1 - glob_blk0) * sizeof(double),
                               hipMemcpyDeviceToDevice, h->stream));
    return GPIMHIP_OK;
}

// The panel-wise vector solves of alpha = K^-1 y on the owner of panel [glob_blk0, glob_blk0 + 4) (distops.hip):
//   forward : piece (512) = Lpp^-1 (y_p - t);  acc[rows below the panel] += L(below, p) piece
//   backward: piece = Lpp^-T (z_p - L(below, p)^T a[below])
// y_p / z_p / t / piece: the panel's 512 entries (device); acc / a: full-length (np) vectors.  Needs the inverses of the
// panel's diagonal blocks, i.e. the handle that factored the panel (gpimhip_dist_panel_factor).
int gpimhip_dist_vec_forward(gpimhip_handle h, const double* Aloc, int64_t ldloc, int32_t loc_blk0, int32_t glob_blk0,
                             const double* y_p, const double* t, double* piece, double* acc) {
    FP64_ONLY(h);
    if (!h || !Aloc || !y_p || !piece || !acc || !dist_plan_ok(h) || glob_blk0 < 0 || loc_blk0 < 0 || glob_blk0 % OUTER_W)
        return GPIMHIP_E_BADARG;
    HIP_TRY(hipSetDevice(h->device));
    const int nb = (int)(h->np / NB);
    if (glob_blk0 >= nb) return GPIMHIP_E_BADARG;
    const int nblk = std::min(OUTER_W, nb - glob_blk0), w = nblk * NB;
    const int64_t r0 = (int64_t)glob_blk0 * NB;
    const double* P = Aloc + r0 * ldloc + (int64_t)loc_blk0 * NB;
    GP_TRY(launch_dist_trsv(h, P, ldloc, h->dinv + (int64_t)glob_blk0 * NB * NB, nblk, 0, y_p, t, piece));
    return launch_dist_rows_acc(h, P + (int64_t)w * ldloc, ldloc, h->np - r0 - w, w, piece, acc + r0 + w);
}
int gpimhip_dist_vec_backward(gpimhip_handle h, const double* Aloc, int64_t ldloc, int32_t loc_blk0, int32_t glob_blk0,
                              const double* z_p, const double* a, double* work, double* piece) {
    FP64_ONLY(h);
    if (!h || !Aloc || !z_p || !a || !work || !piece || !dist_plan_ok(h) || glob_blk0 < 0 || loc_blk0 < 0 ||
        glob_blk0 % OUTER_W)
        return GPIMHIP_E_BADARG;
    HIP_TRY(hipSetDevice(h->device));
    const int nb = (int)(h->np / NB);
    if (glob_blk0 >= nb) return GPIMHIP_E_BADARG;
    const int nblk = std::min(OUTER_W, nb - glob_blk0), w = nblk * NB;
    const int64_t r0 = (int64_t)glob_blk0 * NB, below = h->np - r0 - w;
    const double* P = Aloc + r0 * ldloc + (int64_t)loc_blk0 * NB;
    h->nbatch = 1;
    // work (512) = L(below, p)^T a[below]
    if (below > 0) GP_TRY(launch_gemv_t(h, P + (int64_t)w * ldloc, ldloc, below, w, a + r0 + w, work, 0, 0, 0, 0));
    else HIP_TRY(hipMemsetAsync(work, 0, (size_t)w * sizeof(double), h->stream));
    return launch_dist_trsv(h, P, ldloc, h->dinv + (int64_t)glob_blk0 * NB * NB, nblk, 1, z_p, work, piece);
}
// out (ncols) = A^T x for a row-major nrows x ncols matrix (ncols a multiple of 64): the posterior mean K*^T alpha of
// the distributed model (HBM-bound, fixed summation order)
int gpimhip_matvec_t(gpimhip_handle h, const double* A, int64_t ld, int64_t nrows, int64_t ncols, const double* x,
                     double* out) {
    FP64_ONLY(h);
    if (!h || !A || !x || !out || nrows < 1 || ncols < 64 || ncols % 64 || ld < ncols) return GPIMHIP_E_BADARG;
    HIP_TRY(hipSetDevice(h->device));
    h->nbatch = 1;
    return launch_gemv_t(h, A, ld, nrows, ncols, x, out, 0, 0, 0, 0);
}

int gpimhip_dist_panel_pack(gpimhip_handle h, const double* Aloc, int64_t ldloc, int32_t loc_blk0, int32_t glob_blk0,
                            double* buf, int64_t ldbuf) {
    FP64_ONLY(h);
    if (!h || !Aloc || !buf || !dist_plan_ok(h) || glob_blk0 < 0 || loc_blk0 < 0 || ldbuf < OUTER_W * NB)
        return GPIMHIP_E_BADARG;
    HIP_TRY(hipSetDevice(h->device));
    const int nb = (int)(h->np / NB);
    if (glob_blk0 >= nb || glob_blk0 % OUTER_W) return GPIMHIP_E_BADARG;
    const int nblk = std::min(OUTER_W, nb - glob_blk0);
    return launch_dist_pack(h, Aloc + (int64_t)loc_blk0 * NB, ldloc, (int64_t)glob_blk0 * NB, h->np, nblk * NB,
                            h->dinv + (int64_t)glob_blk0 * NB * NB, nblk, buf, ldbuf);
}

int gpimhip_dist_update(gpimhip_handle h, const double* buf, int64_t ldbuf, int32_t panel_glob_blk0, double* Aloc,
                        int64_t ldloc, int32_t panel_first, int32_t panel_last) {
    FP64_ONLY(h);
    if (!h || !buf || !Aloc || !dist_plan_ok(h) || panel_glob_blk0 < 0 || panel_glob_blk0 % OUTER_W)
        return GPIMHIP_E_BADARG;
    HIP_TRY(hipSetDevice(h->device));
    const DistPlan& D = h->dplan;
    const int nb = D.nb, npanel = (int)D.upd_panel.size();
    if (panel_glob_blk0 >= nb || panel_first <= panel_glob_blk0 / OUTER_W) return GPIMHIP_E_BADARG;
    h->nbatch = 1;
    panel_last = std::min<int32_t>(panel_last, npanel);
    int64_t off = -1, cnt = 0;
    for (int c = panel_first; c < panel_last; ++c) {
        if (!D.upd_panel[c].n) continue;
        if (off < 0) off = D.upd_panel[c].off;
        cnt += D.upd_panel[c].n;                     // owned panels are stored back to back, ascending
    }
    if (cnt == 0) return GPIMHIP_OK;
    // operands: the broadcast buffer holds columns [panel_glob_blk0, +kblk) of L for all rows; the shifted base lets
    // the tile engine use global block indices for them
    const int kblk = std::min(OUTER_W, nb - panel_glob_blk0);
    const double* Ps = buf - (int64_t)panel_glob_blk0 * NB;
    GemmArgs g = gemm_args(Ps, ldbuf, Ps, ldbuf, Aloc, ldloc, -1.0, 1.0, D.d_tiles + off, (int)cnt, h->np);
    g.kfix0 = panel_glob_blk0;
    g.kfix1 = panel_glob_blk0 + kblk;
    g.cmap = 1;
    return launch_gemm(h, false, false, EPI_STORE, g);
}

static int dist_rect_ensure(gpimhip_ctx* h, int cols) {
    DistPlan& D = h->dplan;
    if (D.rect_cols == cols && D.d_rect) return GPIMHIP_OK;
    if (D.d_rect) { (void)hipFree(D.d_rect); D.d_rect = nullptr; }
    std::vector<TileDesc> tl;
    tl.reserve((size_t)D.nb * cols);
    for (int r = 0; r < D.nb; ++r)
        for (int c = 0; c < cols; ++c) tl.push_back({r, c, 0, 1});
    D.n_rect = (int64_t)tl.size();
    GP_TRY(upload_tiles(h, tl, &D.d_rect));
    D.rect_cols = cols;
    return GPIMHIP_OK;
}

// One panel step of the forward substitution  W = L^-1 B  for this rank's right-hand sides B (np x mpad, row-major,
// destroyed), against the broadcast buffer of panel p (gpimhip_dist_panel_pack):
//   for b = 0..3:  W_b = Dinv_b B[4p+b]   ->  Wt rows [128 b, +128)
//                  B[4p+b+1 .. 4p+3] -= L[., 4p+b] W_b                       (rows inside the panel)
//   B[4p+4 ..] -= L[., panel p] Wt                                           (k-depth 512)
//   q[j] += sum over the panel's rows of W[r][j]^2
// The last line rewrites the rank's whole share of B below the panel once per panel: at N = 65536 the streamed inverse
// moved 4.4 TB that way and ran at 39 TFLOP/s.  Panels therefore go in PAIRS where the caller can hold two of them
// (gpimhip_dist_solve_update2): the first panel of a pair updates only the block rows of the second, and after the second
// panel's own solves ONE update of k-depth 1024 -- both panels side by side in a buffer of 1024 columns, both W's
// one below the other -- brings the rest of B up to date: half the passes over B.
static int dist_solve_panel(gpimhip_ctx* h, const double* buf, int64_t ldbuf, int g0, double* Bm, int64_t ldb, int cols,
                            double* Wt, int64_t ldw, int32_t col_tiles) {
    const DistPlan& D = h->dplan;
    const int nb = D.nb, nblk = std::min(OUTER_W, nb - g0);
    const double* dinv = buf + h->np * ldbuf;               // 128 x (128 nblk): the panel's diagonal-block inverses
    const double* Ps = buf - (int64_t)g0 * NB;              // global k-block index -> buffer column
    for (int b = 0; b < nblk; ++b) {
        // W_b = Dinv_b * B[g0 + b]   (NN: A = Dinv_b k-contiguous, B = right-hand sides m-contiguous)
        GemmArgs g = gemm_args(dinv + (int64_t)b * NB, ldbuf, Bm + (int64_t)(g0 + b) * NB * ldb, ldb,
                               Wt + (int64_t)b * NB * ldw, ldw, 1.0, 0.0, D.d_rect, cols, h->np);
        g.kfix0 = 0; g.kfix1 = 1;
        g.cj_max = col_tiles;
        GP_TRY(launch_gemm(h, false, true, EPI_STORE, g));
        const int rows_in = nblk - 1 - b;
        if (rows_in > 0) {
            // B[g0+b+1 .. g0+nblk-1] -= L[., g0+b] * W_b
            GemmArgs u = gemm_args(Ps, ldbuf, Wt + (int64_t)b * NB * ldw, ldw, Bm, ldb, -1.0, 1.0, D.d_rect,
                                   rows_in * cols, h->np);
            u.a_roff = g0 + b + 1; u.a_coff = g0 + b; u.c_roff = g0 + b + 1;
            u.kfix0 = 0; u.kfix1 = 1;
            u.cj_max = col_tiles;
            GP_TRY(launch_gemm(h, false, true, EPI_STORE, u));
        }
    }
    return GPIMHIP_OK;
}
// B[row0 .. row0 + nrows) -= L[., kb0 .. kb0 + kblk) * Wt  (block indices; abase: the buffer whose column 0 is block column kb0)
static int dist_solve_below(gpimhip_ctx* h, const double* abase, int64_t ldbuf, int kb0, int kblk, int row0, int nrows,
                            double* Bm, int64_t ldb, int cols, const double* Wt, int64_t ldw, int32_t col_tiles) {
    if (nrows <= 0) return GPIMHIP_OK;
    const DistPlan& D = h->dplan;
    const double* Ps = abase - (int64_t)kb0 * NB;
    // only the column tiles that are not structurally zero, in 8 x 8 patches, one patch per XCD at a time (until round 5:
    // the row-major list over ALL column tiles with the zero ones leaving at once -- three workgroups in four at the
    // middle of an inverse -- and a row of 100-500 tiles between two uses of a W panel: 37 TFLOP/s per launch)
    const int ncol = col_tiles > 0 ? std::min<int>(col_tiles, cols) : cols;
    GemmArgs u = gemm_args(Ps, ldbuf, Wt, ldw, Bm, ldb, -1.0, 1.0, D.d_rect, nrows * ncol, h->np);
    u.a_roff = row0; u.a_coff = kb0; u.c_roff = row0;
    u.kfix0 = 0; u.kfix1 = kblk;
    u.rect_rows = nrows; u.rect_cols = ncol;
    u.chunk = 64;
    return launch_gemm(h, false, true, EPI_STORE, u);
}
static int dist_solve_check(gpimhip_ctx* h, const double* buf, int32_t g0, const double* Bm, int64_t ldb, int64_t mpad,
                            const double* Wt, int64_t ldw) {
    if (!h || !buf || !Bm || !Wt || !dist_plan_ok(h) || g0 < 0 || g0 % OUTER_W || mpad < NB || mpad % NB || ldb < mpad ||
        ldw < mpad || g0 >= h->dplan.nb)
        return GPIMHIP_E_BADARG;
    return GPIMHIP_OK;
}
int gpimhip_dist_solve_update(gpimhip_handle h, const double* buf, int64_t ldbuf, int32_t panel_glob_blk0, double* Bm,
                              int64_t ldb, int64_t mpad, double* Wt, int64_t ldw, double* q, int32_t col_tiles) {
    FP64_ONLY(h);
    GP_TRY(dist_solve_check(h, buf, panel_glob_blk0, Bm, ldb, mpad, Wt, ldw));
    HIP_TRY(hipSetDevice(h->device));
    const DistPlan& D = h->dplan;
    const int nb = D.nb, g0 = panel_glob_blk0;
    h->nbatch = 1;
    const int cols = (int)(mpad / NB), nblk = std::min(OUTER_W, nb - g0);
    GP_TRY(dist_rect_ensure(h, cols));
    GP_TRY(dist_solve_panel(h, buf, ldbuf, g0, Bm, ldb, cols, Wt, ldw, col_tiles));
    GP_TRY(dist_solve_below(h, buf, ldbuf, g0, nblk, g0 + nblk, nb - g0 - nblk, Bm, ldb, cols, Wt, ldw, col_tiles));
    if (q) GP_TRY(launch_colsumsq_acc(h, Wt, ldw, nblk * NB, mpad, q));
    return GPIMHIP_OK;
}
// The same step for the panels of a PAIR held side by side: `wide` is a buffer of 1024 columns (leading dimension ldbuf
// >= 1024) with the pair's first panel in columns [0, 512) and the second in [512, 1024), both packed like the
// single-panel buffer (np rows + 128 rows of diagonal-block inverses); Wt2 holds 1024 rows.
//   second = 0: the pair's first panel (global block panel_glob_blk0): its own solves, W -> rows [0, 512) of Wt2, and the
//               update of the NEXT panel's block rows only;
//   second = 1: the pair's second panel (panel_glob_blk0 = the first panel's + 4): its own solves, W -> rows [512, 1024),
//               then every block row below it receives both panels at once (k-depth 1024).
int gpimhip_dist_solve_update2(gpimhip_handle h, const double* wide, int64_t ldbuf, int32_t panel_glob_blk0, double* Bm,
                               int64_t ldb, int64_t mpad, double* Wt2, int64_t ldw, double* q, int32_t col_tiles,
                               int32_t second) {
    FP64_ONLY(h);
    GP_TRY(dist_solve_check(h, wide, panel_glob_blk0, Bm, ldb, mpad, Wt2, ldw));
    if (ldbuf < 2 * OUTER_W * NB || (second && panel_glob_blk0 < OUTER_W)) return GPIMHIP_E_BADARG;
    HIP_TRY(hipSetDevice(h->device));
    const DistPlan& D = h->dplan;
    const int nb = D.nb, g0 = panel_glob_blk0;
    h->nbatch = 1;
    const int cols = (int)(mpad / NB), nblk = std::min(OUTER_W, nb - g0);
    GP_TRY(dist_rect_ensure(h, cols));
    const double* half = wide + (second ? OUTER_W * NB : 0);
    double* Wh = Wt2 + (second ? (int64_t)OUTER_W * NB * ldw : 0);
    GP_TRY(dist_solve_panel(h, half, ldbuf, g0, Bm, ldb, cols, Wh, ldw, col_tiles));
    if (!second)
        GP_TRY(dist_solve_below(h, half, ldbuf, g0, nblk, g0 + nblk, std::min(OUTER_W, nb - g0 - nblk), Bm, ldb, cols, Wh, ldw,
                                col_tiles));
    else
        GP_TRY(dist_solve_below(h, wide, ldbuf, g0 - OUTER_W, OUTER_W + nblk, g0 + nblk, nb - g0 - nblk, Bm, ldb, cols, Wt2,
                                ldw, col_tiles));
    if (q) GP_TRY(launch_colsumsq_acc(h, Wh, ldw, nblk * NB, mpad, q));
    return GPIMHIP_OK;
}

// ---- distributed training: covariance columns at u, K^-1 rows, gradient sums, finalize ----
int gpimhip_dist_kmat_cols(gpimhip_handle h, const gpimhip_model_t* m, const double* X, int64_t N, const double* u,
                           int64_t col0, int64_t ncols_pad, double* out, int64_t ld) {
    FP64_ONLY(h);
    if (!h || !X || !u || !out || N < 1 || col0 < 0 || ncols_pad < NB || ncols_pad % NB || ld < ncols_pad || !h->np)
        return GPIMHIP_E_BADARG;
    GP_TRY(check_model(m));
    HIP_TRY(hipSetDevice(h->device));
    h->nbatch = 1;
    GP_TRY(launch_theta(h, m, u));
    const int64_t M = std::max<int64_t>(0, std::min(ncols_pad, N - col0));
    GP_TRY(launch_kmat(h, m, X, N, X + std::min(col0, N - 1) * m->dim, M, h->theta, 0.0, 0, out, ld, h->np, ncols_pad, 0, 0, 0,
                       0, 0));
    return launch_add_diag_theta(h, out, ld, col0, M, std::min(ncols_pad, h->np - col0));
}

int gpimhip_dist_kinv_update_n(gpimhip_handle h, const double* xbuf, int64_t ldx, int32_t panel_glob_blk0, int32_t npanels,
                               const double* Xloc, int64_t ldloc, double* Kinv, int64_t ldk) {
    FP64_ONLY(h);
    if (!h || !xbuf || !Xloc || !Kinv || !dist_plan_ok(h) || panel_glob_blk0 < 0 || panel_glob_blk0 % OUTER_W ||
        panel_glob_blk0 >= h->dplan.nb || npanels < 1)
        return GPIMHIP_E_BADARG;
    HIP_TRY(hipSetDevice(h->device));
    h->nbatch = 1;
    const DistPlan& D = h->dplan;
    const int p0 = panel_glob_blk0 / OUTER_W, p1 = std::min<int>(p0 + npanels, (int)D.kinv_panel.size());
    // the tile lists of consecutive panels are adjacent in the plan (dist_plan_build): one launch for all of them
    PlanRange r = D.kinv_panel[p0];
    for (int p = p0 + 1; p < p1; ++p) r.n += D.kinv_panel[p].n;
    if (!r.n) return GPIMHIP_OK;
    // K^-1[ci, cj] = sum_{kb >= ci} X[kb, ci]^T X[kb, cj]: A = the broadcast column panels of X side by side (block column
    // ci - panel_glob_blk0 of xbuf), B = the owned columns
    GemmArgs g = gemm_args(xbuf, ldx, Xloc, ldloc, Kinv, ldk, 1.0, 0.0, D.d_tiles + r.off, r.n, h->np);
    g.a_coff = -panel_glob_blk0;
    g.krev = 1;
    g.chunk = 64;
    return launch_gemm(h, true, true, EPI_STORE, g);
}
int gpimhip_dist_kinv_update(gpimhip_handle h, const double* xbuf, int64_t ldx, int32_t panel_glob_blk0,
                             const double* Xloc, int64_t ldloc, double* Kinv, int64_t ldk) {
    return gpimhip_dist_kinv_update_n(h, xbuf, ldx, panel_glob_blk0, 1, Xloc, ldloc, Kinv, ldk);
}

int gpimhip_dist_grad_sums(gpimhip_handle h, const gpimhip_model_t* m, const double* X, int64_t N, const double* u,
                           const double* Kinv, int64_t ldk, const double* alpha, double* S_out) {
    FP64_ONLY(h);
    if (!h || !X || !u || !Kinv || !alpha || !S_out || !dist_plan_ok(h)) return GPIMHIP_E_BADARG;
    GP_TRY(check_model(m));
    HIP_TRY(hipSetDevice(h->device));
    h->nbatch = 1;
    const DistPlan& D = h->dplan;
    GP_TRY(launch_theta(h, m, u));
    if (D.grad_tiles.n)
        GP_TRY(launch_grad_reduce_tiles(h, m, Kinv, ldk, X, N, h->np, alpha, D.d_tiles + D.grad_tiles.off, D.grad_tiles.n,
                                        h->grad_part));
    return launch_sum7(h, h->grad_part, D.grad_tiles.n, S_out);
}

int gpimhip_dist_finalize(gpimhip_handle h, const gpimhip_model_t* m, int64_t N, double* u, const double* S, double quad,
                          double half_logdet, double lr, int32_t t, double* loss_out, double* grad_out, double* hist_row) {
    FP64_ONLY(h);
    if (!h || !u || !S || N < 1 || t < 0 || !h->np) return GPIMHIP_E_BADARG;
    GP_TRY(check_model(m));
    HIP_TRY(hipSetDevice(h->device));
    h->nbatch = 1;
    GP_TRY(launch_theta(h, m, u));
    AdamStep st = adam_step_init();
    st.lr_over_bc1 = t > 0 ? lr / (1.0 - pow(0.9, (double)t)) : 0.0;
    st.bc2_sqrt = t > 0 ? sqrt(1.0 - pow(0.999, (double)t)) : 1.0;
    if (t == 1) {
        HIP_TRY(hipMemsetAsync(h->adam_m, 0, MAXP * sizeof(double), h->stream));
        HIP_TRY(hipMemsetAsync(h->adam_v, 0, MAXP * sizeof(double), h->stream));
    }
    return launch_dist_finalize(h, m, N, S, quad, half_logdet, u, t > 0 ? 1 : 0, st, loss_out, grad_out, hist_row);
}

int gpimhip_dist_finalize_dev(gpimhip_handle h, const gpimhip_model_t* m, int64_t N, double* u, const double* red,
                              const double* quad, double lr, int32_t t, double* loss_out, double* grad_out,
                              double* hist_row) {
    FP64_ONLY(h);
    if (!h || !u || !red || !quad || N < 1 || t < 0) return GPIMHIP_E_BADARG;
    GP_TRY(check_model(m));
    HIP_TRY(hipSetDevice(h->device));
    h->nbatch = 1;
    // a rank that holds no block of the model (world size > number of reflection blocks) never built a workspace:
    // the parameters and the Adam state are all this call needs
    if (!h->np) GP_TRY(ws_ensure_b(h, 1, 1, 0, false));
    GP_TRY(launch_theta(h, m, u));
    AdamStep st = adam_step_init();
    st.lr_over_bc1 = t > 0 ? lr / (1.0 - pow(0.9, (double)t)) : 0.0;
    st.bc2_sqrt = t > 0 ? sqrt(1.0 - pow(0.999, (double)t)) : 1.0;
    if (t == 1) {
        HIP_TRY(hipMemsetAsync(h->adam_m, 0, MAXP * sizeof(double), h->stream));
        HIP_TRY(hipMemsetAsync(h->adam_v, 0, MAXP * sizeof(double), h->stream));
    }
    return launch_dist_finalize_dev(h, m, N, red, quad, u, t > 0 ? 1 : 0, st, loss_out, grad_out, hist_row);
}

}  // extern "C"
