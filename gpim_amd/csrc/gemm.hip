// gemm.hip -- the fp64 MFMA tile engine of libgpimhip.
//
// One kernel template covers every O(N^3) stage of the exact-GP hot path
// (SURVEY 8(a) rows a6, a8, a11): Cholesky panel solves and trailing SYRK updates,
// the triangular inverse, K^-1 = L^-T L^-1 and the predictive-variance product
// L^-1 K(X, X*).  Work is described by a list of 128x128 output tiles, each with its own
// k-block range, so triangular operands simply get shorter ranges (no wasted MFMAs on
// structural zeros) and the host can order the list for XCD/L2 locality.
//
// Tile engine: 256 threads = 4 waves (2x2), each wave owns a 64x64 sub-tile = 4x4
// v_mfma_f64_16x16x4_f64 accumulators (128 VGPRs).  Two more shapes serve launches that cannot fill
// the chip with one 4-wave workgroup per 128x128 tile: 8 waves per tile (two MFMA waves on every
// SIMD of the tile's CU) and 64x64 sub-tiles (a 128x128 tile spread over 4 CUs) -- the panel
// solves / in-panel updates of the Cholesky are latency-bound chains of such small launches.
// Operand tiles are double-buffered in LDS, one barrier per 16-deep k-step.  128-wide tiles are staged
// global -> LDS directly (global_load_lds_dwordx4, one wave-wide 16-byte load per 1 KB of LDS, no
// VGPR staging and no ds_write); 64-wide tiles go global -> registers -> LDS.  Every global access is
// a coalesced 16-byte load whatever the transpose:
//   "KM" operand (row-major, m contiguous):  lds[16][128+16]; one load per k-row
//   "MK" operand (row-major, k contiguous):  1 KB groups of 8 rows x 8 chunks, chunk index XOR row
//                                            (direct), or lds[64][16+2] (through registers)
// The MFMA block of a k-step runs at raised wave priority (s_setprio).
// v_mfma_f64_16x16x4_f64 lane maps (cdna_hip_programming.md section 3):
//   A[l&15][l>>4], B[l>>4][l&15], C/D col = l&15, row = (l>>4) + 4*reg.
#include <stdlib.h>
#include <string.h>
#include "gemm_body.hpp"

template <bool A_KM, bool B_KM, int EPI, int NW, int TSM, int TSN>
__global__ __launch_bounds__(NW * 64, 2) void gemm_tiles_kernel(GemmArgs g) {
    __shared__ __attribute__((aligned(16))) double smem[gemm_smem_doubles<TSM, TSN>()];
    gemm_tile_body<A_KM, B_KM, EPI, NW, TSM, TSN>(g, (int)blockIdx.x, (int)blockIdx.y, smem);
}

// Launches of a few tiles per CU with very different k-ranges (mid-size N): the launch lasts as long as its
// longest tile, which in the 4-wave shape shares its CU -- and the CU's MFMA rate -- with a second workgroup.
// Up to this many tiles the 8-wave shape is launched with 24 KB of unused dynamic LDS on top of its 74 KB of
// staging buffers, so that every tile has a CU to itself (K^-1 product at N = 4206: 0.71 -> 0.56 ms).
static int mid_tiles() {
    static const int v = 1100;   // (2048-tile levels of the inverse at N = 16384: 4-wave, two per CU, is 0.25 ms faster)
    return v;
}

// The launch shape (GemmShape) of the double engine for ntiles tiles per problem and `batch` problems in lock-step.
int gemm_shape_f64(bool a_km, bool b_km, int epi, int64_t ntiles, int64_t batch, int shape_div, int inplace) {
    if (ntiles <= 0 || batch <= 0 || !gemm_layout_ok(a_km, b_km, epi)) return -1;
    const int64_t total = ntiles * batch / (shape_div > 1 ? shape_div : 1);
    // up to 640 tiles: 64x64 quadrants, four co-resident workgroups per CU.  A launch of a few hundred tiles whose
    // k-ranges differ by an order of magnitude (triangular inverse, K^-1 product at N ~ 4000) lasts as long as its
    // longest tile; dealt longest-first over 4 x 256 slots, every CU gets a mix (N = 4206: inverse 0.92 -> 0.80 ms,
    // K^-1 product 0.57 -> 0.48; 1200 / 2400 measure the same; round 6: 128x64 halves with 8 waves instead of quadrants
    // 2.303 against 2.292 ms per Adam iteration at N = 4212, 1.144 against 1.084 at N = 2560, the same at 6000)
    const int tile64_max = 640;
    const bool small = total <= tile64_max;
    // few tiles: spread each over four CUs (64x64 quadrants)
    if (epi == EPI_STORE && small && !inplace) return GEMM_SHAPE_QUAD;
    // in-place panel solve: row halves (the workgroup owns the rows it overwrites), 8 waves
    if (epi == EPI_STORE && small) return GEMM_SHAPE_ROWHALF;
    // one tile per CU (see mid_tiles()).  Not for the column-sum epilogue: its cross-wave summation order
    // follows the wave layout, and batched and stand-alone predictions must stay bit-identical.
    if (epi == EPI_STORE && total > 256 && total <= mid_tiles()) return GEMM_SHAPE_8W_LDS;
    // (also every SYRK-shaped update of the Cholesky: measured 8 % faster factorisation at N = 16384,
    // the 512-thread workgroups interleave better with the concurrent panel chain)
    // at most one tile per CU: 8-wave workgroup so every SIMD still holds two MFMA waves
    if (total <= 256 || (!a_km && !b_km)) return GEMM_SHAPE_8W;
    return GEMM_SHAPE_4W;
}

template <bool A_KM, bool B_KM, int EPI>
static int launch_one(gpimhip_ctx* h, const GemmArgs& g) {
    if (g.ntiles <= 0) return GPIMHIP_OK;
    switch (gemm_shape_f64(A_KM, B_KM, EPI, g.ntiles, h->nbatch, g.shape_div, g.inplace)) {
    case GEMM_SHAPE_QUAD:
        hipLaunchKernelGGL((gemm_tiles_kernel<A_KM, B_KM, EPI_STORE, 4, 64, 64>), dim3(g.ntiles * 4, h->nbatch),
                           dim3(256), 0, h->stream, g);
        break;
    case GEMM_SHAPE_ROWHALF:
        hipLaunchKernelGGL((gemm_tiles_kernel<A_KM, B_KM, EPI_STORE, 8, 64, 128>), dim3(g.ntiles * 2, h->nbatch),
                           dim3(512), 0, h->stream, g);
        break;
    case GEMM_SHAPE_8W_LDS:
        hipLaunchKernelGGL((gemm_tiles_kernel<A_KM, B_KM, EPI, 8, 128, 128>), dim3(g.ntiles, h->nbatch), dim3(512),
                           24 * 1024, h->stream, g);
        break;
    case GEMM_SHAPE_8W:
        hipLaunchKernelGGL((gemm_tiles_kernel<A_KM, B_KM, EPI, 8, 128, 128>), dim3(g.ntiles, h->nbatch), dim3(512), 0,
                           h->stream, g);
        break;
    case GEMM_SHAPE_4W:
        hipLaunchKernelGGL((gemm_tiles_kernel<A_KM, B_KM, EPI, 4, 128, 128>), dim3(g.ntiles, h->nbatch), dim3(256), 0,
                           h->stream, g);
        break;
    default:
        gpim_set_error("launch_gemm: no launch shape for this batch");
        return GPIMHIP_E_BADARG;
    }
    HIP_TRY(hipGetLastError());
    return GPIMHIP_OK;
}

// Single-precision handles (gpimhip_set_precision) run the float instantiation of the same engine, written once
// for both element types in gemm_kernel.hpp and compiled in gemm32.hip.  The double kernels stay the hand-tuned
// source of this file: instantiating the generic template for double gives the same instruction counts but a
// schedule that is 0.5 - 0.9 % slower on the triangular inverse and the factorisation at N = 16384 (A/B on one box).
static int launch_gemm_f64(gpimhip_ctx* h, bool a_km, bool b_km, int epi, const GemmArgs& g) {
    if (epi == EPI_STORE) {
        if (!a_km && !b_km) return launch_one<false, false, EPI_STORE>(h, g);   // NT
        if (!a_km && b_km) return launch_one<false, true, EPI_STORE>(h, g);     // NN
        if (a_km && b_km) return launch_one<true, true, EPI_STORE>(h, g);       // TN
    } else {
        if (!a_km && b_km) return launch_one<false, true, EPI_COLSUMSQ>(h, g);
    }
    gpim_set_error("launch_gemm: unsupported operand layout combination");
    return GPIMHIP_E_BADARG;
}

int launch_gemm(gpimhip_ctx* h, bool a_km, bool b_km, int epi, const GemmArgs& g) {
    return h->fp32 ? launch_gemm_f32(h, a_km, b_km, epi, g) : launch_gemm_f64(h, a_km, b_km, epi, g);
}

// ------------------------------------------------------------------------------------------
// diagnostic entry points: the launch shape and the two index maps as host data (no GPU involved), and one tile launch of
// the engine by itself (tests/test_gemm_host.py, tests/test_gpu_gemm.py)
// ------------------------------------------------------------------------------------------
extern "C" int gpimhip_gemm_shape_host(int32_t fp32, int32_t a_km, int32_t b_km, int32_t epi, int64_t ntiles, int64_t batch,
                                       int32_t shape_div, int32_t inplace) {
    return fp32 ? gemm_shape_f32(a_km != 0, b_km != 0, epi, ntiles, batch, shape_div, inplace)
                : gemm_shape_f64(a_km != 0, b_km != 0, epi, ntiles, batch, shape_div, inplace);
}

extern "C" int gpimhip_gemm_tile_pos_host(int32_t fp32, int32_t n, int32_t chunk, int32_t quads, int32_t bx0, int32_t count,
                                          int32_t* p_out, int32_t* quad_out) {
    if (n < 1 || chunk < 0 || (quads != 1 && quads != 2 && quads != 4) || bx0 < 0 || count < 0 ||
        (int64_t)bx0 + count > (int64_t)n * quads || !p_out || !quad_out)
        return GPIMHIP_E_BADARG;
    for (int i = 0; i < count; ++i) {
        int quad = 0;
        p_out[i] = fp32       ? gemm_tile_pos_f32(n, chunk, quads, bx0 + i, quad)
                 : quads == 1 ? gemm_tile_pos<128, 128>(n, chunk, bx0 + i, quad)
                 : quads == 2 ? gemm_tile_pos<64, 128>(n, chunk, bx0 + i, quad)
                              : gemm_tile_pos<64, 64>(n, chunk, bx0 + i, quad);
        quad_out[i] = quad;
    }
    return GPIMHIP_OK;
}

extern "C" int gpimhip_gemm_rect_tile_host(int32_t rect_rows, int32_t rect_cols, int32_t p0, int32_t count, int32_t* ci_out,
                                           int32_t* cj_out) {
    if (rect_rows < 1 || rect_cols < 1 || p0 < 0 || count < 0 || (int64_t)p0 + count > (int64_t)rect_rows * rect_cols ||
        !ci_out || !cj_out)
        return GPIMHIP_E_BADARG;
    for (int i = 0; i < count; ++i) gemm_rect_tile(rect_rows, rect_cols, p0 + i, ci_out[i], cj_out[i]);
    return GPIMHIP_OK;
}

static int gemm_tiles_bad(const char* what) {
    gpim_set_error(std::string("gpimhip_gemm_tiles: ") + what);
    return GPIMHIP_E_BADARG;
}

extern "C" int gpimhip_gemm_tiles(gpimhip_handle h, const gpimhip_gemm_test_t* d) {
    if (!h || !d) return gemm_tiles_bad("null handle or descriptor");
    if (!d->A || !d->B) return gemm_tiles_bad("null operand");
    if (d->epi != EPI_STORE && d->epi != EPI_COLSUMSQ) return gemm_tiles_bad("unknown epilogue");
    if (d->epi == EPI_STORE ? !d->C : !d->colpart) return gemm_tiles_bad("null output (C for the store epilogue, colpart for the column sums)");
    if (d->ntiles <= 0 || d->batch <= 0 || d->batch > 65535) return gemm_tiles_bad("ntiles and batch must be positive (batch <= 65535)");
    if (d->lda <= 0 || d->ldb <= 0 || (d->epi == EPI_STORE ? d->ldc <= 0 : d->ld_colpart <= 0)) return gemm_tiles_bad("leading dimensions must be positive");
    if (!gemm_layout_ok(d->a_km != 0, d->b_km != 0, d->epi)) return gemm_tiles_bad("unsupported operand layout pair (store: NT, NN, TN; column sums: NN)");
    const bool kfix = d->kfix1 > d->kfix0;
    if (d->rect_cols < 0 || d->rect_rows < 0 || d->chunk < 0 || d->bshift < 0 || d->bshift > 30 || d->cj_max < 0 || d->rag < 0 ||
        d->shape_div < 0 || d->kfix0 < 0)
        return gemm_tiles_bad("negative switch");
    if (d->rect_cols > 0) {
        if (!kfix) return gemm_tiles_bad("rect_cols > 0 needs kfix0 < kfix1");
        if (d->rect_rows < 1 || (int64_t)d->rect_rows * d->rect_cols != d->ntiles)
            return gemm_tiles_bad("a rectangle launch has ntiles = rect_rows * rect_cols");
    } else if (!d->tiles) {
        return gemm_tiles_bad("null tile list");
    }
    if (d->cmap && !kfix) return gemm_tiles_bad("cmap needs kfix0 < kfix1");
    HIP_TRY(hipSetDevice(h->device));
    TileDesc* dt = nullptr;
    if (d->rect_cols == 0) {
        static_assert(sizeof(TileDesc) == 4 * sizeof(int32_t), "TileDesc is the (ci, cj, kb0, kb1) quadruple");
        for (int i = 0; i < d->ntiles; ++i) {
            const int32_t* t = d->tiles + 4 * (int64_t)i;
            if (t[0] < 0 || t[1] < 0 || t[2] < 0 || t[3] < t[2]) return gemm_tiles_bad("tile with a negative index or kb1 < kb0");
        }
        HIP_TRY(hipMalloc((void**)&dt, (size_t)d->ntiles * sizeof(TileDesc)));
        if (hipMemcpy(dt, d->tiles, (size_t)d->ntiles * sizeof(TileDesc), hipMemcpyHostToDevice) != hipSuccess) {
            (void)hipFree(dt);
            gpim_set_error("gpimhip_gemm_tiles: copy of the tile list failed");
            return GPIMHIP_E_HIP;
        }
    }
    GemmArgs g;
    memset(&g, 0, sizeof(g));
    g.A = (const double*)d->A; g.lda = d->lda; g.a_roff = d->a_roff; g.a_coff = d->a_coff;
    g.B = (const double*)d->B; g.ldb = d->ldb; g.b_roff = d->b_roff; g.b_coff = d->b_coff;
    g.C = (double*)d->C; g.ldc = d->ldc; g.c_roff = d->c_roff; g.c_coff = d->c_coff;
    g.alpha = d->alpha; g.beta = d->beta;
    g.tiles = dt; g.ntiles = d->ntiles;
    g.cj_max = d->cj_max; g.cmap = d->cmap; g.chunk = d->chunk; g.inplace = d->inplace; g.rag = d->rag; g.krev = d->krev;
    g.kfix0 = d->kfix0; g.kfix1 = d->kfix1; g.rect_rows = d->rect_rows; g.rect_cols = d->rect_cols;
    g.colpart = d->colpart; g.ld_colpart = d->ld_colpart;
    g.shape_div = d->shape_div;
    g.sA = d->sA; g.sB = d->sB; g.sC = d->sC; g.sColpart = d->sColpart;
    g.bshift = d->bshift;
    const int nbatch = h->nbatch;
    h->nbatch = d->batch;
    int rc = launch_gemm(h, d->a_km != 0, d->b_km != 0, d->epi, g);
    h->nbatch = nbatch;
    const hipError_t e = hipStreamSynchronize(h->stream);
    if (dt) (void)hipFree(dt);
    if (rc == GPIMHIP_OK && e != hipSuccess) {
        gpim_set_error(std::string("gpimhip_gemm_tiles: ") + hipGetErrorString(e));
        rc = GPIMHIP_E_HIP;
    }
    return rc;
}
