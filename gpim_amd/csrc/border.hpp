// border.hpp -- launches of the border form of the reflection blocks (border.hip; driven by api.hip: border_*, by the model
// families' drivers in smgp.hip and vgpgp.hip, and by draws.hip: sample_border_impl).
#pragma once
#include "common.hpp"

// What gpimhip_set_border leaves on the handle, and the border's own workspace (sized for the workspace's np).
struct BorderWs {
    int M = 0;                      // missing points (0: border off)
    int64_t mp = 0;                 // M padded to 128
    const int32_t* q = nullptr;     // (device, M) representative of missing point j in the fundamental domain
    const double* coef = nullptr;   // (device, B x M) coefficient c_b(j) of missing point j in block b
    gpimhip_ctx* sub = nullptr;     // handle of S: its own mp x mp workspace, factorisation plans and status word
    int64_t np = 0;                 // the block order the buffers below are sized for
    int B = 0;                      // the batch: 2^r blocks, times T tasks for the multi-output GP (task-major)
    int T = 1;                      // borders handled in lock-step: one S_t per task of the multi-output GP (vgp.hip), else 1;
                                    // sub's batch.  Per-task buffers below are stacked, task t at t times their size
    DevBuf<double> C;               // B x np x mp   C_b[:, j] = c_b(j) B_b^-1[:, q(j)]
    DevBuf<double> Y;               // B x np x mp   Y_b = C_b L_S^-T
    DevBuf<double> tv;              // T x 2 x mp: t = (A^-1 y~)_m, v = L_S^-1 t
    DevBuf<double> scal;            // T x 2: |v|^2, sum log (L_S)_ii
    DevBuf<double> uo;              // 2^r x N (multi-output GP only): U 1_o, the observed points' indicator in the adapted basis
    DevBuf<TileDesc> tiles_y;       // Y = C L_S^-T: (np / 128) x (mp / 128) tiles, k-range [0, cj]
    int n_y = 0;
    DevBuf<TileDesc> tiles_upd;     // B_b^-1 -= Y_b Y_b^T: the lower tiles of the block
    int n_upd = 0;
    DevBuf<double> R;               // T x mp x r_cols: R = sum_b Y_b^T K*_b for one test chunk
    DevBuf<double> rsq;             // T x r_cols: column sums of squares of R
    int64_t r_cols = 0;
};
// api.hip: the handle's border (null: none was ever set), and whether one is in force
BorderWs* bws(const gpimhip_ctx* h);
bool border_on(const gpimhip_ctx* h);
// api.hip: the border's buffers for the workspace's np and batch (T: the borders in lock-step) and for `cols` test columns
// (both outside any capture), and the border stage of one evaluation after the blocks' inverses (nq: the points of the
// fundamental domain; update_inverse: training, B_b^-1 -= Y_b Y_b^T as well)
int border_ensure(gpimhip_ctx* h, int T = 1);
int border_ensure_r(gpimhip_ctx* h, int64_t cols);
int border_iter(gpimhip_ctx* h, int64_t nq, bool update_inverse);

int launch_border_gather_s(gpimhip_ctx* h, const BorderWs* w, const double* Binv, int64_t ld, double* S, int64_t lds);
int launch_border_tidy(gpimhip_ctx* h, const BorderWs* w, double* Linv, int64_t lds);
int launch_border_gather_c(gpimhip_ctx* h, const BorderWs* w, const double* Binv, int64_t ld, int64_t nq);
int launch_border_vectors(gpimhip_ctx* h, const BorderWs* w, const double* Linv, int64_t lds, const double* logdet_part,
                          int nbs, double* alpha);
int launch_border_colsumsq(gpimhip_ctx* h, const BorderWs* w, int64_t cnt);
int launch_border_ones(gpimhip_ctx* h, const BorderWs* w, int64_t N, int B, double* uo);
