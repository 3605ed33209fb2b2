// kron.hpp -- the per-axis part of the Kronecker solver (kron.hip) that other translation units build on: one set of grid
// axes with K_i, its eigen-decomposition and the gradient matrices, the mode products, and the union-axis steps of the draws.
// Used by the dense-by-Kronecker blocks (pkron.hip, pkrongp.hip; DESIGN.md sections 22 and 23), whose complete axes are exactly
// such a set.
#pragma once
#include "common.hpp"

#define KMAXD GPIMHIP_MAX_DIM
// the sweep loop of kron_eigh_kernel ends by its own rule (largest rotation of a sweep < 1e-8) or after this many sweeps
#define EIGH_MAX_SWEEPS 40

struct KronDev {
    int d;
    int n[KMAXD];            // training grid
    int off[KMAXD];          // offset of axis i in the per-axis vectors (coords, lam, mdiag)
    int64_t moff[KMAXD];     // offset of axis i's n_i x n_i matrices
    int64_t N;
    const double* coords;    // [sum n_i]
    double *K, *E, *W, *Qt, *Mm, *Tt, *Vr;   // [sum n_i^2] each
    double *lam, *mdiag;     // [sum n_i]
    // eigen-problems: one per axis, or two (symmetric / skew-symmetric half) when the axis' coordinates
    // are centro-symmetric (any uniform grid): K_i then commutes with the exchange matrix and splits into
    // two problems of half the size -- an eighth of the Jacobi work each, half the round-robin steps
    int nprob;
    int pax[2 * KMAXD], ppart[2 * KMAXD], pn[2 * KMAXD];   // axis, part (0 whole, 1 symmetric, 2 skew), order
    int64_t poff[2 * KMAXD];                                // offset inside the axis' n_i^2 region (W, Vr, Tt)
    int plam[2 * KMAXD];                                    // offset of its eigenvalues / Qt rows inside the axis
    double* stat;            // [2 * nprob] per eigen-problem: sweeps run, largest rotation of the last one (gpimhip_kron_eigh)
};

// One set of grid axes with everything that belongs to an axis alone: coordinates, K_i, the eigen-problem plan and the
// eigen-decomposition (KronDev).  The training grid has one; gpimhip_sample_kron keeps a second one for the union of the
// training and the test axes, without the gradient matrices (E, Mm, mdiag) and without any N-sized vector.
struct KronAxes {
    int d = 0;
    int n[KMAXD] = {0, 0, 0, 0};
    int64_t sum_n = 0, sum_n2 = 0;
    bool grad = false;
    DevBuf<double> arena;
    KronDev dev;
};

// the per-axis state for axes of the orders n[] (grow / re-carve; synchronises when it re-allocates); grad: with E, Mm, mdiag
int kron_axes_ensure(gpimhip_ctx* h, KronAxes& a, int d, const int32_t* n, bool grad);
void kron_axes_free(gpimhip_ctx* h, KronAxes& a);
// the eigen-problem plan from the coordinates in a.dev.coords (one small copy to the host and a synchronisation)
int kron_plan_problems(gpimhip_ctx* h, KronAxes& ax);
// Vr <- I: the next kron_eig_axes starts its rotations cold
int kron_cold_start(gpimhip_ctx* h, const KronDev& dv);
// an axis set ready for its first kron_eig_axes: kron_axes_ensure, the coordinates (device, sum n_i) copied in,
// kron_plan_problems, kron_cold_start
int kron_axes_load(gpimhip_ctx* h, KronAxes& a, int d, const int32_t* n, const double* coords_dev, bool grad);
// K_i (and E_i) at the lengthscales th->ls[i] (th null: h->theta) and the eigen-decomposition (Qt, lam), warm-started from Vr
int kron_eig_axes(gpimhip_ctx* h, const KronAxes& ax, const ThetaDev* th = nullptr);
// Mm_i = Q_i^T E_i Q_i and its diagonal mdiag_i, for every axis of a set with the gradient matrices
int kron_grad_matrices(gpimhip_ctx* h, const KronAxes& ax);
// Ks[t, a] = exp(-((tcoords[toff + t] - c_ax[a]) / th->ls[ax])^2 / 2): the cross-covariance of axis ax, mi x n_ax
int kron_cross(gpimhip_ctx* h, const KronDev& dv, const ThetaDev* th, const double* tcoords, int toff, int mi, int ax, double* Ks);
// out[r, j] = Q_ax[idx[r], j] sqrt(max(lam_ax[j], 0)): `rows` rows of the prior root of axis ax (idx: device, inside the axis)
int kron_root_rows(gpimhip_ctx* h, const KronDev& dv, int ax, const int32_t* idx, int rows, double* out);
// ---- the union of the training and the test axes of a draw (gpimhip_sample_kron, gpimhip_sample_pkron)
// shared: the union axes ARE the training axes (the test grid is the training grid or a crop of it) and the training
// decomposition serves as the union one.  Sums over the axes: n_i, m_i, u_i, n_i u_i, m_i u_i; U = prod u_i
struct KronUnion { bool shared; int64_t sum_n, sum_m, sum_u, sum_nu, sum_mu, U; };
// The union axes and the index maps (host arrays) of entry point `entry` (the prefix of its messages): every axis of either
// grid has a coordinate, a union axis is no longer than the two axes together (nor than the eigen-solver's 4096) and no
// shorter than the training axis, every index lies inside its union axis.  GPIMHIP_E_BADARG with the message set, else *out
int kron_union_check(const char* entry, int d, const int32_t* n, const int32_t* n_test, const int32_t* n_union,
                     const int32_t* idx_train, const int32_t* idx_test, KronUnion* out);
// per axis the rows of the root of union axis i (decomposition du) at the training coordinates (ic, device: sum n_i indices)
// into RX (sum n_i u_i) and at the test coordinates (it) into RT (sum m_i u_i); rx[i] / rt[i]: where axis i's rows start
int kron_union_roots(gpimhip_ctx* h, const KronDev& du, int d, const int32_t* n, const int32_t* n_test, const int32_t* ic,
                     const int32_t* it, double* RX, double* RT, const double** rx, const double** rt);
// out[p, a, q] = sum_b Mx(a, b) in[p, b, q]; Mx(a, b) = M[a * ldm + b] (trans == 0) or M[b * ldm + a]; sq != 0 squares Mx
int modeprod(gpimhip_ctx* h, const double* in, double* out, const double* M, int ma, int nbk, int ldm, int trans, int sq,
             int64_t pre, int64_t post);
// mats[i] (ma[i] x nb[i]) along mode i of `src` (shape nb[], `batch` contiguous tensors), ping-pong between bufa / bufb
int tensor_apply(gpimhip_ctx* h, int d, const int* nbv, const int* mav, const double* const* mats, const int* ldm, int trans,
                 int sq, const double* src, double* bufa, double* bufb, double** result, int64_t batch = 1);
