// grad.hip -- from K^-1 and alpha to the loss, its gradient and the Adam step: the launches of a training iteration behind
// the O(N^3) stages.
//   grad_reduce_kernel       fused  sum_ij (K^-1 - alpha alpha^T)_ij dK_ij/dtheta over the lower tiles   
//                            -- a full matrix, or the tiles a rank of a distributed job holds (launch_grad_reduce_tiles); its LOO
//                            form contracts G2 - (r alpha^T + alpha r^T) for the leave-one-out objective (loograd.hip)
//   grad_reduce_refl_kernel  the same for one reflection block K_s
//   finalize_block           loss, d loss/du, Adam step, history row, next theta (rows a7-a10): finalize_kernel, or the
//                            last workgroup of grad_reduce_kernel (FinFused)
//   finalize_coupled_kernel  one step for the B reflection blocks; coupled_sums_kernel: their sums, for a job that deals them out
//   sum7 / dist_finalize*    the distributed trainer's reduction and step
// All reductions use fixed-shape trees so results are bit-reproducible run to run.
#include "kfun.hpp"
#include <type_traits>
#include "theta.hpp"
#include "refl.hpp"
#include "tile128.hpp"

// ------------------------------------------------------------------------------------------
// finalize: sums the partials in a fixed tree, forms loss and d loss/du, then (fit mode) applies one torch.optim.Adam
// step to u and records the constrained values.  Run by ONE workgroup of 256 threads: finalize_kernel, or the LAST
// workgroup of grad_reduce_kernel to finish (FinFused) -- the Adam step is then not a launch of its own, and the
// theta of the stepped parameters is written for the next iteration's kmat_kernel (no theta launch either).
// ------------------------------------------------------------------------------------------
// block_sum_256's tree for NQ quantities at once with three barriers: red[t] += red[t + 128], += red[t + 64] in LDS order, then
// lane t += lane t + s for s = 32 ... 1 inside wave 0 -- what block_sum_256's steps compute for t < s, bit for bit.
// arr: NQ x 256 doubles of LDS.  Results in out[0 .. NQ) (LDS), valid after the call for every thread.
template <int NQ>
__device__ __forceinline__ void block_sum_256_multi(const double* v, double* arr, double* out) {
    const int tid = threadIdx.x;
    __syncthreads();                                   // (arr may alias what the caller still read)
#pragma unroll
    for (int q = 0; q < NQ; ++q) arr[q * 256 + tid] = v[q];
    __syncthreads();
    if (tid < 64) {
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            const double* a = arr + q * 256;
            double x = (a[tid] + a[tid + 128]) + (a[tid + 64] + a[tid + 192]);
            x += __shfl_down(x, 32);
            x += __shfl_down(x, 16);
            x += __shfl_down(x, 8);
            x += __shfl_down(x, 4);
            x += __shfl_down(x, 2);
            x += __shfl_down(x, 1);
            if (tid == 0) out[q] = x;
        }
    }
    __syncthreads();
}

// everything the finalize step of one problem needs (pointers already offset to the problem by the caller)
struct FinProblem {
    const double* grad_part; const double* z; const double* zb; const double* logdet_part;
    ThetaDev* th; double* u; double* adam_m; double* adam_v;
    FinalizeOut out;
};
// COHERENT: the partial sums were written by other workgroups of the SAME launch (agent-scope loads: sc1, past this CU's L1)
template <bool COHERENT>
__device__ __forceinline__ double fin_load(const double* p) {
    return COHERENT ? __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : *p;
}
// arr: 5 x 256 doubles of LDS, S: 9 doubles of LDS.  theta_next != nullptr: the theta of the stepped parameters goes there.
template <bool COHERENT>
__device__ __forceinline__ void finalize_block(const gpimhip_model_t& m, int64_t N, int64_t np, int nb, int ntile, FinProblem f,
                                               int do_adam, AdamStep st, int32_t* info, ThetaDev* theta_next, double* arr, double* S) {
    const int tid = threadIdx.x;
    double v[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    // (four tiles' loads in flight, added in the order q = tid, tid + 256, ...: device-scope loads are round trips to
    // memory, and one tile per trip made this loop 130 us at N = 16384)
    for (int q0 = tid; q0 < ntile; q0 += 4 * 256) {
        double t[4][7];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int q = q0 + 256 * i;
            const double* g = f.grad_part + (int64_t)(q < ntile ? q : q0) * 8;
#pragma unroll
            for (int k = 0; k < 7; ++k) t[i][k] = fin_load<COHERENT>(g + k);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (q0 + 256 * i < ntile) {
#pragma unroll
                for (int k = 0; k < 7; ++k) v[k] += t[i][k];
            }
    }
    for (int64_t i = tid; i < np; i += 256) v[7] = fma(f.z[i], f.zb[i], v[7]);     // |L^-1 y|^2, or y^T alpha (refined, fp32 matrices)
    for (int k = tid; k < nb; k += 256) v[8] += f.logdet_part[k];
    block_sum_256_multi<5>(v, arr, S);
    block_sum_256_multi<4>(v + 5, arr, S + 5);
    if (tid != 0) return;
    const int P = 2 + m.n_ls + (m.kernel == GPIMHIP_KERNEL_RQ ? 1 : 0);
    if (!finalize_iter_begin(f.out.fi, info, P, st, f.out.loss_out, f.out.hist_row)) return;
    // working storage in LDS (arr is free again): gradient, the current theta (theta_next may be f.th itself), the next one
    double* g = arr;
    ThetaDev* told = reinterpret_cast<ThetaDev*>(arr + 16);
    ThetaDev* tn = reinterpret_cast<ThetaDev*>(arr + 48);
    *told = *f.th;
    finalize_step_ws(m, N, S, S[7], S[8], *told, f.u, f.adam_m, f.adam_v, do_adam, st, f.out.loss_out, f.out.grad_out,
                     f.out.hist_row, prior_constant(m), theta_next, g, *tn);
}
__device__ __forceinline__ FinProblem fin_problem(const gpimhip_model_t& m, int64_t b, int64_t np, int nb, int ntile,
                                                  const double* grad_part, const double* z, const double* zb,
                                                  const double* logdet_part, ThetaDev* th, double* u, double* adam_m,
                                                  double* adam_v, const FinalizeOut& out) {
    const int P = 2 + m.n_ls + (m.kernel == GPIMHIP_KERNEL_RQ ? 1 : 0);
    FinProblem f{grad_part + b * ntile * 8, z + b * np, zb + b * np, logdet_part + b * nb, th + b, u + b * P,
                 adam_m + b * MAXP, adam_v + b * MAXP, out};
    if (out.fi.iter) {
        f.out.fi.iter += b;
        if (out.fi.hist_base) f.out.fi.hist_base += b * out.fi.T * P;
        if (out.fi.loss_base) f.out.fi.loss_base += b * out.fi.T;
    }
    return f;
}

__global__ __launch_bounds__(256) void finalize_kernel(gpimhip_model_t m, int64_t N, int64_t np, int nb,
                                                       int ntile, const double* __restrict__ grad_part,
                                                       const double* __restrict__ z, const double* __restrict__ zb,
                                                       const double* __restrict__ logdet_part,
                                                       ThetaDev* __restrict__ th, double* __restrict__ u,
                                                       double* __restrict__ adam_m, double* __restrict__ adam_v,
                                                       int do_adam, AdamStep st, FinalizeOut out,
                                                       int32_t* __restrict__ info, int carry_theta) {
    __shared__ double arr[5 * 256];
    __shared__ double S[9];
    const FinProblem f = fin_problem(m, blockIdx.y, np, nb, ntile, grad_part, z, zb, logdet_part, th, u, adam_m, adam_v, out);
    finalize_block<false>(m, N, np, nb, ntile, f, do_adam, st, info, carry_theta ? th + blockIdx.y : nullptr, arr, S);
}

// the finalize step as the tail of grad_reduce_kernel
struct FinFused {
    int enabled = 0;
    int do_adam = 0;
    int carry_theta = 0;        // write the theta of the stepped parameters over the current one
    int nb = 0;
    uint32_t* counter = nullptr;    // per problem, 0 between launches
    gpimhip_model_t m = {};
    int64_t N = 0;
    const double* z = nullptr; const double* zb = nullptr; const double* logdet_part = nullptr;
    double* u = nullptr; double* adam_m = nullptr; double* adam_v = nullptr;
    AdamStep st = {};
    FinalizeOut out{nullptr, nullptr, nullptr};
    int32_t* info = nullptr;
};

// ------------------------------------------------------------------------------------------
// gradient reduction over the lower tiles of K^-1:
//   w_ij = (2 - delta_ij) * (Kinv_ij - alpha_i alpha_j)
//   S[0]      += w * k/s2                       -> d/d s2
//   S[1+k]    += w * s2*h * (a_ik - a_jk)^2     -> d/d l_k  (times 1/l_k later)
//   S[5]      += delta_ij * (Kinv_ii - alpha_i^2) -> d/d noise
//   S[6]      += w * s2 * dk/dalpha / s2        -> d/d alpha (RQ)
// ------------------------------------------------------------------------------------------
// alpha_part != nullptr: alpha is given as the row-chunk partial sums of gemv_t_tri_kernel (nR chunks of rc rows) and
// every workgroup adds up the 256 entries it needs itself (no sum launch).  fin.enabled: the last workgroup of a problem to
// finish runs the finalize step (FinFused).
// LOO (the leave-one-out objective, loograd.hip): Kinv holds G2 = S^-1 diag(omega) S^-1 and rvec = S^-1 (alpha / d); the entry's
// weight is G2_ij - (r_i alpha_j + alpha_i r_j) where the marginal likelihood has Kinv_ij - alpha_i alpha_j.  Its finalize
// step is a launch of its own (fin is ignored).
template <int KIND, typename R, bool LOO = false>
__global__ __launch_bounds__(256) void grad_reduce_kernel(const R* __restrict__ Kinv, int64_t ld,
                                                          const double* __restrict__ X, int64_t N, int d,
                                                          const double* __restrict__ alpha,
                                                          ThetaDev* __restrict__ th,
                                                          double* __restrict__ part, int64_t x_bs, int64_t np,
                                                          const TileDesc* __restrict__ tiles,
                                                          const double* __restrict__ alpha_part, int nR, int rc, FinFused fin,
                                                          const double* __restrict__ rvec) {
    // one buffer, carved: the staging of the tile phase, then (last workgroup only) the reduction scratch of the finalize step
    // (LOO: the second vector's rows and columns behind it)
    __shared__ double sh[2 * 128 * 5 + 2 * 128 + 4 * 8 + 16 + (LOO ? 2 * 128 : 0)];
    double (*xa)[5] = reinterpret_cast<double (*)[5]>(sh);
    double (*xz)[5] = reinterpret_cast<double (*)[5]>(sh + 128 * 5);
    double* al_r = sh + 2 * 128 * 5;
    double* al_c = al_r + 128;
    double (*red)[8] = reinterpret_cast<double (*)[8]>(al_c + 128);
    double* rv_r = sh + 2 * 128 * 5 + 2 * 128 + 4 * 8 + 16;
    double* rv_c = rv_r + 128;
    const int tid = threadIdx.x;
    double* part_all = part;
    Kinv += blockIdx.y * np * ld;
    X += blockIdx.y * x_bs;
    if (alpha) alpha += blockIdx.y * np;
    if (alpha_part) alpha_part += (int64_t)blockIdx.y * nR * np;
    part += ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * 8;
    // tiles == nullptr: workgroup q is lower tile q of a full np x np matrix.  Otherwise (distributed layouts:
    // a rank holds some block columns side by side) tile (ci, cj) of the matrix lives at block column kb0 of Kinv.
    int ci, cj;
    int64_t ccol;
    if (tiles) {
        const TileDesc td = tiles[blockIdx.x];
        ci = td.ci; cj = td.cj; ccol = (int64_t)td.kb0 * 128;
    } else {
        lower_tile_from_linear(blockIdx.x, ci, cj);
        ccol = (int64_t)cj * 128;
    }
    const ThetaDev t = th[blockIdx.y];
    {
        const TileSlot s = tile_stage<5>(X, N, X, N, d, t, ci, cj, xa, xz);
        double av = 0.0;
        if (s.valid) av = alpha_part ? gemv_tri_alpha(alpha_part, nR, rc, np, s.g) : alpha[s.g];
        tile_put(s, al_r, al_c, av);
        if (LOO) tile_put(s, rv_r, rv_c, s.valid ? rvec[blockIdx.y * np + s.g] : 0.0);
    }
    __syncthreads();
    double S[7] = {0, 0, 0, 0, 0, 0, 0};
    const int ty = tid >> 4, tx = tid & 15;
    // strictly lower tiles inside the matrix: every entry counts twice, none is skipped (no per-entry 64-bit compares)
    const bool interior = ci > cj && (int64_t)ci * 128 + 128 <= N;
    auto body = [&](auto INTERIOR) {
    for (int rr = 0; rr < 8; ++rr) {
        const int r = ty + 16 * rr;
        const int64_t gi = (int64_t)ci * 128 + r;
        const double a0 = xa[r][0], a1 = xa[r][1], a2 = xa[r][2], a3 = xa[r][3], an = xa[r][4];
        const double ali = al_r[r];
        const double rvi = LOO ? rv_r[r] : 0.0;
#pragma unroll
        for (int cc = 0; cc < 4; ++cc) {
            const typename Vec2<R>::T kv = *reinterpret_cast<const typename Vec2<R>::T*>(Kinv + gi * ld + ccol + tx * 2 + 32 * cc);
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                const int c = tx * 2 + 32 * cc + e;
                const int64_t gj = (int64_t)cj * 128 + c;
                if (!decltype(INTERIOR)::value && (gi >= N || gj > gi)) continue;
                const double g = LOO ? (double)kv[e] - fma(rvi, al_c[c], ali * rv_c[c]) : (double)kv[e] - ali * al_c[c];
                const double w = (!decltype(INTERIOR)::value && gi == gj) ? g : 2.0 * g;
                double dot = a0 * xz[c][0];
                dot = fma(a1, xz[c][1], dot);
                dot = fma(a2, xz[c][2], dot);
                dot = fma(a3, xz[c][3], dot);
                double r2 = clamp0_nan((an - 2.0 * dot) + xz[c][4]);
                const KVal kvv = kfun_grad<KIND>(r2, t.alpha);
                S[0] = fma(w, kvv.e, S[0]);
                const double wh = w * kvv.h;
                const double d0 = a0 - xz[c][0], d1 = a1 - xz[c][1], d2_ = a2 - xz[c][2], d3 = a3 - xz[c][3];
                S[1] = fma(wh, d0 * d0, S[1]);
                S[2] = fma(wh, d1 * d1, S[2]);
                S[3] = fma(wh, d2_ * d2_, S[3]);
                S[4] = fma(wh, d3 * d3, S[4]);
                if (!decltype(INTERIOR)::value && gi == gj) S[5] += g;
                if (KIND == GPIMHIP_KERNEL_RQ) S[6] = fma(w, kvv.ga, S[6]);
            }
        }
    }
    };
    if (interior) body(std::true_type{});
    else body(std::false_type{});
    if (LOO || !fin.enabled) {
        tile_sums_store<false>(S, red, part);
        return;
    }
    // ---- fused finalize: the last workgroup of this problem to finish runs the step (loss, gradient, Adam, next theta).
    // Hand-off of the partial sums between workgroups of one launch:
    //   producer  wave 0 stored this tile's sums write-through (sc1) and waited for them (s_waitcnt vmcnt(0): tile_sums_store);
    //             the barrier puts that wait in front of thread 0's add on the problem's counter;
    //   consumer  the workgroup whose add finds every other one counted invalidates its CU's L1 (agent-scope acquire:
    //             buffer_inv sc1, and the wait for it) before the barrier lets its waves read; the sums themselves are read
    //             with agent-scope loads (finalize_block<true>).
    tile_sums_store<true>(S, red, part);
    int* flag = reinterpret_cast<int*>(sh + 2 * 128 * 5 + 2 * 128 + 4 * 8);
    __syncthreads();
    if (tid == 0) {
        // (one counter per problem; a two-level count -- groups of 32 workgroups -- measured the same at 8256 workgroups: the
        // adds are spread over the launch)
        const bool last = atomicAdd(fin.counter + blockIdx.y, 1u) == gridDim.x - 1;
        *flag = last;
        if (last) {
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            fin.counter[blockIdx.y] = 0;               // ready for the next launch (every other workgroup has passed)
            // not part of the hand-off (the sums are read past the L1 anyway): the invalidate completes asynchronously and the
            // reset is a plain store; this holds the barrier until both have left the wave
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
    }
    __syncthreads();
    if (!*flag) return;
    const int ntile = (int)gridDim.x;
    const FinProblem f = fin_problem(fin.m, blockIdx.y, np, fin.nb, ntile, part_all, fin.z, fin.zb, fin.logdet_part, th, fin.u,
                                     fin.adam_m, fin.adam_v, fin.out);
    // (sh: 1584 doubles; the reduction scratch takes the first 1280, the nine sums sit behind the flag)
    finalize_block<true>(fin.m, fin.N, np, fin.nb, ntile, f, fin.do_adam, fin.st, fin.info,
                         fin.carry_theta ? th + blockIdx.y : nullptr, sh, sh + 2 * 128 * 5 + 2 * 128 + 4 * 8 + 2);
}

// The one launch of grad_reduce_kernel: ntile tiles of each of nbatch problems, sums to part.  tiles: nullptr (workgroup q is
// lower tile q of the full matrix) or the list of a distributed layout.  alpha_part: nullptr (alpha is a vector) or the
// row-chunk partial sums of launch_gemv_t_tri.  fin: nullptr, or the finalize step to run in each problem's last workgroup.
static int launch_grad_reduce_impl(gpimhip_ctx* h, const gpimhip_model_t* m, const double* Kinv, int64_t ld, const double* X,
                                   int64_t x_bs, int64_t N, int64_t np, const double* alpha, const double* alpha_part,
                                   const TileDesc* tiles, int ntile, int nbatch, double* part, const FinFused* fin,
                                   const double* rvec = nullptr) {
    const dim3 grid(ntile, nbatch), block(256);
    const FinFused ff = fin ? *fin : FinFused();
    const int nR = alpha_part ? gemv_tri_chunks(np) : 0, rc = alpha_part ? gemv_tri_rc(np) : 0;
    return with_kind(m->kernel, [&](auto K) {
        constexpr int KIND = decltype(K)::value;
        auto launch = [&](auto* kinv) {
            typedef std::remove_const_t<std::remove_pointer_t<decltype(kinv)>> R;
            hipLaunchKernelGGL((grad_reduce_kernel<KIND, R>), grid, block, 0, h->stream, kinv, ld, X, N, m->dim, alpha, h->theta,
                               part, x_bs, np, tiles, alpha_part, nR, rc, ff, rvec);
        };
        if (rvec)
            hipLaunchKernelGGL((grad_reduce_kernel<KIND, double, true>), grid, block, 0, h->stream, Kinv, ld, X, N, m->dim, alpha,
                               h->theta, part, x_bs, np, tiles, alpha_part, nR, rc, ff, rvec);
        else if (h->fp32) launch(reinterpret_cast<const float*>(Kinv));
        else launch(Kinv);
        HIP_TRY(hipGetLastError());
        return GPIMHIP_OK;
    });
}
int launch_grad_reduce(gpimhip_ctx* h, const gpimhip_model_t* m, const double* Kinv, int64_t ld,
                       const double* X, int64_t N, int nb, const double* alpha, int64_t x_bs) {
    return launch_grad_reduce_impl(h, m, Kinv, ld, X, x_bs, N, (int64_t)nb * NB, alpha, nullptr, nullptr, nb * (nb + 1) / 2,
                                   h->nbatch, h->grad_part, nullptr);
}
// the leave-one-out form (loograd.hip): Kinv holds the lower tiles of G2, rvec = S^-1 (alpha / d); one double-precision problem
int launch_grad_reduce_loo(gpimhip_ctx* h, const gpimhip_model_t* m, const double* Kinv, int64_t ld, const double* X, int64_t N,
                           int nb, const double* alpha, const double* rvec) {
    FP64_ONLY(h);
    return launch_grad_reduce_impl(h, m, Kinv, ld, X, 0, N, (int64_t)nb * NB, alpha, nullptr, nullptr, nb * (nb + 1) / 2, 1,
                                   h->grad_part, nullptr, rvec);
}
// the tiles of K^-1 a rank of a distributed job holds (distgp.hip: gpimhip_dist_grad_sums).  The distributed layouts are
// double: a single-precision handle would send the shared launch to the float kernel.
int launch_grad_reduce_tiles(gpimhip_ctx* h, const gpimhip_model_t* m, const double* Kinv, int64_t ld, const double* X,
                             int64_t N, int64_t np, const double* alpha, const TileDesc* tiles, int ntile, double* part) {
    FP64_ONLY(h);
    return launch_grad_reduce_impl(h, m, Kinv, ld, X, 0, N, np, alpha, nullptr, tiles, ntile, 1, part, nullptr);
}
// The gradient contraction AND the finalize step (loss, gradient, Adam step, history row, next theta) in one launch: what
// launch_finalize does, run by the last workgroup of every problem.
int launch_grad_reduce_fin(gpimhip_ctx* h, const gpimhip_model_t* m, const double* X, int64_t x_bs, int64_t N,
                           bool alpha_deferred, double* u, int do_adam, AdamStep st, const FinalizeOut& out, int carry_theta) {
    const int nb = (int)(h->np / NB);
    FinFused ff;
    ff.enabled = 1;
    ff.do_adam = do_adam;
    ff.carry_theta = carry_theta;
    ff.nb = nb;
    ff.counter = h->fin_counter;
    ff.m = *m;
    ff.N = N;
    ff.z = h->fp32 ? h->ypad : h->z;
    ff.zb = h->fp32 ? h->alpha : h->z;
    ff.logdet_part = h->logdet_part;
    ff.u = u; ff.adam_m = h->adam_m; ff.adam_v = h->adam_v;
    ff.st = st;
    ff.out = out;
    ff.info = h->info;
    return launch_grad_reduce_impl(h, m, h->B, h->ld, X, x_bs, N, h->np, h->alpha, alpha_deferred ? h->gemv_part.p : nullptr,
                                   nullptr, nb * (nb + 1) / 2, h->nbatch, h->grad_part, &ff);
}

// z, zb: the two vectors whose dot product is the loss's quadratic term
int launch_finalize_vec(gpimhip_ctx* h, const gpimhip_model_t* m, int64_t N, int64_t np, double* u, int do_adam, AdamStep st,
                        const FinalizeOut& out, int carry_theta, const double* z, const double* zb) {
    const int nb = (int)(np / NB);
    hipLaunchKernelGGL(finalize_kernel, dim3(1, h->nbatch), dim3(256), 0, h->stream, *m, N, np, nb, nb * (nb + 1) / 2,
                       h->grad_part, z, zb, h->logdet_part, h->theta, u, h->adam_m, h->adam_v, do_adam, st, out, h->info,
                       carry_theta);
    HIP_TRY(hipGetLastError());
    return GPIMHIP_OK;
}
int launch_finalize(gpimhip_ctx* h, const gpimhip_model_t* m, int64_t N, int64_t np, double* u, int do_adam,
                    AdamStep st, const FinalizeOut& out, int carry_theta) {
    return launch_finalize_vec(h, m, N, np, u, do_adam, st, out, carry_theta, h->fp32 ? h->ypad : h->z, h->fp32 ? h->alpha : h->z);
}

// ------------------------------------------------------------------------------------------
// distributed training (distgp.hip: gpimhip_dist_grad_sums / gpimhip_dist_finalize): the gradient contraction over the
// tiles of K^-1 a rank holds (launch_grad_reduce_tiles), reduced to the seven sums S[] in a fixed order; after the all-reduce
// of S across the ranks the same finalize_step as the single-GPU path turns them into loss, gradient and Adam step.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void sum7_kernel(const double* __restrict__ part, int ntile, double* __restrict__ S) {
    __shared__ double red[256];
    for (int k = 0; k < 7; ++k) {
        double v = 0.0;
        for (int q = threadIdx.x; q < ntile; q += 256) v += part[(int64_t)q * 8 + k];
        v = block_sum_256(v, red);
        if (threadIdx.x == 0) S[k] = v;
    }
    if (threadIdx.x == 0) S[7] = 0.0;
}
int launch_sum7(gpimhip_ctx* h, const double* part, int ntile, double* S) {
    hipLaunchKernelGGL(sum7_kernel, dim3(1), dim3(256), 0, h->stream, part, ntile, S);
    HIP_TRY(hipGetLastError());
    return GPIMHIP_OK;
}

__global__ void dist_finalize_kernel(gpimhip_model_t m, int64_t N, const double* __restrict__ S, double q2, double lg,
                                     const ThetaDev* __restrict__ th, double* __restrict__ u, double* __restrict__ adam_m,
                                     double* __restrict__ adam_v, int do_adam, AdamStep st, double* __restrict__ loss_out,
                                     double* __restrict__ grad_out, double* __restrict__ hist_row) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    double Sl[8];
    for (int k = 0; k < 8; ++k) Sl[k] = S[k];
    finalize_step(m, N, Sl, q2, lg, *th, u, adam_m, adam_v, do_adam, st, loss_out, grad_out, hist_row, prior_constant(m));
}
// ... with the scalars where the distributed driver leaves them -- device memory: red[0..7] = the all-reduced gradient
// sums, red[8] = sum log L_ii, red[9] = how many ranks met a non-positive pivot (then nothing is touched but the loss,
// which becomes NaN: the driver raises after its one read-back of the iteration); quad[0] = y^T alpha
__global__ void dist_finalize_dev_kernel(gpimhip_model_t m, int64_t N, const double* __restrict__ red,
                                         const double* __restrict__ quad, const ThetaDev* __restrict__ th,
                                         double* __restrict__ u, double* __restrict__ adam_m, double* __restrict__ adam_v,
                                         int do_adam, AdamStep st, double* __restrict__ loss_out,
                                         double* __restrict__ grad_out, double* __restrict__ hist_row) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    if (red[9] != 0.0) {
        if (loss_out) *loss_out = __builtin_nan("");
        return;
    }
    double Sl[8];
    for (int k = 0; k < 8; ++k) Sl[k] = red[k];
    finalize_step(m, N, Sl, quad[0], red[8], *th, u, adam_m, adam_v, do_adam, st, loss_out, grad_out, hist_row, prior_constant(m));
}
int launch_dist_finalize_dev(gpimhip_ctx* h, const gpimhip_model_t* m, int64_t N, const double* red, const double* quad,
                             double* u, int do_adam, AdamStep st, double* loss_out, double* grad_out, double* hist_row) {
    hipLaunchKernelGGL(dist_finalize_dev_kernel, dim3(1), dim3(64), 0, h->stream, *m, N, red, quad, h->theta, u, h->adam_m,
                       h->adam_v, do_adam, st, loss_out, grad_out, hist_row);
    HIP_TRY(hipGetLastError());
    return GPIMHIP_OK;
}
int launch_dist_finalize(gpimhip_ctx* h, const gpimhip_model_t* m, int64_t N, const double* S, double q2, double lg,
                         double* u, int do_adam, AdamStep st, double* loss_out, double* grad_out, double* hist_row) {
    hipLaunchKernelGGL(dist_finalize_kernel, dim3(1), dim3(64), 0, h->stream, *m, N, S, q2, lg, h->theta, u, h->adam_m,
                       h->adam_v, do_adam, st, loss_out, grad_out, hist_row);
    HIP_TRY(hipGetLastError());
    return GPIMHIP_OK;
}

// ------------------------------------------------------------------------------------------
// Reflection blocks (engine.hip: kmat_refl_kernel has the model).  The gradient sums of grad_reduce_kernel for one block
// K_s: the same contraction with every entry's kernel value and derivative factors summed over the reflections (a mirror
// image's scaled difference (a_k + b_k - c_k / l_k) scales with 1 / l_k like the plain one).  Scalar, with the points'
// weights: the dense kernel's two-columns-per-lane loop and interior fast path are not for it.
// ------------------------------------------------------------------------------------------
template <int KIND>
__global__ __launch_bounds__(256) void grad_reduce_refl_kernel(const double* __restrict__ Kinv, int64_t ld,
                                                               const double* __restrict__ X, int64_t N, int d,
                                                               const double* __restrict__ alpha,
                                                               const ThetaDev* __restrict__ th, double* __restrict__ part,
                                                               int64_t x_bs, int64_t np, ReflArgs refl) {
    __shared__ double xa[128][4];
    __shared__ double xz[128][4];
    __shared__ double al_r[128], al_c[128];
    __shared__ double wr_s[128], wc_s[128];
    __shared__ double red[4][8];
    const int tid = threadIdx.x;
    const int sg = refl_sign_dims(refl.mask, refl.pb_off + (int)blockIdx.y * refl.pb_stride);
    const double* wts = refl.wts ? refl.wts + (int64_t)blockIdx.y * N : nullptr;
    Kinv += blockIdx.y * np * ld;
    X += blockIdx.y * x_bs;
    alpha += blockIdx.y * np;
    th += blockIdx.y;
    part += ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * 8;
    int ci, cj;
    lower_tile_from_linear(blockIdx.x, ci, cj);
    const ThetaDev t = *th;
    {
        const TileSlot s = tile_stage<4>(X, N, X, N, d, t, ci, cj, xa, xz);
        tile_put(s, al_r, al_c, s.valid ? alpha[s.g] : 0.0);
        tile_put(s, wr_s, wc_s, (wts && s.valid) ? wts[s.g] : 1.0);
    }
    __syncthreads();
    double cz[GPIMHIP_MAX_DIM];
    for (int k = 0; k < GPIMHIP_MAX_DIM; ++k) cz[k] = refl.twoc[k] / t.ls[k];
    double S[7] = {0, 0, 0, 0, 0, 0, 0};
    const int ty = tid >> 4, tx = tid & 15;
    for (int rr = 0; rr < 8; ++rr) {
        const int r = ty + 16 * rr;
        const int64_t gi = (int64_t)ci * 128 + r;
        const double ali = al_r[r];
        for (int cc = 0; cc < 8; ++cc) {
            const int c = tx + 16 * cc;
            const int64_t gj = (int64_t)cj * 128 + c;
            if (gi >= N || gj > gi) continue;
            const double g = Kinv[gi * ld + gj] - ali * al_c[c];
            const double ww = wr_s[r] * wc_s[c];
            if (ww == 0.0) continue;                   // (a point that does not exist in this block: an identity row)
            const double w = ((gi == gj) ? g : 2.0 * g) * ww;
            ReflPair p;
            for (int k = 0; k < GPIMHIP_MAX_DIM; ++k) {
                const double dm = xa[r][k] - xz[c][k], dp = (xa[r][k] + xz[c][k]) - cz[k];
                p.dm2[k] = dm * dm;
                p.dp2[k] = dp * dp;
            }
            refl_for_each(p, refl.mask, sg, [&](int gm, double chi, double r2) {
                const KVal kv = kfun_grad<KIND>(r2, t.alpha);
                const double wc = w * chi;
                S[0] = fma(wc, kv.e, S[0]);
                const double wh = wc * kv.h;
#pragma unroll
                for (int k = 0; k < GPIMHIP_MAX_DIM; ++k) S[1 + k] = fma(wh, ((gm >> k) & 1) ? p.dp2[k] : p.dm2[k], S[1 + k]);
                if (KIND == GPIMHIP_KERNEL_RQ) S[6] = fma(wc, kv.ga, S[6]);
            });
            if (gi == gj) S[5] += g;
        }
    }
    tile_sums_store<false>(S, red, part);
}
int launch_grad_reduce_refl(gpimhip_ctx* h, const gpimhip_model_t* m, const double* Kinv, int64_t ld, const double* X,
                            int64_t N, int nb, const double* alpha, int64_t x_bs) {
    const dim3 grid(nb * (nb + 1) / 2, h->nbatch), block(256);
    return with_kind(m->kernel, [&](auto K) {
        hipLaunchKernelGGL((grad_reduce_refl_kernel<decltype(K)::value>), grid, block, 0, h->stream, Kinv, ld, X, N, m->dim, alpha,
                           h->theta, h->grad_part, x_bs, h->np, h->refl);
        HIP_TRY(hipGetLastError());
        return GPIMHIP_OK;
    });
}
// The sums of the B coupled blocks, problem by problem in a fixed order, by one workgroup: S[0..7] (LDS, thread 0's to read)
// += the gradient sums, q2 += sum z zb, lg += sum log L_ii.  red: 256 doubles of LDS.
__device__ __forceinline__ void coupled_block_sums(int64_t np, int nb, int ntile, int B, const double* __restrict__ grad_part,
                                                   const double* __restrict__ z, const double* __restrict__ zb,
                                                   const double* __restrict__ logdet_part, double* red, double* S, double& q2,
                                                   double& lg) {
    const int tid = threadIdx.x;
    if (tid < 8) S[tid] = 0.0;
    __syncthreads();
    for (int b = 0; b < B; ++b) {
        for (int k = 0; k < 7; ++k) {
            double v = 0.0;
            for (int q = tid; q < ntile; q += 256) v += grad_part[((int64_t)b * ntile + q) * 8 + k];
            v = block_sum_256(v, red);
            if (tid == 0) S[k] += v;
        }
        double qb = 0.0;
        for (int64_t i = tid; i < np; i += 256) qb = fma(z[b * np + i], zb[b * np + i], qb);
        q2 += block_sum_256(qb, red);
        double lb = 0.0;
        for (int k = tid; k < nb; k += 256) lb += logdet_part[(int64_t)b * nb + k];
        lg += block_sum_256(lb, red);
    }
}
// finalize for the coupled blocks: the sums of all B problems, ONE loss / gradient / Adam step on the parameters of
// problem 0, which are then copied to the other problems' slots
__global__ __launch_bounds__(256) void finalize_coupled_kernel(gpimhip_model_t m, int64_t n_total, int64_t np, int nb, int ntile, int B,
                                                               const double* __restrict__ grad_part, const double* __restrict__ z,
                                                               const double* __restrict__ zb,
                                                               const double* __restrict__ logdet_part,
                                                               const ThetaDev* __restrict__ th, double* __restrict__ u,
                                                               double* __restrict__ adam_m, double* __restrict__ adam_v,
                                                               int do_adam, AdamStep st, FinalizeOut out,
                                                               int32_t* __restrict__ info,
                                                               const double* __restrict__ border_scal) {
    __shared__ double red[256];
    __shared__ double S[8];
    const int P = 2 + m.n_ls + (m.kernel == GPIMHIP_KERNEL_RQ ? 1 : 0);
    double q2 = 0.0, lg = 0.0;
    coupled_block_sums(np, nb, ntile, B, grad_part, z, zb, logdet_part, red, S, q2, lg);
    if (threadIdx.x != 0) return;
    if (border_scal) {          // border of the missing points (border.hip): - |L_S^-1 t|^2 and + log det L_S
        q2 -= border_scal[0];
        lg += border_scal[1];
    }
    if (!finalize_iter_begin(out.fi, info, P, st, out.loss_out, out.hist_row)) return;
    finalize_step(m, n_total, S, q2, lg, *th, u, adam_m, adam_v, do_adam, st, out.loss_out, out.grad_out, out.hist_row,
                  prior_constant(m));
    for (int b = 1; b < B; ++b)
        for (int k = 0; k < P; ++k) u[(int64_t)b * P + k] = u[k];
}
int launch_finalize_coupled(gpimhip_ctx* h, const gpimhip_model_t* m, int64_t N, int64_t np, double* u, int do_adam,
                            AdamStep st, const FinalizeOut& out, const double* border_scal) {
    const int nb = (int)(np / NB);
    hipLaunchKernelGGL(finalize_coupled_kernel, dim3(1), dim3(256), 0, h->stream, *m, h->refl.n_total > 0 ? h->refl.n_total : N * h->nbatch, np, nb,
                       nb * (nb + 1) / 2, h->nbatch,
                       h->grad_part, h->z, h->fp32 ? h->alpha : h->z, h->logdet_part, h->theta, u, h->adam_m, h->adam_v, do_adam,
                       st, out, h->info, border_scal);
    HIP_TRY(hipGetLastError());
    return GPIMHIP_OK;
}
// the sums of the LOCAL blocks, for a job that deals the blocks to its ranks (gpimhip_refl_sums): out[0..7] = the gradient
// sums, out[8] = sum log L_ii, out[9] = 1 if a factorisation failed, out[10] = sum |L^-1 y|^2
__global__ __launch_bounds__(256) void coupled_sums_kernel(int64_t np, int nb, int ntile, int B, const double* __restrict__ grad_part,
                                                           const double* __restrict__ z, const double* __restrict__ logdet_part,
                                                           const int32_t* __restrict__ info, double* __restrict__ out) {
    __shared__ double red[256];
    __shared__ double S[8];
    double q2 = 0.0, lg = 0.0;
    coupled_block_sums(np, nb, ntile, B, grad_part, z, z, logdet_part, red, S, q2, lg);
    if (threadIdx.x != 0) return;
    for (int k = 0; k < 8; ++k) out[k] = S[k];
    out[8] = lg;
    out[9] = (*info != 0) ? 1.0 : 0.0;
    out[10] = q2;
}
int launch_coupled_sums(gpimhip_ctx* h, int64_t np, double* out11) {
    const int nb = (int)(np / NB);
    hipLaunchKernelGGL(coupled_sums_kernel, dim3(1), dim3(256), 0, h->stream, np, nb, nb * (nb + 1) / 2, h->nbatch, h->grad_part,
                       h->z, h->logdet_part, h->info, out11);
    HIP_TRY(hipGetLastError());
    return GPIMHIP_OK;
}
