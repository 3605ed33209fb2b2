// refl.hpp -- the reflection helpers of the symmetry-reduced exact GP (engine.hip: kmat_refl_kernel; grad.hip: grad_reduce_refl_kernel;
// vgp.hip: vgp_kbeta_refl_kernel).  See engine.hip for the model.
#pragma once
#include "kfun.hpp"

struct ReflPair {
    double dm2[GPIMHIP_MAX_DIM], dp2[GPIMHIP_MAX_DIM];       // squared scaled differences to z and to its mirror image
};
// the dimensions whose sign is -1 in the block of problem pb: bit j of pb belongs to the j-th reflected dimension
__device__ __forceinline__ int refl_sign_dims(int mask, int pb) {
    int sg = 0, j = 0;
#pragma unroll
    for (int k = 0; k < GPIMHIP_MAX_DIM; ++k)
        if ((mask >> k) & 1) {
            if ((pb >> j) & 1) sg |= 1 << k;
            ++j;
        }
    return sg;
}
// f(g, chi, r2) for every reflection g (a subset of mask, as a bit mask over the dimensions); constant trip counts and a
// wave-uniform skip, so that everything stays in registers (unused dimensions hold zeros in p)
template <typename F>
__device__ __forceinline__ void refl_for_each(const ReflPair& p, int mask, int sg, F f) {
#pragma unroll
    for (int g = 0; g < (1 << GPIMHIP_MAX_DIM); ++g) {
        if (g & ~mask) continue;
        double r2 = 0.0;
#pragma unroll
        for (int k = 0; k < GPIMHIP_MAX_DIM; ++k) r2 += ((g >> k) & 1) ? p.dp2[k] : p.dm2[k];
        f(g, (__popc(g & sg) & 1) ? -1.0 : 1.0, r2);
    }
}
