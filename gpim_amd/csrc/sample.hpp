// sample.hpp -- shared declarations of the joint posterior draws (sample.hip kernels, api.hip driver).
#pragma once
#include "common.hpp"

// J[i][i] += jitter + noise(theta) for the n_train leading points, += (noiseless ? 0 : noise(theta)) + jitter_s for the
// n_test points behind them (the identity padding at the end is kmat's)
int launch_sample_diag(gpimhip_ctx* h, double* J, int64_t ld, int64_t n_train, int64_t n_test, const ThetaDev* theta,
                       int noiseless, double jitter_s);
// One sweep of the trapezoid L[N:, :] of the factor of the joint matrix (sample.hip): mean, variance and the draws
// s0 .. s0 + min(S - s0, group) - 1.  mean_ws (M): written when s0 == 0, read by the later groups.
int launch_sample_draws(gpimhip_ctx* h, const double* L, int64_t ld, int64_t N, int64_t M, const double* z, const double* Z,
                        int S, int s0, const ThetaDev* theta, int noiseless, double jitter_s, double* mean_ws,
                        double* mean_out, double* var_out, double* out);
int sample_draw_group(int S);
