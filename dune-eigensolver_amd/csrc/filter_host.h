// filter_host.h -- host side of the Chebyshev window filter (slice.cpp launches what this plans): the
// Jackson-damped expansion coefficients of the indicator of [a, b], the scalars of every fused product
// step of its Clenshaw evaluation, the argument checks and the default degree.  Plain host arithmetic:
// no device code, no HIP runtime call and no context, so host tests compile filter_host.cpp alone and
// need no GPU.
#pragma once
#include "internal.h"

#include <vector>

namespace eigmi {

constexpr int kFilterMinDegree = 2;
constexpr int kFilterDefaultMin = 20, kFilterDefaultMax = 2000;  // clamp of the default degree

// The window in the filter's variable t = (lambda - c) / e: c, e from [lmin, lmax], the window clamped
// into it, theta_a = arccos a^ > theta_b = arccos b^.
struct FilterWindow {
  double c = 0.0, e = 1.0;
  double theta_a = 0.0, theta_b = 0.0;
};
// EIG_ERR_ARG unless the bounds are finite with lmin < lmax, a < b, and [a, b] meets [lmin, lmax].
FilterWindow filter_window(double a, double b, double lmin, double lmax);

// degree = 0: the Jackson kernel's resolution pi / (d + 2) at a quarter of the window's angular width
// theta_a - theta_b, i.e. d = ceil(4 pi / width) - 2, clamped to [kFilterDefaultMin, kFilterDefaultMax]
// (DESIGN.md 4g has the sweep behind the factor 4).
int filter_default_degree(const FilterWindow &w);

// gamma_k = g_k mu_k, k = 0 .. d: mu_0 = (theta_a - theta_b) / pi, mu_k = 2 (sin k theta_a - sin k theta_b)
// / (k pi), g_k the Jackson factors for alpha = pi / (d + 2).  degree = 0 takes the default; otherwise
// EIG_ERR_ARG below kFilterMinDegree.  Returns d.
int filter_coefs(double a, double b, double lmin, double lmax, int degree, std::vector<double> &gamma);

// One fused product step, out = s1 (A Xk) + s0 Xk + s2 Xold + g B.
struct FiltScalars {
  double s1, s0, s2, g;
};
// The step that forms b_k of the Clenshaw recurrence (k = d - 1 .. 1) or the result (k = 0), B = X throughout:
//   k = d - 1: Xk = X itself (b_d = gamma_d X is never formed: its factor goes into s1 and s0), s2 = 0
//   k = d - 2: Xk = b_{d-1}, and b_d = gamma_d X goes into g (g = gamma_k - gamma_d), s2 = 0
//   else:      Xk = b_{k+1}, Xold = b_{k+2} (overwritten), s2 = -1, g = gamma_k
// with s1 = 2 / e, s0 = -2 c / e for k >= 1 and s1 = 1 / e, s0 = -c / e for k = 0.
FiltScalars filter_step_scalars(const std::vector<double> &gamma, const FilterWindow &w, int k);

// p(t) at one point of [-1, 1] (the scalar Clenshaw sum; host tests and the count estimate's checks).
double filter_poly(const std::vector<double> &gamma, double t);

// Spectrum bounds from k Lanczos steps: the extreme eigenvalues of the tridiagonal (alpha[0 .. k-1] on the
// diagonal, beta[1 .. k-1] beside it) moved out by the last residual norm beta[k].
void lanczos_bounds(int k, const double *alpha, const double *beta, double &lmin, double &lmax);

}  // namespace eigmi
