// filter_host.cpp -- host side of the Chebyshev window filter (filter_host.h): window, coefficients,
// per-step scalars, default degree, Lanczos spectrum bounds.  No device call and no context.
#include "filter_host.h"

#include <algorithm>
#include <cmath>

namespace eigmi {

namespace {
const double kPi = 3.14159265358979323846;
}

FilterWindow filter_window(double a, double b, double lmin, double lmax)
{
  EIG_CHECK(std::isfinite(a) && std::isfinite(b) && std::isfinite(lmin) && std::isfinite(lmax) && lmin < lmax,
            EIG_ERR_ARG, "filter: finite bounds with lmin < lmax required");
  EIG_CHECK(a < b, EIG_ERR_ARG, "filter: a < b required");
  EIG_CHECK(!(b < lmin) && !(a > lmax), EIG_ERR_ARG, "filter: [a, b] does not meet [lmin, lmax]");
  FilterWindow w;
  w.c = 0.5 * (lmax + lmin);
  w.e = 0.5 * (lmax - lmin);
  const double ah = std::min(1.0, std::max(-1.0, (std::max(a, lmin) - w.c) / w.e));
  const double bh = std::min(1.0, std::max(-1.0, (std::min(b, lmax) - w.c) / w.e));
  w.theta_a = std::acos(ah);
  w.theta_b = std::acos(bh);
  return w;
}

int filter_default_degree(const FilterWindow &w)
{
  const double width = w.theta_a - w.theta_b;
  if (!(width > 0.0)) return kFilterDefaultMax;
  const double d = std::ceil(4.0 * kPi / width) - 2.0;
  return (int)std::min((double)kFilterDefaultMax, std::max((double)kFilterDefaultMin, d));
}

int filter_coefs(double a, double b, double lmin, double lmax, int degree, std::vector<double> &gamma)
{
  const FilterWindow w = filter_window(a, b, lmin, lmax);
  const int d = degree == 0 ? filter_default_degree(w) : degree;
  EIG_CHECK(d >= kFilterMinDegree, EIG_ERR_ARG, "filter: degree >= 2 (or 0 for the default) required");
  const double al = kPi / (d + 2);
  gamma.assign((size_t)d + 1, 0.0);
  for (int k = 0; k <= d; ++k)
  {
    const double mu = k == 0 ? (w.theta_a - w.theta_b) / kPi
                             : 2.0 * (std::sin(k * w.theta_a) - std::sin(k * w.theta_b)) / (k * kPi);
    const double g = ((d + 2 - k) * std::sin(al) * std::cos(k * al) + std::cos(al) * std::sin(k * al)) /
                     ((d + 2) * std::sin(al));
    gamma[k] = g * mu;
  }
  return d;
}

FiltScalars filter_step_scalars(const std::vector<double> &gamma, const FilterWindow &w, int k)
{
  const int d = (int)gamma.size() - 1;
  EIG_CHECK(d >= kFilterMinDegree && k >= 0 && k < d, EIG_ERR_ARG, "filter step: 0 <= k < degree required");
  FiltScalars f;
  f.s1 = (k == 0 ? 1.0 : 2.0) / w.e;
  f.s0 = -w.c * f.s1;
  f.s2 = -1.0;
  f.g = gamma[k];
  if (k == d - 1)
  {
    f.s1 = gamma[d] * f.s1;
    f.s0 = gamma[d] * f.s0;
    f.s2 = 0.0;
  }
  else if (k == d - 2)
  {
    f.s2 = 0.0;
    f.g = gamma[k] - gamma[d];
  }
  return f;
}

double filter_poly(const std::vector<double> &gamma, double t)
{
  double b1 = 0.0, b2 = 0.0;
  for (int k = (int)gamma.size() - 1; k >= 1; --k)
  {
    const double b0 = gamma[k] + 2.0 * t * b1 - b2;
    b2 = b1;
    b1 = b0;
  }
  return gamma[0] + t * b1 - b2;
}

void lanczos_bounds(int k, const double *alpha, const double *beta, double &lmin, double &lmax)
{
  EIG_CHECK(k >= 1 && alpha && beta, EIG_ERR_ARG, "spectrum bounds: at least one Lanczos step required");
  std::vector<double> d(alpha, alpha + k), e(k > 1 ? k - 1 : 0), Z;
  for (int j = 1; j < k; ++j) e[j - 1] = beta[j];
  tridiag_eig(k, d, e, Z);
  lmin = d[0] - beta[k];
  lmax = d[k - 1] + beta[k];
}

}  // namespace eigmi
