// Stand-alone host test of csrc/filter_host.cpp (with csrc/dense.cpp for the tridiagonal eigenvalues): the
// Jackson-damped window coefficients, the per-step scalars of the folded Clenshaw evaluation against the
// textbook recurrence on a diagonal matrix, the default degree, the refusals and the Lanczos bounds.  No
// library and no GPU runtime; built plain and with ASan + UBSan by tests/test_filter_host.py.
#include <cmath>
#include <cstdio>
#include <vector>

#include "../../dune-eigensolver_amd/csrc/filter_host.h"

using namespace eigmi;

static int fails = 0;
#define CHECK(cond)                                                  \
  do {                                                               \
    if (!(cond))                                                     \
    {                                                                \
      std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);    \
      ++fails;                                                       \
    }                                                                \
  } while (0)

template <class F>
static int status_of(F &&f)
{
  try
  {
    f();
    return EIG_OK;
  }
  catch (const Error &e)
  {
    return e.code;
  }
}

static const double kPi = 3.14159265358979323846;

static void test_coefficients()
{
  const double a = 0.9, b = 1.2, lmin = 0.0, lmax = 13.0;
  for (int d : {2, 3, 20, 80, 200})
  {
    std::vector<double> g;
    CHECK(filter_coefs(a, b, lmin, lmax, d, g) == d);
    CHECK((int)g.size() == d + 1);
    const FilterWindow w = filter_window(a, b, lmin, lmax);
    CHECK(w.c == 6.5 && w.e == 6.5 && w.theta_a > w.theta_b);
    CHECK(g[0] == (w.theta_a - w.theta_b) / kPi);
    // independent formula for one inner coefficient
    const int k = d / 2 + 1;
    const double al = kPi / (d + 2);
    const double mu = 2.0 * (std::sin(k * w.theta_a) - std::sin(k * w.theta_b)) / (k * kPi);
    const double jk = ((d + 2 - k) * std::sin(al) * std::cos(k * al) + std::cos(al) * std::sin(k * al)) / ((d + 2) * std::sin(al));
    CHECK(std::fabs(g[k] - jk * mu) <= 1e-17);
    // the Jackson-damped expansion of an indicator stays in [0, 1]; ~1 at the window's centre for a resolving
    // degree, small far from it
    double lo = 1.0, hi = 0.0;
    for (int i = 0; i <= 2000; ++i)
    {
      const double p = filter_poly(g, -1.0 + 2.0 * i / 2000.0);
      lo = std::min(lo, p);
      hi = std::max(hi, p);
    }
    CHECK(lo > -1e-12 && hi < 1.0 + 1e-12);
    if (d >= 200)
    {
      CHECK(filter_poly(g, (1.05 - w.c) / w.e) > 0.9);
      CHECK(filter_poly(g, (6.0 - w.c) / w.e) < 1e-4);
    }
  }
  // the window is clamped into [lmin, lmax]
  std::vector<double> g1, g2;
  filter_coefs(-5.0, 1.0, 0.0, 13.0, 40, g1);
  filter_coefs(0.0, 1.0, 0.0, 13.0, 40, g2);
  CHECK(g1 == g2);
}

// The d product steps with their scalars on a diagonal matrix (one "row" per sample eigenvalue) against the
// textbook recurrence b_k = gamma_k x + 2 t b_{k+1} - b_{k+2}, p = gamma_0 x + t b_1 - b_2.
static void test_step_scalars()
{
  const double a = 4.0, b = 4.6, lmin = -2.0, lmax = 15.0;
  const FilterWindow w = filter_window(a, b, lmin, lmax);
  for (int d : {2, 3, 4, 5, 31})
  {
    std::vector<double> g;
    filter_coefs(a, b, lmin, lmax, d, g);
    for (int i = 0; i <= 40; ++i)
    {
      const double lam = lmin + (lmax - lmin) * i / 40.0, x = 1.0 + 0.25 * i;
      double cur = x, old = 0.0;  // the panels: cur = b_{k+1} (X itself at first), old = b_{k+2}
      for (int k = d - 1; k >= 0; --k)
      {
        const FiltScalars f = filter_step_scalars(g, w, k);
        if (k >= d - 2) CHECK(f.s2 == 0.0);
        else CHECK(f.s2 == -1.0);
        const double out = f.s1 * (lam * cur) + f.s0 * cur + (f.s2 != 0.0 ? f.s2 * old : 0.0) + f.g * x;
        old = cur;
        cur = out;
      }
      const double t = (lam - w.c) / w.e;
      double b1 = 0.0, b2 = 0.0;
      for (int k = d; k >= 1; --k)
      {
        const double b0 = g[k] * x + 2.0 * t * b1 - b2;
        b2 = b1;
        b1 = b0;
      }
      const double ref = g[0] * x + t * b1 - b2;
      CHECK(std::fabs(cur - ref) <= 1e-13 * std::max(1.0, std::fabs(ref)));
      CHECK(std::fabs(filter_poly(g, t) * x - ref) <= 1e-13 * std::max(1.0, std::fabs(ref)));
    }
    // the last step carries the half factor, the others the full one
    CHECK(filter_step_scalars(g, w, 0).s0 == -w.c * filter_step_scalars(g, w, 0).s1);
    if (d > 3) CHECK(filter_step_scalars(g, w, 1).s1 == 2.0 / w.e && filter_step_scalars(g, w, 0).s1 == 1.0 / w.e);
    CHECK(status_of([&] { filter_step_scalars(g, w, d); }) == EIG_ERR_ARG);
    CHECK(status_of([&] { filter_step_scalars(g, w, -1); }) == EIG_ERR_ARG);
  }
}

static void test_default_degree()
{
  auto deg = [](double a, double b) {
    std::vector<double> g;
    return filter_coefs(a, b, 0.0, 13.0, 0, g);
  };
  const FilterWindow w = filter_window(0.9, 1.2, 0.0, 13.0);
  CHECK(deg(0.9, 1.2) == (int)(std::ceil(4.0 * kPi / (w.theta_a - w.theta_b)) - 2.0));
  CHECK(filter_default_degree(w) == deg(0.9, 1.2));
  CHECK(deg(6.0, 6.001) == kFilterDefaultMax);
  CHECK(deg(0.0, 13.0) == kFilterDefaultMin);
  CHECK(deg(0.9, 1.2) > deg(0.9, 1.5));  // a narrower window takes a higher degree
}

static void test_refusals()
{
  std::vector<double> g;
  auto st = [&](double a, double b, double lmin, double lmax, int d) {
    return status_of([&] { filter_coefs(a, b, lmin, lmax, d, g); });
  };
  CHECK(st(0.9, 1.2, 0.0, 13.0, 80) == EIG_OK);
  CHECK(st(1.2, 0.9, 0.0, 13.0, 80) == EIG_ERR_ARG);
  CHECK(st(1.0, 1.0, 0.0, 13.0, 80) == EIG_ERR_ARG);
  CHECK(st(14.0, 15.0, 0.0, 13.0, 80) == EIG_ERR_ARG);
  CHECK(st(-3.0, -1.0, 0.0, 13.0, 80) == EIG_ERR_ARG);
  CHECK(st(0.9, 1.2, 13.0, 0.0, 80) == EIG_ERR_ARG);
  CHECK(st(0.9, 1.2, 5.0, 5.0, 80) == EIG_ERR_ARG);
  CHECK(st(0.9, 1.2, 0.0, 13.0, 1) == EIG_ERR_ARG);
  CHECK(st(0.9, 1.2, 0.0, 13.0, -7) == EIG_ERR_ARG);
  CHECK(st(0.9, std::nan(""), 0.0, 13.0, 80) == EIG_ERR_ARG);
  CHECK(st(0.9, 1.2, 0.0, HUGE_VAL, 80) == EIG_ERR_ARG);
  CHECK(st(13.0, 14.0, 0.0, 13.0, 2) == EIG_OK);  // touching the bound is not empty
}

static void test_lanczos_bounds()
{
  // T = tridiag(-1, 2, -1) of order 5: eigenvalues 2 - 2 cos(j pi / 6)
  const double alpha[5] = {2.0, 2.0, 2.0, 2.0, 2.0}, beta[6] = {0.0, -1.0, -1.0, -1.0, -1.0, 0.375};
  double lo = 0.0, hi = 0.0;
  lanczos_bounds(5, alpha, beta, lo, hi);
  CHECK(std::fabs(lo - (2.0 - 2.0 * std::cos(kPi / 6.0) - 0.375)) <= 1e-14);
  CHECK(std::fabs(hi - (2.0 - 2.0 * std::cos(5.0 * kPi / 6.0) + 0.375)) <= 1e-14);
  const double b1[2] = {0.0, 0.5};
  lanczos_bounds(1, alpha, b1, lo, hi);  // one step: alpha -+ beta_1
  CHECK(lo == 1.5 && hi == 2.5);
  CHECK(status_of([&] { lanczos_bounds(0, alpha, beta, lo, hi); }) == EIG_ERR_ARG);
}

int main()
{
  test_coefficients();
  test_step_scalars();
  test_default_degree();
  test_refusals();
  test_lanczos_bounds();
  if (fails == 0) std::printf("ALL OK\n");
  return fails == 0 ? 0 : 1;
}
