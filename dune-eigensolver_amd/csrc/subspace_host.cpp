// subspace_host.cpp -- host arithmetic shared by the block eigensolvers (subspace_host.h).  No device call,
// no HIP header and no context; links with dense.cpp alone.
#include "subspace_host.h"

#include <algorithm>
#include <cmath>

namespace eigmi {

// dense.cpp (internal.h declares it beside the device structures, which this file stays clear of)
void sym_eig(int n, const std::vector<double> &A, std::vector<double> &w, std::vector<double> &Z);

void symmetrise(int N, std::vector<double> &H)
{
  for (int r = 0; r < N; ++r)
    for (int c = r + 1; c < N; ++c)
      H[(size_t)r * N + c] = H[(size_t)c * N + r] = 0.5 * (H[(size_t)r * N + c] + H[(size_t)c * N + r]);
}

void ritz_select(int N, std::vector<double> &H, int m, int which, std::vector<double> &theta, std::vector<double> &Cx)
{
  std::vector<double> ev, Z;
  symmetrise(N, H);
  sym_eig(N, H, ev, Z);
  theta.resize(m);
  Cx.assign((size_t)N * m, 0.0);
  for (int j = 0; j < m; ++j)
  {
    const int pick = which == EIG_WHICH_LA ? N - 1 - j : j;
    theta[j] = ev[pick];
    for (int r = 0; r < N; ++r) Cx[(size_t)r * m + j] = Z[(size_t)r * N + pick];
  }
}

void householder_q(int N, int m, std::vector<double> &A, std::vector<double> &Q)
{
  std::vector<double> V((size_t)N * m, 0.0), beta(m, 0.0);  // reflector j: I - beta_j v_j v_j^T, v_j in column j
  for (int j = 0; j < m; ++j)
  {
    double nrm = 0.0;
    for (int r = j; r < N; ++r) nrm += A[(size_t)r * m + j] * A[(size_t)r * m + j];
    nrm = std::sqrt(nrm);
    if (nrm == 0.0) continue;  // a zero column: no reflector (Q keeps the unit vector e_j)
    const double a = A[(size_t)j * m + j];
    const double alpha = a >= 0.0 ? -nrm : nrm;
    for (int r = j; r < N; ++r) V[(size_t)r * m + j] = A[(size_t)r * m + j];
    V[(size_t)j * m + j] = a - alpha;
    double vv = 0.0;
    for (int r = j; r < N; ++r) vv += V[(size_t)r * m + j] * V[(size_t)r * m + j];
    if (vv == 0.0) continue;
    beta[j] = 2.0 / vv;
    for (int c = j; c < m; ++c)
    {
      double d = 0.0;
      for (int r = j; r < N; ++r) d += V[(size_t)r * m + j] * A[(size_t)r * m + c];
      d *= beta[j];
      for (int r = j; r < N; ++r) A[(size_t)r * m + c] -= d * V[(size_t)r * m + j];
    }
  }
  Q.assign((size_t)N * m, 0.0);
  for (int j = 0; j < m; ++j) Q[(size_t)j * m + j] = 1.0;
  for (int j = m - 1; j >= 0; --j)
  {
    if (beta[j] == 0.0) continue;
    for (int c = 0; c < m; ++c)
    {
      double d = 0.0;
      for (int r = j; r < N; ++r) d += V[(size_t)r * m + j] * Q[(size_t)r * m + c];
      d *= beta[j];
      for (int r = j; r < N; ++r) Q[(size_t)r * m + c] -= d * V[(size_t)r * m + j];
    }
  }
}

void search_coefficients(int N, int m, const std::vector<double> &Cx, std::vector<double> &C)
{
  std::vector<double> Cp = Cx, G((size_t)m * m), Q;
  std::fill(Cp.begin(), Cp.begin() + (size_t)m * m, 0.0);
  for (int pass = 0; pass < 2; ++pass)
  {
    for (int a = 0; a < m; ++a)
      for (int b = 0; b < m; ++b)
      {
        double d = 0.0;
        for (int r = 0; r < N; ++r) d += Cx[(size_t)r * m + a] * Cp[(size_t)r * m + b];
        G[(size_t)a * m + b] = d;
      }
    for (int r = 0; r < N; ++r)
      for (int b = 0; b < m; ++b)
      {
        double d = 0.0;
        for (int a = 0; a < m; ++a) d += Cx[(size_t)r * m + a] * G[(size_t)a * m + b];
        Cp[(size_t)r * m + b] -= d;
      }
  }
  householder_q(N, m, Cp, Q);
  C.assign((size_t)N * 2 * m, 0.0);
  for (int r = 0; r < N; ++r)
    for (int j = 0; j < m; ++j)
    {
      C[(size_t)r * 2 * m + j] = Cx[(size_t)r * m + j];
      C[(size_t)r * 2 * m + m + j] = Q[(size_t)r * m + j];
    }
}

std::vector<double> block_tridiag(int b, int k, const std::vector<double> &A, const std::vector<double> &B)
{
  const int N = k * b;
  std::vector<double> T((size_t)N * N, 0.0);
  for (int j = 0; j < k; ++j)
  {
    for (int r = 0; r < b; ++r)
      for (int c = 0; c < b; ++c) T[(size_t)(j * b + r) * N + j * b + c] = A[((size_t)j * b + r) * b + c];
    if (j + 1 < k)  // T_{j+1,j} = B_{j+1}, T_{j,j+1} = B_{j+1}^T
      for (int r = 0; r < b; ++r)
        for (int c = 0; c < b; ++c)
        {
          const double v = B[((size_t)j * b + r) * b + c];
          T[(size_t)((j + 1) * b + r) * N + j * b + c] = v;
          T[(size_t)(j * b + c) * N + (j + 1) * b + r] = v;
        }
  }
  return T;
}

void si_ritz_order(std::vector<double> &th, double sigma, int nev, int which, std::vector<int> &pick)
{
  const int N = (int)th.size();
  std::vector<int> ord(N);
  for (int i = 0; i < N; ++i) ord[i] = i;
  std::stable_sort(ord.begin(), ord.end(), [&](int a, int c) { return std::fabs(th[a]) > std::fabs(th[c]); });
  ord.resize(nev);
  for (int i = 0; i < N; ++i) th[i] = th[i] != 0.0 ? sigma + 1.0 / th[i] : HUGE_VAL;
  std::stable_sort(ord.begin(), ord.end(), [&](int a, int c) {
    return which == EIG_WHICH_SA ? th[a] < th[c] : th[a] > th[c];
  });
  pick = ord;
}

bool lobpcg_converged(const std::vector<double> &sums, const std::vector<double> &theta, int m, int nev, double tol)
{
  bool conv = true;
  for (int j = 0; j < nev; ++j)
    conv = conv && std::sqrt(sums[j]) <= tol * std::fabs(theta[j]) * std::sqrt(sums[m + j]);
  return conv;
}

bool window_converged(const std::vector<double> &theta, const std::vector<double> &rr, const std::vector<double> &xx,
                      double a, double b, double tol)
{
  if (rr.empty()) return false;
  const double scale = std::max(std::fabs(a), std::fabs(b));
  int cnt = 0;
  for (size_t j = 0; j < theta.size(); ++j)
  {
    if (!window_accept(theta[j], a, b)) continue;
    ++cnt;
    if (!(std::sqrt(rr[j]) <= tol * std::max(std::fabs(theta[j]), scale) * std::sqrt(xx[j]))) return false;
  }
  return cnt > 0;
}

double orth_deviation(int N, const std::vector<double> &G)
{
  double dev = 0.0;
  for (int r = 0; r < N; ++r)
    for (int c = 0; c < N; ++c)
    {
      const double d = std::fabs(G[(size_t)r * N + c] - (r == c ? 1.0 : 0.0));
      if (!(d <= dev)) dev = d == d ? d : HUGE_VAL;  // (a NaN counts as a miss)
    }
  return dev;
}

bool cholqr_reuse(int b, const std::vector<double> &R0)
{
  double dmax = 0.0, dmin = HUGE_VAL;
  for (int i = 0; i < b; ++i)
  {
    const double d = std::fabs(R0[(size_t)i * b + i]);
    dmax = std::max(dmax, d);
    dmin = std::min(dmin, d);
  }
  return dmin > 0.0 && dmax <= kCholQrReuseCond * dmin;
}

void mv8_column(const double *h, int64_t ld, int64_t own, int64_t n, int j, double scale, double *out)
{
  const double *col = h + ((size_t)(j / 8) * ld + own) * 8 + j % 8;
  for (int64_t r = 0; r < n; ++r) out[r] = scale * col[(size_t)r * 8];
}

}  // namespace eigmi
