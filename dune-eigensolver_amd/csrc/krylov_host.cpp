// krylov_host.cpp -- host arithmetic of the Krylov drivers (krylov_host.h).  No HIP runtime call.
#include "krylov_host.h"

namespace eigmi {

// position of block column `col` in block row i of A, or -1
static i64 find_block(const HostCsr &A, i64 i, i32 col)
{
  const i32 *b0 = A.c.data() + A.rp[i], *b1 = A.c.data() + A.rp[i + 1];
  const i32 *hit = std::lower_bound(b0, b1, col);
  return hit != b1 && *hit == col ? (i64)(hit - A.c.data()) : -1;
}

void pattern_axpy(i64 r0, i64 r1, int b, HostCsr &A, double alpha, const HostCsr &B, const char *who)
{
  if (alpha == 0.0) return;
  const int bb = b * b;
  for (i64 i = r0; i < r1; ++i)
    for (i64 q = B.rp[i]; q < B.rp[i + 1]; ++q)
    {
      const i64 hit = find_block(A, i, B.c[q]);
      EIG_CHECK(hit >= 0, EIG_ERR_SHAPE, std::string(who) + ": pattern(B) must be contained in pattern(A)");
      for (int t = 0; t < bb; ++t) A.v[(size_t)hit * bb + t] += alpha * B.v[(size_t)q * bb + t];
    }
}

void pattern_shift_diag(i64 r0, i64 r1, int b, HostCsr &A, double alpha, const char *who)
{
  if (alpha == 0.0) return;
  const int bb = b * b;
  for (i64 i = r0; i < r1; ++i)
  {
    const i64 hit = find_block(A, i, (i32)i);
    EIG_CHECK(hit >= 0, EIG_ERR_SHAPE, std::string(who) + ": A has no diagonal entry");
    // the identity's block: alpha onto the diagonal entries of the diagonal block
    for (int d = 0; d < b; ++d) A.v[(size_t)hit * bb + d * b + d] += alpha;
  }
}

double extension_column(int m, int j, const double *row, std::vector<double> &ctot, const char *breakdown)
{
  std::fill(ctot.begin(), ctot.end(), 0.0);
  for (int pass = 0; pass < 2; ++pass)
    for (int i = 0; i <= j; ++i) ctot[i] += row[pass * (m + 1) + i];
  const double beta = std::sqrt(std::max(0.0, row[2 * (m + 1)]));
  double cmax = 0.0;
  for (int i = 0; i <= j; ++i) cmax = std::max(cmax, std::fabs(ctot[i]));
  EIG_CHECK(beta > 1e-14 * cmax, EIG_ERR_BREAKDOWN, breakdown);
  return beta;
}

void krylov_schur_restart(int m, int nev, std::vector<double> &G, std::vector<double> &cvec,
                          const std::vector<std::complex<double>> &w, const std::vector<std::complex<double>> &Y,
                          const std::vector<int> &ord, int &kk, std::vector<double> &Z,
                          std::vector<std::pair<int, bool>> &units)
{
  // about nev + (m - nev) / 2 wanted vectors, never splitting a conjugate pair.  The kept set is built from
  // whole units in "LM" order -- a real Ritz value (one column) or a conjugate pair (real and imaginary
  // part: two columns; its partner is looked up by value, wherever the sort put it) -- so span(Z) is
  // G-invariant whatever the ordering of equal moduli.
  const int target = thick_restart_size(m, nev);
  units.clear();  // (eigenvalue index, complex pair)
  kk = 0;
  {
    std::vector<char> used(m, 0);
    for (int q = 0; q < m && kk < target; ++q)
    {
      const int e = ord[q];
      if (used[e]) continue;
      used[e] = 1;
      const bool cplx = w[e].imag() != 0.0;
      if (cplx)
      {
        int partner = -1;
        for (int q2 = 0; q2 < m; ++q2)
          if (!used[ord[q2]] && w[ord[q2]] == std::conj(w[e]))
          {
            partner = ord[q2];
            break;
          }
        EIG_CHECK(partner >= 0, EIG_ERR_BREAKDOWN, "Arnoldi: complex Ritz value without its conjugate");
        used[partner] = 1;
        if (kk + 2 > m - 1) break;  // a pair that does not fit is dropped whole
      }
      units.push_back({e, cplx});
      kk += cplx ? 2 : 1;
    }
  }
  EIG_CHECK(kk >= 1, EIG_ERR_BREAKDOWN, "Arnoldi: no Ritz vector to keep at restart");
  Z.assign((size_t)m * kk, 0.0);  // row-major m x kk
  {
    int col = 0;
    for (auto &u : units)
    {
      for (int i = 0; i < m; ++i) Z[(size_t)i * kk + col] = Y[(size_t)i * m + u.first].real();
      ++col;
      if (u.second)
      {
        for (int i = 0; i < m; ++i) Z[(size_t)i * kk + col] = Y[(size_t)i * m + u.first].imag();
        ++col;
      }
    }
    for (int c = 0; c < kk; ++c)  // MGS, twice
      for (int pass = 0; pass < 2; ++pass)
      {
        for (int p = 0; p < c; ++p)
        {
          double d = 0.0;
          for (int i = 0; i < m; ++i) d += Z[(size_t)i * kk + p] * Z[(size_t)i * kk + c];
          for (int i = 0; i < m; ++i) Z[(size_t)i * kk + c] -= d * Z[(size_t)i * kk + p];
        }
        double nr = 0.0;
        for (int i = 0; i < m; ++i) nr += Z[(size_t)i * kk + c] * Z[(size_t)i * kk + c];
        nr = std::sqrt(nr);
        EIG_CHECK(nr > 0.0, EIG_ERR_BREAKDOWN, "Arnoldi: dependent Ritz vectors at restart");
        for (int i = 0; i < m; ++i) Z[(size_t)i * kk + c] /= nr;
      }
  }
  // G <- Z^T G Z, c <- Z^T c
  std::vector<double> GZ((size_t)m * kk, 0.0), Gn((size_t)m * m, 0.0), cn(kk, 0.0);
  for (int i = 0; i < m; ++i)
    for (int q = 0; q < kk; ++q)
    {
      double a = 0.0;
      for (int l = 0; l < m; ++l) a += G[(size_t)i * m + l] * Z[(size_t)l * kk + q];
      GZ[(size_t)i * kk + q] = a;
    }
  for (int p = 0; p < kk; ++p)
  {
    for (int q = 0; q < kk; ++q)
    {
      double a = 0.0;
      for (int i = 0; i < m; ++i) a += Z[(size_t)i * kk + p] * GZ[(size_t)i * kk + q];
      Gn[(size_t)p * m + q] = a;
    }
    for (int i = 0; i < m; ++i) cn[p] += Z[(size_t)i * kk + p] * cvec[i];
  }
  {
    // the restarted decomposition is a Krylov decomposition only if span(Z) is G-invariant:
    // ||G Z - Z (Z^T G Z)|| small relative to ||G||
    double gmax = 0.0, rmax = 0.0;
    for (double g : G) gmax = std::max(gmax, std::fabs(g));
    for (int i = 0; i < m; ++i)
      for (int q = 0; q < kk; ++q)
      {
        double a = GZ[(size_t)i * kk + q];
        for (int p = 0; p < kk; ++p) a -= Z[(size_t)i * kk + p] * Gn[(size_t)p * m + q];
        rmax = std::max(rmax, std::fabs(a));
      }
    EIG_CHECK(rmax <= 1e-6 * std::max(gmax, 1e-300), EIG_ERR_BREAKDOWN,
              "Arnoldi: restart subspace is not invariant under the projected matrix");
  }
  G.swap(Gn);
  cvec = cn;
}

}  // namespace eigmi
