// eigmi::Multigrid and eigmi::Lobpcg::precond_mg (include/eigmi.hh) on the 3x3-blocked Q1 elasticity matrix of
// 6 x 6 x 6 nodes (eig_gen_matrix kind 5): the hierarchy's shape, a solve whose reported residual equals the one
// computed on the host from the downloaded X and falls with the cycle count, LOBPCG with one V-cycle against
// LOBPCG with Chebyshev-Jacobi, and the facade's error mapping.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <vector>

#include "eigmi.hh"

// a host array in MultiVector<double,8> layout, as DeviceMultiVector::upload / download take it
struct Flat {
  static const std::size_t blocksize = 8;
  double *p;
  double &operator()(std::size_t, std::size_t) const { return *p; }
};

int main()
{
  const int N = 6, b = 3, m = 8, nev = 4;
  const int64_t nb = (int64_t)N * N * N, n = nb * b;
  std::vector<int64_t> rowptr(nb + 1);
  std::vector<int32_t> col(eig_gen_nnzb(5, N));
  std::vector<double> val(col.size() * b * b);
  if (eig_gen_matrix(5, N, 0, rowptr.data(), col.data(), val.data()) != EIG_OK) return std::printf("generator failed\n"), 1;
  int failures = 0;
  auto expect = [&](bool ok, const char *what) {
    if (!ok) std::printf("FAILED: %s\n", what), ++failures;
  };
  eigmi::Context ctx(0);
  auto K = eigmi::Matrix::from_bcsr(ctx, rowptr, col, val, b, b);
  expect(K.info().n == n, "n = block rows * 3");
  eigmi::Multigrid mg(K, N, N, N, 8, 2, 5.0);
  const eigmi::Multigrid::Info inf = mg.info();
  std::printf("multigrid on q1elast(6): %d levels, %lld coarse rows, coarse degree %d, lmax %.6f\n", inf.levels,
              (long long)inf.coarse_rows, inf.coarse_degree, inf.lmax_fine);
  expect(inf.levels == 2 && inf.coarse_rows == 27 * b && inf.coarse_degree >= 1 && inf.lmax_fine > 1.0, "hierarchy shape");

  // B: fixed pseudo-random columns (MultiVector<double,8> layout with one block: entry (r, j) at r * 8 + j)
  std::vector<double> hB((size_t)n * m), hX(hB.size());
  unsigned long long st = 12345;
  for (double &v : hB) st = st * 6364136223846793005ull + 1442695040888963407ull, v = (double)(st >> 11) / 9007199254740992.0 - 0.5;
  eigmi::DeviceMultiVector dB(ctx, n, m), dX(ctx, n, m);
  Flat fB{hB.data()}, fX{hX.data()};
  dB.upload(fB);
  double prev = 1.0;
  for (int cycles : {1, 3, 6})
  {
    const double r = mg.solve(dB, dX, cycles, true);
    dX.download(fX);
    double worst = 0.0;
    std::vector<double> x(n), y(n);
    for (int j = 0; j < m; ++j)
    {
      for (int64_t i = 0; i < n; ++i) x[i] = hX[(size_t)i * 8 + j];
      K.mv_host(x.data(), y.data());
      double rr = 0.0, bb = 0.0;
      for (int64_t i = 0; i < n; ++i)
      {
        const double bj = hB[(size_t)i * 8 + j];
        rr += (bj - y[i]) * (bj - y[i]);
        bb += bj * bj;
      }
      worst = std::max(worst, std::sqrt(rr / bb));
    }
    std::printf("  %d cycle(s): reported residual %.6e, host %.6e\n", cycles, r, worst);
    expect(std::fabs(r - worst) <= 1e-9 * worst, "reported residual equals the host's");
    expect(r < prev, "the residual falls with the cycles");
    prev = r;
  }
  expect(prev < 1e-2, "six cycles reduce the residual below 1e-2");

  // LOBPCG, K x = lambda x: one V-cycle against Chebyshev-Jacobi (degree 4 on [g / 10, g], g the scalar Gershgorin bound)
  double g = 0.0;
  for (int64_t I = 0; I < nb; ++I)
    for (int r = 0; r < b; ++r)
    {
      double s = 0.0, d = 0.0;
      for (int64_t q = rowptr[I]; q < rowptr[I + 1]; ++q)
        for (int c = 0; c < b; ++c)
        {
          s += std::fabs(val[(size_t)q * 9 + r * 3 + c]);
          if (col[q] == I && c == r) d = val[(size_t)q * 9 + r * 3 + c];
        }
      g = std::max(g, s / d);
    }
  std::vector<double> lmg, lch, res;
  int it_mg = 0, it_ch = 0;
  {
    eigmi::Lobpcg s(K, nullptr, 8);
    s.precond_mg(mg, 1);
    expect(s.step(300, nev, 1e-8, &it_mg), "LOBPCG with one V-cycle converges");
    s.ritz(nev, lmg, nullptr, &res);
  }
  {
    eigmi::Lobpcg s(K, nullptr, 8);
    s.precond_cheb(4, g / 10.0, g);
    expect(s.step(300, nev, 1e-8, &it_ch), "LOBPCG with Chebyshev-Jacobi converges");
    s.ritz(nev, lch);
  }
  std::printf("LOBPCG q1elast(6): %d iterations with one V-cycle, %d with Chebyshev-Jacobi degree 4\n", it_mg, it_ch);
  for (int i = 0; i < nev; ++i)
  {
    std::printf("  lambda %.15g (Chebyshev run %.15g) residual %.2e\n", lmg[i], lch[i], res[i]);
    expect(std::fabs(lmg[i] / lch[i] - 1) <= 1e-10 && res[i] <= 1e-8 * lmg[i], "eigenvalue and residual");
  }
  try  // node extents that do not multiply to the block rows: EIG_ERR_SHAPE -> std::invalid_argument or runtime_error
  {
    eigmi::Multigrid bad(K, N, N, N + 1);
    expect(false, "wrong extents must throw");
  }
  catch (const std::exception &)
  {
  }
  if (failures) return std::printf("%d FAILURES\n", failures), 1;
  std::printf("ALL OK\n");
  return 0;
}
