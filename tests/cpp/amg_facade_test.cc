// eigmi::Multigrid::amg and eigmi::Multigrid::level_info (include/eigmi.hh) on the 7-point Poisson matrix of
// 12 x 12 x 12 nodes (eig_gen_matrix kind 4), built without its grid: the hierarchy's shape and operator complexity,
// a solve whose residual falls with the cycle count, LOBPCG with one V-cycle, and the refusal of a theta above the
// stencil's strength 1/6 as an exception.
#include <cmath>
#include <cstdio>
#include <vector>

#include "eigmi.hh"

struct Flat {
  static const std::size_t blocksize = 8;
  double *p;
  double &operator()(std::size_t, std::size_t) const { return *p; }
};

int main()
{
  const int N = 12, m = 8, nev = 4;
  const int64_t n = (int64_t)N * N * N;
  std::vector<int64_t> rowptr(n + 1);
  std::vector<int32_t> col(eig_gen_nnzb(4, N));
  std::vector<double> val(col.size());
  if (eig_gen_matrix(4, N, 0, rowptr.data(), col.data(), val.data()) != EIG_OK) return std::printf("generator failed\n"), 1;
  int failures = 0;
  auto expect = [&](bool ok, const char *what) {
    if (!ok) std::printf("FAILED: %s\n", what), ++failures;
  };
  eigmi::Context ctx(0);
  auto K = eigmi::Matrix::from_bcsr(ctx, rowptr, col, val, 1, 1);
  eigmi::Multigrid mg = eigmi::Multigrid::amg(K, 0.08, 8, 2, 5.0);
  const eigmi::Multigrid::Info inf = mg.info();
  int64_t total = 0;
  for (int l = 0; l < inf.levels; ++l)
  {
    const eigmi::Multigrid::LevelInfo li = mg.level_info(l);
    std::printf("level %d: %lld rows, %lld entries, lmax %.6f\n", l, (long long)li.rows, (long long)li.nnz, li.lmax);
    expect(li.rows >= 1 && li.nnz >= li.rows && li.lmax >= 1.0, "level info");
    if (l == 0) expect(li.rows == n && li.nnz == (int64_t)col.size(), "level 0 is the matrix");
    total += li.nnz;
  }
  expect(inf.levels >= 2 && inf.coarse_rows <= 1024 && inf.coarse_rows == mg.level_info(inf.levels - 1).rows, "hierarchy shape");
  expect((double)total / (double)col.size() < 2.0, "operator complexity below 2");

  std::vector<double> hB((size_t)n * m);
  unsigned long long st = 12345;
  for (double &v : hB) st = st * 6364136223846793005ull + 1442695040888963407ull, v = (double)(st >> 11) / 9007199254740992.0 - 0.5;
  eigmi::DeviceMultiVector dB(ctx, n, m), dX(ctx, n, m);
  Flat fB{hB.data()};
  dB.upload(fB);
  double prev = 1.0;
  for (int cycles : {1, 4, 8})
  {
    const double r = mg.solve(dB, dX, cycles, true);
    std::printf("  %d cycle(s): residual %.3e\n", cycles, r);
    expect(r < prev, "the residual falls with the cycles");
    prev = r;
  }
  expect(prev < 1e-3, "eight cycles reduce the residual below 1e-3");
  {
    eigmi::Lobpcg s(K, nullptr, 8);
    s.precond_mg(mg, 1);
    int it = 0;
    std::vector<double> ev, res;
    expect(s.step(300, nev, 1e-8, &it), "LOBPCG with one AMG V-cycle converges");
    s.ritz(nev, ev, nullptr, &res);
    const double h = M_PI / (N + 1), exact = 3.0 * (2.0 - 2.0 * std::cos(h));
    std::printf("LOBPCG: %d iterations, lambda_1 %.15g (exact %.15g)\n", it, ev[0], exact);
    expect(std::fabs(ev[0] / exact - 1.0) <= 1e-10 && res[0] <= 1e-8 * ev[0], "smallest eigenvalue");
  }
  try
  {
    eigmi::Multigrid bad = eigmi::Multigrid::amg(K, 0.2);
    expect(false, "a theta above 1/6 must throw");
  }
  catch (const std::exception &e)
  {
    std::printf("refused: %s\n", e.what());
  }
  if (failures) return std::printf("%d FAILURES\n", failures), 1;
  std::printf("ALL OK\n");
  return 0;
}
