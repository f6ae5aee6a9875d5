// eigmi::Lobpcg (include/eigmi.hh) on the 2-D Laplacian 16 x 16: the four smallest eigenvalues against
// the analytic spectrum 4 - 2 cos(i pi / 17) - 2 cos(j pi / 17), and the facade's error mapping.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <vector>

#include "eigmi.hh"

int main()
{
  const int N = 16, nev = 4;
  std::vector<int64_t> rowptr(1, 0);
  std::vector<int32_t> col;
  std::vector<double> val;
  for (int k = 0; k < N * N; ++k)
  {
    const int x = k % N, y = k / N;
    auto put = [&](int c, double v) { col.push_back(c); val.push_back(v); };
    if (y > 0) put(k - N, -1);
    if (x > 0) put(k - 1, -1);
    put(k, 4);
    if (x < N - 1) put(k + 1, -1);
    if (y < N - 1) put(k + N, -1);
    rowptr.push_back((int64_t)col.size());
  }
  std::vector<double> exact;
  for (int i = 1; i <= N; ++i)
    for (int j = 1; j <= N; ++j) exact.push_back(4 - 2 * std::cos(i * M_PI / (N + 1)) - 2 * std::cos(j * M_PI / (N + 1)));
  std::sort(exact.begin(), exact.end());
  int failures = 0;
  eigmi::Context ctx(0);
  auto K = eigmi::Matrix::from_bcsr(ctx, rowptr, col, val);
  {
    eigmi::Lobpcg solver(K, nullptr, 8);
    solver.precond_cheb(4, 0.2, 2.0);
    int iters = 0;
    const bool conv = solver.step(200, nev, 1e-8, &iters);
    std::vector<double> lambda, res;
    solver.ritz(nev, lambda, nullptr, &res);
    std::printf("LOBPCG 16 x 16: %d iterations, converged %d\n", iters, (int)conv);
    if (!conv) ++failures;
    for (int i = 0; i < nev; ++i)
    {
      std::printf("  lambda %.15g (exact %.15g) residual %.2e\n", lambda[i], exact[i], res[i]);
      if (std::fabs(lambda[i] / exact[i] - 1) > 1e-10 || res[i] > 1e-8 * lambda[i]) ++failures;
    }
  }
  try  // a preconditioner at the largest end: EIG_ERR_ARG -> std::runtime_error
  {
    eigmi::Lobpcg la(K, nullptr, 8, EIG_WHICH_LA);
    la.precond_cheb(4, 0.2, 2.0);
    ++failures;
  }
  catch (const std::runtime_error &)
  {
  }
  if (failures) return std::printf("%d FAILURES\n", failures), 1;
  std::printf("ALL OK\n");
  return 0;
}
