// Host-side unit checks of the smoothed-aggregation AMG setup (csrc/amg_setup.cpp, compiled with this file,
// csrc/mg_setup.cpp and csrc/dense.cpp alone).  No GPU and no library: plain host code.
//  (a) aggregation on a 6 x 5 x 4 7-point grid, a 40-row random SPD pattern and every level of a 16 x 12 x 10
//      hierarchy: every row in exactly one aggregate, no aggregate empty, every member of an aggregate of two or
//      more rows has a strong neighbour inside it; a row without strong neighbours is a singleton;
//  (b) P against an independent dense (I - omega D^-1 A) T (1e-15), ascending columns, no stored zero; P^T's CSR
//      is the transpose of P's, values bitwise;
//  (c) A_c against P^T A P scattered entry by entry into a dense array (1e-14 max|A_c|), bitwise symmetric,
//      ascending columns;
//  (d) the hierarchy's stopping rule and the refusals: theta above the 7-point strength 1/6 on 1728 rows is
//      EIG_ERR_ARG with the sizes in the message (and returns), a non-positive diagonal entry EIG_ERR_BREAKDOWN,
//      a level of <= 256 rows is a one-level hierarchy.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>

#include "../../dune-eigensolver_amd/csrc/amg_setup.h"

using namespace eigmi;

static int failures = 0;
#define CHECK(cond)                                                   \
  do {                                                                \
    if (!(cond))                                                      \
    {                                                                 \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);   \
      ++failures;                                                     \
    }                                                                 \
  } while (0)

static double hash01(i64 a, i64 b, i64 c)
{
  unsigned long long x = (unsigned long long)a * 0x9E3779B97F4A7C15ull + (unsigned long long)b * 0xC2B2AE3D27D4EB4Full +
                         (unsigned long long)c * 0x165667B19E3779F9ull + 0x27D4EB2F165667C5ull;
  x ^= x >> 29;
  x *= 0xBF58476D1CE4E5B9ull;
  x ^= x >> 32;
  return ((double)(x >> 11) + 0.5) / 9007199254740992.0;
}

// 7-point matrix on nx x ny x nz: off-diagonals -w(edge), w = 1 (vary = false) or in (0.5, 1.5); diagonal = the sum
// of the six face weights (Dirichlet boundary: the missing neighbours' weights stay in the diagonal)
static MgCsr grid7(int nx, int ny, int nz, bool vary)
{
  const i64 n = (i64)nx * ny * nz;
  MgCsr A;
  A.rp.assign(n + 1, 0);
  const int off[6][3] = {{0, 0, -1}, {0, -1, 0}, {-1, 0, 0}, {1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
  for (i64 i = 0; i < n; ++i)
  {
    const int x = (int)(i % nx), y = (int)((i / nx) % ny), z = (int)(i / ((i64)nx * ny));
    double diag = 0.0;
    double w[6];
    i64 nb[6];
    for (int s = 0; s < 6; ++s)
    {
      const int X = x + off[s][0], Y = y + off[s][1], Z = z + off[s][2];
      const bool in = X >= 0 && X < nx && Y >= 0 && Y < ny && Z >= 0 && Z < nz;
      nb[s] = in ? ((i64)Z * ny + Y) * nx + X : -1;
      w[s] = vary && in ? 0.5 + hash01(std::min(i, nb[s]), std::max(i, nb[s]), 7) : 1.0;
      diag += w[s];
    }
    for (int s = 0; s < 3; ++s)
      if (nb[s] >= 0) A.col.push_back((i32)nb[s]), A.val.push_back(-w[s]);
    A.col.push_back((i32)i), A.val.push_back(diag);
    for (int s = 3; s < 6; ++s)
      if (nb[s] >= 0) A.col.push_back((i32)nb[s]), A.val.push_back(-w[s]);
    A.rp[i + 1] = (i64)A.col.size();
  }
  return A;
}

// n-row random symmetric pattern (each pair with probability ~p), off-diagonals in (-1.5, 0.5) of either sign,
// strictly diagonally dominant, so SPD; row `lonely` (if >= 0) has its diagonal only
static MgCsr random_spd(i64 n, double p, i64 lonely)
{
  std::vector<double> D((size_t)n * n, 0.0);
  for (i64 i = 0; i < n; ++i)
    for (i64 j = i + 1; j < n; ++j)
      if (i != lonely && j != lonely && hash01(i, j, 1) < p) D[i * n + j] = D[j * n + i] = 0.5 - 2.0 * hash01(i, j, 2);
  MgCsr A;
  A.rp.assign(n + 1, 0);
  for (i64 i = 0; i < n; ++i)
  {
    double s = 0.0;
    for (i64 j = 0; j < n; ++j) s += std::fabs(D[i * n + j]);
    D[i * n + i] = s + 0.25 + hash01(i, i, 3);
    for (i64 j = 0; j < n; ++j)
      if (D[i * n + j] != 0.0) A.col.push_back((i32)j), A.val.push_back(D[i * n + j]);
    A.rp[i + 1] = (i64)A.col.size();
  }
  return A;
}

static std::vector<double> dense(const MgCsr &A, i64 nr, i64 nc)
{
  std::vector<double> D((size_t)nr * nc, 0.0);
  for (i64 i = 0; i < nr; ++i)
    for (i64 k = A.rp[i]; k < A.rp[i + 1]; ++k) D[i * nc + A.col[k]] = A.val[k];
  return D;
}

static bool ascending(const MgCsr &A, i64 nr, i64 nc)
{
  for (i64 i = 0; i < nr; ++i)
    for (i64 k = A.rp[i]; k < A.rp[i + 1]; ++k)
      if (A.col[k] < 0 || A.col[k] >= nc || (k > A.rp[i] && A.col[k - 1] >= A.col[k])) return false;
  return true;
}

static void check_aggregates(const MgCsr &A, i64 n, double theta, const std::vector<i64> &agg, i64 na)
{
  CHECK((i64)agg.size() == n && na >= 1 && na <= n);
  std::vector<i64> size(na, 0);
  bool in_range = true;
  for (i64 i = 0; i < n; ++i)
  {
    if (agg[i] < 0 || agg[i] >= na)
      in_range = false;
    else
      ++size[agg[i]];
  }
  CHECK(in_range);
  if (!in_range) return;
  CHECK(*std::min_element(size.begin(), size.end()) >= 1);
  const std::vector<double> D = dense(A, n, n);
  i64 loose = 0, lonely_grouped = 0;
  for (i64 i = 0; i < n; ++i)
  {
    bool any = false, inside = false;
    for (i64 k = A.rp[i]; k < A.rp[i + 1]; ++k)
    {
      const i64 j = A.col[k];
      if (j == i || !(std::fabs(A.val[k]) >= theta * std::sqrt(D[i * n + i] * D[j * n + j]))) continue;
      any = true;
      inside = inside || agg[j] == agg[i];
    }
    if (size[agg[i]] > 1 && !inside) ++loose;
    if (!any && size[agg[i]] != 1) ++lonely_grouped;
  }
  CHECK(loose == 0);
  CHECK(lonely_grouped == 0);
}

// P, P^T and A_c of one level against independent dense computations
static void check_level(const MgCsr &A, i64 n, double theta, const char *what)
{
  std::vector<i64> agg;
  const i64 nc = amg_aggregate(n, A.rp.data(), A.col.data(), A.val.data(), theta, agg);
  check_aggregates(A, n, theta, agg, nc);
  const double lmax = mg_gershgorin(A, n), omega = 4.0 / (3.0 * lmax);
  MgCsr P, PT, Ac;
  amg_prolongator(A, n, agg, nc, lmax, P);
  amg_transpose(P, n, nc, PT);
  amg_galerkin(A, P, PT, n, nc, Ac);
  const std::vector<double> Ad = dense(A, n, n), Pd = dense(P, n, nc), PTd = dense(PT, nc, n), Acd = dense(Ac, nc, nc);
  CHECK(ascending(P, n, nc) && ascending(PT, nc, n) && ascending(Ac, nc, nc));
  CHECK(std::find(P.val.begin(), P.val.end(), 0.0) == P.val.end());
  CHECK(P.col.size() == PT.col.size());
  // (b) P = (I - omega D^-1 A) T, dense
  double perr = 0.0;
  std::vector<double> s(nc);
  for (i64 i = 0; i < n; ++i)
  {
    std::fill(s.begin(), s.end(), 0.0);
    for (i64 j = 0; j < n; ++j) s[agg[j]] += Ad[i * n + j];  // row i of A T, every column of the dense row
    for (i64 J = 0; J < nc; ++J)
    {
      const double ref = (agg[i] == J ? 1.0 : 0.0) - omega * s[J] / Ad[i * n + i];
      perr = std::max(perr, std::fabs(ref - Pd[i * nc + J]));
    }
  }
  CHECK(perr <= 1e-15);
  bool tr = true;
  for (i64 i = 0; i < n; ++i)
    for (i64 J = 0; J < nc; ++J) tr = tr && std::memcmp(&Pd[i * nc + J], &PTd[J * n + i], sizeof(double)) == 0;
  CHECK(tr);
  // (c) A_c = P^T A P, scattered entry by entry
  std::vector<double> G((size_t)nc * nc, 0.0);
  for (i64 i = 0; i < n; ++i)
    for (i64 k = A.rp[i]; k < A.rp[i + 1]; ++k)
      for (i64 a = P.rp[i]; a < P.rp[i + 1]; ++a)
        for (i64 b = P.rp[A.col[k]]; b < P.rp[A.col[k] + 1]; ++b)
          G[(size_t)P.col[a] * nc + P.col[b]] += P.val[a] * A.val[k] * P.val[b];
  double gmax = 0.0, gerr = 0.0;
  bool sym = true;
  for (i64 I = 0; I < nc; ++I)
    for (i64 J = 0; J < nc; ++J)
    {
      gmax = std::max(gmax, std::fabs(Acd[I * nc + J]));
      gerr = std::max(gerr, std::fabs(Acd[I * nc + J] - G[I * nc + J]));
      sym = sym && std::memcmp(&Acd[I * nc + J], &Acd[J * nc + I], sizeof(double)) == 0;
    }
  CHECK(gerr <= 1e-14 * gmax);
  CHECK(sym);
  std::printf("%s: %lld rows -> %lld aggregates, |P - dense| %.1e, |A_c - P^T A P| / max|A_c| %.1e\n", what, (long long)n,
              (long long)nc, perr, gerr / gmax);
}

template <class F>
static int thrown_code(F &&f, std::string *msg = nullptr)
{
  try
  {
    f();
  }
  catch (const Error &e)
  {
    if (msg) *msg = e.what();
    return e.code;
  }
  return EIG_OK;
}

int main()
{
  check_level(grid7(6, 5, 4, false), 120, 0.08, "7-point 6 x 5 x 4");
  check_level(grid7(6, 5, 4, true), 120, 0.08, "7-point 6 x 5 x 4, varying");
  check_level(random_spd(40, 0.15, 17), 40, 0.08, "random SPD, 40 rows");
  check_level(random_spd(40, 0.15, -1), 40, 0.3, "random SPD, 40 rows, theta 0.3");

  // a whole hierarchy (the products run on several threads at 1920 rows): every level checked as above
  {
    AmgHierarchy H;
    amg_build(grid7(16, 12, 10, true), 1920, 0.08, H);
    CHECK(H.A.size() >= 2 && H.P.size() + 1 == H.A.size() && H.PT.size() == H.P.size() && H.rows.size() == H.A.size());
    CHECK(H.rows.back() <= 1024 && H.cdeg >= 1 && H.clo > 0.0 && H.chi > H.clo);
    for (size_t l = 0; l + 1 < H.A.size(); ++l)
    {
      CHECK(2 * H.rows[l + 1] <= H.rows[l] && H.rows[l] > kAmgCoarsestRows);
      // the level's own products are those of the stand-alone calls, bitwise
      std::vector<i64> agg;
      const double th = 0.08 * std::ldexp(1.0, -(int)l);
      const i64 nc = amg_aggregate(H.rows[l], H.A[l].rp.data(), H.A[l].col.data(), H.A[l].val.data(), th, agg);
      CHECK(nc == H.rows[l + 1]);
      MgCsr P;
      amg_prolongator(H.A[l], H.rows[l], agg, nc, H.lmax[l], P);
      CHECK(P.rp == H.P[l].rp && P.col == H.P[l].col && P.val == H.P[l].val);
      check_level(H.A[l], H.rows[l], th, "16 x 12 x 10 hierarchy level");
    }
    std::printf("hierarchy:");
    for (i64 r : H.rows) std::printf(" %lld", (long long)r);
    std::printf(", coarse degree %d\n", H.cdeg);
  }
  // <= 256 rows: one level
  {
    AmgHierarchy H;
    amg_build(grid7(6, 5, 4, false), 120, 0.08, H);
    CHECK(H.A.size() == 1 && H.P.empty() && H.cdeg >= 1);
  }
  // theta above the 7-point strength 1/6: no strong entry, 1728 singletons, refused (and returns)
  {
    AmgHierarchy H;
    std::string msg;
    CHECK(thrown_code([&] { amg_build(grid7(12, 12, 12, false), 1728, 0.25, H); }, &msg) == EIG_ERR_ARG);
    CHECK(msg.find("1728 -> 1728") != std::string::npos);
    // the same level at <= 1024 rows becomes the coarsest instead
    CHECK(thrown_code([&] { amg_build(grid7(10, 10, 10, false), 1000, 0.25, H); }) == EIG_OK && H.A.size() == 1);
  }
  // a non-positive diagonal entry
  {
    MgCsr A = grid7(8, 8, 8, false);
    for (i64 k = A.rp[100]; k < A.rp[101]; ++k)
      if (A.col[k] == 100) A.val[k] = -6.0;
    AmgHierarchy H;
    std::vector<i64> agg;
    CHECK(thrown_code([&] { amg_build(A, 512, 0.08, H); }) == EIG_ERR_BREAKDOWN);
    CHECK(thrown_code([&] { amg_aggregate(512, A.rp.data(), A.col.data(), A.val.data(), 0.08, agg); }) == EIG_ERR_BREAKDOWN);
    CHECK(thrown_code([&] { amg_build(grid7(8, 8, 8, false), 512, -0.1, H); }) == EIG_ERR_ARG);
  }
  if (failures)
  {
    std::printf("%d FAILURES\n", failures);
    return 1;
  }
  std::printf("ALL OK\n");
  return 0;
}
