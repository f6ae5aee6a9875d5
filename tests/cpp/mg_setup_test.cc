// Host-side unit checks of the multigrid hierarchy setup (csrc/mg_setup.cpp, compiled with this file and
// csrc/dense.cpp alone).  No GPU and no library: plain host code.
//  (a) the blocked Galerkin operator on 66 x 9 x 17 (b = 3) and 17 x 40 x 12 (b = 4), every level down to the
//      coarsest: equal to an independent P^T A P (scattered entry by entry into a map, no stencil slots) to
//      1e-14 max|G|, bitwise symmetric, at most 27 blocks per row, ascending columns; the level grids are
//      17 x 40 x 12 -> 8 x 20 x 6 -> 4 x 10 x 3 -> 2 x 5 x 1;
//  (b) block Jacobi on every level: D^-1 D = I to 1e-13, D^-1 bitwise symmetric, the block Gershgorin bound >=
//      Rayleigh quotients of D^-1 A from a power iteration (each a lower bound of lambda_max) and, on the
//      coarsest level, >= the dense lambda_max of mg_spectrum_bounds; the coarse degree formula;
//  (c) b = 1: a literal coarse row of the scalar path (L_x + 2 L_y + 4 L_z on 7 x 5 x 6, exact dyadic values),
//      and the scalar Gershgorin bound;
//  (d) refusals: a diagonal block that is not positive definite (EIG_ERR_BREAKDOWN), a matrix that couples nodes
//      two steps apart (EIG_ERR_ARG); mg_coarsest_rows counts scalar rows.
#include <algorithm>
#include <array>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <map>
#include <utility>

#include "../../dune-eigensolver_amd/csrc/mg_setup.h"

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

template <class F>
static int thrown_code(F &&f)
{
  try
  {
    f();
  }
  catch (const Error &e)
  {
    return e.code;
  }
  return EIG_OK;
}

// a number in (0, 1) from three integers (fixed, no generator state)
static double hash01(i64 a, i64 b, i64 c)
{
  unsigned long long x = (unsigned long long)a * 0x9E3779B97F4A7C15ull + (unsigned long long)b * 0xC2B2AE3D27D4EB4Full +
                         (unsigned long long)c * 0x165667B19E3779F9ull + 0x27D4EB2F165667C5ull;
  x ^= x >> 29;
  x *= 0xBF58476D1CE4E5B9ull;
  x ^= x >> 32;
  return ((double)(x >> 11) + 0.5) / 9007199254740992.0;
}

// Symmetric blocked 27-point matrix on d[0] x d[1] x d[2] nodes: block (I, J), I < J, has general (unsymmetric)
// entries in (-1.5, -0.5) per edge, block (J, I) is its transpose, the diagonal block is symmetric and dominates
// its block row, so A is SPD.
static MgCsr box27(const int *d, int b)
{
  const int bb = b * b;
  const i64 n = (i64)d[0] * d[1] * d[2];
  MgCsr A;
  A.rp.assign(n + 1, 0);
  for (i64 I = 0; I < n; ++I)
  {
    const int X = (int)(I % d[0]), Y = (int)((I / d[0]) % d[1]), Z = (int)(I / ((i64)d[0] * d[1]));
    size_t diag = 0;
    std::vector<double> rowsum(b, 0.0);
    for (int s = 0; s < 27; ++s)
    {
      const int x = X + s % 3 - 1, y = Y + (s / 3) % 3 - 1, z = Z + s / 9 - 1;
      if (x < 0 || x >= d[0] || y < 0 || y >= d[1] || z < 0 || z >= d[2]) continue;
      const i64 J = ((i64)z * d[1] + y) * d[0] + x;
      A.col.push_back((i32)J);
      if (J == I) diag = A.val.size();
      for (int r = 0; r < b; ++r)
        for (int c = 0; c < b; ++c)
        {
          double v = 0.0;
          if (J != I)
          {
            v = I < J ? -0.5 - hash01(I, J, r * b + c) : -0.5 - hash01(J, I, c * b + r);
            rowsum[r] += std::fabs(v);
          }
          A.val.push_back(v);
        }
    }
    for (int r = 0; r < b; ++r)
      for (int c = 0; c < b; ++c)
        A.val[diag + r * b + c] = r == c ? rowsum[r] + 2.0 * b + hash01(I, I, r) : 0.5 + 0.4 * hash01(I, I, 100 + std::min(r, c) * b + std::max(r, c));
    A.rp[I + 1] = (i64)A.col.size();
    (void)bb;
  }
  return A;
}

// trilinear P column weights of fine node index f per direction: pairs (coarse, weight)
static int pcol(int f, int nc, int *c, double *w)
{
  int k = 0;
  if (f % 2 == 1)
  {
    c[k] = (f - 1) / 2, w[k++] = 1.0;
  }
  else
  {
    if (f / 2 - 1 >= 0) c[k] = f / 2 - 1, w[k++] = 0.5;
    if (f / 2 < nc) c[k] = f / 2, w[k++] = 0.5;
  }
  return k;
}

typedef std::map<std::pair<i64, i64>, std::array<double, 16>> BlockMap;

// P^T A P scattered entry by entry: for every stored fine block (i, j) and every pair of coarse nodes (I of i,
// J of j) G(I, J) += w_i w_j a
static BlockMap scatter_ptap(const MgCsr &A, int b, const int *fd, const int *cd)
{
  BlockMap G;
  const i64 n = (i64)fd[0] * fd[1] * fd[2];
  auto nodes = [&](i64 i, i64 *out, double *w) {
    const int x = (int)(i % fd[0]), y = (int)((i / fd[0]) % fd[1]), z = (int)(i / ((i64)fd[0] * fd[1]));
    int cx[2], cy[2], cz[2];
    double wx[2], wy[2], wz[2];
    const int kx = pcol(x, cd[0], cx, wx), ky = pcol(y, cd[1], cy, wy), kz = pcol(z, cd[2], cz, wz);
    int k = 0;
    for (int a = 0; a < kz; ++a)
      for (int c = 0; c < ky; ++c)
        for (int e = 0; e < kx; ++e) out[k] = ((i64)cz[a] * cd[1] + cy[c]) * cd[0] + cx[e], w[k++] = wz[a] * wy[c] * wx[e];
    return k;
  };
  for (i64 i = 0; i < n; ++i)
  {
    i64 Is[8], Js[8];
    double wi[8], wj[8];
    const int ki = nodes(i, Is, wi);
    for (i64 q = A.rp[i]; q < A.rp[i + 1]; ++q)
    {
      const int kj = nodes(A.col[q], Js, wj);
      for (int a = 0; a < ki; ++a)
        for (int c = 0; c < kj; ++c)
        {
          auto it = G.find({Is[a], Js[c]});
          if (it == G.end()) it = G.emplace(std::make_pair(Is[a], Js[c]), std::array<double, 16>{}).first;
          for (int e = 0; e < b * b; ++e) it->second[e] += wi[a] * wj[c] * A.val[(size_t)q * b * b + e];
        }
    }
  }
  return G;
}

static void mv(const MgCsr &A, i64 nb, int b, const std::vector<double> &x, std::vector<double> &y)
{
  y.assign((size_t)nb * b, 0.0);
  for (i64 I = 0; I < nb; ++I)
    for (i64 q = A.rp[I]; q < A.rp[I + 1]; ++q)
      for (int r = 0; r < b; ++r)
        for (int c = 0; c < b; ++c) y[I * b + r] += A.val[(size_t)q * b * b + r * b + c] * x[(size_t)A.col[q] * b + c];
}

static void check_level_jacobi(const MgCsr &A, i64 nb, int b, bool dense)
{
  const int bb = b * b;
  std::vector<double> dinv;
  const double bound = mg_block_jacobi(A, nb, b, dinv);
  CHECK(dinv.size() == (size_t)nb * bb);
  double worst = 0.0;
  bool sym = true;
  for (i64 I = 0; I < nb; ++I)
  {
    const double *D = nullptr;
    for (i64 q = A.rp[I]; q < A.rp[I + 1]; ++q)
      if (A.col[q] == I) D = &A.val[(size_t)q * bb];
    CHECK(D != nullptr);
    if (!D) return;
    for (int r = 0; r < b; ++r)
      for (int c = 0; c < b; ++c)
      {
        double s = 0.0;
        for (int k = 0; k < b; ++k) s += dinv[I * bb + r * b + k] * D[k * b + c];
        worst = std::max(worst, std::fabs(s - (r == c ? 1.0 : 0.0)));
        sym = sym && std::memcmp(&dinv[I * bb + r * b + c], &dinv[I * bb + c * b + r], sizeof(double)) == 0;
      }
  }
  CHECK(worst <= 1e-13);
  CHECK(sym);
  // power iteration on D^-1 A: every Rayleigh quotient x^T A x / x^T D x is a lower bound of lambda_max
  std::vector<double> x((size_t)nb * b), y, z(x.size());
  for (size_t i = 0; i < x.size(); ++i) x[i] = hash01((i64)i, 7, 11) - 0.5;
  double rq = 0.0;
  for (int it = 0; it < 60; ++it)
  {
    mv(A, nb, b, x, y);
    double xax = 0.0, nrm = 0.0;
    for (size_t i = 0; i < x.size(); ++i) xax += x[i] * y[i];
    for (i64 I = 0; I < nb; ++I)  // z = D^-1 y
      for (int r = 0; r < b; ++r)
      {
        double s = 0.0;
        for (int c = 0; c < b; ++c) s += dinv[I * bb + r * b + c] * y[I * b + c];
        z[I * b + r] = s;
      }
    // x^T D x = x^T A x at the previous step's scaling is not kept: recompute with D from D^-1 z = y, i.e.
    // x^T D x through the diagonal blocks
    double xdx = 0.0;
    for (i64 I = 0; I < nb; ++I)
      for (i64 q = A.rp[I]; q < A.rp[I + 1]; ++q)
        if (A.col[q] == I)
          for (int r = 0; r < b; ++r)
            for (int c = 0; c < b; ++c) xdx += x[I * b + r] * A.val[(size_t)q * bb + r * b + c] * x[I * b + c];
    rq = std::max(rq, xax / xdx);
    for (double v : z) nrm = std::max(nrm, std::fabs(v));
    for (size_t i = 0; i < x.size(); ++i) x[i] = z[i] / nrm;
  }
  std::printf("  level %lld nodes, b = %d: block Gershgorin bound %.6f, Rayleigh quotient %.6f", (long long)nb, b, bound,
              rq);
  CHECK(bound >= rq);
  CHECK(rq > 0.5);
  if (dense)
  {
    double lo, hi;
    mg_spectrum_bounds(A, nb, b, lo, hi);
    std::printf(", dense spectrum [%.6f, %.6f]", lo, hi);
    CHECK(lo > 0.0 && hi >= rq * (1.0 - 1e-12) && bound >= hi);
  }
  std::printf("\n");
}

static void check_hierarchy(const int *dims, int b, const std::vector<std::array<int, 3>> &expect)
{
  const int bb = b * b;
  int fd[3] = {dims[0], dims[1], dims[2]};
  MgCsr A = box27(fd, b);
  size_t level = 0;
  for (;; ++level)
  {
    CHECK(level < expect.size() && fd[0] == expect[level][0] && fd[1] == expect[level][1] && fd[2] == expect[level][2]);
    const i64 nf = (i64)fd[0] * fd[1] * fd[2];
    check_level_jacobi(A, nf, b, mg_last_level(fd));
    if (mg_last_level(fd)) break;
    int cd[3] = {fd[0] / 2, fd[1] / 2, fd[2] / 2};
    const i64 nc = (i64)cd[0] * cd[1] * cd[2];
    MgCsr C;
    mg_galerkin(A, b, fd, cd, C);
    CHECK((i64)C.rp.size() == nc + 1 && C.val.size() == C.col.size() * bb);
    BlockMap G = scatter_ptap(A, b, fd, cd);
    double gmax = 0.0, err = 0.0;
    for (auto &e : G)
      for (int t = 0; t < bb; ++t) gmax = std::max(gmax, std::fabs(e.second[t]));
    size_t seen = 0;
    bool ascending = true, symmetric = true;
    i64 widest = 0;
    for (i64 I = 0; I < nc; ++I)
    {
      widest = std::max(widest, C.rp[I + 1] - C.rp[I]);
      for (i64 q = C.rp[I]; q < C.rp[I + 1]; ++q)
      {
        const i64 J = C.col[q];
        if (q > C.rp[I]) ascending = ascending && C.col[q - 1] < J;
        auto it = G.find({I, J});
        if (it != G.end()) ++seen;
        for (int t = 0; t < bb; ++t) err = std::max(err, std::fabs(C.val[(size_t)q * bb + t] - (it != G.end() ? it->second[t] : 0.0)));
        // the transposed partner, bit for bit
        const i32 *lo = &C.col[C.rp[J]], *hi = &C.col[C.rp[J + 1]];
        const i32 *p = std::lower_bound(lo, hi, (i32)I);
        if (p == hi || *p != I)
        {
          symmetric = false;
          continue;
        }
        const double *tb = &C.val[(size_t)(p - &C.col[0]) * bb];
        for (int r = 0; r < b; ++r)
          for (int c = 0; c < b; ++c)
            symmetric = symmetric && std::memcmp(&C.val[(size_t)q * bb + r * b + c], &tb[c * b + r], sizeof(double)) == 0;
      }
    }
    std::printf("  %d x %d x %d -> %d x %d x %d (b = %d): max |Galerkin - scattered P^T A P| = %.3e, max|G| = %.3e\n", fd[0],
                fd[1], fd[2], cd[0], cd[1], cd[2], b, err, gmax);
    CHECK(err <= 1e-14 * gmax);
    CHECK(seen == G.size());  // every block of P^T A P is stored
    CHECK(ascending && symmetric && widest <= 27);
    A = std::move(C);
    for (int k = 0; k < 3; ++k) fd[k] = cd[k];
  }
  CHECK(level + 1 == expect.size());
  CHECK(mg_coarsest_rows(dims[0], dims[1], dims[2], b) == (i64)fd[0] * fd[1] * fd[2] * b);
}

static void check_scalar_literal()
{
  // A = L_x + 2 L_y + 4 L_z (L = tridiag(-1, 2, -1)) on 7 x 5 x 6 -> 3 x 2 x 3; coarse row 13 = node (1, 0, 2)
  const int fd[3] = {7, 5, 6}, cd[3] = {3, 2, 3};
  MgCsr A;
  const i64 n = 7 * 5 * 6;
  A.rp.assign(n + 1, 0);
  for (i64 i = 0; i < n; ++i)
  {
    const int x = (int)(i % 7), y = (int)((i / 7) % 5), z = (int)(i / 35);
    const int off[7] = {-35, -7, -1, 0, 1, 7, 35};
    const double v[7] = {-4.0, -2.0, -1.0, 14.0, -1.0, -2.0, -4.0};
    const bool ok[7] = {z > 0, y > 0, x > 0, true, x < 6, y < 4, z < 5};
    for (int k = 0; k < 7; ++k)
      if (ok[k]) A.col.push_back((i32)(i + off[k])), A.val.push_back(v[k]);
    A.rp[i + 1] = (i64)A.col.size();
  }
  MgCsr C;
  mg_galerkin(A, 1, fd, cd, C);
  const i32 cols[12] = {6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17};
  const double vals[12] = {-0.8125, -3.375, -0.8125, -0.21875, -1.0625, -0.21875,
                           1.9375,  19.125, 1.9375,  -0.09375, 0.6875,  -0.09375};
  CHECK(C.rp.size() == 19 && C.rp[14] - C.rp[13] == 12);
  if (C.rp.size() == 19 && C.rp[14] - C.rp[13] == 12)
    for (int k = 0; k < 12; ++k) CHECK(C.col[C.rp[13] + k] == cols[k] && C.val[C.rp[13] + k] == vals[k]);
  // fine Gershgorin: an interior row has (4 + 4 + 2 + 2 + 1 + 1 + 14) / 14
  CHECK(mg_gershgorin(A, n) == 28.0 / 14.0);
  double lo, hi;
  mg_spectrum_bounds(C, 18, 1, lo, hi);
  CHECK(lo > 0.0 && hi < mg_gershgorin(C, 18) * (1.0 + 1e-12));
  CHECK(mg_coarse_degree(1.0, 1.0) == 1 && mg_coarse_degree(1e-9, 1.0) == 2000);
  // kappa = 9: rho = 1 / 2, ceil(log(0.5e-15) / log(0.5)) = 51
  CHECK(mg_coarse_degree(1.0, 9.0) == 51);
}

static void check_refusals()
{
  const int d[3] = {5, 4, 3};
  MgCsr A = box27(d, 2);
  std::vector<double> dinv;
  for (i64 q = A.rp[7]; q < A.rp[8]; ++q)
    if (A.col[q] == 7)
    {
      const double bad[4] = {1.0, 2.0, 2.0, 1.0};  // eigenvalues 3 and -1
      std::copy(bad, bad + 4, &A.val[(size_t)q * 4]);
    }
  CHECK(thrown_code([&] { mg_block_jacobi(A, 60, 2, dinv); }) == EIG_ERR_BREAKDOWN);
  double lo, hi;
  CHECK(thrown_code([&] { mg_spectrum_bounds(A, 60, 2, lo, hi); }) == EIG_ERR_BREAKDOWN);
  MgCsr S;  // scalar: a zero diagonal entry
  S.rp = {0, 1, 2};
  S.col = {0, 1};
  S.val = {1.0, 0.0};
  CHECK(thrown_code([&] { mg_gershgorin(S, 2); }) == EIG_ERR_BREAKDOWN);
  // nodes two steps apart in x on 9 x 3 x 3
  const int f[3] = {9, 3, 3}, c[3] = {4, 1, 1};
  MgCsr T;
  T.rp.assign(82, 0);
  for (i64 i = 0; i < 81; ++i)
  {
    if (i % 9 >= 2) T.col.push_back((i32)(i - 2)), T.val.insert(T.val.end(), {-1.0, 0.0, 0.0, -1.0});
    T.col.push_back((i32)i), T.val.insert(T.val.end(), {4.0, 1.0, 1.0, 4.0});
    if (i % 9 < 7) T.col.push_back((i32)(i + 2)), T.val.insert(T.val.end(), {-1.0, 0.0, 0.0, -1.0});
    T.rp[i + 1] = (i64)T.col.size();
  }
  MgCsr C;
  CHECK(thrown_code([&] { mg_galerkin(T, 2, f, c, C); }) == EIG_ERR_ARG);
  const int flat[3] = {256, 256, 4};
  CHECK(mg_coarsest_rows(flat[0], flat[1], flat[2], 3) == 128 * 128 * 2 * 3);
  CHECK(mg_coarsest_rows(64, 64, 64, 3) == 4 * 4 * 4 * 3);
}

int main()
{
  const int g1[3] = {66, 9, 17}, g2[3] = {17, 40, 12};
  std::printf("(a, b) 66 x 9 x 17, b = 3\n");
  check_hierarchy(g1, 3, {{66, 9, 17}, {33, 4, 8}, {16, 2, 4}});
  std::printf("(a, b) 17 x 40 x 12, b = 4\n");
  check_hierarchy(g2, 4, {{17, 40, 12}, {8, 20, 6}, {4, 10, 3}, {2, 5, 1}});
  std::printf("(c) scalar path\n");
  check_scalar_literal();
  std::printf("(d) refusals\n");
  check_refusals();
  if (failures) std::printf("%d check(s) FAILED\n", failures);
  else std::printf("ALL OK\n");
  return failures ? 1 : 0;
}
