// Host-side unit checks of the Krylov drivers' host arithmetic (csrc/krylov_host.cpp, compiled with this file
// and csrc/dense.cpp).  No GPU and no library: plain host code.
//  * the sparse-pattern updates against literal values (scalar and 2 x 2 blocks, pattern(B) a strict subset,
//    alpha = 0, the two EIG_ERR_SHAPE errors with the caller's prefix);
//  * the ARPACK++ defaults;
//  * one extension column from a hand-made read-back row, and its breakdown test;
//  * the Arnoldi driver's Krylov-Schur restart on 12 x 12 upper-Hessenberg matrices of known spectrum
//    (2 x 2 rotation-scaling blocks and real 1 x 1 blocks under a dense upper triangle; two equal moduli).
#include <cstdio>
#include <cstring>
#include <set>
#include <string>

#include "../../dune-eigensolver_amd/csrc/krylov_host.h"

using namespace eigmi;
typedef std::complex<double> C;

static int failures = 0;
#define CHECK(cond)                                                   \
  do {                                                                \
    if (!(cond))                                                      \
    {                                                                 \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);   \
      ++failures;                                                     \
    }                                                                 \
  } while (0)

// runs f; returns the code and text of the eigmi::Error it threw ("" and EIG_OK: none)
template <class F>
static int thrown(F f, std::string &text)
{
  text.clear();
  try
  {
    f();
  }
  catch (const Error &e)
  {
    text = e.what();
    return e.code;
  }
  return EIG_OK;
}

// ---- pattern updates -------------------------------------------------------------------------------
static void test_pattern()
{
  std::string text;
  // 4-row scalar matrix, tridiagonal pattern; B: the diagonal and (1, 2), (3, 2)
  const HostCsr A0 = {{0, 2, 5, 8, 10}, {0, 1, 0, 1, 2, 1, 2, 3, 2, 3}, {4, -1, -1, 4, -1, -1, 4, -1, -1, 4}};
  const HostCsr B = {{0, 1, 3, 4, 6}, {0, 1, 2, 2, 2, 3}, {1, 2, 0.5, 3, 0.25, 4}};
  const HostCsr Bout = {{0, 1, 1, 1, 1}, {3}, {7.0}};  // stores (0, 3): outside A's pattern
  {
    HostCsr A = A0;
    pattern_axpy(0, 4, 1, A, -2.0, B, "who");
    CHECK((A.v == std::vector<double>{2, -1, -1, 0, -2, -1, -2, -1, -1.5, -4}));
    pattern_shift_diag(0, 4, 1, A, 0.5, "who");
    CHECK((A.v == std::vector<double>{2.5, -1, -1, 0.5, -2, -1, -1.5, -1, -1.5, -3.5}));
    // a row range touches its rows only
    A = A0;
    pattern_axpy(1, 2, 1, A, 1.0, B, "who");
    pattern_shift_diag(2, 4, 1, A, 1.0, "who");
    CHECK((A.v == std::vector<double>{4, -1, -1, 6, -0.5, -1, 5, -1, -1, 5}));
    // alpha = 0: untouched and unchecked
    A = A0;
    pattern_axpy(0, 4, 1, A, 0.0, Bout, "who");
    pattern_shift_diag(0, 4, 1, A, 0.0, "who");
    CHECK(A.v == A0.v && A.c == A0.c && A.rp == A0.rp);
    CHECK(thrown([&] { pattern_axpy(0, 4, 1, A, 1.0, Bout, "solver X"); }, text) == EIG_ERR_SHAPE);
    CHECK(text == "solver X: pattern(B) must be contained in pattern(A)");
    // row 2 without its diagonal entry
    HostCsr A2 = {{0, 2, 5, 7, 9}, {0, 1, 0, 1, 2, 1, 3, 2, 3}, std::vector<double>(9, 1.0)};
    CHECK(thrown([&] { pattern_shift_diag(0, 4, 1, A2, 1.0, "solver Y"); }, text) == EIG_ERR_SHAPE);
    CHECK(text == "solver Y: A has no diagonal entry");
  }
  {
    // 2 block rows, b = 2: A stores (0,0) (0,1) (1,0) (1,1), B only (0,0) and (1,1)
    HostCsr A = {{0, 2, 4}, {0, 1, 0, 1}, {1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16}};
    const HostCsr B2 = {{0, 1, 2}, {0, 1}, {1, 0.5, 0.25, 2, 4, 8, 16, 32}};
    pattern_axpy(0, 2, 2, A, 2.0, B2, "who");
    CHECK((A.v == std::vector<double>{3, 3, 3.5, 8, 5, 6, 7, 8, 9, 10, 11, 12, 21, 30, 47, 80}));
    pattern_shift_diag(0, 2, 2, A, -1.0, "who");
    CHECK((A.v == std::vector<double>{2, 3, 3.5, 7, 5, 6, 7, 8, 9, 10, 11, 12, 20, 30, 47, 79}));
    // block row 1 of B stores block column 0, block row 1 of this A does not
    HostCsr A1 = {{0, 2, 3}, {0, 1, 1}, std::vector<double>(12, 0.0)};
    const HostCsr B1 = {{0, 1, 2}, {0, 0}, B2.v};
    CHECK(thrown([&] { pattern_axpy(0, 2, 2, A1, 1.0, B1, "blk"); }, text) == EIG_ERR_SHAPE);
    CHECK(text == "blk: pattern(B) must be contained in pattern(A)");
  }
}

// ---- defaults --------------------------------------------------------------------------------------
static void test_defaults()
{
  CHECK(arpack_ncv(1000, 4, 0) == 20);    // max(2 nev + 1, 20)
  CHECK(arpack_ncv(1000, 12, 0) == 25);   // 2 nev + 1
  CHECK(arpack_ncv(16, 4, 0) == 16);      // capped by n
  CHECK(arpack_ncv(1000, 4, -3) == 20);
  CHECK(arpack_ncv(1000, 4, 11) == 11);   // given: kept
  CHECK(arpack_tol(0.0) == 2.220446049250313e-16);
  CHECK(arpack_tol(-1.0) == 2.220446049250313e-16);
  CHECK(arpack_tol(1e-9) == 1e-9);
  CHECK(arpack_maxit(7, 0) == 700);
  CHECK(arpack_maxit(7, -1) == 700);
  CHECK(arpack_maxit(7, 33) == 33);
  CHECK(thick_restart_size(12, 2) == 7 && thick_restart_size(12, 4) == 8 && thick_restart_size(12, 9) == 10);
  CHECK(thick_restart_size(20, 4) == 12);
  std::vector<int> ord;
  order_largest_magnitude(std::vector<double>{1.0, -3.0, 2.0, 3.0, -0.5}, ord);
  CHECK((ord == std::vector<int>{1, 3, 2, 0, 4}));  // equal moduli keep their order
  order_largest_magnitude(std::vector<C>{C(0, 1), C(3, 4), C(3, -4), C(-6, 0)}, ord);
  CHECK((ord == std::vector<int>{3, 1, 2, 0}));
}

// ---- one extension column ------------------------------------------------------------------------------
static void test_extension()
{
  const int m = 4;
  CHECK(extension_stride(m) == 11);
  // column j = 2: pass 1 at [0 .. 2], pass 2 at [5 .. 7], the squared norm at [10]; the other entries are
  // other columns' leftovers and must not be read
  const double row[11] = {1.0, -2.0, 0.5, 99.0, 99.0, 0.25, 0.0, -0.5, 99.0, 99.0, 6.25};
  std::vector<double> ctot(m + 1, 77.0);
  std::string text;
  const double beta = extension_column(m, 2, row, ctot, "unused");
  CHECK(beta == 2.5);
  CHECK((ctot == std::vector<double>{1.25, -2.0, 0.0, 0.0, 0.0}));
  // a negative squared norm (rounding) is beta = 0: a breakdown, as is beta <= 1e-14 max|c|
  double bad[11];
  std::memcpy(bad, row, sizeof bad);
  bad[10] = -1e-30;
  CHECK(thrown([&] { extension_column(m, 2, bad, ctot, "broke down"); }, text) == EIG_ERR_BREAKDOWN);
  CHECK(text == "broke down");
  bad[10] = 2e-14 * 2e-14;  // beta = 1e-14 max|c| exactly (max|c| = 2): not above
  CHECK(thrown([&] { extension_column(m, 2, bad, ctot, "broke down"); }, text) == EIG_ERR_BREAKDOWN);
  bad[10] = 2.1e-14 * 2.1e-14;
  CHECK(thrown([&] { extension_column(m, 2, bad, ctot, "broke down"); }, text) == EIG_OK);
}

// ---- Krylov-Schur restart ----------------------------------------------------------------------------------
// A unit of the spectrum: a real eigenvalue re (im = 0) or the pair re +- i im.
struct Unit {
  double re, im;
};
constexpr int kM = 12;
// max |G Z - Z Gn| / max |G| over the cases below, measured with the restart block as it stood inside
// arnoldi_core before it moved to krylov_host.cpp (bitwise the same Z, Gn and c there): 1.665e-16.  10 x that.
static const double kInvarianceBound = 1.665e-15;

// Upper Hessenberg, block upper triangular: the units' blocks on the diagonal ([re -im; im re] for a pair),
// a fixed dense fill above them.  Its eigenvalues are the units'.
static std::vector<double> hessenberg(const std::vector<Unit> &units)
{
  std::vector<double> G((size_t)kM * kM, 0.0);
  for (int i = 0; i < kM; ++i)
    for (int j = i + 1; j < kM; ++j) G[(size_t)i * kM + j] = 0.25 * ((7 * i + 3 * j) % 11 - 5) / 5.0;
  int r = 0;
  for (const Unit &u : units)
  {
    G[(size_t)r * kM + r] = u.re;
    if (u.im != 0.0)
    {
      G[(size_t)r * kM + r + 1] = -u.im;
      G[(size_t)(r + 1) * kM + r] = u.im;
      G[(size_t)(r + 1) * kM + r + 1] = u.re;
      ++r;
    }
    ++r;
  }
  return G;
}

// index of the unit an eigenvalue belongs to (nearest; pairs by either member)
static int unit_of(const std::vector<Unit> &units, C w)
{
  int best = -1;
  double d = 1e300;
  for (size_t u = 0; u < units.size(); ++u)
  {
    const double du = std::min(std::abs(w - C(units[u].re, units[u].im)), std::abs(w - C(units[u].re, -units[u].im)));
    if (du < d) d = du, best = (int)u;
  }
  return d < 1e-10 ? best : -1;
}

struct RestartResult {
  int kk = 0;
  std::vector<double> G0, G, cvec, Z;
  std::vector<std::pair<int, bool>> kept;
  std::vector<C> w, Y;
  std::vector<int> ord;
};

// the restart the Arnoldi driver runs after an extension to m = 12 vectors: eigenpairs of G, "LM" order, c = e_m
static RestartResult run_restart(const std::vector<Unit> &units, int nev)
{
  RestartResult r;
  r.G0 = r.G = hessenberg(units);
  r.cvec.assign(kM, 0.0);
  r.cvec[kM - 1] = 1.0;
  if (!gen_eig(kM, r.G, r.w, r.Y))
  {
    std::printf("FAILED: gen_eig\n");
    ++failures;
    return r;
  }
  order_largest_magnitude(r.w, r.ord);
  krylov_schur_restart(kM, nev, r.G, r.cvec, r.w, r.Y, r.ord, r.kk, r.Z, r.kept);
  return r;
}

// max |Z^T Z - I|
static double ortho_defect(const RestartResult &r)
{
  double e = 0.0;
  for (int p = 0; p < r.kk; ++p)
    for (int q = 0; q < r.kk; ++q)
    {
      double a = 0.0;
      for (int i = 0; i < kM; ++i) a += r.Z[(size_t)i * r.kk + p] * r.Z[(size_t)i * r.kk + q];
      e = std::max(e, std::fabs(a - (p == q ? 1.0 : 0.0)));
    }
  return e;
}

// max |G0 Z - Z Gn| / max |G0|
static double invariance_defect(const RestartResult &r)
{
  double gmax = 0.0, e = 0.0;
  for (double g : r.G0) gmax = std::max(gmax, std::fabs(g));
  for (int i = 0; i < kM; ++i)
    for (int q = 0; q < r.kk; ++q)
    {
      double a = 0.0;
      for (int l = 0; l < kM; ++l) a += r.G0[(size_t)i * kM + l] * r.Z[(size_t)l * r.kk + q];
      for (int p = 0; p < r.kk; ++p) a -= r.Z[(size_t)i * r.kk + p] * r.G[(size_t)p * kM + q];
      e = std::max(e, std::fabs(a));
    }
  return e / gmax;
}

// Spectrum 1, "LM" order: the pair of modulus 5 (columns 1-2), 4 (3), the pair of modulus 3 and the real -3
// (equal moduli: 4-6 in either order), 2.5 (7), the pair of modulus 2 (8-9), 1.5 (10), 1, 0.5.
static const std::vector<Unit> kSpec1 = {{1.5, 0.0}, {3.0, 4.0}, {-3.0, 0.0}, {0.5, 0.0}, {1.8, 2.4}, {4.0, 0.0},
                                         {1.0, 0.0}, {-1.2, 1.6}, {2.5, 0.0}};
// Spectrum 2: the pair of modulus 5 (1-2), 4 (3), the pair of modulus 3 and -3 (4-6), 2.5, 2.25, 2.125 (7-9),
// the pair of modulus 2 (10-11), 1.
static const std::vector<Unit> kSpec2 = {{2.125, 0.0}, {3.0, 4.0}, {-3.0, 0.0}, {2.25, 0.0}, {1.8, 2.4}, {4.0, 0.0},
                                         {1.0, 0.0}, {-1.2, 1.6}, {2.5, 0.0}};

struct RestartCase {
  const std::vector<Unit> *spec;
  int nev, kk;
  std::set<int> kept;  // indices into *spec
};
static const RestartCase kCases[] = {
    // target 7: whole units fill it exactly
    {&kSpec1, 2, 7, {1, 5, 4, 2, 8}},
    // target 8 falls between the two members of the modulus-2 pair (columns 8-9): the pair is kept whole
    {&kSpec1, 4, 9, {1, 5, 4, 2, 8, 7}},
    // target 10 = m - 2, reached by real values
    {&kSpec1, 9, 10, {1, 5, 4, 2, 8, 7, 0}},
    // target 10 and the modulus-2 pair arrives at kk = 9 = m - 3, the latest a unit can arrive (kk < target
    // <= m - 2): it is kept whole, kk = m - 1.  So "kk + 2 > m - 1" -- the guard that would drop a pair that
    // does not fit beside v_m -- cannot fire for any (m, nev): this is its boundary.
    {&kSpec2, 8, 11, {1, 5, 4, 2, 8, 3, 0, 7}},
    // target 8, reached by the real 2.25
    {&kSpec2, 4, 8, {1, 5, 4, 2, 8, 3}},
};

static void test_restart()
{
  for (const RestartCase &tc : kCases)
  {
    const RestartResult r = run_restart(*tc.spec, tc.nev);
    CHECK(r.kk == tc.kk);
    std::set<int> kept;
    int cols = 0;
    for (auto &u : r.kept)
    {
      const int id = unit_of(*tc.spec, r.w[u.first]);
      CHECK(id >= 0 && u.second == ((*tc.spec)[id].im != 0.0));
      kept.insert(id);
      cols += u.second ? 2 : 1;
    }
    CHECK(kept == tc.kept && cols == r.kk && kept.size() == r.kept.size());
    CHECK((int)r.Z.size() == kM * r.kk && (int)r.cvec.size() == r.kk && (int)r.G.size() == kM * kM);
    const double od = ortho_defect(r), id = invariance_defect(r);
    std::printf("restart nev=%d kk=%d  |Z^T Z - I| = %.3e  |G Z - Z Gn| / |G| = %.3e\n", tc.nev, r.kk, od, id);
    // MGS twice at m = 12 leaves a few ulps; one pass alone leaves the eigenvector basis's conditioning
    CHECK(od <= 1e-13);
    CHECK(id <= kInvarianceBound);
    // c = e_m: Z^T c is Z's last row; outside the leading kk x kk block the new G is zero
    for (int p = 0; p < r.kk; ++p) CHECK(r.cvec[p] == r.Z[(size_t)(kM - 1) * r.kk + p]);
    for (int i = 0; i < kM; ++i)
      for (int j = 0; j < kM; ++j)
        if (i >= r.kk || j >= r.kk) CHECK(r.G[(size_t)i * kM + j] == 0.0);
  }
}

int main()
{
  test_pattern();
  test_defaults();
  test_extension();
  test_restart();
  if (failures) return 1;
  std::printf("ALL OK\n");
  return 0;
}
