// Stand-alone host test of csrc/subspace_host.cpp (with csrc/dense.cpp for sym_eig): the host arithmetic the
// block eigensolvers share -- Householder Q, LOBPCG's search coefficients, the small Rayleigh-Ritz pick, the
// block tridiagonal, the shift-invert Ritz order, the two convergence tests, the orthonormality deviation, the
// Chebyshev-Jacobi scalars, CholQR2's reuse test and the MultiVector column unpack.  No library and no GPU
// runtime; built plain and with ASan + UBSan by tests/test_subspace_host.py.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>

#include "../../dune-eigensolver_amd/csrc/subspace_host.h"

using namespace eigmi;
typedef std::vector<double> Vec;

static int fails = 0;
#define CHECK(cond)                                                  \
  do {                                                               \
    if (!(cond))                                                     \
    {                                                                \
      std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);    \
      ++fails;                                                       \
    }                                                                \
  } while (0)

// orthogonality and eigen-relation bound: about 5 N eps at N = 96
static const double kTol = 1e-13;

// uniform in [-1, 1), a fixed stream
static unsigned long long rng_state = 0x9E3779B97F4A7C15ull;
static double rnd()
{
  rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
  return (double)(rng_state >> 11) / 9007199254740992.0 * 2.0 - 1.0;
}
static Vec random_matrix(int N, int m)
{
  Vec A((size_t)N * m);
  for (double &v : A) v = rnd();
  return A;
}

// C (p x r) = A^T B for row-major A (N x p), B (N x r)
static Vec at_b(int N, int p, int r, const Vec &A, const Vec &B)
{
  Vec C((size_t)p * r, 0.0);
  for (int i = 0; i < N; ++i)
    for (int a = 0; a < p; ++a)
      for (int b = 0; b < r; ++b) C[(size_t)a * r + b] += A[(size_t)i * p + a] * B[(size_t)i * r + b];
  return C;
}
// C (N x r) = A B for row-major A (N x p), B (p x r)
static Vec a_b(int N, int p, int r, const Vec &A, const Vec &B)
{
  Vec C((size_t)N * r, 0.0);
  for (int i = 0; i < N; ++i)
    for (int a = 0; a < p; ++a)
      for (int b = 0; b < r; ++b) C[(size_t)i * r + b] += A[(size_t)i * p + a] * B[(size_t)a * r + b];
  return C;
}
static double max_diff(const Vec &A, const Vec &B)
{
  double d = A.size() == B.size() ? 0.0 : HUGE_VAL;
  for (size_t i = 0; i < A.size() && i < B.size(); ++i) d = std::max(d, std::fabs(A[i] - B[i]));
  return d;
}
// max |Q^T Q - I| of a row-major N x m matrix
static double orth_err(int N, int m, const Vec &Q) { return orth_deviation(m, at_b(N, m, m, Q, Q)); }
// max |Q Q^T A - A|: A (N x r) lies in the span of Q's columns
static double span_err(int N, int m, int r, const Vec &Q, const Vec &A)
{
  return max_diff(a_b(N, m, r, Q, at_b(N, m, r, Q, A)), A);
}
static Vec orthonormal(int N, int m)
{
  Vec A = random_matrix(N, m), Q;
  householder_q(N, m, A, Q);
  return Q;
}

static void test_householder_q()
{
  const int shapes[][2] = {{96, 8}, {96, 32}, {40, 8}, {33, 32}, {8, 8}, {32, 32}};
  for (auto &sh : shapes)
  {
    const int N = sh[0], m = sh[1];
    const Vec A0 = random_matrix(N, m);
    Vec A = A0, Q;
    householder_q(N, m, A, Q);
    CHECK((int)Q.size() == N * m);
    const double oe = orth_err(N, m, Q), se = span_err(N, m, m, Q, A0);
    std::printf("householder_q %2d x %2d: |Q^T Q - I| %.2e, |Q Q^T A - A| %.2e\n", N, m, oe, se);
    CHECK(oe <= kTol);
    CHECK(se <= kTol);
  }
  for (int m : {8, 32})
    for (int zc : {0, 3, m - 1})
    {
      // a zero column: no reflector there; column 0 of Q stays the unit vector e_0 exactly
      const int N = 3 * m;
      Vec A0 = random_matrix(N, m);
      for (int r = 0; r < N; ++r) A0[(size_t)r * m + zc] = 0.0;
      Vec A = A0, Q;
      householder_q(N, m, A, Q);
      CHECK(orth_err(N, m, Q) <= kTol);
      CHECK(span_err(N, m, m, Q, A0) <= kTol);
      if (zc == 0)
        for (int r = 0; r < N; ++r) CHECK(Q[(size_t)r * m] == (r == 0 ? 1.0 : 0.0));
    }
}

static void test_search_coefficients()
{
  for (int m : {8, 32})
    for (int kb : {2, 3})
    {
      const int N = kb * m;
      const Vec Cx = orthonormal(N, m);
      Vec C;
      search_coefficients(N, m, Cx, C);
      CHECK((int)C.size() == N * 2 * m);
      const double oe = orth_err(N, 2 * m, C);  // orthonormal columns, Cx^T Cp = 0 among them
      Vec Cp((size_t)N * m);
      for (int r = 0; r < N; ++r)
        for (int j = 0; j < m; ++j)
        {
          CHECK(C[(size_t)r * 2 * m + j] == Cx[(size_t)r * m + j]);
          Cp[(size_t)r * m + j] = C[(size_t)r * 2 * m + m + j];
        }
      const Vec cross = at_b(N, m, m, Cx, Cp);
      double ce = 0.0;
      for (double v : cross) ce = std::max(ce, std::fabs(v));
      // span(Cp) = span(Y), Y = (I - Cx Cx^T) Z with Z = Cx, X rows zeroed: each contains the other
      Vec Z = Cx;
      std::fill(Z.begin(), Z.begin() + (size_t)m * m, 0.0);
      Vec Y = Z;
      const Vec P = a_b(N, m, m, Cx, at_b(N, m, m, Cx, Z));
      for (size_t i = 0; i < Y.size(); ++i) Y[i] -= P[i];
      Vec Ycopy = Y, Qy;
      householder_q(N, m, Ycopy, Qy);
      const double s1 = span_err(N, m, m, Cp, Y), s2 = span_err(N, m, m, Qy, Cp);
      std::printf("search_coefficients N %2d m %2d: orth %.2e, Cx^T Cp %.2e, span %.2e / %.2e\n", N, m, oe, ce, s1, s2);
      CHECK(oe <= kTol);
      CHECK(ce <= kTol);
      CHECK(s1 <= kTol);
      CHECK(s2 <= kTol);
    }
}

static void test_ritz_select()
{
  const int shapes[][2] = {{24, 8}, {96, 32}};
  for (auto &sh : shapes)
  {
    const int N = sh[0], m = sh[1];
    // H = Q diag(d) Q^T with the known spectrum d_i = -1 + 2 i / (N - 1), placed in a scrambled order
    const Vec Q = orthonormal(N, N);
    Vec d(N), QD((size_t)N * N), Qt((size_t)N * N);
    for (int i = 0; i < N; ++i) d[(i * 7 + 3) % N] = -1.0 + 2.0 * i / (N - 1);  // (7 and N are coprime)
    for (int r = 0; r < N; ++r)
      for (int c = 0; c < N; ++c)
      {
        QD[(size_t)r * N + c] = Q[(size_t)r * N + c] * d[c];
        Qt[(size_t)c * N + r] = Q[(size_t)r * N + c];
      }
    const Vec H = a_b(N, N, N, QD, Qt);
    Vec sorted = d;
    std::sort(sorted.begin(), sorted.end());
    for (int which : {EIG_WHICH_SA, EIG_WHICH_LA})
    {
      Vec Hc = H, theta, Cx;
      ritz_select(N, Hc, m, which, theta, Cx);
      CHECK((int)theta.size() == m && (int)Cx.size() == N * m);
      double te = 0.0;
      for (int j = 0; j < m; ++j)
        te = std::max(te, std::fabs(theta[j] - (which == EIG_WHICH_SA ? sorted[j] : sorted[N - 1 - j])));
      Vec Hs = H;
      symmetrise(N, Hs);
      Vec HC = a_b(N, N, m, Hs, Cx), CT = Cx;
      for (int r = 0; r < N; ++r)
        for (int j = 0; j < m; ++j) CT[(size_t)r * m + j] *= theta[j];
      const double re = max_diff(HC, CT), oe = orth_err(N, m, Cx);
      std::printf("ritz_select N %2d m %2d %s: theta %.2e, H Cx - Cx theta %.2e, orth %.2e\n", N, m,
                  which == EIG_WHICH_SA ? "SA" : "LA", te, re, oe);
      CHECK(te <= kTol);
      CHECK(re <= kTol);
      CHECK(oe <= kTol);
      for (int j = 0; j + 1 < m; ++j) CHECK(which == EIG_WHICH_SA ? theta[j] < theta[j + 1] : theta[j] > theta[j + 1]);
    }
    // an unsymmetric perturbation H + E - E^T symmetrises back to H: entries on a 2^-30 grid, so every sum
    // below is exact and the two answers agree bit for bit
    Vec Hg = H, E = random_matrix(N, N);
    symmetrise(N, Hg);
    const double grid = 1073741824.0;
    for (double &v : Hg) v = std::nearbyint(v * grid) / grid;
    for (double &v : E) v = std::nearbyint(v * grid) / grid;
    Vec Hp = Hg;
    for (int r = 0; r < N; ++r)
      for (int c = 0; c < N; ++c) Hp[(size_t)r * N + c] = Hg[(size_t)r * N + c] + E[(size_t)r * N + c] - E[(size_t)c * N + r];
    CHECK(max_diff(Hp, Hg) > 0.1);
    Vec t0, C0, t1, C1;
    ritz_select(N, Hg, m, EIG_WHICH_SA, t0, C0);
    ritz_select(N, Hp, m, EIG_WHICH_SA, t1, C1);
    CHECK(t0 == t1);
    CHECK(C0 == C1);
  }
}

static void test_block_tridiag()
{
  for (int b : {8, 32})
  {
    // symmetric diagonal blocks; the off-diagonal blocks of k - 1 steps only, so a read of the last step's B
    // (or, k = 1, of any B) is out of bounds
    auto sym_block = [&](Vec &A) {
      Vec S = random_matrix(b, b);
      symmetrise(b, S);
      A.insert(A.end(), S.begin(), S.end());
    };
    {
      Vec A, B;
      sym_block(A);
      const Vec T = block_tridiag(b, 1, A, B);
      CHECK(T == A);
    }
    const int k = 3, N = k * b;
    Vec A, B = random_matrix((k - 1) * b, b);
    for (int j = 0; j < k; ++j) sym_block(A);
    const Vec T = block_tridiag(b, k, A, B);
    CHECK((int)T.size() == N * N);
    for (int r = 0; r < N; ++r)
      for (int c = 0; c < N; ++c)
      {
        const int jr = r / b, jc = c / b, ir = r % b, ic = c % b;
        double want = 0.0;
        if (jr == jc) want = A[((size_t)jr * b + ir) * b + ic];
        if (jr == jc + 1) want = B[((size_t)jc * b + ir) * b + ic];  // T_{j+1,j} = B_{j+1}
        if (jc == jr + 1) want = B[((size_t)jr * b + ic) * b + ir];  // T_{j,j+1} = B_{j+1}^T
        CHECK(T[(size_t)r * N + c] == want);
        CHECK(T[(size_t)r * N + c] == T[(size_t)c * N + r]);
      }
  }
}

static void test_si_ritz_order()
{
  // mixed signs, one exact zero, a tie in |th| (2 and -2: the stable sort keeps index 3 ahead of index 4)
  const Vec th0 = {0.5, -0.25, 0.0, 2.0, -2.0, 0.1, -4.0};
  const double sigma = 1.0;
  // |th| descending: 6, 3, 4, 0, 1, 5, 2;  lambda = sigma + 1 / th: 3, -3, inf, 1.5, 0.5, 11, 0.75
  struct Case {
    int nev, which;
    std::vector<int> want;
  } cases[] = {{5, EIG_WHICH_SA, {1, 4, 6, 3, 0}},
               {5, EIG_WHICH_LA, {0, 3, 6, 4, 1}},
               {2, EIG_WHICH_SA, {6, 3}},
               {2, EIG_WHICH_LA, {3, 6}},
               {7, EIG_WHICH_SA, {1, 4, 6, 3, 0, 5, 2}},
               {7, EIG_WHICH_LA, {2, 5, 0, 3, 6, 4, 1}}};
  for (const Case &c : cases)
  {
    Vec th = th0;
    std::vector<int> pick;
    si_ritz_order(th, sigma, c.nev, c.which, pick);
    CHECK(pick == c.want);
    CHECK(th[2] == HUGE_VAL);
    for (int i = 0; i < 7; ++i)
      if (i != 2) CHECK(th[i] == sigma + 1.0 / th0[i]);
  }
}

static void test_convergence()
{
  const double nan = std::numeric_limits<double>::quiet_NaN();
  {
    // ||r|| = 1 against tol |theta| ||M x|| = 0.25 * 2 * 2: the boundary counts as converged
    const int m = 8, nev = 3;
    const Vec theta(m, -2.0);
    Vec sums(2 * m, 4.0);
    for (int j = 0; j < m; ++j) sums[j] = 1.0;
    CHECK(lobpcg_converged(sums, theta, m, nev, 0.25));
    Vec s = sums;
    s[1] = 1.0 + 2.0 * std::numeric_limits<double>::epsilon();  // the smallest sum whose root exceeds 1
    CHECK(!lobpcg_converged(s, theta, m, nev, 0.25));
    s = sums;
    s[0] = nan;
    CHECK(!lobpcg_converged(s, theta, m, nev, 0.25));
    s = sums;
    s[m + 2] = nan;
    CHECK(!lobpcg_converged(s, theta, m, nev, 0.25));
    // only j < nev is looked at
    s = sums;
    s[nev] = nan;
    s[m - 1] = 1e30;
    s[m + nev] = nan;
    CHECK(lobpcg_converged(s, theta, m, nev, 0.25));
    CHECK(lobpcg_converged(s, theta, m, 0, 0.25));
  }
  {
    // window [0.4, 1]: columns 1, 2 (theta = 0.4: the edge is inside) are accepted; ||r|| = 1 against
    // tol max(|theta|, |a|, |b|) ||x|| = 0.5 * 1 * 2
    const double a = 0.4, b = 1.0, tol = 0.5;
    CHECK(window_accept(a, a, b) && window_accept(b, a, b) && window_accept(0.7, a, b));
    CHECK(!window_accept(std::nextafter(a, 0.0), a, b) && !window_accept(std::nextafter(b, 2.0), a, b));
    CHECK(!window_accept(nan, a, b));
    const Vec theta = {0.1, 0.4, 0.9, 1.5, 2.0, 2.5, 3.0, 3.5};
    const Vec rr(8, 1.0), xx(8, 4.0);
    CHECK(window_converged(theta, rr, xx, a, b, tol));
    Vec r = rr;
    r[2] = 1.0 + 2.0 * std::numeric_limits<double>::epsilon();
    CHECK(!window_converged(theta, r, xx, a, b, tol));
    r = rr;
    r[1] = nan;
    CHECK(!window_converged(theta, r, xx, a, b, tol));
    // only accepted columns are looked at
    r = rr;
    r[0] = nan;
    r[3] = 1e30;
    Vec x = xx;
    x[7] = nan;
    CHECK(window_converged(theta, r, x, a, b, tol));
    // an empty window never converges, nor does a workspace without residuals
    CHECK(!window_converged(theta, Vec(8, 0.0), xx, 10.0, 11.0, tol));
    CHECK(!window_converged(theta, Vec(), Vec(), a, b, tol));
  }
}

static void test_orth_deviation()
{
  const double nan = std::numeric_limits<double>::quiet_NaN();
  for (int N : {8, 32, 96})
  {
    Vec I((size_t)N * N, 0.0);
    for (int i = 0; i < N; ++i) I[(size_t)i * N + i] = 1.0;
    CHECK(orth_deviation(N, I) == 0.0);
    Vec G = I;
    G[(size_t)1 * N + 2] = -1e-3;
    CHECK(orth_deviation(N, G) == 1e-3);
    G[(size_t)(N - 1) * N + N - 1] = 1.25;
    CHECK(orth_deviation(N, G) == 0.25);
    for (size_t at : {(size_t)0, (size_t)N + 3, (size_t)N * N - 1})
    {
      Vec B = G;
      B[at] = nan;
      CHECK(orth_deviation(N, B) == HUGE_VAL);
    }
  }
}

static void test_cheb_jacobi()
{
  const double bounds[][2] = {{0.5, 2.5}, {0.2, 2.0}};
  for (auto &bd : bounds)
  {
    const double lmin = bd[0], lmax = bd[1];
    const ChebJacobi cj(lmin, lmax);
    CHECK(cj.gamma == 2.0 / (lmin + lmax));
    CHECK(cj.mu == (lmax - lmin) / (lmax + lmin));
    const double mu = cj.mu;
    double omega = cj.omega1();
    CHECK(omega == 1.0 / (1.0 - 0.5 * mu * mu));
    for (int k = 2; k <= 30; ++k)
    {
      const double next = cj.next(omega);
      CHECK(next == 1.0 / (1.0 - 0.25 * mu * mu * omega));
      omega = next;
    }
    const double limit = 2.0 / (1.0 + std::sqrt(1.0 - mu * mu));
    std::printf("ChebJacobi [%g, %g]: omega_30 - limit %.2e\n", lmin, lmax, omega - limit);
    CHECK(std::fabs(omega - limit) <= 1e-12);
  }
}

static void test_cholqr_reuse()
{
  for (int b : {8, 32})
  {
    Vec R((size_t)b * b, 7.0);  // (only the diagonal is looked at)
    for (int i = 0; i < b; ++i) R[(size_t)i * b + i] = 1.0;
    CHECK(cholqr_reuse(b, R));
    Vec S = R;
    S[(size_t)3 * b + 3] = kCholQrReuseCond;  // spread exactly 1e4: inside
    CHECK(cholqr_reuse(b, S));
    S[(size_t)3 * b + 3] = std::nextafter(kCholQrReuseCond, 2e4);  // just outside
    CHECK(!cholqr_reuse(b, S));
    S = R;
    S[(size_t)(b - 1) * b + b - 1] = 0.0;  // a zero pivot
    CHECK(!cholqr_reuse(b, S));
    S = R;
    S[0] = -3.0;  // a negative diagonal counts by its magnitude
    CHECK(cholqr_reuse(b, S));
    S[0] = -2e4;
    CHECK(!cholqr_reuse(b, S));
  }
  CHECK(kCholQrReuseCond == 1e4);
}

static void test_mv8_column()
{
  // three column blocks, ld > n, own > 0; out holds exactly n doubles
  const int64_t ld = 13, own = 3, n = 7;
  const int m = 24;
  Vec h((size_t)ld * m);
  for (size_t i = 0; i < h.size(); ++i) h[i] = 0.25 * (double)i - 11.0;
  for (int j : {0, 7, 8, 19, 23})
    for (double scale : {1.0, -0.5})
    {
      Vec out((size_t)n, 0.0);
      mv8_column(h.data(), ld, own, n, j, scale, out.data());
      for (int64_t r = 0; r < n; ++r) CHECK(out[(size_t)r] == scale * h[(size_t)(((j / 8) * ld + own + r) * 8 + j % 8)]);
    }
}

int main()
{
  test_householder_q();
  test_search_coefficients();
  test_ritz_select();
  test_block_tridiag();
  test_si_ritz_order();
  test_convergence();
  test_orth_deviation();
  test_cheb_jacobi();
  test_cholqr_reuse();
  test_mv8_column();
  if (fails == 0) std::printf("ALL OK\n");
  return fails == 0 ? 0 : 1;
}
