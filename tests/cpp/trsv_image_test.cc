// Host-side unit checks of the triangular-solve images (csrc/trsv_image.cpp, compiled with this file alone).
// No GPU and no library: plain host code.  Expectations are literal or exact: every value is a power of two or
// a single product of powers of two.
//  (a) factor_rows: L rows ascending without the unit diagonal, U rows descending without the pivot, ud, and
//      the two argument errors;
//  (b) row_splits against the brute-force definition for n = 1, 63, 64, 65, 130;
//  (c) the staged admission at its edges (kSlab / kSlab + 1 outside entries, kRing4 / kRing4 + 1 blocks away),
//      once in L and once in U;
//  (d) the coupled-block distances and the block-inverse admission (gd 8 / 9, a zero pivot, the tile cap);
//  (e) the block-inverse tiles of bidiagonal blocks against their closed forms, ragged last block;
//  (f) the conditioning gate at 2^-13 / 2^-14 and on a NaN entry;
//  (g) a 4-thread build equals the 1-thread build bit for bit, and refuses an ill-conditioned block;
//  (h) the staged image read back by its layout rule, rows of 0, 1, 127, 128 outside entries, 129 refused;
//  (i) export_envelope on a 5 x 5 envelope with an exact zero inside it.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <utility>

#include "../../dune-eigensolver_amd/csrc/trsv_image.h"

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

template <class T>
static bool same_bits(const std::vector<T> &a, const std::vector<T> &b)
{
  return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(T)) == 0);
}

// true when f() throws eigmi::Error with EIG_ERR_ARG
template <class F>
static bool throws_arg(F &&f)
{
  try
  {
    f();
  }
  catch (const Error &e)
  {
    return e.code == EIG_ERR_ARG;
  }
  return false;
}

// Factors row by row: L row i lists (column, value) ascending, U row i descending; pivots 1 unless set.
typedef std::vector<std::vector<std::pair<i32, double>>> RowList;
struct Factors {
  i64 n;
  RowList l, u;
  std::vector<double> ud;
  explicit Factors(i64 n_) : n(n_), l(n_), u(n_), ud(n_, 1.0) {}
  FactorRows rows() const
  {
    FactorRows R;
    R.lrp.assign(1, 0);
    R.urp.assign(1, 0);
    for (i64 i = 0; i < n; ++i)
    {
      for (auto &e : l[i])
      {
        R.lc.push_back(e.first);
        R.lv.push_back(e.second);
      }
      for (auto &e : u[i])
      {
        R.uc.push_back(e.first);
        R.uv.push_back(e.second);
      }
      R.lrp.push_back((i64)R.lc.size());
      R.urp.push_back((i64)R.uc.size());
    }
    R.ud = ud;
    return R;
  }
  TrsvPlan plan() const
  {
    const FactorRows R = rows();
    return trsv_plan(n, R, row_splits(n, R));
  }
};

// ---- (a) ------------------------------------------------------------------------------------------------------
static void test_factor_rows()
{
  // L rows (unit diagonal last), row 3 stored in descending order; U columns (pivot last), column 3 shuffled
  std::vector<i64> Lp = {0, 1, 3, 5, 9, 11}, Lj = {0, 0, 1, 1, 2, 2, 1, 0, 3, 3, 4};
  std::vector<double> Lx = {1, 0.5, 1, 0.25, 1, 2, 8, 4, 1, 0.125, 1};
  std::vector<i64> Up = {0, 1, 3, 5, 9, 12}, Ui = {0, 0, 1, 1, 2, 2, 0, 1, 3, 3, 0, 4};
  std::vector<double> Ux = {2, 3, 4, 5, 8, 6, 7, 9, 16, 10, 11, 32};
  const FactorRows R = factor_rows(5, Lp, Lj, Lx, Up, Ui, Ux);
  CHECK((R.lrp == std::vector<i64>{0, 0, 1, 2, 5, 6}));
  CHECK((R.lc == std::vector<i32>{0, 1, 0, 1, 2, 3}));
  CHECK((R.lv == std::vector<double>{0.5, 0.25, 4, 8, 2, 0.125}));
  CHECK((R.urp == std::vector<i64>{0, 3, 5, 6, 7, 7}));
  CHECK((R.uc == std::vector<i32>{4, 3, 1, 3, 2, 3, 4}));
  CHECK((R.uv == std::vector<double>{11, 7, 3, 9, 5, 6, 10}));
  CHECK((R.ud == std::vector<double>{2, 4, 8, 16, 32}));
  {
    std::vector<i64> Lj2 = Lj;
    Lj2[1] = 1;  // row 1: an entry on the diagonal before the unit diagonal
    CHECK(throws_arg([&] { factor_rows(5, Lp, Lj2, Lx, Up, Ui, Ux); }));
    Lj2[1] = 3;  // above it
    CHECK(throws_arg([&] { factor_rows(5, Lp, Lj2, Lx, Up, Ui, Ux); }));
  }
  {
    // column 2 empty
    std::vector<i64> Up2 = {0, 1, 3, 3, 7, 10}, Ui2 = {0, 0, 1, 2, 0, 1, 3, 3, 0, 4};
    std::vector<double> Ux2 = {2, 3, 4, 6, 7, 9, 16, 10, 11, 32};
    CHECK(throws_arg([&] { factor_rows(5, Lp, Lj, Lx, Up2, Ui2, Ux2); }));
  }
}

// ---- (b) ------------------------------------------------------------------------------------------------------
static void test_row_splits()
{
  const i64 offs[] = {70, 64, 63, 5, 1};
  for (i64 n : {1, 63, 64, 65, 130})
  {
    Factors F(n);
    for (i64 i = 0; i < n; ++i)
      for (i64 d : offs)
      {
        if (i - d >= 0) F.l[i].push_back({(i32)(i - d), 1.0});  // ascending
        if (i + d < n) F.u[i].push_back({(i32)(i + d), 1.0});   // descending
      }
    const FactorRows R = F.rows();
    const RowSplits S = row_splits(n, R);
    CHECK((i64)S.ls.size() == n && (i64)S.us.size() == n);
    for (i64 i = 0; i < n; ++i)
    {
      i64 k = R.lrp[i];
      while (k < R.lrp[i + 1] && R.lc[k] / 64 != i / 64) ++k;
      CHECK(S.ls[i] == k);
      k = R.urp[i];
      while (k < R.urp[i + 1] && R.uc[k] / 64 != i / 64) ++k;
      CHECK(S.us[i] == k);
    }
  }
}

// ---- (c) ------------------------------------------------------------------------------------------------------
static void test_staged_admission()
{
  const i64 n = 6 * 64;
  // L: the last row takes `count` columns from column 64 on (blocks 1.., all within kRing4 of block 5)
  auto slab_l = [&](int count) {
    Factors F(n);
    for (int k = 0; k < count; ++k) F.l[n - 1].push_back({(i32)(64 + k), 1.0});
    return F.plan();
  };
  // U: row 0 takes `count` columns descending from column 64 + count - 1 (blocks 1..3)
  auto slab_u = [&](int count) {
    Factors F(n);
    for (int k = count - 1; k >= 0; --k) F.u[0].push_back({(i32)(64 + k), 1.0});
    return F.plan();
  };
  CHECK(slab_l(kSlab).staged);
  CHECK(!slab_l(kSlab + 1).staged);
  CHECK(slab_u(kSlab).staged);
  CHECK(!slab_u(kSlab + 1).staged);
  // one entry `dist` blocks away: L from the first row of block 5 back, U from row 0 forward
  auto far_l = [&](int dist) {
    Factors F(n);
    F.l[5 * 64].push_back({(i32)((5 - dist) * 64 + 63), 1.0});
    return F.plan();
  };
  auto far_u = [&](int dist) {
    Factors F(n);
    F.u[0].push_back({(i32)(dist * 64), 1.0});
    return F.plan();
  };
  CHECK(far_l(kRing4).staged && far_l(kRing4).gd[0] == kRing4 && far_l(kRing4).gd[1] == 0);
  CHECK(!far_l(kRing4 + 1).staged && far_l(kRing4 + 1).gd[0] == kRing4 + 1);
  CHECK(far_u(kRing4).staged && far_u(kRing4).gd[1] == kRing4 && far_u(kRing4).gd[0] == 0);
  CHECK(!far_u(kRing4 + 1).staged && far_u(kRing4 + 1).gd[1] == kRing4 + 1);
}

// ---- (d) ------------------------------------------------------------------------------------------------------
static void test_binv_admission()
{
  const i64 n = 10 * 64;
  {
    Factors F(n);  // block-diagonal: bidiagonal inside every block
    for (i64 i = 0; i < n; ++i)
    {
      if (i % 64) F.l[i].push_back({(i32)(i - 1), 0.5});
      if (i % 64 != 63) F.u[i].push_back({(i32)(i + 1), 0.5});
    }
    const TrsvPlan p = F.plan();
    CHECK(p.gd[0] == 0 && p.gd[1] == 0 && p.binv_admitted && p.staged);
    F.ud[n / 2] = 0.0;  // one zero pivot
    CHECK(!F.plan().binv_admitted);
  }
  for (int reach : {8, 9})
  {
    Factors F(n);
    F.l[reach * 64].push_back({0, 0.5});
    F.u[0].push_back({64, 0.5});
    const TrsvPlan p = F.plan();
    CHECK(p.gd[0] == reach && p.gd[1] == 1);
    CHECK(p.binv_admitted == (reach == 8));
    CHECK(!p.staged);
  }
  // tile cap with empty rows and unit pivots: 2 tiles per block
  for (i64 extra : {0, 1})
  {
    const i64 big = 16384 * 64 + extra;
    FactorRows R;
    R.lrp.assign(big + 1, 0);
    R.urp.assign(big + 1, 0);
    R.ud.assign(big, 1.0);
    const TrsvPlan p = trsv_plan(big, R, row_splits(big, R));
    CHECK(p.gd[0] == 0 && p.gd[1] == 0 && p.staged);
    CHECK(p.binv_admitted == (extra == 0));
  }
}

// ---- (e) ------------------------------------------------------------------------------------------------------
static void test_tiles_exact()
{
  const i64 n = 130, nblocks = 3;
  const double a = 0.5;
  Factors F(n);
  for (i64 i = 0; i < n; ++i)
  {
    if (i - 64 >= 0) F.l[i].push_back({(i32)(i - 64), 0.25});   // the block at distance 1
    if (i % 64) F.l[i].push_back({(i32)(i - 1), a});
    if (i + 128 < n) F.u[i].push_back({(i32)(i + 128), 0.25});  // the block at distance 2
    if (i % 64 != 63 && i + 1 < n) F.u[i].push_back({(i32)(i + 1), 0.5});
    F.ud[i] = 2.0;
  }
  const FactorRows R = F.rows();
  const RowSplits S = row_splits(n, R);
  const TrsvPlan p = trsv_plan(n, R, S);
  CHECK(p.gd[0] == 1 && p.gd[1] == 2 && p.binv_admitted);
  const BinvTiles L = build_binv_tiles(n, R.lrp, R.lc, R.lv, S.ls, nullptr, p.gd[0]);
  const BinvTiles U = build_binv_tiles(n, R.urp, R.uc, R.uv, S.us, R.ud.data(), p.gd[1]);
  CHECK(L.ok && U.ok);
  CHECK(L.dinv.size() == (size_t)nblocks * 4096 && L.g.size() == (size_t)nblocks * 1 * 4096);
  CHECK(U.dinv.size() == (size_t)nblocks * 4096 && U.g.size() == (size_t)nblocks * 2 * 4096);
  for (i64 b = 0; b < nblocks; ++b)
  {
    const i64 nbr = std::min<i64>(64, n - b * 64);
    for (int t = 0; t < 64; ++t)
      for (int r = 0; r < 64; ++r)
      {
        const bool in = t < nbr && r < nbr;
        // inv(L_bb)[r][t] = (-a)^(r - t), inv(U_bb)[r][t] = (1/2) (-1/4)^(t - r); identity past n
        const double el = in ? (r >= t ? std::pow(-a, r - t) : 0.0) : (r == t ? 1.0 : 0.0);
        const double eu = in ? (t >= r ? 0.5 * std::pow(-0.25, t - r) : 0.0) : (r == t ? 1.0 : 0.0);
        CHECK(L.dinv[(size_t)b * 4096 + t * 64 + r] == el);
        CHECK(U.dinv[(size_t)b * 4096 + t * 64 + r] == eu);
        // L: T(b, 1) = I / 4 on the block's rows (block 0 has no block before it)
        const double gl = (b > 0 && in && r >= t) ? std::pow(-a, r - t) * 0.25 : 0.0;
        CHECK(L.g[((size_t)b * 1 + 0) * 4096 + t * 64 + r] == gl);
        // U: only rows 0 and 1 reach block 2 (columns 128, 129): T(0, 2) = I / 4 on those two; the
        // block at distance 1 carries no entry, blocks 3 and 4 are outside the matrix
        const double gu = (b == 0 && t < 2 && r <= t) ? 0.5 * std::pow(-0.25, t - r) * 0.25 : 0.0;
        CHECK(U.g[((size_t)b * 2 + 0) * 4096 + t * 64 + r] == 0.0);
        CHECK(U.g[((size_t)b * 2 + 1) * 4096 + t * 64 + r] == gu);
      }
  }
}

// ---- (f) ------------------------------------------------------------------------------------------------------
static void test_gate()
{
  auto one = [](double pivot) {
    Factors F(1);
    F.ud[0] = pivot;
    const FactorRows R = F.rows();
    const RowSplits S = row_splits(1, R);
    return build_binv_tiles(1, R.urp, R.uc, R.uv, S.us, R.ud.data(), 0);
  };
  const BinvTiles t = one(0x1.0p-13);  // 1 * 8192 * 64 = 524288
  CHECK(t.ok && t.dinv[0] == 8192.0 && t.dinv[65] == 1.0 && t.dinv[1] == 0.0);
  CHECK(!one(0x1.0p-14).ok);  // 1 * 16384 * 64 = 1048576 > 1e6
  const double nan = std::numeric_limits<double>::quiet_NaN();
  {
    Factors F(2);
    F.u[0].push_back({1, nan});
    const FactorRows R = F.rows();
    const RowSplits S = row_splits(2, R);
    CHECK(!build_binv_tiles(2, R.urp, R.uc, R.uv, S.us, R.ud.data(), 0).ok);
  }
  {
    Factors F(2);
    F.l[1].push_back({0, nan});
    const FactorRows R = F.rows();
    const RowSplits S = row_splits(2, R);
    CHECK(!build_binv_tiles(2, R.lrp, R.lc, R.lv, S.ls, nullptr, 0).ok);
  }
  CHECK(!one(nan).ok);
}

// ---- (g) ------------------------------------------------------------------------------------------------------
// a dyadic value in [-1/8, 1/8) per (row, column)
static double small_value(i64 i, i64 j)
{
  uint64_t h = (uint64_t)i * 1000003u + (uint64_t)j + 0x9e3779b97f4a7c15ull;
  h = (h ^ (h >> 30)) * 0xbf58476d1ce4e5b9ull;
  h ^= h >> 31;
  return ((double)(h >> 40) * 0x1.0p-24 - 0.5) * 0.25;
}
static void test_threads()
{
  const i64 n = 2500;  // 40 blocks, the last of 4 rows
  Factors F(n);
  for (i64 i = 0; i < n; ++i)
  {
    for (i64 d : {130, 64, 3, 1})
      if (i - d >= 0) F.l[i].push_back({(i32)(i - d), small_value(i, i - d)});
    for (i64 d : {70, 2, 1})
      if (i + d < n) F.u[i].push_back({(i32)(i + d), small_value(i, i + d)});
    F.ud[i] = 1.0 + (double)(i % 5) * 0.25;
  }
  FactorRows R = F.rows();
  const RowSplits S = row_splits(n, R);
  const TrsvPlan p = trsv_plan(n, R, S);
  CHECK(p.gd[0] == 3 && p.gd[1] == 2 && p.binv_admitted);
  BinvTiles one[2], four[2];
  for (int threads : {1, 4})
  {
    trsv_image_threads = threads;
    BinvTiles *out = threads == 1 ? one : four;
    out[0] = build_binv_tiles(n, R.lrp, R.lc, R.lv, S.ls, nullptr, p.gd[0]);
    out[1] = build_binv_tiles(n, R.urp, R.uc, R.uv, S.us, R.ud.data(), p.gd[1]);
  }
  for (int f = 0; f < 2; ++f)
  {
    CHECK(one[f].ok && four[f].ok);
    CHECK(same_bits(one[f].dinv, four[f].dinv) && same_bits(one[f].g, four[f].g));
    double big = 0.0;
    for (double v : four[f].g) big = std::max(big, std::fabs(v));
    CHECK(big > 0.0);
  }
  R.ud[20 * 64 + 5] = 0x1.0p-30;  // one ill-conditioned block in the middle
  trsv_image_threads = 4;
  CHECK(!build_binv_tiles(n, R.urp, R.uc, R.uv, S.us, R.ud.data(), p.gd[1]).ok);
  trsv_image_threads = 1;
  CHECK(!build_binv_tiles(n, R.urp, R.uc, R.uv, S.us, R.ud.data(), p.gd[1]).ok);
  trsv_image_threads = 0;
}

// ---- (h) ------------------------------------------------------------------------------------------------------
// Reads one factor's staged image back by its layout rule and compares it with the rows.
static void check_staged(i64 n, const std::vector<i64> &rp, const std::vector<i32> &cj, const std::vector<double> &cv,
                         const std::vector<i64> &split, const std::vector<i32> &w_expected)
{
  const StagedImage im = build_staged_image(n, rp, cj, cv, split);
  const i64 nblocks = (n + 63) / 64;
  CHECK(im.w == w_expected);
  CHECK((i64)im.v1.size() == nblocks * kSlab * 64 && im.c1.size() == im.v1.size());
  CHECK((i64)im.tile.size() == nblocks * 4096 && (i64)im.tmask.size() == nblocks * 64);
  std::vector<i32> c1(im.c1.size(), -1);
  std::vector<double> v1(im.v1.size(), 0.0), tile(im.tile.size(), 0.0);
  std::vector<unsigned long long> tmask(im.tmask.size(), 0ull);
  for (i64 i = 0; i < n; ++i)
  {
    const i64 b = i / 64, r = i % 64;
    for (i64 q = rp[i]; q < split[i]; ++q)
    {
      c1[(b * kSlab + (q - rp[i])) * 64 + r] = cj[q];
      v1[(b * kSlab + (q - rp[i])) * 64 + r] = cv[q];
    }
    for (i64 q = split[i]; q < rp[i + 1]; ++q)
    {
      tile[b * 4096 + (cj[q] - b * 64) * 64 + r] = cv[q];
      tmask[b * 64 + r] |= 1ull << (cj[q] - b * 64);
    }
  }
  // every entry where the rule puts it, padding columns -1 (values 0), nothing else set
  CHECK(im.c1 == c1);
  CHECK(same_bits(im.v1, v1));
  CHECK(same_bits(im.tile, tile));
  CHECK(im.tmask == tmask);
}
static void test_staged_image()
{
  const i64 n = 3 * 64 + 5;
  Factors F(n);
  // block 2: rows of 0, 1, 127 and 128 outside entries (plus in-block entries)
  F.l[129].push_back({5, 0.5});
  for (int k = 1; k < 128; ++k) F.l[130].push_back({(i32)k, (double)k});
  for (int k = 0; k < 128; ++k) F.l[131].push_back({(i32)k, -(double)(k + 1)});
  F.l[130].push_back({128, 0.25});
  F.l[131].push_back({128, 2.0});
  F.l[131].push_back({130, 4.0});
  F.l[191].push_back({128, 8.0});
  F.l[191].push_back({190, 16.0});
  // ragged last block: rows 192 .. 196
  F.l[193].push_back({192, 32.0});
  F.l[194].push_back({100, 64.0});
  F.l[196].push_back({192, 0.125});
  F.l[196].push_back({194, 0.0625});
  F.l[196].push_back({195, 128.0});
  // U (descending): row 0 with 128 outside entries, in-block entries of the first and the ragged block
  for (int k = 127; k >= 0; --k) F.u[0].push_back({(i32)(64 + k), (double)(k + 1)});
  F.u[0].push_back({63, 0.5});
  F.u[0].push_back({1, 0.25});
  F.u[1].push_back({70, 2.0});
  F.u[192].push_back({196, 4.0});
  F.u[192].push_back({193, 8.0});
  F.u[195].push_back({196, 16.0});
  const FactorRows R = F.rows();
  const RowSplits S = row_splits(n, R);
  CHECK(trsv_plan(n, R, S).staged);
  check_staged(n, R.lrp, R.lc, R.lv, S.ls, {0, 0, 128, 1});
  check_staged(n, R.urp, R.uc, R.uv, S.us, {128, 0, 0, 0});
  // literal spot checks of the rule itself
  const StagedImage im = build_staged_image(n, R.lrp, R.lc, R.lv, S.ls);
  CHECK(im.c1[(2 * kSlab + 0) * 64 + 1] == 5 && im.v1[(2 * kSlab + 0) * 64 + 1] == 0.5);
  CHECK(im.c1[(2 * kSlab + 1) * 64 + 1] == -1);
  CHECK(im.c1[(2 * kSlab + 126) * 64 + 2] == 127 && im.c1[(2 * kSlab + 127) * 64 + 2] == -1);
  CHECK(im.c1[(2 * kSlab + 127) * 64 + 3] == 127 && im.v1[(2 * kSlab + 127) * 64 + 3] == -128.0);
  CHECK(im.c1[(2 * kSlab + 0) * 64 + 0] == -1);
  CHECK(im.c1[(3 * kSlab + 0) * 64 + 2] == 100);
  CHECK(im.tmask[3 * 64 + 4] == 0xdull && im.tmask[3 * 64 + 1] == 1ull && im.tmask[3 * 64 + 0] == 0ull);
  CHECK(im.tile[3 * 4096 + 3 * 64 + 4] == 128.0 && im.tile[3 * 4096 + 2 * 64 + 4] == 0.0625);
  CHECK(im.tmask[2 * 64 + 3] == 5ull && im.tmask[2 * 64 + 63] == ((1ull << 62) | 1ull));
  // a row of 129 outside entries
  Factors G(4 * 64);
  for (int k = 0; k < 129; ++k) G.l[192].push_back({(i32)k, 1.0});
  const FactorRows RG = G.rows();
  const RowSplits SG = row_splits(G.n, RG);
  CHECK(!trsv_plan(G.n, RG, SG).staged);
  CHECK(throws_arg([&] { build_staged_image(G.n, RG.lrp, RG.lc, RG.lv, SG.ls); }));
}

// ---- (i) ------------------------------------------------------------------------------------------------------
static void test_export_envelope()
{
  const i64 n = 5;
  const std::vector<i64> f = {0, 0, 1, 1, 3};
  double L[5][5] = {}, U[5][5] = {}, D[5] = {2, 4, 8, 16, 32};
  L[1][0] = 0.5;
  L[2][1] = 0.0;  // an exact zero inside the envelope
  L[3][1] = 0.25;
  L[3][2] = 0.125;
  L[4][3] = 2.0;
  U[0][1] = 3.0;
  U[1][2] = 5.0;
  U[1][3] = 0.0;  // and one in U
  U[2][3] = 7.0;
  U[3][4] = 9.0;
  const ExportedFactors E = export_envelope(
      n, f, [&](i64 r, i64 c) { return L[r][c]; }, [&](i64 r, i64 c) { return U[r][c]; }, [&](i64 k) { return D[k]; });
  CHECK((E.Lp == std::vector<i64>{0, 1, 3, 4, 7, 9}));
  CHECK((E.Lj == std::vector<i64>{0, 0, 1, 2, 1, 2, 3, 3, 4}));
  CHECK((E.Lx == std::vector<double>{1, 0.5, 1, 1, 0.25, 0.125, 1, 2, 1}));
  CHECK((E.Up == std::vector<i64>{0, 1, 3, 5, 7, 9}));
  CHECK((E.Ui == std::vector<i64>{0, 0, 1, 1, 2, 2, 3, 3, 4}));
  CHECK((E.Ux == std::vector<double>{2, 3, 4, 5, 8, 7, 16, 9, 32}));
  // and back through factor_rows
  const FactorRows R = factor_rows(n, E.Lp, E.Lj, E.Lx, E.Up, E.Ui, E.Ux);
  CHECK((R.lc == std::vector<i32>{0, 1, 2, 3}) && (R.uc == std::vector<i32>{1, 2, 3, 4}));
  CHECK((R.ud == std::vector<double>{2, 4, 8, 16, 32}));
}

int main()
{
  test_factor_rows();
  test_row_splits();
  test_staged_admission();
  test_binv_admission();
  test_tiles_exact();
  test_gate();
  test_threads();
  test_staged_image();
  test_export_envelope();
  if (failures)
  {
    std::printf("%d check(s) FAILED\n", failures);
    return 1;
  }
  std::printf("ALL OK\n");
  return 0;
}
