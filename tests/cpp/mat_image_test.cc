// Host-side unit checks of the matrix images (csrc/mat_image.cpp, compiled with this file and csrc/gen.cpp).
// No GPU and no library: plain host code.  The checks state what defines an image, not how it is built:
//  (a) reading the SELL image back by the layout rule of internal.h (padding dropped) gives the input CSR, for a
//      1 x 1 matrix, 3 x 3 blocks, a ragged matrix with a partial last slice and shifted columns; stencil slices
//      give the same rows through their offsets and row masks;
//  (b) which slices become stencil slices (8 offsets yes, 9 no, EIG_MAT_NO_STENCIL none) and the counts by hand;
//  (c) reading the band image back (offset d >= 0 at [j(d)][w], d < 0 at [j(-d)][w + d], gated by the row mask)
//      gives every row's entries bitwise and in order;
//  (d) the cases in which no band image is built;
//  (e) the uniform band, (f) the geometric masks, (g) the 27-point box masks, each against literal expectations;
//  (h) the interior / boundary slices and the plane-march split of a slab;
//  (i) a threaded build (Poisson 64^3: 4096 slices) equals the one-thread build bit for bit;
//  (j) validate_csr and diag_share on a 3-row example.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <string>

#include "../../dune-eigensolver_amd/csrc/mat_image.h"

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

// host block-CSR rows [row0, row0 + nb) of a matrix; bb values per block
struct Csr {
  i64 row0 = 0, nb = 0;
  int bb = 1;
  std::vector<i64> rp;
  std::vector<i32> c;
  std::vector<double> v;
};

template <class T>
static bool same_bits(const std::vector<T> &a, const std::vector<T> &b)
{
  return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(T)) == 0);
}
static bool same(const Csr &a, const Csr &b) { return a.rp == b.rp && a.c == b.c && same_bits(a.v, b.v); }

// a value per unordered pair (i, j): a(i, j) = a(j, i) bit for bit, no two pairs alike
static double pair_value(i64 i, i64 j)
{
  uint64_t h = (uint64_t)std::min(i, j) * 1000003u + (uint64_t)std::max(i, j) + 0x9e3779b97f4a7c15ull;
  h = (h ^ (h >> 30)) * 0xbf58476d1ce4e5b9ull;
  h ^= h >> 31;
  return (i == j ? 8.0 : -1.5) + (double)(h >> 11) * 0x1.0p-53;
}

// rows [row0, row0 + nb): row g stores the columns cols(g) lists (ascending) with value val(g, col)
static Csr make_rows(i64 row0, i64 nb, const std::function<void(i64, std::vector<i64> &)> &cols,
                     const std::function<double(i64, i64)> &val = pair_value)
{
  Csr A;
  A.row0 = row0;
  A.nb = nb;
  A.rp.assign(1, 0);
  std::vector<i64> cc;
  for (i64 r = 0; r < nb; ++r)
  {
    cc.clear();
    cols(row0 + r, cc);
    for (i64 q : cc)
    {
      A.c.push_back((i32)q);
      A.v.push_back(val(row0 + r, q));
    }
    A.rp.push_back((i64)A.c.size());
  }
  return A;
}
// n x n band: row g stores g + d for every d of offs (ascending) that stays inside
static Csr banded(i64 n, const std::vector<i64> &offs, const std::function<double(i64, i64)> &val = pair_value)
{
  return make_rows(0, n, [&](i64 g, std::vector<i64> &cc) {
    for (i64 d : offs)
      if (g + d >= 0 && g + d < n) cc.push_back(g + d);
  }, val);
}
// rows [row0, row0 + nb) of the 7-point (ny > 0) or 2-D 5-point (ny = 0: nx x nz) grid, every row storing exactly
// its in-grid neighbours
static Csr grid(i64 nx, i64 ny, i64 nz, i64 row0, i64 nb, const std::function<double(i64, i64)> &val = pair_value)
{
  const i64 D = ny > 0 ? nx * ny : nx;
  return make_rows(row0, nb, [&](i64 g, std::vector<i64> &cc) {
    const i64 x = g % nx, y = ny > 0 ? (g / nx) % ny : 0, z = g / D;
    if (z > 0) cc.push_back(g - D);
    if (ny > 0 && y > 0) cc.push_back(g - nx);
    if (x > 0) cc.push_back(g - 1);
    cc.push_back(g);
    if (x < nx - 1) cc.push_back(g + 1);
    if (ny > 0 && y < ny - 1) cc.push_back(g + nx);
    if (z < nz - 1) cc.push_back(g + D);
  }, val);
}
static double poisson_value(i64 i, i64 j) { return i == j ? 6.0 : -1.0; }

static Csr generated(int kind, int N, i64 row0 = 0, i64 nb = -1)
{
  Csr A;
  const i64 n = (kind <= 3) ? (i64)N * N : (i64)N * N * N;
  A.row0 = row0;
  A.nb = nb < 0 ? n : nb;
  A.bb = kind == 5 ? 9 : 1;
  const i64 nnz = eig_gen_nnzb_rows(kind, N, row0, A.nb);
  A.rp.resize(A.nb + 1);
  A.c.resize(nnz);
  A.v.resize(nnz * A.bb);
  CHECK(eig_gen_matrix_rows(kind, N, row0, A.nb, A.rp.data(), A.c.data(), A.v.data()) == EIG_OK);
  return A;
}
static void add_entry(Csr &A, i64 g, i64 col, double v)
{
  const i64 r = g - A.row0;
  i64 p = A.rp[r];
  while (p < A.rp[r + 1] && A.c[p] < col) ++p;
  A.c.insert(A.c.begin() + p, (i32)col);
  A.v.insert(A.v.begin() + p, v);
  for (i64 q = r + 1; q <= A.nb; ++q) ++A.rp[q];
}
static void drop_entry(Csr &A, i64 g, i64 col)
{
  const i64 r = g - A.row0;
  for (i64 p = A.rp[r]; p < A.rp[r + 1]; ++p)
    if (A.c[p] == col)
    {
      A.c.erase(A.c.begin() + p);
      A.v.erase(A.v.begin() + p);
      for (i64 q = r + 1; q <= A.nb; ++q) --A.rp[q];
      return;
    }
  CHECK(!"drop_entry: no such entry");
}

// the whole n x ncols matrix on one rank
static MatShape whole(i64 n, i64 ncols, int b = 1, int flags = 0)
{
  MatShape s;
  s.br = s.bc = b;
  s.kflags = flags;
  s.nb_rows_global = n;
  s.nb_cols = ncols;
  s.window = ncols * b;
  return s;
}
// a rank's rows [row0, ...) of an n x n matrix whose window starts at block column win0 and has `window` columns
static MatShape slab(i64 n, i64 row0, i64 win0, i64 window, int flags = 0)
{
  MatShape s = whole(n, n, 1, flags);
  s.row_begin = row0;
  s.window = window;
  s.own_offset = row0 - win0;
  return s;
}
static SellImage sell_of(const MatShape &sh, const Csr &A, i64 col_shift = 0)
{
  return build_sell_image(sh, A.nb, A.rp.data(), A.c.data(), A.v.data(), col_shift);
}
static SymImage sym_of(const MatShape &sh, const Csr &A, i64 col_shift = 0)
{
  const SellImage S = sell_of(sh, A, col_shift);
  return build_sym_image(sh, S.nslices, S.nnzb_padded, A.nb, A.rp.data(), A.c.data(), A.v.data());
}

// ---- (a) SELL round trip ------------------------------------------------------------------------------
// internal.h: entry k of slice row l sits at slice_ptr[s] + k * 64 + l (columns, -1 = padding) and
// (slice_ptr[s] + k * 64) * bb + t * 64 + l (values)
static Csr sell_read(const SellImage &S, const Csr &like, i64 col_shift)
{
  Csr B;
  B.row0 = like.row0;
  B.nb = like.nb;
  B.bb = like.bb;
  B.rp.assign(1, 0);
  for (i64 r = 0; r < like.nb; ++r)
  {
    const i64 s = r / 64, l = r % 64, base = S.slice_ptr[s], w = (S.slice_ptr[s + 1] - base) / 64;
    for (i64 k = 0; k < w; ++k)
    {
      const i32 c = S.col[base + k * 64 + l];
      if (c < 0) continue;
      B.c.push_back(c + (i32)col_shift);
      for (int t = 0; t < like.bb; ++t) B.v.push_back(S.val[(base + k * 64) * like.bb + t * 64 + l]);
    }
    B.rp.push_back((i64)B.c.size());
  }
  return B;
}
// the same rows through the stencil slices' offsets and row masks (explicit slices: through their columns)
static Csr stencil_read(const SellImage &S, const Csr &like, i64 col_shift)
{
  Csr B;
  B.row0 = like.row0;
  B.nb = like.nb;
  B.rp.assign(1, 0);
  for (i64 r = 0; r < like.nb; ++r)
  {
    const i64 s = r / 64, l = r % 64, base = S.slice_ptr[s], w = (S.slice_ptr[s + 1] - base) / 64;
    for (i64 k = 0; k < w; ++k)
    {
      if (S.st_width[s] > 0)
      {
        CHECK(w == S.st_width[s]);
        if (!(S.st_mask[s * 64 + l] >> k & 1)) continue;
        B.c.push_back((i32)(like.row0 + r + S.st_delta[8 * s + k]));
      }
      else
      {
        if (S.col[base + k * 64 + l] < 0) continue;
        B.c.push_back(S.col[base + k * 64 + l] + (i32)col_shift);
      }
      B.v.push_back(S.val[base + k * 64 + l]);
    }
    B.rp.push_back((i64)B.c.size());
  }
  return B;
}
static void check_sell(const MatShape &sh, const Csr &A, i64 col_shift = 0)
{
  const SellImage S = sell_of(sh, A, col_shift);
  CHECK(S.nslices == (A.nb + 63) / 64 && S.nnzb_padded == S.slice_ptr[S.nslices]);
  CHECK(same(sell_read(S, A, col_shift), A));
  if (A.bb == 1) CHECK(same(stencil_read(S, A, col_shift), A));
  i64 bw = 0;
  for (i64 r = 0; r < A.nb; ++r)
    for (i64 p = A.rp[r]; p < A.rp[r + 1]; ++p) bw = std::max<i64>(bw, std::llabs(A.c[p] - (A.row0 + r)));
  CHECK(S.bandwidth == bw);
}
static void test_sell()
{
  const Csr one = make_rows(0, 1, [](i64, std::vector<i64> &cc) { cc.push_back(0); });
  check_sell(whole(1, 1), one);
  const SellImage S1 = sell_of(whole(1, 1), one);
  CHECK(S1.nslices == 1 && S1.nnzb_padded == 64 && S1.n_stencil_slices == 1 && S1.sell_explicit == 0);
  const Csr q1 = generated(5, 3);  // 27 block rows of 3 x 3 blocks: explicit columns
  check_sell(whole(27, 27, 3), q1);
  CHECK(sell_of(whole(27, 27, 3), q1).n_stencil_slices == 0);
  // ragged: 150 rows (the last slice holds 22) of 0 .. 11 scattered entries, some rows empty
  const Csr rag = make_rows(0, 150, [](i64 g, std::vector<i64> &cc) {
    for (i64 k = 0; k < (g * 7) % 12; ++k) cc.push_back((g * 3 + k * k * 5 + k) % 13 + 13 * k);
  });
  check_sell(whole(150, 160), rag);
  check_sell(whole(150, 160, 1, EIG_MAT_NO_STENCIL), rag);
  // shifted columns: planes 2 .. 4 of the 8 x 8 x 8 Poisson matrix, the window starting one plane below
  const Csr mid = generated(4, 8, 128, 192);
  check_sell(slab(512, 128, 64, 320), mid, 64);
  const SellImage Sm = sell_of(slab(512, 128, 64, 320), mid, 64);
  CHECK(Sm.n_stencil_slices == 3 && Sm.col[Sm.slice_ptr[0]] == 0);  // row 128's first entry: column 64, shifted
}

// ---- (b) stencil slices -------------------------------------------------------------------------------
static void test_stencil()
{
  // 128 rows of two entries: the rows of slice 0 use the offsets 0 .. 9 but 8 (9 in all), those of slice 1 0 .. 7
  const Csr A = make_rows(0, 128, [](i64 g, std::vector<i64> &cc) {
    cc.push_back(g);
    cc.push_back(g + 1 + g % (g < 64 ? 8 : 7) + (g < 64 && g % 8 == 7));
  });
  const SellImage S = sell_of(whole(128, 140), A);
  CHECK(S.st_width[0] == -1 && S.st_width[1] == 8);
  for (int k = 0; k < 8; ++k) CHECK(S.st_delta[8 + k] == k);
  CHECK(S.n_stencil_slices == 1 && S.sell_explicit == 2 * 64 && S.nnzb_padded == 2 * 64 + 8 * 64);
  CHECK(S.st_mask[64 + 3] == (1u | 1u << 5));  // row 67: offsets 0 and 1 + 67 % 7 = 5
  const SellImage N = sell_of(whole(128, 140, 1, EIG_MAT_NO_STENCIL), A);
  CHECK(N.st_width[0] == -1 && N.st_width[1] == -1);
  CHECK(N.n_stencil_slices == 0 && N.sell_explicit == 4 * 64 && N.nnzb_padded == 4 * 64);
  check_sell(whole(128, 140), A);
}

// ---- (c) band round trip ------------------------------------------------------------------------------
static void check_band(const MatShape &sh, const Csr &A, const SymImage &S)
{
  CHECK(S.built);
  if (!S.built) return;
  CHECK(S.mask_bytes == (S.nd <= 8 ? 1 : 4) && S.ld % 64 == 0 && S.val.size() == (size_t)S.nup * S.ld);
  // off ascending; dj = the rank of |off| among the distinct |off|
  std::vector<i64> ups;
  for (int k = 0; k < S.nd; ++k)
  {
    if (k) CHECK(S.off[k] > S.off[k - 1]);
    ups.push_back(std::llabs((i64)S.off[k]));
  }
  std::sort(ups.begin(), ups.end());
  ups.erase(std::unique(ups.begin(), ups.end()), ups.end());
  CHECK((int)ups.size() == S.nup);
  for (int k = 0; k < S.nd; ++k) CHECK(ups[S.dj[k]] == std::llabs((i64)S.off[k]));
  Csr B;
  B.rp.assign(1, 0);
  for (i64 r = 0; r < A.nb; ++r)
  {
    const i64 w = sh.own_offset + r;
    const uint32_t m = S.mask_bytes == 1 ? S.mask8[r] : S.mask32[r];
    for (int k = 0; k < S.nd; ++k)
    {
      if (!(m >> k & 1)) continue;
      const i64 d = S.off[k];
      B.c.push_back((i32)(A.row0 + r + d));
      B.v.push_back(S.val[(size_t)S.dj[k] * S.ld + (d >= 0 ? w : w + d)]);
    }
    B.rp.push_back((i64)B.c.size());
  }
  CHECK(same(B, A));
}
static const std::vector<i64> kTwelve = {-11, -7, -5, -3, -2, -1, 1, 2, 3, 5, 7, 11};
// planes 1 .. 4 of the 8 x 8 x 6 grid (D = 64), the window covering the ghost planes 0 and 5.  (Two owned planes of
// a 4-plane grid never get a band image: its 4 arrays span the window, 4 (nb + 2 D) > 0.9 * 7 nb at nb = 2 D.)
static Csr slab_rows(const std::function<double(i64, i64)> &val = pair_value) { return grid(8, 8, 6, 64, 256, val); }
static MatShape slab_shape(int flags = 0) { return slab(384, 64, 0, 384, flags); }

static void test_band()
{
  const Csr g3 = grid(3, 4, 5, 0, 60);
  check_band(whole(60, 60), g3, sym_of(whole(60, 60), g3));
  const Csr g2 = grid(6, 0, 5, 0, 30);
  check_band(whole(30, 30), g2, sym_of(whole(30, 30), g2));
  const Csr kuhn = generated(6, 4);
  const SymImage Sk = sym_of(whole(64, 64), kuhn);
  check_band(whole(64, 64), kuhn, Sk);
  CHECK(Sk.nd == 15 && Sk.nup == 8 && Sk.mask_bytes == 4);
  // one-sided: the entries at -2 have no stored mirror, those at -1 / +1 are pairs
  const Csr os = banded(100, {-2, -1, 0, 1});
  const SymImage So = sym_of(whole(100, 100), os);
  check_band(whole(100, 100), os, So);
  CHECK(So.nd == 4 && So.nup == 3 && So.mask_bytes == 1);
  const Csr b12 = banded(200, kTwelve);
  const SymImage S12 = sym_of(whole(200, 200), b12);
  check_band(whole(200, 200), b12, S12);
  CHECK(S12.nd == 12 && S12.nup == 6 && S12.mask_bytes == 4);
  // slab: the ghost rows of plane 0 get their +D slots from the lower entries of plane 1 alone
  const Csr sl = slab_rows();
  const SymImage Ss = sym_of(slab_shape(), sl);
  check_band(slab_shape(), sl, Ss);
  if (Ss.built)
    for (i64 x = 0; x < 64; ++x)
      CHECK(Ss.val[(size_t)Ss.dj[6] * Ss.ld + x] == pair_value(x, x + 64));  // a(x, x + D) of ghost row x
}

// ---- (d) refusals -------------------------------------------------------------------------------------
static void test_refusals()
{
  Csr g3 = grid(3, 4, 5, 0, 60);
  CHECK(sym_of(whole(60, 60), g3).built);
  CHECK(!sym_of(whole(60, 60, 1, EIG_MAT_NO_BAND), g3).built);
  CHECK(!sym_of(whole(60, 61), g3).built);  // not square
  // a(16, 17) one unit in the last place away from a(17, 16)
  for (i64 p = g3.rp[16]; p < g3.rp[17]; ++p)
    if (g3.c[p] == 17) g3.v[p] = std::nextafter(g3.v[p], 0.0);
  CHECK(!sym_of(whole(60, 60), g3).built);
  std::vector<i64> wide;
  for (i64 d = -16; d <= 16; ++d) wide.push_back(d);
  const Csr b33 = banded(200, wide);
  CHECK(!sym_of(whole(200, 200), b33).built);
  wide.pop_back();  // 32 offsets: built
  const Csr b32 = banded(200, wide);
  CHECK(sym_of(whole(200, 200), b32).built);
  // rows [D, 3 D) of the 4 x 4 x 4 Poisson matrix: 4 arrays of 128 window rows > 0.9 * 7 * 64 padded SELL values
  const Csr two = generated(4, 4, 16, 32);
  const SellImage S2 = sell_of(slab(64, 16, 0, 64), two);
  CHECK(S2.nnzb_padded == 7 * 64);
  CHECK(!sym_of(slab(64, 16, 0, 64), two).built);
}

// ---- (e) uniform band ---------------------------------------------------------------------------------
static void test_uniform()
{
  const Csr p = grid(3, 4, 5, 0, 60, poisson_value);
  const SymImage S = sym_of(whole(60, 60), p);
  CHECK(S.built && S.uniform && S.nup == 4);
  CHECK(S.uc[0] == 6.0 && S.uc[1] == -1.0 && S.uc[2] == -1.0 && S.uc[3] == -1.0);
  const Csr var = generated(8, 4);
  const SymImage Sv = sym_of(whole(64, 64), var);
  CHECK(Sv.built && !Sv.uniform && Sv.uc[0] == 0.0 && Sv.geo);
  // constant per offset but for one lower entry whose mirror is not stored: the mirror pass compares nothing
  auto const_value = [](i64 i, i64 j) { return 10.0 + (double)std::llabs(j - i); };
  Csr os = banded(100, {-2, -1, 0, 1}, const_value);
  CHECK(sym_of(whole(100, 100), os).built && sym_of(whole(100, 100), os).uniform);
  for (i64 p2 = os.rp[50]; p2 < os.rp[51]; ++p2)
    if (os.c[p2] == 48) os.v[p2] = 7.0;
  const SymImage So = sym_of(whole(100, 100), os);
  CHECK(So.built && !So.uniform);
  check_band(whole(100, 100), os, So);
}

// ---- (f) geometric masks ------------------------------------------------------------------------------
static void test_geo()
{
  Csr g3 = grid(3, 4, 5, 0, 60);
  const SymImage S3 = sym_of(whole(60, 60), g3);
  CHECK(S3.geo && S3.gx == 3 && S3.gy == 4 && S3.gz == 5 && S3.gz0 == 0 && S3.box27 == 0);
  const Csr g2 = grid(6, 0, 5, 0, 30);
  const SymImage S2 = sym_of(whole(30, 30), g2);
  CHECK(S2.geo && S2.gx == 6 && S2.gy == 1 && S2.gz == 5 && S2.gz0 == 0);
  const SymImage Ss = sym_of(slab_shape(), slab_rows());
  CHECK(Ss.geo && Ss.gx == 8 && Ss.gy == 8 && Ss.gz == 6 && Ss.gz0 == 1);
  // an interior entry dropped: (31, 32) is x = 1 -> 2 of line y = 2, z = 2
  Csr miss = g3;
  drop_entry(miss, 31, 32);
  const SymImage Sm = sym_of(whole(60, 60), miss);
  CHECK(Sm.built && !Sm.geo && Sm.box27 == 0);
  check_band(whole(60, 60), miss, Sm);
  // a periodic wrap in x: (2, 3) joins x = 2 of line 0 to x = 0 of line 1, through the stored offset +1
  Csr wrap = g3;
  add_entry(wrap, 2, 3, pair_value(2, 3));
  add_entry(wrap, 3, 2, pair_value(2, 3));
  const SymImage Sw = sym_of(whole(60, 60), wrap);
  CHECK(Sw.built && Sw.nd == 7 && !Sw.geo && Sw.box27 == 0);
}

// ---- (g) box masks ------------------------------------------------------------------------------------
static void test_box27()
{
  // the Kuhn edges: 0, +-e_i, +-(e_i + e_j), +-(1, 1, 1), i.e. all steps inside {0, 1}^3 or {0, -1}^3
  unsigned kuhn_bits = 0;
  for (int a = -1; a <= 1; ++a)
    for (int b = -1; b <= 1; ++b)
      for (int c = -1; c <= 1; ++c)
        if ((a >= 0 && b >= 0 && c >= 0) || (a <= 0 && b <= 0 && c <= 0)) kuhn_bits |= 1u << ((a + 1) * 9 + (b + 1) * 3 + c + 1);
  Csr kuhn = generated(6, 4);
  const SymImage S = sym_of(whole(64, 64), kuhn);
  CHECK(S.built && !S.geo && S.box27 == kuhn_bits && __builtin_popcount(S.box27) == 15);
  CHECK(S.gx == 4 && S.gy == 4 && S.gz == 4 && S.gz0 == 0);
  // row 3 (x = 3, the last of its line) stores column 4 = x + 1 out of the grid, through the stored offset +1
  add_entry(kuhn, 3, 4, -0.25);
  add_entry(kuhn, 4, 3, -0.25);
  const SymImage Sb = sym_of(whole(64, 64), kuhn);
  CHECK(Sb.built && Sb.nd == 15 && Sb.box27 == 0);
  check_band(whole(64, 64), kuhn, Sb);
}

// ---- (h) slice split ----------------------------------------------------------------------------------
// planes of 128 rows (2 slices) from global row 128 on: a row stores its diagonal, a row of a plane with ghost[z]
// also the first column above the owned range
static SliceSplit split_of(const std::vector<int> &ghost, i64 D)
{
  const i64 nb = 128 * (i64)ghost.size();
  const Csr A = make_rows(128, nb, [&](i64 g, std::vector<i64> &cc) {
    cc.push_back(g);
    if (ghost[(g - 128) / 128]) cc.push_back(128 + nb);
  });
  return split_slices((nb + 63) / 64, nb, 128, A.rp.data(), A.c.data(), D);
}
static void test_split()
{
  // 6 planes of the 3-point pattern -D / 0 / +D: the first and the last plane reference ghost rows
  const Csr A = make_rows(128, 768, [](i64 g, std::vector<i64> &cc) {
    cc.push_back(g - 128);
    cc.push_back(g);
    cc.push_back(g + 128);
  });
  const SliceSplit S = split_slices(12, 768, 128, A.rp.data(), A.c.data(), 128);
  CHECK((S.interior == std::vector<i32>{2, 3, 4, 5, 6, 7, 8, 9}) && (S.boundary == std::vector<i32>{0, 1, 10, 11}));
  CHECK(S.mz0 == 1 && S.mz1 == 5 && (S.march_bnd == std::vector<i32>{0, 1, 10, 11}));
  const SliceSplit S0 = split_slices(12, 768, 128, A.rp.data(), A.c.data(), 0);  // no march geometry
  CHECK(S0.interior == S.interior && S0.boundary == S.boundary && S0.mz1 <= S0.mz0 && S0.march_bnd.empty());
  const SliceSplit L = split_of({1, 0, 0, 1, 0, 0, 0, 1}, 128);  // runs [1, 3) and [4, 7): the longer
  CHECK(L.mz0 == 4 && L.mz1 == 7 && (L.march_bnd == std::vector<i32>{0, 1, 2, 3, 4, 5, 6, 7, 14, 15}));
  const SliceSplit T = split_of({1, 0, 0, 1, 0, 0, 1}, 128);  // runs [1, 3) and [4, 6): the earlier
  CHECK(T.mz0 == 1 && T.mz1 == 3 && (T.march_bnd == std::vector<i32>{0, 1, 6, 7, 8, 9, 10, 11, 12, 13}));
  CHECK((T.interior == std::vector<i32>{2, 3, 4, 5, 8, 9, 10, 11}));
  const SliceSplit O = split_of({1, 0, 1, 0, 1}, 128);  // runs of one plane: no split
  CHECK(O.mz1 <= O.mz0 && O.march_bnd.empty() && O.interior.size() == 4);
  const SliceSplit W = split_of({0, 0, 0}, 128);  // nothing references a ghost: every plane, no boundary slice
  CHECK(W.mz0 == 0 && W.mz1 == 3 && W.march_bnd.empty() && W.boundary.empty());
}

// ---- (i) threaded passes ------------------------------------------------------------------------------
static void test_threads()
{
  const Csr A = generated(4, 64);  // 262144 rows, 4096 slices
  const MatShape sh = whole(A.nb, A.nb);
  SellImage S[3];
  SymImage B[3];
  const int threads[3] = {1, 4, 0};
  for (int i = 0; i < 3; ++i)
  {
    mat_image_threads = threads[i];
    S[i] = sell_of(sh, A);
    B[i] = build_sym_image(sh, S[i].nslices, S[i].nnzb_padded, A.nb, A.rp.data(), A.c.data(), A.v.data());
  }
  mat_image_threads = 0;
  CHECK(S[0].nslices == 4096 && S[0].n_stencil_slices == 4096 && S[0].bandwidth == 4096);
  CHECK(B[0].built && B[0].uniform && B[0].geo && B[0].gx == 64 && B[0].gy == 64 && B[0].gz == 64 && B[0].gz0 == 0);
  for (int i = 1; i < 3; ++i)
  {
    CHECK(S[i].slice_ptr == S[0].slice_ptr && S[i].col == S[0].col && same_bits(S[i].val, S[0].val));
    CHECK(S[i].st_width == S[0].st_width && S[i].st_delta == S[0].st_delta && S[i].st_mask == S[0].st_mask);
    CHECK(S[i].nnzb_padded == S[0].nnzb_padded && S[i].n_stencil_slices == S[0].n_stencil_slices &&
          S[i].sell_explicit == S[0].sell_explicit && S[i].bandwidth == S[0].bandwidth);
    CHECK(B[i].built && B[i].nd == B[0].nd && B[i].nup == B[0].nup && B[i].ld == B[0].ld &&
          B[i].mask_bytes == B[0].mask_bytes);
    CHECK(std::memcmp(B[i].off, B[0].off, sizeof(B[0].off)) == 0 && std::memcmp(B[i].dj, B[0].dj, sizeof(B[0].dj)) == 0);
    CHECK(same_bits(B[i].val, B[0].val) && B[i].mask8 == B[0].mask8 && B[i].mask32 == B[0].mask32);
    CHECK(B[i].uniform == B[0].uniform && std::memcmp(B[i].uc, B[0].uc, sizeof(B[0].uc)) == 0);
    CHECK(B[i].geo == B[0].geo && B[i].box27 == B[0].box27 && B[i].gx == B[0].gx && B[i].gy == B[0].gy &&
          B[i].gz == B[0].gz && B[i].gz0 == B[0].gz0);
  }
  check_band(sh, A, B[1]);
}

// ---- (j) validate_csr, diag_share ---------------------------------------------------------------------
static int validate_code(const std::vector<i64> &rp, const std::vector<i32> &c, i64 ncols, std::string &text)
{
  try
  {
    validate_csr((i64)rp.size() - 1, ncols, rp.data(), c.data());
  }
  catch (const Error &e)
  {
    text = e.what();
    return e.code;
  }
  return EIG_OK;
}
static void test_validate_diag()
{
  std::string text;
  // rows {0, 2}, {1}, {0, 1}: the last row stores no diagonal
  const std::vector<i64> rp = {0, 2, 3, 5};
  const std::vector<i32> c = {0, 2, 1, 0, 1};
  const std::vector<double> v = {1.5, 9.0, 2.25, 9.0, 9.0};
  CHECK(validate_code(rp, c, 3, text) == EIG_OK);
  CHECK(validate_code(rp, {0, 2, 1, 1, 0}, 3, text) == EIG_ERR_ARG && text == "columns must be strictly ascending per row");
  CHECK(validate_code(rp, c, 2, text) == EIG_ERR_SHAPE && text == "column index out of range");
  CHECK(validate_code({1, 2, 3, 5}, c, 3, text) == EIG_ERR_ARG && text == "rowptr[0] must be 0");
  CHECK(validate_code({0, 2, 1, 5}, c, 3, text) == EIG_ERR_ARG && text == "rowptr must be non-decreasing");
  const DiagShare d = diag_share(1, 1, 3, 0, rp.data(), c.data(), v.data());
  CHECK(d.sum == 3.75 && d.count == 2);
  // the same rows as global rows 1 .. 3: none stores its diagonal
  const DiagShare s = diag_share(1, 1, 3, 1, rp.data(), c.data(), v.data());
  CHECK(s.sum == 0.0 && s.count == 0);
  // one 2 x 2 block on the diagonal: its scalar diagonal
  const std::vector<i64> brp = {0, 1};
  const std::vector<i32> bc = {0};
  const std::vector<double> bv = {1.0, 2.0, 3.0, 4.0};
  const DiagShare b = diag_share(2, 2, 1, 0, brp.data(), bc.data(), bv.data());
  CHECK(b.sum == 5.0 && b.count == 2);
}

int main()
{
  test_sell();
  test_stencil();
  test_band();
  test_refusals();
  test_uniform();
  test_geo();
  test_box27();
  test_split();
  test_threads();
  test_validate_diag();
  if (failures)
  {
    std::printf("%d check(s) FAILED\n", failures);
    return 1;
  }
  std::printf("ALL OK\n");
  return 0;
}
