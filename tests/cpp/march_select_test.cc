// Host-side unit checks of the plane-march variant table (csrc/march_variants.h) and of the selection and
// planning (csrc/march_plan.cpp, compiled with this file: march_select / kuhn_variant / march_plan /
// marchg_plan / lanczos_kernel_info / kernel_for).  No GPU and no library: plain host code.
//  * the traits of every variant against literal lists (waves, family arguments, pack, byte model);
//  * the P1 Kuhn value-pack variants read the pack through one 32-bit buffer descriptor of 64 B per
//    row, so a grid with sym_ld * 64 >= 2^31 (2^25 rows and more) must take the band arrays (12);
//  * for every image class, tune value 0..18 and both launch kinds the variant march_select returns,
//    and that it is valid, dispatched and has its family's preconditions met on the image;
//  * the plans of march_plan (runs, items, variant, stores, direction, body, line groups, planes, far spans)
//    and marchg_plan, and the kernel names and byte counts of the queries, against literals.
#include <cstdio>
#include <initializer_list>

#include <string>

#include "../../dune-eigensolver_amd/csrc/internal.h"
#include "../../dune-eigensolver_amd/csrc/march_plan.h"
#include "../../dune-eigensolver_amd/csrc/march_variants.h"

using namespace eigmi;

// The box-image queries of kernel_for live with their kernels (k_box.hip); this program is march_plan.cpp and
// this file alone, and its images are no box images.
namespace eigmi {
bool box_prepare(const eig_mat_s &) { return false; }
int box_cols(const eig_mat_s &) { return 32; }
}  // namespace eigmi

// ---- the table ---------------------------------------------------------------------------------
constexpr bool in(int v, std::initializer_list<int> l)
{
  for (int x : l)
    if (x == v) return true;
  return false;
}
constexpr std::initializer_list<int> kLive = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 14, 15, 16, 18, 19, 20, 22, 23, 24};
constexpr bool validity_ok()
{
  for (int v = -3; v < 40; ++v)
    if (march_traits(v).valid != in(v, kLive) || march_in_dispatch(v) != in(v, kLive)) return false;
  return true;
}
static_assert(validity_ok(), "valid variants");
static_assert(!march_traits(13).valid && !march_traits(17).valid && !march_traits(21).valid &&
                  !march_traits(-1).valid && !march_traits(25).valid,
              "13, 17, 21 and out-of-range numbers are no variants");
static_assert(MarchDispatch::size() == 22, "dispatch list");

constexpr bool waves_ok()
{
  for (int v : kLive)
  {
    const int fused = in(v, {0, 3, 7, 18}) ? 7 : in(v, {1, 2}) ? 8 : in(v, {4, 8, 10, 14, 15, 24}) ? 6
                    : in(v, {5, 11, 12, 19, 22}) ? 5 : in(v, {6, 9, 16, 20, 23}) ? 4 : -1;
    const int mv = in(v, {12, 16, 19, 20, 22, 23, 24}) ? 5 : 8;
    if (march_traits(v).fused_waves != fused || march_traits(v).mv_waves != mv) return false;
  }
  return true;
}
static_assert(waves_ok(), "launch-bounds waves");

constexpr bool geo_is(int v, MarchFamily f, int pf, bool pg, int val)
{
  const MarchTraits t = march_traits(v);
  return t.family == f && t.pf == pf && t.pg == pg && t.val == val;
}
constexpr bool kuhn_is(int v, bool kp, bool lx)
{
  const MarchTraits t = march_traits(v);
  return t.family == kMarchKuhn && t.kp == kp && t.lx == lx;
}
static_assert(march_traits(0).family == kMarchMasked && march_traits(1).family == kMarchMasked &&
                  march_traits(2).family == kMarchMasked, "masked body");
static_assert(geo_is(3, kMarchGeo, 0, false, 0) && geo_is(4, kMarchGeo, 1, false, 0) &&
                  geo_is(5, kMarchGeo, 2, false, 0) && geo_is(6, kMarchGeo, 2, true, 0), "geo <PF, PG>");
static_assert(geo_is(7, kMarchGeo2, 0, false, 0) && geo_is(8, kMarchGeo2, 1, false, 0) &&
                  geo_is(9, kMarchGeo2, 2, true, 0), "geo2 <PF, PG, 0>");
static_assert(geo_is(10, kMarchGeo2, 0, false, 1) && geo_is(11, kMarchGeo2, 0, false, 2) &&
                  geo_is(14, kMarchGeo2, 0, false, 4) && geo_is(15, kMarchGeo2, 0, false, 5) &&
                  geo_is(18, kMarchGeo2, 0, false, 5), "geo2 <0, false, VAL>");
static_assert(kuhn_is(12, false, false) && kuhn_is(16, true, false) && kuhn_is(19, true, false) &&
                  kuhn_is(20, true, true), "Kuhn <KP, LX>");
static_assert(march_traits(22).family == kMarchGeo2L2 && march_traits(23).family == kMarchGeo2L2 &&
                  march_traits(24).family == kMarchGeo2L2, "two-line march");

constexpr bool classes_ok()
{
  for (int v : kLive)
  {
    const MarchTraits t = march_traits(v);
    if (t.needs_pack() != in(v, {15, 16, 18, 19, 20, 22, 23, 24})) return false;
    // byte model: 1..9 stream no band array, the 7-point pack marches 4, everything else all of them
    const int arrays = in(v, {1, 2, 3, 4, 5, 6, 7, 8, 9}) ? 0 : in(v, {15, 18, 22, 23, 24}) ? 4 : 8;
    if (t.stream_arrays(8) != arrays) return false;
    if (t.geo_masks != !in(v, {0, 1})) return false;             // loaded masks: 0 and 1
    if (t.whole_planes() != !in(v, {0, 1, 2})) return false;     // formerly "variant >= 3"
    if (t.geo2_path() != !in(v, {0, 1, 2, 3, 4, 5, 6})) return false;  // formerly "variant >= 7"
    if ((t.values == kMarchUniform) != in(v, {1, 2, 3, 4, 5, 6, 7, 8, 9})) return false;
    // template head: <uint32_t, false> for Kuhn, <uint8_t, true> otherwise
    const bool kuhn = in(v, {12, 16, 19, 20});
    if (t.mask_bytes() != (kuhn ? 4 : 1) || t.span1() != !kuhn || t.any_head() != (v == 0)) return false;
    // march_plan's rules
    if (t.wide_runs != (in(v, {0, 1, 2, 3, 4, 5, 6, 8, 9}) ? 6 : 8)) return false;
    if (t.wide_two != in(v, {12, 16, 19, 20, 15, 22, 23, 24})) return false;
    if (t.line_groups != in(v, {10, 11, 14, 15})) return false;
    if (t.down_body != in(v, {22, 23}) || t.pipe_body != in(v, {22, 23})) return false;
  }
  return true;
}
static_assert(classes_ok(), "pack, byte-model class, masks, paths, template head, run-count rules");

// ---- the selection -----------------------------------------------------------------------------
static int bad = 0;

// an nx x ny x nz grid image: 7-point (nd = 7), the 2-D 5-point band of nx-row planes (nd = 5) or
// the P1 Kuhn 15-point box (nd = 15); one ghost plane either side in the window
static eig_mat_s grid_image(int nx, int ny, int nz, int nd)
{
  eig_mat_s A;
  const int D = nx * ny;
  A.nb_rows = (long long)D * nz;
  A.sym_ld = A.window = A.nb_rows + 2LL * D;
  A.sym_gx = nx, A.sym_gy = ny, A.sym_gz = nz;
  A.sym_nd = nd;
  if (nd == 15)
  {
    A.sym_box27 = kKuhn15;
    A.sym_mask_bytes = 4;
    A.sym_nup = 8;
    int k = 0;
    for (int q = 0; q < 27; ++q)
      if (kKuhn15 >> q & 1u) A.sym_off[k++] = (q / 9 - 1) * D + ((q / 3) % 3 - 1) * nx + (q % 3 - 1);
  }
  else
  {
    const int off7[7] = {-D, -nx, -1, 0, 1, nx, D}, off5[5] = {-D, -1, 0, 1, D};
    for (int k = 0; k < nd; ++k) A.sym_off[k] = nd == 7 ? off7[k] : off5[k];
    A.sym_mask_bytes = 1;
    A.sym_nup = (nd + 1) / 2;
    A.sym_geo = true;
  }
  for (int k = 0; k < nd; ++k) A.sym_dj[k] = k < nd / 2 ? nd / 2 - k : k - nd / 2;
  return A;
}

// what every returned variant must satisfy on its image
static bool preconditions(const eig_mat_s &A, int v)
{
  const MarchTraits t = march_traits(v);
  if (!t.valid || !march_in_dispatch(v)) return false;
  const long long two31 = 1LL << 31;
  if (t.family == kMarchKuhn && A.sym_box27 != kKuhn15) return false;
  if (t.geo2_path() && !(A.sym_gx % 64 == 0 && A.window * 16 < two31)) return false;
  if (t.family == kMarchGeo2L2 && !(A.sym_nd == 7 && A.sym_gy > 0 && A.sym_gy % 2 == 0)) return false;
  if (t.needs_pack() && !(A.sym_ld * (t.family == kMarchKuhn ? 64 : 32) < two31)) return false;
  if (t.values == kMarchUniform && !(A.sym_uniform && !(A.kflags & EIG_MAT_NO_UNIFORM))) return false;
  if (t.geo_masks && t.family != kMarchKuhn && !A.sym_geo) return false;
  return true;
}

// want_fused / want_mv: the variant for tune values 0 .. 18
static void expect_table(const char *name, eig_mat_s A, const int (&want_fused)[19], const int (&want_mv)[19],
                         bool distributed = false)
{
  for (int fused = 0; fused < 2; ++fused)
    for (int tune = 0; tune <= 18; ++tune)
    {
      A.tune_march_prefetch = tune;
      const int got = march_select(A, fused != 0, distributed), want = fused ? want_fused[tune] : want_mv[tune];
      if (got != want || !preconditions(A, got))
      {
        std::printf("%s, tune %d, %s: variant %d, want %d%s\n", name, tune, fused ? "fused" : "eig_mv", got, want,
                    preconditions(A, got) ? "" : " (preconditions not met)");
        ++bad;
      }
    }
}

static void test_selection()
{
  // tune value:                 0   1   2   3   4   5   6   7   8   9  10  11  12  13  14  15  16  17  18
  const int all1[19] =          {1,  1,  1,  1,  1,  1,  1,  1,  1,  1,  1,  1,  1,  1,  1,  1,  1,  1,  1};
  const int uni_geo2[19] =      {7,  2,  3,  4,  5,  6,  7,  8,  9,  7,  7,  7,  7,  7,  7,  7,  7,  7,  7};
  const int uni_other[19] =     {4,  2,  3,  4,  5,  6,  3,  4,  6,  4,  4,  4,  4,  4,  4,  4,  4,  4,  4};
  const int val7_fused[19] =    {15, 0, 15, 15, 15, 15, 15, 15, 15, 10, 11, 15, 14, 15, 15, 18, 22, 23, 24};
  const int val7_mv[19] =       {0,  0,  0,  0,  0,  0,  0,  0,  0, 10, 11,  0, 14, 15,  0, 18, 22, 23, 24};
  const int val7odd_fused[19] = {15, 0, 15, 15, 15, 15, 15, 15, 15, 10, 11, 15, 14, 15, 15, 18, 15, 15, 15};
  const int val7odd_mv[19] =    {0,  0,  0,  0,  0,  0,  0,  0,  0, 10, 11,  0, 14, 15,  0, 18, 15, 15, 15};
  const int val7big_fused[19] = {22, 0, 22, 22, 22, 22, 22, 22, 22, 10, 11, 22, 14, 15, 22, 18, 22, 23, 24};
  const int val5_fused[19] =    {10, 0, 10, 10, 10, 10, 10, 10, 10, 10, 11, 10, 14, 15, 10, 18, 15, 15, 15};
  const int val5_mv[19] =       {0,  0,  0,  0,  0,  0,  0,  0,  0, 10, 11,  0, 14, 15,  0, 18, 15, 15, 15};
  const int kuhn[19] =          {20, 0, 20, 20, 20, 20, 20, 20, 20, 20, 20, 20, 20, 16, 12, 19, 20, 20, 20};
  const int kuhn_gy6[19] =      {16, 0, 16, 16, 16, 16, 16, 16, 16, 16, 16, 16, 16, 16, 12, 19, 16, 16, 16};
  const int all0[19] =          {0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0};

  eig_mat_s A = grid_image(64, 64, 64, 7);
  A.sym_uniform = true;
  A.sym_geo = false;
  expect_table("uniform, not geometric", A, all1, all1);
  A.sym_geo = true;
  expect_table("uniform geometric 64^3", A, uni_geo2, uni_geo2);
  A.kflags |= EIG_MAT_NO_UNIFORM;  // the array loads kept: a value image
  expect_table("uniform 64^3 with EIG_MAT_NO_UNIFORM", A, val7_fused, val7_mv);
  A = grid_image(24, 24, 24, 7);
  A.sym_uniform = true;
  expect_table("uniform geometric 24^3", A, uni_other, uni_other);
  // the tune values that name value marches take the automatic variant on uniform images
  for (const eig_mat_s &U : {grid_image(64, 64, 64, 7), grid_image(24, 24, 24, 7)})
    for (int fused = 0; fused < 2; ++fused)
      for (int tune = 9; tune <= 18; ++tune)
      {
        eig_mat_s B = U;
        B.sym_uniform = true;
        const int automatic = march_select(B, fused != 0, false);
        B.tune_march_prefetch = tune;
        if (march_select(B, fused != 0, false) != automatic || automatic != (U.sym_gx == 64 ? 7 : 4))
        {
          std::printf("uniform nx %d, tune %d: not the automatic variant\n", U.sym_gx, tune);
          ++bad;
        }
      }

  expect_table("value 64^3", grid_image(64, 64, 64, 7), val7_fused, val7_mv);
  expect_table("value 64 x 63 x 64", grid_image(64, 63, 64, 7), val7odd_fused, val7odd_mv);
  A = grid_image(256, 256, 64, 7);
  if (A.nb_rows < EIG_MARCH_2L_MIN_ROWS) ++bad, std::printf("256 x 256 x 64 is below EIG_MARCH_2L_MIN_ROWS\n");
  expect_table("value 256 x 256 x 64", A, val7big_fused, val7_mv);
  expect_table("value 5-point 64 x 64", grid_image(64, 1, 64, 5), val5_fused, val5_mv);
  expect_table("value 24^3 (no geo2 grid)", grid_image(24, 24, 24, 7), all0, all0);

  expect_table("Kuhn 64^3", grid_image(64, 64, 64, 15), kuhn, kuhn);
  expect_table("Kuhn 64 x 6 x 64", grid_image(64, 6, 64, 15), kuhn_gy6, kuhn_gy6);
  expect_table("Kuhn 64^3, distributed", grid_image(64, 64, 64, 15), all0, all0, true);
}

// ---- the Kuhn pack's descriptor guard ----------------------------------------------------------
static void test_kuhn_pack_guard()
{
  auto expect = [&](long long ld, int tune, int want, int gy = 256) {
    eig_mat_s A;
    A.sym_ld = ld;
    A.sym_gy = gy;
    A.tune_march_prefetch = tune;
    const int got = eigmi::kuhn_variant(A);
    if (got != want)
    {
      std::printf("sym_ld %lld tune %d: variant %d, want %d\n", ld, tune, got, want);
      ++bad;
    }
  };
  const long long n256 = 256LL * 256 * 256, n448 = 448LL * 448 * 448, nwrap = 256LL * 512 * 512;
  expect(n256, 0, 20);       // the pack with the line exchange in LDS (lines in groups of 4)
  expect(n256, 0, 16, 254);  // lines not a multiple of 4: the pack alone
  expect(n256, 13, 16);
  expect(n256, 15, 19);
  expect(n256, 14, 12);
  expect((1LL << 25) - 1, 0, 20);
  expect(1LL << 25, 0, 12);  // 64 B * 2^25 = 2^31: the descriptor's record count no longer fits
  expect(n448, 0, 12);
  expect(n448, 15, 12);
  expect(nwrap, 0, 12);      // 64 * 2^26 = 2^32: would wrap to a zero-sized descriptor
  // the same through march_select on a whole Kuhn image of 2^25 rows and more
  eig_mat_s A;
  A.sym_box27 = kKuhn15;
  A.sym_nd = 15;
  A.sym_gx = 512, A.sym_gy = 256, A.sym_gz = 256;
  A.nb_rows = A.window = A.sym_ld = 1LL << 25;
  for (int tune : {0, 13, 15})
  {
    A.tune_march_prefetch = tune;
    const int got = march_select(A, true, false);
    if (got != 12 || !preconditions(A, got)) ++bad, std::printf("Kuhn 2^25 rows, tune %d: variant %d, want 12\n", tune, got);
  }
}

// ---- the plans ---------------------------------------------------------------------------------
// march_plan, marchg_plan and the kernel queries on images built as above, on a 256-CU device and one rank.
// Every literal below is what the planning code computed before it moved out of k_spmv.hip.
static double band_values[1];  // the plans only form addresses from sym_val
static eig_ctx_s ctx256;

static eig_mat_s plan_image(int nx, int ny, int nz, int nd)
{
  eig_mat_s A = grid_image(nx, ny, nz, nd);
  ctx256.num_cu = 256;
  A.ctx = &ctx256;
  A.sym_val = band_values;
  A.nslices = (A.nb_rows + 63) / 64;
  return A;
}
static eig_mat_s uniform_image(int nx, int ny, int nz)
{
  eig_mat_s A = plan_image(nx, ny, nz, 7);
  A.sym_uniform = true;
  const double uc[4] = {6.0, -1.0, -2.0, -3.0};  // the arrays of the offsets 0, +1, +nx, +D
  for (int j = 0; j < 4; ++j) A.sym_uc[j] = uc[j];
  return A;
}

struct WantPlan {
  int nseg, ncol, uni, tstore, down, pipe, lines;
  long long zb, nplanes, D;
  int dn, dq;
};
static void expect_plan(const char *name, const MarchPlan &mp, const WantPlan &w)
{
  const bool ok = mp.nseg == w.nseg && mp.ncol == w.ncol && mp.uni == w.uni && mp.tstore == w.tstore &&
                  mp.down == w.down && mp.pipe == w.pipe && mp.lines == w.lines && mp.zb == w.zb &&
                  mp.nplanes == w.nplanes && mp.D == w.D && mp.dn == w.dn && mp.dq == w.dq && mp.pack == nullptr;
  if (ok) return;
  std::printf("%s: plan {%d, %d, %d, %d, %d, %d, %d, %lld, %lld, %lld, %d, %d}%s\n", name, mp.nseg, mp.ncol, mp.uni,
              mp.tstore, mp.down, mp.pipe, mp.lines, (long long)mp.zb, (long long)mp.nplanes, (long long)mp.D,
              (int)mp.dn, (int)mp.dq, mp.pack ? " with a pack" : "");
  ++bad;
}
// a plan that does not march is all zeros
static const WantPlan kNoPlan = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};

static void test_plans()
{
  // value 7-point 256^3, fused: the 2-line march on two runs of line pairs, 256 workgroups = num_cu: pipelined
  eig_mat_s A = plan_image(256, 256, 256, 7);
  expect_plan("value 256^3 fused", march_plan(A, kSymN8, 0, -1, true), {2, 512, 22, 0, 0, 1, 0, 0, 256, 65536, -256, 256});
  expect_plan("value 256^3 eig_mv", march_plan(A, kSymN8), {8, 1024, 0, 0, 0, 0, 0, 0, 256, 65536, -256, 256});
  ctx256.num_cu = 255;
  expect_plan("value 256^3 fused, 255 CUs", march_plan(A, kSymN8, 0, -1, true),
              {2, 512, 22, 0, 0, 0, 0, 0, 256, 65536, -256, 256});
  ctx256.num_cu = 256;
  A.tune_cache = 32;
  expect_plan("value 256^3 fused, cache 32", march_plan(A, kSymN8, 0, -1, true),
              {2, 512, 22, 0, 0, 0, 0, 0, 256, 65536, -256, 256});
  A.tune_cache = 16;
  expect_plan("value 256^3 fused, cache 16", march_plan(A, kSymN8, 0, -1, true),
              {2, 512, 22, 0, 1, 1, 0, 0, 256, 65536, -256, 256});
  A.tune_cache = 1;
  expect_plan("value 256^3 fused, cache 1", march_plan(A, kSymN8, 0, -1, true),
              {2, 512, 22, 1, 0, 1, 0, 0, 256, 65536, -256, 256});
  A.tune_cache = 0;
  // EIG_TUNE_MARCH_RUNS: taken as it is, lowered to what kMaxRedBlocks workgroups hold, never past the planes
  A.tune_march_prefetch = 13;  // variant 15: 1024 items per run
  A.tune_march_runs = 64;
  expect_plan("value 256^3 fused, variant 15, 64 runs asked", march_plan(A, kSymN8, 0, -1, true),
              {8, 1024, 15, 0, 0, 0, 0, 0, 256, 65536, -256, 256});
  A.tune_march_runs = 5;
  expect_plan("value 256^3 fused, variant 15, 5 runs asked", march_plan(A, kSymN8, 0, -1, true),
              {5, 1024, 15, 0, 0, 0, 0, 0, 256, 65536, -256, 256});
  A.tune_march_prefetch = 0;
  A.tune_march_runs = 1000;
  expect_plan("value 256^3 fused, 1000 runs asked", march_plan(A, kSymN8, 0, -1, true),
              {16, 512, 22, 0, 0, 0, 0, 0, 256, 65536, -256, 256});
  A.tune_march_runs = 0;
  A.kflags |= EIG_MAT_NO_MARCH;
  expect_plan("value 256^3 fused, EIG_MAT_NO_MARCH", march_plan(A, kSymN8, 0, -1, true), kNoPlan);
  A.kflags = 0;
  expect_plan("value 256^3 on the gather image mode", march_plan(A, kSym8, 0, -1, true), kNoPlan);

  // below EIG_MARCH_PIPE_MIN_ROWS the automatic 2-line march keeps the plain bodies; asked for, it pipelines
  A = plan_image(256, 256, 64, 7);
  expect_plan("value 256 x 256 x 64 fused", march_plan(A, kSymN8, 0, -1, true),
              {2, 512, 22, 0, 0, 0, 0, 0, 64, 65536, -256, 256});
  A.tune_march_prefetch = 16;
  expect_plan("value 256 x 256 x 64 fused, variant 22 asked", march_plan(A, kSymN8, 0, -1, true),
              {2, 512, 22, 0, 0, 1, 0, 0, 64, 65536, -256, 256});

  A = plan_image(128, 128, 128, 7);
  expect_plan("value 128^3 fused", march_plan(A, kSymN8, 0, -1, true), {8, 256, 15, 1, 0, 0, 0, 0, 128, 16384, -128, 128});
  expect_plan("value 128^3 eig_mv", march_plan(A, kSymN8), {32, 256, 0, 0, 0, 0, 0, 0, 128, 16384, -128, 128});
  A.tune_march_prefetch = 16;  // the 2-line march on narrow planes: twice the runs of line pairs
  expect_plan("value 128^3 fused, variant 22 asked", march_plan(A, kSymN8, 0, -1, true),
              {16, 128, 22, 1, 0, 0, 0, 0, 128, 16384, -128, 128});

  A = uniform_image(256, 256, 256);
  expect_plan("uniform 256^3 fused", march_plan(A, kSymN8, 0, -1, true), {8, 1024, 7, 0, 0, 0, 0, 0, 256, 65536, -256, 256});
  {
    const MarchPlan mp = march_plan(A, kSymN8, 0, -1, true);
    if (mp.cD != -3.0 || mp.c0 != 6.0 || mp.c1 != -1.0 || mp.cn != -2.0 || mp.cq != -2.0 || mp.gx != 256 || mp.gz != 256)
      ++bad, std::printf("uniform 256^3: constants %g %g %g %g %g, grid %d %d\n", mp.cD, mp.c0, mp.c1, mp.cn, mp.cq, mp.gx, mp.gz);
  }

  A = plan_image(256, 256, 256, 15);
  expect_plan("Kuhn 256^3 eig_mv", march_plan(A, kSymN32), {2, 1024, 20, 0, 0, 0, 0, 0, 256, 65536, -65792, 256});
  expect_plan("Kuhn 256^3 fused", march_plan(A, kSymN32, 0, -1, true), {2, 1024, 20, 0, 0, 0, 0, 0, 256, 65536, -65792, 256});
  {
    // band array of every upper box offset, -1 where the Kuhn stencil stores none
    const MarchPlan mp = march_plan(A, kSymN32);
    const int kj[14] = {0, 1, -1, 2, 3, -1, -1, -1, -1, 4, 5, -1, 6, 7};
    for (int q = 13; q < 27; ++q)
      if (mp.kj[q] != kj[q - 13]) ++bad, std::printf("Kuhn 256^3: kj[%d] = %d, want %d\n", q, mp.kj[q], kj[q - 13]);
  }

  A = plan_image(64, 64, 64, 7);
  A.tune_march_lines = 4;
  expect_plan("value 64^3 fused, line groups", march_plan(A, kSymN8, 0, -1, true), {32, 64, 15, 1, 0, 0, 4, 0, 64, 4096, -64, 64});
  A.tune_march_prefetch = 15;
  expect_plan("value 64^3 fused, variant 18, line groups asked", march_plan(A, kSymN8, 0, -1, true),
              {32, 64, 18, 1, 0, 0, 0, 0, 64, 4096, -64, 64});
  A.tune_march_prefetch = 16;
  A.tune_march_lines = 0;
  A.tune_cache = 64;  // the pipelined body wherever it can run
  expect_plan("value 64^3 fused, variant 22, cache 64", march_plan(A, kSymN8, 0, -1, true),
              {64, 32, 22, 1, 0, 1, 0, 0, 64, 4096, -64, 64});
  A.tune_cache = 0;
  A.tune_march_prefetch = 0;
  // interior planes of a slab: from 2 planes on
  expect_plan("value 64^3 fused, planes [1, 3)", march_plan(A, kSymN8, 1, 3, true), {2, 64, 15, 1, 0, 0, 0, 1, 2, 4096, -64, 64});
  expect_plan("value 64^3 eig_mv, planes [1, 3)", march_plan(A, kSymN8, 1, 3), {2, 64, 0, 0, 0, 0, 0, 1, 2, 4096, -64, 64});
  expect_plan("value 64^3 fused, planes [1, 2)", march_plan(A, kSymN8, 1, 2, true), kNoPlan);
  // the SpMM march: 16-row columns
  expect_plan("value 64^3, chunk 16", march_plan(A, kSymN8, 0, -1, false, 16), {32, 256, 0, 0, 0, 0, 0, 0, 64, 4096, -64, 64});
  // a whole matrix marches from 4 planes on
  A = plan_image(64, 64, 3, 7);
  expect_plan("value 64 x 64 x 3 fused", march_plan(A, kSymN8, 0, -1, true), kNoPlan);
  expect_plan("value 64 x 64 x 3 eig_mv", march_plan(A, kSymN8), kNoPlan);
}

static void test_marchg_plan()
{
  // the Kuhn band: the carried offset is the widest multiple of 16 whose four spans hold at most kGSpan offsets
  eig_mat_s A = plan_image(64, 64, 64, 15);
  MarchPlan mp;
  GSpans sp;
  const bool ok = marchg_plan(A, mp, sp);
  const int want[10] = {3, 11, 0, 3, 4, 6, 9, 11, 12, 15};
  const int got[10] = {sp.kPm, sp.kPp, sp.s1b, sp.s1e, sp.s2b, sp.s2e, sp.s3b, sp.s3e, sp.s4b, sp.s4e};
  bool same = ok;
  for (int k = 0; k < 10; ++k) same = same && got[k] == want[k];
  if (!same || mp.D != 4096 || mp.ncol != 256 || mp.nseg != 24 || mp.nplanes != 64 || mp.zb != 0 || mp.mrows != 64 * 4096)
  {
    ++bad;
    std::printf("marchg Kuhn 64^3: %d, P %lld ncol %d nseg %d nplanes %lld mrows %lld, spans", (int)ok, (long long)mp.D,
                mp.ncol, mp.nseg, (long long)mp.nplanes, (long long)mp.mrows);
    for (int k = 0; k < 10; ++k) std::printf(" %d", got[k]);
    std::printf("\n");
  }
  // the same band without its -1 offset does not qualify
  for (int k = 6; k < 14; ++k) A.sym_off[k] = A.sym_off[k + 1], A.sym_dj[k] = A.sym_dj[k + 1];
  A.sym_nd = 14;
  if (A.sym_off[6] != 0 || marchg_plan(A, mp, sp)) ++bad, std::printf("marchg: a band without -1 qualified\n");
  A = plan_image(64, 64, 64, 15);
  A.kflags |= EIG_MAT_NO_MARCH;
  if (marchg_plan(A, mp, sp)) ++bad, std::printf("marchg: EIG_MAT_NO_MARCH ignored\n");
}

static void expect_info(const char *name, const eig_mat_s &A, bool fused, const char *want_name, long long want_bytes)
{
  std::string got;
  i64 bytes = 0;
  lanczos_kernel_info(A, fused, got, bytes);
  if (got != want_name || bytes != want_bytes || kernel_for(A, fused ? 2 : 1) != want_name)
    ++bad, std::printf("%s: %s, %lld bytes\n", name, got.c_str(), (long long)bytes);
}

static void test_kernel_info()
{
  const long long n256 = 256LL * 256 * 256;
  eig_mat_s A = plan_image(256, 256, 256, 7);
  expect_info("value 256^3 fused", A, true, "k_lanczos_fused_march", 8 * 4 * n256 + 32 * n256);    // the pack's 4 arrays
  expect_info("value 256^3 K1", A, false, "k_lanczos_spmv_march", 8 * 4 * n256 + n256 + 24 * n256);  // arrays and masks
  if (kernel_for(A, 0) != "k_spmv_march" || kernel_for(A, 3) != "k_spmm8_march" || kernel_for(A, 4) != "k_spmm8_marchg_cheb")
    ++bad, std::printf("value 256^3: %s %s %s\n", kernel_for(A, 0).c_str(), kernel_for(A, 3).c_str(), kernel_for(A, 4).c_str());
  A.kflags |= EIG_MAT_NO_MARCH;
  expect_info("value 256^3 fused, no march", A, true, "k_lanczos_fused_b1", 8 * 4 * n256 + n256 + 32 * n256);
  expect_info("value 256^3 K1, no march", A, false, "k_lanczos_spmv_b1", 8 * 4 * n256 + n256 + 24 * n256);
  if (kernel_for(A, 0) != "k_spmv_b1" || kernel_for(A, 3) != "k_sell_mv8g" || kernel_for(A, 4) != "k_sell_mv8q_cheb")
    ++bad, std::printf("value 256^3, no march: %s %s %s\n", kernel_for(A, 0).c_str(), kernel_for(A, 3).c_str(), kernel_for(A, 4).c_str());
  A = uniform_image(256, 256, 256);
  expect_info("uniform 256^3 fused", A, true, "k_lanczos_fused_march", 32 * n256);  // the vectors alone
  expect_info("uniform 256^3 K1", A, false, "k_lanczos_spmv_march", 24 * n256);
  A = plan_image(256, 256, 256, 15);
  expect_info("Kuhn 256^3 fused", A, true, "k_lanczos_fused_march", 8 * 8 * n256 + 32 * n256);
  expect_info("Kuhn 256^3 K1", A, false, "k_lanczos_spmv_march", 8 * 8 * n256 + 24 * n256);
  if (kernel_for(A, 3) != "k_spmm8_marchg") ++bad, std::printf("Kuhn 256^3 SpMM: %s\n", kernel_for(A, 3).c_str());
  // the queries build nothing
  if (march_variant(A, true) != 20 || march_pipe(A) != 0 || A.sym_pack) ++bad, std::printf("Kuhn 256^3: queries\n");
  A = plan_image(256, 256, 256, 7);
  if (march_variant(A, true) != 22 || march_variant(A, false) != 0 || march_pipe(A) != 1 || march_split_active(A) || A.sym_pack)
    ++bad, std::printf("value 256^3: queries\n");
}

int main()
{
  test_kuhn_pack_guard();
  test_selection();
  test_plans();
  test_marchg_plan();
  test_kernel_info();
  std::printf(bad ? "FAILED\n" : "ALL OK\n");
  return bad ? 1 : 0;
}
