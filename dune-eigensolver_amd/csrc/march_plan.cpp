// march_plan.cpp -- host side of the plane march (kernels: k_march.hip): does an image march, which variant
// (march_variants.h) runs, with how many plane runs, in which direction, with which body and cache policy;
// the byte model and the kernel-name queries.  Plain C++: every function reads a matrix's host-side fields
// (and its context's num_cu / distributed()) and nothing else -- no allocation, no launch, no device access --
// so tests/cpp/march_select_test.cc runs all of it without a GPU.
#include "march_plan.h"

#include <algorithm>
#include <iterator>

namespace eigmi {

// Band-image kernels on this matrix: 0 = none (the SELL / stencil kernels: EIG_MAT_NO_BAND), 1 =
// every offset through its own gather (EIG_MAT_BAND_GATHER), 2 = the lane-shift path (default).
int sym_kernels(const eig_mat_s &A)
{
  return (A.kflags & EIG_MAT_NO_BAND) ? 0 : (A.kflags & EIG_MAT_BAND_GATHER) ? 1 : 2;
}

bool is_sym_mode(int mode) { return mode >= kSym8; }

int image_mode(const eig_mat_s &A)
{
  const int sk = A.sym_val ? sym_kernels(A) : 0;
  if (sk)
  {
    bool near = false;  // offsets +-1 present: the lane-shift path applies
    for (int k = 0; k < A.sym_nd; ++k) near = near || A.sym_off[k] == 1 || A.sym_off[k] == -1;
    if (sk == 2 && near) return A.sym_mask_bytes == 1 ? kSymN8 : kSymN32;
    return A.sym_mask_bytes == 1 ? kSym8 : kSym32;
  }
  if (A.n_stencil_slices == 0) return kExplicit;
  return A.n_stencil_slices == A.nslices ? kStencil : kMixed;
}

// Band array of the offset a D + b nx + c at 27-box position q = (a + 1) 9 + (b + 1) 3 + (c + 1), -1
// when the band does not store it
int box_band_array(const eig_mat_s &A, i64 D, int q)
{
  const i64 off = (i64)(q / 9 - 1) * D + (i64)((q / 3) % 3 - 1) * A.sym_gx + (q % 3 - 1);
  for (int k = 0; k < A.sym_nd; ++k)
    if (A.sym_off[k] == off) return A.sym_dj[k];
  return -1;
}

// EIG_MAT_NO_MARCH: the plane-marching kernels are off for this matrix (the slice kernels run).
// (The general-band march -- SpMM of non-extreme carried bands, Chebyshev -- is a plane march too.)
bool march_enabled(const eig_mat_s &A) { return (A.kflags & EIG_MAT_NO_MARCH) == 0; }
// Far spans of the ascending offset list: the offsets [1, klo) lie in (-D, -1), [khi, nd - 1) in (+1, +D)
std::pair<int, int> far_spans(const eig_mat_s &A)
{
  int klo = A.sym_nd, khi = A.sym_nd;
  for (int k = A.sym_nd - 1; k >= 0; --k)
  {
    if (A.sym_off[k] >= -1) klo = k;
    if (A.sym_off[k] > 1) khi = k;
  }
  return {klo, khi};
}
// Far spans of at most one offset each (u8-mask bands only: at most 8 offsets, so (-D, -1) and
// (+1, +D) hold at most one offset each exactly when nd <= 7 with -1/0/+1 present).
bool march_span1(const eig_mat_s &A)
{
  const auto [klo, khi] = far_spans(A);
  return A.sym_mask_bytes == 1 && klo - 1 <= 1 && (A.sym_nd - 1) - khi <= 1;
}
// every vector a launch touches fits in half of the 256 MB MALL (MarchPlan::tstore)
bool vectors_fit_mall(const eig_mat_s &A) { return A.window * 16 * 3 <= (i64(128) << 20); }

// The Kuhn pack is read through one 32-bit buffer descriptor of 64 B per row: grids of 2^25 rows and
// more (e.g. 448^3, or 256 x 512 x 512, whose descriptor size would wrap to 0) take the arrays.
bool kuhn_pack_fits(const eig_mat_s &A) { return A.sym_ld * 64 < (i64(1) << 31); }
// The variant of an image the Kuhn march applies to.  On its value pack (16): fused step 256^3 346 us,
// eig_mv 292 us (the arrays, 12: 407 / 330 us; profiles/r04d_p1k.jsonl).  Default 20 (the line exchange
// in LDS) where the lines come in groups of 4: 256^3 fused step 333.2 vs 340.8 us, eig_mv 278.7 vs
// 292.2 us (profiles/r05g_p1k.jsonl).  Tune values: 13 = 16, 14 = the arrays, 15 = 19.
int kuhn_variant(const eig_mat_s &A)
{
  const int tp = A.tune_march_prefetch;
  if (tp == 14 || !kuhn_pack_fits(A)) return 12;
  if (tp == 15) return 19;
  return tp != 13 && A.sym_gy % 4 == 0 ? 20 : 16;
}

// The march variant (march_variants.h) of a launch on A: by image class, the automatic choice or what
// eig_mat_tune(EIG_TUNE_MARCH_PREFETCH) names, where the image meets that variant's preconditions.
int march_select(const eig_mat_s &A, bool fused, bool distributed)
{
  // by tune value; kAuto and every value past a table's end = the automatic choice
  constexpr int kAuto = -1;
  constexpr int kUniformGeo2[] = {kAuto, 2, 3, 4, 5, 6, 7, 8, 9}, kUniformGeo[] = {kAuto, 2, 3, 4, 5, 6, 3, 4, 6};
  constexpr int kValue[] = {kAuto, 0, kAuto, kAuto, kAuto, kAuto, kAuto, kAuto, kAuto, 10,
                            11,    kAuto, 14, 15, kAuto, 18, 22, 23, 24};
  const int tp = A.tune_march_prefetch;
  auto asked = [tp](const auto &table) { return tp >= 0 && tp < (int)std::size(table) ? table[tp] : kAuto; };
  // whole 64-x runs per wave and 32-bit byte offsets into the pair vectors (geo2 and Kuhn)
  const bool runs64 = A.sym_gx % 64 == 0 && A.window * 16 < (i64(1) << 31);
  // the P1 Kuhn 15-point image on one rank; tune value 1 = no Kuhn march
  if (A.sym_box27 == kKuhn15 && A.sym_nd == 15 && !distributed && runs64 && A.sym_ld * 8 < (i64(1) << 31) && tp != 1)
    return kuhn_variant(A);
  const bool geo2 = A.sym_geo && runs64;
  if (A.sym_uniform && !(A.kflags & EIG_MAT_NO_UNIFORM))
  {
    if (!A.sym_geo) return 1;
    // a geo2 request on a grid that does not qualify takes the march_rows_geo variant with its prefetches.
    // Automatic (measured: profiles/r03bj_march_variants.jsonl, r03bn_*, r03bp_*; tools/gpu.sh prefetch):
    // geo2 without prefetch (7) where the grid allows it -- fused step 256^3 125.8 us at 8 plane runs
    // (plain march 130.0), 128^3 20.1 us (plain 30.2; with the MALL-resident plain stores,
    // MarchPlan::tstore), one rank's 256^2 x 32 slab 20.5 us (plain 34.5); eig_mv 256^3 46.1 us (plain
    // 59.4), 128^3 8.0 (12.1).  The prefetching geo2 variants (8, 9) are within a few per cent either
    // way.  Grids geo2 does not take: march_rows_geo with the +D operand two planes ahead (4).
    const int v = geo2 ? asked(kUniformGeo2) : asked(kUniformGeo);
    return v != kAuto ? v : geo2 ? 7 : 4;
  }
  // value images (EIG_MAT_NO_UNIFORM keeps the array loads): geometric masks only on geo2 grids with
  // single-offset far spans and a pack descriptor (32 B per row) that fits
  if (!geo2 || !march_span1(A) || A.sym_ld * 32 >= (i64(1) << 31)) return 0;
  // two grid lines per wave: 7-point bands on grids of an even line count, else one line of the pack
  const bool two = A.sym_nd == 7 && A.sym_gy % 2 == 0 && A.sym_gy > 0;
  const int v = asked(kValue);
  if (v != kAuto) return march_traits(v).family == kMarchGeo2L2 && !two ? 15 : v;
  // automatic: the fused step on the value pack (15: 223.7 us at 256^3, one rank's 256^2 x 32 slab
  // 30.4 us; the arrays 226.8 / 31.7), eig_mv / K1 on the plain masked march (0: 152.1 us against 161.4 on
  // the pack): profiles/r04d_latency.jsonl, r04d_slab.jsonl; the 2-line march from EIG_MARCH_2L_MIN_ROWS
  // rows (kMarch2lDefault, march_plan.h)
  if (!fused) return 0;
  if (A.sym_nd != 7) return 10;
  return two && A.nb_rows >= EIG_MARCH_2L_MIN_ROWS && kMarch2lDefault ? 22 : 15;
}
int march_select(const eig_mat_s &A, bool fused) { return march_select(A, fused, A.ctx->distributed()); }

// The variant a launch runs on an image of mode `mode`: a Kuhn variant whatever the mode (its
// selection tested the image); every other variant needs u8 masks with single-offset far spans,
// and where the image lacks them the band-array march (variant 0) of its mask width runs.
int march_launch_variant(const eig_mat_s &A, int mode, int variant)
{
  if (march_traits(variant).family == kMarchKuhn) return variant;
  return mode == kSymN8 && march_span1(A) ? variant : 0;
}
unsigned march_grid(const MarchPlan &mp) { return (unsigned)((mp.ncol * (i64)mp.nseg + kWaves - 1) / kWaves); }

// Plane-marching plan for a whole-matrix launch on the lane-shift band image, or nseg = 0 when the
// band does not qualify: symmetric offset set with off[0] = -D, off[nd-1] = +D, D a multiple of 64,
// at least 4 planes.  Plane runs per column: enough items for one resident wave per SIMD slot
// (8 per SIMD), at most kMaxRedBlocks workgroups.
// Band geometry the march needs (independent of the matrix's kernel flags): widest offset D.
bool march_geometry(const eig_mat_s &A, i64 &D, int chunk)
{
  D = 0;
  if (!A.sym_val || A.sym_nd < 3) return false;
  bool near = false;
  for (int k = 0; k < A.sym_nd; ++k) near = near || A.sym_off[k] == 1 || A.sym_off[k] == -1;
  D = A.sym_off[A.sym_nd - 1];
  return near && D > 1 && D % chunk == 0 && A.sym_off[0] == -D;
}

// [zb, ze): plane range of a split launch (the interior planes of a distributed slab); ze < 0 =
// the whole matrix.
// chunk: rows per wave column (64 for the scalar kernels, 16 for the 8-column SpMM).
// MarchPlan::pack stays null: the launch paths (k_march.hip launch_plan, march_prepare) build the value pack
// the plan's variant streams and set it; a query leaves it unbuilt.
MarchPlan march_plan(const eig_mat_s &A, int mode, i64 zb, i64 ze, bool fused, int chunk)
{
  MarchPlan mp{};
  if (mode != kSymN8 && mode != kSymN32) return mp;
  i64 D;
  const int uni = march_select(A, fused);
  const MarchTraits T = march_traits(uni);
  const bool two_lines = T.family == kMarchGeo2L2;
  const bool kuhn = chunk == 64 && T.family == kMarchKuhn;
  if (!march_enabled(A) || !(kuhn ? (D = (i64)A.sym_gx * A.sym_gy) > 0 : march_geometry(A, D, chunk))) return mp;
  if (ze < 0) ze = (A.nb_rows + D - 1) / D;
  const i64 nplanes = ze - zb;
  if (nplanes < 2 || (zb == 0 && nplanes < 4)) return mp;
  const i64 ncol = D / chunk;
  // about one work item per resident wave slot (8 per SIMD)
  const i64 resident = 8LL * 4 * A.ctx->num_cu;  // waves
  i64 nseg = std::max<i64>(1, (resident + ncol - 1) / ncol);
  nseg = std::min<i64>(nseg, nplanes);
  // the fused step prefers longer plane runs (fewer fronts in the XCDs' L2 at once) wherever the
  // grid is small; measured with eig_mat_tune sweeps (tools/gpu.sh latency, profiles/r03h_latency):
  //  * wide planes (>= 1024 columns: 256^2 per plane): 256^3 8 runs 220.8 us (7: 224.6, 6: 232.5,
  //    4: 267.3); one rank's 256^2 x 32 slab 2 runs 33.7 us (4: 35.5, 7: 36.7, 1: 47.3); the 16-plane
  //    slab 2 runs 21.7 us (1: 28.3, 4: 23.9, 7: 26.2)  ->  nplanes / 32 runs, at least 2, at most 8
  //  * narrower planes (128^3: 256 columns): 12 runs 34.9 us (16: 35.5, 28: 36.5, 32: 36.7)  ->
  //    runs of >= 10 planes, as long as that leaves a quarter of the resident slots busy (64^3, 64
  //    columns: 6 runs of 10 planes took 20.1 us, 64 runs of one plane 13.3)
  //  * (round 3, uniform-band march: 256^3 6 runs 129.8-134.0 us, 8 runs 133.6-137.1: at most 6)
  //  * round 6, the value pack marches (15, 22-24) on wide planes: TWO runs per column, i.e. long
  //    chains of half the planes each (profiles/r06q_*, r06r_runs_*: 256^3 2-line 193.2 us at 2 runs
  //    vs 208.3 at its former 16 (1: 268.2); 1-line 204.4 at 2 vs 225.2 at 8 (1: 255.8, 4: 261.6);
  //    256^2 slabs of 32 / 64 / 96 / 128 planes 27.6 / 45.6 / 77.9 / 102.2 us for the 2-line march
  //    at 2 runs, the best or equal of every count tried).  On 128^3 (256 columns) 2 runs are slow
  //    (52.3 us vs 28.3): the rule is for wide planes only.  The same holds for the P1 Kuhn march
  //    (profiles/r06t_runs_p1k.jsonl: fused step 312.5 us at 2 runs vs 333.9 at 8, 4: 380.9; eig_mv
  //    263.2 vs 280.0); not for the 7-point value eig_mv (151.9 vs 154.7 on one box, 152.8 vs 152.2 on
  //    another: r06r_runs_256.jsonl, r06u_runs_uniform_mv.jsonl) nor the uniform-band march (fused
  //    132.7 vs 132.1, eig_mv 61.3 vs 48.9).
  const bool wide_pack = ncol >= 1024 && chunk == 64 && T.wide_two && (kuhn || fused);
  if (wide_pack)
    nseg = std::min<i64>(2, nplanes);
  else if (fused && ncol >= 1024)
    nseg = std::min<i64>(nplanes / 2 > 0 ? nplanes / 2 : 1,
                         std::max<i64>(2, std::min<i64>(T.wide_runs, nplanes / 32)));
  else if (fused)  // (geo2 marches: runs of >= 16 planes -- 128^3 8 runs 24.3 us, 12: 25.3, 16: 26.4)
    nseg = std::min(nseg, std::max<i64>({1, nplanes / (T.geo2_path() ? 16 : 10), (resident / 4 + ncol - 1) / ncol}));
  // the 2-line variants march line PAIRS: half the items per plane run, so twice the runs for as many waves
  const i64 items_per_run = two_lines ? ncol / 2 : ncol;
  if (two_lines && !wide_pack) nseg = std::min<i64>(nplanes, 2 * nseg);
  if (A.tune_march_runs > 0) nseg = std::min<i64>(A.tune_march_runs, nplanes);  // eig_mat_tune
  while (nseg > 1 && (items_per_run * nseg + kWaves - 1) / kWaves > kMaxRedBlocks) --nseg;
  if ((items_per_run * nseg + kWaves - 1) / kWaves > kMaxRedBlocks) return mp;
  mp.D = D;
  const auto [klo, khi] = far_spans(A);
  mp.dn = klo > 1 ? A.sym_off[1] : 0;
  mp.Un = A.sym_val + (i64)(klo > 1 ? A.sym_dj[1] : 0) * A.sym_ld;
  mp.dq = khi < A.sym_nd - 1 ? A.sym_off[khi] : 0;
  mp.Uq = A.sym_val + (i64)(khi < A.sym_nd - 1 ? A.sym_dj[khi] : 0) * A.sym_ld;
  for (int q = 0; q < 27; ++q) mp.kj[q] = -1;
  if (kuhn)  // band array of each upper box offset a D + b nx + c
    for (int q = 13; q < 27; ++q) mp.kj[q] = (signed char)box_band_array(A, D, q);
  if (A.sym_geo || kuhn)
  {
    mp.gx = A.sym_gx;
    mp.gy = A.sym_gy;
    mp.gz = A.sym_gz;
    mp.gz0 = A.sym_gz0;
  }
  if (A.sym_uniform)
  {
    const int kD = A.sym_nd - 1;
    int kz = -1, k1 = -1;
    for (int k = 0; k < A.sym_nd; ++k)
    {
      if (A.sym_off[k] == 0) kz = k;
      if (A.sym_off[k] == 1) k1 = k;
    }
    mp.cD = A.sym_uc[A.sym_dj[kD]];
    mp.c0 = kz >= 0 ? A.sym_uc[A.sym_dj[kz]] : 0.0;
    mp.c1 = k1 >= 0 ? A.sym_uc[A.sym_dj[k1]] : 0.0;
    mp.cn = klo > 1 ? A.sym_uc[A.sym_dj[1]] : 0.0;
    mp.cq = khi < A.sym_nd - 1 ? A.sym_uc[A.sym_dj[khi]] : 0.0;
  }
  mp.uni = uni;
  mp.pack = nullptr;
  // measured (tools/march_copy.hip *_pp, profiles/r03bo_march_copy.jsonl): the step's ping-pong at
  // 128^3 (2 x 32 MB of pairs) 12.9 us with plain stores vs 17.6 us nontemporal; at 256^3 (2 x 268
  // MB) no difference either way -- plain stores where every vector a launch touches fits in half
  // of the 256 MB MALL
  // fused step only (eig_mv's y, written repeatedly beside the same x, measured slower: 128^3 9.6 vs
  // 8.0 us)
  mp.tstore = fused && T.geo2_path() && (vectors_fit_mall(A) || (A.tune_cache & 1));
  mp.cache = A.tune_cache;
  // EIG_TUNE_CACHE 16: every launch of the 2-line variants with a downward body marches down (eig_mv and the
  // classic K1 too, when tuned onto them).  The fused step's alternation (neither bit, or both): launch_lanczos_fused_march
  mp.down = T.down_body && (A.tune_cache & 24) == 16;
  // the pipelined body (march_rows_geo2_2l<DOWN, PIPE>) takes kMarchPipeLds of LDS per workgroup -- one
  // workgroup per CU -- so it is on only where the launch has no more than that anyway: the two-run plan on
  // wide planes.  EIG_TUNE_CACHE 32: never; 64: wherever the body can run (tests reach small grids with it).
  // (The pack goes through one buffer descriptor there: 32-bit byte offsets over both of its pair arrays.)
  // Short runs pay the pipeline's fill (a first plane that overlaps nothing) for fewer planes: 256^2 slabs,
  // 7 interleaved rounds, kernel medians pipelined / plain (profiles/r08_pipe_sweep.jsonl): 32 planes 28.2 /
  // 26.8 us, 64 planes 46.3 / 44.9, 128 planes 91.1 / 96.2, 256^3 180.3 / 185.1 -- so where the variant is
  // the automatic choice the body is on from EIG_MARCH_PIPE_MIN_ROWS owned rows (like EIG_MARCH_2L_MIN_ROWS, the
  // threshold gates the automatic choice only: a variant asked for by EIG_TUNE_MARCH_PREFETCH takes the
  // plan's rule as it is).
  {
    const i64 wgs = (items_per_run * nseg + kWaves - 1) / kWaves;
    const bool can = fused && T.pipe_body && A.sym_ld * 32 < (i64(1) << 32);
    const bool pays = A.tune_march_prefetch != 0 || A.nb_rows >= EIG_MARCH_PIPE_MIN_ROWS;
    mp.pipe = can && !(A.tune_cache & 32) && ((A.tune_cache & 64) || (wide_pack && wgs <= A.ctx->num_cu && pays));
  }
  // line groups (MarchTraits::line_groups, on grids of whole 64-x runs and 4-line groups)
  mp.lines = A.tune_march_lines == 4 && T.line_groups && mp.gx % 64 == 0 &&
                     mp.gx > 0 && mp.gy % 4 == 0 && (i64)mp.gx * mp.gy == D
                 ? 4
                 : 0;
  mp.zb = zb;
  mp.nplanes = nplanes;
  mp.mrows = A.nslices * 64;
  mp.ncol = (int)items_per_run;
  mp.nseg = (int)nseg;
  return mp;
}

// eig_mat_info.march_variant: the variant a whole-matrix launch takes, -1 when it does not march
int march_variant(const eig_mat_s &A, bool fused)
{
  if (A.br != 1 || A.bc != 1) return -1;
  const MarchPlan mp = march_plan(A, image_mode(A), 0, -1, fused);
  return mp.nseg > 0 ? mp.uni : -1;
}

// eig_mat_info.march_pipe: a whole-matrix fused launch takes the pipelined body (MarchPlan::pipe)
int march_pipe(const eig_mat_s &A)
{
  if (A.br != 1 || A.bc != 1) return 0;
  const MarchPlan mp = march_plan(A, image_mode(A), 0, -1, true);
  return mp.nseg > 0 ? mp.pipe : 0;
}

bool march_split_active(const eig_mat_s &A)
{
  return A.mz1 > A.mz0 && march_plan(A, image_mode(A), A.mz0, A.mz1).nseg > 0;
}

bool marches(const eig_mat_s &A, int mode)
{
  // (distributed launches with a halo take the interior / boundary split, never the march)
  const bool whole = !A.ctx->distributed() || (A.recvs.empty() && A.sends.empty());
  return whole ? march_plan(A, mode).nseg > 0 : march_split_active(A);
}

// General band geometry for k_spmm8_marchg: carried offset P (widest multiple of 16 with -P stored),
// +-1 stored, every span at most kGSpan offsets.  False when the band does not qualify.
bool gspans(const eig_mat_s &A, i64 &P, GSpans &sp)
{
  if (!A.sym_val || A.sym_nd < 3) return false;
  const int nd = A.sym_nd;
  auto kof = [&](i64 d) {
    for (int k = 0; k < nd; ++k)
      if (A.sym_off[k] == d) return k;
    return -1;
  };
  if (kof(1) < 0 || kof(-1) < 0) return false;
  const auto [klo, khi] = far_spans(A);
  // candidates for P from the widest down; the first whose four spans fit
  for (int kp = nd - 1; kp >= khi; --kp)
  {
    const i64 d = A.sym_off[kp];
    if (d % 16 != 0 || kof(-d) < 0) continue;
    sp.kPm = kof(-d);
    sp.kPp = kp;
    sp.s1b = 0, sp.s1e = sp.kPm;
    sp.s2b = sp.kPm + 1, sp.s2e = klo;
    sp.s3b = khi, sp.s3e = sp.kPp;
    sp.s4b = sp.kPp + 1, sp.s4e = nd;
    if (sp.s1e - sp.s1b <= kGSpan && sp.s2e - sp.s2b <= kGSpan && sp.s3e - sp.s3b <= kGSpan &&
        sp.s4e - sp.s4b <= kGSpan)
    {
      P = d;
      return true;
    }
  }
  return false;
}

bool marchg_plan(const eig_mat_s &A, MarchPlan &mp, GSpans &sp)
{
  if (A.br != 1 || A.bc != 1 || !march_enabled(A)) return false;
  const int mode = image_mode(A);
  if (mode != kSymN8 && mode != kSymN32) return false;
  i64 P;
  if (!gspans(A, P, sp)) return false;
  const i64 nplanes = (A.nb_rows + P - 1) / P;
  if (nplanes < 4) return false;
  const i64 ncol = P / 16;
  const i64 resident = 6LL * 4 * A.ctx->num_cu;  // waves at the kernel's 6 waves / SIMD
  i64 nseg = std::min<i64>(std::max<i64>(1, (resident + ncol - 1) / ncol), nplanes);
  mp = MarchPlan{};
  mp.D = P;
  mp.zb = 0;
  mp.nplanes = nplanes;
  mp.mrows = A.nslices * 64;
  mp.ncol = (int)ncol;
  mp.nseg = (int)nseg;
  return true;
}

void lanczos_kernel_info(const eig_mat_s &A, bool fused, std::string &name, i64 &bytes)
{
  const i64 n = A.nb_rows * A.br, vec = fused ? 32 * n : 24 * n;  // fused: (t, u) pairs in + out; K1: x, u_{j-1}, t
  if (A.br == A.bc && A.br >= 2 && A.br <= 4)
  {
    // blocked SELL-64 image: every padded block value and column index, the slice pointers, the vectors
    bytes = (8 * (i64)A.br * A.bc + 4) * A.nnzb_padded + 8 * (A.nslices + 1) + vec;
    name = fused ? "k_lanczos_fused_blk" : "k_lanczos_spmv_blk";
    return;
  }
  const int mode = A.br == 1 && A.bc == 1 ? image_mode(A) : kExplicit;
  if (is_sym_mode(mode))
  {
    bytes = 8 * (i64)A.sym_nup * n + (i64)A.sym_mask_bytes * n + vec;
    const bool march = marches(A, mode);
    // the march streams the band arrays its variant reads (uniform values: none; the 7-point pack: 4),
    // the row mask unless it comes from the coordinates, and the vectors
    if (march)
    {
      const MarchTraits T = march_traits(march_launch_variant(A, mode, march_select(A, fused)));
      bytes = 8 * (i64)T.stream_arrays(A.sym_nup) * n + (T.geo_masks ? 0 : (i64)A.sym_mask_bytes * n) + vec;
    }
    name = fused ? (march ? "k_lanczos_fused_march" : "k_lanczos_fused_b1")
                 : (march ? "k_lanczos_spmv_march" : "k_lanczos_spmv_b1");
  }
  else
  {
    bytes = sell_image_bytes(A) + vec;
    name = fused ? "k_lanczos_fused_b1" : "k_lanczos_spmv_b1";
  }
}

// Bytes the SELL-64 slice kernels stream per pass over the image (one row per lane): every padded
// value, the 4-B column index of each explicit-slice entry, per stencil slice its width and 8
// offsets (36 B) and a 1-B mask per row, and the slice pointers -- not SURVEY 8(d)'s CSR count (the
// stencil slices read no column indices).
i64 sell_image_bytes(const eig_mat_s &A)
{
  const i64 bb = (i64)A.br * A.bc, C = 64 * (i64)A.R;
  return 8 * bb * A.nnzb_padded + 4 * A.sell_explicit + 8 * (A.nslices + 1) +
         (A.n_stencil_slices ? 4 * A.nslices + A.n_stencil_slices * (32 + C) : 0);
}

// EIG_LANCZOS_AUTO: the fused step on every 1x1 image.  (Round 3 took the two-kernel step on
// scattered images while k_lanczos_fused_b1 spilled 36-46 VGPRs there -- 634 vs 427 us on the
// scrambled + RCM 256^3 Poisson, the spill write-back being the 3.5x write excess PMC showed; at 6
// waves / SIMD without the spills it runs 408 us, step 415 vs 436 us, PMC 0.97x of the CSR bytes:
// profiles/r03ah_csr*.)
// Blocked images (square blocks 2..4) keep the two-kernel step: at C3 (Q1 elasticity 64^3, 3x3
// blocks, 521 MB of matrix against 25 MB of vectors) the two-kernel step took 99.46 / 99.33 us and
// the fused step 103.69 / 103.49 us, alternated in one process (profiles/blocked_lanczos_c3.jsonl) --
// kernel trace: k_lanczos_fused_blk 105.9 us against k_lanczos_spmv_blk 91.7 + k_lanczos_update
// 8.5 us; the 16-B gathers cost more than the update kernel they save.
bool fused_step_pays(const eig_mat_s &A) { return A.br == 1 && A.bc == 1; }

std::string kernel_for(const eig_mat_s &A, int op)
{
  const bool b1 = A.br == 1 && A.bc == 1;
  const int mode = b1 ? image_mode(A) : kExplicit;
  std::string name;
  i64 bytes;
  switch (op)
  {
    case 0:
      if (!b1) return "k_spmv_blk";
      return marches(A, mode) ? "k_spmv_march" : "k_spmv_b1";
    case 1:
    case 2:
      lanczos_kernel_info(A, op == 2, name, bytes);
      return name;
    case 3:
    case 4:
      // 3-D box stencils whose rows are class-constant: the row-class kernels for any m % 8 == 0
      if (b1 && box_prepare(A) && A.box_ctab) return op == 3 ? "k_boxc_mv8" : "k_boxc_mv8_cheb";
    {
      if (!b1) return (op == 3 && A.br == A.bc) ? "k_spmm_blk_mv8" : "none";  // square blocks 2..4 (k_mv8.hip)
      if (op == 3 && march_plan(A, mode, 0, -1, false, 16).nseg > 0) return "k_spmm8_march";
      MarchPlan mp;
      GSpans sp;
      if (marchg_plan(A, mp, sp)) return op == 3 ? "k_spmm8_marchg" : "k_spmm8_marchg_cheb";
      return op == 3 ? (b1 && A.nb_rows > 0 ? "k_sell_mv8g" : "none") : "k_sell_mv8q_cheb";
    }
    case 5:
    case 6:
      if (b1 && box_prepare(A))
      {
        if (A.box_ctab) return op == 5 ? "k_boxc_mv8" : "k_boxc_mv8_cheb";  // row-class image
        if (box_cols(A) == 16) return op == 5 ? "k_box_mv16p" : "k_box_mv16p_cheb";
        return op == 5 ? "k_box_mv32" : "k_box_mv32_cheb";
      }
      return kernel_for(A, op - 2);
    case EIG_OP_FILT8:
    case EIG_OP_FILT32:
      // the filter step (launch_filt_step): blocked, row-class / box image, else SELL -- never the band march
      if (!b1) return (A.br == A.bc && A.br >= 2 && A.br <= 4) ? "k_spmm_blk_mv8_filt" : "none";
      if (box_prepare(A))
      {
        if (A.box_ctab) return "k_boxc_mv8_filt";
        if (op == EIG_OP_FILT32) return box_cols(A) == 16 ? "k_box_mv16p_filt" : "k_box_mv32_filt";
      }
      if (A.nb_rows <= 0) return "none";
      return op == EIG_OP_FILT8 ? "k_sell_mv8g_filt" : "k_sell_mv8q_filt";
    default:
      return "none";
  }
}

}  // namespace eigmi
