// march_plan.h -- what the plane-march kernels (k_march.hip) and their host-side planning (march_plan.cpp)
// share: the image modes, the plan structures passed as kernel arguments, and the selection / planning /
// query functions.  Host-only declarations and plain data: no device code, so host tests compile
// march_plan.cpp with this header and no GPU.
#pragma once
#include "internal.h"
#include "march_variants.h"

#include <string>
#include <utility>

namespace eigmi {

constexpr int kWaves = kStreamThreads / 64;

// Image modes: every slice explicit, every slice stencil, or mixed (per-slice wave-uniform branch);
// kSym8 / kSym32: the symmetric band image with u8 / u32 row masks (R = 1 only); kSymN8 / kSymN32:
// the same with the lane-shift path for the offsets -1 / 0 / +1.
enum { kExplicit = 0, kStencil = 1, kMixed = 2, kSym8 = 3, kSym32 = 4, kSymN8 = 5, kSymN32 = 6 };

// Plan of one plane-march launch (march_plan; a kernel argument of the march kernels of k_march.hip, whose
// "Plane-marching fused step" comment describes the march itself).
struct MarchPlan {
  i64 D;        // rows per plane (the band's widest offset)
  i64 zb;       // first plane marched
  i64 nplanes;  // planes marched: zb .. zb + nplanes - 1 (whole launch: ceil(rows / D) from 0)
  i64 mrows;    // rows covered by the row mask (nslices * 64)
  int ncol;     // D / 64
  int nseg;     // plane runs per column
  // first entries of the far spans (-D, -1) and (+1, +D): offset (0 = empty span) and band array
  i32 dn, dq;
  const double *Un, *Uq;
  // uniform band (eig_mat_s::sym_uniform): the band values of the +D, 0, +1, far-span (dn / dq)
  // arrays, taken instead of the array loads by the UNI kernels
  double cD, c0, c1, cn, cq;
  // geometric row masks (eig_mat_s::sym_geo, uniform bands only): the nx x ny x nz grid whose
  // in-grid neighbours are exactly the stored entries -- the march derives each row's mask from
  // its coordinates instead of loading it; gz0 = the global plane of the rank's first row
  int gx, gy, gz, gz0;
  int uni;  // the march variant the launch takes (march_select; march_variants.h says what each is)
  // results stored with plain (MALL-allocating) stores instead of nontemporal ones: the vectors of a
  // small grid stay in the 256 MB memory-side cache for the next launch (geo2 kernels)
  int tstore;
  // box marches (the Kuhn variants): band array of the upper offset at 27-box position (a+1) 9 + (b+1) 3 + (c+1),
  // -1 when the stencil does not store it
  signed char kj[27];
  const double *pack;
  // eig_mat_tune(EIG_TUNE_CACHE) bits for the value march (measurement): 2 = the value streams with the
  // default cache policy instead of nontemporal, 4 = the +D pair stream nontemporal
  // 8 = every launch marches upward, 16 = every launch of variants 22 / 23 marches downward (MarchPlan::down)
  int cache;
  // geo2 value marches: 4 = a workgroup's 4 waves march the same 64 x of 4 consecutive y lines (their
  // +-nx gathers then mostly read lines their sibling waves just loaded on the same CU) instead of the
  // 4 x runs of one line; 0 = the item order (eig_mat_tune EIG_TUNE_MARCH_LINES)
  int lines;
  // the 2-line value marches 22 / 23: 1 = every plane run is marched from its last plane down to its first
  // (march_rows_geo2_2l<DOWN>); wave-uniform, a kernel argument -- a launch captured into a graph replays
  // its own direction
  int down;
  // the fused launches of variants 22 / 23: 1 = the body that loads every plane through LDS, one plane ahead
  // (march_rows_geo2_2l<DOWN, PIPE>; the launch then carries kMarchPipeLds bytes of dynamic LDS); wave-uniform,
  // a kernel argument like `down`
  int pipe;
};

// The pipelined body's LDS (k_march.hip "PIPE"): two buffers per wave of kMarchPipeRegions lane-linear regions
// of 64 x 16 B, one region per load of a plane.
constexpr int kMarchPipeRegions = 13;
constexpr unsigned kMarchPipeBuf = kMarchPipeRegions * 1024u;  // one plane of one wave
constexpr unsigned kMarchPipeLds = kWaves * 2 * kMarchPipeBuf;  // dynamic LDS of a pipelined launch
constexpr int kMaxPipeDevices = 64;  // device indices whose kernels launch_lanczos_fused_march has raised to it

// General band march (k_spmm8_marchg): the gathered offsets of a span, and the spans of an image (gspans).
constexpr int kGSpan = 3;
struct GSpans {
  int kPm, kPp;                      // mask bits of -P / +P
  int s1b, s1e, s2b, s2e, s3b, s3e, s4b, s4e;
};

// The 2-line fused march (variant 22; k_march.hip march_rows_geo2_2l)
// is the default on ranks of at least EIG_MARCH_2L_MIN_ROWS rows: 256^3 (16.8 M
// rows) 206.5-206.8 us vs 223.5 us for variant 15 (profiles/r06e_sweep256_2lines.jsonl, 0.65 of HBM),
// but 2 M-row grids (128^3, one rank's 256^2 x 32 slab) 28.2-28.4 vs 27.7-27.9 us: fewer, longer
// wave chains cost more there than the halved gathers save.  256^2 slabs (profiles/r06m_threshold.jsonl):
// 4 M rows 47.1 vs 46.1 us, 6 M rows 84.3 vs 89.8 us, 8 M rows 111.7 vs 116.7 us; with two plane runs
// per column on wide planes (march_plan, round 6) 4 M rows 45.6 vs 46.0 us, 2 M rows 27.6 either way --
// the threshold is 4 M.
constexpr bool kMarch2lDefault = true;
// Serpentine (the downward body: k_march.hip "DOWN", MarchTraits::down_body):
// A fused launch of variant 22 / 23 marches down when its launch index is odd (launch_lanczos_fused_march).
// Measured at 256^3, one process, 7 interleaved rounds (profiles/r07_serpentine_ab.jsonl): every
// launch upward 191.8 us (max - min over rounds 1.0), every launch downward 198.4 us (the downward body is
// the slower one), alternating 185.0 us -- each launch gains what the memory-side cache still holds of the
// one before it.  Plain pair stores or default-policy (+D, 0) loads (EIG_TUNE_CACHE 1 / 2) change nothing
// there (184.8 - 185.0 us), so the nontemporal defaults stay.
constexpr bool kMarch2lSerpentine = true;

// ---- march_plan.cpp: pure functions of a matrix's host-side fields (and, where named, of A.ctx->num_cu and
// A.ctx->distributed()).  None allocates, launches or touches the device.  (march_geometry, march_select,
// kuhn_variant, march_variant, march_pipe, march_split_active and the kernel queries: internal.h.) ----------
int sym_kernels(const eig_mat_s &A);
bool is_sym_mode(int mode);
int image_mode(const eig_mat_s &A);
bool march_enabled(const eig_mat_s &A);
std::pair<int, int> far_spans(const eig_mat_s &A);
bool march_span1(const eig_mat_s &A);
bool vectors_fit_mall(const eig_mat_s &A);
int march_select(const eig_mat_s &A, bool fused);  // on A's own context
int march_launch_variant(const eig_mat_s &A, int mode, int variant);
unsigned march_grid(const MarchPlan &mp);  // workgroups of the plan's launch
int box_band_array(const eig_mat_s &A, i64 D, int q);
// The plan of a launch on planes [zb, ze) (ze < 0: the whole matrix), nseg = 0 where nothing marches.
// MarchPlan::pack stays null: a launch sets it (k_march.hip launch_plan), a query has no use for it.
MarchPlan march_plan(const eig_mat_s &A, int mode, i64 zb = 0, i64 ze = -1, bool fused = false, int chunk = 64);
// Whether a whole-matrix launch on A marches (one rank, or no halo: the whole plan; else the interior-plane
// split).  Tests the eig_mv / K1 plan, also where the caller goes on to name the fused kernel.
bool marches(const eig_mat_s &A, int mode);
bool gspans(const eig_mat_s &A, i64 &P, GSpans &sp);
// Plan and spans of the general-band march (k_spmm8_marchg) on A; false where it does not apply.
bool marchg_plan(const eig_mat_s &A, MarchPlan &mp, GSpans &sp);

}  // namespace eigmi
