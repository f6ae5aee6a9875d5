// trsv_image.h -- the host images of exported LU factors that k_trsv.hip uploads and its kernels read: the row form
// of the factors with its block splits, the admission rules of the staged and the block-inverse kernels, the
// 64 x 64 block-inverse tiles with their conditioning gate, the slab / tile layout of the staged kernel, and the
// exported (UMFPACK) form of an envelope factorisation.  Plain host arithmetic: no device code, no HIP runtime
// call, no context and no TrsvImage, so host tests compile trsv_image.cpp alone and need no GPU.
#pragma once
#include "internal.h"

#include <vector>

namespace eigmi {

constexpr int kTB = 64;     // rows per block
constexpr int kRing4 = 4;   // ring slots of the staged kernel (power of two)
constexpr int kSlab = 128;  // slab entries per row staged at once (LDS: 96 KiB of slab + 32 KiB tile)
// block-inverse image: at most kBinvMaxGD coupled blocks per factor (envelope bandwidth <= 512 rows)
// and kBinvTiles 64 x 64 double tiles for both factors (1 GiB); a diagonal block whose estimated
// condition max|D_b| max|inv(D_b)| 64 exceeds kBinvCond keeps the factors on the substitution
// kernels (products with an inverse of an ill-conditioned block lose what substitution keeps)
constexpr int kBinvMaxGD = 8;
constexpr i64 kBinvTiles = 32768;
constexpr double kBinvCond = 1e6;

// The factors in the row form the device solves read: L rows without the unit diagonal (ascending
// columns), U rows without the diagonal (descending columns) and the U diagonal.
struct FactorRows {
  std::vector<i64> lrp;
  std::vector<i32> lc;
  std::vector<double> lv;
  std::vector<i64> urp;
  std::vector<i32> uc;
  std::vector<double> uv, ud;
};
// From the exported form (lu.cpp): L in compressed rows with the unit diagonal last, U in compressed
// columns with the pivot last.  EIG_ERR_ARG for an L entry on or above the diagonal, a U entry on or
// below it, or an empty U column.
FactorRows factor_rows(i64 n, const std::vector<i64> &Lp, const std::vector<i64> &Lj, const std::vector<double> &Lx,
                       const std::vector<i64> &Up, const std::vector<i64> &Ui, const std::vector<double> &Ux);

// split points: L row i -> first entry inside i's 64-row block; U row i (descending columns) ->
// first entry with a column inside the block
struct RowSplits {
  std::vector<i64> ls, us;
};
RowSplits row_splits(i64 n, const FactorRows &rows);

// What TrsvImage keeps on the host until the staged image is built (k_trsv.hip).
struct TrsvHost {
  FactorRows rows;
  RowSplits splits;
};

// Which kernels the factors are admitted to.  staged: every row of both factors has at most kSlab
// entries outside its block, all within kRing4 blocks.  gd: the farthest coupled block of L / of U.
// binv_admitted: no zero U pivot (it leaves the reference's division to produce inf / nan), at most
// kBinvTiles tiles (one per diagonal block and per coupled block) and both gd <= kBinvMaxGD; the
// conditioning gate of build_binv_tiles comes after it.
struct TrsvPlan {
  bool staged = false;
  int gd[2] = {0, 0};
  bool binv_admitted = false;
};
TrsvPlan trsv_plan(i64 n, const FactorRows &rows, const RowSplits &splits);

// Block-inverse image of one factor (diag == nullptr: the unit lower factor): dinv + b * 4096 holds
// inv(D_b) as [t][r] (rows past n: identity), g + (b * gd + d - 1) * 4096 holds G(b, d) =
// inv(D_b) T(b, d) as [t][r], zero where block b -+ d is outside the matrix or carries no entry.
// ok == false (dinv, g unspecified): a diagonal block fails max|D_b| max|inv(D_b)| 64 <= kBinvCond.
struct BinvTiles {
  bool ok = false;
  std::vector<double> dinv, g;
};
BinvTiles build_binv_tiles(i64 n, const std::vector<i64> &rp, const std::vector<i32> &cj, const std::vector<double> &cv,
                           const std::vector<i64> &split, const double *diag, int gd);

// Block-staged image of one factor (k_tsolve_staged), per 64-row block b: w[b] = the widest row's count
// of outside-the-block entries; entry k of row bs + r at (b * kSlab + k) * 64 + r of v1 / c1 in the row's
// own order (column -1 = padding); the inside entries as a dense tile [t][r] at tile + b * 4096 with bit
// t of tmask[b * 64 + r].  EIG_ERR_ARG for a row wider than kSlab (trsv_plan's staged excludes it).
struct StagedImage {
  std::vector<i32> w;
  std::vector<double> v1;
  std::vector<i32> c1;
  std::vector<double> tile;
  std::vector<unsigned long long> tmask;
};
StagedImage build_staged_image(i64 n, const std::vector<i64> &rp, const std::vector<i32> &cj,
                               const std::vector<double> &cv, const std::vector<i64> &split);

// Threads of build_binv_tiles over the blocks: 0 = up to 16 hardware threads (the default), n > 0 = exactly n
// (host tests compare a threaded build with a one-thread build).  Fewer than 32 blocks stay serial.
extern int trsv_image_threads;

// The exported form of an envelope factorisation: L rows over the envelope [f_k, k) with the unit diagonal
// last, U columns over [f_k, k) with the pivot last; exact zeros dropped.  Lat(k, j), Uat(i, k) and Dat(k)
// read the factors.
struct ExportedFactors {
  std::vector<i64> Lp, Lj, Up, Ui;
  std::vector<double> Lx, Ux;
};
template <class FL, class FU, class FD>
ExportedFactors export_envelope(i64 n, const std::vector<i64> &f, FL &&Lat, FU &&Uat, FD &&Dat)
{
  ExportedFactors E;
  E.Lp.assign(n + 1, 0);
  E.Up.assign(n + 1, 0);
  for (i64 k = 0; k < n; ++k)
  {
    i64 cl = 1, cu = 1;  // + the unit / pivot diagonal
    for (i64 j = f[k]; j < k; ++j) cl += Lat(k, j) != 0.0;
    for (i64 i = f[k]; i < k; ++i) cu += Uat(i, k) != 0.0;
    E.Lp[k + 1] = E.Lp[k] + cl;
    E.Up[k + 1] = E.Up[k] + cu;
  }
  E.Lj.resize(E.Lp[n]);
  E.Lx.resize(E.Lp[n]);
  E.Ui.resize(E.Up[n]);
  E.Ux.resize(E.Up[n]);
  for (i64 k = 0; k < n; ++k)
  {
    i64 q = E.Lp[k];
    for (i64 j = f[k]; j < k; ++j)
      if (Lat(k, j) != 0.0)
      {
        E.Lj[q] = j;
        E.Lx[q++] = Lat(k, j);
      }
    E.Lj[q] = k;
    E.Lx[q] = 1.0;
    q = E.Up[k];
    for (i64 i = f[k]; i < k; ++i)
      if (Uat(i, k) != 0.0)
      {
        E.Ui[q] = i;
        E.Ux[q++] = Uat(i, k);
      }
    E.Ui[q] = k;
    E.Ux[q] = Dat(k);
  }
  return E;
}

}  // namespace eigmi
