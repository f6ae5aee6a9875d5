// trsv_image.cpp -- host images of exported LU factors (trsv_image.h): row form, block splits, kernel admission,
// block-inverse tiles and the staged slab / tile layout.  k_trsv.hip uploads what these return.
#include <algorithm>
#include <atomic>
#include <cmath>
#include <thread>
#include <utility>

#include "trsv_image.h"

namespace eigmi {

int trsv_image_threads = 0;

FactorRows factor_rows(i64 n, const std::vector<i64> &Lp, const std::vector<i64> &Lj, const std::vector<double> &Lx,
                       const std::vector<i64> &Up, const std::vector<i64> &Ui, const std::vector<double> &Ux)
{
  FactorRows R;
  // L rows: the reference subtracts entries Lp[i] .. Lp[i+1]-2 in stored order (the last entry is
  // the unit diagonal, kernels_cpp.hh:716-722).  Stored order is kept when ascending; otherwise the
  // row is sorted by column (then equal to the reference to rounding, not bitwise).
  R.lrp.assign(n + 1, 0);
  R.urp.assign(n + 1, 0);
  R.ud.assign(n, 0.0);
  // L: rows copied as stored when ascending (the usual case), else through a sorted copy
  R.lc.reserve(Lx.size());
  R.lv.reserve(Lx.size());
  std::vector<std::pair<i64, double>> e;
  for (i64 i = 0; i < n; ++i)
  {
    const i64 b = Lp[i], t = Lp[i + 1] - 1;  // (the last entry is the unit diagonal)
    bool sorted = true;
    for (i64 k = b; k < t; ++k)
    {
      EIG_CHECK(Lj[k] >= 0 && Lj[k] < i, EIG_ERR_ARG, "L factor: entry not strictly below the diagonal");
      if (k > b && Lj[k] < Lj[k - 1]) sorted = false;
    }
    if (sorted)
      for (i64 k = b; k < t; ++k)
      {
        R.lc.push_back((i32)Lj[k]);
        R.lv.push_back(Lx[k]);
      }
    else
    {
      e.clear();
      for (i64 k = b; k < t; ++k) e.push_back({Lj[k], Lx[k]});
      std::stable_sort(e.begin(), e.end(), [](const auto &a, const auto &c) { return a.first < c.first; });
      for (auto &q : e)
      {
        R.lc.push_back((i32)q.first);
        R.lv.push_back(q.second);
      }
    }
    R.lrp[i + 1] = (i64)R.lc.size();
  }
  // U: column j holds rows Ui[Up[j] .. Up[j+1]-2] above the diagonal Ux[Up[j+1]-1]; the reference's
  // push loop (kernels_cpp.hh:730-745) updates row i with columns j in DECREASING order, which is
  // the order the pull form below uses -- bitwise whatever the order inside a column.  Transposed
  // by a counting sort over the columns in descending order (rows come out descending).
  for (i64 j = 0; j < n; ++j)
  {
    EIG_CHECK(Up[j + 1] > Up[j], EIG_ERR_ARG, "U factor: empty column");
    R.ud[j] = Ux[Up[j + 1] - 1];
    for (i64 k = Up[j]; k < Up[j + 1] - 1; ++k)
    {
      EIG_CHECK(Ui[k] >= 0 && Ui[k] < j, EIG_ERR_ARG, "U factor: entry not strictly above the diagonal");
      ++R.urp[Ui[k] + 1];
    }
  }
  for (i64 i = 0; i < n; ++i) R.urp[i + 1] += R.urp[i];
  R.uc.resize((size_t)R.urp[n]);
  R.uv.resize((size_t)R.urp[n]);
  {
    std::vector<i64> next(R.urp.begin(), R.urp.end() - 1);
    for (i64 j = n - 1; j >= 0; --j)
      for (i64 k = Up[j]; k < Up[j + 1] - 1; ++k)
      {
        const i64 at = next[Ui[k]]++;
        R.uc[at] = (i32)j;
        R.uv[at] = Ux[k];
      }
  }
  return R;
}

RowSplits row_splits(i64 n, const FactorRows &R)
{
  RowSplits S;
  S.ls.resize(n);
  S.us.resize(n);
  for (i64 i = 0; i < n; ++i)
  {
    const i64 bs = i / kTB * kTB, be = std::min(bs + kTB, n);
    i64 k = R.lrp[i];
    while (k < R.lrp[i + 1] && R.lc[k] < bs) ++k;
    S.ls[i] = k;
    k = R.urp[i];
    while (k < R.urp[i + 1] && R.uc[k] >= be) ++k;
    S.us[i] = k;
  }
  return S;
}

namespace {

// admission to the staged kernel: <= kSlab outside entries per row, all within kRing4 blocks
bool fits(i64 n, const std::vector<i64> &rp, const std::vector<i32> &cj, const std::vector<i64> &split, bool lower)
{
  for (i64 i = 0; i < n; ++i)
  {
    if (split[i] - rp[i] > kSlab) return false;
    const i64 blk = i / kTB;
    for (i64 q = rp[i]; q < split[i]; ++q)
    {
      const i64 cb = cj[q] / kTB;
      if (lower ? (cb < blk - kRing4) : (cb > blk + kRing4)) return false;
    }
  }
  return true;
}

// the farthest block an outside entry couples a row's block to
int coupled(i64 n, const std::vector<i64> &rp, const std::vector<i32> &cj, const std::vector<i64> &split, bool lower)
{
  int dm = 0;
  for (i64 i = 0; i < n; ++i)
    for (i64 q = rp[i]; q < split[i]; ++q)
      dm = std::max<int>(dm, (int)(lower ? i / kTB - cj[q] / kTB : cj[q] / kTB - i / kTB));
  return dm;
}

// f(b0, b1) over contiguous block ranges on up to 16 host threads
template <class F>
void parallel_blocks(i64 nb, F &&f)
{
  unsigned nt = std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
  if (trsv_image_threads > 0) nt = (unsigned)trsv_image_threads;
  if (nb < 32) nt = 1;
  if (nt == 1) return f(0, nb);
  std::vector<std::thread> th;
  for (unsigned t = 0; t < nt; ++t) th.emplace_back([&, t] { f(nb * t / nt, nb * (t + 1) / nt); });
  for (auto &t : th) t.join();
}

}  // namespace

TrsvPlan trsv_plan(i64 n, const FactorRows &R, const RowSplits &S)
{
  TrsvPlan plan;
  plan.staged = fits(n, R.lrp, R.lc, S.ls, true) && fits(n, R.urp, R.uc, S.us, false);
  plan.gd[0] = coupled(n, R.lrp, R.lc, S.ls, true);
  plan.gd[1] = coupled(n, R.urp, R.uc, S.us, false);
  const i64 nblocks = (n + kTB - 1) / kTB;
  const i64 tiles = nblocks * (2 + plan.gd[0] + plan.gd[1]);
  bool pivots = true;  // a zero U pivot leaves the reference's division to produce inf / nan
  for (i64 i = 0; i < n; ++i) pivots = pivots && R.ud[i] != 0.0;
  plan.binv_admitted = pivots && tiles <= kBinvTiles && plan.gd[0] <= kBinvMaxGD && plan.gd[1] <= kBinvMaxGD;
  return plan;
}

BinvTiles build_binv_tiles(i64 n, const std::vector<i64> &rp, const std::vector<i32> &cj, const std::vector<double> &cv,
                           const std::vector<i64> &split, const double *diag, int gd)
{
  const bool lower = diag == nullptr;
  const i64 nblocks = (n + kTB - 1) / kTB;
  const size_t T2 = (size_t)kTB * kTB;
  BinvTiles out;
  std::vector<double> &dinv = out.dinv, &gt = out.g;
  dinv.assign((size_t)nblocks * T2, 0.0);
  gt.assign((size_t)std::max<i64>(nblocks * gd, 1) * T2, 0.0);
  std::atomic<bool> ok{true};
  // blocks are independent: threads over contiguous block ranges
  parallel_blocks(nblocks, [&](i64 b0, i64 b1) {
    // Di holds inv(D_b) by columns (Di[j * 64 + i] = inv(D)[i][j]): each column is one triangular
    // solve with contiguous operands, and it is already the device layout of dinv ([t][r])
    std::vector<double> Db(T2), Di(T2), Tb(T2);
    for (i64 b = b0; b < b1 && ok.load(std::memory_order_relaxed); ++b)
    {
      const i64 bs = b * kTB, nbr = std::min<i64>(kTB, n - bs);
      // the diagonal block D[r][t] (rows past n: identity)
      std::fill(Db.begin(), Db.end(), 0.0);
      for (int r = 0; r < kTB; ++r) Db[r * kTB + r] = (r < nbr && !lower) ? diag[bs + r] : 1.0;
      for (i64 r = 0; r < nbr; ++r)
        for (i64 q = split[bs + r]; q < rp[bs + r + 1]; ++q) Db[r * kTB + (cj[q] - bs)] = cv[q];
      // its inverse, column j = the solution of D x = e_j (lower: top-down, upper: bottom-up)
      std::fill(Di.begin(), Di.end(), 0.0);
      for (int j = 0; j < kTB; ++j)
      {
        double *x = &Di[(size_t)j * kTB];
        if (lower)
          for (int i = j; i < kTB; ++i)
          {
            const double *Dr = &Db[(size_t)i * kTB];
            double v = i == j ? 1.0 : 0.0;
            for (int k = j; k < i; ++k) v -= Dr[k] * x[k];
            x[i] = v / Dr[i];
          }
        else
          for (int i = j; i >= 0; --i)
          {
            const double *Dr = &Db[(size_t)i * kTB];
            double v = i == j ? 1.0 : 0.0;
            for (int k = i + 1; k <= j; ++k) v -= Dr[k] * x[k];
            x[i] = v / Dr[i];
          }
      }
      {
        double dm = 0.0, im = 0.0;
        bool nan = false;  // std::max drops a NaN operand: without this a NaN entry would pass the estimate
        for (size_t q = 0; q < T2; ++q)
        {
          dm = std::max(dm, std::fabs(Db[q]));
          im = std::max(im, std::fabs(Di[q]));
          nan = nan || std::isnan(Db[q]) || std::isnan(Di[q]);
        }
        if (nan || !(dm * im * kTB <= kBinvCond)) ok = false;  // (an overflowed estimate, inf * 0, included)
      }
      std::copy(Di.begin(), Di.end(), dinv.begin() + (size_t)b * T2);
      // G(b, d) = inv(D_b) T(b, d), T(b, d)[r'][t] = the entry of row bs + r' in column t of block b -+ d
      for (int d = 1; d <= gd; ++d)
      {
        const i64 src = lower ? b - d : b + d;
        if (src < 0 || src >= nblocks) continue;
        std::fill(Tb.begin(), Tb.end(), 0.0);
        bool any = false;
        for (i64 r = 0; r < nbr; ++r)
          for (i64 q = rp[bs + r]; q < split[bs + r]; ++q)
            if (cj[q] / kTB == src)
            {
              Tb[r * kTB + (cj[q] - src * kTB)] += cv[q];
              any = true;
            }
        if (!any) continue;
        double *gb = &gt[((size_t)b * gd + (d - 1)) * T2];
        for (int rr = 0; rr < kTB; ++rr)  // G[:, t] += inv(D)[:, rr] T[rr][t] (column rr of inv(D):
        {                                 // rows rr.. (lower) / ..rr (upper) are its nonzeros)
          const double *dcol = &Di[(size_t)rr * kTB];
          const int r0 = lower ? rr : 0, r1 = lower ? kTB : rr + 1;
          for (int t = 0; t < kTB; ++t)
          {
            const double tv = Tb[rr * kTB + t];
            if (tv == 0.0) continue;
            double *gcol = gb + (size_t)t * kTB;
            for (int r = r0; r < r1; ++r) gcol[r] += dcol[r] * tv;
          }
        }
      }
    }
  });
  out.ok = ok;
  return out;
}

StagedImage build_staged_image(i64 n, const std::vector<i64> &rp, const std::vector<i32> &cj,
                               const std::vector<double> &cv, const std::vector<i64> &split)
{
  const i64 nblocks = (n + kTB - 1) / kTB;
  const i64 slab = std::max<i64>(nblocks * kSlab * kTB, 1);
  StagedImage S;
  S.w.assign(std::max<i64>(nblocks, 1), 0);
  S.v1.assign(slab, 0.0);
  S.c1.assign(slab, -1);
  S.tile.assign((size_t)std::max<i64>(nblocks, 1) * kTB * kTB, 0.0);
  S.tmask.assign((size_t)std::max<i64>(nblocks, 1) * kTB, 0ull);
  for (i64 b = 0; b < nblocks; ++b)
    for (i64 i = b * kTB; i < std::min(n, b * kTB + kTB); ++i)
    {
      const i64 r = i - b * kTB;
      EIG_CHECK(split[i] - rp[i] <= kSlab, EIG_ERR_ARG, "staged image: a row has more than kSlab outside entries");
      S.w[b] = std::max(S.w[b], (i32)(split[i] - rp[i]));
      for (i64 q = rp[i]; q < split[i]; ++q)
      {
        const i64 at = (b * kSlab + (q - rp[i])) * kTB + r;
        S.v1[at] = cv[q];
        S.c1[at] = cj[q];
      }
      for (i64 q = split[i]; q < rp[i + 1]; ++q)
      {
        const i64 t = cj[q] - b * kTB;
        S.tile[(size_t)b * kTB * kTB + t * kTB + r] = cv[q];
        S.tmask[(size_t)b * kTB + r] |= 1ull << t;
      }
    }
  return S;
}

}  // namespace eigmi
