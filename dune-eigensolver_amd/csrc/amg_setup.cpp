// amg_setup.cpp -- host setup of the smoothed-aggregation AMG hierarchy (amg_setup.h): strength of connection,
// aggregation, the smoothed prolongator and its transpose, the Galerkin triple product and the stopping rule.
// No device call.  Every sum runs over a row's stored entries in turn, whatever the thread count.
#include "amg_setup.h"

#include <algorithm>
#include <cmath>
#include <string>
#include <thread>

namespace eigmi {

namespace {

int setup_threads() { return (int)std::min<unsigned>(16u, std::max(1u, std::thread::hardware_concurrency())); }

// C = L R (L: nrows x *, R: * x ncols): row i = sum over the stored k of row i of L, in turn, of L[i, k] * R[k, :],
// each entry summed from 0.0; columns ascending, every structural entry kept.  Threads take contiguous row ranges.
void spgemm(const MgCsr &L, i64 nrows, const MgCsr &R, i64 ncols, MgCsr &C)
{
  const int nt = (int)std::max<i64>(1, std::min<i64>(setup_threads(), nrows / 64));
  std::vector<std::vector<i32>> tcol(nt);
  std::vector<std::vector<double>> tval(nt);
  std::vector<i64> len(nrows, 0);
  std::vector<std::thread> th;
  for (int t = 0; t < nt; ++t)
    th.emplace_back([&, t] {
      const i64 b = nrows * t / nt, e = nrows * (t + 1) / nt;
      std::vector<double> acc(ncols, 0.0);
      std::vector<i64> mark(ncols, -1);
      std::vector<i32> list;
      for (i64 i = b; i < e; ++i)
      {
        list.clear();
        for (i64 p = L.rp[i]; p < L.rp[i + 1]; ++p)
        {
          const i64 k = L.col[p];
          const double v = L.val[p];
          for (i64 q = R.rp[k]; q < R.rp[k + 1]; ++q)
          {
            const i32 c = R.col[q];
            if (mark[c] != i)
            {
              mark[c] = i;
              acc[c] = 0.0;
              list.push_back(c);
            }
            acc[c] += v * R.val[q];
          }
        }
        std::sort(list.begin(), list.end());
        len[i] = (i64)list.size();
        for (i32 c : list)
        {
          tcol[t].push_back(c);
          tval[t].push_back(acc[c]);
        }
      }
    });
  for (auto &x : th) x.join();
  C.rp.assign(nrows + 1, 0);
  for (i64 i = 0; i < nrows; ++i) C.rp[i + 1] = C.rp[i] + len[i];
  C.col.clear();
  C.val.clear();
  C.col.reserve((size_t)C.rp[nrows]);
  C.val.reserve((size_t)C.rp[nrows]);
  for (int t = 0; t < nt; ++t)
  {
    C.col.insert(C.col.end(), tcol[t].begin(), tcol[t].end());
    C.val.insert(C.val.end(), tval[t].begin(), tval[t].end());
  }
}

}  // namespace

i64 amg_aggregate(i64 n, const i64 *rp, const i32 *col, const double *val, double theta_l, std::vector<i64> &agg)
{
  std::vector<double> d(n, 0.0);
  for (i64 i = 0; i < n; ++i)
  {
    for (i64 k = rp[i]; k < rp[i + 1]; ++k)
      if (col[k] == i) d[i] = val[k];
    EIG_CHECK(d[i] > 0.0, EIG_ERR_BREAKDOWN, "algebraic multigrid: a level has a non-positive diagonal entry");
  }
  auto strong = [&](i64 i, i64 k) {
    const i64 j = col[k];
    return j != i && std::fabs(val[k]) >= theta_l * std::sqrt(d[i] * d[j]);
  };
  agg.assign(n, -1);
  i64 na = 0;
  for (i64 i = 0; i < n; ++i)  // pass 1
  {
    if (agg[i] >= 0) continue;
    bool any = false, free = true;
    for (i64 k = rp[i]; k < rp[i + 1] && free; ++k)
      if (strong(i, k))
      {
        any = true;
        free = agg[col[k]] < 0;
      }
    if (!any || !free) continue;
    agg[i] = na;
    for (i64 k = rp[i]; k < rp[i + 1]; ++k)
      if (strong(i, k)) agg[col[k]] = na;
    ++na;
  }
  const std::vector<i64> after1 = agg;
  for (i64 i = 0; i < n; ++i)  // pass 2
  {
    if (agg[i] >= 0) continue;
    double best = -1.0;
    i64 target = -1;
    for (i64 k = rp[i]; k < rp[i + 1]; ++k)
      if (strong(i, k) && after1[col[k]] >= 0 && std::fabs(val[k]) > best)
      {
        best = std::fabs(val[k]);
        target = after1[col[k]];
      }
    if (target >= 0) agg[i] = target;
  }
  for (i64 i = 0; i < n; ++i)  // pass 3
  {
    if (agg[i] >= 0) continue;
    agg[i] = na;
    for (i64 k = rp[i]; k < rp[i + 1]; ++k)
      if (strong(i, k) && agg[col[k]] < 0) agg[col[k]] = na;
    ++na;
  }
  return na;
}

void amg_prolongator(const MgCsr &A, i64 n, const std::vector<i64> &agg, i64 nc, double lmax, MgCsr &P)
{
  const double omega = 4.0 / (3.0 * lmax);
  P.rp.assign(n + 1, 0);
  P.col.clear();
  P.val.clear();
  std::vector<double> acc(nc, 0.0);
  std::vector<i64> mark(nc, -1);
  std::vector<i32> list;
  for (i64 i = 0; i < n; ++i)
  {
    double dii = 0.0;
    for (i64 k = A.rp[i]; k < A.rp[i + 1]; ++k)
      if (A.col[k] == i) dii = A.val[k];
    EIG_CHECK(dii > 0.0, EIG_ERR_BREAKDOWN, "algebraic multigrid: a level has a non-positive diagonal entry");
    const double c = omega / dii;
    list.clear();
    auto touch = [&](i64 J) {
      if (mark[J] != i)
      {
        mark[J] = i;
        acc[J] = 0.0;
        list.push_back((i32)J);
      }
    };
    for (i64 k = A.rp[i]; k < A.rp[i + 1]; ++k)
    {
      const i64 J = agg[A.col[k]];
      touch(J);
      acc[J] += c * A.val[k];
    }
    touch(agg[i]);
    std::sort(list.begin(), list.end());
    for (i32 J : list)
    {
      const double v = (J == agg[i] ? 1.0 : 0.0) - acc[J];
      if (v == 0.0) continue;
      P.col.push_back(J);
      P.val.push_back(v);
    }
    P.rp[i + 1] = (i64)P.col.size();
  }
}

void amg_transpose(const MgCsr &P, i64 n, i64 nc, MgCsr &PT)
{
  PT.rp.assign(nc + 1, 0);
  for (i32 c : P.col) ++PT.rp[c + 1];
  for (i64 J = 0; J < nc; ++J) PT.rp[J + 1] += PT.rp[J];
  PT.col.assign(P.col.size(), 0);
  PT.val.assign(P.val.size(), 0.0);
  std::vector<i64> cur(PT.rp.begin(), PT.rp.end() - 1);
  for (i64 i = 0; i < n; ++i)
    for (i64 k = P.rp[i]; k < P.rp[i + 1]; ++k)
    {
      const i64 q = cur[P.col[k]]++;
      PT.col[q] = (i32)i;
      PT.val[q] = P.val[k];
    }
}

void amg_galerkin(const MgCsr &A, const MgCsr &P, const MgCsr &PT, i64 n, i64 nc, MgCsr &Ac)
{
  MgCsr AP, G;
  spgemm(A, n, P, nc, AP);
  spgemm(PT, nc, AP, nc, G);
  // the upper triangle (diagonal included) without exact zeros, then its strict part mirrored below: row I is
  // the mirrored entries (rows J < I ascending) followed by its own upper entries
  std::vector<i64> cnt(nc + 1, 0);
  for (i64 I = 0; I < nc; ++I)
    for (i64 k = G.rp[I]; k < G.rp[I + 1]; ++k)
    {
      const i64 J = G.col[k];
      if (J < I || G.val[k] == 0.0) continue;
      ++cnt[I + 1];
      if (J > I) ++cnt[J + 1];
    }
  Ac.rp.assign(nc + 1, 0);
  for (i64 I = 0; I < nc; ++I) Ac.rp[I + 1] = Ac.rp[I] + cnt[I + 1];
  Ac.col.assign((size_t)Ac.rp[nc], 0);
  Ac.val.assign((size_t)Ac.rp[nc], 0.0);
  std::vector<i64> cur(Ac.rp.begin(), Ac.rp.end() - 1);
  for (i64 I = 0; I < nc; ++I)  // lower parts: filled by ascending source row
    for (i64 k = G.rp[I]; k < G.rp[I + 1]; ++k)
    {
      const i64 J = G.col[k];
      if (J <= I || G.val[k] == 0.0) continue;
      const i64 q = cur[J]++;
      Ac.col[q] = (i32)I;
      Ac.val[q] = G.val[k];
    }
  for (i64 I = 0; I < nc; ++I)
    for (i64 k = G.rp[I]; k < G.rp[I + 1]; ++k)
    {
      const i64 J = G.col[k];
      if (J < I || G.val[k] == 0.0) continue;
      const i64 q = cur[I]++;
      Ac.col[q] = (i32)J;
      Ac.val[q] = G.val[k];
    }
}

void amg_build(MgCsr A0, i64 n, double theta, AmgHierarchy &H)
{
  EIG_CHECK(n >= 1 && theta >= 0.0 && (i64)A0.rp.size() == n + 1, EIG_ERR_ARG, "algebraic multigrid: bad argument");
  H = AmgHierarchy();
  H.A.push_back(std::move(A0));
  H.rows.push_back(n);
  for (;;)
  {
    const int l = (int)H.A.size() - 1;
    const i64 nl = H.rows[l];
    H.lmax.push_back(mg_gershgorin(H.A[l], nl));
    bool last = nl <= kAmgCoarsestRows;
    std::vector<i64> agg;
    i64 nc = 0;
    if (!last)
    {
      nc = amg_aggregate(nl, H.A[l].rp.data(), H.A[l].col.data(), H.A[l].val.data(), theta * std::ldexp(1.0, -l), agg);
      if (2 * nc > nl || l + 1 == kAmgMaxLevels)
      {
        std::string sizes;
        for (i64 r : H.rows) sizes += std::to_string(r) + " -> ";
        EIG_CHECK(nl <= kMgMaxCoarse, EIG_ERR_ARG,
                  "algebraic multigrid: the hierarchy stalls at " + sizes + std::to_string(nc) + " rows (a level must "
                  "coarsen by a factor 2 or have at most " + std::to_string(kMgMaxCoarse) + " rows, at most " +
                  std::to_string(kAmgMaxLevels) + " levels): lower theta");
        last = true;
      }
    }
    if (last)
    {
      mg_spectrum_bounds(H.A[l], nl, 1, H.clo, H.chi);
      H.clo *= 0.999;
      H.chi *= 1.001;
      H.cdeg = mg_coarse_degree(H.clo, H.chi);
      return;
    }
    MgCsr P, PT, Ac;
    amg_prolongator(H.A[l], nl, agg, nc, H.lmax[l], P);
    amg_transpose(P, nl, nc, PT);
    amg_galerkin(H.A[l], P, PT, nl, nc, Ac);
    H.P.push_back(std::move(P));
    H.PT.push_back(std::move(PT));
    H.A.push_back(std::move(Ac));
    H.rows.push_back(nc);
  }
}

}  // namespace eigmi
