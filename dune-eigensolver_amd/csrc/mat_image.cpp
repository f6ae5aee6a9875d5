// mat_image.cpp -- builds the host images of mat_image.h from a host CSR matrix.  Every bitwise guarantee of the
// kernels rests on these passes: a row sums exactly its stored entries in ascending-column order, a band slot
// holds whichever mirror is stored, and the geometric masks are a property of the pattern alone.
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <thread>

#include "mat_image.h"

namespace eigmi {

int mat_image_threads = 0;

namespace {

template <class F>
void parallel_slices(i64 ns, F &&f)
{
  unsigned nt = std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
  if (mat_image_threads > 0) nt = (unsigned)mat_image_threads;
  if (ns < 4096) nt = 1;
  if (nt == 1) f(0, ns);
  else
  {
    std::vector<std::thread> th;
    for (unsigned t = 0; t < nt; ++t) th.emplace_back([&, t] { f(ns * t / nt, ns * (t + 1) / nt); });
    for (auto &t : th) t.join();
  }
}

}  // namespace

// Build the SELL-C image (C = 64 R) of `nb` block rows (rowptr/col/vals on the host; columns are
// shifted by col_shift into window-local block columns; global row = row_begin + r).
// 1x1 slices whose rows use at most 8 distinct offsets (col - row) become stencil slices: their
// value slots are indexed by offset and a per-row mask marks the stored entries (internal.h).
SellImage build_sell_image(const MatShape &A, i64 nb, const int64_t *rowptr, const int32_t *col, const double *vals,
                           i64 col_shift)
{
  SellImage S;
  const int bb = A.br * A.bc;
  const i64 C = 64;  // R = 1, one row per lane
  const i64 ns = (nb + C - 1) / C;
  const bool try_stencil = (bb == 1) && !(A.kflags & EIG_MAT_NO_STENCIL);
  const i64 row0 = A.row_begin;
  std::vector<i32> &swidth = S.st_width, &sdelta = S.st_delta;
  swidth.assign(ns, -1);
  sdelta.assign(8 * (size_t)ns, 0);
  std::vector<i64> &sp = S.slice_ptr, wdt(ns, 0);
  sp.assign(ns + 1, 0);
  parallel_slices(ns, [&](i64 s0, i64 s1) {
    std::vector<i64> offs;
    for (i64 s = s0; s < s1; ++s)
    {
      i64 w = 0;
      offs.clear();
      bool ok = try_stencil;
      for (i64 r = s * C; r < std::min(nb, s * C + C); ++r)
      {
        w = std::max<i64>(w, rowptr[r + 1] - rowptr[r]);
        for (i64 p = rowptr[r]; ok && p < rowptr[r + 1]; ++p)
        {
          const i64 d = (i64)col[p] - (row0 + r);
          if (std::find(offs.begin(), offs.end(), d) == offs.end())
          {
            if (offs.size() == 8 || d < INT32_MIN || d > INT32_MAX) ok = false;
            else offs.push_back(d);
          }
        }
      }
      if (ok && !offs.empty())
      {
        std::sort(offs.begin(), offs.end());
        swidth[s] = (i32)offs.size();
        for (size_t k = 0; k < offs.size(); ++k) sdelta[8 * s + k] = (i32)offs[k];
        w = (i64)offs.size();
      }
      wdt[s] = w;
    }
  });
  for (i64 s = 0; s < ns; ++s) sp[s + 1] = sp[s] + C * wdt[s];
  const i64 total = sp[ns];
  std::vector<i32> &cimg = S.col;
  std::vector<double> &vimg = S.val;
  std::vector<uint8_t> &mimg = S.st_mask;
  cimg.resize(std::max<i64>(total, 1));
  vimg.resize(std::max<i64>(total * bb, 1));
  mimg.assign(try_stencil ? (size_t)(ns * C) : 0, 0);
  parallel_slices(ns, [&](i64 s0, i64 s1) {
    for (i64 s = s0; s < s1; ++s)
    {
      const i64 base = sp[s], w = (sp[s + 1] - base) / C;
      for (i64 l = 0; l < C; ++l)
      {
        const i64 r = s * C + l;
        const i64 len = (r < nb) ? rowptr[r + 1] - rowptr[r] : 0;
        for (i64 k = 0; k < w; ++k)
        {
          cimg[base + k * C + l] = -1;
          for (int t = 0; t < bb; ++t) vimg[(base + k * C) * bb + t * C + l] = 0.0;
        }
        for (i64 e = 0; e < len; ++e)
        {
          const i64 p = rowptr[r] + e;
          i64 k = e;
          if (swidth[s] > 0)
          {
            const i64 d = (i64)col[p] - (row0 + r);
            k = std::find(&sdelta[8 * s], &sdelta[8 * s] + swidth[s], (i32)d) - &sdelta[8 * s];
            mimg[s * C + l] |= (uint8_t)(1u << k);
          }
          cimg[base + k * C + l] = (i32)(col[p] - col_shift);
          for (int t = 0; t < bb; ++t) vimg[(base + k * C) * bb + t * C + l] = vals[p * bb + t];
        }
      }
    }
  });
  {
    std::vector<i64> bw(16, 0);
    const i64 nt = std::min<i64>(16, std::max<i64>(1, nb / 65536));
    std::vector<std::thread> th;
    for (i64 t = 0; t < nt; ++t)
      th.emplace_back([&, t] {
        i64 m = 0;
        for (i64 r = nb * t / nt; r < nb * (t + 1) / nt; ++r)
          for (i64 p = rowptr[r]; p < rowptr[r + 1]; ++p) m = std::max<i64>(m, std::llabs((i64)col[p] - (row0 + r)));
        bw[t] = m;
      });
    for (auto &x : th) x.join();
    S.bandwidth = *std::max_element(bw.begin(), bw.end());
  }
  S.nslices = ns;
  S.nnzb_padded = total;
  S.n_stencil_slices = 0;
  S.sell_explicit = 0;
  for (i64 q = 0; q < ns; ++q)
  {
    S.n_stencil_slices += swidth[q] > 0;
    if (swidth[q] <= 0) S.sell_explicit += sp[q + 1] - sp[q];
  }
  return S;
}

namespace {

// uniform band: one value per array over every stored entry, lower entries included (a lower entry
// whose mirror is not stored on this rank -- a ghost row's coupling, or a one-sided pattern -- was
// never compared in the mirror pass, and the uniform march kernels take the array's constant for it)
void uniform_band(SymImage &S, i64 nb, i64 row0, const int64_t *rowptr, const int32_t *col, const double *vals,
                  const std::vector<i64> &offs, const std::vector<int> &kj)
{
  const int nup = S.nup;
  auto kof = [&](i64 d) { return (int)(std::lower_bound(offs.begin(), offs.end(), d) - offs.begin()); };
  std::mutex mu;
  std::vector<double> uc(nup, 0.0);
  std::vector<char> seen(nup, 0);
  bool uni = true;
  parallel_slices(nb, [&](i64 r0, i64 r1) {
    std::vector<double> v(nup, 0.0);
    std::vector<char> sn(nup, 0);
    bool ok = true;
    for (i64 r = r0; r < r1 && ok; ++r)
      for (i64 p = rowptr[r]; p < rowptr[r + 1]; ++p)
      {
        const i64 d = (i64)col[p] - (row0 + r);
        const int j = kj[kof(d)];
        if (!sn[j])
        {
          sn[j] = 1;
          v[j] = vals[p];
        }
        else if (std::memcmp(&v[j], &vals[p], sizeof(double)) != 0)
        {
          ok = false;
          break;
        }
      }
    std::lock_guard<std::mutex> lk(mu);
    uni = uni && ok;
    for (int j = 0; j < nup && uni; ++j)
      if (sn[j])
      {
        if (!seen[j])
        {
          seen[j] = 1;
          uc[j] = v[j];
        }
        else if (std::memcmp(&uc[j], &v[j], sizeof(double)) != 0)
          uni = false;
      }
  });
  S.uniform = uni;
  for (int j = 0; j < nup; ++j) S.uc[j] = uni ? uc[j] : 0.0;
}

// geometric masks: a grid whose rows store exactly their in-grid neighbours -- the whole grid on
// one rank, or a rank's slab of whole planes (row0 and nb multiples of the plane size D; z is
// the global plane, so the slab's first / last planes keep their ghost-plane bits).  A property of
// the pattern alone: the uniform marches take the values from their arguments, the value march
// (march variant 10) streams them from the band arrays.
void geometric_masks(SymImage &S, const MatShape &A, i64 nb, const std::vector<i64> &offs)
{
  const int nd = S.nd, mb = S.mask_bytes;
  const i64 row0 = A.row_begin;
  const std::vector<uint8_t> &m8 = S.mask8;
  S.geo = false;
  if (mb == 1 && offs.front() == -offs.back() && (nd == 7 || nd == 5))
  {
    const i64 D = offs.back();
    const i64 nx = nd == 7 ? offs[5] : D;
    bool shape = D > 1 && nx > 1 && D % nx == 0 && nb % D == 0 && row0 % D == 0 && A.nb_rows_global % D == 0 &&
                 (nd == 5 || (offs[4] == 1 && offs[2] == -1 && offs[1] == -nx && nx < D));
    if (nd == 5) shape = shape && offs[1] == -1 && offs[3] == 1;
    if (shape)
    {
      const i64 ny = D / nx, nz = A.nb_rows_global / D;
      std::atomic<bool> same{true};
      parallel_slices(nb, [&](i64 r0, i64 r1) {
        for (i64 r = r0; r < r1 && same.load(std::memory_order_relaxed); ++r)
        {
          const i64 g = row0 + r;
          const i64 x = g % nx, y = (g / nx) % ny, z = g / D;
          unsigned e = 0;
          int k = 0;
          e |= (z > 0 ? 1u : 0u) << k++;
          if (nd == 7) e |= (y > 0 ? 1u : 0u) << k++;
          e |= (x > 0 ? 1u : 0u) << k++;
          e |= 1u << k++;
          e |= (x < nx - 1 ? 1u : 0u) << k++;
          if (nd == 7) e |= (y < ny - 1 ? 1u : 0u) << k++;
          e |= (z < nz - 1 ? 1u : 0u) << k++;
          if (e != m8[r]) same = false;
        }
      });
      if (same && nx <= INT32_MAX && ny <= INT32_MAX && nz <= INT32_MAX)
      {
        S.geo = true;
        S.gx = (int)nx;
        S.gy = (int)ny;
        S.gz = (int)nz;
        S.gz0 = (int)(row0 / D);
      }
    }
  }
}

// box-geometric masks (general 27-point box subsets, e.g. the P1 Kuhn 15-point stencil): decompose the
// offsets as a D + b nx + c -- nx the smallest offset > 1 (or that + 1 when (0, 1, -1) is stored), D
// the smallest offset past nx + 1 (or that + 1, + nx - 1, + nx, + nx + 1) -- then check row by row
void box27_masks(SymImage &S, const MatShape &A, i64 nb, const std::vector<i64> &offs)
{
  const int nd = S.nd, mb = S.mask_bytes;
  const i64 row0 = A.row_begin;
  const std::vector<uint8_t> &m8 = S.mask8;
  const std::vector<uint32_t> &m32 = S.mask32;
  S.box27 = 0;
  if (!S.geo && nd >= 3 && nd <= 27 && offs.front() == -offs.back())
  {
    i64 s1 = 0;
    for (i64 d : offs)
      if (d > 1 && (s1 == 0 || d < s1)) s1 = d;
    std::vector<int> bx(nd), by(nd), bz(nd);
    auto decompose = [&](i64 nxc, i64 Dc) {
      for (int k = 0; k < nd; ++k)
      {
        bool found = false;
        for (int a = -1; a <= 1 && !found; ++a)
          for (int b2 = -1; b2 <= 1 && !found; ++b2)
            for (int c = -1; c <= 1 && !found; ++c)
              if (a * Dc + b2 * nxc + c == offs[k]) bz[k] = a, by[k] = b2, bx[k] = c, found = true;
        if (!found) return false;
      }
      return true;
    };
    i64 gnx = 0, gD = 0;
    for (i64 nxc : {s1, s1 + 1})
    {
      if (nxc < 3 || gD) continue;
      i64 t = 0;
      for (i64 d : offs)
        if (d > nxc + 1 && (t == 0 || d < t)) t = d;
      if (t == 0) continue;
      for (i64 Dc : {t, t + 1, t + nxc - 1, t + nxc, t + nxc + 1})
        if (!gD && Dc % nxc == 0 && Dc / nxc >= 3 && A.nb_rows_global % Dc == 0 && nb % Dc == 0 && row0 % Dc == 0 &&
            decompose(nxc, Dc))
          gnx = nxc, gD = Dc;
    }
    if (gD && A.nb_rows_global / gD >= 3 && gnx <= INT32_MAX && gD / gnx <= INT32_MAX &&
        A.nb_rows_global / gD <= INT32_MAX)
    {
      decompose(gnx, gD);
      const i64 gny = gD / gnx, gnz = A.nb_rows_global / gD;
      std::atomic<bool> same{true};
      parallel_slices(nb, [&](i64 r0, i64 r1) {
        for (i64 r = r0; r < r1 && same.load(std::memory_order_relaxed); ++r)
        {
          const i64 g = row0 + r;
          const i64 x = g % gnx, y = (g / gnx) % gny, z = g / gD;
          uint32_t e = 0;
          for (int k = 0; k < nd; ++k)
          {
            const i64 xx = x + bx[k], yy = y + by[k], zz = z + bz[k];
            if (xx >= 0 && xx < gnx && yy >= 0 && yy < gny && zz >= 0 && zz < gnz) e |= 1u << k;
          }
          if (e != (mb == 1 ? (uint32_t)m8[r] : m32[r])) same = false;
        }
      });
      if (same)
      {
        for (int k = 0; k < nd; ++k) S.box27 |= 1u << ((bz[k] + 1) * 9 + (by[k] + 1) * 3 + (bx[k] + 1));
        S.gx = (int)gnx;
        S.gy = (int)gny;
        S.gz = (int)gnz;
        S.gz0 = (int)(row0 / gD);
      }
    }
  }
}

}  // namespace

// Symmetric band image (internal.h, eig_mat_s::sym_*) next to the SELL image, for square 1x1
// matrices with at most kSymMaxOff distinct offsets whose stored mirror pairs are bitwise equal
// and whose band arrays are smaller than the SELL values.  Pass 1 (rows in parallel) stores each
// row's entries at d >= 0 in slot [j(d)][w]; pass 2 stores the entries at d < 0 in slot
// [j(-d)][w + d], which only the mirror (row w + d, offset -d) of pass 1 can also own -- a set
// slot with different bits rejects the image.  Ghost rows below the owned range (distributed)
// get their slots from the owned rows' lower entries alone.  built stays false when not applicable.
SymImage build_sym_image(const MatShape &A, i64 nslices, i64 nnzb_padded, i64 nb, const int64_t *rowptr,
                         const int32_t *col, const double *vals)
{
  SymImage S;
  if (A.br != 1 || A.bc != 1 || (A.kflags & EIG_MAT_NO_BAND) || nb == 0) return S;
  if (A.nb_cols != A.nb_rows_global) return S;
  const i64 row0 = A.row_begin;
  // distinct offsets (per thread, then merged)
  std::vector<i64> offs;
  {
    std::mutex mu;
    bool ok = true;
    parallel_slices(nb, [&](i64 r0, i64 r1) {
      std::vector<i64> mine;
      for (i64 r = r0; r < r1 && mine.size() <= (size_t)kSymMaxOff; ++r)
        for (i64 p = rowptr[r]; p < rowptr[r + 1]; ++p)
        {
          const i64 d = (i64)col[p] - (row0 + r);
          if (std::find(mine.begin(), mine.end(), d) == mine.end()) mine.push_back(d);
        }
      std::lock_guard<std::mutex> lk(mu);
      if (mine.size() > (size_t)kSymMaxOff) ok = false;
      for (i64 d : mine)
        if (std::find(offs.begin(), offs.end(), d) == offs.end()) offs.push_back(d);
    });
    if (!ok || offs.size() > (size_t)kSymMaxOff || offs.empty()) return S;
  }
  std::sort(offs.begin(), offs.end());
  std::vector<i64> ups;
  for (i64 d : offs)
  {
    if (d < INT32_MIN || d > INT32_MAX) return S;
    const i64 a = std::llabs(d);
    if (std::find(ups.begin(), ups.end(), a) == ups.end()) ups.push_back(a);
  }
  std::sort(ups.begin(), ups.end());
  const int nd = (int)offs.size(), nup = (int)ups.size();
  const i64 ns = nslices, own = A.own_offset;
  const i64 ld = ((std::max<i64>(A.window, own + ns * 64) + 63) / 64) * 64;
  // only worth it when the band arrays are smaller than the SELL values the kernels would stream
  if ((double)nup * (double)ld > 0.9 * (double)nnzb_padded) return S;
  auto jof = [&](i64 a) { return (int)(std::lower_bound(ups.begin(), ups.end(), a) - ups.begin()); };
  std::vector<int> kj(nd);
  for (int k = 0; k < nd; ++k) kj[k] = jof(std::llabs(offs[k]));
  std::vector<double> &U = S.val;
  U.assign((size_t)nup * ld, 0.0);
  std::vector<uint8_t> set((size_t)nup * ld, 0);
  const int mb = nd <= 8 ? 1 : 4;
  std::vector<uint8_t> &m8 = S.mask8;
  std::vector<uint32_t> &m32 = S.mask32;
  m8.assign(mb == 1 ? (size_t)ns * 64 : 0, 0);
  m32.assign(mb == 4 ? (size_t)ns * 64 : 0, 0);
  std::atomic<bool> good{true};
  auto kof = [&](i64 d) { return (int)(std::lower_bound(offs.begin(), offs.end(), d) - offs.begin()); };
  parallel_slices(nb, [&](i64 r0, i64 r1) {
    for (i64 r = r0; r < r1; ++r)
    {
      uint32_t m = 0;
      for (i64 p = rowptr[r]; p < rowptr[r + 1]; ++p)
      {
        const i64 d = (i64)col[p] - (row0 + r);
        const int k = kof(d);
        m |= 1u << k;
        if (d >= 0)
        {
          const size_t q = (size_t)kj[k] * ld + (size_t)(own + r);
          U[q] = vals[p];
          set[q] = 1;
        }
      }
      if (mb == 1) m8[r] = (uint8_t)m;
      else m32[r] = m;
    }
  });
  parallel_slices(nb, [&](i64 r0, i64 r1) {
    for (i64 r = r0; r < r1 && good.load(std::memory_order_relaxed); ++r)
      for (i64 p = rowptr[r]; p < rowptr[r + 1]; ++p)
      {
        const i64 d = (i64)col[p] - (row0 + r);
        if (d >= 0) break;  // ascending columns: the rest are upper entries
        const i64 x = own + r + d;
        if (x < 0 || x >= ld)
        {
          good = false;
          break;
        }
        const size_t q = (size_t)kj[kof(d)] * ld + (size_t)x;
        if (set[q])
        {
          if (std::memcmp(&U[q], &vals[p], sizeof(double)) != 0)
          {
            good = false;
            break;
          }
        }
        else
          U[q] = vals[p];
      }
  });
  if (!good) return SymImage();
  S.mask_bytes = mb;
  S.nd = nd;
  S.nup = nup;
  S.ld = ld;
  for (int k = 0; k < nd; ++k)
  {
    S.off[k] = (i32)offs[k];
    S.dj[k] = kj[k];
  }
  uniform_band(S, nb, row0, rowptr, col, vals, offs, kj);
  geometric_masks(S, A, nb, offs);
  box27_masks(S, A, nb, offs);
  S.built = true;
  return S;
}

SliceSplit split_slices(i64 nslices, i64 nb, i64 row_begin, const int64_t *rowptr, const int32_t *col, i64 D)
{
  SliceSplit S;
  // interior / boundary slices: a slice is interior when every column is owned
  std::vector<i32> &inter = S.interior, &bound = S.boundary;
  const i64 own_lo = row_begin, own_hi = row_begin + nb;
  for (i64 s = 0; s < nslices; ++s)
  {
    bool in = true;
    const i64 C = 64;
    for (i64 r = s * C; r < std::min(nb, s * C + C) && in; ++r)
      for (i64 p = rowptr[r]; p < rowptr[r + 1]; ++p)
        if (col[p] < own_lo || col[p] >= own_hi)
        {
          in = false;
          break;
        }
    (in ? inter : bound).push_back((i32)s);
  }
  // plane-march split: the longest run of planes whose slices are all interior (>= 2 planes)
  if (D > 0)
  {
    const i64 spp = D / 64, np = (nb + D - 1) / D;
    std::vector<char> is_in(nslices, 0);
    for (i32 q : inter) is_in[q] = 1;
    i64 best0 = 0, best1 = 0;
    for (i64 z = 0; z < np;)
    {
      auto plane_in = [&](i64 zz) {
        for (i64 q = zz * spp; q < std::min(nslices, (zz + 1) * spp); ++q)
          if (!is_in[q]) return false;
        return true;
      };
      if (!plane_in(z))
      {
        ++z;
        continue;
      }
      i64 e = z;
      while (e < np && plane_in(e)) ++e;
      if (e - z > best1 - best0) best0 = z, best1 = e;
      z = e;
    }
    if (best1 - best0 >= 2)
    {
      for (i64 q = 0; q < nslices; ++q)
        if (q < best0 * spp || q >= best1 * spp) S.march_bnd.push_back((i32)q);
      S.mz0 = best0;
      S.mz1 = best1;
    }
  }
  return S;
}

void validate_csr(i64 nb, i64 ncols, const int64_t *rowptr, const int32_t *col)
{
  EIG_CHECK(rowptr[0] == 0, EIG_ERR_ARG, "rowptr[0] must be 0");
  for (i64 r = 0; r < nb; ++r)
  {
    EIG_CHECK(rowptr[r + 1] >= rowptr[r], EIG_ERR_ARG, "rowptr must be non-decreasing");
    for (i64 p = rowptr[r]; p < rowptr[r + 1]; ++p)
    {
      EIG_CHECK(col[p] >= 0 && col[p] < ncols, EIG_ERR_SHAPE, "column index out of range");
      if (p > rowptr[r]) EIG_CHECK(col[p] > col[p - 1], EIG_ERR_ARG, "columns must be strictly ascending per row");
    }
  }
}

DiagShare diag_share(int br, int bc, i64 nb, i64 row_begin, const int64_t *rowptr, const int32_t *col,
                     const double *vals)
{
  DiagShare S;
  for (i64 r = 0; r < nb; ++r)
    for (i64 p = rowptr[r]; p < rowptr[r + 1]; ++p)
      if (col[p] == row_begin + r)
        for (int i = 0; i < std::min(br, bc); ++i)
        {
          S.sum += vals[p * br * bc + (i64)i * bc + i];
          ++S.count;
        }
  return S;
}

}  // namespace eigmi
