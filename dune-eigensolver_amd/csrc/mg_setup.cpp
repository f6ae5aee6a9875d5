// mg_setup.cpp -- host setup of the multigrid hierarchy (mg_setup.h): node coarsening, the blocked Galerkin
// operator, the Jacobi / block-Jacobi smoother data and the coarsest level's spectrum bounds.  No device call.
#include "mg_setup.h"

#include <algorithm>
#include <cmath>
#include <string>
#include <thread>

namespace eigmi {

namespace {

int setup_threads() { return (int)std::min<unsigned>(16u, std::max(1u, std::thread::hardware_concurrency())); }

// per-direction coarse neighbours of fine index f: (c0, w) and (c1, w) (c = -1: none)
inline void split1(int f, int nc, int &c0, int &c1, double &w)
{
  if (f & 1)
  {
    c0 = (f - 1) >> 1;
    c1 = -1;
    w = 1.0;
  }
  else
  {
    c0 = (f >> 1) - 1;
    c1 = (f >> 1) < nc ? (f >> 1) : -1;
    w = 0.5;
  }
}

// D = L L^T (lower, row-major b x b); false when D is not positive definite (or not finite)
bool chol_lower(int b, const double *D, double *L)
{
  for (int i = 0; i < b * b; ++i) L[i] = 0.0;
  for (int j = 0; j < b; ++j)
  {
    double d = D[j * b + j];
    for (int k = 0; k < j; ++k) d -= L[j * b + k] * L[j * b + k];
    if (!(d > 0.0) || !std::isfinite(d)) return false;
    L[j * b + j] = std::sqrt(d);
    for (int i = j + 1; i < b; ++i)
    {
      double s = D[j * b + i];  // the upper triangle is the one the mirroring keeps
      for (int k = 0; k < j; ++k) s -= L[i * b + k] * L[j * b + k];
      L[i * b + j] = s / L[j * b + j];
    }
  }
  return true;
}

// Li = L^-1 (lower)
void lower_inv(int b, const double *L, double *Li)
{
  for (int i = 0; i < b * b; ++i) Li[i] = 0.0;
  for (int j = 0; j < b; ++j)
  {
    Li[j * b + j] = 1.0 / L[j * b + j];
    for (int i = j + 1; i < b; ++i)
    {
      double s = 0.0;
      for (int k = j; k < i; ++k) s += L[i * b + k] * Li[k * b + j];
      Li[i * b + j] = -s / L[i * b + i];
    }
  }
}

// the diagonal block of block row I (the last stored match, as the device's diagonal extraction), or null
const double *diag_block(const MgCsr &A, i64 I, int b)
{
  const double *d = nullptr;
  for (i64 k = A.rp[I]; k < A.rp[I + 1]; ++k)
    if (A.col[k] == I) d = &A.val[(size_t)k * b * b];
  return d;
}

// Li[I] = L_I^-1 of every diagonal block; EIG_ERR_BREAKDOWN when one is missing or not positive definite
void diag_factors(const MgCsr &A, i64 nb, int b, std::vector<double> &Li)
{
  const int bb = b * b;
  Li.assign((size_t)nb * bb, 0.0);
  for (i64 I = 0; I < nb; ++I)
  {
    double L[16];
    const double *D = diag_block(A, I, b);
    EIG_CHECK(D && chol_lower(b, D, L), EIG_ERR_BREAKDOWN,
              "multigrid: a level has a diagonal block that is not positive definite");
    lower_inv(b, L, &Li[(size_t)I * bb]);
  }
}

// N = Li_I A_IJ Li_J^T (b x b row-major)
inline void scaled_block(int b, const double *LiI, const double *a, const double *LiJ, double *N)
{
  double T[16];
  for (int r = 0; r < b; ++r)
    for (int c = 0; c < b; ++c)
    {
      double s = 0.0;
      for (int k = 0; k <= r; ++k) s += LiI[r * b + k] * a[k * b + c];
      T[r * b + c] = s;
    }
  for (int r = 0; r < b; ++r)
    for (int c = 0; c < b; ++c)
    {
      double s = 0.0;
      for (int k = 0; k <= c; ++k) s += T[r * b + k] * LiJ[c * b + k];
      N[r * b + c] = s;
    }
}

}  // namespace

i64 mg_coarsest_rows(int nx, int ny, int nz, int b)
{
  int d[3] = {nx, ny, nz};
  while (!mg_last_level(d))
    for (int &x : d) x /= 2;
  return (i64)d[0] * d[1] * d[2] * b;
}

void mg_galerkin(const MgCsr &A, int b, const int *fd, const int *cd, MgCsr &Ac)
{
  const int bb = b * b;
  const i64 nc = (i64)cd[0] * cd[1] * cd[2];
  std::vector<double> slot((size_t)nc * 27 * bb, 0.0);
  const int nt = setup_threads();
  std::vector<std::thread> th;
  std::vector<int> bad(nt, 0);
  for (int t = 0; t < nt; ++t)
    th.emplace_back([&, t] {
      for (i64 I = t; I < nc; I += nt)
      {
        const int X = (int)(I % cd[0]), Y = (int)((I / cd[0]) % cd[1]), Z = (int)(I / ((i64)cd[0] * cd[1]));
        double *acc = &slot[(size_t)I * 27 * bb];
        for (int dz = -1; dz <= 1; ++dz)
        {
          const int z = 2 * Z + 1 + dz;
          if (z < 0 || z >= fd[2]) continue;
          for (int dy = -1; dy <= 1; ++dy)
          {
            const int y = 2 * Y + 1 + dy;
            if (y < 0 || y >= fd[1]) continue;
            for (int dx = -1; dx <= 1; ++dx)
            {
              const int x = 2 * X + 1 + dx;
              if (x < 0 || x >= fd[0]) continue;
              const double wi = (dz ? 0.5 : 1.0) * (dy ? 0.5 : 1.0) * (dx ? 0.5 : 1.0);
              const i64 i = ((i64)z * fd[1] + y) * fd[0] + x;
              for (i64 k = A.rp[i]; k < A.rp[i + 1]; ++k)
              {
                const i64 j = A.col[k];
                const int jx = (int)(j % fd[0]), jy = (int)((j / fd[0]) % fd[1]), jz = (int)(j / ((i64)fd[0] * fd[1]));
                int cz[2], cy[2], cx[2];
                double wz, wy, wx;
                split1(jz, cd[2], cz[0], cz[1], wz);
                split1(jy, cd[1], cy[0], cy[1], wy);
                split1(jx, cd[0], cx[0], cx[1], wx);
                const double wj = wz * wy * wx;
                const double *v = &A.val[(size_t)k * bb];
                for (int p = 0; p < 2; ++p)
                {
                  if (cz[p] < 0) continue;
                  for (int q = 0; q < 2; ++q)
                  {
                    if (cy[q] < 0) continue;
                    for (int r = 0; r < 2; ++r)
                    {
                      if (cx[r] < 0) continue;
                      const int oz = cz[p] - Z, oy = cy[q] - Y, ox = cx[r] - X;
                      if (oz < -1 || oz > 1 || oy < -1 || oy > 1 || ox < -1 || ox > 1)
                      {
                        bad[t] = 1;
                        continue;
                      }
                      double *dst = acc + (size_t)((oz + 1) * 9 + (oy + 1) * 3 + (ox + 1)) * bb;
                      for (int e = 0; e < bb; ++e) dst[e] += wi * v[e] * wj;
                    }
                  }
                }
              }
            }
          }
        }
      }
    });
  for (auto &x : th) x.join();
  for (int f : bad)
    EIG_CHECK(!f, EIG_ERR_ARG, "multigrid: the matrix couples nodes more than one grid step apart (not a box stencil "
                               "on the given grid)");
  // mirror the upper blocks into the lower ones (transposed) and the diagonal blocks' upper triangles into their
  // lower ones, then compress (in-bounds neighbours, ascending columns)
  for (i64 I = 0; I < nc; ++I)
  {
    const int X = (int)(I % cd[0]), Y = (int)((I / cd[0]) % cd[1]), Z = (int)(I / ((i64)cd[0] * cd[1]));
    for (int s = 0; s < 13; ++s)  // offsets before the centre: J < I
    {
      const int oz = s / 9 - 1, oy = (s / 3) % 3 - 1, ox = s % 3 - 1;
      const int jx = X + ox, jy = Y + oy, jz = Z + oz;
      if (jx < 0 || jx >= cd[0] || jy < 0 || jy >= cd[1] || jz < 0 || jz >= cd[2]) continue;
      const i64 J = ((i64)jz * cd[1] + jy) * cd[0] + jx;
      double *lo = &slot[((size_t)I * 27 + s) * bb];
      const double *up = &slot[((size_t)J * 27 + (26 - s)) * bb];
      for (int r = 0; r < b; ++r)
        for (int c = 0; c < b; ++c) lo[r * b + c] = up[c * b + r];
    }
    double *dg = &slot[((size_t)I * 27 + 13) * bb];
    for (int r = 1; r < b; ++r)
      for (int c = 0; c < r; ++c) dg[r * b + c] = dg[c * b + r];
  }
  Ac.rp.assign(nc + 1, 0);
  Ac.col.clear();
  Ac.val.clear();
  Ac.col.reserve((size_t)nc * 27);
  Ac.val.reserve((size_t)nc * 27 * bb);
  for (i64 I = 0; I < nc; ++I)
  {
    const int X = (int)(I % cd[0]), Y = (int)((I / cd[0]) % cd[1]), Z = (int)(I / ((i64)cd[0] * cd[1]));
    for (int s = 0; s < 27; ++s)
    {
      const int oz = s / 9 - 1, oy = (s / 3) % 3 - 1, ox = s % 3 - 1;
      const int jx = X + ox, jy = Y + oy, jz = Z + oz;
      if (jx < 0 || jx >= cd[0] || jy < 0 || jy >= cd[1] || jz < 0 || jz >= cd[2]) continue;
      Ac.col.push_back((i32)(((i64)jz * cd[1] + jy) * cd[0] + jx));
      const double *v = &slot[((size_t)I * 27 + s) * bb];
      Ac.val.insert(Ac.val.end(), v, v + bb);
    }
    Ac.rp[I + 1] = (i64)Ac.col.size();
  }
}

double mg_gershgorin(const MgCsr &A, i64 n)
{
  double g = 0.0;
  for (i64 r = 0; r < n; ++r)
  {
    double d = 0.0, s = 0.0;
    for (i64 k = A.rp[r]; k < A.rp[r + 1]; ++k)
    {
      s += std::fabs(A.val[k]);
      if (A.col[k] == r) d = A.val[k];
    }
    EIG_CHECK(d > 0.0, EIG_ERR_BREAKDOWN, "multigrid: a level has a non-positive diagonal entry");
    g = std::max(g, s / d);
  }
  return g;
}

double mg_block_jacobi(const MgCsr &A, i64 nb, int b, std::vector<double> &dinv)
{
  EIG_CHECK(b >= 1 && b <= 4, EIG_ERR_BLOCKSIZE, "multigrid: block Jacobi takes blocks 1..4");
  const int bb = b * b;
  std::vector<double> Li;
  diag_factors(A, nb, b, Li);
  // D^-1 = L^-T L^-1: the upper triangle computed, the lower mirrored
  dinv.assign((size_t)nb * bb, 0.0);
  for (i64 I = 0; I < nb; ++I)
  {
    const double *l = &Li[(size_t)I * bb];
    double *d = &dinv[(size_t)I * bb];
    for (int r = 0; r < b; ++r)
      for (int c = r; c < b; ++c)
      {
        double s = 0.0;
        for (int k = c; k < b; ++k) s += l[k * b + r] * l[k * b + c];
        d[r * b + c] = s;
        d[c * b + r] = s;
      }
  }
  const int nt = setup_threads();
  std::vector<double> best(nt, 0.0);
  std::vector<std::thread> th;
  for (int t = 0; t < nt; ++t)
    th.emplace_back([&, t] {
      std::vector<double> G(bb), w, Z;
      double N[16];
      for (i64 I = t; I < nb; I += nt)
      {
        double sum = 0.0;
        for (i64 k = A.rp[I]; k < A.rp[I + 1]; ++k)
        {
          scaled_block(b, &Li[(size_t)I * bb], &A.val[(size_t)k * bb], &Li[(size_t)A.col[k] * bb], N);
          for (int r = 0; r < b; ++r)  // G = N^T N, symmetric bitwise
            for (int c = r; c < b; ++c)
            {
              double s = 0.0;
              for (int e = 0; e < b; ++e) s += N[e * b + r] * N[e * b + c];
              G[r * b + c] = G[c * b + r] = s;
            }
          sym_eig(b, G, w, Z);
          sum += std::sqrt(std::max(w.back(), 0.0));
        }
        best[t] = std::max(best[t], sum);
      }
    });
  for (auto &x : th) x.join();
  return *std::max_element(best.begin(), best.end());
}

void mg_spectrum_bounds(const MgCsr &A, i64 nb, int b, double &lo, double &hi)
{
  const i64 n = nb * b;
  const int bb = b * b;
  std::vector<double> S((size_t)n * n, 0.0), w, Z;
  if (b == 1)
  {
    std::vector<double> d(n);
    for (i64 r = 0; r < n; ++r)
      for (i64 k = A.rp[r]; k < A.rp[r + 1]; ++k)
        if (A.col[k] == r) d[r] = A.val[k];
    for (i64 r = 0; r < n; ++r)
      for (i64 k = A.rp[r]; k < A.rp[r + 1]; ++k)
        S[(size_t)r * n + A.col[k]] = A.val[k] / std::sqrt(d[r] * d[A.col[k]]);
  }
  else
  {
    std::vector<double> Li;
    diag_factors(A, nb, b, Li);
    double N[16];
    // the upper blocks computed, the lower ones (and the diagonal blocks' lower triangles) mirrored
    for (i64 I = 0; I < nb; ++I)
      for (i64 k = A.rp[I]; k < A.rp[I + 1]; ++k)
      {
        const i64 J = A.col[k];
        if (J < I) continue;
        scaled_block(b, &Li[(size_t)I * bb], &A.val[(size_t)k * bb], &Li[(size_t)J * bb], N);
        for (int r = 0; r < b; ++r)
          for (int c = (J == I ? r : 0); c < b; ++c)
          {
            S[(size_t)(I * b + r) * n + J * b + c] = N[r * b + c];
            S[(size_t)(J * b + c) * n + I * b + r] = N[r * b + c];
          }
      }
  }
  sym_eig((int)n, S, w, Z);
  lo = w.front();
  hi = w.back();
  EIG_CHECK(lo > 0.0, EIG_ERR_BREAKDOWN, "multigrid: the coarsest operator is not positive definite");
}

int mg_coarse_degree(double clo, double chi)
{
  const double kappa = chi / clo, rho = (std::sqrt(kappa) - 1.0) / (std::sqrt(kappa) + 1.0);
  int deg = rho > 0.0 ? (int)std::ceil(std::log(0.5e-15) / std::log(rho)) : 1;
  return std::min(std::max(deg, 1), 2000);
}

}  // namespace eigmi
