// k_amg.hip -- transfers of the smoothed-aggregation algebraic multigrid (mg.cpp, amg_setup.cpp) on window-layout
// MultiVector<double,8> panels (gfx950).  The panels are rectangular: the fine one has ldf rows, the coarse ldc.
//
//   k_amg_restrict     Bc(I, :)  = sum_k PT[I, k] Rf(col_k, :)      (PT = P^T stored as its own CSR)
//   k_amg_prolong_add  Xf(i, :) += sum_k P[i, k]  Xc(col_k, :)
//
// Both are a row gather on a row-pointer CSR (i64 rowptr, i32 columns, double values): one (row, 8-column block)
// per lane quad, lane q of the quad moving the 16-B piece q of the 64-B panel rows -- the mapping of
// k_lobpcg_resid and k_mg_* -- and blockIdx.y the column block.  A row's entries are summed in stored (ascending
// column) order from 0, so a result depends on nothing but its row: no atomics, run-to-run bitwise equal.  The
// four lanes of a quad read the same (column, value) pair (one request, broadcast), the 16 rows of a wave read one
// contiguous stretch of the CSR arrays, and the gathered 64-B panel rows -- 64 B per entry and column block against
// 12 B of index and value -- are the traffic that counts.  The image has no padding: only stored entries are
// read, so a panel row that no stored entry of a row names never reaches that row's sum, and only the `rows`
// owned rows of the output are written.
#include <algorithm>

#include "internal.h"

namespace eigmi {

namespace {

constexpr int kAmgRows = 64;  // rows per 256-thread workgroup (four lanes each)

// U consecutive stored entries from k on: the U index / value pairs, then the U gathered 16-B pieces, all issued
// before the first is used (U loads in flight per lane); added in stored order
template <int U>
__device__ __forceinline__ void amg_entries(i64 k, int q, const i32 *__restrict__ col, const double *__restrict__ val,
                                            const double *__restrict__ in, double &a0, double &a1)
{
  i32 c[U];
  double w[U];
  double2 v[U];
#pragma unroll
  for (int u = 0; u < U; ++u)
  {
    c[u] = col[k + u];
    w[u] = val[k + u];
  }
#pragma unroll
  for (int u = 0; u < U; ++u) v[u] = *reinterpret_cast<const double2 *>(in + (i64)c[u] * 8 + q * 2);
#pragma unroll
  for (int u = 0; u < U; ++u)
  {
    a0 += w[u] * v[u].x;
    a1 += w[u] * v[u].y;
  }
}

// sum_k val[k] * In(col[k], piece q) over the stored entries of row r, in turn: batches of 8 (the long rows of
// P^T are a chain of dependent gathers otherwise), then 4, 2, 1 (a row of P has 3 or 4 entries on average)
__device__ __forceinline__ double2 amg_row_sum(i64 r, int q, const i64 *__restrict__ rp, const i32 *__restrict__ col,
                                               const double *__restrict__ val, const double *__restrict__ in)
{
  double a0 = 0.0, a1 = 0.0;
  const i64 k1 = rp[r + 1];
  i64 k = rp[r];
  for (; k + 8 <= k1; k += 8) amg_entries<8>(k, q, col, val, in, a0, a1);
  if (k + 4 <= k1)
  {
    amg_entries<4>(k, q, col, val, in, a0, a1);
    k += 4;
  }
  if (k + 2 <= k1)
  {
    amg_entries<2>(k, q, col, val, in, a0, a1);
    k += 2;
  }
  if (k < k1) amg_entries<1>(k, q, col, val, in, a0, a1);
  return make_double2(a0, a1);
}

}  // namespace

// Bc (rows x 8 per column block, ldc rows allocated) = PT Rf (ldf rows per column block)
__global__ __launch_bounds__(256) void k_amg_restrict(i64 rows, const i64 *__restrict__ rp, const i32 *__restrict__ col,
                                                      const double *__restrict__ val, i64 ldf, i64 ldc,
                                                      const double *__restrict__ Rf, double *__restrict__ Bc)
{
  const double *in = Rf + (i64)blockIdx.y * ldf * 8;
  double *out = Bc + (i64)blockIdx.y * ldc * 8;
  const int q = threadIdx.x & 3;
  for (i64 r = (i64)blockIdx.x * kAmgRows + (threadIdx.x >> 2); r < rows; r += (i64)gridDim.x * kAmgRows)
    *reinterpret_cast<double2 *>(out + r * 8 + q * 2) = amg_row_sum(r, q, rp, col, val, in);
}

// Xf (rows x 8 per column block, ldf rows allocated) += P Xc (ldc rows per column block)
__global__ __launch_bounds__(256) void k_amg_prolong_add(i64 rows, const i64 *__restrict__ rp,
                                                         const i32 *__restrict__ col, const double *__restrict__ val,
                                                         i64 ldf, i64 ldc, const double *__restrict__ Xc,
                                                         double *__restrict__ Xf)
{
  const double *in = Xc + (i64)blockIdx.y * ldc * 8;
  double *out = Xf + (i64)blockIdx.y * ldf * 8;
  const int q = threadIdx.x & 3;
  for (i64 r = (i64)blockIdx.x * kAmgRows + (threadIdx.x >> 2); r < rows; r += (i64)gridDim.x * kAmgRows)
  {
    double2 *dst = reinterpret_cast<double2 *>(out + r * 8 + q * 2);
    const double2 x = *dst;  // (its latency overlaps the gather)
    const double2 a = amg_row_sum(r, q, rp, col, val, in);
    *dst = make_double2(x.x + a.x, x.y + a.y);
  }
}

namespace {
inline unsigned amg_grid(i64 rows, i64 m)
{
  const i64 g = (rows + kAmgRows - 1) / kAmgRows, cap = 8 * (i64)kStreamBlocks / (m / 8);
  return (unsigned)std::max<i64>(1, std::min(g, cap));
}
}  // namespace

// cn coarse rows; PT's device CSR (cn + 1 row pointers)
void launch_amg_restrict(i64 cn, const i64 *rp, const i32 *col, const double *val, i64 m, i64 ldf, i64 ldc,
                         const double *Rf, double *Bc, hipStream_t s)
{
  EIG_CHECK(m > 0 && m % 8 == 0 && cn >= 0 && ldc >= cn, EIG_ERR_ARG, "algebraic multigrid restriction: bad shape");
  if (cn == 0) return;
  hipLaunchKernelGGL(k_amg_restrict, dim3(amg_grid(cn, m), (unsigned)(m / 8)), dim3(256), 0, s, cn, rp, col, val, ldf,
                     ldc, Rf, Bc);
  EIG_HIP(hipGetLastError());
}

// fn fine rows; P's device CSR (fn + 1 row pointers)
void launch_amg_prolong_add(i64 fn, const i64 *rp, const i32 *col, const double *val, i64 m, i64 ldf, i64 ldc,
                            const double *Xc, double *Xf, hipStream_t s)
{
  EIG_CHECK(m > 0 && m % 8 == 0 && fn >= 0 && ldf >= fn, EIG_ERR_ARG, "algebraic multigrid prolongation: bad shape");
  if (fn == 0) return;
  hipLaunchKernelGGL(k_amg_prolong_add, dim3(amg_grid(fn, m), (unsigned)(m / 8)), dim3(256), 0, s, fn, rp, col, val,
                     ldf, ldc, Xc, Xf);
  EIG_HIP(hipGetLastError());
}

}  // namespace eigmi
