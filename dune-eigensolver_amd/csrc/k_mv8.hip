// k_mv8.hip -- the sparse products on MultiVector<double,8> blocks (gfx950): SpMM on the SELL and
// blocked images with the Chebyshev and residual epilogues, and the column dots.  The dense
// tall-skinny kernels (Gram panel, block Gram-Schmidt / B-Gram-Schmidt) are in k_orth.hip.
//
// Layout is the reference's block-column-major MultiVector<double,8> (multivector.hh:130-139):
// column block b of an n x m multivector is n rows of 8 contiguous doubles (64 B) starting at
// Q + b*8*n.  Kernels keep the reference's per-element operation order wherever the result is
// not a reduction, so SpMM / projections are bitwise the reference arithmetic on equal inputs.
#include <algorithm>

#include <cstdlib>

#include "internal.h"
#include "reduce_dev.h"

namespace eigmi {

// ---------------------------------------------------------------------------------------------
// a2: Qout = A Qin (matmul_sparse_tallskinny_blocked, kernels_cpp.hh:626-657).
// A workgroup (4 waves) takes one 64-row SELL slice at a time; lane L of wave w handles row
// 16 w + L/4 of the slice and the column pair 2 (L%4), 2 (L%4)+1 (16-B loads of Qin rows) for up
// to MB column blocks, so the matrix slice is read once for MB column blocks.
// ---------------------------------------------------------------------------------------------
template <int MB>
__global__ __launch_bounds__(256) void k_spmm_mv8(i64 nrows, i64 nslices, const i64 *__restrict__ slice_ptr,
                                                  const double *__restrict__ val, const i32 *__restrict__ col,
                                                  const double *__restrict__ Qin, double *__restrict__ Qout, i64 n,
                                                  int nblk_total, int C)
{
  const int wave = threadIdx.x >> 6, L = threadIdx.x & 63;
  const int cp = L & 3;
  const int b0 = blockIdx.y * MB;
  const i64 nsub = (i64)nslices * (C / 64);  // 64-row sub-slices
  for (i64 ss = blockIdx.x; ss < nsub; ss += gridDim.x)
  {
    const i64 s = ss / (C / 64);
    const int ri = (int)(ss % (C / 64)) * 64 + wave * 16 + (L >> 2);
    const i64 base = slice_ptr[s];
    const int width = (int)((slice_ptr[s + 1] - base) / C);
    double2 acc[MB];
#pragma unroll
    for (int q = 0; q < MB; ++q) acc[q] = make_double2(0.0, 0.0);
    for (int k = 0; k < width; ++k)
    {
      const i32 c = col[base + (i64)k * C + ri];
      if (c < 0) continue;
      const double a = val[base + (i64)k * C + ri];
#pragma unroll
      for (int q = 0; q < MB; ++q)
      {
        if (b0 + q < nblk_total)
        {
          const double2 xv = *reinterpret_cast<const double2 *>(Qin + ((i64)(b0 + q) * n + c) * 8 + 2 * cp);
          acc[q].x += a * xv.x;
          acc[q].y += a * xv.y;
        }
      }
    }
    const i64 r = s * C + ri;
    if (r < nrows)
    {
#pragma unroll
      for (int q = 0; q < MB; ++q)
        if (b0 + q < nblk_total) *reinterpret_cast<double2 *>(Qout + ((i64)(b0 + q) * n + r) * 8 + 2 * cp) = acc[q];
    }
  }
}

// ---------------------------------------------------------------------------------------------
// a2 on square B x B blocks (B = 2, 3, 4; the reference throws "only implemented for
// FieldMatrix<..,1,1>" here): Qout = A Qin over the blocked SELL-64 image (internal.h: block column
// of entry k of slice row r at slice_ptr[s] + k*64 + r, value t = r_blk*B + c_blk at
// (slice_ptr[s] + k*64)*B*B + t*64 + r, padding col < 0).  Qin / Qout have n = nbrows*B scalar rows;
// block row I, component r is scalar row I*B + r.
// Mapping as k_spmm_mv8: a workgroup (4 waves) takes one 64-block-row slice at a time, lane L of
// wave w owns block row 16 w + L/4 and the column pair 2 (L%4), 2 (L%4)+1 of up to MB column blocks
// (B*MB double2 accumulators), so a slice's values are read once per MB column blocks.  The matrix
// stream (columns, values) is read once per workgroup row: nontemporal loads, the next block column
// fetched one entry ahead.  The B Qin rows of a block column are contiguous (B*64 B per column
// block), read as 16 B per lane.
// Arithmetic per scalar row and column: s = 0; over the stored blocks in stored order, over
// c = 0..B-1: s += a[r][c] * x[col*B + c] (products and sums rounded separately) -- the order of
// k_spmv_blk, and of the 1x1 product on the matrix's scalar expansion, so the result is bitwise both.
// ---------------------------------------------------------------------------------------------
// The slices workgroup blockIdx.x walks: s0, s0 + step, ... < s1.  xcd_map (gridDim.x a multiple of
// 8): the slices are cut into 8 contiguous shares and the workgroups with blockIdx.x % 8 == x -- dealt
// to XCD x (round-robin dispatch: a speed assumption only, as k_sell_mv8q's) -- walk share x, so the
// Qin rows an XCD's resident workgroups gather are one neighbourhood of the matrix, not the whole
// front of the grid, and stay in its own L2.  Otherwise the plain grid stride.
struct BlkSliceWalk {
  i64 s0, s1, step;
};
__device__ __forceinline__ BlkSliceWalk blk_slice_walk(i64 nslices, int xcd_map)
{
  const i64 share = xcd_map ? (nslices + 7) / 8 : nslices;
  BlkSliceWalk w;
  w.s0 = xcd_map ? (blockIdx.x & 7) * share + (blockIdx.x >> 3) : blockIdx.x;
  w.s1 = xcd_map ? min(nslices, ((blockIdx.x & 7) + 1) * share) : nslices;
  w.step = xcd_map ? gridDim.x >> 3 : gridDim.x;
  return w;
}

// acc[q][r] = column pair cp of (A Qin)(slice s, slice row ri, component r) for the column blocks
// b0 + q < nblk_total: the row sums of the blocked product in the order stated above.  Padding entries
// (col < 0) gather nothing.
template <int B, int MB>
__device__ __forceinline__ void spmm_blk_row(const i64 *__restrict__ slice_ptr, const double *__restrict__ val,
                                             const i32 *__restrict__ col, const double *__restrict__ Qin, i64 n,
                                             int nblk_total, int b0, i64 s, int ri, int cp, double2 (&acc)[MB][B])
{
  constexpr int BB = B * B;
  const i64 base = slice_ptr[s];
  const int width = (int)((slice_ptr[s + 1] - base) >> 6);
#pragma unroll
  for (int q = 0; q < MB; ++q)
#pragma unroll
    for (int r = 0; r < B; ++r) acc[q][r] = make_double2(0.0, 0.0);
  i32 c = width > 0 ? __builtin_nontemporal_load(col + base + ri) : -1;
  for (int k = 0; k < width; ++k)
  {
    const i32 cn = k + 1 < width ? __builtin_nontemporal_load(col + base + (i64)(k + 1) * 64 + ri) : -1;
    if (c >= 0)
    {
      const double *vb = val + (base + (i64)k * 64) * BB + ri;
      double a[BB];
#pragma unroll
      for (int t = 0; t < BB; ++t) a[t] = __builtin_nontemporal_load(vb + t * 64);
#pragma unroll
      for (int q = 0; q < MB; ++q)
      {
        if (b0 + q < nblk_total)
        {
          const double2 *xr = reinterpret_cast<const double2 *>(Qin + ((i64)(b0 + q) * n + (i64)c * B) * 8) + cp;
          double2 xv[B];
#pragma unroll
          for (int cc = 0; cc < B; ++cc) xv[cc] = xr[cc * 4];
#pragma unroll
          for (int r = 0; r < B; ++r)
          {
            double2 sacc = acc[q][r];
#pragma unroll
            for (int cc = 0; cc < B; ++cc)
            {
              sacc.x += a[r * B + cc] * xv[cc].x;
              sacc.y += a[r * B + cc] * xv[cc].y;
            }
            acc[q][r] = sacc;
          }
        }
      }
    }
    c = cn;
  }
}

template <int B, int MB>
__global__ __launch_bounds__(256) void k_spmm_blk_mv8(i64 nbrows, i64 nslices, const i64 *__restrict__ slice_ptr,
                                                      const double *__restrict__ val, const i32 *__restrict__ col,
                                                      const double *__restrict__ Qin, double *__restrict__ Qout, i64 n,
                                                      int nblk_total, int xcd_map)
{
  const int wave = threadIdx.x >> 6, L = threadIdx.x & 63;
  const int cp = L & 3;
  const int ri = wave * 16 + (L >> 2);
  const int b0 = blockIdx.y * MB;
  const BlkSliceWalk w = blk_slice_walk(nslices, xcd_map);
  for (i64 s = w.s0; s < w.s1; s += w.step)
  {
    double2 acc[MB][B];
    spmm_blk_row<B, MB>(slice_ptr, val, col, Qin, n, nblk_total, b0, s, ri, cp, acc);
    const i64 row = s * 64 + ri;
    if (row < nbrows)
    {
#pragma unroll
      for (int q = 0; q < MB; ++q)
        if (b0 + q < nblk_total)
        {
          double2 *yr = reinterpret_cast<double2 *>(Qout + ((i64)(b0 + q) * n + row * B) * 8) + cp;
#pragma unroll
          for (int r = 0; r < B; ++r) yr[r * 4] = acc[q][r];
        }
    }
  }
}

// One Chebyshev-Jacobi step of the mass solve fused into the blocked product (k_sell_mv8q<kCheb>'s
// epilogue, k_block.hip, on the blocked image): the same image, lane mapping, slice schedule and row
// sums as k_spmm_blk_mv8; then per scalar row I*B + r and column pair, with acc = (M x_k)_row,
//     x_{k+1} = omega (x_k + (gamma dinv[row]) (b - acc) - x_{k-1}) + x_{k-1}
// written in place over x_{k-1} (Xold: each lane reads its own rows before it stores them); x_k is
// the gathered input Xk, never Xold.  dinv is the inverse SCALAR diagonal (k_diag_inv_blk).  dinv, b
// and x_{k-1} are read once (nontemporal loads, nontemporal stores of the result); the row's own x_k
// was gathered through the diagonal block a moment ago.  Every epilogue access is under the store's
// guards (row < nbrows, b0 + q < nblk_total).
//
// BJ (block Jacobi, the multigrid smoother on blocks): dinv holds D_I^-1, the inverse of the diagonal block
// of every block row (B x B row-major), and the scaling becomes z = D_I^-1 t with t = b - acc over the
// node's B rows (z_r = sum over c = 0..B-1 in order of dinv[r][c] t_c, products and sums rounded
// separately), x_{k+1} = omega (x_k + gamma z - x_{k-1}) + x_{k-1}.  The B^2 doubles are loaded here, after
// the product's value registers are dead.  The point instance (BJ = false) is the code it was.
template <int B, int MB, bool BJ = false>
__global__ __launch_bounds__(256) void k_spmm_blk_mv8_cheb(i64 nbrows, i64 nslices, const i64 *__restrict__ slice_ptr,
                                                           const double *__restrict__ val,
                                                           const i32 *__restrict__ col, const double *__restrict__ Xk,
                                                           double *__restrict__ Xold, i64 n, int nblk_total,
                                                           int xcd_map, const double *__restrict__ Bv,
                                                           const double *__restrict__ dinv, double omega, double gamma)
{
  const int wave = threadIdx.x >> 6, L = threadIdx.x & 63;
  const int cp = L & 3;
  const int ri = wave * 16 + (L >> 2);
  const int b0 = blockIdx.y * MB;
  const BlkSliceWalk w = blk_slice_walk(nslices, xcd_map);
  for (i64 s = w.s0; s < w.s1; s += w.step)
  {
    double2 acc[MB][B];
    spmm_blk_row<B, MB>(slice_ptr, val, col, Xk, n, nblk_total, b0, s, ri, cp, acc);
    const i64 row = s * 64 + ri;
    if (row < nbrows)
    {
      double gd[BJ ? B * B : B];
      if constexpr (BJ)
      {
#pragma unroll
        for (int t = 0; t < B * B; ++t) gd[t] = __builtin_nontemporal_load(dinv + row * (B * B) + t);
      }
      else
      {
#pragma unroll
        for (int r = 0; r < B; ++r) gd[r] = gamma * __builtin_nontemporal_load(dinv + row * B + r);
      }
#pragma unroll
      for (int q = 0; q < MB; ++q)
        if (b0 + q < nblk_total)
        {
          const i64 at = ((i64)(b0 + q) * n + row * B) * 8 + 2 * cp;
          dv2 xk[B], bb[B], xo[B];
#pragma unroll
          for (int r = 0; r < B; ++r)
          {
            xk[r] = *reinterpret_cast<const dv2 *>(Xk + at + r * 8);
            bb[r] = __builtin_nontemporal_load(reinterpret_cast<const dv2 *>(Bv + at + r * 8));
            xo[r] = __builtin_nontemporal_load(reinterpret_cast<const dv2 *>(Xold + at + r * 8));
          }
          if constexpr (BJ)
          {
            dv2 t[B];
#pragma unroll
            for (int r = 0; r < B; ++r) t[r] = dv2{bb[r].x - acc[q][r].x, bb[r].y - acc[q][r].y};
#pragma unroll
            for (int r = 0; r < B; ++r)
            {
              dv2 z = dv2{0.0, 0.0};
#pragma unroll
              for (int c = 0; c < B; ++c)
              {
                z.x += gd[r * B + c] * t[c].x;
                z.y += gd[r * B + c] * t[c].y;
              }
              const double o0 = omega * (xk[r].x + gamma * z.x - xo[r].x) + xo[r].x;
              const double o1 = omega * (xk[r].y + gamma * z.y - xo[r].y) + xo[r].y;
              __builtin_nontemporal_store(dv2{o0, o1}, reinterpret_cast<dv2 *>(Xold + at + r * 8));
            }
            continue;
          }
#pragma unroll
          for (int r = 0; r < B; ++r)
          {
            const double o0 = omega * (xk[r].x + gd[r] * (bb[r].x - acc[q][r].x) - xo[r].x) + xo[r].x;
            const double o1 = omega * (xk[r].y + gd[r] * (bb[r].y - acc[q][r].y) - xo[r].y) + xo[r].y;
            __builtin_nontemporal_store(dv2{o0, o1}, reinterpret_cast<dv2 *>(Xold + at + r * 8));
          }
        }
    }
  }
}

// One Clenshaw step of the Chebyshev window filter (filter_host.h) fused into the blocked product: the same
// image, lane mapping, slice walk and row sums as k_spmm_blk_mv8 (spmm_blk_row); then per scalar row and column
// pair, with acc = (A x_k)_row,
//     out = s1 acc + s0 x_k + s2 x_old + g b        (fused multiply-adds: tolerance-checked)
// written in place over x_old (Xold: each lane reads its own rows before it stores them; s2 == 0, the filter's
// first two steps, reads none); x_k is the gathered input Xk, never Xold.  b and x_old are read once
// (nontemporal loads, nontemporal stores of the result); no D^-1 stream.  Every epilogue access is under the
// store's guards (row < nbrows, b0 + q < nblk_total).
template <int B, int MB>
__global__ __launch_bounds__(256) void k_spmm_blk_mv8_filt(i64 nbrows, i64 nslices, const i64 *__restrict__ slice_ptr,
                                                           const double *__restrict__ val,
                                                           const i32 *__restrict__ col, const double *__restrict__ Xk,
                                                           double *__restrict__ Xold, i64 n, int nblk_total,
                                                           int xcd_map, const double *__restrict__ Bv, double s1,
                                                           double s0, double s2, double g)
{
  const int wave = threadIdx.x >> 6, L = threadIdx.x & 63;
  const int cp = L & 3;
  const int ri = wave * 16 + (L >> 2);
  const int b0 = blockIdx.y * MB;
  const BlkSliceWalk w = blk_slice_walk(nslices, xcd_map);
  for (i64 s = w.s0; s < w.s1; s += w.step)
  {
    double2 acc[MB][B];
    spmm_blk_row<B, MB>(slice_ptr, val, col, Xk, n, nblk_total, b0, s, ri, cp, acc);
    const i64 row = s * 64 + ri;
    if (row < nbrows)
    {
#pragma unroll
      for (int q = 0; q < MB; ++q)
        if (b0 + q < nblk_total)
        {
          const i64 at = ((i64)(b0 + q) * n + row * B) * 8 + 2 * cp;
          dv2 xk[B], bb[B], xo[B];
#pragma unroll
          for (int r = 0; r < B; ++r)
          {
            xk[r] = *reinterpret_cast<const dv2 *>(Xk + at + r * 8);
            bb[r] = __builtin_nontemporal_load(reinterpret_cast<const dv2 *>(Bv + at + r * 8));
            xo[r] = dv2{0.0, 0.0};
          }
          if (s2 != 0.0)
          {
#pragma unroll
            for (int r = 0; r < B; ++r)
              xo[r] = __builtin_nontemporal_load(reinterpret_cast<const dv2 *>(Xold + at + r * 8));
          }
#pragma unroll
          for (int r = 0; r < B; ++r)
          {
            const double o0 = __builtin_fma(s1, acc[q][r].x, __builtin_fma(s0, xk[r].x, __builtin_fma(s2, xo[r].x, g * bb[r].x)));
            const double o1 = __builtin_fma(s1, acc[q][r].y, __builtin_fma(s0, xk[r].y, __builtin_fma(s2, xo[r].y, g * bb[r].y)));
            __builtin_nontemporal_store(dv2{o0, o1}, reinterpret_cast<dv2 *>(Xold + at + r * 8));
          }
        }
    }
  }
}

// R = Bv - A X: the residual epilogue on the blocked product (the multigrid's residual on blocks).  The same
// image, lane mapping, slice walk and row sums as k_spmm_blk_mv8 (spmm_blk_row), then one subtraction per
// element; every epilogue access is under the store's guards (row < nbrows, b0 + q < nblk_total).  R may be
// Bv (each lane reads its own B entries before it stores them), never X (the gathered input).
template <int B, int MB>
__global__ __launch_bounds__(256) void k_spmm_blk_mv8_resid(i64 nbrows, i64 nslices, const i64 *__restrict__ slice_ptr,
                                                            const double *__restrict__ val,
                                                            const i32 *__restrict__ col, const double *__restrict__ X,
                                                            double *R, i64 n, int nblk_total, int xcd_map,
                                                            const double *Bv)
{
  const int wave = threadIdx.x >> 6, L = threadIdx.x & 63;
  const int cp = L & 3;
  const int ri = wave * 16 + (L >> 2);
  const int b0 = blockIdx.y * MB;
  const BlkSliceWalk w = blk_slice_walk(nslices, xcd_map);
  for (i64 s = w.s0; s < w.s1; s += w.step)
  {
    double2 acc[MB][B];
    spmm_blk_row<B, MB>(slice_ptr, val, col, X, n, nblk_total, b0, s, ri, cp, acc);
    const i64 row = s * 64 + ri;
    if (row < nbrows)
    {
#pragma unroll
      for (int q = 0; q < MB; ++q)
        if (b0 + q < nblk_total)
        {
          const i64 at = ((i64)(b0 + q) * n + row * B) * 8 + 2 * cp;
          dv2 bb[B];
#pragma unroll
          for (int r = 0; r < B; ++r) bb[r] = *reinterpret_cast<const dv2 *>(Bv + at + r * 8);
#pragma unroll
          for (int r = 0; r < B; ++r)
            *reinterpret_cast<dv2 *>(R + at + r * 8) = dv2{bb[r].x - acc[q][r].x, bb[r].y - acc[q][r].y};
        }
    }
  }
}

// X = gamma D^-1 Bv with the block-diagonal D (binv: B x B row-major inverse per block row): the first step of
// the block-Jacobi Chebyshev recurrence, k_cheb_init's counterpart.  One thread per (column block, node, 16-B
// quarter); z_r summed over c = 0..B-1 in order as in k_spmm_blk_mv8_cheb<.., true>, then gamma * z_r.
template <int B>
__global__ __launch_bounds__(256) void k_cheb_init_bjac(i64 nbrows, int nblk, const double *__restrict__ Bv,
                                                        const double *__restrict__ binv, double gamma,
                                                        double *__restrict__ X)
{
  const i64 total = nbrows * nblk * 4;
  for (i64 idx = (i64)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (i64)gridDim.x * 256)
  {
    const int cp = (int)(idx & 3);
    const i64 nr = idx >> 2, cb = nr / nbrows, row = nr - cb * nbrows;
    const i64 at = (cb * nbrows * B + row * B) * 8 + 2 * cp;
    double d[B * B];
    dv2 t[B];
#pragma unroll
    for (int e = 0; e < B * B; ++e) d[e] = binv[row * (B * B) + e];
#pragma unroll
    for (int r = 0; r < B; ++r) t[r] = *reinterpret_cast<const dv2 *>(Bv + at + r * 8);
#pragma unroll
    for (int r = 0; r < B; ++r)
    {
      dv2 z = dv2{0.0, 0.0};
#pragma unroll
      for (int c = 0; c < B; ++c)
      {
        z.x += d[r * B + c] * t[c].x;
        z.y += d[r * B + c] * t[c].y;
      }
      *reinterpret_cast<dv2 *>(X + at + r * 8) = dv2{gamma * z.x, gamma * z.y};
    }
  }
}

// column blocks per workgroup of k_spmm_blk_mv8<B, .>: the most that keep the kernel at 4 waves per
// SIMD (<= 128 VGPRs) without scratch (DESIGN.md "Blocked SpMM")
template <int B>
constexpr int spmm_blk_mb()
{
  return B == 4 ? 2 : 4;
}

// grid.x of the blocked product kernels and whether they walk the XCD shares
static int spmm_blk_grid_x(const eig_mat_s &A, bool &xcd)
{
  static const bool flat = std::getenv("EIGMI_SPMM_BLK_FLAT") != nullptr;  // A/B: the plain grid stride
  // XCD shares need a grid of whole groups of 8 and at least a slice per workgroup
  xcd = !flat && A.nslices >= 64;
  int gx = grid_for(A.nslices, 1, kStreamBlocks);
  if (xcd) gx = std::min(kStreamBlocks, (gx + 7) / 8 * 8);
  return gx;
}

template <int B, int MB>
static void launch_spmm_blk_mb(const eig_mat_s &A, int nblk, const double *Qin, double *Qout, hipStream_t s)
{
  const int gy = (nblk + MB - 1) / MB;
  bool xcd;
  const int gx = spmm_blk_grid_x(A, xcd);
  hipLaunchKernelGGL((k_spmm_blk_mv8<B, MB>), dim3(gx, gy), dim3(256), 0, s, A.nb_rows, A.nslices, A.slice_ptr, A.val,
                     A.col, Qin, Qout, A.nb_rows * B, nblk, xcd ? 1 : 0);
}

// The Chebyshev step on blocks: one launch for all column blocks (grid.y), the product's grid and
// column blocks per workgroup (the epilogue's loads come after the product's value registers are dead:
// DESIGN.md "Block Lanczos on blocks" has the register counts).
template <int B, bool BJ = false>
static void launch_cheb_blk(const eig_mat_s &M, int nblk, const double *Xk, double *Xold, const double *Bv,
                            const double *dinv, double omega, double gamma, hipStream_t s)
{
  constexpr int MB = spmm_blk_mb<B>();
  const int gy = (nblk + MB - 1) / MB;
  bool xcd;
  const int gx = spmm_blk_grid_x(M, xcd);
  hipLaunchKernelGGL((k_spmm_blk_mv8_cheb<B, MB, BJ>), dim3(gx, gy), dim3(256), 0, s, M.nb_rows, M.nslices,
                     M.slice_ptr, M.val, M.col, Xk, Xold, M.nb_rows * B, nblk, xcd ? 1 : 0, Bv, dinv, omega, gamma);
}

// The filter step on blocks: the Chebyshev step's grid and column blocks per workgroup.
template <int B>
static void launch_filt_blk(const eig_mat_s &A, int nblk, const double *Xk, double *Xold, const double *Bv, double s1,
                            double s0, double s2, double g, hipStream_t s)
{
  constexpr int MB = spmm_blk_mb<B>();
  const int gy = (nblk + MB - 1) / MB;
  bool xcd;
  const int gx = spmm_blk_grid_x(A, xcd);
  hipLaunchKernelGGL((k_spmm_blk_mv8_filt<B, MB>), dim3(gx, gy), dim3(256), 0, s, A.nb_rows, A.nslices, A.slice_ptr,
                     A.val, A.col, Xk, Xold, A.nb_rows * B, nblk, xcd ? 1 : 0, Bv, s1, s0, s2, g);
}

template <int B>
static void launch_resid_blk(const eig_mat_s &A, int nblk, const double *X, const double *Bv, double *R, hipStream_t s)
{
  constexpr int MB = spmm_blk_mb<B>();
  const int gy = (nblk + MB - 1) / MB;
  bool xcd;
  const int gx = spmm_blk_grid_x(A, xcd);
  hipLaunchKernelGGL((k_spmm_blk_mv8_resid<B, MB>), dim3(gx, gy), dim3(256), 0, s, A.nb_rows, A.nslices, A.slice_ptr,
                     A.val, A.col, X, R, A.nb_rows * B, nblk, xcd ? 1 : 0, Bv);
}

static void check_blk_square(const eig_mat_s &M, const char *who)
{
  EIG_CHECK(M.br == M.bc && M.br >= 2 && M.br <= 4, EIG_ERR_BLOCKSIZE, std::string(who) + ": square blocks 2..4");
  EIG_CHECK(!M.ctx->distributed(), EIG_ERR_ARG, std::string(who) + ": single rank only");
  EIG_CHECK(M.R == 1 && M.nb_rows == M.nb_cols, EIG_ERR_SHAPE, std::string(who) + ": square matrix required");
}

void launch_resid_blk_mv8(const eig_mat_s &A, i64 m, const double *X, const double *Bv, double *R, hipStream_t s)
{
  const int nblk = (int)(m / 8);
  check_blk_square(A, "blocked residual");
  EIG_CHECK(X != R, EIG_ERR_ARG, "blocked residual: R must not be X");
  if (nblk <= 0 || A.nb_rows <= 0) return;
  switch (A.br)
  {
    case 2: launch_resid_blk<2>(A, nblk, X, Bv, R, s); break;
    case 3: launch_resid_blk<3>(A, nblk, X, Bv, R, s); break;
    default: launch_resid_blk<4>(A, nblk, X, Bv, R, s); break;
  }
  EIG_HIP(hipGetLastError());
}

void launch_filt_step_blk(const eig_mat_s &A, i64 m, const double *Xk, double *Xold, const double *Bv, double s1,
                          double s0, double s2, double g, hipStream_t s)
{
  const int nblk = (int)(m / 8);
  check_blk_square(A, "blocked filter step");
  EIG_CHECK(Xk != Xold && Bv != Xold, EIG_ERR_ARG, "blocked filter step: the output buffer must be neither x_k nor b");
  if (nblk <= 0 || A.nb_rows <= 0) return;
  switch (A.br)
  {
    case 2: launch_filt_blk<2>(A, nblk, Xk, Xold, Bv, s1, s0, s2, g, s); break;
    case 3: launch_filt_blk<3>(A, nblk, Xk, Xold, Bv, s1, s0, s2, g, s); break;
    default: launch_filt_blk<4>(A, nblk, Xk, Xold, Bv, s1, s0, s2, g, s); break;
  }
  EIG_HIP(hipGetLastError());
}

void launch_cheb_step_bjac(const eig_mat_s &M, i64 m, const double *Xk, double *Xold, const double *Bv,
                           const double *binv, double omega, double gamma, hipStream_t s)
{
  const int nblk = (int)(m / 8);
  check_blk_square(M, "block-Jacobi Chebyshev step");
  EIG_CHECK(Xk != Xold, EIG_ERR_ARG, "block-Jacobi Chebyshev step: x_k must not be the output buffer");
  if (nblk <= 0 || M.nb_rows <= 0) return;
  switch (M.br)
  {
    case 2: launch_cheb_blk<2, true>(M, nblk, Xk, Xold, Bv, binv, omega, gamma, s); break;
    case 3: launch_cheb_blk<3, true>(M, nblk, Xk, Xold, Bv, binv, omega, gamma, s); break;
    default: launch_cheb_blk<4, true>(M, nblk, Xk, Xold, Bv, binv, omega, gamma, s); break;
  }
  EIG_HIP(hipGetLastError());
}

void launch_cheb_init_bjac(const eig_mat_s &M, i64 m, const double *Bv, const double *binv, double gamma, double *X,
                           hipStream_t s)
{
  const int nblk = (int)(m / 8);
  check_blk_square(M, "block-Jacobi first step");
  if (nblk <= 0 || M.nb_rows <= 0) return;
  const int g = grid_for(M.nb_rows * nblk * 4, 256, kStreamBlocks);
  switch (M.br)
  {
    case 2: hipLaunchKernelGGL(k_cheb_init_bjac<2>, dim3(g), dim3(256), 0, s, M.nb_rows, nblk, Bv, binv, gamma, X); break;
    case 3: hipLaunchKernelGGL(k_cheb_init_bjac<3>, dim3(g), dim3(256), 0, s, M.nb_rows, nblk, Bv, binv, gamma, X); break;
    default: hipLaunchKernelGGL(k_cheb_init_bjac<4>, dim3(g), dim3(256), 0, s, M.nb_rows, nblk, Bv, binv, gamma, X); break;
  }
  EIG_HIP(hipGetLastError());
}

void launch_cheb_step_blk(const eig_mat_s &M, i64 m, const double *Xk, double *Xold, const double *Bv,
                          const double *dinv, double omega, double gamma, hipStream_t s)
{
  const int nblk = (int)(m / 8);
  EIG_CHECK(M.br == M.bc && M.br >= 2 && M.br <= 4, EIG_ERR_BLOCKSIZE, "blocked Chebyshev step: square blocks 2..4");
  EIG_CHECK(!M.ctx->distributed(), EIG_ERR_ARG, "blocked Chebyshev step: single rank only");
  EIG_CHECK(M.R == 1 && M.nb_rows == M.nb_cols, EIG_ERR_SHAPE, "blocked Chebyshev step: square matrix required");
  EIG_CHECK(Xk != Xold, EIG_ERR_ARG, "blocked Chebyshev step: x_k must not be the output buffer");
  if (nblk <= 0 || M.nb_rows <= 0) return;
  switch (M.br)
  {
    case 2: launch_cheb_blk<2>(M, nblk, Xk, Xold, Bv, dinv, omega, gamma, s); break;
    case 3: launch_cheb_blk<3>(M, nblk, Xk, Xold, Bv, dinv, omega, gamma, s); break;
    default: launch_cheb_blk<4>(M, nblk, Xk, Xold, Bv, dinv, omega, gamma, s); break;
  }
  EIG_HIP(hipGetLastError());
}

// One instantiation per block size, also for a narrow product: instantiations with 1 / 2 column
// blocks (72 / 98 VGPRs at B = 3, 7 / 4 waves per SIMD) ran m = 8 at the same 240-250 us as this one
// in a same-run A/B (DESIGN.md "Blocked SpMM": the kernel is bound by its memory-instruction rate,
// not by the waves in flight).
template <int B>
static void launch_spmm_blk(const eig_mat_s &A, int nblk, const double *Qin, double *Qout, hipStream_t s)
{
  launch_spmm_blk_mb<B, spmm_blk_mb<B>()>(A, nblk, Qin, Qout, s);
}

void launch_spmm_mv8(const eig_mat_s &A, i64 m, const double *Qin, double *Qout, hipStream_t s)
{
  const int nblk = (int)(m / 8);
  if (A.br == A.bc && A.br > 1)
  {
    // square blocks: the blocked image (R = 1), one rank, columns index Qin's scalar rows directly
    EIG_CHECK(!A.ctx->distributed(), EIG_ERR_ARG, "blocked SpMM: single rank only");
    EIG_CHECK(A.R == 1 && A.nb_rows == A.nb_cols, EIG_ERR_SHAPE, "blocked SpMM: square matrix required");
    if (nblk <= 0 || A.nb_rows <= 0) return;
    switch (A.br)
    {
      case 2: launch_spmm_blk<2>(A, nblk, Qin, Qout, s); return;
      case 3: launch_spmm_blk<3>(A, nblk, Qin, Qout, s); return;
      case 4: launch_spmm_blk<4>(A, nblk, Qin, Qout, s); return;
      default: break;
    }
  }
  EIG_CHECK(A.br == 1 && A.bc == 1, EIG_ERR_BLOCKSIZE,
            "matmul_sparse_tallskinny_blocked: only implemented for FieldMatrix<..,1,1> and square blocks 2..4");
  if (A.R == 1)
  {
    // row per lane over 64-row slices, window layout (k_block.hip); ld = n on one rank
    launch_sell_mv8(A, m, Qin, Qout, s);
    return;
  }
  const int MB = 4;
  const int gy = (nblk + MB - 1) / MB;
  const int gx = grid_for(A.nslices * A.R, 1, kStreamBlocks);
  // Qin is a window-layout multivector on one rank (window == n); columns index it directly.
  hipLaunchKernelGGL(k_spmm_mv8<MB>, dim3(gx, gy), dim3(256), 0, s, A.nb_rows, A.nslices, A.slice_ptr, A.val, A.col,
                     Qin, Qout, A.nb_rows, nblk, 64 * A.R);
}

void launch_spmm_dot_mv8(const eig_mat_s &A, i64 m, const double *X, double *Y, double *dp, hipStream_t s,
                         ReduceWS red)
{
  static const bool off = std::getenv("EIGMI_NO_SPMM_DOT") != nullptr;  // A/B: the two launches
  // the same kernel choice as launch_spmm_mv8 -> launch_sell_mv8 (box first, then the band march)
  if (!off && A.R == 1 && A.br == 1 && A.bc == 1)
  {
    if (launch_box_spmm_dot(A, m, X, Y, dp, red, s)) return;
    if (!box_spmm_applies(A, m) && launch_spmm_march_dot(A, m, X, Y, dp, red, s)) return;
  }
  launch_spmm_mv8(A, m, X, Y, s);
  launch_dot_diag_mv8(A.nb_rows * A.br, m, X, Y, dp, 0, s, red);  // scalar rows
}

bool launch_spmm_dot_gram_mv8(const eig_mat_s &A, i64 m, const double *X, double *Y, double *dp, double *gram,
                              hipStream_t s, ReduceWS red)
{
  if (m != 8 || A.R != 1 || A.br != 1 || A.bc != 1 || A.ctx->distributed()) return false;
  // the same kernel choice as launch_spmm_dot_mv8 (the row-class box kernel, else the band march);
  // the kernel's last workgroup also zeroes the look-ahead MGS's barrier word, so the MGS of this
  // block that follows (launch_mgs_lookahead_gram with this gram) needs no extra launch
  unsigned *bar = mgs_lookahead_state(A.ctx, A.ctx->stream).st + kMgsLaBar;
  const bool ok = launch_box_spmm_dot_gram(A, m, X, Y, dp, gram, red, s, bar) ||
                  (!box_spmm_applies(A, m) && launch_spmm_march_dot_gram(A, m, X, Y, dp, gram, red, s, bar));
  A.ctx->mgs.bar_clean = ok ? gram : nullptr;
  return ok;
}

// ---------------------------------------------------------------------------------------------
// a5: dp[j] = q1_j . q2_j (dot_products_diagonal_blocked, kernels_cpp.hh:24-55).  grid.y = column
// block; thread t always sees the column pair 2 (t%4) because the grid stride is a multiple of 4.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kStreamThreads) void k_dot_diag_mv8(i64 n, const double *__restrict__ Q1,
                                                                 const double *__restrict__ Q2, double *dp,
                                                                 double *partials, unsigned *tickets)
{
  __shared__ double tot[8];
  const i64 off = (i64)blockIdx.y * n * 8;
  const double2 *a = reinterpret_cast<const double2 *>(Q1 + off);
  const double2 *b = reinterpret_cast<const double2 *>(Q2 + off);
  const i64 n4 = n * 4;
  double sx = 0.0, sy = 0.0;
  for (i64 i = (i64)blockIdx.x * kStreamThreads + threadIdx.x; i < n4; i += (i64)gridDim.x * kStreamThreads)
  {
    const double2 x = a[i], y = b[i];
    sx += x.x * y.x;
    sy += x.y * y.y;
  }
  const int cp = threadIdx.x & 3;
  double v[8];
#pragma unroll
  for (int q = 0; q < 4; ++q)
  {
    v[2 * q] = (q == cp) ? sx : 0.0;
    v[2 * q + 1] = (q == cp) ? sy : 0.0;
  }
  if (grid_sum_n<8, kStreamThreads>(v, partials + (size_t)blockIdx.y * gridDim.x * 8, tickets + (size_t)blockIdx.y * kTicketStride, tot,
                                    blockIdx.x, gridDim.x))
  {
    if (threadIdx.x < 8) dp[blockIdx.y * 8 + threadIdx.x] = tot[threadIdx.x];
  }
}

void launch_dot_diag_mv8(i64 n, i64 m, const double *Q1, const double *Q2, double *dp, int ticket, hipStream_t s,
                         ReduceWS red)
{
  const int nb = (int)(m / 8);
  EIG_CHECK(ticket + nb <= kNumTickets, EIG_ERR_ARG, "dot_diag_mv8: too many column blocks");
  int G = grid_for(n * 4, (i64)kStreamThreads * 4, 1024);
  while ((i64)G * nb * 8 > (i64)kMaxRedBlocks * kMaxRedVals) G /= 2;
  hipLaunchKernelGGL(k_dot_diag_mv8, dim3(G, nb), dim3(kStreamThreads), 0, s, n, Q1, Q2, dp, red.partials,
                     red.ticket(ticket));
}

}  // namespace eigmi
