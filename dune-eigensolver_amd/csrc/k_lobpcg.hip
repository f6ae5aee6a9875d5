// k_lobpcg.hip -- the two streaming kernels of LOBPCG (lobpcg.cpp), gfx950:
//
//   k_lobpcg_resid    R = KX - MX diag(theta) and the 2 m column sums ||r_j||^2, ||(MX)_j||^2 in one
//                     pass over KX and MX
//   k_lobpcg_update   [X' P'] = S [C_x C_p] in place on the basis S = [X | W | P] (or [X | W]), both
//                     products on v_mfma_f64_16x16x4f64
//
// Layout: MultiVector<double,8>, column block c of a multivector with leading dimension ld is ld
// rows of 8 contiguous doubles at Q + 8 c ld (k_block.hip).  An n x 3 m multivector is three n x m
// ones back to back, so X, W and P are the column blocks [0, m/8), [m/8, 2 m/8) and [2 m/8, 3 m/8).
#include <algorithm>

#include "internal.h"
#include "reduce_dev.h"

namespace eigmi {

// ---------------------------------------------------------------------------------------------
// Residual.  Workgroup (x, y): column block y, rows strided by x; quad mapping (4 lanes per row,
// lane cp holds columns 2 cp, 2 cp + 1: one wave instruction reads 16 whole 64-B rows).
// r = kx - theta mx is one product and one subtraction, each rounded on its own, so the host
// reproduces R bit for bit.  Sums: per lane sequential over its rows, lanes of one column pair by
// xor shuffles over lane bits 2..5, waves in wave order, workgroups by grid_sum2 (reduction group =
// column block y, its own ticket): a fixed order, bitwise reproducible, no floating-point atomics.
// sums[j] = ||r_j||^2, sums[m + j] = ||(MX)_j||^2.
// ---------------------------------------------------------------------------------------------
constexpr int kResidThreads = 256;
constexpr int kResidMaxBlocks = 1024;

__global__ __launch_bounds__(kResidThreads) void k_lobpcg_resid(i64 n, i64 ld, int m, const double *__restrict__ KX,
                                                                const double *__restrict__ MX,
                                                                const double *__restrict__ theta,
                                                                double *__restrict__ R, double *__restrict__ sums,
                                                                double *partials, unsigned *tickets)
{
  constexpr int E = 16;
  __shared__ double wsum[kResidThreads / 64][E];
  __shared__ double vals[E];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, cp = threadIdx.x & 3;
  const int cb = blockIdx.y;
  const double t0 = theta[8 * cb + 2 * cp], t1 = theta[8 * cb + 2 * cp + 1];
  const double *kx = KX + (i64)cb * ld * 8 + 2 * cp;
  const double *mx = MX + (i64)cb * ld * 8 + 2 * cp;
  double *rr = R + (i64)cb * ld * 8 + 2 * cp;
  double v[4] = {0.0, 0.0, 0.0, 0.0};  // ||r||^2 and ||mx||^2 of this lane's two columns
  const i64 stride = (i64)gridDim.x * (kResidThreads / 4);
  for (i64 r = ((i64)blockIdx.x * kResidThreads + threadIdx.x) >> 2; r < n; r += stride)
  {
    const dv2 a = *reinterpret_cast<const dv2 *>(kx + r * 8);
    const dv2 b = *reinterpret_cast<const dv2 *>(mx + r * 8);
    dv2 d;
    d[0] = __dsub_rn(a[0], __dmul_rn(t0, b[0]));
    d[1] = __dsub_rn(a[1], __dmul_rn(t1, b[1]));
    *reinterpret_cast<dv2 *>(rr + r * 8) = d;
    v[0] += d[0] * d[0];
    v[1] += d[1] * d[1];
    v[2] += b[0] * b[0];
    v[3] += b[1] * b[1];
  }
#pragma unroll
  for (int msk = 4; msk < 64; msk <<= 1)
#pragma unroll
    for (int q = 0; q < 4; ++q) v[q] += __shfl_xor(v[q], msk, 64);
  if (lane < 4)
  {
    wsum[wave][2 * cp] = v[0];
    wsum[wave][2 * cp + 1] = v[1];
    wsum[wave][8 + 2 * cp] = v[2];
    wsum[wave][8 + 2 * cp + 1] = v[3];
  }
  __syncthreads();
  if (threadIdx.x < E)
  {
    double t = 0.0;
#pragma unroll
    for (int w = 0; w < kResidThreads / 64; ++w) t += wsum[w][threadIdx.x];
    vals[threadIdx.x] = t;
  }
  __syncthreads();
  double *part = partials + (size_t)cb * (gridDim.x + 8) * E;
  if (!grid_sum2<kResidThreads>(vals, E, part, part + (size_t)gridDim.x * E, tickets + (size_t)cb * kTicketStride,
                                blockIdx.x, gridDim.x, vals))
    return;
  if (threadIdx.x < E) sums[(threadIdx.x >> 3) * m + 8 * cb + (threadIdx.x & 7)] = vals[threadIdx.x];
}

void launch_lobpcg_resid(eig_ctx_t ctx, i64 n, i64 ld, i64 m, const double *KX, const double *MX,
                         const double *theta, double *R, double *sums, hipStream_t s)
{
  EIG_CHECK(n > 0 && m >= 8 && m <= 32 && m % 8 == 0, EIG_ERR_ARG, "lobpcg residual: n > 0, m in {8, 16, 24, 32}");
  const int gx = (int)std::max<i64>(1, std::min<i64>(kResidMaxBlocks, (n + 63) / 64));
  static_assert((size_t)4 * (kResidMaxBlocks + 8) * 16 <= (size_t)kMaxRedBlocks * kMaxRedVals, "partials fit");
  hipLaunchKernelGGL(k_lobpcg_resid, dim3(gx, (unsigned)(m / 8)), dim3(kResidThreads), 0, s, n, ld, (int)m, KX, MX,
                     theta, R, sums, ctx->red.partials, ctx->red.ticket(0));
  EIG_HIP(hipGetLastError());
}

// ---------------------------------------------------------------------------------------------
// Update.  With the basis S = [X | W | P] (KB = 3) or [X | W] (KB = 2) of 8 MB columns each and
// C = [C_x C_p] (8 KB MB x 16 MB, row-major): X <- S C_x, P <- S C_p, in place; W stays.
// A wave takes 16 rows per iteration (k_cholqr_fold's operand layout): lane (k, i) = (lane >> 4,
// lane & 15) loads columns 2 k, 2 k + 1 of row i of every 8-column block (a 16-B load; one wave
// instruction reads 16 whole 64-B rows), and MFMA h of block cb takes inner index k -> basis column
// 8 cb + 2 k + h with B[k][j] = C[8 cb + 2 k + h][16 t + j] for output tile t, held in registers
// for the whole launch.  The 2 m = 16 MB output columns are MB tiles of 16: column oc < m is X'
// column oc, column oc >= m is P' column oc - m.  The accumulator holds row k + 4 q, column 16 t + i.
// In place: a wave has read its 16 rows completely (the MFMAs depend on every load) before it
// writes them, and no other wave touches them; the next tile's loads are issued before the MFMAs.
// At KB = 2 the P slice is written, never read.  grid.y = the family (S, KS, MS).
// ---------------------------------------------------------------------------------------------
constexpr int kUpdThreads = 256;
struct LobpcgFamilies {
  double *f[3];
};

template <int MB, int KB>
__device__ __forceinline__ void upd_load(const double *S, i64 ld, i64 row, int k, dv2 (&z)[KB * MB])
{
#pragma unroll
  for (int cb = 0; cb < KB * MB; ++cb) z[cb] = *reinterpret_cast<const dv2 *>(S + ((i64)cb * ld + row) * 8 + 2 * k);
}

template <int MB, int KB>
__global__ __launch_bounds__(kUpdThreads) void k_lobpcg_update(i64 n, i64 ld, LobpcgFamilies fam,
                                                               const double *__restrict__ C)
{
  constexpr int NB = KB * MB;  // basis column blocks read
  constexpr int NT = MB;       // output tiles of 16 columns
  constexpr int M2 = 16 * MB;  // columns of C
  double *S = fam.f[blockIdx.y];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int k = lane >> 4, i = lane & 15;
  double cf[NB][2][NT];
#pragma unroll
  for (int cb = 0; cb < NB; ++cb)
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
      for (int t = 0; t < NT; ++t) cf[cb][h][t] = C[(size_t)(8 * cb + 2 * k + h) * M2 + 16 * t + i];
  // where this lane's accumulator column goes: column block and column inside it
  i64 ooff[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t)
  {
    const int oc = 16 * t + i;
    const int blk = oc < 8 * MB ? (oc >> 3) : 2 * MB + ((oc - 8 * MB) >> 3);
    ooff[t] = (i64)blk * ld * 8 + (oc & 7);
  }
  const i64 ntile = (n + 15) / 16;
  const i64 ws = (i64)gridDim.x * (kUpdThreads / 64);
  i64 tile = (i64)blockIdx.x * (kUpdThreads / 64) + wave;
  if (tile >= ntile) return;
  dv2 z[NB];
  upd_load<MB, KB>(S, ld, (tile * 16 + i < n ? tile * 16 + i : n - 1), k, z);
  while (true)
  {
    const i64 next = tile + ws;
    const bool more = next < ntile;
    dv2 zn[NB];
    if (more) upd_load<MB, KB>(S, ld, (next * 16 + i < n ? next * 16 + i : n - 1), k, zn);
    d4 acc[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[t] = d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int cb = 0; cb < NB; ++cb)
#pragma unroll
      for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int t = 0; t < NT; ++t) acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(z[cb][h], cf[cb][h][t], acc[t], 0, 0, 0);
#pragma unroll
    for (int q = 0; q < 4; ++q)
    {
      const i64 row = tile * 16 + 4 * q + k;
      if (row < n)
      {
#pragma unroll
        for (int t = 0; t < NT; ++t) S[ooff[t] + row * 8] = acc[t][q];
      }
    }
    if (!more) break;
    for (int cb = 0; cb < NB; ++cb) z[cb] = zn[cb];
    tile = next;
  }
}

template <int MB, int KB>
static void update_launch(int gx, int nfam, i64 n, i64 ld, const LobpcgFamilies &fam, const double *C, hipStream_t s)
{
  hipLaunchKernelGGL((k_lobpcg_update<MB, KB>), dim3(gx, nfam), dim3(kUpdThreads), 0, s, n, ld, fam, C);
}

// The rows past n of the last tile read row n - 1 (a valid address) and are not stored: an MFMA output
// row depends on its own input row only.
void launch_lobpcg_update(eig_ctx_t ctx, i64 n, i64 ld, i64 m, int kb, double *S, double *KS, double *MS,
                          const double *C, hipStream_t s)
{
  EIG_CHECK(n > 0 && m >= 8 && m <= 32 && m % 8 == 0 && (kb == 2 || kb == 3) && S, EIG_ERR_ARG,
            "lobpcg update: n > 0, m in {8, 16, 24, 32}, kb in {2, 3}");
  LobpcgFamilies fam{{S, KS, MS}};
  int nfam = 1;
  if (KS) fam.f[nfam++] = KS;
  if (MS) fam.f[nfam++] = MS;
  const i64 ntile = (n + 15) / 16;
  // one wave per SIMD holds the coefficient tiles (up to 96 doubles a lane): a workgroup per CU and family
  const int gx = (int)std::max<i64>(1, std::min<i64>(ctx->num_cu, (ntile + 3) / 4));
  const int mb = (int)(m / 8);
#define EIG_UPD(MB_)                                                         \
  case MB_:                                                                  \
    if (kb == 2)                                                             \
      update_launch<MB_, 2>(gx, nfam, n, ld, fam, C, s);                     \
    else                                                                     \
      update_launch<MB_, 3>(gx, nfam, n, ld, fam, C, s);                     \
    break;
  switch (mb)
  {
    EIG_UPD(1)
    EIG_UPD(2)
    EIG_UPD(3)
    EIG_UPD(4)
  }
#undef EIG_UPD
  EIG_HIP(hipGetLastError());
}

}  // namespace eigmi
