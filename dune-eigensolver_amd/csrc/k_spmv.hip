// k_spmv.hip -- sparse matrix x vector on the SELL-C image (gfx950).
//
// Replaces BCRSMatrix::mv (dune-istl; called at arpack_geneo_wrapper.hh:275 through multMvB)
// and the b = 1 product matmul_sparse_tallskinny_naive (kernels_cpp.hh:596-621).
//
// Layout (internal.h): slices of C = 64 R block rows, one wavefront per slice; lane l owns the R
// adjacent rows l R .. l R + R - 1.  Entry k of slice row r sits at slice_ptr[s] + k C + r
// (column-major over the slice), so the k-th (value, column) of a lane's R rows is one R-wide
// vector load and a wave-instruction reads 512 R bytes contiguous.  Every row keeps its stored
// (ascending-column) order and accumulates from 0.0, mul then add (-ffp-contract=off): y is
// bitwise BCRSMatrix::mv.  Padding entries carry column -1 and are skipped.
//
// Work split: a workgroup of 4 waves walks a CONTIGUOUS chunk of slices (waves interleaved), so
// rows that share x lines stay in one CU / one XCD's L2; 2048 workgroups (8 per CU) are resident.
//
// Here: the slice kernels (k_spmv_b1 / _blk, k_lanczos_spmv_b1 / _blk, k_lanczos_fused_b1 / _blk), the
// pipelined step's row half (k_lanczos_pipe), k_fused_tail, and the launchers launch_spmv,
// launch_lanczos_spmv and launch_lanczos_fused.  On a banded 1x1 image each of those first offers the
// launch to the plane-march kernels (k_march.hip: launch_spmv_march, ...) and runs its slice kernel
// when they decline.  Device code both files use is in spmv_dev.h; the image modes the launchers
// dispatch on are host-only code in march_plan.h / march_plan.cpp.
#include "internal.h"
#include "march_plan.h"
#include "spmv_dev.h"

#include <type_traits>

namespace eigmi {

template <int R>
struct Vec;
template <>
struct Vec<1> {
  typedef double d;
  typedef i32 i;
};
template <>
struct Vec<2> {
  typedef double d __attribute__((ext_vector_type(2)));
  typedef i32 i __attribute__((ext_vector_type(2)));
};
template <>
struct Vec<4> {
  typedef double d __attribute__((ext_vector_type(4)));
  typedef i32 i __attribute__((ext_vector_type(4)));
};

template <int R>
__device__ __forceinline__ double lane_get(const typename Vec<R>::d &v, int q)
{
  if constexpr (R == 1) return v;
  else return v[q];
}
template <int R>
__device__ __forceinline__ i32 lane_geti(const typename Vec<R>::i &v, int q)
{
  if constexpr (R == 1) return v;
  else return v[q];
}

__device__ __forceinline__ void chunk_of(i64 count, i64 &b, i64 &e)
{
  const i64 G = gridDim.x;
  const i64 per = (count + G - 1) / G;
  b = (i64)blockIdx.x * per;
  e = b + per;
  if (e > count) e = count;
}

// Slice order of the row kernels: an XCD-aware sweep.  Workgroups are dealt round-robin over the 8
// XCDs, so XCD x takes the x-th eighth of the launch's slices and its workgroups sweep it together
// (grid-stride inside the eighth): the rows in flight on one XCD stay within a window of (its
// workgroups x 4) slices, and the gathered x rows of a banded (e.g. RCM-ordered) matrix are that
// window +- the bandwidth, which the XCD's L2 can hold.  Measured against contiguous per-workgroup
// chunks (256^3, tools/gpu_csr2.sh): scrambled + RCM SpMV 313 -> 305 us, K1 371 -> 359 us, fused
// step 671 -> 634 us; 7-point SELL image SpMV 268 -> 261 us.  Wave w of a workgroup takes slices
// it0, it0 + step, ... < end.  (Fewer than 8 workgroups: contiguous chunks.)
__device__ __forceinline__ void slice_sweep(i64 count, int wave, i64 &it0, i64 &end, i64 &step)
{
  const int G = gridDim.x;
  if (G < 8)
  {
    i64 b, e;
    chunk_of(count, b, e);
    it0 = b + wave;
    end = e;
    step = kWaves;
    return;
  }
  const int x = blockIdx.x & 7, i = blockIdx.x >> 3;
  const int Gx = (G - x + 7) >> 3;  // workgroups on XCD x
  it0 = count * x / 8 + (i64)i * kWaves + wave;
  end = count * (x + 1) / 8;
  step = (i64)Gx * kWaves;
}

// acc[q] = sum_k a[k][q] * x[c[k][q]] for the R rows of this lane, k ascending.  KC entries are
// prefetched per round (8 (value, column) loads in flight per lane for every R).
template <int R, class X>
__device__ __forceinline__ void rows_dot(const double *__restrict__ val, const i32 *__restrict__ col, const X &x,
                                         i64 base, int width, int lane, double (&acc)[R])
{
  constexpr int C = 64 * R;
  constexpr int KC = 8 / R;
  typedef typename Vec<R>::d dv;
  typedef typename Vec<R>::i iv;
#pragma unroll
  for (int q = 0; q < R; ++q) acc[q] = 0.0;
  // slice base pointers are wave-uniform (scalar); per-lane offsets are 32-bit
  const double *vs = val + base;
  const i32 *cs = col + base;
  for (int k0 = 0; k0 < width; k0 += KC)
  {
    dv a[KC];
    iv c[KC];
#pragma unroll
    for (int k = 0; k < KC; ++k)
    {
      if (k0 + k < width)
      {
        const int idx = (k0 + k) * C + lane * R;
        c[k] = __builtin_nontemporal_load(reinterpret_cast<const iv *>(cs + idx));
        a[k] = __builtin_nontemporal_load(reinterpret_cast<const dv *>(vs + idx));
      }
      else
      {
        c[k] = (iv)(-1);
        a[k] = (dv)(0.0);
      }
    }
    double xv[KC][R];
#pragma unroll
    for (int k = 0; k < KC; ++k)
#pragma unroll
      for (int q = 0; q < R; ++q)
      {
        const i32 cc = lane_geti<R>(c[k], q);
        xv[k][q] = (cc >= 0) ? x(cc) : 0.0;
      }
#pragma unroll
    for (int k = 0; k < KC; ++k)
#pragma unroll
      for (int q = 0; q < R; ++q)
        if (lane_geti<R>(c[k], q) >= 0) acc[q] += lane_get<R>(a[k], q) * xv[k][q];
  }
}

// Stencil slice: entry k of row r is stored iff bit k of mask[r]; its column is r + own + delta_k
// (window-local).  Offsets ascend, so each row still accumulates in ascending-column order.
template <int R, class X>
__device__ __forceinline__ void rows_dot_stencil(const double *__restrict__ val, const i32 *__restrict__ delta,
                                                 const uint8_t *__restrict__ mask, const X &x,
                                                 i64 base, int width, int lane, i64 xrow0, i64 xlast,
                                                 double (&acc)[R])
{
  constexpr int C = 64 * R;
  constexpr int KC = 8 / R;
  typedef typename Vec<R>::d dv;
#pragma unroll
  for (int q = 0; q < R; ++q) acc[q] = 0.0;
  const double *vs = val + base;
  unsigned m[R];
#pragma unroll
  for (int q = 0; q < R; ++q) m[q] = mask[lane * R + q];
  for (int k0 = 0; k0 < width; k0 += KC)
  {
    dv a[KC];
    int dk[KC];
#pragma unroll
    for (int k = 0; k < KC; ++k)
    {
      dk[k] = (k0 + k < width) ? delta[k0 + k] : 0;  // wave-uniform (scalar) loads
      a[k] = (k0 + k < width) ? __builtin_nontemporal_load(reinterpret_cast<const dv *>(vs + (k0 + k) * C + lane * R))
                              : (dv)(0.0);
    }
    // gather addresses do not depend on the mask (clamped into the window instead), so the x loads
    // issue together with the value loads; the mask only gates the accumulation below.
    double xv[KC][R];
#pragma unroll
    for (int k = 0; k < KC; ++k)
#pragma unroll
      for (int q = 0; q < R; ++q)
      {
        i64 g = xrow0 + q + dk[k];
        g = g < 0 ? 0 : (g > xlast ? xlast : g);
        xv[k][q] = x(g);
      }
#pragma unroll
    for (int k = 0; k < KC; ++k)
#pragma unroll
      for (int q = 0; q < R; ++q)
        if ((m[q] >> (k0 + k)) & 1u) acc[q] += lane_get<R>(a[k], q) * xv[k][q];
  }
}

// Row r (window index w = own + r) of the symmetric band image, one row per lane; a row sums
// exactly its stored entries in ascending-column order (bitwise BCRSMatrix::mv when the matrix is
// bitwise symmetric, which mat_image.cpp build_sym_image checks).  `centre` returns the row's own operand x[w] (the
// fused step takes its (t, u) from it).
// NEAR: the offsets -1 / 0 / +1 share one centre load -- the neighbours' operands and the
// mirrored -1 value come from the adjacent lanes by DPP lane shifts (lanes 0 / 63 load theirs):
// 3 gathers + 1 value load fewer per row, i.e. ~30 % fewer L1 requests for a 7-point stencil.
template <class MT, int KC, bool NEAR, class X>
__device__ __forceinline__ void row_sym(const SymImg &S, i64 r, i64 w, int lane, const X &x, i64 xl, double &acc,
                                        typename X::raw &centre)
{
  acc = 0.0;
  const unsigned m = static_cast<const MT *>(S.mask)[r];
  const i64 wc = w > xl ? xl : w;
  if constexpr (!NEAR)
  {
    sym_span<KC>(S, 0, S.nd, m, w, w, x, xl, acc);
    centre = x.load(wc);
  }
  else
  {
    // near loads first: they fly while the far-negative span waits for its own
    const double a0 = S.j0 >= 0 ? S.val[(i64)S.j0 * S.ld + w] : 0.0;
    const double ap = S.val[(i64)S.j1 * S.ld + w];
    const typename X::raw pc = x.load(wc);
    typename X::raw el, er;
    double ae = 0.0;
    const i64 wl = w - 1 < 0 ? 0 : (w - 1 > xl ? xl : w - 1), wr = w + 1 > xl ? xl : w + 1;
    if (lane == 0)
    {
      el = x.load(wl);
      ae = S.val[(i64)S.j1 * S.ld + wl];
    }
    if (lane == 63) er = x.load(wr);
    sym_span<KC>(S, 0, S.klo, m, w, w, x, xl, acc);
    typename X::raw pl = lane_shift<false>(pc), pr = lane_shift<true>(pc);
    double am = lane_shift<false>(ap);
    if (lane == 0)
    {
      pl = el;
      am = ae;
    }
    if (lane == 63) pr = er;
    if (S.km1 >= 0 && ((m >> S.km1) & 1u)) acc += am * x.val(pl);
    if (S.k0 >= 0 && ((m >> S.k0) & 1u)) acc += a0 * x.val(pc);
    if (S.kp1 >= 0 && ((m >> S.kp1) & 1u)) acc += ap * x.val(pr);
    sym_span<KC>(S, S.khi, S.nd, m, w, w, x, xl, acc);
    centre = pc;
  }
}

// (image modes kExplicit .. kSymN32: march_plan.h)
template <int MODE>
constexpr bool is_sym()
{
  return MODE >= kSym8;
}
template <int MODE>
using sym_mask_t = typename std::conditional<MODE == kSym8 || MODE == kSymN8, uint8_t, uint32_t>::type;
template <int MODE>
constexpr bool sym_near()
{
  return MODE == kSymN8 || MODE == kSymN32;
}

// Row sums of slice s for this lane's R rows.
template <int R, int MODE, class X>
__device__ __forceinline__ void slice_dot(const SellB1 &A, i64 s, const X &x, i64 own, int lane, double (&acc)[R])
{
  constexpr int C = 64 * R;
  if constexpr (is_sym<MODE>())
  {
    if constexpr (R == 1)  // (the launchers pick these modes only for R = 1 images)
    {
      const i64 r = s * 64 + lane;
      typename X::raw centre;
      row_sym<sym_mask_t<MODE>, 4, sym_near<MODE>()>(A.sym, r, own + r, lane, x, A.xlast, acc[0], centre);
    }
    return;
  }
  else
  {
  const i64 base = A.slice_ptr[s];
  const int width = (int)((A.slice_ptr[s + 1] - base) / C);
  const bool st = (MODE == kStencil) || (MODE == kMixed && A.st_width[s] > 0);
  if (MODE != kExplicit && st)
    rows_dot_stencil<R, X>(A.val, A.st_delta + 8 * s, A.st_mask + s * C, x, base, width, lane,
                        own + s * C + (i64)lane * R, A.xlast, acc);
  else
    rows_dot<R, X>(A.val, A.col, x, base, width, lane, acc);
  }
}

// Explicit-column slices, software-pipelined (CPF; eig_mat_tune EIG_TUNE_SELL_CPF): the NEXT slice's
// first 8 column indices are loaded while this slice's gathers are in flight, so a slice issues its
// value loads and its gathers together -- one memory round trip per slice instead of two (column
// index, then the gather it addresses).  Products and their order are rows_dot's (bitwise).
__device__ __forceinline__ void sell_cols8(const SellB1 &A, i64 s, int lane, i32 (&c)[8])
{
  const i64 base = A.slice_ptr[s];
  const int width = (int)((A.slice_ptr[s + 1] - base) >> 6);
  const i32 *cs = A.col + base;
#pragma unroll
  for (int k = 0; k < 8; ++k) c[k] = k < width ? __builtin_nontemporal_load(cs + k * 64 + lane) : -1;
}

// the explicit-column slices' cross-slice column prefetch (eig_mat_tune EIG_TUNE_SELL_CPF: 1 on; 0 and
// 2 (automatic) off -- a measurement switch.  Scrambled + RCM Poisson 256^3, same-box A/B
// (profiles/r05zf_csr.jsonl): fused step 402-403 -> 436-437 us, eig_mv 308 -> 315 us: the extra
// registers cost a wave per SIMD, and those waves hid the column round trip already)
static bool sell_cpf(const eig_mat_s &A, bool fused)
{
  (void)fused;
  return A.tune_sell_cpf == 1;
}

// One explicit slice with its first 8 column indices already in registers (cc): the value loads
// and the gathers issue together, then the next slice's columns (sn >= 0) into cn, then the
// products in rows_dot's order (and its later rounds for rows wider than 8 entries).
template <class X>
__device__ __forceinline__ double sell_row_cpf(const SellB1 &A, i64 s, const X &x, int lane, const i32 (&cc)[8],
                                               i64 sn, i32 (&cn)[8])
{
  const i64 base = A.slice_ptr[s];
  const int width = (int)((A.slice_ptr[s + 1] - base) >> 6);
  const double *vs = A.val + base;
  double a[8], xv[8];
#pragma unroll
  for (int k = 0; k < 8; ++k)
  {
    a[k] = k < width ? __builtin_nontemporal_load(vs + k * 64 + lane) : 0.0;
    xv[k] = cc[k] >= 0 ? x(cc[k]) : 0.0;
  }
  if (sn >= 0) sell_cols8(A, sn, lane, cn);
  double acc = 0.0;
#pragma unroll
  for (int k = 0; k < 8; ++k)
    if (cc[k] >= 0) acc += a[k] * xv[k];
  for (int k0 = 8; k0 < width; k0 += 8)
  {
    i32 c2[8];
    double a2[8], x2[8];
#pragma unroll
    for (int k = 0; k < 8; ++k)
    {
      const bool in = k0 + k < width;
      c2[k] = in ? __builtin_nontemporal_load(A.col + base + (k0 + k) * 64 + lane) : -1;
      a2[k] = in ? __builtin_nontemporal_load(vs + (k0 + k) * 64 + lane) : 0.0;
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) x2[k] = c2[k] >= 0 ? x(c2[k]) : 0.0;
#pragma unroll
    for (int k = 0; k < 8; ++k)
      if (c2[k] >= 0) acc += a2[k] * x2[k];
  }
  return acc;
}

// 8 waves per SIMD (8 workgroups per CU) except the mixed image, which carries both row paths.
template <int MODE>
constexpr int min_waves()
{
  return MODE == kMixed ? 1 : 8;
}

// y[own + r] = (A x)[r], 1x1 blocks (x: window base).
template <int R, int MODE, bool CPF = false>
__global__ __launch_bounds__(kStreamThreads, CPF ? 6 : min_waves<MODE>()) void k_spmv_b1(i64 nrows, i64 own, SellB1 A,
                                                               const i32 *__restrict__ slices, i64 first, i64 count,
                                                               const double *__restrict__ x, double *__restrict__ y)
{
  constexpr int C = 64 * R;
  // wave index through readfirstlane: the slice loop, slice_ptr loads and row bases stay scalar
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  i64 it0, end, step;
  slice_sweep(count, wave, it0, end, step);
  if constexpr (CPF && R == 1 && (MODE == kExplicit || MODE == kMixed))
  {
    // explicit slices software-pipelined (sell_row_cpf): the next slice's columns fly with this
    // slice's gathers; stencil slices of a mixed image as slice_dot
    auto sid = [&](i64 it) { return slices ? (i64)slices[first + it] : first + it; };
    auto expl = [&](i64 s) { return MODE == kExplicit || A.st_width[s] <= 0; };  // (explicit: width -1)
    i32 cn[8];
    if (it0 < end && expl(sid(it0))) sell_cols8(A, sid(it0), lane, cn);
    for (i64 it = it0; it < end; it += step)
    {
      const i64 s = sid(it);
      const i64 sn = it + step < end && expl(sid(it + step)) ? sid(it + step) : -1;
      double acc;
      if (expl(s))
      {
        i32 cc[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) cc[k] = cn[k];
        acc = sell_row_cpf(A, s, XPlain{x}, lane, cc, sn, cn);
      }
      else
      {
        if (sn >= 0) sell_cols8(A, sn, lane, cn);
        double a1[1];
        slice_dot<1, MODE>(A, s, XPlain{x}, own, lane, a1);
        acc = a1[0];
      }
      const i64 r0 = s * C + lane;
      if (r0 < nrows) y[own + r0] = acc;
    }
    return;
  }
  for (i64 it = it0; it < end; it += step)
  {
    const i64 s = slices ? (i64)slices[first + it] : first + it;
    double acc[R];
    slice_dot<R, MODE>(A, s, XPlain{x}, own, lane, acc);
    const i64 r0 = s * C + (i64)lane * R;
#pragma unroll
    for (int q = 0; q < R; ++q)
      if (r0 + q < nrows) y[own + r0 + q] = acc[q];
  }
}

// General br x bc blocks (C = 64): lane = block row, per block br*bc values column-major over lanes.
template <int BR, int BC>
__global__ __launch_bounds__(kStreamThreads) void k_spmv_blk(i64 nbrows, const i64 *__restrict__ slice_ptr,
                                                             const i32 *__restrict__ slices, i64 first, i64 count,
                                                             const double *__restrict__ val,
                                                             const i32 *__restrict__ col,
                                                             const double *__restrict__ x, double *__restrict__ y)
{
  constexpr int BB = BR * BC;
  // wave index through readfirstlane: the slice loop, slice_ptr loads and row bases stay scalar
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  i64 b, e;
  chunk_of(count, b, e);
  for (i64 it = b + wave; it < e; it += kWaves)
  {
    const i64 s = slices ? (i64)slices[first + it] : first + it;
    const i64 base = slice_ptr[s];
    const int width = (int)((slice_ptr[s + 1] - base) >> 6);
    double acc[BR];
#pragma unroll
    for (int r = 0; r < BR; ++r) acc[r] = 0.0;
    for (int k = 0; k < width; ++k)
    {
      const i64 ci = base + (i64)k * 64 + lane;
      const i32 c = __builtin_nontemporal_load(col + ci);
      if (c < 0) continue;
      const double *vb = val + (base + (i64)k * 64) * BB + lane;
      double a[BB], xv[BC];
#pragma unroll
      for (int t = 0; t < BB; ++t) a[t] = __builtin_nontemporal_load(vb + t * 64);
#pragma unroll
      for (int cc = 0; cc < BC; ++cc) xv[cc] = x[(i64)c * BC + cc];
#pragma unroll
      for (int r = 0; r < BR; ++r)
      {
        double sacc = acc[r];
#pragma unroll
        for (int cc = 0; cc < BC; ++cc) sacc += a[r * BC + cc] * xv[cc];
        acc[r] = sacc;
      }
    }
    const i64 row = s * 64 + lane;
    if (row < nbrows)
    {
#pragma unroll
      for (int r = 0; r < BR; ++r) y[row * BR + r] = acc[r];
    }
  }
}

// ---------------------------------------------------------------------------------------------
// Lanczos step, kernel 1 (DESIGN.md "Lanczos step"):
//   t = (A u_j) * sig_j - gam_j * u_{j-1},  dsum[j] = t . u_j  (grid reduction)
// with beta_j = sqrt(nsum[j]), sig_j = 1/beta_j, gam_j = beta_j / sqrt(nsum[j-1]).
// u, up, t are WINDOW buffers; owned rows at `own`.  `carry` (nullable) is a partial dot from a
// previous launch of the same step (interior slices), added first by the last workgroup.
// ---------------------------------------------------------------------------------------------
template <int R, int MODE>
__global__ __launch_bounds__(kStreamThreads, min_waves<MODE>()) void k_lanczos_spmv_b1(
    i64 nrows, i64 own, SellB1 A, const i32 *__restrict__ slices, i64 first, i64 count,
    const double *__restrict__ u, const double *__restrict__ up, double *__restrict__ t, int j,
    const double *__restrict__ nsum,
    double *__restrict__ dot_out, double *__restrict__ beta_out, const double *__restrict__ carry,
    double *partials, unsigned *ticket)
{
  constexpr int C = 64 * R;
  __shared__ double tot[1];
  // wave index through readfirstlane: the slice loop, slice_ptr loads and row bases stay scalar
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const double beta = sqrt(nsum[j]);
  const double sig = 1.0 / beta;
  const double gam = (j > 0) ? beta * (1.0 / sqrt(nsum[j - 1])) : 0.0;
  i64 it0, end, step;
  slice_sweep(count, wave, it0, end, step);
  double d = 0.0;
  for (i64 it = it0; it < end; it += step)
  {
    const i64 s = slices ? (i64)slices[first + it] : first + it;
    const i64 r0 = s * C + (i64)lane * R;
    // epilogue operands issued before the row loop so their latency hides under the matrix stream
    double upv[R], uv[R];
#pragma unroll
    for (int q = 0; q < R; ++q)
    {
      const bool ok = r0 + q < nrows;
      upv[q] = (ok && j > 0) ? up[own + r0 + q] : 0.0;
      uv[q] = ok ? u[own + r0 + q] : 0.0;
    }
    double acc[R];
    slice_dot<R, MODE>(A, s, XPlain{u}, own, lane, acc);
#pragma unroll
    for (int q = 0; q < R; ++q)
    {
      const i64 r = r0 + q;
      if (r < nrows)
      {
        double ti = acc[q] * sig;
        if (j > 0) ti = ti - gam * upv[q];
        t[own + r] = ti;
        d += ti * uv[q];
      }
    }
  }
  double v[1] = {d};
  if (grid_sum<1, kStreamThreads>(v, partials, ticket, tot))
  {
    if (threadIdx.x == 0)
    {
      dot_out[0] = carry ? (carry[0] + tot[0]) : tot[0];
      if (beta_out) beta_out[0] = beta;
    }
  }
}

// ---------------------------------------------------------------------------------------------
// The Lanczos step on square b x b blocks (blocked SELL-64 image, one rank: window = owned rows).
// blk_rows_dot is k_spmv_blk's row loop: lane = block row, acc[r] of scalar row lane b + r starts
// from 0.0 and takes the stored blocks in stored order, c = 0..b-1 inside a block, mul then add --
// bitwise BCRSMatrix::mv on x (XPlain) or on u_k formed in the gather (XPair: the b pairs of a block
// column are 16 b contiguous bytes, b 16-B loads).
// ---------------------------------------------------------------------------------------------
template <int B, class X>
__device__ __forceinline__ void blk_rows_dot(const i64 *__restrict__ slice_ptr, const double *__restrict__ val,
                                             const i32 *__restrict__ col, i64 s, int lane, const X &x,
                                             double (&acc)[B])
{
  constexpr int BB = B * B;
  const i64 base = slice_ptr[s];
  const int width = (int)((slice_ptr[s + 1] - base) >> 6);
#pragma unroll
  for (int r = 0; r < B; ++r) acc[r] = 0.0;
  for (int k = 0; k < width; ++k)
  {
    const i32 c = __builtin_nontemporal_load(col + base + (i64)k * 64 + lane);
    if (c < 0) continue;
    const double *vb = val + (base + (i64)k * 64) * BB + lane;
    double a[BB];
    typename X::raw xr[B];
#pragma unroll
    for (int t = 0; t < BB; ++t) a[t] = __builtin_nontemporal_load(vb + t * 64);
#pragma unroll
    for (int cc = 0; cc < B; ++cc) xr[cc] = x.load((i64)c * B + cc);
    double xv[B];
#pragma unroll
    for (int cc = 0; cc < B; ++cc) xv[cc] = x.val(xr[cc]);
#pragma unroll
    for (int r = 0; r < B; ++r)
    {
      double sacc = acc[r];
#pragma unroll
      for (int cc = 0; cc < B; ++cc) sacc += a[r * B + cc] * xv[cc];
      acc[r] = sacc;
    }
  }
}

// Waves / SIMD the blocked step kernels are built for: no scratch in any instantiation (the
// resource-usage report).
template <int B>
constexpr int lanczos_blk_waves(bool fused)
{
  return B == 2 ? 8 : B == 3 ? (fused ? 6 : 8) : (fused ? 4 : 5);
}

// Kernel 1 on blocks: k_lanczos_spmv_b1's epilogue per scalar row.  Kernel 2 is k_lanczos_update on
// the nbrows * b scalar rows.
template <int B>
__global__ __launch_bounds__(kStreamThreads, lanczos_blk_waves<B>(false)) void k_lanczos_spmv_blk(
    i64 nbrows, const i64 *__restrict__ slice_ptr, const i32 *__restrict__ slices, i64 first, i64 count,
    const double *__restrict__ val, const i32 *__restrict__ col, const double *__restrict__ u,
    const double *__restrict__ up, double *__restrict__ t, int j, const double *__restrict__ nsum,
    double *__restrict__ dot_out, double *__restrict__ beta_out, const double *__restrict__ carry, double *partials,
    unsigned *ticket)
{
  __shared__ double tot[1];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const double beta = sqrt(nsum[j]);
  const double sig = 1.0 / beta;
  const double gam = (j > 0) ? beta * (1.0 / sqrt(nsum[j - 1])) : 0.0;
  i64 b, e;
  chunk_of(count, b, e);
  double d = 0.0;
  for (i64 it = b + wave; it < e; it += kWaves)
  {
    const i64 s = slices ? (i64)slices[first + it] : first + it;
    const i64 row = s * 64 + lane;
    const bool ok = row < nbrows;
    // epilogue operands issued before the row loop so their latency hides under the matrix stream
    double upv[B], uv[B];
#pragma unroll
    for (int r = 0; r < B; ++r)
    {
      upv[r] = (ok && j > 0) ? up[row * B + r] : 0.0;
      uv[r] = ok ? u[row * B + r] : 0.0;
    }
    double acc[B];
    blk_rows_dot<B>(slice_ptr, val, col, s, lane, XPlain{u}, acc);
    if (ok)
    {
#pragma unroll
      for (int r = 0; r < B; ++r)
      {
        double ti = acc[r] * sig;
        if (j > 0) ti = ti - gam * upv[r];
        t[row * B + r] = ti;
        d += ti * uv[r];
      }
    }
  }
  double v[1] = {d};
  if (grid_sum<1, kStreamThreads>(v, partials, ticket, tot))
  {
    if (threadIdx.x == 0)
    {
      dot_out[0] = carry ? (carry[0] + tot[0]) : tot[0];
      if (beta_out) beta_out[0] = beta;
    }
  }
}

// Fused step, one stencil slice, one row per lane: gathers the (t, u) pairs at the slice's offsets
// (16-B loads, clamped addresses as rows_dot_stencil), accumulates sum a (t - c u) in offset order
// and takes the row's own (t, u) from the delta = 0 gather instead of a separate load.  KC entries
// in flight per round.  Same arithmetic and order as the generic path (bitwise equal).
template <int KC>
__device__ __forceinline__ void fused_row_stencil(const SellB1 &A, i64 s, const dpair *__restrict__ P, double c,
                                                  i64 own, int lane, double &acc, double &tv, double &uv)
{
  const i64 base = A.slice_ptr[s];
  const int width = (int)((A.slice_ptr[s + 1] - base) >> 6);
  const i32 *dl = A.st_delta + 8 * s;
  const unsigned m = A.st_mask[s * 64 + lane];
  const double *vs = A.val + base;
  const i64 xrow0 = own + s * 64 + lane;
  const i64 xl = A.xlast;
  acc = 0.0;
  bool centre = false;  // wave-uniform: the offset list holds delta = 0
  for (int k0 = 0; k0 < width; k0 += KC)
  {
    double a[KC];
    dpair pr[KC];
    int dk[KC];
#pragma unroll
    for (int k = 0; k < KC; ++k)
    {
      const bool in = k0 + k < width;
      dk[k] = in ? dl[k0 + k] : 0;
      a[k] = in ? __builtin_nontemporal_load(vs + (k0 + k) * 64 + lane) : 0.0;
    }
#pragma unroll
    for (int k = 0; k < KC; ++k)
    {
      i64 g = xrow0 + dk[k];
      g = g < 0 ? 0 : (g > xl ? xl : g);
      pr[k] = (k0 + k < width) ? P[g] : dpair{0.0, 0.0};
    }
#pragma unroll
    for (int k = 0; k < KC; ++k)
    {
      if (k0 + k < width && dk[k] == 0)
      {
        tv = pr[k].x;
        uv = pr[k].y;
        centre = true;
      }
      if ((m >> (k0 + k)) & 1u) acc += a[k] * (pr[k].x - c * pr[k].y);
    }
  }
  if (!centre)
  {
    const i64 g = xrow0 > xl ? xl : xrow0;
    const dpair pv = P[g];
    tv = pv.x;
    uv = pv.y;
  }
}

// Register budget for 8 waves / SIMD (W): stencil rows take 4 entries per round to fit 64 VGPRs
// (measured: 5 waves with 8 entries per round and 6 waves were no faster).
// (explicit-column and mixed images: 6 waves / SIMD; at 8 their row loops spill 36 / 46 VGPRs to
// scratch, whose write-back is the write traffic PMC showed beyond the pair stores.  Stencil
// images: 7 (at 8: 20 B of scratch per lane; 3-D Poisson 256^3 on the SELL stencil image 353.2 ->
// 333.3 us, tools/stencil_fused.py)
template <int MODE>
constexpr int fused_b1_waves()
{
  return (MODE == kExplicit || MODE == kMixed) ? 6 : MODE == kStencil ? 7 : 8;
}

template <int R, int MODE, bool CPF = false>
__global__ __launch_bounds__(kStreamThreads, CPF ? 5 : fused_b1_waves<MODE>()) void k_lanczos_fused_b1(
    i64 nrows, i64 own, SellB1 A, const i32 *__restrict__ slices, i64 first, i64 count,
    const dpair *__restrict__ P, dpair *__restrict__ Pout, FusedArgs fa, double *__restrict__ out,
    const double *__restrict__ carry, double *partials, unsigned *ticket)
{
  constexpr int C = 64 * R;
  constexpr int W = 8;
  __shared__ double tot[3];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const FusedStep fs = fused_begin(fa);
  if (fs.act == kFusedHalt || fs.act == kFusedNoop)
  {
    double z[3] = {0.0, 0.0, 0.0};
    if (fa.xch & kXchPublish) fused_finish<2>(z, partials, ticket, tot, out, nullptr, fa);
    else fused_idle(out);
    return;
  }
  const double c = fs.c, gam = fs.gam, sig = fs.sig, mu = fs.mu;
  const int k = fs.j;
  i64 it0, end, step;
  slice_sweep(count, wave, it0, end, step);
  if (fs.act == kFusedRepair)
  {
    // this launch's rows: its slices
    double m2 = 0.0;
    for (i64 it = it0; it < end; it += step)
    {
      const i64 s = slices ? (i64)slices[first + it] : first + it;
#pragma unroll
      for (int q = 0; q < R; ++q)
      {
        const i64 r = s * C + (i64)lane * R + q;
        if (r < nrows)
        {
          const dpair p = P[own + r];
          const double u = p.x - c * p.y;
          Pout[own + r] = dpair{u, p.y};
          m2 += u * u;
        }
      }
    }
    double v[3] = {0.0, 0.0, m2};
    fused_finish<2>(v, partials, ticket, tot, out, carry, fa);
    return;
  }
  const XPair xc{P, c};
  double d = 0.0, q2 = 0.0, m2 = 0.0;
  auto sid = [&](i64 it) { return slices ? (i64)slices[first + it] : first + it; };
  auto expl = [&](i64 s) { return MODE == kExplicit || A.st_width[s] <= 0; };  // (explicit: width -1)
  constexpr bool kCpf = CPF && R == 1 && (MODE == kExplicit || MODE == kMixed);
  i32 cn[8];
  if constexpr (kCpf)
  {
    if (it0 < end && expl(sid(it0))) sell_cols8(A, sid(it0), lane, cn);
  }
  for (i64 it = it0; it < end; it += step)
  {
    const i64 s = sid(it);
    const i64 r0 = s * C + (i64)lane * R;
    double tv[R], uv[R], acc[R];
    if constexpr (kCpf)
    {
      const bool more = it + step < end;
      if (expl(s))
      {
        i32 cc[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) cc[k] = cn[k];
        const dpair pv = r0 < nrows ? P[own + r0] : dpair{0.0, 0.0};
        const i64 sn = more && expl(sid(it + step)) ? sid(it + step) : -1;
        acc[0] = sell_row_cpf(A, s, xc, lane, cc, sn, cn);
        tv[0] = pv.x;
        uv[0] = pv.y;
      }
      else
      {
        if (more && expl(sid(it + step))) sell_cols8(A, sid(it + step), lane, cn);
        fused_row_stencil<(W >= 8 ? 4 : 8)>(A, s, P, c, own, lane, acc[0], tv[0], uv[0]);
      }
    }
    else if constexpr (is_sym<MODE>())
    {
      if constexpr (R == 1)
      {
        dpair pc;
        // far spans: 4 entries per round (2 on the lane-shift path, whose near operands stay live
        // across the far-negative span) at 8 waves / SIMD, 8 at 5
        constexpr int KC = W >= 8 ? (sym_near<MODE>() ? 2 : 4) : 8;
        row_sym<sym_mask_t<MODE>, KC, sym_near<MODE>()>(A.sym, r0, own + r0, lane, xc, A.xlast, acc[0], pc);
        tv[0] = pc.x;
        uv[0] = pc.y;
      }
    }
    else if (R == 1 && MODE != kExplicit && (MODE == kStencil || A.st_width[s] > 0))
    {
      fused_row_stencil<(W >= 8 ? 4 : 8)>(A, s, P, c, own, lane, acc[0], tv[0], uv[0]);
    }
    else
    {
#pragma unroll
      for (int q = 0; q < R; ++q)
      {
        const bool ok = r0 + q < nrows;
        const dpair pv = ok ? P[own + r0 + q] : dpair{0.0, 0.0};
        tv[q] = pv.x;
        uv[q] = pv.y;
      }
      slice_dot<R, MODE>(A, s, xc, own, lane, acc);
    }
#pragma unroll
    for (int q = 0; q < R; ++q)
    {
      const i64 r = r0 + q;
      if (r < nrows)
      {
        const double uk = tv[q] - c * uv[q];
        double ti = (acc[q] - mu * uk) * sig;
        if (k > 0) ti = ti - gam * uv[q];
        Pout[own + r] = dpair{ti, uk};
        d += ti * uk;
        q2 += ti * ti;
        m2 += uk * uk;
      }
    }
  }
  double v[3] = {d, q2, m2};
  fused_finish<2>(v, partials, ticket, tot, out, carry, fa);
}

// The guarded fused step on square b x b blocks: k_lanczos_fused_b1's control words, branches and
// per-row epilogue over the nbrows * b scalar rows (one rank: pairs indexed by the scalar row), the
// row products by blk_rows_dot on the pairs.
template <int B>
__global__ __launch_bounds__(kStreamThreads, lanczos_blk_waves<B>(true)) void k_lanczos_fused_blk(
    i64 nbrows, const i64 *__restrict__ slice_ptr, const i32 *__restrict__ slices, i64 first, i64 count,
    const double *__restrict__ val, const i32 *__restrict__ col, const dpair *__restrict__ P,
    dpair *__restrict__ Pout, FusedArgs fa, double *__restrict__ out, const double *__restrict__ carry,
    double *partials, unsigned *ticket)
{
  __shared__ double tot[3];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const FusedStep fs = fused_begin(fa);
  if (fs.act == kFusedHalt || fs.act == kFusedNoop)
  {
    double z[3] = {0.0, 0.0, 0.0};
    if (fa.xch & kXchPublish) fused_finish<2>(z, partials, ticket, tot, out, nullptr, fa);
    else fused_idle(out);
    return;
  }
  const double c = fs.c, gam = fs.gam, sig = fs.sig, mu = fs.mu;
  const int k = fs.j;
  if (fs.act == kFusedRepair)
  {
    double v[3] = {0.0, 0.0, fused_repair_rows(0, nbrows * B, 0, c, P, Pout)};
    fused_finish<2>(v, partials, ticket, tot, out, carry, fa);
    return;
  }
  const XPair xc{P, c};
  double d = 0.0, q2 = 0.0, m2 = 0.0;
  i64 b, e;
  chunk_of(count, b, e);
  for (i64 it = b + wave; it < e; it += kWaves)
  {
    const i64 s = slices ? (i64)slices[first + it] : first + it;
    const i64 row = s * 64 + lane;
    const bool ok = row < nbrows;
    // the rows' own pairs issued before the row loop so their latency hides under the matrix stream
    dpair pv[B];
#pragma unroll
    for (int r = 0; r < B; ++r) pv[r] = ok ? P[row * B + r] : dpair{0.0, 0.0};
    double acc[B];
    blk_rows_dot<B>(slice_ptr, val, col, s, lane, xc, acc);
    if (ok)
    {
#pragma unroll
      for (int r = 0; r < B; ++r)
      {
        const double uk = pv[r].x - c * pv[r].y;
        double ti = (acc[r] - mu * uk) * sig;
        if (k > 0) ti = ti - gam * pv[r].y;
        Pout[row * B + r] = dpair{ti, uk};
        d += ti * uk;
        q2 += ti * ti;
        m2 += uk * uk;
      }
    }
  }
  double v[3] = {d, q2, m2};
  fused_finish<2>(v, partials, ticket, tot, out, carry, fa);
}

// ---------------------------------------------------------------------------------------------
// Pipelined one-reduction step, row half (restatement orc_lanczos_pipelined).  The
// step's SpMV multiplies t_{k-1} (S = A t_{k-1}, a plain eig_mv launch), which needs no scalar of the
// previous launch, so on N GPUs it runs while that launch's 3-value allreduce is in flight.  This
// kernel then applies the scalars (fused_begin: the same modes, prediction and repairs as the fused
// step) row by row:
//   u_k = t_{k-1} - c u_{k-1},  z_k = S - c z_{k-1}  (= A u_k),  t_k = (z_k - mu u_k) sig - gam u_{k-1}
// T (t) is updated in place; UZ holds the (u, z) pairs.  A repair writes T = u_k and keeps UZ (the
// launch after it has c = 0: u = T, z = S = A u_k exactly).  Bytes: 32 B read + 24 B written per row.
// Rows [0, n) are owned rows (pointers already offset to the owned part).
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kStreamThreads) void k_lanczos_pipe(i64 n, double *__restrict__ T,
                                                                 dpair *__restrict__ UZ,
                                                                 const double *__restrict__ S, FusedArgs fa,
                                                                 double *__restrict__ out, double *partials,
                                                                 unsigned *ticket)
{
  __shared__ double tot[3];
  const FusedStep fs = fused_begin(fa);
  if (fs.act == kFusedHalt || fs.act == kFusedNoop)
  {
    fused_idle(out);
    return;
  }
  const double c = fs.c, gam = fs.gam, sig = fs.sig, mu = fs.mu;
  const bool k0 = fs.j > 0;
  const i64 stride = (i64)gridDim.x * kStreamThreads;
  double d = 0.0, q2 = 0.0, m2 = 0.0;
  if (fs.act == kFusedRepair)
  {
    for (i64 i = (i64)blockIdx.x * kStreamThreads + threadIdx.x; i < n; i += stride)
    {
      const double u = T[i] - c * UZ[i].x;
      T[i] = u;
      m2 += u * u;
    }
  }
  else
  {
    auto row = [&](double t, double s, dpair uz, double &tn, dpair &uzn) {
      const double u = t - c * uz.x;
      const double z = s - c * uz.y;
      double ti = (z - mu * u) * sig;
      if (k0) ti = ti - gam * uz.x;
      tn = ti;
      uzn = dpair{u, z};
      d += ti * u;
      q2 += ti * ti;
      m2 += u * u;
    };
    // two rows per lane: 16-B loads of T and S, two 16-B (u, z) pairs (4 items in flight per lane
    // with all loads issued first measured no faster: the launch is HBM-bound at 56 B per row)
    const i64 n2 = n >> 1;
    double2 *T2 = reinterpret_cast<double2 *>(T);
    const double2 *S2 = reinterpret_cast<const double2 *>(S);
    for (i64 i = (i64)blockIdx.x * kStreamThreads + threadIdx.x; i < n2; i += stride)
    {
      const double2 t = T2[i], s = S2[i];
      const dpair a = UZ[2 * i], b = UZ[2 * i + 1];
      double2 tn;
      dpair an, bn;
      row(t.x, s.x, a, tn.x, an);
      row(t.y, s.y, b, tn.y, bn);
      T2[i] = tn;
      UZ[2 * i] = an;
      UZ[2 * i + 1] = bn;
    }
    if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0)
    {
      double tn;
      dpair zn;
      row(T[n - 1], S[n - 1], UZ[n - 1], tn, zn);
      T[n - 1] = tn;
      UZ[n - 1] = zn;
    }
  }
  double v[3] = {d, q2, m2};
  if (grid_sum<3, kStreamThreads>(v, partials, ticket, tot))
  {
    if (threadIdx.x < 3) out[threadIdx.x] = tot[threadIdx.x];
  }
}

// Final beta of a fused run (eig_lanczos_tridiag): after the forced repair launch L-1 (or a repair
// the recurrence took itself), the exact ||u_j||^2 is in fred[3(L-1)+2] and (rn, rm) in aux[2L..]:
// beta[j] = sqrt(mex) rn / rm, nsum[j] = mex -- the values the post-repair step would store.
__global__ void k_fused_tail(double *nsum, double *beta, const double *fred, const int *ctl, const double *aux, int L)
{
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const int j = ctl[2 * L], mode = ctl[2 * L + 1];
  if (mode == kFusedPost)
  {
    const double mex = fred[3 * (L - 1) + 2];
    nsum[j] = mex;
    beta[j] = mex > 0.0 ? sqrt(mex) * aux[2 * L] / aux[2 * L + 1] : 0.0;
  }
  else if (j == 0)
    beta[0] = sqrt(nsum[0]);
}

// Grid = min(work, resident workgroups): every workgroup takes one contiguous chunk, so a grid
// larger than what the CUs hold at once would leave a tail of late chunks.
template <class K>
static int grid_for_slices(K kernel, i64 count, int num_cu)
{
  static thread_local std::pair<const void *, int> cache{nullptr, 0};
  int per_cu = 0;
  if (cache.first == (const void *)kernel) per_cu = cache.second;
  else
  {
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, kStreamThreads, 0) != hipSuccess || per_cu < 1)
      per_cu = 4;
    cache = {(const void *)kernel, per_cu};
  }
  const i64 cap = (i64)per_cu * num_cu;
  const i64 need = (count + kWaves - 1) / kWaves;
  if (need < 1) return 1;
  return (int)(need < cap ? need : cap);
}

// Calls f(std::integral_constant<int, MODE>{}) with the image mode (march_plan.h) as a value: a launcher's
// generic lambda so instantiates its slice kernel once per mode.
template <class F>
static void with_image_mode(int mode, const F &f)
{
  if (mode == kExplicit) f(std::integral_constant<int, kExplicit>{});
  else if (mode == kStencil) f(std::integral_constant<int, kStencil>{});
  else if (mode == kSym8) f(std::integral_constant<int, kSym8>{});
  else if (mode == kSym32) f(std::integral_constant<int, kSym32>{});
  else if (mode == kSymN8) f(std::integral_constant<int, kSymN8>{});
  else if (mode == kSymN32) f(std::integral_constant<int, kSymN32>{});
  else f(std::integral_constant<int, kMixed>{});
}

// The scalars of fused launch fl as a kernel argument (no in-kernel exchange: launch_lanczos_fused adds it)
static FusedArgs fused_args(const FusedLaunch &fl)
{
  return FusedArgs{fl.st.nsum, fl.st.alpha, fl.st.beta, fl.st.fred, fl.st.ctl, fl.st.aux, fl.st.mu2, fl.st.pn, fl.L,
                   fl.force, 0, Mailbox{}};
}

void launch_spmv(const eig_mat_s &A, const double *x, double *y, const i32 *slices, i64 first, i64 count,
                 hipStream_t s, bool keep)
{
  if (count <= 0 && slices != &kMarchInteriorTag) return;
  const int ncu = A.ctx->num_cu;
  double *yo = y + A.own_offset;
  if (A.br == 1 && A.bc == 1)
  {
    const int mode = image_mode(A);
    if (launch_spmv_march(A, mode, x, y, slices, first, count, s, keep)) return;
    with_image_mode(mode, [&](auto mc) {
      constexpr int M = decltype(mc)::value;
      auto launch = [&](auto cpf) {
        constexpr bool CPF = decltype(cpf)::value;
        const int G = grid_for_slices(k_spmv_b1<1, M, CPF>, count, ncu);
        hipLaunchKernelGGL((k_spmv_b1<1, M, CPF>), dim3(G), dim3(kStreamThreads), 0, s, A.nb_rows, A.own_offset,
                           sell_b1(A), slices, first, count, x, y);
      };
      if (sell_cpf(A, false) && (M == kExplicit || M == kMixed)) launch(std::true_type{});
      else launch(std::false_type{});
    });
    return;
  }
#define EIG_BLK(R_, C_)                                                                                 \
  if (A.br == R_ && A.bc == C_)                                                                         \
  {                                                                                                     \
    const int G = grid_for_slices(k_spmv_blk<R_, C_>, count, ncu);                                      \
    hipLaunchKernelGGL((k_spmv_blk<R_, C_>), dim3(G), dim3(kStreamThreads), 0, s, A.nb_rows, A.slice_ptr, \
                       slices, first, count, A.val, A.col, x, yo);                                      \
    return;                                                                                             \
  }
  EIG_BLK(1, 2) EIG_BLK(1, 3) EIG_BLK(1, 4)
  EIG_BLK(2, 1) EIG_BLK(2, 2) EIG_BLK(2, 3) EIG_BLK(2, 4)
  EIG_BLK(3, 1) EIG_BLK(3, 2) EIG_BLK(3, 3) EIG_BLK(3, 4)
  EIG_BLK(4, 1) EIG_BLK(4, 2) EIG_BLK(4, 3) EIG_BLK(4, 4)
#undef EIG_BLK
  throw Error(EIG_ERR_BLOCKSIZE, "eig_mv: block size not supported (br, bc must be in 1..4)");
}

void launch_lanczos_spmv(const eig_mat_s &A, const double *u, const double *up, double *t, int j,
                         const LanczosState &st, const i32 *slices, i64 first, i64 count, double *dot_out,
                         double *beta_out, const double *carry, int ticket, hipStream_t s, ReduceWS red)
{
  EIG_CHECK(lanczos_blocks_ok(A), EIG_ERR_BLOCKSIZE, "Lanczos step: square blocks 1..4 only (blocks: one rank)");
#define EIG_LZB(B_)                                                                                          \
  if (A.br == B_)                                                                                            \
  {                                                                                                          \
    hipLaunchKernelGGL((k_lanczos_spmv_blk<B_>),                                                             \
                       dim3(grid_for_slices(k_lanczos_spmv_blk<B_>, count, A.ctx->num_cu)), dim3(kStreamThreads), \
                       0, s, A.nb_rows, A.slice_ptr, slices, first, count, A.val, A.col, u, up, t, j, st.nsum, \
                       dot_out, beta_out, carry, red.partials, red.ticket(ticket));                          \
    return;                                                                                                  \
  }
  EIG_LZB(2) EIG_LZB(3) EIG_LZB(4)
#undef EIG_LZB
  if (!carry && launch_lanczos_spmv_march(A, image_mode(A), u, up, t, j, st, slices, first, count, dot_out, beta_out,
                                          ticket, s, red))
    return;
  with_image_mode(image_mode(A), [&](auto mode) {
    constexpr int M = decltype(mode)::value;
    hipLaunchKernelGGL((k_lanczos_spmv_b1<1, M>), dim3(grid_for_slices(k_lanczos_spmv_b1<1, M>, count, A.ctx->num_cu)),
                       dim3(kStreamThreads), 0, s, A.nb_rows, A.own_offset, sell_b1(A), slices, first, count, u, up, t, j,
                       st.nsum, dot_out, beta_out, carry, red.partials, red.ticket(ticket));
  });
}

void launch_lanczos_fused(const eig_mat_s &A, const double *P, double *Pout, const FusedLaunch &fl,
                          const i32 *slices, i64 first, i64 count, const double *carry, double *out, int ticket,
                          hipStream_t s, ReduceWS red)
{
  EIG_CHECK(lanczos_blocks_ok(A), EIG_ERR_BLOCKSIZE, "Lanczos step: square blocks 1..4 only (blocks: one rank)");
  FusedArgs fa = fused_args(fl);
  if (fl.xch)
  {
    EIG_CHECK(A.ctx->step_exchange(), EIG_ERR_ARG, "fused step: in-kernel exchange without the mailbox");
    fa.xch = fl.xch & kXchPublish;
    fa.mb = A.ctx->mailbox_dev();
  }
#define EIG_LFB(B_)                                                                                          \
  if (A.br == B_)                                                                                            \
  {                                                                                                          \
    hipLaunchKernelGGL((k_lanczos_fused_blk<B_>),                                                            \
                       dim3(grid_for_slices(k_lanczos_fused_blk<B_>, count, A.ctx->num_cu)),                 \
                       dim3(kStreamThreads), 0, s, A.nb_rows, A.slice_ptr, slices, first, count, A.val, A.col, \
                       reinterpret_cast<const dpair *>(P), reinterpret_cast<dpair *>(Pout), fa, out, carry,   \
                       red.partials, red.ticket(ticket));                                                    \
    return;                                                                                                  \
  }
  EIG_LFB(2) EIG_LFB(3) EIG_LFB(4)
#undef EIG_LFB
  if (!carry && launch_lanczos_fused_march(A, image_mode(A), P, Pout, fa, fl.L, slices, first, count, out, ticket, s, red))
    return;
  with_image_mode(image_mode(A), [&](auto mode) {
    constexpr int M = decltype(mode)::value;
    auto launch = [&](auto cpf) {
      constexpr bool CPF = decltype(cpf)::value;
      hipLaunchKernelGGL((k_lanczos_fused_b1<1, M, CPF>),
                         dim3(grid_for_slices(k_lanczos_fused_b1<1, M, CPF>, count, A.ctx->num_cu)),
                         dim3(kStreamThreads), 0, s, A.nb_rows, A.own_offset, sell_b1(A), slices, first, count,
                         reinterpret_cast<const dpair *>(P), reinterpret_cast<dpair *>(Pout), fa, out, carry,
                         red.partials, red.ticket(ticket));
    };
    if (sell_cpf(A, true) && (M == kExplicit || M == kMixed)) launch(std::true_type{});
    else launch(std::false_type{});
  });
}

void launch_lanczos_pipe(const eig_mat_s &A, double *T, double *UZ, const double *S, const FusedLaunch &fl,
                         double *out, hipStream_t s, ReduceWS red)
{
  EIG_CHECK(A.br == 1 && A.bc == 1, EIG_ERR_BLOCKSIZE, "Lanczos driver: 1x1 blocks only");
  const i64 n = A.nb_rows, own = A.own_offset;
  EIG_CHECK((own & 1) == 0 && (((uintptr_t)T | (uintptr_t)UZ | (uintptr_t)S) & 15) == 0, EIG_ERR_ARG,
            "pipelined Lanczos: vectors must be 16-B aligned");
  const FusedArgs fa = fused_args(fl);
  const i64 per = 2LL * kStreamThreads;
  const int G = (int)std::max<i64>(1, std::min<i64>(kStreamBlocks, (n + per - 1) / per));
  hipLaunchKernelGGL(k_lanczos_pipe, dim3(G), dim3(kStreamThreads), 0, s, n, T + own,
                     reinterpret_cast<dpair *>(UZ) + own, S + own, fa, out, red.partials, red.ticket(0));
}

void launch_fused_tail(const LanczosState &st, int L, hipStream_t s)
{
  hipLaunchKernelGGL(k_fused_tail, dim3(1), dim3(64), 0, s, st.nsum, st.beta, st.fred, st.ctl, st.aux, L);
}

}  // namespace eigmi
