// spmv_dev.h -- device code the SELL slice kernels (k_spmv.hip) and the plane-march kernels
// (k_march.hip) share (gfx950): the gathered-operand functors (XPlain, XPair), the DPP lane shifts, the symmetric band image (SymImg, sym_span), the SELL image as a kernel
// argument (SellB1, sell_b1) and the fused Lanczos step's scalars, prologue and epilogue (FusedArgs,
// fused_begin, fused_finish).  Whatever only one of the two files uses lives in that file.
// Device code: included by the two .hip files only, never by the host-only .cpp files or host tests.
#pragma once
#include "internal.h"
#include "reduce_dev.h"
#include "xch_dev.h"

namespace eigmi {

// Gathered operand x[g]: a plain vector, or the fused Lanczos step's u_k = t_{k-1} - c u_{k-1}
// formed on the fly from the interleaved (t, u) pair vector (mul then sub, -ffp-contract=off:
// bitwise what the step stores for u_k).
struct XPlain {
  const double *__restrict__ x;
  typedef double raw;
  __device__ __forceinline__ const void *ptr() const { return x; }
  __device__ __forceinline__ double operator()(i64 g) const { return x[g]; }
  __device__ __forceinline__ raw load(i64 g) const { return x[g]; }
  __device__ __forceinline__ double val(raw v) const { return v; }
};
// (t, u) interleaved: one 16-B gather fetches both operands of an entry.
typedef double dpair __attribute__((ext_vector_type(2)));
struct XPair {
  const dpair *__restrict__ p;
  double c;
  typedef dpair raw;
  __device__ __forceinline__ const void *ptr() const { return p; }
  __device__ __forceinline__ double operator()(i64 g) const
  {
    const dpair v = p[g];
    return v.x - c * v.y;
  }
  __device__ __forceinline__ raw load(i64 g) const { return p[g]; }
  __device__ __forceinline__ double val(raw v) const { return v.x - c * v.y; }
};

// Whole-wave lane shifts on the DPP path (GFX9 wave_shr:1 / wave_shl:1, VALU moves, no LDS):
// lane_prev(v) in lane l is v of lane l - 1, lane_next(v) is v of lane l + 1 (lane 0 / 63 get 0 and
// are patched by the caller).
__device__ __forceinline__ int dpp_prev(int v) { return __builtin_amdgcn_update_dpp(0, v, 0x138, 0xf, 0xf, true); }
__device__ __forceinline__ int dpp_next(int v) { return __builtin_amdgcn_update_dpp(0, v, 0x130, 0xf, 0xf, true); }
template <bool NEXT>
__device__ __forceinline__ double lane_shift(double v)
{
  const long long b = __double_as_longlong(v);
  const int lo = NEXT ? dpp_next((int)b) : dpp_prev((int)b);
  const int hi = NEXT ? dpp_next((int)(b >> 32)) : dpp_prev((int)(b >> 32));
  return __longlong_as_double(((long long)hi << 32) | (unsigned)lo);
}
template <bool NEXT>
__device__ __forceinline__ dpair lane_shift(dpair v)
{
  return dpair{lane_shift<NEXT>(v.x), lane_shift<NEXT>(v.y)};
}

// Symmetric band image (internal.h, eig_mat_s::sym_*): the stored diagonals of the upper triangle,
// one window-indexed array each; the entry at offset -d of row w is the entry at +d of row w - d.
struct SymImg {
  const double *val;  // nup arrays of ld doubles
  const void *mask;   // owned row r: bit k = row stores the entry at off[k] (u8 or u32 per row)
  i64 ld;
  int nd;                 // offsets, ascending = ISTL column order
  // near offsets {-1, 0, +1} (the lane-shift path): off[klo..khi) are the ones present; km1 / k0 /
  // kp1 their mask bits (-1 = absent), j0 / j1 the arrays of |d| = 0 / 1 (-1 = absent)
  int klo, khi, km1, k0, kp1, j0, j1;
  i32 off[kSymMaxOff];
  i32 dj[kSymMaxOff];     // array index of |off[k]|
};

// Offsets off[kb..ke) of row w: one coalesced value load each (at w for d >= 0, at w + d for d < 0:
// the mirrored upper entry, re-read from L2 / MALL after the rows d earlier streamed it) plus one
// coalesced gather; the mask gates the accumulation.
template <int KC, class X>
__device__ __forceinline__ void sym_span(const SymImg &S, int kb, int ke, unsigned m, i64 w, i64 wv, const X &x,
                                         i64 xl, double &acc)
{
  for (int k0 = kb; k0 < ke; k0 += KC)
  {
    double a[KC], xv[KC];
#pragma unroll
    for (int k = 0; k < KC; ++k)
    {
      const bool in = k0 + k < ke;
      const int d = in ? S.off[k0 + k] : 0;
      i64 g = w + d;
      g = g < 0 ? 0 : (g > xl ? xl : g);
      const i64 va = (i64)(in ? S.dj[k0 + k] : 0) * S.ld + (d < 0 ? g : wv);
      a[k] = in ? S.val[va] : 0.0;
      xv[k] = in ? x(g) : 0.0;
    }
#pragma unroll
    for (int k = 0; k < KC; ++k)
      if ((m >> (k0 + k)) & 1u) acc += a[k] * xv[k];
  }
}

struct SellB1 {
  const i64 *slice_ptr;
  const double *val;
  const i32 *col;
  const i32 *st_width;  // null when the image has no stencil slices
  const i32 *st_delta;
  const uint8_t *st_mask;
  i64 xlast;  // window length - 1 (gather clamp)
  SymImg sym;
};

inline SellB1 sell_b1(const eig_mat_s &A)
{
  SellB1 b{A.slice_ptr, A.val, A.col, A.st_width, A.st_delta, A.st_mask, A.window - 1, {}};
  if (A.sym_val)
  {
    b.sym.val = A.sym_val;
    b.sym.mask = A.sym_mask;
    b.sym.ld = A.sym_ld;
    b.sym.nd = A.sym_nd;
    for (int k = 0; k < kSymMaxOff; ++k)
    {
      b.sym.off[k] = k < A.sym_nd ? A.sym_off[k] : 0;
      b.sym.dj[k] = k < A.sym_nd ? A.sym_dj[k] : 0;
    }
    b.sym.klo = b.sym.khi = A.sym_nd;
    b.sym.km1 = b.sym.k0 = b.sym.kp1 = b.sym.j0 = b.sym.j1 = -1;
    for (int k = A.sym_nd - 1; k >= 0; --k)
    {
      const int d = A.sym_off[k];
      if (d >= -1) b.sym.klo = k;
      if (d > 1) b.sym.khi = k;
      if (d == -1) b.sym.km1 = k;
      if (d == 0) b.sym.k0 = k, b.sym.j0 = A.sym_dj[k];
      if (d == 1) b.sym.kp1 = k;
      if (d == 1 || d == -1) b.sym.j1 = A.sym_dj[k];
    }
  }
  return b;
}

// ---------------------------------------------------------------------------------------------
// Fused one-reduction Lanczos step.  u_k = t_{k-1} - c u_{k-1} is formed inside the
// gathers of the SpMV that needs it (XPair), and its squared norm is PREDICTED from the previous
// step's reductions instead of being reduced before the SpMV:
//   c = dsum/m,  nt_k = tsq - c dsum       (m = measured ||u_{k-1}||^2, reduced when u_{k-1} was
//                                             formed; using it keeps the prediction error at
//                                             rounding level -- tsq - alpha^2 alone diverges)
//   t_k = ((A u_k) - mu u_k) sig_k - gam_k u_{k-1},  sig_k = 1/sqrt(nt_k)
//   (dsum_k, tsq_k, m_k) = (t_k . u_k, t_k . t_k, u_k . u_k)   -> ONE allreduce of 3 doubles
// Guard against cancellation (nt_k = ||t||^2 - (t.u)^2/||u||^2 loses digits when |alpha| >> beta):
//  * the step runs on A - mu I, mu = trace(A)/n (a constant inside the spectrum): the Krylov space,
//    beta and alpha - mu are unchanged, but |alpha - mu| stays of the order of the spectral width
//    however far the operator is shifted (A + 1e6 I costs nothing extra);
//  * when the prediction still keeps less than kFusedTau of tsq (nt <= tau tsq, incl. nt <= 0 and
//    NaN), the launch REPAIRS instead of stepping: it forms u_k explicitly into the output pairs
//    (u_k, u_{k-1}) and reduces its exact norm; the next launch then takes step k with c = 0 and
//    the exact nt_k (the same per-row code: x - 0 y = x).  The decision is made on the device from
//    the allreduced sums (identical on every rank), so no step synchronises with the host; the
//    host tops the launch count up afterwards (drivers.cpp).  Launch L reads its logical step j
//    and mode from ctl[2L], ctl[2L+1] and block 0 writes those of launch L+1.
// Same formulas as orc_lanczos_fused (oracle.cc).
// ---------------------------------------------------------------------------------------------
constexpr double kFusedTau = 1e-2;
enum { kFusedStep = 0, kFusedPost = 1, kFusedHalt = 2, kFusedRepair = 3, kFusedNoop = 4 };

struct FusedArgs {
  double *nsum, *alpha, *beta;  // per logical step
  const double *fred;           // per launch: 3 allreduced sums
  int *ctl;                     // per launch: (logical step j, mode) at its start
  double *aux;                  // per launch: (rn, rm) handed from a repair to the next launch
  const double *mu2;            // (sum of the diagonal, rows), allreduced: mu = mu2[0] / mu2[1]
  double *pn;                   // per launch: nsum[j - 1] of its step (LanczosState::pn)
  int L;                        // launch index
  int force;                    // 1: repair even if the prediction is sound (exact final beta)
  int xch;                      // kXchPublish: the last workgroup allreduces the sums through the
                                // peers' mailboxes (xch_dev.h) instead of an allreduce launch after
  Mailbox mb;                   // (xch != 0) this rank's mailbox
};

struct FusedStep {
  int j, act;
  double c, nt, ap, bk, gam, sig, mu, rn, rm;
};

// Prologue of a fused launch (every thread; wave- and grid-uniform); block 0 / thread 0 stores the
// step's scalars and the next launch's control word.  Returns the action.
__device__ __forceinline__ FusedStep fused_begin(const FusedArgs &f)
{
  FusedStep s;
  // every operand the prologue may need, loaded together (addresses depend on L only: one memory
  // round trip before the launch's streams start, instead of ctl -> nsum[j - 1])
  const int cj = f.ctl[2 * f.L], mode = f.ctl[2 * f.L + 1];
  const double mu0 = f.mu2[0], mu1 = f.mu2[1];
  const int Lp = f.L > 0 ? f.L - 1 : 0;
  const double fd = f.fred[3 * Lp], fq = f.fred[3 * Lp + 1], fm = f.fred[3 * Lp + 2];
  const double ax0 = f.aux[2 * f.L], ax1 = f.aux[2 * f.L + 1], pnl = f.pn[f.L], ns0 = f.nsum[0];
  s.j = cj;
  s.mu = mu0 / mu1;
  s.c = s.ap = s.bk = s.gam = s.rn = s.rm = 0.0;
  s.nt = 1.0;
  const int j = s.j;
  if (mode == kFusedHalt) s.act = kFusedHalt;
  else if (f.force && (j == 0 || mode != kFusedStep)) s.act = kFusedNoop;
  else if (mode == kFusedPost)
  {
    const double mex = fm;
    s.rn = ax0;
    s.rm = ax1;
    s.nt = mex;
    if (!(mex > 0.0)) s.act = kFusedHalt;  // u_j = 0: invariant subspace
    else
    {
      s.bk = sqrt(mex) * s.rn / s.rm;
      s.gam = s.bk / s.rm;
      s.act = kFusedPost;
    }
  }
  else if (j == 0)
  {
    s.nt = ns0;
    s.act = kFusedStep;
  }
  else
  {
    const double d = fd, q = fq, m = fm;
    s.rn = sqrt(pnl);
    s.rm = sqrt(m);
    s.c = d / m;
    s.ap = s.c * s.rn + s.mu;
    s.nt = q - s.c * d;
    if (f.force || !(s.nt > kFusedTau * q)) s.act = kFusedRepair;
    else
    {
      s.bk = sqrt(s.nt) * s.rn / s.rm;
      s.gam = s.bk / s.rm;
      s.act = kFusedStep;
    }
  }
  s.sig = 1.0 / sqrt(s.nt);
  if (blockIdx.x == 0 && threadIdx.x == 0)  // (both launches of a split step store the same values)
  {
    int nj = j, nm = kFusedStep;
    switch (s.act)
    {
      case kFusedStep:
        if (j > 0)
        {
          f.nsum[j] = s.nt;
          f.alpha[j - 1] = s.ap;
          f.beta[j] = s.bk;
        }
        else
          f.beta[0] = sqrt(s.nt);
        nj = j + 1;
        break;
      case kFusedPost:
        f.nsum[j] = s.nt;
        f.beta[j] = s.bk;
        nj = j + 1;
        break;
      case kFusedRepair:
        f.alpha[j - 1] = s.ap;
        f.aux[2 * f.L + 2] = s.rn;
        f.aux[2 * f.L + 3] = s.rm;
        nm = kFusedPost;
        break;
      case kFusedHalt:
        if (mode == kFusedPost)
        {
          f.nsum[j] = 0.0;
          f.beta[j] = 0.0;
        }
        nm = kFusedHalt;
        break;
      default:  // kFusedNoop
        nm = mode;
        if (mode == kFusedPost)
        {
          f.aux[2 * f.L + 2] = f.aux[2 * f.L];
          f.aux[2 * f.L + 3] = f.aux[2 * f.L + 1];
        }
        break;
    }
    f.ctl[2 * f.L + 2] = nj;
    f.ctl[2 * f.L + 3] = nm;
    // nsum[j' - 1] for the next launch: the norm this launch fixed (step / post: nsum[j]); otherwise
    // the logical step does not advance and the value carries over
    f.pn[f.L + 1] = (s.act == kFusedStep || s.act == kFusedPost) ? s.nt : pnl;
  }
  return s;
}

// Launch with nothing to compute (halted recurrence, or a forced repair with nothing to repair):
// the reduction slot reads zero.
// (The host forces a repair only after reading a stepping state, so kFusedNoop is defensive.)
__device__ __forceinline__ void fused_idle(double *out)
{
  if (blockIdx.x == 0 && threadIdx.x < 3) out[threadIdx.x] = 0.0;
}

// End of a fused launch: the grid reduction of the three sums (plus a split step's carry) into
// out; with kXchPublish the last workgroup first allreduces them with the peers through their
// mailboxes (xch_dev.h), so out holds the global sums when the kernel ends.  An idle launch takes
// this path with zero sums when it exchanges (every rank idles at the same launch).
template <int U>
__device__ __forceinline__ void fused_finish(double (&v)[3], double *partials, unsigned *ticket, double *tot,
                                             double *out, const double *carry, const FusedArgs &fa)
{
  if (grid_sum<3, kStreamThreads, U>(v, partials, ticket, tot))
  {
    if (fa.xch & kXchPublish)
    {
      if (carry)
      {
        if (threadIdx.x < 3) tot[threadIdx.x] += carry[threadIdx.x];
        __syncthreads();
      }
      xch_exchange(fa.mb, tot);
      if (threadIdx.x < 3) out[threadIdx.x] = tot[threadIdx.x];
    }
    else if (threadIdx.x < 3)
      out[threadIdx.x] = carry ? (carry[threadIdx.x] + tot[threadIdx.x]) : tot[threadIdx.x];
  }
}

// Repair launch body for rows [r0, r1) (owned-row indices, grid-stride): u = t - c u_prev into the
// output pair (u, u_prev), and ||u||^2.  The same mul-then-sub as the gathers (XPair), so the step
// that follows multiplies exactly the u_k the unrepaired step would have formed.
__device__ __forceinline__ double fused_repair_rows(i64 r0, i64 r1, i64 own, double c, const dpair *__restrict__ P,
                                                    dpair *__restrict__ Pout)
{
  double m2 = 0.0;
  const i64 stride = (i64)gridDim.x * blockDim.x;
  for (i64 r = r0 + (i64)blockIdx.x * blockDim.x + threadIdx.x; r < r1; r += stride)
  {
    const dpair p = P[own + r];
    const double u = p.x - c * p.y;
    Pout[own + r] = dpair{u, p.y};
    m2 += u * u;
  }
  return m2;
}
}  // namespace eigmi
