// k_march.hip -- the plane-march kernels on the symmetric band image (gfx950), and their launchers.
//
// 2.5-D blocking of a banded 1x1 image: rows split into planes of D rows (D = the band's widest offset), a
// wave owns a 64-row column of a run of planes, and the +-D operands ride in registers from plane to plane
// ("Plane-marching fused step" below describes the march).  What runs on it:
//   k_spmv_march, k_lanczos_spmv_march, k_lanczos_fused_march -- eig_mv, the classic Lanczos kernel 1 and the
//     fused one-reduction step: bitwise the per-row arithmetic of the slice kernels k_spmv_b1 /
//     k_lanczos_spmv_b1 / k_lanczos_fused_b1 (k_spmv.hip).  Their row bodies, one per family of march
//     variants (march_variants.h): march_rows_geo, march_rows_geo2, march_rows_geo2_2l (with its DOWN and
//     PIPE bodies), march_rows_kuhn and the generic march_rows, which also dispatches to the others;
//   k_spmm8_march, k_spmm8_marchg -- the 8-column SpMM, and the fused Chebyshev step, on the same march;
//   k_sym_pack, k_kuhn_pack -- the packed value images some variants stream instead of the band arrays.
// Launchers: launch_spmv_march, launch_lanczos_spmv_march and launch_lanczos_fused_march are what launch_spmv,
// launch_lanczos_spmv and launch_lanczos_fused (k_spmv.hip) try first -- false where no plan applies, and
// the slice kernels then run; launch_spmm_march*, launch_cheb_march likewise for the multivector products.
//
// Device code and its launchers only.  Which image mode, march variant and plan a launch takes -- and the
// image modes, MarchPlan, GSpans and kWaves the kernels share with that logic -- are host-only code in
// march_plan.h / march_plan.cpp.  What the kernels share with the slice kernels is in spmv_dev.h.
#include "internal.h"
#include "march_plan.h"
#include "march_variants.h"
#include "spmv_dev.h"

#include <atomic>
#include <type_traits>

namespace eigmi {

// XCD-aware work-item order for the plane marches: workgroups are dealt round-robin over the 8 XCDs
// (MI355X_MICROARCH "Workgroup dispatch"), so workgroup b takes logical item swizzled_block(b) and
// each XCD walks ONE contiguous eighth of the items -- a column's +-plane neighbours then sit in
// the same XCD's L2.  Bijective for any grid size (the first G % 8 groups hold one workgroup more).
// (The slice kernels take plain contiguous chunks: measured faster there -- the 256 MB MALL
// already serves their plane re-reads.)
__device__ __forceinline__ i64 swizzled_block()
{
  const int G = gridDim.x, bid = blockIdx.x;
  if (G < 16) return bid;
  const int q = G >> 3, r = G & 7, x = bid & 7, i = bid >> 3;
  return (i64)(x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + i;
}

// ---------------------------------------------------------------------------------------------
// Plane-marching fused step (2.5-D blocking of the symmetric band image).  When the band's widest
// offset D (= N^2 for a 3-D 7-point grid, N for 2-D) is a multiple of 64 and every other offset is
// narrower, rows split into "planes" of D rows and a wave owns one 64-row column of a run of
// planes: lane l handles rows c*64 + l + z*D for z = z0 .. z1-1.  The -D neighbour of a row is then
// the row the same lane handled one iteration earlier and the +D neighbour the one it handles
// next, so the far pair operands and the mirrored -D value ride in registers: each (t, u) pair is
// loaded once (as the +D operand, then carried as the centre and as the -D operand) and each
// upper value once.  Offsets in (-D, D) other than -1/0/+1 are gathered (their rows were just
// streamed by the neighbouring columns of the same plane, on the same XCD: L2 hits); -1/0/+1 use
// the lane shifts.  Per-row arithmetic and order are those of row_sym (bitwise the same t, u);
// only the assignment of rows to waves differs, so the three reductions sum in another order.
// Work items (column, plane run) are spread so each XCD takes one contiguous plane run across all
// columns (swizzled_block): the column neighbours of a row share the XCD's L2.
// A launch's plan is a MarchPlan (march_plan.h), made by march_plan (march_plan.cpp).
// ---------------------------------------------------------------------------------------------
// store helper of the geo2 epilogues: temporal when the plan says the vectors fit the MALL
template <class T>
__device__ __forceinline__ void march_store(const MarchPlan &mp, T v, T *p)
{
  if (mp.tstore)
    *p = v;
  else
    __builtin_nontemporal_store(v, p);
}

// Geometric uniform-band march with the +D operand loaded PF + 1 planes ahead (march variants 3 .. 6;
// eig_mat_tune(EIG_TUNE_MARCH_PREFETCH)).  The plain march waits for every load of plane z --
// including the +D pair that only arrives from HBM -- and, at the loop head, for the store of
// plane z - 1 (one vmcnt counter, in order), so a wave has one plane's memory in flight.  Here the
// plane's loads are issued gathers first, prefetch last, so the waits for the L2 gathers leave the
// prefetch in flight; the prefetch slots rotate through a loop unrolled PF + 1 times (no register
// moves of in-flight loads); the edge operand is loaded by every lane (lanes 1..62 fetch lane 0's,
// one cache line) so no divergent branch merges pending loads; and there is no row test (a
// geometric image covers whole planes: every marched row exists).  Products, sums and their order
// are those of march_rows<UNI = 2>: bitwise the same results.
template <int PF, bool PG, class X, class EPI>
__device__ __forceinline__ void march_rows_geo(const SellB1 &A, const MarchPlan &mp, i64 own, int lane, int wave,
                                               const X &x, EPI &epi)
{
  typedef typename X::raw raw;
  const SymImg &S = A.sym;
  const int xl = (int)A.xlast, D = (int)mp.D, own32 = (int)own;
  const int nd = S.nd;
  const int item = (int)swizzled_block() * kWaves + wave;
  if (item >= mp.ncol * mp.nseg) return;
  const int col = item % mp.ncol, seg = item / mp.ncol;
  const int z0 = (int)(mp.zb + seg * mp.nplanes / mp.nseg), z1 = (int)(mp.zb + (seg + 1) * mp.nplanes / mp.nseg);
  auto cx = [&](int g) -> unsigned { return g < 0 ? 0u : (unsigned)(g > xl ? xl : g); };
  const int kn0 = 1, kp0 = S.khi, kp1 = nd - 1;
  unsigned gxy = 0;
  {
    const int pr = col * 64 + lane, gxc = pr % mp.gx, gyc = pr / mp.gx;
    unsigned b = 0;
    int k = 1;
    if (mp.dn) b |= (gyc > 0 ? 1u : 0u) << k++;
    b |= (gxc > 0 ? 1u : 0u) << k++;
    b |= 1u << k++;
    b |= (gxc < mp.gx - 1 ? 1u : 0u) << k++;
    if (mp.dq) b |= (gyc < mp.gy - 1 ? 1u : 0u) << k++;
    gxy = b;
  }
  int w = own32 + col * 64 + lane + z0 * D;
  const int eoff = lane == 63 ? 1 : -1 - lane;  // lane 63: row w + 1; the others: lane 0's row w - 1
  // slots: plane z's pair (the centre), z + 1 (the +D operand), ..., z + PF + 1 (in flight); body k
  // of a trip reads slots k and k + 1 and loads into slot k + PF + 1 (mod PF + 2): no slot is copied
  constexpr int NS = PF + 2;
  struct Gath {
    raw eg, xn, xq;
  };
  auto gather = [&](int wg, Gath &g) {
    g.eg = x.load(cx(wg + eoff));
    if (mp.dn) g.xn = x.load(cx(wg + mp.dn));
    if (mp.dq) g.xq = x.load(cx(wg + mp.dq));
  };
  double pmv = x.val(x.load(cx(w - D)));
  raw sl[NS];
  Gath gs[2];
#pragma unroll
  for (int k = 0; k <= PF; ++k) sl[k] = x.load(cx(w + k * D));
  if constexpr (PG) gather(w, gs[0]);
  // PG: plane z + 1's gathers are issued in body z (before its prefetch), so the wait for them in
  // body z + 1 leaves the loads of body z + 1 in flight as well
  auto body = [&](int z, const raw &pcur, const raw &pd, raw &pf, Gath &gc, Gath &gn) {
    if constexpr (PG)
      gather(w + D, gn);
    else
      gather(w, gc);
    pf = x.load(cx(w + (PF + 1) * D));
    const int zg = z + mp.gz0;
    const unsigned m = gxy | (zg > 0 ? 1u : 0u) | (zg < mp.gz - 1 ? 1u << kp1 : 0u);
    double acc = 0.0;
    if (m & 1u) acc += mp.cD * pmv;
    if (mp.dn && ((m >> kn0) & 1u)) acc += mp.cn * x.val(gc.xn);
    const double vc = x.val(pcur);
    double vl = lane_shift<false>(vc), vr = lane_shift<true>(vc);
    const double ve = x.val(gc.eg);
    if (lane == 0) vl = ve;
    if (lane == 63) vr = ve;
    if (S.km1 >= 0 && ((m >> S.km1) & 1u)) acc += mp.c1 * vl;
    if (S.k0 >= 0 && ((m >> S.k0) & 1u)) acc += mp.c0 * vc;
    if (S.kp1 >= 0 && ((m >> S.kp1) & 1u)) acc += mp.c1 * vr;
    if (mp.dq && ((m >> kp0) & 1u)) acc += mp.cq * x.val(gc.xq);
    if ((m >> kp1) & 1u) acc += mp.cD * x.val(pd);
    epi(w - own32, w, acc, pcur);
    pmv = vc;
    w += D;
  };
  // (NS bodies per trip; with PG the gather sets alternate, so NS must be even)
  static_assert(!PG || NS % 2 == 0, "gather prefetch: an even number of bodies per trip");
  int z = z0;
  for (; z + NS - 1 < z1; z += NS)
  {
#pragma unroll
    for (int k = 0; k < NS; ++k)
      body(z + k, sl[k], sl[(k + 1) % NS], sl[(k + PF + 1) % NS], gs[PG ? k & 1 : 0], gs[PG ? (k + 1) & 1 : 1]);
  }
#pragma unroll
  for (int k = 0; k < NS - 1; ++k)
    if (z + k < z1)
      body(z + k, sl[k], sl[(k + 1) % NS], sl[(k + PF + 1) % NS], gs[PG ? k & 1 : 0], gs[PG ? (k + 1) & 1 : 1]);
}

// Raw buffer loads (32-bit byte offset, hardware range check: an offset at or past the descriptor's
// byte count, or any offset through a zero-record descriptor, returns 0 without a memory access).
__device__ __forceinline__ void bload(__amdgpu_buffer_rsrc_t r, unsigned off, dpair &v)
{
  v = __builtin_bit_cast(dpair, __builtin_amdgcn_raw_buffer_load_b128(r, (int)off, 0, 0));
}
__device__ __forceinline__ void bload(__amdgpu_buffer_rsrc_t r, unsigned off, double &v)
{
  v = __builtin_bit_cast(double, __builtin_amdgcn_raw_buffer_load_b64(r, (int)off, 0, 0));
}
__device__ __forceinline__ void bload_nt(__amdgpu_buffer_rsrc_t r, unsigned off, dpair &v)
{
  v = __builtin_bit_cast(dpair, __builtin_amdgcn_raw_buffer_load_b128(r, (int)off, 0, 2));
}
__device__ __forceinline__ void bload_nt(__amdgpu_buffer_rsrc_t r, unsigned off, double &v)
{
  v = __builtin_bit_cast(double, __builtin_amdgcn_raw_buffer_load_b64(r, (int)off, 0, 2));
}
// lane l takes v of lane l - 1 (NEXT = false) or l + 1; the lane without a source keeps `old`
template <bool NEXT>
__device__ __forceinline__ double lane_shift_or(double v, double old)
{
  return __builtin_amdgcn_update_dpp(old, v, NEXT ? 0x130 : 0x138, 0xf, 0xf, false);
}

// Geometric uniform-band march without row masks or selects (UNI 7..9; grids whose x extent is a
// multiple of 64, so each wave's 64 rows share one y line and one plane, and windows under 2 GiB).
// Every stored offset of a row is its in-grid neighbour (verified at upload), so the only missing
// terms are at the grid faces -- and a missing neighbour's operand is made EXACTLY zero instead of
// being masked out: the -nx / +nx gathers of a wave on the first / last y line go through a
// zero-record buffer descriptor (wave-uniform choice), the +D operand of the last global plane too
// (plane-uniform), the -D operand of the first global plane is set to 0, and the lane-0 / lane-63
// edge operand of a wave at x = 0 / x = nx - 1 is an out-of-range offset (the other 62 lanes'
// edge loads are out of range as well: no traffic).  The value of a zero pair is +0 and the band
// constant times it is +-0; acc starts at +0 and can never become -0 under round-to-nearest, so
// acc + (+-0) == acc bit for bit (also for Inf / NaN acc): each row's sum, term order and rounding
// are those of march_rows<UNI = 2> -- bitwise the same results -- with ~half its VALU work (no
// mask bits, selects or 64-bit address clamps).  Prefetch slots as in march_rows_geo.
// pre(x): called once the wave's first loads are in flight (the fused step's scalar prologue runs
// under them; it sets x's scalars); false = the launch does not march (the loads are dropped).
struct MarchNoPre {
  template <class X>
  __device__ __forceinline__ bool operator()(X &) const { return true; }
};
// VAL (march variants 10 / 11: geometric bands whose values are not uniform): the band values are
// streamed from the symmetric band arrays instead -- the +D / 0 / +1 / +nx values of each row once
// (nontemporal), the mirrored -D value carried from the previous plane in a register, the mirrored
// -1 value by the same lane shift as the operands (lane 0 loads its own), the mirrored -nx value
// re-read at row w - nx (the +nx array, streamed 4 columns earlier on the same XCD: an L2 hit).
// A missing neighbour's value reads as 0.0 (its slot is unset, or the same zero-record / out-of-range
// load as its operand) and its operand as exactly zero, so its product is +-0 and the row's sum is
// that of the masked march bit for bit.  VAL = 2 (variant 11) issues the next plane's value streams
// one plane ahead (the last plane of a run issues none).
template <int PF, bool PG, int VAL, class X, class EPI, class PRE>
__device__ __forceinline__ void march_rows_geo2(const SellB1 &A, const MarchPlan &mp, i64 own, int lane, int wave,
                                                X x, EPI &epi, PRE &pre)
{
  typedef typename X::raw raw;
  constexpr unsigned SZ = sizeof(raw);
  const int D = (int)mp.D, own32 = (int)own;
  int col, seg;
  if (mp.lines == 4)
  {
    // workgroup -> (x run, group of 4 lines, plane run); wave -> line of the group
    const int nxc = mp.gx / 64, per = nxc * (mp.gy / 4);
    const int wg = (int)swizzled_block();
    if (wg >= per * mp.nseg) return;
    seg = wg / per;
    const int r = wg % per;
    col = ((r / nxc) * 4 + wave) * nxc + r % nxc;
  }
  else
  {
    const int item = (int)swizzled_block() * kWaves + wave;
    if (item >= mp.ncol * mp.nseg) return;
    col = item % mp.ncol;
    seg = item / mp.ncol;
  }
  const int z0 = (int)(mp.zb + seg * mp.nplanes / mp.nseg), z1 = (int)(mp.zb + (seg + 1) * mp.nplanes / mp.nseg);
  const unsigned nbytes = (unsigned)(A.xlast + 1) * SZ;
  const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(x.ptr()), 0, (int)nbytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t r0 = __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(x.ptr()), 0, 0, 0x00020000);
  // the wave's line: first x and its y (wave-uniform)
  const int x0 = (col * 64) % mp.gx, yw = (col * 64) / mp.gx;
  // (2-D grids have no +-nx offsets: both gathers read zeros through r0, and cn = cq = 0, so
  // their terms add +-0 -- no branch around a load in the loop)
  const __amdgpu_buffer_rsrc_t rn = mp.dn && yw > 0 ? rs : r0, rq = mp.dq && yw < mp.gy - 1 ? rs : r0;
  constexpr unsigned kOut = 0x80000000u;  // + any window offset (< 2 GiB): past the byte count
  const unsigned eoff = lane == 0 ? (x0 > 0 ? 0u - SZ : kOut) : lane == 63 ? (x0 + 64 < mp.gx ? SZ : kOut) : kOut;
  const unsigned dnb = (unsigned)mp.dn * SZ, dqb = (unsigned)mp.dq * SZ, Db = (unsigned)D * SZ;
  int w = own32 + col * 64 + lane + z0 * D;
  unsigned vo = (unsigned)w * SZ;
  const int zg0 = z0 + mp.gz0;
  constexpr int NS = PF + 2;
  struct Gath {
    raw eg, xn, xq;
  };
  auto gather = [&](unsigned v, Gath &g) {
    bload(rs, v + eoff, g.eg);
    bload(rn, v + dnb, g.xn);
    bload(rq, v + dqb, g.xq);
  };
  // VAL: one descriptor per band array (8-B slots, window-indexed like the operands); vv = w * 8
  const SymImg &S = A.sym;
  const unsigned vbytes = (unsigned)S.ld * 8u;
  auto arr = [&](int j, bool on) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<double *>(S.val + (i64)(j >= 0 ? j : 0) * S.ld), 0,
                                             on && j >= 0 ? (int)vbytes : 0, 0x00020000);
  };
  const __amdgpu_buffer_rsrc_t vD = arr(S.dj[S.nd - 1], VAL), v0 = arr(S.j0, VAL), v1 = arr(S.j1, VAL),
                               vq = arr(S.dj[S.khi], VAL && mp.dq), vn = arr(S.dj[S.khi], VAL && mp.dn && yw > 0);
  const unsigned eov = lane == 0 && x0 > 0 ? 0u - 8u : kOut;  // lane 0: the mirrored -1 value at w - 1
  const unsigned dnv = (unsigned)mp.dn * 8u, Dv = (unsigned)D * 8u;
  unsigned vv = (unsigned)w * 8u;
  struct Vals {
    double aD, a0, ap, aq, an, ae;
  };
  const __amdgpu_buffer_rsrc_t vz = arr(0, false);
  const double *pD = S.val + (i64)S.dj[S.nd - 1] * S.ld, *p1 = S.val + (i64)(S.j1 >= 0 ? S.j1 : 0) * S.ld;
  const double *p0 = S.j0 >= 0 ? S.val + (i64)S.j0 * S.ld : nullptr, *pq = S.val + (i64)S.dj[S.khi] * S.ld;
  auto vload = [&](unsigned o, Vals &v, bool on) {  // on: wave-uniform (false: zeros, no traffic)
    if constexpr (VAL == 5)
    {
      // variant 15: the pack through 64-bit global addresses (wave-uniform / lane-0 conditions
      // instead of range-checked descriptors)
      const i64 r = (i64)(o >> 3);
      const dpair *P01 = reinterpret_cast<const dpair *>(mp.pack), *P23 = P01 + S.ld;
      const dpair p0 = (mp.cache & 2) ? P01[r] : __builtin_nontemporal_load(P01 + r);
      const dpair p1 = P23[r];
      v.aD = p0.x;
      v.a0 = p0.y;
      v.ap = p1.x;
      v.aq = p1.y;
      v.an = mp.dn && yw > 0 ? P23[r + mp.dn].y : 0.0;
      v.ae = lane == 0 && x0 > 0 ? P23[r - 1].x : 0.0;
    }
    else if constexpr (VAL == 4)
    {
      // (measurement variant 14: the same loads through 64-bit global addresses, as the plain march)
      const i64 r = (i64)(o >> 3);
      v.aD = on ? __builtin_nontemporal_load(pD + r) : 0.0;
      v.a0 = on && p0 ? __builtin_nontemporal_load(p0 + r) : 0.0;
      v.ap = on ? __builtin_nontemporal_load(p1 + r) : 0.0;
      v.aq = on && mp.dq ? pq[r] : 0.0;
      v.an = on && mp.dn && yw > 0 ? pq[r + mp.dn] : 0.0;
      v.ae = on && lane == 0 && x0 > 0 ? p1[r - 1] : 0.0;
    }
    else
    {
      v.aD = __builtin_bit_cast(double, __builtin_amdgcn_raw_buffer_load_b64(on ? vD : vz, (int)o, 0, 2));
      v.a0 = __builtin_bit_cast(double, __builtin_amdgcn_raw_buffer_load_b64(on ? v0 : vz, (int)o, 0, 2));
      v.ap = __builtin_bit_cast(double, __builtin_amdgcn_raw_buffer_load_b64(on ? v1 : vz, (int)o, 0, 2));
      v.aq = __builtin_bit_cast(double, __builtin_amdgcn_raw_buffer_load_b64(on ? vq : vz, (int)o, 0, 0));
      v.an = __builtin_bit_cast(double, __builtin_amdgcn_raw_buffer_load_b64(on ? vn : vz, (int)(o + dnv), 0, 0));
      v.ae = __builtin_bit_cast(double, __builtin_amdgcn_raw_buffer_load_b64(on ? v1 : vz, (int)(o + eov), 0, 0));
    }
  };
  constexpr bool VPF = VAL == 2;  // value streams one plane ahead
  Vals vs[2];
  double amD = 0.0;  // VAL: the mirrored -D value (the +D value of the row below)
  raw pm{};
  if (zg0 > 0)
  {
    bload(rs, vo - Db, pm);  // (plane 0 of the grid: no -D neighbour)
    if constexpr (VAL) amD = __builtin_bit_cast(double, __builtin_amdgcn_raw_buffer_load_b64(vD, (int)(vv - Dv), 0, 0));
  }
  raw sl[NS];
  bload(rs, vo, sl[0]);
#pragma unroll
  for (int k = 1; k <= PF; ++k) bload(zg0 + k < mp.gz ? rs : r0, vo + (unsigned)k * Db, sl[k]);
  Gath gs[2];
  if constexpr (PG) gather(vo, gs[0]);
  if constexpr (VPF) vload(vv, vs[0], true);
  if (!pre(x)) return;
  double pmv = zg0 > 0 ? x.val(pm) : 0.0;
  auto body = [&](int z, const raw &pcur, const raw &pd, raw &pf, Gath &gc, Gath &gn, Vals &vc_, Vals &vn_) {
    if constexpr (PG)
      gather(vo + Db, gn);
    else
      gather(vo, gc);
    if constexpr (VAL == 1 || VAL >= 4) vload(vv, vc_, true);
    const int zg = z + mp.gz0;
    if (VAL == 5 && (mp.cache & 4))
      bload_nt(zg + PF + 1 < mp.gz ? rs : r0, vo + (unsigned)(PF + 1) * Db, pf);
    else
      bload(zg + PF + 1 < mp.gz ? rs : r0, vo + (unsigned)(PF + 1) * Db, pf);
    if constexpr (VPF) vload(vv + Dv, vn_, z + 1 < z1);
    double acc = 0.0;
    const double vc = x.val(pcur), ve = x.val(gc.eg);
    const double vl = lane_shift_or<false>(vc, ve), vr = lane_shift_or<true>(vc, ve);
    if constexpr (VAL)
    {
      const double am = lane_shift_or<false>(vc_.ap, vc_.ae);
      acc += amD * pmv;
      acc += vc_.an * x.val(gc.xn);
      acc += am * vl;
      acc += vc_.a0 * vc;
      acc += vc_.ap * vr;
      acc += vc_.aq * x.val(gc.xq);
      acc += vc_.aD * x.val(pd);
      amD = vc_.aD;
    }
    else
    {
      acc += mp.cD * pmv;
      acc += mp.cn * x.val(gc.xn);
      acc += mp.c1 * vl;
      acc += mp.c0 * vc;
      acc += mp.c1 * vr;
      acc += mp.cq * x.val(gc.xq);
      acc += mp.cD * x.val(pd);
    }
    epi(w - own32, w, acc, pcur);
    pmv = vc;
    w += D;
    vo += Db;
    vv += Dv;
  };
  static_assert(!PG || NS % 2 == 0, "gather prefetch: an even number of bodies per trip");
  static_assert(!VPF || NS % 2 == 0, "value prefetch: an even number of bodies per trip");
  int z = z0;
  for (; z + NS - 1 < z1; z += NS)
  {
#pragma unroll
    for (int k = 0; k < NS; ++k)
      body(z + k, sl[k], sl[(k + 1) % NS], sl[(k + PF + 1) % NS], gs[PG ? k & 1 : 0], gs[PG ? (k + 1) & 1 : 1],
           vs[VPF ? k & 1 : 0], vs[VPF ? (k + 1) & 1 : 1]);
  }
#pragma unroll
  for (int k = 0; k < NS - 1; ++k)
    if (z + k < z1)
      body(z + k, sl[k], sl[(k + 1) % NS], sl[(k + PF + 1) % NS], gs[PG ? k & 1 : 0], gs[PG ? (k + 1) & 1 : 1],
           vs[VPF ? k & 1 : 0], vs[VPF ? (k + 1) & 1 : 1]);
}

// Value march with TWO grid lines per wave (march variant 22; round 6): lane = x of a 64-x run, the
// wave's rows (x, y0) and (x, y0 + 1) of every plane it marches (y0 even; mp.ncol counts line PAIRS).
// Per plane and lane, two rows of variant 15 (the pair pack through 64-bit addresses, the +D operand
// loaded, the centre and -D carried), except that each line's neighbour across the pair comes from
// registers: line y0's +nx operand is line y0 + 1's centre, line y0 + 1's -nx operand is line y0's
// centre and its mirrored -nx value a(w + nx, w) = a(w, w + nx) is line y0's own (+1, +nx) pack
// entry.  Gathered: line y0 - 1's operand and mirrored value, line y0 + 2's operand -- half of the
// gathers of variant 15, whose mirrored value gathers cost 13 us at 256^3 (section 4e ablation).  Every
// row sums the same products in the same order as variant 15 (bitwise its rows); the launch's three
// sums add the rows in another order (each lane adds its two rows per plane).
// (Where it is the default, with its measurements: kMarch2lDefault, march_plan.h.)
// DOWN (variants 22 / 23, MarchPlan::down; DESIGN section 4e "serpentine"): the same work items march their
// runs from plane z1 - 1 down to z0, so a launch that follows an upward one starts on the planes that one
// touched last -- what the 256 MiB memory-side cache can still hold of the previous launch's pair stores
// and of the value pack.  What is carried and what is loaded swap: the centres, the plane's diagonal
// values and its two +D products a(w, w + D) u(w + D), already rounded (both factors were at hand one
// plane above: the (+D, 0) pair loaded there and that plane's centre), ride in registers; per plane the -D
// operands (the next centres) and the (+D, 0) pairs of the plane BELOW are loaded -- their .x is this
// plane's mirrored -D value, and .x times this plane's centre and .y are what the next plane carries.
// Each row still adds its seven products in the order -D, -nx, -1, 0, +1, +nx, +D; without contraction
// (-ffp-contract=off) a product rounds the same wherever it is formed, so the rows are bitwise the upward
// ones; a lane adds its rows into the launch's three sums top plane first.
// (Which launches march down, with the measurements: kMarch2lSerpentine, march_plan.h.  The variants whose
// kernels hold this body: MarchTraits::down_body.)

// PIPE (the fused launches of variants 22 / 23 where MarchPlan::pipe is set; DESIGN section 4e "pipeline"): with
// one wave per SIMD nothing else issues loads while the wave does a plane's arithmetic, and the registers
// hold one plane of loads, so every iteration of the bodies below pays the memory latency and the arithmetic
// one after the other.  Here every loop load is an LDS-DMA (buffer_load ... lds: no register destination)
// issued ONE PLANE AHEAD into the other of two LDS buffers of the wave; a buffer is kMarchPipeRegions
// lane-linear regions of 64 x 16 B, one region per load, wave-private -- no barrier.  Iteration z issues plane
// z +- 1's 13 DMAs, waits with one counted vmcnt that retires plane z's (the new 13 and the previous plane's
// 2 stores stay in flight), reads its operands back (ds_read_b128, waited for inside the reading statement,
// so the buffer is free before the iteration after refills it) and does the arithmetic of the plain body in
// its order.  A DMA's address is always in range: where the plain body reads an exact zero through a
// zero-record descriptor or an out-of-range offset (grid faces, the planes below the first and above the
// last), the DMA reads the lane's own row instead and the zero is selected after the LDS read (the
// conditions are wave- or lane-uniform) -- the same +0 operands, so every row is bitwise the plain body's,
// and a lane adds its rows into the three sums in the same order: alpha and beta are bitwise too.  The 8-B
// loads (line y0 - 1's mirrored value, lane 0's mirrored -1 values) are 16-B DMAs of the pair that holds them.
// Measured at 256^3, 7 interleaved rounds (profiles/r08_pipe_sweep.jsonl): 180.3 us against 185.1
// for the plain bodies (max - min 0.8) -- the gain is the downward launches' (all-down 189.3 against 195.4;
// all-up 189.8 either way: the plain upward body already overlapped most of its products with the loads).
// (The variants whose fused kernel holds these bodies: MarchTraits::pipe_body; kMarchPipeRegions and the LDS
// sizes: march_plan.h.)
typedef __attribute__((address_space(3))) char lds_char;
template <int AUX>
__device__ __forceinline__ void bdma(__amdgpu_buffer_rsrc_t r, unsigned off, lds_char *l)
{
  __builtin_amdgcn_raw_ptr_buffer_load_lds(r, l, 16, (int)off, 0, 0, AUX);
}
// LDS reads of a plane's operands (a: the lane's slot of region 0) and the wait for them, in one statement each:
// the compiler neither sees an LDS-DMA's write nor counts these reads.  Three statements, the operands that
// shrink to their values first, so that a plane's 13 operands are never all in registers at once.
// regions 6, 7, 9, 10 (whole pairs), the .y of region 8's pair, the .x of the pairs of regions 11 and 12
__device__ __forceinline__ void lds_read_near(unsigned a, dpair &r6, dpair &r7, dpair &r9, dpair &r10, double &y8,
                                              double &x11, double &x12)
{
  asm volatile("ds_read_b128 %0, %7 offset:6144\n\tds_read_b128 %1, %7 offset:7168\n\t"
               "ds_read_b128 %2, %7 offset:9216\n\tds_read_b128 %3, %7 offset:10240\n\t"
               "ds_read_b64 %4, %7 offset:8200\n\tds_read_b64 %5, %7 offset:11264\n\t"
               "ds_read_b64 %6, %7 offset:12288\n\ts_waitcnt lgkmcnt(0)"
               : "=&v"(r6), "=&v"(r7), "=&v"(r9), "=&v"(r10), "=&v"(y8), "=&v"(x11), "=&v"(x12)
               : "v"(a)
               : "memory");
}
// regions 4, 5, 0, 1
__device__ __forceinline__ void lds_read_mid(unsigned a, dpair &r4, dpair &r5, dpair &r0, dpair &r1)
{
  asm volatile("ds_read_b128 %0, %4 offset:4096\n\tds_read_b128 %1, %4 offset:5120\n\tds_read_b128 %2, %4\n\t"
               "ds_read_b128 %3, %4 offset:1024\n\ts_waitcnt lgkmcnt(0)"
               : "=&v"(r4), "=&v"(r5), "=&v"(r0), "=&v"(r1)
               : "v"(a)
               : "memory");
}
// regions 2, 3
__device__ __forceinline__ void lds_read_far(unsigned a, dpair &r2, dpair &r3)
{
  asm volatile("ds_read_b128 %0, %2 offset:2048\n\tds_read_b128 %1, %2 offset:3072\n\ts_waitcnt lgkmcnt(0)"
               : "=&v"(r2), "=&v"(r3)
               : "v"(a)
               : "memory");
}

template <bool DOWN, bool PIPE = false, class X, class EPI, class PRE>
__device__ __forceinline__ void march_rows_geo2_2l(const SellB1 &A, const MarchPlan &mp, i64 own, int lane, int wave,
                                                   X x, EPI &epi, PRE &pre)
{
  typedef typename X::raw raw;
  constexpr unsigned SZ = sizeof(raw);
  const int D = (int)mp.D, own32 = (int)own, gx = mp.gx;
  const int item = (int)swizzled_block() * kWaves + wave;
  if (item >= mp.ncol * mp.nseg) return;
  const int col2 = item % mp.ncol, seg = item / mp.ncol;
  const int xcols = gx / 64;
  const int x0 = (col2 % xcols) * 64, y0 = (col2 / xcols) * 2;
  const int z0 = (int)(mp.zb + seg * mp.nplanes / mp.nseg), z1 = (int)(mp.zb + (seg + 1) * mp.nplanes / mp.nseg);
  const unsigned nbytes = (unsigned)(A.xlast + 1) * SZ;
  const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(x.ptr()), 0, (int)nbytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t r0 = __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(x.ptr()), 0, 0, 0x00020000);
  // line y0 - 1 (operand + mirrored value gathered) and line y0 + 2 (operand gathered)
  const bool has_n = mp.dn && y0 > 0, has_q = mp.dq && y0 + 2 < mp.gy;
  const __amdgpu_buffer_rsrc_t rn = has_n ? rs : r0, rq = has_q ? rs : r0;
  constexpr unsigned kOut = 0x80000000u;
  const unsigned eoff = lane == 0 ? (x0 > 0 ? 0u - SZ : kOut) : lane == 63 ? (x0 + 64 < gx ? SZ : kOut) : kOut;
  const unsigned dnb = (unsigned)mp.dn * SZ, dqb = (unsigned)mp.dq * SZ, Db = (unsigned)D * SZ, nxb = (unsigned)gx * SZ;
  int w = own32 + y0 * gx + x0 + lane + z0 * D;  // line y0's row; line y0 + 1's at w + gx
  unsigned vo = (unsigned)w * SZ;
  const int zg0 = z0 + mp.gz0;
  const SymImg &S = A.sym;
  const dpair *P01 = reinterpret_cast<const dpair *>(mp.pack), *P23 = P01 + S.ld;
  const bool le = lane == 0 && x0 > 0;  // lane 0's mirrored -1 value (row x0 - 1) exists
  if constexpr (PIPE)
  {
    static_assert(SZ == sizeof(dpair), "the pipelined body marches the fused step's pair vector");
    extern __shared__ char march_pipe_lds[];
    lds_char *const Lw = (lds_char *)march_pipe_lds + (unsigned)wave * (2 * kMarchPipeBuf);
    const unsigned ra0 = (unsigned)(size_t)Lw + (unsigned)lane * 16u;  // the lane's slot of region 0, buffer 0
    // the pack through one descriptor too, its second pair array ldb bytes on (the plan admits the body only
    // where these byte offsets fit 32 bits)
    const unsigned ldb = (unsigned)S.ld * 16u;
    const __amdgpu_buffer_rsrc_t rp = __builtin_amdgcn_make_buffer_rsrc(const_cast<dpair *>(P01), 0, (int)(2u * ldb), 0x00020000);
    const bool edge = lane == 0 || lane == 63;
    // offsets of the operands that may be missing: the lane's own row (0) where they are.  eo: the row across
    // the wave edge (lanes 0 and 63; 0 elsewhere too); lo: the row before lane 0's (wave-uniform: only lane 0's
    // mirrored -1 value is ever used, lane_shift_or keeps it for the lane without a source)
    const bool lok = x0 > 0;
    const unsigned eo = lane == 0 ? (lok ? 0u - SZ : 0u) : (lane == 63 && x0 + 64 < gx ? SZ : 0u), lo = lok ? 0u - SZ : 0u;
    const unsigned no = has_n ? dnb : 0u, qo = has_q ? dqb : 0u;
    // regions: 0, 1 the far (+-D) operands of the two lines; 2, 3 the (+D, 0) values (xfar / pfar: the byte
    // offsets of the plane they come from); 4, 5 the (+1, +nx) values; 6, 7 the operands of lines y0 - 1,
    // y0 + 2; 8 line y0 - 1's (+1, +nx) values; 9, 10 the x-edge operands (lanes 0 and 63); 11, 12 the
    // (+1, +nx) values of the rows before lane 0's
    auto issue = [&](unsigned v, unsigned xfar, unsigned pfar, lds_char *L) {
      bdma<0>(rs, v + xfar, L);
      bdma<0>(rs, v + nxb + xfar, L + 1024);
      if (mp.cache & 2)
      {
        bdma<0>(rp, v + pfar, L + 2 * 1024);
        bdma<0>(rp, v + nxb + pfar, L + 3 * 1024);
      }
      else
      {
        bdma<2>(rp, v + pfar, L + 2 * 1024);
        bdma<2>(rp, v + nxb + pfar, L + 3 * 1024);
      }
      bdma<0>(rp, v + ldb, L + 4 * 1024);
      bdma<0>(rp, v + ldb + nxb, L + 5 * 1024);
      bdma<0>(rs, v + no, L + 6 * 1024);
      bdma<0>(rs, v + nxb + qo, L + 7 * 1024);
      bdma<0>(rp, v + ldb + no, L + 8 * 1024);
      if (edge)
      {
        bdma<0>(rs, v + eo, L + 9 * 1024);
        bdma<0>(rs, v + nxb + eo, L + 10 * 1024);
      }
      if (lane == 0)
      {
        bdma<0>(rp, v + ldb + lo, L + 11 * 1024);
        bdma<0>(rp, v + ldb + nxb + lo, L + 12 * 1024);
      }
    };
    const dpair zero = dpair{0.0, 0.0};
    // "the operand exists" = its offset is not 0, compared per plane: the kernel is at its scalar-register
    // limit, and a condition mask kept over the loop is two registers that then spill
    auto eok = [&] {  // the lane's row across the wave edge
      unsigned t = eo;
      asm volatile("" : "+v"(t));
      return t != 0u;
    };
    auto nz = [](unsigned t) {  // (wave-uniform offsets)
      t = __builtin_amdgcn_readfirstlane(t);
      asm volatile("" : "+s"(t));
      return t != 0u;
    };
    unsigned bo = 0;  // byte offset of the buffer that holds the plane at hand
    if constexpr (DOWN)
    {
      auto row = [&](double amD, double vmD, double an, double vn, double am, double vl, double a0, double vc, double a1,
                     double vr, double aq, double vq, double prodD) {
        double acc = 0.0;
        acc += amD * vmD;
        acc += an * vn;
        acc += am * vl;
        acc += a0 * vc;
        acc += a1 * vr;
        acc += aq * vq;
        acc += prodD;
        return acc;
      };
      w += (z1 - 1 - z0) * D;
      vo = (unsigned)w * SZ;
      const int gbot = -mp.gz0;  // the rank's index of global plane 0: plane z has a plane below when z > gbot
      issue(vo, z1 - 1 > gbot ? 0u - Db : 0u, z1 - 1 > gbot ? 0u - Db : 0u, Lw);
      const bool above = z1 + mp.gz0 < mp.gz;
      raw pu0{}, pu1{};
      if (above)
      {
        bload(rs, vo + Db, pu0);
        bload(rs, vo + nxb + Db, pu1);
      }
      dpair p0a = (mp.cache & 2) ? P01[w] : __builtin_nontemporal_load(P01 + w);
      dpair p1a = (mp.cache & 2) ? P01[w + gx] : __builtin_nontemporal_load(P01 + w + gx);
      raw c0, c1;
      bload(rs, vo, c0);
      bload(rs, vo + nxb, c1);
      const bool go = pre(x);
      // every load so far lands here: a later use of an ordinary load would drain the DMAs in flight with it
      asm volatile("s_waitcnt vmcnt(0)" : "+v"(pu0), "+v"(pu1), "+v"(p0a), "+v"(p1a), "+v"(c0), "+v"(c1)::"memory");
      if (!go) return;
      double a00 = p0a.y, a01 = p1a.y;
      double pD0 = p0a.x * (above ? x.val(pu0) : 0.0), pD1 = p1a.x * (above ? x.val(pu1) : 0.0);
      for (int z = z1 - 1; z >= z0; --z)
      {
        // in order on the counter: this plane's 13 DMAs, the previous plane's 2 stores, the next plane's 13 DMAs
        if (z > z0)
        {
          const unsigned far = z - 1 > gbot ? 0u - Db : 0u;
          issue(vo - Db, far, far, Lw + (bo ^ kMarchPipeBuf));
          asm volatile("s_waitcnt vmcnt(15)" ::: "memory");
        }
        else
          asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
        dpair m0, m1, q0a, q1a, p0b, p1b, xn0, xq1, eg0, eg1;
        double any, ae0x, ae1x;
        lds_read_near(ra0 + bo, xn0, xq1, eg0, eg1, any, ae0x, ae1x);
        const bool hn = nz(no), lk = nz(lo);
        if (!hn) xn0 = zero;
        if (!nz(qo)) xq1 = zero;
        if (!eok()) eg0 = eg1 = zero;
        const double an0 = hn ? any : 0.0;
        const double ae0 = lk ? ae0x : 0.0, ae1 = lk ? ae1x : 0.0;
        double vn0 = x.val(xn0), vq1 = x.val(xq1), ve0 = x.val(eg0), ve1 = x.val(eg1);
        asm volatile("" : "+v"(vn0), "+v"(vq1), "+v"(ve0), "+v"(ve1));  // (the pairs are dead before the next reads)
        lds_read_mid(ra0 + bo, p0b, p1b, m0, m1);
        lds_read_far(ra0 + bo, q0a, q1a);
        if (!(z > gbot)) m0 = m1 = q0a = q1a = zero;
        const double vc0 = x.val(c0), vc1 = x.val(c1);
        const double acc0 = row(q0a.x, x.val(m0), an0, vn0, lane_shift_or<false>(p0b.x, ae0),
                                lane_shift_or<false>(vc0, ve0), a00, vc0, p0b.x, lane_shift_or<true>(vc0, ve0), p0b.y,
                                vc1, pD0);
        const double acc1 = row(q1a.x, x.val(m1), p0b.y, vc0, lane_shift_or<false>(p1b.x, ae1),
                                lane_shift_or<false>(vc1, ve1), a01, vc1, p1b.x, lane_shift_or<true>(vc1, ve1), p1b.y,
                                vq1, pD1);
        epi(w - own32, w, acc0, c0);
        epi(w + gx - own32, w + gx, acc1, c1);
        pD0 = q0a.x * vc0;
        pD1 = q1a.x * vc1;
        a00 = q0a.y;
        a01 = q1a.y;
        c0 = m0;
        c1 = m1;
        w -= D;
        vo -= Db;
        bo ^= kMarchPipeBuf;
      }
    }
    else
    {
      const int gtop = mp.gz - 1 - mp.gz0;  // the rank's index of the top global plane: plane z has one above when z < gtop
      issue(vo, z0 < gtop ? Db : 0u, 0u, Lw);
      double amD0 = 0.0, amD1 = 0.0;
      raw pm0{}, pm1{};
      if (zg0 > 0)
      {
        bload(rs, vo - Db, pm0);
        bload(rs, vo + nxb - Db, pm1);
        amD0 = P01[w - D].x;
        amD1 = P01[w + gx - D].x;
      }
      raw c0, c1;
      bload(rs, vo, c0);
      bload(rs, vo + nxb, c1);
      const bool go = pre(x);
      // every load so far lands here: a later use of an ordinary load would drain the DMAs in flight with it
      asm volatile("s_waitcnt vmcnt(0)" : "+v"(pm0), "+v"(pm1), "+v"(amD0), "+v"(amD1), "+v"(c0), "+v"(c1)::"memory");
      if (!go) return;
      double pmv0 = zg0 > 0 ? x.val(pm0) : 0.0, pmv1 = zg0 > 0 ? x.val(pm1) : 0.0;
      for (int z = z0; z < z1; ++z)
      {
        // in order on the counter: this plane's 13 DMAs, the previous plane's 2 stores, the next plane's 13 DMAs
        if (z + 1 < z1)
        {
          issue(vo + Db, z + 1 < gtop ? Db : 0u, 0u, Lw + (bo ^ kMarchPipeBuf));
          asm volatile("s_waitcnt vmcnt(15)" ::: "memory");
        }
        else
          asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
        dpair d0, d1, p0a, p1a, p0b, p1b, xn0, xq1, eg0, eg1;
        double any, ae0x, ae1x;
        lds_read_near(ra0 + bo, xn0, xq1, eg0, eg1, any, ae0x, ae1x);
        const bool hn = nz(no), lk = nz(lo);
        if (!hn) xn0 = zero;
        if (!nz(qo)) xq1 = zero;
        if (!eok()) eg0 = eg1 = zero;
        const double an0 = hn ? any : 0.0;
        const double ae0 = lk ? ae0x : 0.0, ae1 = lk ? ae1x : 0.0;
        double vn0 = x.val(xn0), vq1 = x.val(xq1), ve0 = x.val(eg0), ve1 = x.val(eg1);
        asm volatile("" : "+v"(vn0), "+v"(vq1), "+v"(ve0), "+v"(ve1));  // (the pairs are dead before the next reads)
        lds_read_mid(ra0 + bo, p0b, p1b, d0, d1);
        lds_read_far(ra0 + bo, p0a, p1a);
        if (!(z < gtop)) d0 = d1 = zero;
        const double vc0 = x.val(c0), vc1 = x.val(c1);
        double acc0 = 0.0, acc1 = 0.0;
        {
          const double ve = ve0;
          const double vl = lane_shift_or<false>(vc0, ve), vr = lane_shift_or<true>(vc0, ve);
          const double am = lane_shift_or<false>(p0b.x, ae0);
          acc0 += amD0 * pmv0;
          acc0 += an0 * vn0;
          acc0 += am * vl;
          acc0 += p0a.y * vc0;
          acc0 += p0b.x * vr;
          acc0 += p0b.y * vc1;
          acc0 += p0a.x * x.val(d0);
        }
        {
          const double ve = ve1;
          const double vl = lane_shift_or<false>(vc1, ve), vr = lane_shift_or<true>(vc1, ve);
          const double am = lane_shift_or<false>(p1b.x, ae1);
          acc1 += amD1 * pmv1;
          acc1 += p0b.y * vc0;
          acc1 += am * vl;
          acc1 += p1a.y * vc1;
          acc1 += p1b.x * vr;
          acc1 += p1b.y * vq1;
          acc1 += p1a.x * x.val(d1);
        }
        epi(w - own32, w, acc0, c0);
        epi(w + gx - own32, w + gx, acc1, c1);
        pmv0 = vc0;
        pmv1 = vc1;
        amD0 = p0a.x;
        amD1 = p1a.x;
        c0 = d0;
        c1 = d1;
        w += D;
        vo += Db;
        bo ^= kMarchPipeBuf;
      }
    }
    return;
  }
  if constexpr (DOWN)
  {
    // one row's sum: the seven products in ascending-offset order; the +D product comes in already rounded
    // (carried from the plane above, where both its factors were at hand: two registers per row less than
    // carrying the factors, which is what keeps every load of a plane in flight at 5 waves per SIMD)
    auto row = [&](double amD, double vmD, double an, double vn, double am, double vl, double a0, double vc, double a1,
                   double vr, double aq, double vq, double prodD) {
      double acc = 0.0;
      acc += amD * vmD;
      acc += an * vn;
      acc += am * vl;
      acc += a0 * vc;
      acc += a1 * vr;
      acc += aq * vq;
      acc += prodD;
      return acc;
    };
    w += (z1 - 1 - z0) * D;
    vo = (unsigned)w * SZ;
    const bool above = z1 + mp.gz0 < mp.gz;  // plane z1 exists globally: the top plane's +D operands
    raw pu0{}, pu1{};
    if (above)
    {
      bload(rs, vo + Db, pu0);
      bload(rs, vo + nxb + Db, pu1);
    }
    const dpair p0a = (mp.cache & 2) ? P01[w] : __builtin_nontemporal_load(P01 + w);
    const dpair p1a = (mp.cache & 2) ? P01[w + gx] : __builtin_nontemporal_load(P01 + w + gx);
    raw c0, c1;
    bload(rs, vo, c0);
    bload(rs, vo + nxb, c1);
    if (!pre(x)) return;
    // carried: the plane's diagonal values and its +D products a(w, w + D) u(w + D)
    double a00 = p0a.y, a01 = p1a.y;
    double pD0 = p0a.x * (above ? x.val(pu0) : 0.0), pD1 = p1a.x * (above ? x.val(pu1) : 0.0);
    // one plane; BELOW: the plane below exists globally (global plane 0 is peeled off the loop, so the loop
    // body has no branch that depends on the plane: there the -D operands come through the zero-record
    // descriptor and the (+D, 0) pairs of the plane below are exact zeros, not loaded)
    auto plane = [&](auto below_c) {
      constexpr bool below = decltype(below_c)::value;
      // the HBM streams first (the -D operands open each row's sum), ahead of the branches of the masked
      // edge loads: issued after them the compiler placed them behind a full wait, two round trips per plane
      raw eg0, eg1, xn0, xq1, m0, m1;
      bload(below ? rs : r0, vo - Db, m0);
      bload(below ? rs : r0, vo + nxb - Db, m1);
      dpair q0a = dpair{0.0, 0.0}, q1a = dpair{0.0, 0.0};
      if constexpr (below)
      {
        q0a = (mp.cache & 2) ? P01[w - D] : __builtin_nontemporal_load(P01 + w - D);
        q1a = (mp.cache & 2) ? P01[w + gx - D] : __builtin_nontemporal_load(P01 + w + gx - D);
      }
      const dpair p0b = P23[w], p1b = P23[w + gx];
      bload(rs, vo + eoff, eg0);
      bload(rs, vo + nxb + eoff, eg1);
      bload(rn, vo + dnb, xn0);
      bload(rq, vo + nxb + dqb, xq1);
      const double an0 = has_n ? P23[w + mp.dn].y : 0.0;
      const double ae0 = le ? P23[w - 1].x : 0.0, ae1 = le ? P23[w + gx - 1].x : 0.0;
      const double vc0 = x.val(c0), vc1 = x.val(c1);
      const double ve0 = x.val(eg0), ve1 = x.val(eg1);
      const double acc0 = row(q0a.x, x.val(m0), an0, x.val(xn0), lane_shift_or<false>(p0b.x, ae0),
                              lane_shift_or<false>(vc0, ve0), a00, vc0, p0b.x, lane_shift_or<true>(vc0, ve0), p0b.y,
                              vc1, pD0);
      const double acc1 = row(q1a.x, x.val(m1), p0b.y, vc0, lane_shift_or<false>(p1b.x, ae1),
                              lane_shift_or<false>(vc1, ve1), a01, vc1, p1b.x, lane_shift_or<true>(vc1, ve1), p1b.y,
                              x.val(xq1), pD1);
      epi(w - own32, w, acc0, c0);
      epi(w + gx - own32, w + gx, acc1, c1);
      // the plane below: its +D entry times this plane's operand, its diagonal, its centres
      pD0 = q0a.x * vc0;
      pD1 = q1a.x * vc1;
      a00 = q0a.y;
      a01 = q1a.y;
      c0 = m0;
      c1 = m1;
      w -= D;
      vo -= Db;
    };
    const bool floor0 = zg0 == 0;  // the run ends on global plane 0
    for (int z = z1 - 1; z >= z0 + (floor0 ? 1 : 0); --z) plane(std::true_type{});
    if (floor0) plane(std::false_type{});
    return;
  }
  double amD0 = 0.0, amD1 = 0.0;
  raw pm0{}, pm1{};
  if (zg0 > 0)
  {
    bload(rs, vo - Db, pm0);
    bload(rs, vo + nxb - Db, pm1);
    amD0 = P01[w - D].x;
    amD1 = P01[w + gx - D].x;
  }
  raw c0, c1;
  bload(rs, vo, c0);
  bload(rs, vo + nxb, c1);
  if (!pre(x)) return;
  double pmv0 = zg0 > 0 ? x.val(pm0) : 0.0, pmv1 = zg0 > 0 ? x.val(pm1) : 0.0;
  for (int z = z0; z < z1; ++z)
  {
    const int zg = z + mp.gz0;
    raw eg0, eg1, xn0, xq1, d0, d1;
    bload(rs, vo + eoff, eg0);
    bload(rs, vo + nxb + eoff, eg1);
    bload(rn, vo + dnb, xn0);
    bload(rq, vo + nxb + dqb, xq1);
    const dpair p0a = (mp.cache & 2) ? P01[w] : __builtin_nontemporal_load(P01 + w), p0b = P23[w];
    const dpair p1a = (mp.cache & 2) ? P01[w + gx] : __builtin_nontemporal_load(P01 + w + gx), p1b = P23[w + gx];
    const double an0 = has_n ? P23[w + mp.dn].y : 0.0;
    const double ae0 = le ? P23[w - 1].x : 0.0, ae1 = le ? P23[w + gx - 1].x : 0.0;
    const __amdgpu_buffer_rsrc_t rd = zg + 1 < mp.gz ? rs : r0;
    bload(rd, vo + Db, d0);
    bload(rd, vo + nxb + Db, d1);
    const double vc0 = x.val(c0), vc1 = x.val(c1);
    double acc0 = 0.0, acc1 = 0.0;
    {
      const double ve = x.val(eg0);
      const double vl = lane_shift_or<false>(vc0, ve), vr = lane_shift_or<true>(vc0, ve);
      const double am = lane_shift_or<false>(p0b.x, ae0);
      acc0 += amD0 * pmv0;
      acc0 += an0 * x.val(xn0);
      acc0 += am * vl;
      acc0 += p0a.y * vc0;
      acc0 += p0b.x * vr;
      acc0 += p0b.y * vc1;  // +nx: line y0 + 1's centre
      acc0 += p0a.x * x.val(d0);
    }
    {
      const double ve = x.val(eg1);
      const double vl = lane_shift_or<false>(vc1, ve), vr = lane_shift_or<true>(vc1, ve);
      const double am = lane_shift_or<false>(p1b.x, ae1);
      acc1 += amD1 * pmv1;
      acc1 += p0b.y * vc0;  // -nx: line y0's centre, mirrored value = line y0's +nx entry
      acc1 += am * vl;
      acc1 += p1a.y * vc1;
      acc1 += p1b.x * vr;
      acc1 += p1b.y * x.val(xq1);
      acc1 += p1a.x * x.val(d1);
    }
    epi(w - own32, w, acc0, c0);
    epi(w + gx - own32, w + gx, acc1, c1);
    pmv0 = vc0;
    pmv1 = vc1;
    amD0 = p0a.x;
    amD1 = p1a.x;
    c0 = d0;
    c1 = d1;
    w += D;
    vo += Db;
  }
}

// Box march for the P1 Kuhn 15-point stencil (march variant 12; config C5's K and M, any values): the
// band's offsets are a D + b nx + c with (a, b, c) in the Kuhn edge set {0, +-e_i, +-(e_i + e_j),
// +-(1, 1, 1)} and every row stores exactly its in-grid neighbours among them (eig_mat_s::sym_box27,
// checked at upload).  A wave owns 64 consecutive x of one grid line (nx a multiple of 64) and marches
// z, keeping the operand lines it needs in registers as values x.val (the fused step's u_k):
//   plane z - 1: lines y - 1, y        plane z: y - 1, y, y + 1        plane z + 1: y, y + 1
// each line with one edge register (lane 0: the row at x0 - 1, lane 63: x0 + 64; DPP lane shifts take
// it as the "old" operand).  Per plane only plane z + 1's three lines are loaded (y: the stream, y +- 1:
// gathers the neighbouring columns streamed, L2 hits); the rest are carried (z + 1 -> z -> z - 1).
// Values: the row's 8 upper band arrays streamed once (0, +1, +nx, +nx+1, +D, +D+1, +D+nx, +D+nx+1);
// the mirrored lower entries from the rows below: -1 by the lane shift of the +1 stream, -D / -D-1
// carried from the previous plane's +D / +D+1 streams, -nx / -nx-1 / -D-nx / -D-nx-1 gathered at line
// y - 1 (planes z and z - 1).  Missing neighbours read as exact zeros (zero-record descriptors for
// lines / planes outside the grid, out-of-range edge offsets at x = 0 / nx - 1), so each row sums its
// stored entries in ascending-column order bit for bit as the reference row loop.
// KP (march variant 16): the values from the Kuhn pack (mp.pack: four arrays of value pairs (0, +1),
// (+nx, +nx+1), (+D, +D+1), (+D+nx, +D+nx+1) per window row -- 4 instead of 8 16-B/8-B streams and
// 2 instead of 4 gathers) through 64-bit global addresses, lane 0's edge values by exec-masked loads.
// LX (march variant 20, the pack): a workgroup's 4 waves march the SAME 64 x of 4 consecutive lines
// y0 .. y0 + 3 (instead of 4 x-runs of one line), and every line a wave streams -- its operand line of
// plane z + 1 and its pack pairs (+nx, +nx+1) of plane z and (+D+nx, +D+nx+1) of plane z - 1 -- goes
// through LDS to the waves of lines y +- 1 (double-buffered, one barrier per plane): only lines
// y0 - 1 and y0 + 4 are still gathered from L2, 2 of the 8 line gathers per plane of the workgroup
// (the gathers that miss L2 were the Kuhn step's 1.32x read excess, profiles/r04af_kuhn_*).  Lines
// per grid a multiple of 4; the same products in the same order as variant 16 (bitwise).
template <bool KP, bool LX, class X, class EPI, class PRE>
__device__ __forceinline__ void march_rows_kuhn(const SellB1 &A, const MarchPlan &mp, i64 own, int lane, int wave,
                                                X x, EPI &epi, PRE &pre)
{
  typedef typename X::raw raw;
  constexpr unsigned SZ = sizeof(raw);
  constexpr unsigned kOut = 0x80000000u;
  const int D = (int)mp.D, own32 = (int)own, gx = mp.gx;
  int col, seg;
  if constexpr (LX)
  {
    // workgroup -> (x run, group of 4 lines, plane run); workgroup-uniform, so every wave of it reaches
    // the same barriers
    const int nxc = gx / 64, per = nxc * (mp.gy / 4);
    const int wg = (int)swizzled_block();
    if (wg >= per * mp.nseg) return;
    seg = wg / per;
    const int r = wg % per;
    col = ((r / nxc) * 4 + wave) * nxc + r % nxc;
  }
  else
  {
    const int item = (int)swizzled_block() * kWaves + wave;
    if (item >= mp.ncol * mp.nseg) return;
    col = item % mp.ncol;
    seg = item / mp.ncol;
  }
  const int z0 = (int)(mp.zb + seg * mp.nplanes / mp.nseg), z1 = (int)(mp.zb + (seg + 1) * mp.nplanes / mp.nseg);
  const unsigned nbytes = (unsigned)(A.xlast + 1) * SZ;
  const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(x.ptr()), 0, (int)nbytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t r0 = __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(x.ptr()), 0, 0, 0x00020000);
  const int x0 = (col * 64) % gx, yw = (col * 64) / gx;
  const __amdgpu_buffer_rsrc_t rm = yw > 0 ? rs : r0, rp = yw < mp.gy - 1 ? rs : r0;  // lines y - 1, y + 1
  const unsigned eoff = lane == 0 ? (x0 > 0 ? 0u - SZ : kOut) : lane == 63 ? (x0 + 64 < gx ? SZ : kOut) : kOut;
  const unsigned nxb = (unsigned)gx * SZ, Db = (unsigned)D * SZ;
  int w = own32 + col * 64 + lane + z0 * D;
  unsigned vo = (unsigned)w * SZ;
  const int zg0 = z0 + mp.gz0;
  // value arrays (8-B window-indexed slots): one descriptor per upper array, zero-record where absent
  const SymImg &S = A.sym;
  const unsigned vbytes = (unsigned)S.ld * 8u;
  auto arr = [&](int pos, bool on) {
    const int j = mp.kj[pos];
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<double *>(S.val + (i64)(j >= 0 ? j : 0) * S.ld), 0,
                                             on && j >= 0 ? (int)vbytes : 0, 0x00020000);
  };
  const __amdgpu_buffer_rsrc_t a0d = arr(13, true), a1d = arr(14, true), aNd = arr(16, true), aN1d = arr(17, true),
                               aDd = arr(22, true), aD1d = arr(23, true), aDNd = arr(25, true), aDN1d = arr(26, true),
                               aNm = arr(16, yw > 0), aN1m = arr(17, yw > 0), vz = arr(13, false);
  const unsigned eov = lane == 0 && x0 > 0 ? 0u - 8u : kOut;  // lane 0: the value slot at x0 - 1
  const unsigned nxv = (unsigned)gx * 8u, Dv = (unsigned)D * 8u;
  unsigned vv = (unsigned)w * 8u;
  auto ld8 = [&](__amdgpu_buffer_rsrc_t r, unsigned o) {
    return __builtin_bit_cast(double, __builtin_amdgcn_raw_buffer_load_b64(r, (int)o, 0, 0));
  };
  auto ld8nt = [&](__amdgpu_buffer_rsrc_t r, unsigned o) {  // once-read streams: nontemporal
    return __builtin_bit_cast(double, __builtin_amdgcn_raw_buffer_load_b64(r, (int)o, 0, 2));
  };
  // operand lines: raw loads first (the fused prologue sets x.c meanwhile), values after
  const bool below = zg0 > 0;
  raw rAm, rAme, rA0, rA0e, rBm, rBme, rB0, rB0e, rBp, rBpe;
  {
    const __amdgpu_buffer_rsrc_t p0 = below ? rs : r0, pm = below ? rm : r0;
    bload(pm, vo - Db - nxb, rAm);
    bload(pm, vo - Db - nxb + eoff, rAme);
    bload(p0, vo - Db, rA0);
    bload(p0, vo - Db + eoff, rA0e);
  }
  bload(rm, vo - nxb, rBm);
  bload(rm, vo - nxb + eoff, rBme);
  bload(rs, vo, rB0);
  bload(rs, vo + eoff, rB0e);
  bload(rp, vo + nxb, rBp);
  bload(rp, vo + nxb + eoff, rBpe);
  // Kuhn pack: array q of pairs at byte 16 (q ld + w), one descriptor (32-bit offsets)
  const __amdgpu_buffer_rsrc_t kp = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<double *>(KP && mp.pack ? mp.pack : S.val), 0, KP && mp.pack ? (int)(8u * vbytes) : 0, 0x00020000);
  const unsigned kq = 2u * vbytes;  // bytes per pair array
  auto kl = [&](int q, unsigned row_off) {  // pair of array q at byte offset row_off (= 16 row)
    return __builtin_bit_cast(dpair, __builtin_amdgcn_raw_buffer_load_b128(kp, (int)(row_off + (unsigned)q * kq), 0, 0));
  };
  auto kle = [&](int q, unsigned row_off, bool on) {  // lane 0's edge value (.y); others: out of range
    const unsigned o = on ? row_off + (unsigned)q * kq + 8u : kOut;
    return __builtin_bit_cast(double, __builtin_amdgcn_raw_buffer_load_b64(kp, (int)o, 0, 0));
  };
  // the once-read pair streams (0, +1) and (+D, +D+1): default cache policy.  Measured against
  // nontemporal loads at 256^3 (P1 K, profiles/r04v_p1k.jsonl, r04w_p1k.jsonl): fused step 336.0 vs
  // 340.1 us and 337.0 vs 349.2 us on two boxes, eig_mv 282.9 vs 285.9 us -- although FETCH_SIZE
  // rises (100.7 vs 97.6 B per row; why the default policy is faster is not established)
  auto klnt = [&](int q, unsigned row_off) {
    return __builtin_bit_cast(dpair, __builtin_amdgcn_raw_buffer_load_b128(kp, (int)(row_off + (unsigned)q * kq), 0, 0));
  };
  const unsigned nxk = 2u * nxv, Dk = 2u * Dv;
  const bool le = lane == 0 && x0 > 0;  // lane 0's value edge (row x0 - 1) exists
  double aDp = 0.0, aD1p = 0.0, aD1pe = 0.0;
  if constexpr (KP)
  {
    if (below)
    {
      const dpair k2 = kl(2, 2u * vv - Dk);
      aDp = k2.x;
      aD1p = k2.y;
      aD1pe = kle(2, 2u * vv - Dk - 16u, le);
    }
  }
  else
  {
    aDp = below ? ld8(aDd, vv - Dv) : 0.0;
    aD1p = below ? ld8(aD1d, vv - Dv) : 0.0;
    aD1pe = below ? ld8(aD1d, vv - Dv + eov) : 0.0;
  }
  // LX: the line exchange (raw operand line of plane z + 1, pack pairs (+nx, +nx+1) of plane z and
  // (+D+nx, +D+nx+1) of plane z - 1 per wave), double-buffered by plane parity
  __shared__ raw lx_c[LX ? 2 : 1][LX ? kWaves : 1][64];
  __shared__ dpair lx_k1[LX ? 2 : 1][LX ? kWaves : 1][64], lx_k3[LX ? 2 : 1][LX ? kWaves : 1][64];
  const bool lx_lo = LX && wave > 0, lx_hi = LX && wave < kWaves - 1;  // line y - 1 / y + 1 in this workgroup
  dpair k3prev = {0.0, 0.0};  // LX: this line's (+D+nx, +D+nx+1) pair of the previous plane
  if constexpr (LX && KP)
  {
    if (below) k3prev = kl(3, 2u * vv - Dk);
  }
  if (!pre(x)) return;
  double Am = x.val(rAm), Ame = x.val(rAme), A0 = x.val(rA0), A0e = x.val(rA0e), Bm = x.val(rBm), Bme = x.val(rBme),
         Bp = x.val(rBp), Bpe = x.val(rBpe);
  double B0 = x.val(rB0), B0e = x.val(rB0e);
  raw pB0 = rB0;
  for (int z = z0; z < z1; ++z)
  {
    const int zg = z + mp.gz0;
    const bool up = zg + 1 < mp.gz, dn = zg > 0;
    raw rC0, rC0e, rCp, rCpe, rCm, rCme;
    {
      const __amdgpu_buffer_rsrc_t q0 = up ? rs : r0, qp = up ? rp : r0, qm = up ? rm : r0;
      bload(q0, vo + Db, rC0);
      bload(q0, vo + Db + eoff, rC0e);
      if (!lx_hi) bload(qp, vo + Db + nxb, rCp);
      bload(qp, vo + Db + nxb + eoff, rCpe);
      if (!lx_lo) bload(qm, vo + Db - nxb, rCm);
      bload(qm, vo + Db - nxb + eoff, rCme);
    }
    // the row's upper values (once-read streams nontemporal; +nx.. arrays are re-read by line y + 1)
    double a0, a1, aN, aN1, aD, aD1, aDN, aDN1, a1e = 0.0, aD1e = 0.0;
    double aNl = 0.0, aN1l = 0.0, aN1le = 0.0, aDNl = 0.0, aDN1l = 0.0, aDN1le = 0.0;
    if constexpr (KP)
    {
      const unsigned ko = 2u * vv;
      const dpair k0 = klnt(0, ko), k1 = kl(1, ko), k2 = klnt(2, ko), k3 = kl(3, ko);
      a0 = k0.x, a1 = k0.y, aN = k1.x, aN1 = k1.y, aD = k2.x, aD1 = k2.y, aDN = k3.x, aDN1 = k3.y;
      a1e = kle(0, ko - 16u, le);
      aD1e = kle(2, ko - 16u, le);
      // mirrored lower entries at line y - 1 (plane z: -nx, -nx-1; plane z - 1: -D-nx, -D-nx-1): the
      // wave-uniform line / plane conditions pick an out-of-range offset (zeros, no traffic)
      const bool ym = yw > 0, dm = dn && yw > 0;
      dpair kn = {0.0, 0.0}, kd = {0.0, 0.0};
      if (!lx_lo)
      {
        kn = __builtin_bit_cast(dpair,
                                __builtin_amdgcn_raw_buffer_load_b128(kp, (int)(ym ? ko - nxk + kq : kOut), 0, 0));
        kd = __builtin_bit_cast(
            dpair, __builtin_amdgcn_raw_buffer_load_b128(kp, (int)(dm ? ko - Dk - nxk + 3u * kq : kOut), 0, 0));
      }
      aN1le = kle(1, ko - nxk - 16u, le && ym);
      aDN1le = kle(3, ko - Dk - nxk - 16u, le && dm);
      if constexpr (LX)
      {
        // this wave's lines to the workgroup, then the neighbours' from it
        const int b = z & 1;
        lx_c[b][wave][lane] = rC0;
        lx_k1[b][wave][lane] = k1;
        lx_k3[b][wave][lane] = k3prev;
        k3prev = k3;
        __syncthreads();
        if (lx_hi) rCp = lx_c[b][wave + 1][lane];
        if (lx_lo)
        {
          rCm = lx_c[b][wave - 1][lane];
          kn = lx_k1[b][wave - 1][lane];
          kd = dn ? lx_k3[b][wave - 1][lane] : dpair{0.0, 0.0};
        }
      }
      aNl = kn.x, aN1l = kn.y;
      aDNl = kd.x, aDN1l = kd.y;
    }
    else
    {
      a0 = ld8nt(a0d, vv), a1 = ld8nt(a1d, vv), aN = ld8(aNd, vv), aN1 = ld8(aN1d, vv);
      aD = ld8nt(aDd, vv), aD1 = ld8nt(aD1d, vv), aDN = ld8(aDNd, vv), aDN1 = ld8(aDN1d, vv);
      a1e = ld8(a1d, vv + eov), aD1e = ld8(aD1d, vv + eov);
      // mirrored lower entries at line y - 1 (plane z: -nx, -nx-1; plane z - 1: -D-nx, -D-nx-1)
      aNl = ld8(aNm, vv - nxv), aN1l = ld8(aN1m, vv - nxv), aN1le = ld8(aN1m, vv - nxv + eov);
      const __amdgpu_buffer_rsrc_t dnm = dn && yw > 0 ? aDNd : vz, dn1m = dn && yw > 0 ? aDN1d : vz;
      aDNl = ld8(dnm, vv - Dv - nxv), aDN1l = ld8(dn1m, vv - Dv - nxv), aDN1le = ld8(dn1m, vv - Dv - nxv + eov);
    }
    const double C0 = x.val(rC0), C0e = x.val(rC0e), Cp = x.val(rCp), Cpe = x.val(rCpe);
    double acc = 0.0;
    acc += lane_shift_or<false>(aDN1l, aDN1le) * lane_shift_or<false>(Am, Ame);  // (-1, -1, -1)
    acc += aDNl * Am;                                                            // (-1, -1,  0)
    acc += lane_shift_or<false>(aD1p, aD1pe) * lane_shift_or<false>(A0, A0e);    // (-1,  0, -1)
    acc += aDp * A0;                                                             // (-1,  0,  0)
    acc += lane_shift_or<false>(aN1l, aN1le) * lane_shift_or<false>(Bm, Bme);    // ( 0, -1, -1)
    acc += aNl * Bm;                                                             // ( 0, -1,  0)
    acc += lane_shift_or<false>(a1, a1e) * lane_shift_or<false>(B0, B0e);        // ( 0,  0, -1)
    acc += a0 * B0;                                                              // ( 0,  0,  0)
    acc += a1 * lane_shift_or<true>(B0, B0e);                                    // ( 0,  0, +1)
    acc += aN * Bp;                                                              // ( 0, +1,  0)
    acc += aN1 * lane_shift_or<true>(Bp, Bpe);                                   // ( 0, +1, +1)
    acc += aD * C0;                                                              // (+1,  0,  0)
    acc += aD1 * lane_shift_or<true>(C0, C0e);                                   // (+1,  0, +1)
    acc += aDN * Cp;                                                             // (+1, +1,  0)
    acc += aDN1 * lane_shift_or<true>(Cp, Cpe);                                  // (+1, +1, +1)
    epi(w - own32, w, acc, pB0);
    // carry z + 1 -> z -> z - 1
    Am = Bm, Ame = Bme, A0 = B0, A0e = B0e;
    Bm = x.val(rCm), Bme = x.val(rCme);
    B0 = C0, B0e = C0e, pB0 = rC0;
    Bp = Cp, Bpe = Cpe;
    aDp = aD, aD1p = aD1, aD1pe = aD1e;
    w += D;
    vo += Db;
    vv += Dv;
  }
}

// A variant's traits as namespace-scope constants for the kernels below (a local constexpr copy
// would be one more stack object in each kernel before optimisation)
template <int UNI>
constexpr MarchTraits kTraits = march_traits(UNI);
template <int UNI>
constexpr bool kWholePlanes = kTraits<UNI>.whole_planes();
template <int UNI>
constexpr bool kUniformValues = kTraits<UNI>.values == kMarchUniform;
template <int UNI>
constexpr bool kMarchDownBody = kTraits<UNI>.down_body;
template <int UNI>
constexpr bool kMarchPipeBody = kTraits<UNI>.pipe_body;

// The rows of this wave's work item, in plane order: epi(r, w, acc, centre) gets each row's sum
// and its own operand x[w] (raw: a double, or the (t, u) pair of the fused step).
// The first entry of both far spans is issued with the row's streams, so a 7-point row waits
// once.  SPAN1: each far span holds at most one offset (3-D 7-point, 2-D 5-point), so the generic
// span loops are compiled out.  (Measured and dropped: issuing the far spans offset group by
// offset group after the near math; prefetching the next plane's streams, or its far-span
// operands, one iteration ahead -- both spill in the fused kernel and gave nothing in the others;
// y-line workgroup grouping with a barrier per plane; temporal result stores.)
// UNI (uniform band, SPAN1 only): the band values come from the plan's constants -- the values the
// arrays hold at every slot the mask admits -- so only the row mask and the operands are streamed;
// the same products and sums in the same order, bit for bit.  (Measured and dropped for UNI: issuing
// plane z + 1's mask / gathers / edge operand before plane z's arithmetic -- 256^3 fused step 145 vs
// 137 us at the 7 waves / SIMD it needs, 128^3 28.0 vs 30.7: profiles/r03bc_latency.jsonl.)
template <class MT, int KC, bool SPAN1, int UNI, class X, class EPI, class PRE = MarchNoPre>
__device__ __forceinline__ void march_rows(const SellB1 &A, const MarchPlan &mp, i64 own, int lane, int wave,
                                           const X &x, EPI &epi, PRE &&pre = PRE{})
{
  static_assert(kTraits<UNI>.valid, "not a march variant (march_variants.h)");
  static_assert(kTraits<UNI>.any_head() ||
                    (SPAN1 == kTraits<UNI>.span1() && (int)sizeof(MT) == kTraits<UNI>.mask_bytes()),
                "march variant instantiated with another template head than its traits name");
  if constexpr (kTraits<UNI>.family == kMarchKuhn)
  {
    march_rows_kuhn<kTraits<UNI>.kp, kTraits<UNI>.lx>(A, mp, own, lane, wave, x, epi, pre);
    return;
  }
  else if constexpr (kTraits<UNI>.family == kMarchGeo2L2)
  {
    // the pipelined bodies: the fused step (the pair vector) of the variants kept at 96 registers
    if constexpr (kMarchPipeBody<UNI> && std::is_same<X, XPair>::value)
      if (mp.pipe)
      {
        if (mp.down)
          march_rows_geo2_2l<true, true>(A, mp, own, lane, wave, x, epi, pre);
        else
          march_rows_geo2_2l<false, true>(A, mp, own, lane, wave, x, epi, pre);
        return;
      }
    if constexpr (kMarchDownBody<UNI>)
      if (mp.down)
      {
        march_rows_geo2_2l<true>(A, mp, own, lane, wave, x, epi, pre);
        return;
      }
    march_rows_geo2_2l<false>(A, mp, own, lane, wave, x, epi, pre);
    return;
  }
  else if constexpr (kTraits<UNI>.family == kMarchGeo2)
  {
    march_rows_geo2<kTraits<UNI>.pf, kTraits<UNI>.pg, kTraits<UNI>.val>(A, mp, own, lane, wave, x, epi, pre);
    return;
  }
  else if constexpr (kTraits<UNI>.family == kMarchGeo)
  {
    march_rows_geo<kTraits<UNI>.pf, kTraits<UNI>.pg>(A, mp, own, lane, wave, x, epi);
    return;
  }
  constexpr bool GEO = kTraits<UNI>.geo_masks;
  typedef typename X::raw raw;
  // 32-bit row / window indices (window < 2^31, enforced at upload) keep the address math short
  const SymImg &S = A.sym;
  const int xl = (int)A.xlast, D = (int)mp.D, ldl = (int)(S.ld - 1), own32 = (int)own, mrows = (int)mp.mrows;
  const int nd = S.nd;
  const double *UD = S.val + (i64)S.dj[nd - 1] * S.ld;
  const double *U1 = S.val + (i64)S.j1 * S.ld;
  const double *U0 = S.val + (i64)(S.j0 >= 0 ? S.j0 : 0) * S.ld;
  const MT *mask = static_cast<const MT *>(S.mask);
  const int item = (int)swizzled_block() * kWaves + wave;
  if (item >= mp.ncol * mp.nseg) return;
  const int col = item % mp.ncol, seg = item / mp.ncol;
  const int z0 = (int)(mp.zb + seg * mp.nplanes / mp.nseg), z1 = (int)(mp.zb + (seg + 1) * mp.nplanes / mp.nseg);
  auto cx = [&](int g) -> unsigned { return g < 0 ? 0u : (unsigned)(g > xl ? xl : g); };
  auto cv = [&](int g) -> unsigned { return g < 0 ? 0u : (unsigned)(g > ldl ? ldl : g); };
  const int kn0 = 1, kn1 = S.klo, kp0 = S.khi, kp1 = nd - 1;  // far spans (-D, -1) and (+1, +D)
  // GEO: the lane's row keeps its (x, y) in every plane; bit k of the mask = the neighbour at
  // off[k] lies in the grid (verified row by row at upload)
  unsigned gxy = 0;
  if constexpr (GEO)
  {
    const int pr = col * 64 + lane, gxc = pr % mp.gx, gyc = pr / mp.gx;
    // offsets ascending: -D, (-nx), -1, 0, +1, (+nx), +D -- the far-span bits only when present
    unsigned b = 0;
    int k = 1;
    if (mp.dn) b |= (gyc > 0 ? 1u : 0u) << k++;
    b |= (gxc > 0 ? 1u : 0u) << k++;
    b |= 1u << k++;
    b |= (gxc < mp.gx - 1 ? 1u : 0u) << k++;
    if (mp.dq) b |= (gyc < mp.gy - 1 ? 1u : 0u) << k++;
    gxy = b;
  }
  struct Stream {
    unsigned m;
    double aD, a0, ap;
    raw pD;
  };
  // streams read exactly once (the row mask, the 0 / +1 / +D band values): nontemporal loads keep
  // them from evicting the (t, u) / band lines the neighbouring columns re-read from L2
  auto ld1 = [&](const double *p, unsigned i) { return __builtin_nontemporal_load(p + i); };
  auto load_stream = [&](int w, int z, Stream &st) {
    const int r = w - own32;
    const unsigned wv = (unsigned)(w > ldl ? ldl : w);
    if constexpr (GEO)
    {
      const int zg = z + mp.gz0;  // (z: the wave's plane on this rank)
      st.m = gxy | (zg > 0 ? 1u : 0u) | (zg < mp.gz - 1 ? 1u << kp1 : 0u);
    }
    else
      st.m = r < mrows ? (unsigned)__builtin_nontemporal_load(mask + (unsigned)r) : 0u;
    st.pD = x.load(cx(w + D));
    if constexpr (kUniformValues<UNI>)
    {
      st.aD = mp.cD;
      st.a0 = mp.c0;
      st.ap = mp.c1;
    }
    else
    {
      st.aD = ld1(UD, wv);
      st.a0 = S.j0 >= 0 ? ld1(U0, wv) : 0.0;
      st.ap = ld1(U1, wv);
    }
  };
  // carried operands: the -D operand (as its value x.val), its mirrored matrix entry, the centre
  int w = own32 + col * 64 + lane + z0 * D;
  double pmv = x.val(x.load(cx(w - D)));
  double amD = kUniformValues<UNI> ? mp.cD : UD[cv(w - D)];
  raw pcur = x.load(cx(w));
  Stream cur;
  const bool edge = lane == 0 || lane == 63;
  for (int z = z0; z < z1; ++z, w += D)
  {
    const int r = w - own32;
    const unsigned wv = (unsigned)(w > ldl ? ldl : w);
    load_stream(w, z, cur);
    // lanes 0 / 63: the row across the wave edge (one load for both), and lane 0's mirrored -1 entry
    raw eg;
    double ae = 0.0;
    if (edge) eg = x.load(cx(lane == 0 ? w - 1 : w + 1));
    if (lane == 0) ae = kUniformValues<UNI> ? mp.c1 : U1[cv(w - 1)];
    double an = 0.0, aq = 0.0;
    raw xn, xq;
    if (mp.dn)
    {
      const unsigned g = cx(w + mp.dn);  // (negative offset: the mirrored slot at the gathered row)
      an = kUniformValues<UNI> ? mp.cn : mp.Un[g];
      xn = x.load(g);
    }
    if (mp.dq)
    {
      aq = kUniformValues<UNI> ? mp.cq : mp.Uq[wv];
      xq = x.load(cx(w + mp.dq));
    }
    const unsigned m = cur.m;
    double acc = 0.0;
    if (m & 1u) acc += amD * pmv;
    if (mp.dn && ((m >> kn0) & 1u)) acc += an * x.val(xn);
    if (!SPAN1) sym_span<KC>(S, kn0 + 1, kn1, m, w, wv, x, xl, acc);
    // neighbours' operand VALUES shifted across lanes (x.val per lane, then moved: the same bits
    // as evaluating x.val on the shifted raw operand, at half the registers for pairs)
    const double vc = x.val(pcur);
    double vl = lane_shift<false>(vc), vr = lane_shift<true>(vc);
    double am = lane_shift<false>(cur.ap);
    if (edge)
    {
      const double ve = x.val(eg);
      if (lane == 0)
      {
        vl = ve;
        am = ae;
      }
      else
        vr = ve;
    }
    if (S.km1 >= 0 && ((m >> S.km1) & 1u)) acc += am * vl;
    if (S.k0 >= 0 && ((m >> S.k0) & 1u)) acc += cur.a0 * vc;
    if (S.kp1 >= 0 && ((m >> S.kp1) & 1u)) acc += cur.ap * vr;
    if (mp.dq && ((m >> kp0) & 1u)) acc += aq * x.val(xq);
    if (!SPAN1) sym_span<KC>(S, kp0 + 1, kp1, m, w, wv, x, xl, acc);
    if ((m >> kp1) & 1u) acc += cur.aD * x.val(cur.pD);
    epi(r, w, acc, pcur);
    pmv = vc;
    pcur = cur.pD;
    amD = cur.aD;
  }
}

// y[own + r] = (A x)[r] on the plane march (BCRSMatrix::mv; bitwise k_spmv_b1).
// resident waves per SIMD of the eig_mv / K1 march kernels (the box march holds ~90 VGPRs)
constexpr int march_mv_waves(int uni) { return march_traits(uni).mv_waves; }

template <class MT, bool SPAN1, int UNI>
__global__ __launch_bounds__(kStreamThreads, march_mv_waves(UNI)) void k_spmv_march(i64 nrows, i64 own, SellB1 A, MarchPlan mp,
                                                                  const double *__restrict__ x,
                                                                  double *__restrict__ y)
{
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  auto epi = [&](int r, int w, double acc, double) {
    if constexpr (kTraits<UNI>.geo2_path())
      march_store(mp, acc, y + (unsigned)w);  // (geometric: whole planes)
    else if (kWholePlanes<UNI> || r < nrows)
      __builtin_nontemporal_store(acc, y + (unsigned)w);
  };
  march_rows<MT, 2, SPAN1, UNI>(A, mp, own, lane, wave, XPlain{x}, epi);
}

// Classic Lanczos kernel 1 on the plane march (same per-row arithmetic as k_lanczos_spmv_b1; the
// row's own u_j is the march's centre operand).
template <class MT, bool SPAN1, int UNI>
__global__ __launch_bounds__(kStreamThreads, march_mv_waves(UNI)) void k_lanczos_spmv_march(
    i64 nrows, i64 own, SellB1 A, MarchPlan mp, const double *__restrict__ u, const double *__restrict__ up,
    double *__restrict__ t, int j, const double *__restrict__ nsum, double *__restrict__ dot_out,
    double *__restrict__ beta_out, double *partials, unsigned *ticket)
{
  __shared__ double tot[1];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const double beta = sqrt(nsum[j]);
  const double sig = 1.0 / beta;
  const double gam = (j > 0) ? beta * (1.0 / sqrt(nsum[j - 1])) : 0.0;
  double d = 0.0;
  auto epi = [&](int r, int w, double acc, double uv) {
    if (r < nrows)
    {
      double ti = acc * sig;
      if (j > 0) ti = ti - gam * up[(unsigned)w];
      __builtin_nontemporal_store(ti, t + (unsigned)w);
      d += ti * uv;
    }
  };
  march_rows<MT, 2, SPAN1, UNI>(A, mp, own, lane, wave, XPlain{u}, epi);
  double v[1] = {d};
  if (grid_sum<1, kStreamThreads>(v, partials, ticket, tot))
  {
    if (threadIdx.x == 0)
    {
      dot_out[0] = tot[0];
      if (beta_out) beta_out[0] = beta;
    }
  }
}

// Fused one-reduction step on the plane march (per-row arithmetic of k_lanczos_fused_b1).  A repair
// launch (fused_begin) takes the rows of the planes this launch marches.  Built for 7 waves / SIMD
// (72 VGPRs; at 8 the pair operands spill: -5 %).
// resident waves per SIMD the fused march kernels are built for (registers: no spills)
constexpr int march_fused_waves(int uni) { return march_traits(uni).fused_waves; }

template <class MT, bool SPAN1, int UNI>
__global__ __launch_bounds__(kStreamThreads, march_fused_waves(UNI)) void k_lanczos_fused_march(
    i64 nrows, i64 own, SellB1 A, MarchPlan mp, const dpair *__restrict__ P, dpair *__restrict__ Pout, FusedArgs fa,
    double *__restrict__ out, double *partials, unsigned *ticket)
{
  __shared__ double tot[3];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  double d = 0.0, q2 = 0.0, m2 = 0.0;
  if constexpr (kTraits<UNI>.geo2_path())
  {
    // geo2: the scalar prologue runs while the wave's first plane loads are in flight (the march
    // calls `pre` after issuing them); waves without a work item run it after the march returns
    FusedStep fs{};
    bool begun = false;
    auto epi = [&](int, int w, double acc, dpair pc) {
      const double uk = pc.x - fs.c * pc.y;
      double ti = (acc - fs.mu * uk) * fs.sig;
      if (fs.j > 0) ti = ti - fs.gam * pc.y;
      march_store(mp, dpair{ti, uk}, Pout + (unsigned)w);
      d += ti * uk;
      q2 += ti * ti;
      m2 += uk * uk;
    };
    auto pre = [&](XPair &x) {
      fs = fused_begin(fa);
      begun = true;
      x.c = fs.c;
      return fs.act == kFusedStep || fs.act == kFusedPost;
    };
    march_rows<MT, 2, SPAN1, UNI>(A, mp, own, lane, wave, XPair{P, 0.0}, epi, pre);
    if (!begun) fs = fused_begin(fa);
    if (fs.act == kFusedHalt || fs.act == kFusedNoop)
    {
      if (!(fa.xch & kXchPublish))
      {
        fused_idle(out);
        return;
      }
      d = q2 = m2 = 0.0;
    }
    if (fs.act == kFusedRepair)
    {
      const i64 r0 = mp.zb * mp.D, r1 = std::min<i64>(nrows, (mp.zb + mp.nplanes) * mp.D);
      m2 = fused_repair_rows(r0, r1, own, fs.c, P, Pout);
    }
    double v[3] = {d, q2, m2};
    fused_finish<8>(v, partials, ticket, tot, out, nullptr, fa);
    return;
  }
  const FusedStep fs = fused_begin(fa);
  if (fs.act == kFusedHalt || fs.act == kFusedNoop)
  {
    double z[3] = {0.0, 0.0, 0.0};
    if (fa.xch & kXchPublish) fused_finish<8>(z, partials, ticket, tot, out, nullptr, fa);
    else fused_idle(out);
    return;
  }
  const double c = fs.c, gam = fs.gam, sig = fs.sig, mu = fs.mu;
  const int k = fs.j;
  if (fs.act == kFusedRepair)
  {
    const i64 r0 = mp.zb * mp.D, r1 = std::min<i64>(nrows, (mp.zb + mp.nplanes) * mp.D);
    m2 = fused_repair_rows(r0, r1, own, c, P, Pout);
  }
  else
  {
    auto epi = [&](int r, int w, double acc, dpair pc) {
      if (kWholePlanes<UNI> || r < nrows)  // (geometric images cover whole planes: no row test)
      {
        const double uk = pc.x - c * pc.y;
        double ti = (acc - mu * uk) * sig;
        if (k > 0) ti = ti - gam * pc.y;
        __builtin_nontemporal_store(dpair{ti, uk}, Pout + (unsigned)w);
        d += ti * uk;
        q2 += ti * ti;
        m2 += uk * uk;
      }
    };
    march_rows<MT, 2, SPAN1, UNI>(A, mp, own, lane, wave, XPair{P, c}, epi);
  }
  double v[3] = {d, q2, m2};
  fused_finish<8>(v, partials, ticket, tot, out, nullptr, fa);
}

// ---------------------------------------------------------------------------------------------
// a2 SpMM Y = A X for one 8-column block of a MultiVector<double,8> (kernels_cpp.hh:626-657) on the
// band-image plane march.  Lane = (row rq = lane >> 2 of a 16-row wave column, column pair
// cp = lane & 3): every operand load of the wave reads 16 consecutive X rows = 1 KiB contiguous,
// the 4 lanes of a row share the row's band values and mask byte (one cache line per wave).  The
// wave marches its 16-row column through the planes like march_rows: the -D / centre operands are
// carried, the +D operand loaded once; the +-1 operands (and the mirrored -1 value) come from the
// lanes 4 apart by ds_bpermute (rows 0 / 15 of the wave load theirs); the +-N operands are L2 hits.
// Per column, each row sums its stored entries in ascending-column order with separately rounded
// products and sums: bitwise the reference loop.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ double lane_from(double v, int src_lane)
{
  const long long b = __double_as_longlong(v);
  const int lo = __builtin_amdgcn_ds_bpermute(src_lane << 2, (int)b);
  const int hi = __builtin_amdgcn_ds_bpermute(src_lane << 2, (int)(b >> 32));
  return __longlong_as_double(((long long)hi << 32) | (unsigned)lo);
}

// One column block per workgroup (blockIdx.y): sharing the band stream between 2 / 4 blocks measured
// equal / 6 % slower (m = 32 at 256^3) -- the vector streams bound the launch.
// DOT: also dp[8 qb + j] = X_j . Y_j over the rows (StandardLargest's :84-85 in one launch): each
// lane adds its row's own operand x its result, one deterministic grid sum per column block
// (partials part + grid.x * 8 qb, ticket tick + qb kTicketStride); Y is unchanged.
// DOT = 2: also the window Gram of Y (one column block, m = 8: StandardLargest's next MGS starts from
// it, k_mgs_la_gram) -- dots and Gram in one two-level grid sum (reduce_dev.h quad_gram_block).
template <class MT, int DOT = 0>
__global__ __launch_bounds__(kStreamThreads, DOT == 2 ? 5 : DOT ? 6 : 8) void k_spmm8_march(i64 nrows, i64 own, i64 ld, SellB1 A,
                                                                   MarchPlan mp, const double *__restrict__ X,
                                                                   double *__restrict__ Y, double *dp = nullptr,
                                                                   double *part = nullptr, unsigned *tick = nullptr,
                                                                   double *gram = nullptr, unsigned *zero_word = nullptr)
{
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int qb = (int)blockIdx.y;  // column block
  const int rq = lane >> 2, cp = lane & 3;
  const SymImg &S = A.sym;
  const int xl = (int)A.xlast, D = (int)mp.D, ldl = (int)(S.ld - 1), own32 = (int)own, mrows = (int)mp.mrows;
  const int nd = S.nd;
  const double *UD = S.val + (i64)S.dj[nd - 1] * S.ld;
  const double *U1 = S.val + (i64)S.j1 * S.ld;
  const double *U0 = S.val + (i64)(S.j0 >= 0 ? S.j0 : 0) * S.ld;
  const MT *mask = static_cast<const MT *>(S.mask);
  const int item = (int)swizzled_block() * kWaves + wave;
  // (DOT: a wave past the last item joins the workgroup's reduction with an empty march)
  const bool live = item < mp.ncol * mp.nseg;
  if (!DOT && !live) return;
  const int col = item % mp.ncol, seg = item / mp.ncol;
  const int z0 = (int)(mp.zb + seg * mp.nplanes / mp.nseg);
  const int z1 = live ? (int)(mp.zb + (seg + 1) * mp.nplanes / mp.nseg) : z0;
  dpair dsum{0.0, 0.0};
  double gacc[2][8] = {};  // DOT == 2: this lane's share of the window Gram
  // column block qb, column pair cp: row g's operand at Xb[g]
  const dpair *Xb = reinterpret_cast<const dpair *>(X + (i64)qb * ld * 8) + cp;
  dpair *Yb = reinterpret_cast<dpair *>(Y + (i64)qb * ld * 8) + cp;
  auto xat = [&](int g) { return Xb[(unsigned)(g < 0 ? 0 : (g > xl ? xl : g)) * 4u]; };
  auto cv = [&](int g) -> unsigned { return g < 0 ? 0u : (unsigned)(g > ldl ? ldl : g); };
  auto fma2 = [](dpair acc, double a, dpair x) { return dpair{acc.x + a * x.x, acc.y + a * x.y}; };
  const int kn0 = 1, kn1 = S.klo, kp0 = S.khi, kp1 = nd - 1;
  const bool top = rq == 0, bot = rq == 15;
  int w = own32 + col * 16 + rq + z0 * D;
  dpair pm = xat(w - D);
  double amD = UD[cv(w - D)];
  dpair pcur = xat(w);
  for (int z = z0; z < z1; ++z, w += D)
  {
    const int r = w - own32;
    const unsigned wv = (unsigned)(w > ldl ? ldl : w);
    const unsigned m = r < mrows ? (unsigned)__builtin_nontemporal_load(mask + (unsigned)r) : 0u;
    const double aD = __builtin_nontemporal_load(UD + wv);
    const dpair pD = xat(w + D);
    const double a0 = S.j0 >= 0 ? __builtin_nontemporal_load(U0 + wv) : 0.0;
    const double ap = __builtin_nontemporal_load(U1 + wv);
    dpair eg;
    double ae = 0.0;
    if (top || bot) eg = xat(top ? w - 1 : w + 1);
    if (top) ae = U1[cv(w - 1)];
    double an = 0.0, aq = 0.0;
    dpair xn, xq;
    if (mp.dn)
    {
      const int g = w + mp.dn;
      an = mp.Un[cv(g)];
      xn = xat(g);
    }
    if (mp.dq)
    {
      aq = mp.Uq[wv];
      xq = xat(w + mp.dq);
    }
    dpair acc{0.0, 0.0};
    if (m & 1u) acc = fma2(acc, amD, pm);
    if (mp.dn && ((m >> kn0) & 1u)) acc = fma2(acc, an, xn);
    for (int k = kn0 + 1; k < kn1; ++k)  // (further far-negative offsets: generic gathers)
      if ((m >> k) & 1u)
      {
        const int g = w + S.off[k];
        acc = fma2(acc, S.val[(i64)S.dj[k] * S.ld + cv(g)], xat(g));
      }
    // rows w -/+ 1: lanes 4 apart (same column pair); the wave's first / last row loads its own
    const int up = (lane - 4) & 63, dn = (lane + 4) & 63;
    dpair pl{lane_from(pcur.x, up), lane_from(pcur.y, up)}, pr{lane_from(pcur.x, dn), lane_from(pcur.y, dn)};
    double am = lane_from(ap, up);
    if (top)
    {
      pl = eg;
      am = ae;
    }
    if (bot) pr = eg;
    if (S.km1 >= 0 && ((m >> S.km1) & 1u)) acc = fma2(acc, am, pl);
    if (S.k0 >= 0 && ((m >> S.k0) & 1u)) acc = fma2(acc, a0, pcur);
    if (S.kp1 >= 0 && ((m >> S.kp1) & 1u)) acc = fma2(acc, ap, pr);
    if (mp.dq && ((m >> kp0) & 1u)) acc = fma2(acc, aq, xq);
    for (int k = kp0 + 1; k < kp1; ++k)
      if ((m >> k) & 1u) acc = fma2(acc, S.val[(i64)S.dj[k] * S.ld + wv], xat(w + S.off[k]));
    if ((m >> kp1) & 1u) acc = fma2(acc, aD, pD);
    if (r < nrows)
    {
      __builtin_nontemporal_store(acc, Yb + (unsigned)w * 4u);
      if (DOT)
      {
        dsum.x += pcur.x * acc.x;
        dsum.y += pcur.y * acc.y;
      }
    }
    if constexpr (DOT == 2) quad_gram_add(gacc, r < nrows ? acc.x : 0.0, r < nrows ? acc.y : 0.0);  // (a quad = a row)
    pm = pcur;
    pcur = pD;
    amD = aD;
  }
  if constexpr (DOT == 2)
  {
    __shared__ double gs[kStreamThreads / 64 * 72], gv[72], gt[72];
    quad_gram_block<kStreamThreads>(gacc, dsum.x, dsum.y, gs, gv);
    if (grid_sum2<kStreamThreads>(gv, 72, part, part + (size_t)gridDim.x * 72, tick, blockIdx.x, gridDim.x, gt))
    {
      if (threadIdx.x < 64) gram[threadIdx.x] = gt[threadIdx.x];
      if (threadIdx.x < 8) dp[threadIdx.x] = gt[64 + threadIdx.x];
      if (threadIdx.x == 0 && zero_word) *zero_word = 0u;  // (the next MGS's barrier word)
    }
  }
  else if constexpr (DOT)
  {
    __shared__ double tot[8];
    double v[8];
#pragma unroll
    for (int q = 0; q < 4; ++q)
    {
      v[2 * q] = q == cp ? dsum.x : 0.0;
      v[2 * q + 1] = q == cp ? dsum.y : 0.0;
    }
    if (grid_sum_n<8, kStreamThreads>(v, part + (size_t)qb * gridDim.x * 8, tick + (size_t)qb * kTicketStride, tot,
                                      blockIdx.x, gridDim.x))
    {
      if (threadIdx.x < 8) dp[qb * 8 + threadIdx.x] = tot[threadIdx.x];
    }
  }
}

bool launch_spmm_march(const eig_mat_s &A, i64 m, const double *X, double *Y, hipStream_t s);

// ---------------------------------------------------------------------------------------------
// General band march for the 8-column SpMM and the fused Chebyshev step (k_spmm8_marchg).  The
// carried offset P is the widest band offset that is a multiple of 16 with -P stored too (3-D P1
// on the Kuhn split: P = N^2 + N); the others split into four spans of gathered offsets -- S1 below
// -P, S2 in (-P, -1), S3 in (+1, +P), S4 above +P -- of at most kGSpan offsets each, loaded
// predicated and unrolled (gathered operand + band value, the mirrored slot for negative offsets),
// S1 / S2 with the row's streams and S3 / S4 after the near terms.  Accumulation in ascending
// offset order: S1, -P, S2, -1, 0, +1, S3, +P, S4.  EPI = kStore: separately rounded products
// and sums over the stored entries (bitwise the reference SpMM); kGCheb: fused multiply-adds and
// the Chebyshev update of k_sell_mv8q's kCheb epilogue (tolerance-checked).
// ---------------------------------------------------------------------------------------------
enum { kGStore = 0, kGCheb = 1 };

template <class X>
__device__ __forceinline__ void gspan_load(const SymImg &S, int kb, int ke, int w, unsigned wv, int xl, int ldl,
                                           const X &xat, double (&a)[kGSpan], dpair (&x)[kGSpan])
{
#pragma unroll
  for (int k = 0; k < kGSpan; ++k)
  {
    const bool in = kb + k < ke;
    const int d = in ? S.off[kb + k] : 0;
    int g = w + d;
    g = g < 0 ? 0 : (g > xl ? xl : g);
    const unsigned gv = (unsigned)(g > ldl ? ldl : g);
    a[k] = in ? S.val[(i64)S.dj[kb + k] * S.ld + (d < 0 ? gv : wv)] : 0.0;
    x[k] = in ? xat(g) : dpair{0.0, 0.0};
  }
}

template <int EPI>
__device__ __forceinline__ dpair gacc(dpair acc, double a, dpair x)
{
  if (EPI == kGStore) return dpair{acc.x + a * x.x, acc.y + a * x.y};
  return dpair{__builtin_fma(a, x.x, acc.x), __builtin_fma(a, x.y, acc.y)};
}

template <int EPI>
__device__ __forceinline__ void gspan_acc(int kb, int ke, unsigned m, const double (&a)[kGSpan],
                                          const dpair (&x)[kGSpan], dpair &acc)
{
#pragma unroll
  for (int k = 0; k < kGSpan; ++k)
    if (kb + k < ke && ((m >> (kb + k)) & 1u)) acc = gacc<EPI>(acc, a[k], x[k]);
}

template <class MT, int EPI>
__global__ __launch_bounds__(kStreamThreads, 6) void k_spmm8_marchg(
    i64 nrows, i64 own, i64 ld, SellB1 A, MarchPlan mp, GSpans sp, const double *__restrict__ X,
    double *__restrict__ Y, const double *__restrict__ Bv, const double *__restrict__ dinv, double omega,
    double gamma)
{
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int rq = lane >> 2, cp = lane & 3;
  const SymImg &S = A.sym;
  const int xl = (int)A.xlast, P = (int)mp.D, ldl = (int)(S.ld - 1), own32 = (int)own, mrows = (int)mp.mrows;
  const double *UP = S.val + (i64)S.dj[sp.kPp] * S.ld;
  const double *U1 = S.val + (i64)S.j1 * S.ld;
  const double *U0 = S.val + (i64)(S.j0 >= 0 ? S.j0 : 0) * S.ld;
  const MT *mask = static_cast<const MT *>(S.mask);
  // (Measured and dropped at 256^3, m = 32: the workgroup's 4 waves on the 4 column blocks of one
  // item, so the band values / mask / D^-1 are fetched once per 4 blocks -- 6.62 vs 6.73 ms, with
  // any number of plane runs per column; rocprof: L2 misses on the gathered X rows dominate.)
  // (Measured and dropped: a persistent schedule with XCD-owned column ranges walked by 128-768
  // resident waves per XCD -- slower at every count, 7.5-19.5 ms: the march is latency-bound per
  // wave and wants full occupancy.)
  const int item = (int)swizzled_block() * kWaves + wave;
  if (item >= mp.ncol * mp.nseg) return;
  const int col = item % mp.ncol, seg = item / mp.ncol, blk = (int)blockIdx.y;
  const int z0 = (int)(mp.zb + seg * mp.nplanes / mp.nseg), z1 = (int)(mp.zb + (seg + 1) * mp.nplanes / mp.nseg);
  const i64 boff = (i64)blk * ld * 8;
  const dpair *Xb = reinterpret_cast<const dpair *>(X + boff) + cp;
  dpair *Yb = reinterpret_cast<dpair *>(Y + boff) + cp;
  const dpair *Bb = EPI == kGCheb ? reinterpret_cast<const dpair *>(Bv + boff) + cp : nullptr;
  auto xat = [&](int g) { return Xb[(unsigned)(g < 0 ? 0 : (g > xl ? xl : g)) * 4u]; };
  auto cv = [&](int g) -> unsigned { return g < 0 ? 0u : (unsigned)(g > ldl ? ldl : g); };
  const bool top = rq == 0, bot = rq == 15;
  int w = own32 + col * 16 + rq + z0 * P;
  dpair pm = xat(w - P);
  double amP = UP[cv(w - P)];
  dpair pcur = xat(w);
  for (int z = z0; z < z1; ++z, w += P)
  {
    const int r = w - own32;
    const unsigned wv = (unsigned)(w > ldl ? ldl : w);
    const unsigned m = r < mrows ? (unsigned)__builtin_nontemporal_load(mask + (unsigned)r) : 0u;
    const double aP = __builtin_nontemporal_load(UP + wv);
    const dpair pP = xat(w + P);
    const double a0 = S.j0 >= 0 ? __builtin_nontemporal_load(U0 + wv) : 0.0;
    const double ap = __builtin_nontemporal_load(U1 + wv);
    dpair eg;
    double ae = 0.0;
    if (top || bot) eg = xat(top ? w - 1 : w + 1);
    if (top) ae = U1[cv(w - 1)];
    double a1[kGSpan], a2[kGSpan];
    dpair x1[kGSpan], x2[kGSpan];
    gspan_load(S, sp.s1b, sp.s1e, w, wv, xl, ldl, xat, a1, x1);
    gspan_load(S, sp.s2b, sp.s2e, w, wv, xl, ldl, xat, a2, x2);
    dpair acc{0.0, 0.0};
    gspan_acc<EPI>(sp.s1b, sp.s1e, m, a1, x1, acc);
    if ((m >> sp.kPm) & 1u) acc = gacc<EPI>(acc, amP, pm);
    gspan_acc<EPI>(sp.s2b, sp.s2e, m, a2, x2, acc);
    const int up = (lane - 4) & 63, dn = (lane + 4) & 63;
    dpair pl{lane_from(pcur.x, up), lane_from(pcur.y, up)}, pr{lane_from(pcur.x, dn), lane_from(pcur.y, dn)};
    double am = lane_from(ap, up);
    if (top)
    {
      pl = eg;
      am = ae;
    }
    if (bot) pr = eg;
    if (S.km1 >= 0 && ((m >> S.km1) & 1u)) acc = gacc<EPI>(acc, am, pl);
    if (S.k0 >= 0 && ((m >> S.k0) & 1u)) acc = gacc<EPI>(acc, a0, pcur);
    if (S.kp1 >= 0 && ((m >> S.kp1) & 1u)) acc = gacc<EPI>(acc, ap, pr);
    gspan_load(S, sp.s3b, sp.s3e, w, wv, xl, ldl, xat, a1, x1);
    gspan_load(S, sp.s4b, sp.s4e, w, wv, xl, ldl, xat, a2, x2);
    gspan_acc<EPI>(sp.s3b, sp.s3e, m, a1, x1, acc);
    if ((m >> sp.kPp) & 1u) acc = gacc<EPI>(acc, aP, pP);
    gspan_acc<EPI>(sp.s4b, sp.s4e, m, a2, x2, acc);
    if (r < nrows)
    {
      if (EPI == kGStore)
        __builtin_nontemporal_store(acc, Yb + (unsigned)w * 4u);
      else
      {
        const double di = __builtin_nontemporal_load(dinv + r);
        const dpair bb = __builtin_nontemporal_load(Bb + (unsigned)w * 4u);
        const dpair xo = __builtin_nontemporal_load(Yb + (unsigned)w * 4u);
        const double gd = gamma * di;
        const double o0 = omega * (pcur.x + gd * (bb.x - acc.x) - xo.x) + xo.x;
        const double o1 = omega * (pcur.y + gd * (bb.y - acc.y) - xo.y) + xo.y;
        __builtin_nontemporal_store(dpair{o0, o1}, Yb + (unsigned)w * 4u);
      }
    }
    pm = pcur;
    pcur = pP;
    amP = aP;
  }
}

// The packed value image of the 7-point pack marches (MarchTraits::needs_pack): two arrays of value
// pairs, (+D, 0) and (+1, +nx)
// per window row (the 5-point 2-D band: +nx = 0), so a wave reads each with one 16-B load per lane
// of 1 KB contiguous; built from the band arrays at first use, freed by a shift.
__global__ void k_sym_pack(i64 ld, const double *__restrict__ UD, const double *__restrict__ U0,
                           const double *__restrict__ U1, const double *__restrict__ Uq, double *__restrict__ out)
{
  for (i64 w = (i64)blockIdx.x * blockDim.x + threadIdx.x; w < ld; w += (i64)gridDim.x * blockDim.x)
  {
    reinterpret_cast<dpair *>(out)[w] = dpair{UD[w], U0 ? U0[w] : 0.0};
    reinterpret_cast<dpair *>(out)[ld + w] = dpair{U1[w], Uq ? Uq[w] : 0.0};
  }
}
// Kuhn pack (the Kuhn variants with KP): four pair arrays, (0, +1), (+nx, +nx+1), (+D, +D+1), (+D+nx, +D+nx+1)
__global__ void k_kuhn_pack(i64 ld, const double *__restrict__ val, int4 ja, int4 jb, double *__restrict__ out)
{
  const int j0[4] = {ja.x, ja.z, jb.x, jb.z}, j1[4] = {ja.y, ja.w, jb.y, jb.w};
  for (i64 w = (i64)blockIdx.x * blockDim.x + threadIdx.x; w < ld; w += (i64)gridDim.x * blockDim.x)
#pragma unroll
    for (int q = 0; q < 4; ++q)
      reinterpret_cast<dpair *>(out)[(i64)q * ld + w] = dpair{val[(i64)j0[q] * ld + w], val[(i64)j1[q] * ld + w]};
}
void sym_pack_fill(eig_mat_s &A, hipStream_t s)
{
  if (A.sym_box27 == kKuhn15)
  {
    // band array of each upper Kuhn offset (the 27-box positions 13 14 | 16 17 | 22 23 | 25 26)
    const i64 D = (i64)A.sym_gx * A.sym_gy;
    auto j = [&](int q) { return std::max(0, box_band_array(A, D, q)); };
    hipLaunchKernelGGL(k_kuhn_pack, dim3(2048), dim3(256), 0, s, A.sym_ld, A.sym_val,
                       make_int4(j(13), j(14), j(16), j(17)), make_int4(j(22), j(23), j(25), j(26)), A.sym_pack);
    EIG_HIP(hipGetLastError());
    return;
  }
  const SellB1 b = sell_b1(A);
  const SymImg &S = b.sym;
  const double *UD = S.val + (i64)S.dj[S.nd - 1] * S.ld, *U1 = S.val + (i64)S.j1 * S.ld;
  const double *U0 = S.j0 >= 0 ? S.val + (i64)S.j0 * S.ld : nullptr;
  const double *Uq = S.khi < S.nd - 1 ? S.val + (i64)S.dj[S.khi] * S.ld : nullptr;
  hipLaunchKernelGGL(k_sym_pack, dim3(2048), dim3(256), 0, s, S.ld, UD, U0, U1, Uq, A.sym_pack);
  EIG_HIP(hipGetLastError());
}

// The value pack, built at the first launch that marches on it (never by a plan made for a query:
// eig_mat_get_info, kernel names, byte models).  eig_lanczos_capture builds it before capturing,
// so no graph records the pack kernel; a shift refills the same buffer in place.
const double *sym_pack_prepare(const eig_mat_s &Ac)
{
  eig_mat_s &A = const_cast<eig_mat_s &>(Ac);
  if (A.sym_pack) return A.sym_pack;
  const i64 bytes = A.sym_ld * (A.sym_box27 == kKuhn15 ? 64 : 32);
  EIG_HIP(hipMalloc(&A.sym_pack, (size_t)bytes));
  A.sym_pack_bytes = bytes;
  A.device_bytes += bytes;
  sym_pack_fill(A, A.ctx->stream);
  return A.sym_pack;
}

// Calls f(MT{}) with the row-mask word of a lane-shift band image: uint8_t for kSymN8, uint32_t for kSymN32.
template <class F>
static void with_mask_type(int mode, const F &f)
{
  if (mode == kSymN8) f(uint8_t{});
  else f(uint32_t{});
}

// Launch the march kernel of plan variant `variant`: calls launch(MT{}, SPAN1, UNI) once, with the
// template head <MT, SPAN1, UNI> as values (a mask word, a std::bool_constant, a std::integral_constant)
// -- the head of the variant's traits, or for variant 0 the one of the image's mask width and far
// spans.  A launcher's generic lambda so instantiates its kernel once per entry of MarchDispatch
// (variant 0: all three heads).
template <int... V, class Launch>
static void march_launch(std::integer_sequence<int, V...>, const eig_mat_s &A, int mode, int variant,
                         const Launch &launch)
{
  const int v = march_launch_variant(A, mode, variant);
  const bool u8 = mode == kSymN8, span1 = u8 && march_span1(A);
  auto launch_if = [&](auto vc) {
    constexpr MarchTraits T = march_traits(decltype(vc)::value);
    if (v != vc) return false;
    if constexpr (!T.any_head())
      launch(std::conditional_t<T.mask_bytes() == 4, uint32_t, uint8_t>{}, std::bool_constant<T.span1()>{}, vc);
    else if (span1)
      launch(uint8_t{}, std::true_type{}, vc);
    else if (u8)
      launch(uint8_t{}, std::false_type{}, vc);
    else
      launch(uint32_t{}, std::false_type{}, vc);
    return true;
  };
  const bool launched = (launch_if(std::integral_constant<int, V>{}) || ...);
  EIG_CHECK(launched, EIG_ERR_ARG, "march launch: variant without a kernel");
}

const i32 kMarchInteriorTag = 0;

// march_plan (march_plan.cpp) for a launch: the plan, and the value pack its variant streams, built here at the
// first launch that marches on it.  (A query calls march_plan itself and so never builds the pack.)
static MarchPlan march_plan_packed(const eig_mat_s &A, int mode, i64 zb, i64 ze, bool fused)
{
  MarchPlan mp = march_plan(A, mode, zb, ze, fused);
  if (mp.nseg > 0) mp.pack = march_traits(mp.uni).needs_pack() ? sym_pack_prepare(A) : nullptr;
  return mp;
}

void march_prepare(const eig_mat_s &A)
{
  if (A.br != 1 || A.bc != 1) return;
  const int mode = image_mode(A);
  for (bool fused : {false, true})
  {
    (void)march_plan_packed(A, mode, 0, -1, fused);
    if (A.mz1 > A.mz0) (void)march_plan_packed(A, mode, A.mz0, A.mz1, fused);
  }
}

// Plan for a launch: the whole matrix (slices == nullptr over all slices), the interior planes of a
// distributed slab (slices == &kMarchInteriorTag), or none (nseg = 0: the slice kernels run).
static MarchPlan launch_plan(const eig_mat_s &A, int mode, const i32 *slices, i64 first, i64 count,
                             bool fused = false)
{
  if (slices == &kMarchInteriorTag)
  {
    const MarchPlan mp = march_plan_packed(A, mode, A.mz0, A.mz1, fused);
    EIG_CHECK(mp.nseg > 0, EIG_ERR_ARG, "interior-plane launch without a march plan");
    return mp;
  }
  if (!slices && first == 0 && count == A.nslices) return march_plan_packed(A, mode, 0, -1, fused);
  return MarchPlan{};
}

// The march half of launch_spmv / launch_lanczos_spmv / launch_lanczos_fused (k_spmv.hip), mode = image_mode(A):
// true when the launch had a plan and its march kernel was launched, false (nothing launched) when the
// slice kernels are to run.
bool launch_spmv_march(const eig_mat_s &A, int mode, const double *x, double *y, const i32 *slices, i64 first,
                       i64 count, hipStream_t s, bool keep)
{
  MarchPlan mp = launch_plan(A, mode, slices, first, count);
  // keep: y is read by the very next launch (the pipelined step's S) -- plain stores on grids
  // whose vectors fit the MALL, as the fused step's (MarchPlan::tstore)
  if (keep && march_traits(mp.uni).geo2_path() && vectors_fit_mall(A)) mp.tstore = 1;
  if (mp.nseg <= 0) return false;
  march_launch(MarchDispatch{}, A, mode, mp.uni, [&](auto mt, auto span1, auto uni) {
    hipLaunchKernelGGL((k_spmv_march<decltype(mt), span1(), uni()>), dim3(march_grid(mp)), dim3(kStreamThreads), 0,
                       s, A.nb_rows, A.own_offset, sell_b1(A), mp, x, y);
  });
  return true;
}

bool launch_lanczos_spmv_march(const eig_mat_s &A, int mode, const double *u, const double *up, double *t, int j,
                               const LanczosState &st, const i32 *slices, i64 first, i64 count, double *dot_out,
                               double *beta_out, int ticket, hipStream_t s, ReduceWS red)
{
  const MarchPlan mp = launch_plan(A, mode, slices, first, count);
  if (mp.nseg <= 0) return false;
  march_launch(MarchDispatch{}, A, mode, mp.uni, [&](auto mt, auto span1, auto uni) {
    hipLaunchKernelGGL((k_lanczos_spmv_march<decltype(mt), span1(), uni()>), dim3(march_grid(mp)),
                       dim3(kStreamThreads), 0, s, A.nb_rows, A.own_offset, sell_b1(A), mp, u, up, t, j, st.nsum,
                       dot_out, beta_out, red.partials, red.ticket(ticket));
  });
  return true;
}

// L: the launch index (FusedLaunch::L), which sets the serpentine direction
bool launch_lanczos_fused_march(const eig_mat_s &A, int mode, const double *P, double *Pout, const FusedArgs &fa,
                                int L, const i32 *slices, i64 first, i64 count, double *out, int ticket,
                                hipStream_t s, ReduceWS red)
{
  MarchPlan mp = launch_plan(A, mode, slices, first, count, true);
  if (mp.nseg <= 0) return false;
  // serpentine: odd launches march down, so each launch starts on the planes the one before it
  // finished on (whole-matrix and interior-plane launches alike; a repair launch marches nothing
  // but takes an index, so the parity simply continues).  EIG_TUNE_CACHE 8 / 16 fix the direction,
  // 24 alternates whatever the default is
  if (march_traits(mp.uni).down_body && ((A.tune_cache & 24) == 24 || (kMarch2lSerpentine && !(A.tune_cache & 24))))
    mp.down = L & 1;
  march_launch(MarchDispatch{}, A, mode, mp.uni, [&](auto mt, auto span1, auto uni) {
    if constexpr (kTraits<uni()>.pipe_body)
    {
      // the pipelined body's LDS is past the 64 KiB a kernel gets unasked: raise the kernel's limit once
      // per device
      static std::atomic<bool> raised[kMaxPipeDevices];
      const int dev = A.ctx->device;
      EIG_CHECK(!mp.pipe || (dev >= 0 && dev < kMaxPipeDevices), EIG_ERR_ARG, "pipelined march: device index");
      if (mp.pipe && !raised[dev].load(std::memory_order_acquire))
      {
        EIG_HIP(hipFuncSetAttribute(
            reinterpret_cast<const void *>(&k_lanczos_fused_march<decltype(mt), span1(), uni()>),
            hipFuncAttributeMaxDynamicSharedMemorySize, (int)kMarchPipeLds));
        raised[dev].store(true, std::memory_order_release);
      }
    }
    else
      mp.pipe = 0;
    hipLaunchKernelGGL((k_lanczos_fused_march<decltype(mt), span1(), uni()>), dim3(march_grid(mp)),
                       dim3(kStreamThreads), mp.pipe ? kMarchPipeLds : 0, s, A.nb_rows, A.own_offset, sell_b1(A), mp,
                       reinterpret_cast<const dpair *>(P), reinterpret_cast<dpair *>(Pout), fa, out, red.partials,
                       red.ticket(ticket));
  });
  return true;
}

template <int EPI>
static bool launch_marchg(const eig_mat_s &A, i64 m, const double *X, double *Y, const double *Bv,
                          const double *dinv, double omega, double gamma, hipStream_t s)
{
  MarchPlan mp;
  GSpans sp;
  if (m <= 0 || !marchg_plan(A, mp, sp)) return false;
  const dim3 grid(march_grid(mp), (unsigned)(m / 8));
  with_mask_type(image_mode(A), [&](auto mt) {
    hipLaunchKernelGGL((k_spmm8_marchg<decltype(mt), EPI>), grid, dim3(kStreamThreads), 0, s, A.nb_rows, A.own_offset,
                       A.window, sell_b1(A), mp, sp, X, Y, Bv, dinv, omega, gamma);
  });
  return true;
}

bool launch_cheb_march(const eig_mat_s &M, i64 m, const double *Xk, double *Xold, const double *B, const double *dinv,
                       double omega, double gamma, hipStream_t s)
{
  return launch_marchg<kGCheb>(M, m, Xk, Xold, B, dinv, omega, gamma, s);
}

bool launch_spmm_march(const eig_mat_s &A, i64 m, const double *X, double *Y, hipStream_t s)
{
  if (A.br != 1 || A.bc != 1 || m <= 0) return false;
  const int mode = image_mode(A);
  const MarchPlan mp = march_plan(A, mode, 0, -1, false, 16);
  if (mp.nseg == 0) return launch_marchg<kGStore>(A, m, X, Y, nullptr, nullptr, 0.0, 0.0, s);
  const dim3 grid(march_grid(mp), (unsigned)(m / 8));
  with_mask_type(mode, [&](auto mt) {
    hipLaunchKernelGGL((k_spmm8_march<decltype(mt)>), grid, dim3(kStreamThreads), 0, s, A.nb_rows, A.own_offset, A.window,
                       sell_b1(A), mp, X, Y);
  });
  return true;
}

// Y = A X with the diagonal dots dp (k_spmm8_march<MT, true>) where the band march applies to the
// whole matrix on one rank; false otherwise (the caller runs the product and k_dot_diag_mv8).
bool launch_spmm_march_dot(const eig_mat_s &A, i64 m, const double *X, double *Y, double *dp, ReduceWS red,
                           hipStream_t s)
{
  if (A.br != 1 || A.bc != 1 || m <= 0 || A.ctx->distributed()) return false;
  const int mode = image_mode(A);
  if (!is_sym_mode(mode)) return false;
  const MarchPlan mp = march_plan(A, mode, 0, -1, false, 16);
  if (mp.nseg == 0) return false;
  const dim3 grid(march_grid(mp), (unsigned)(m / 8));
  if ((i64)grid.x * 8 * grid.y > (i64)kMaxRedBlocks * kMaxRedVals || grid.y > (unsigned)kNumTickets) return false;
  with_mask_type(mode, [&](auto mt) {
    hipLaunchKernelGGL((k_spmm8_march<decltype(mt), true>), grid, dim3(kStreamThreads), 0, s, A.nb_rows, A.own_offset,
                       A.window, sell_b1(A), mp, X, Y, dp, red.partials, red.ticket(0));
  });
  return true;
}

// The same with the window Gram of Y (k_spmm8_march<MT, 2>), m = 8 only.
bool launch_spmm_march_dot_gram(const eig_mat_s &A, i64 m, const double *X, double *Y, double *dp, double *gram,
                                ReduceWS red, hipStream_t s, unsigned *zero_word)
{
  if (A.br != 1 || A.bc != 1 || m != 8 || A.ctx->distributed()) return false;
  const int mode = image_mode(A);
  if (!is_sym_mode(mode)) return false;
  const MarchPlan mp = march_plan(A, mode, 0, -1, false, 16);
  if (mp.nseg == 0) return false;
  const dim3 grid(march_grid(mp), 1u);
  if ((i64)grid.x * 72 + 8 * 72 > (i64)kMaxRedBlocks * kMaxRedVals) return false;
  with_mask_type(mode, [&](auto mt) {
    hipLaunchKernelGGL((k_spmm8_march<decltype(mt), 2>), grid, dim3(kStreamThreads), 0, s, A.nb_rows, A.own_offset,
                       A.window, sell_b1(A), mp, X, Y, dp, red.partials, red.ticket(0), gram, zero_word);
  });
  return true;
}

}  // namespace eigmi
