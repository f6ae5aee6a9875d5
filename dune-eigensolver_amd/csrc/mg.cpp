// mg.cpp -- geometric multigrid inner solve for the spectral transformation of config C5 (the
// smallest end of K x = lambda M x, which GeneralizedInverse returns: eigensolver.hh:204-351; there
// with an UMFPACK LU, which does not exist at 256^3 -- SURVEY 7, hard part 4).
//
// Hierarchy (host setup, once): a box grid nx x ny x nz (lexicographic) is coarsened by keeping the
// fine nodes of odd index in every direction (nc = nf / 2), with trilinear P (k_mg.hip) and the
// Galerkin operator A_c = P^T A P computed on the host from the fine rows (27-point coarse
// stencils; any fine stencil within +-1 node per direction), mirrored so that every coarse matrix
// is bitwise symmetric (it then takes the band / box images of the device upload).  Levels stop at
// <= 64 rows or a direction < 3 nodes; grids whose coarsest level would exceed kMgMaxCoarse rows (flat
// grids: a direction runs out first) are refused.  The host part (mg_setup.h / mg_setup.cpp) has no device call.
//
// Square blocks b = 2..4 (FieldMatrix<double,b,b>; one rank): coarsening is by nodes (nx ny nz = block rows, a
// vector has b scalar rows per node, node-major), P = P_trilinear (x) I_b, the Galerkin operator has a b x b block
// per stencil slot, and the smoother is Chebyshev with BLOCK Jacobi: D the block diagonal (D_I^-1 per node,
// k_spmm_blk_mv8_cheb<.., true>), lmax the block Gershgorin bound max_I sum_J ||L_I^-1 A_IJ L_J^-T||_2,
// D_I = L_I L_I^T.  Point Jacobi ignores the coupling inside a node and contracts half as fast.
//
// Algebraic hierarchies (eig_amg_create; 1x1 blocks, any pattern, no grid): amg_setup.h / amg_setup.cpp build
// every level on the host from the matrix alone -- strength of connection, three-pass aggregation, the smoothed
// prolongator P = (I - omega D^-1 A) T and its transpose, A_c = P^T (A P) mirrored -- and a level carries the device
// CSR of P and P^T for the transfers of k_amg.hip instead of grid extents.  The V-cycle below is the same one:
// vcycle() only picks the transfers by the level's kind.
//
// Solve (device, no reductions): X = S_k B with S_k = sum_{i<k} (I - V A)^i V, i.e. `cycles`
// stationary iterations x += V (b - A x) from x = 0, V one symmetric V-cycle:
//   pre-smooth  x = p(D^-1 A) D^-1 b      (Chebyshev-Jacobi, degree nu, on [lmax / ratio, lmax],
//                                          lmax the Gershgorin bound of D^-1 A; cheb_solve)
//   r = b - A x;  x += P V_c (P^T r);  r = b - A x;  x += p(D^-1 A) D^-1 r   (the same polynomial)
// the coarsest level by a Chebyshev-Jacobi solve on its exact spectrum bounds (host eigenvalues)
// to 1e-15.  With V symmetric, S_k is a fixed symmetric linear operator, so the block Lanczos on
// OP = S_k M (eig_blanczos_create_si_mg) runs on a self-adjoint operator in the M-inner product,
// with no inner product inside the solve (halo-only when distributed -- single rank here).
#include <algorithm>
#include <cmath>
#include <cstring>
#include <thread>
#include <vector>

#include "amg_setup.h"
#include "mg_setup.h"
#include "subspace.h"

using namespace eigmi;

namespace eigmi {
// b: scalar rows per grid node (k_mg.hip)
void launch_mg_restrict(const int *fdim, const int *cdim, int b, i64 m, i64 ldf, i64 ldc, const double *Rf, double *Bc,
                        hipStream_t s);
void launch_mg_prolong_add(const int *fdim, const int *cdim, int b, i64 m, i64 ldf, i64 ldc, const double *Xc,
                           double *Xf, hipStream_t s);
void launch_mv8_axpby(i64 n, i64 m, i64 ld, double a, const double *X, double b, double *Y, hipStream_t s);
// transfers of an algebraic hierarchy on the device CSR of P^T (cn rows) / P (fn rows) (k_amg.hip)
void launch_amg_restrict(i64 cn, const i64 *rp, const i32 *col, const double *val, i64 m, i64 ldf, i64 ldc,
                         const double *Rf, double *Bc, hipStream_t s);
void launch_amg_prolong_add(i64 fn, const i64 *rp, const i32 *col, const double *val, i64 m, i64 ldf, i64 ldc,
                            const double *Xc, double *Xf, hipStream_t s);
}  // namespace eigmi

// Device CSR of a transfer operator (row pointers i64, columns i32, values double).
struct AmgCsrDev {
  DevBuf *rp = nullptr, *col = nullptr, *val = nullptr;
  void upload(const MgCsr &h)
  {
    rp = new DevBuf(h.rp.size() * sizeof(i64));
    col = new DevBuf(h.col.size() * sizeof(i32));
    val = new DevBuf(h.val.size() * sizeof(double));
    EIG_HIP(hipMemcpy(rp->p, h.rp.data(), h.rp.size() * sizeof(i64), hipMemcpyHostToDevice));
    if (!h.col.empty())
    {
      EIG_HIP(hipMemcpy(col->p, h.col.data(), h.col.size() * sizeof(i32), hipMemcpyHostToDevice));
      EIG_HIP(hipMemcpy(val->p, h.val.data(), h.val.size() * sizeof(double), hipMemcpyHostToDevice));
    }
  }
  void release()
  {
    delete rp;
    delete col;
    delete val;
    rp = col = val = nullptr;
  }
};

struct MgLevel {
  eig_mat_s *A = nullptr;
  bool own = false;  // coarse levels own their matrix
  int dim[3] = {0, 0, 0};                     // nodes per direction
  int b = 1;                                  // scalar rows per node (the block size)
  i64 n = 0;                                  // scalar rows (nodes * b)
  i64 nnz = 0;                                // stored scalar entries of A
  // algebraic hierarchy (eig_amg_create): the transfers to the next level, P (n rows) and P^T (rows of the next
  // level); a geometric level has none and uses dim[]
  bool algebraic = false;
  AmgCsrDev P, PT;
  double lmax = 2.0;                          // (block) Gershgorin bound of D^-1 A
  double clo = 0.0, chi = 0.0;                // coarsest: exact spectrum bounds of D^-1 A
  int cdeg = 0;                               // coarsest: Chebyshev degree
  // dinv: 1 / a_rr per scalar row (b = 1), the inverse b x b diagonal block per node (b > 1)
  DevBuf *dinv = nullptr, *B = nullptr, *T = nullptr, *C[4] = {nullptr, nullptr, nullptr, nullptr};
};

struct eig_mg_s {
  eig_ctx_t ctx = nullptr;
  std::vector<MgLevel> lev;
  int max_cols = 32, nu = 2;
  double ratio = 10.0;
  ~eig_mg_s()
  {
    for (auto &L : lev)
    {
      for (DevBuf *b : {L.dinv, L.B, L.T, L.C[0], L.C[1], L.C[2], L.C[3]}) delete b;
      L.P.release();
      L.PT.release();
      if (L.own && L.A) eig_mat_destroy(L.A);
    }
  }
};

namespace {

// Chebyshev semi-iteration with block Jacobi on square blocks 2..4: cheb_solve's recurrence (subspace.cpp) with
// z = D_I^-1 (b - M x_k) per node; the in-place two-buffer form.  Returns the buffer holding x_degree.
double *cheb_solve_bjac(eig_mat_s &M, i64 m, int degree, double lmin, double lmax, const double *Bv, const double *binv,
                        double *Xa, double *Xb, hipStream_t s)
{
  const ChebJacobi cj(lmin, lmax);
  double omega = cj.omega1();
  launch_cheb_init_bjac(M, m, Bv, binv, cj.gamma, Xa, s);
  if (degree <= 1) return Xa;
  EIG_HIP(hipMemsetAsync(Xb, 0, (size_t)M.window * m * sizeof(double), s));  // x_0 = 0
  for (int k = 1; k < degree; ++k)
  {
    if (k > 1) omega = cj.next(omega);
    launch_cheb_step_bjac(M, m, Xa, Xb, Bv, binv, omega, cj.gamma, s);
    std::swap(Xa, Xb);
  }
  return Xa;
}

// p(D^-1 A) D^-1 b on a level: point Jacobi on 1x1 blocks, block Jacobi on blocks
double *smooth(MgLevel &L, i64 m, int degree, double lo, double hi, const double *b, double *Xa, double *Xb, double *Xc,
               hipStream_t s)
{
  if (L.b > 1) return cheb_solve_bjac(*L.A, m, degree, lo, hi, b, L.dinv->d(), Xa, Xb, s);
  return cheb_solve(*L.A, m, degree, lo, hi, b, L.dinv->d(), Xa, Xb, Xc, s);
}

void alloc_level(MgLevel &L, int m, hipStream_t s)
{
  const size_t bytes = (size_t)std::max<i64>(L.n, 1) * m * sizeof(double);
  L.dinv = new DevBuf((size_t)std::max<i64>(L.n, 1) * L.b * sizeof(double));
  L.B = new DevBuf(bytes);
  L.T = new DevBuf(bytes);
  for (auto &c : L.C) c = new DevBuf(bytes);
  (void)s;
}

// V_l b: the V-cycle on level l (all buffers n_l x m, ld = n_l); returns the level buffer (one of
// C[0..3]) that holds the result.  Residuals come from the SpMM's residual epilogue (T = b - A x in
// one pass), the smoothers' zero start is not read (box kernels), and the smoothed iterate stays where
// cheb_solve left it (the post-smoother takes the three other C buffers).
double *vcycle(eig_mg_s &mg, size_t l, i64 m, const double *b)
{
  MgLevel &L = mg.lev[l];
  hipStream_t s = mg.ctx->stream;
  double *C[4] = {L.C[0]->d(), L.C[1]->d(), L.C[2]->d(), L.C[3]->d()};
  if (l + 1 == mg.lev.size())
    return smooth(L, m, L.cdeg, L.clo, L.chi, b, C[0], C[1], C[2], s);
  MgLevel &Cl = mg.lev[l + 1];
  const double lo = L.lmax / mg.ratio, hi = L.lmax;
  double *x = smooth(L, m, mg.nu, lo, hi, b, C[0], C[1], C[2], s);
  double *T = L.T->d();
  launch_resid_mv8(*L.A, m, x, b, T, s);  // T = b - A x
  if (L.algebraic)
    launch_amg_restrict(Cl.n, (const i64 *)L.PT.rp->p, (const i32 *)L.PT.col->p, (const double *)L.PT.val->p, m, L.n, Cl.n,
                        T, Cl.B->d(), s);
  else
    launch_mg_restrict(L.dim, Cl.dim, L.b, m, L.n, Cl.n, T, Cl.B->d(), s);
  const double *xc = vcycle(mg, l + 1, m, Cl.B->d());
  if (L.algebraic)
    launch_amg_prolong_add(L.n, (const i64 *)L.P.rp->p, (const i32 *)L.P.col->p, (const double *)L.P.val->p, m, L.n, Cl.n, xc,
                           x, s);
  else
    launch_mg_prolong_add(L.dim, Cl.dim, L.b, m, L.n, Cl.n, xc, x, s);
  launch_resid_mv8(*L.A, m, x, b, T, s);  // T = b - A x
  // x += post-smoothing correction: a degree-2 smoother on the row-class image adds its x_2 in
  // place (cheb_solve's first step, its gamma and omega_1); 1x1 blocks only
  const ChebJacobi cj(lo, hi);
  if (L.b == 1 && mg.nu == 2 && launch_box_cheb_first_add(*L.A, m, T, cj.omega1(), cj.gamma, x, s)) return x;
  double *q[3];
  for (int i = 0, j = 0; i < 4; ++i)
    if (C[i] != x) q[j++] = C[i];
  const double *p = smooth(L, m, mg.nu, lo, hi, T, q[0], q[1], q[2], s);
  launch_mv8_axpby(L.n, m, L.n, 1.0, p, 1.0, x, s);
  return x;
}

}  // namespace

namespace eigmi {

// X = S_cycles B (window-layout pointers of the level-0 matrix, m columns), stream-ordered.
void mg_apply(eig_mg_s &mg, i64 m, const double *B, double *X, int cycles)
{
  MgLevel &L = mg.lev[0];
  hipStream_t s = mg.ctx->stream;
  EIG_CHECK(m > 0 && m % 8 == 0 && m <= mg.max_cols && cycles >= 1, EIG_ERR_ARG,
            "multigrid solve: 8 <= m <= max_cols (multiple of 8), cycles >= 1");
  const size_t bytes = (size_t)L.n * m * sizeof(double);
  double *R = L.B->d();
  const double *rhs = B;  // residual of the current iterate (B itself before the first correction)
  for (int it = 0; it < cycles; ++it)
  {
    const double *E = vcycle(mg, 0, m, rhs);
    // r -= A e (in place after the first iteration) and X = E / X += E: one pass on the row-class
    // image (the residual kernel's epilogue also writes X), a copy or axpby and the residual
    // otherwise
    if (L.b == 1 && it + 1 < cycles && launch_box_resid_acc(*L.A, m, E, rhs, R, X, it == 0, s))
    {
      rhs = R;
      continue;
    }
    if (it == 0)
      EIG_HIP(hipMemcpyAsync(X, E, bytes, hipMemcpyDeviceToDevice, s));
    else
      launch_mv8_axpby(L.n, m, L.n, 1.0, E, 1.0, X, s);
    if (it + 1 < cycles)
    {
      launch_resid_mv8(*L.A, m, E, rhs, R, s);
      rhs = R;
    }
  }
}

}  // namespace eigmi

namespace eigmi {
eig_mat_s *mg_matrix(const eig_mg_s &mg) { return mg.lev.front().A; }
int mg_max_cols(const eig_mg_s &mg) { return mg.max_cols; }
}  // namespace eigmi

extern "C" int eig_mg_create(eig_mat_t A, int nx, int ny, int nz, int max_cols, int smooth_degree, double smooth_ratio,
                             eig_mg_t *out)
{
  return guard(A ? A->ctx : nullptr, [&] {
    EIG_CHECK(A && out && nx > 0 && ny > 0 && nz > 0 && max_cols >= 8 && max_cols % 8 == 0 && smooth_degree >= 1 &&
                  smooth_ratio > 1.0,
              EIG_ERR_ARG, "eig_mg_create: bad argument");
    EIG_CHECK(A->br == A->bc && A->br >= 1 && A->br <= 4, EIG_ERR_BLOCKSIZE,
              "eig_mg_create: square blocks FieldMatrix<double,b,b>, b = 1..4, only");
    const int bs = A->br;
    EIG_CHECK(!A->ctx->distributed() && A->nb_rows == A->nb_cols && A->window == A->nb_rows * bs, EIG_ERR_ARG,
              "eig_mg_create: square single-rank matrix required");
    EIG_CHECK((i64)nx * ny * nz == A->nb_rows, EIG_ERR_SHAPE,
              "eig_mg_create: nx * ny * nz must equal the (block) rows");
    {
      // the coarsest level is solved through a dense host eigenvalue problem (mg_spectrum_bounds): coarsening
      // halves every direction and stops at a direction below 3 nodes, so a flat grid (e.g. nz = 1, or
      // 256 x 256 x 4) would end far above 64 nodes -- refuse it instead of an O(n^3) dense solve
      const i64 n = mg_coarsest_rows(nx, ny, nz, bs);
      EIG_CHECK(n <= kMgMaxCoarse, EIG_ERR_ARG,
                "eig_mg_create: the grid coarsens only to " + std::to_string(n) + " rows (a direction falls below 3 "
                "nodes first; at most " + std::to_string(kMgMaxCoarse) + " rows are solved densely): semi-"
                "coarsening of flat grids is not implemented");
    }
    eig_ctx_t ctx = A->ctx;
    EIG_HIP(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    auto *mg = new eig_mg_s();
    try
    {
      mg->ctx = ctx;
      mg->max_cols = max_cols;
      mg->nu = smooth_degree;
      mg->ratio = smooth_ratio;
      MgCsr h;
      mat_download_bcsr(*A, h.rp, h.col, h.val);
      MgLevel L0;
      L0.A = A;
      L0.dim[0] = nx, L0.dim[1] = ny, L0.dim[2] = nz;
      L0.b = bs;
      L0.n = A->nb_rows * bs;
      mg->lev.push_back(L0);
      std::vector<double> binv;
      for (;;)
      {
        MgLevel &F = mg->lev.back();
        const i64 nodes = F.n / bs;
        F.nnz = (i64)h.col.size() * bs * bs;
        if (bs == 1)
        {
          F.lmax = mg_gershgorin(h, F.n);
          alloc_level(F, max_cols, s);
          launch_diag_inv(*F.A, F.dinv->d(), s);
        }
        else
        {
          F.lmax = mg_block_jacobi(h, nodes, bs, binv);
          alloc_level(F, max_cols, s);
          EIG_HIP(hipMemcpy(F.dinv->d(), binv.data(), binv.size() * sizeof(double), hipMemcpyHostToDevice));
        }
        if (mg_last_level(F.dim))
        {
          mg_spectrum_bounds(h, nodes, bs, F.clo, F.chi);
          F.clo *= 0.999;
          F.chi *= 1.001;
          F.cdeg = mg_coarse_degree(F.clo, F.chi);
          break;
        }
        MgLevel C;
        for (int d = 0; d < 3; ++d) C.dim[d] = F.dim[d] / 2;
        const i64 cn = (i64)C.dim[0] * C.dim[1] * C.dim[2];
        C.b = bs;
        C.n = cn * bs;
        MgCsr hc;
        mg_galerkin(h, bs, F.dim, C.dim, hc);
        eig_mat_t Ac = nullptr;
        const int rc = eig_mat_create_bcsr(ctx, cn, cn, bs, bs, hc.rp.data(), hc.col.data(), hc.val.data(), &Ac);
        if (rc != EIG_OK) throw Error(rc, std::string("multigrid: coarse upload: ") + eig_last_error(ctx));
        C.A = Ac;
        C.own = true;
        mg->lev.push_back(C);
        h = std::move(hc);
      }
      EIG_HIP(hipStreamSynchronize(s));
    }
    catch (...)
    {
      delete mg;
      throw;
    }
    *out = mg;
  });
}

extern "C" int eig_amg_create(eig_mat_t A, double theta, int max_cols, int smooth_degree, double smooth_ratio,
                              eig_mg_t *out)
{
  return guard(A ? A->ctx : nullptr, [&] {
    EIG_CHECK(A && out && theta >= 0.0 && max_cols >= 8 && max_cols % 8 == 0 && smooth_degree >= 1 && smooth_ratio > 1.0,
              EIG_ERR_ARG, "eig_amg_create: bad argument");
    EIG_CHECK(A->br == 1 && A->bc == 1, EIG_ERR_BLOCKSIZE,
              "eig_amg_create: 1x1 blocks only (blocked matrices need their near-null-space)");
    EIG_CHECK(!A->ctx->distributed() && A->nb_rows == A->nb_cols && A->window == A->nb_rows && A->nb_rows >= 1,
              EIG_ERR_ARG, "eig_amg_create: square single-rank matrix required");
    eig_ctx_t ctx = A->ctx;
    EIG_HIP(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    // the whole hierarchy on the host first (amg_setup.cpp; a refusal leaves nothing on the device)
    AmgHierarchy H;
    {
      MgCsr h;
      mat_download_bcsr(*A, h.rp, h.col, h.val);
      amg_build(std::move(h), A->nb_rows, theta, H);
    }
    auto *mg = new eig_mg_s();
    try
    {
      mg->ctx = ctx;
      mg->max_cols = max_cols;
      mg->nu = smooth_degree;
      mg->ratio = smooth_ratio;
      const size_t nl = H.A.size();
      mg->lev.reserve(nl);
      for (size_t l = 0; l < nl; ++l)
      {
        mg->lev.emplace_back();
        MgLevel &L = mg->lev.back();
        L.n = H.rows[l];
        L.nnz = (i64)H.A[l].col.size();
        L.lmax = H.lmax[l];
        L.algebraic = true;
        if (l == 0)
          L.A = A;
        else
        {
          eig_mat_t Ac = nullptr;
          const int rc = eig_mat_create_bcsr(ctx, L.n, L.n, 1, 1, H.A[l].rp.data(), H.A[l].col.data(), H.A[l].val.data(), &Ac);
          if (rc != EIG_OK) throw Error(rc, std::string("algebraic multigrid: coarse upload: ") + eig_last_error(ctx));
          L.A = Ac;
          L.own = true;
        }
        alloc_level(L, max_cols, s);
        launch_diag_inv(*L.A, L.dinv->d(), s);
        if (l + 1 < nl)
        {
          L.P.upload(H.P[l]);
          L.PT.upload(H.PT[l]);
        }
        else
        {
          L.clo = H.clo;
          L.chi = H.chi;
          L.cdeg = H.cdeg;
        }
      }
      EIG_HIP(hipStreamSynchronize(s));
    }
    catch (...)
    {
      delete mg;
      throw;
    }
    *out = mg;
  });
}

extern "C" int eig_amg_aggregate(int64_t n, const int64_t *rowptr, const int32_t *col, const double *val, double theta_l,
                                 int64_t *agg, int64_t *naggregates)
{
  return guard(nullptr, [&] {
    EIG_CHECK(n >= 0 && rowptr && agg && naggregates && theta_l >= 0.0 && (n == 0 || rowptr[n] == 0 || (col && val)),
              EIG_ERR_ARG, "eig_amg_aggregate: bad argument");
    for (i64 i = 0; i < n; ++i)
    {
      EIG_CHECK(rowptr[i] <= rowptr[i + 1], EIG_ERR_ARG, "eig_amg_aggregate: row pointers must ascend");
      for (i64 k = rowptr[i]; k < rowptr[i + 1]; ++k)
        EIG_CHECK(col[k] >= 0 && col[k] < n, EIG_ERR_SHAPE, "eig_amg_aggregate: column out of range");
    }
    std::vector<i64> a;
    *naggregates = amg_aggregate(n, rowptr, col, val, theta_l, a);
    std::copy(a.begin(), a.end(), agg);
  });
}

extern "C" int eig_amg_transfer_mv8(eig_ctx_t ctx, int add, int64_t nrows, int64_t ncols, const int64_t *rowptr,
                                    const int32_t *col, const double *val, int64_t m, const double *In, double *Out)
{
  return guard(ctx, [&] {
    EIG_CHECK(ctx && rowptr && In && Out && nrows >= 1 && ncols >= 1 && m > 0 && m % 8 == 0 && m <= 32 && rowptr[0] == 0 &&
                  (rowptr[nrows] == 0 || (col && val)),
              EIG_ERR_ARG, "eig_amg_transfer_mv8: bad argument");
    MgCsr h;
    h.rp.assign(rowptr, rowptr + nrows + 1);
    for (i64 i = 0; i < nrows; ++i) EIG_CHECK(h.rp[i] <= h.rp[i + 1], EIG_ERR_ARG, "eig_amg_transfer_mv8: row pointers must ascend");
    h.col.assign(col, col + h.rp[nrows]);
    h.val.assign(val, val + h.rp[nrows]);
    for (i32 c : h.col) EIG_CHECK(c >= 0 && c < ncols, EIG_ERR_SHAPE, "eig_amg_transfer_mv8: column out of range");
    EIG_HIP(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    AmgCsrDev d;
    try
    {
      d.upload(h);
      if (add)
        launch_amg_prolong_add(nrows, (const i64 *)d.rp->p, (const i32 *)d.col->p, (const double *)d.val->p, m, nrows, ncols,
                               In, Out, s);
      else
        launch_amg_restrict(nrows, (const i64 *)d.rp->p, (const i32 *)d.col->p, (const double *)d.val->p, m, ncols, nrows, In,
                            Out, s);
      EIG_HIP(hipStreamSynchronize(s));
    }
    catch (...)
    {
      d.release();
      throw;
    }
    d.release();
  });
}

extern "C" int eig_mg_level_info(eig_mg_t mg, int level, int64_t *rows, int64_t *nnz, double *lmax)
{
  return guard(mg ? mg->ctx : nullptr, [&] {
    EIG_CHECK(mg && level >= 0 && level < (int)mg->lev.size(), EIG_ERR_ARG, "eig_mg_level_info: no such level");
    const MgLevel &L = mg->lev[level];
    if (rows) *rows = L.n;
    if (nnz) *nnz = L.nnz;
    if (lmax) *lmax = L.lmax;
  });
}

extern "C" int eig_mg_info(eig_mg_t mg, int *levels, int64_t *coarse_rows, int *coarse_degree, double *lmax_fine)
{
  return guard(mg ? mg->ctx : nullptr, [&] {
    EIG_CHECK(mg, EIG_ERR_ARG, "eig_mg_info: null handle");
    if (levels) *levels = (int)mg->lev.size();
    if (coarse_rows) *coarse_rows = mg->lev.back().n;
    if (coarse_degree) *coarse_degree = mg->lev.back().cdeg;
    if (lmax_fine) *lmax_fine = mg->lev.front().lmax;
  });
}

extern "C" int eig_mg_solve(eig_mg_t mg, int64_t m, const double *B, double *X, int cycles, double *resid_host)
{
  return guard(mg ? mg->ctx : nullptr, [&] {
    EIG_CHECK(mg && B && X, EIG_ERR_ARG, "eig_mg_solve: null argument");
    EIG_CHECK(X != B, EIG_ERR_ARG, "eig_mg_solve: X must not alias B");
    eig_ctx_t ctx = mg->ctx;
    EIG_HIP(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    mg_apply(*mg, m, B, X, cycles);
    if (resid_host)
    {
      // max over columns of ||B - A X|| / ||B||
      MgLevel &L = mg->lev[0];
      double *T = L.T->d();
      double *dp = (double *)ctx_buffer(ctx, kSlotMgResidDots, (size_t)2 * m * sizeof(double));
      launch_resid_mv8(*L.A, m, X, B, T, s);
      launch_dot_diag_mv8(L.n, m, T, T, dp, 0, s, ctx->red);
      launch_dot_diag_mv8(L.n, m, B, B, dp + m, 0, s, ctx->red);
      std::vector<double> h((size_t)2 * m);
      download(h, dp, s);
      double r = 0.0;
      for (i64 j = 0; j < m; ++j) r = std::max(r, h[j] > 0.0 ? std::sqrt(h[j] / std::max(h[m + j], 1e-300)) : 0.0);
      *resid_host = r;
    }
    EIG_HIP(hipStreamSynchronize(s));
  });
}

extern "C" int eig_mg_destroy(eig_mg_t mg)
{
  if (!mg) return EIG_OK;
  (void)hipSetDevice(mg->ctx->device);
  (void)hipStreamSynchronize(mg->ctx->stream);
  delete mg;
  return EIG_OK;
}
