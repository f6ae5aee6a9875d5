// subspace.cpp -- the launching half of what the block eigensolvers share (subspace.h): the Chebyshev-Jacobi
// solve, CholQR2 in the M-inner product, the small transfers and read-backs around them, and the C entry
// points of the mass solve and the two panel kernels.
#include <algorithm>
#include <cmath>

#include "subspace.h"

namespace eigmi {

void halo_mv(const eig_mat_s &A, double *X, i64 m, hipStream_t s)
{
  if (!A.ctx->distributed()) return;
  for (i64 c = 0; c < m / 8; ++c) halo_exchange(A, X + c * A.window * 8, s, nullptr, 8);
}

double *cheb_solve(eig_mat_s &M, i64 m, int degree, double lmin, double lmax, const double *Bv, const double *dinv,
                   double *Xa, double *Xb, double *Xc, hipStream_t s)
{
  // scalar rows; ld and own are scalar units already.  Square blocks 2..4 (one rank) take the in-place
  // two-buffer branch below: the box kernels are 1x1 images
  const bool blocked = M.br > 1 || M.bc > 1;
  const i64 n = M.nb_rows * M.br, ld = M.window, own = M.own_offset;
  const ChebJacobi cj(lmin, lmax);
  const double gamma = cj.gamma;
  double omega = cj.omega1();
  // Row-class image (one rank): x_1 = gamma D^-1 b is never stored -- the first step forms it while
  // b's planes enter the LDS ring (x_2 straight from b), the second forms x_{k-1} = x_1 from the
  // row's b.  Same arithmetic as the k_cheb_init + box-step chain below.
  if (degree >= 2 && Xc && !blocked && !M.ctx->distributed() && launch_box_cheb_first(M, m, Bv, omega, gamma, Xa, s))
  {
    if (degree == 2) return Xa;
    omega = cj.next(omega);
    EIG_CHECK(launch_box_cheb_second(M, m, Xa, Bv, omega, gamma, Xc, s), EIG_ERR_ARG,
              "Chebyshev: second row-class step refused");
    double *x2 = Xa;
    Xa = Xc;  // x_3
    Xc = Xb;
    Xb = x2;
    for (int k = 3; k < degree; ++k)
    {
      omega = cj.next(omega);
      launch_box_cheb(M, m, Xa, Xb, Bv, dinv, omega, gamma, s, Xc);  // Xc = x_{k+1}
      double *t = Xb;
      Xb = Xa;
      Xa = Xc;
      Xc = t;
    }
    return Xa;
  }
  launch_cheb_init(n, ld, own, m, Bv, dinv, gamma, Xa, s);
  if (degree <= 1) return Xa;
  const bool oop = Xc && !blocked && m % 32 == 0 && box_prepare(M);
  // x_0 = 0: the box kernel (a third output buffer) takes it as "not read"; the in-place kernels
  // read a cleared buffer
  if (!oop) EIG_HIP(hipMemsetAsync(Xb, 0, (size_t)ld * m * sizeof(double), s));
  for (int k = 1; k < degree; ++k)
  {
    if (k > 1) omega = cj.next(omega);
    halo_mv(M, Xa, m, s);
    if (oop)
    {
      launch_box_cheb(M, m, Xa, k == 1 ? nullptr : Xb, Bv, dinv, omega, gamma, s, Xc);  // Xc = x_{k+1}
      double *t = Xb;
      Xb = Xa;
      Xa = Xc;
      Xc = t;
    }
    else
    {
      launch_cheb_step(M, m, Xa, Xb, Bv, dinv, omega, gamma, s);
      std::swap(Xa, Xb);
    }
  }
  return Xa;
}

bool mcholqr2_mv(const CholQr2 &q, double *Z, double *Vdst, std::vector<double> &Rtot, long long &recomputed)
{
  eig_ctx_t ctx = q.ctx;
  hipStream_t s = ctx->stream;
  const int b = q.b;
  const i64 n = q.n, ld = q.ld, own = q.own;
  // M = I: M Z is Z itself, nothing to form or to carry
  double *MZ = q.M ? q.MZ : Z;
  double *Gd = q.small;
  double *Sd = Gd + (size_t)b * b;
  double *Rd = q.chol, *Rt = Rd + (size_t)b * b;
  int *flag = reinterpret_cast<int *>(Rt + (size_t)b * b);
  EIG_HIP(hipMemsetAsync(flag, 0, sizeof(int), s));
  if (q.M)
  {
    halo_mv(*q.M, Z, b, s);
    launch_spmm_mv8(*q.M, b, Z, MZ, s);
  }
  launch_panel_gram(ctx, n, ld, b, b, Z + own * 8, MZ + own * 8, Gd, s);
  allreduce_sum(ctx, Gd, (i64)b * b, s);
  launch_chol_small(b, 0, Gd, Rd, Sd, Rt, flag, s);  // Sd = R0^-1, Rt = R0
  // The second pass may reuse M Z updated by the same factor (row-local: M (Z R0^-1) = (M Z) R0^-1 up
  // to rounding) instead of a second M SpMM -- but that rounding gap is ~eps cond(Z), so for an
  // ill-conditioned block the second pass would no longer restore M-orthonormality to ~eps (CholQR2's
  // guarantee).  R0's diagonal decides (one small read-back): beyond kCholQrReuseCond the second pass
  // recomputes M (Z R0^-1).
  std::vector<double> r0((size_t)b * b);
  download(r0, Rd, s);
  const bool reuse = cholqr_reuse(b, r0);
  recomputed += !reuse && q.M;
  if (reuse && b == 32 && q.M && !q.finish_mz)
  {
    // Z <- Z R0^-1 and the second pass's Gram (Z R0^-1)^T (M Z R0^-1) in one pass over Z and M Z
    // (k_cholqr_fold): M Z R0^-1 is never stored, Z R0^-1 is not read back
    launch_cholqr_fold(ctx, n, ld, Z + own * 8, MZ + own * 8, Sd, Gd, s);
  }
  else
  {
    launch_panel_update(n, ld, ld, b, b, Z + own * 8, Sd, 1.0, 0.0, Z + own * 8, s);
    if (q.M)
    {
      if (reuse)
        launch_panel_update(n, ld, ld, b, b, MZ + own * 8, Sd, 1.0, 0.0, MZ + own * 8, s);
      else
      {
        halo_mv(*q.M, Z, b, s);
        launch_spmm_mv8(*q.M, b, Z, MZ, s);
      }
    }
    launch_panel_gram(ctx, n, ld, b, b, Z + own * 8, MZ + own * 8, Gd, s);
  }
  allreduce_sum(ctx, Gd, (i64)b * b, s);
  launch_chol_small(b, 1, Gd, Rd, Sd, Rt, flag, s);  // Sd = R1^-1, Rt <- R1 R0
  launch_panel_update(n, ld, ld, b, b, Z + own * 8, Sd, 1.0, 0.0, Vdst + own * 8, s);
  // the caller carries M Vdst: the same factor on M Z (row-local, as above)
  if (q.finish_mz && q.M) launch_panel_update(n, ld, ld, b, b, MZ + own * 8, Sd, 1.0, 0.0, MZ + own * 8, s);
  Rtot.assign((size_t)b * b, 0.0);
  int hflag = 0;
  EIG_HIP(hipMemcpyAsync(Rtot.data(), Rt, Rtot.size() * sizeof(double), hipMemcpyDeviceToHost, s));
  EIG_HIP(hipMemcpyAsync(&hflag, flag, sizeof(int), hipMemcpyDeviceToHost, s));
  EIG_HIP(hipStreamSynchronize(s));
  return !hflag;
}

void upload(const std::vector<double> &h, double *d, hipStream_t s)
{
  EIG_HIP(hipMemcpyAsync(d, h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice, s));
  EIG_HIP(hipStreamSynchronize(s));
}

void download(std::vector<double> &h, const double *d, hipStream_t s)
{
  EIG_HIP(hipMemcpyAsync(h.data(), d, h.size() * sizeof(double), hipMemcpyDeviceToHost, s));
  EIG_HIP(hipStreamSynchronize(s));
}

// (delegating: the holder is complete before the loop, so a failed creation still destroys the events made)
TimingEvents::TimingEvents(size_t count) : TimingEvents()
{
  ev.reserve(count);
  for (size_t i = 0; i < count; ++i)
  {
    hipEvent_t e;
    EIG_HIP(hipEventCreate(&e));
    ev.push_back(e);
  }
}

TimingEvents::~TimingEvents()
{
  for (auto &e : ev) (void)hipEventDestroy(e);
}

void small_ritz(int N, const double *Hdev, int m, int which, std::vector<double> &theta, std::vector<double> &Cx,
                hipStream_t s)
{
  std::vector<double> H((size_t)N * N);
  download(H, Hdev, s);
  ritz_select(N, H, m, which, theta, Cx);
}

void residual_sums(eig_ctx_t ctx, i64 n, i64 ld, i64 m, const double *KX, const double *MX, const double *theta_d,
                   double *dst, double *sums_d, std::vector<double> &sums, hipStream_t s)
{
  launch_lobpcg_resid(ctx, n, ld, m, KX, MX, theta_d, dst, sums_d, s);
  sums.resize((size_t)2 * m);
  download(sums, sums_d, s);
}

void copy_evecs(eig_ctx_t ctx, const double *Q, i64 ld, i64 own, i64 n, int nev, const int *cols, const double *scale,
                double *evec_host)
{
  if (!evec_host) return;
  int last = nev - 1;
  for (int q = 0; cols && q < nev; ++q) last = std::max(last, cols[q]);
  std::vector<double> h((size_t)(last / 8 + 1) * ld * 8);  // the column blocks up to the last column wanted
  download(h, Q, ctx->stream);
  for (int q = 0; q < nev; ++q)
    mv8_column(h.data(), ld, own, n, cols ? cols[q] : q, scale ? scale[q] : 1.0, evec_host + (size_t)q * n);
}

void random_block(eig_ctx_t ctx, i64 n, i64 m, unsigned seed, double *Q)
{
  std::vector<double> h((size_t)(n * m));
  host_random_normal(n * m, seed, h.data());
  upload(h, Q, ctx->stream);
}

void check_square_single_rank(const eig_mat_s *A, const char *who, const char *blocks_text, bool sell_r1)
{
  EIG_CHECK(!A->ctx->distributed(), EIG_ERR_ARG, std::string(who) + ": one rank only");
  EIG_CHECK(A->br == A->bc && A->br >= 1 && A->br <= 4, EIG_ERR_BLOCKSIZE, std::string(who) + blocks_text);
  const i64 n = A->nb_rows * A->br;
  EIG_CHECK(A->nb_rows_global == A->nb_cols && A->nb_rows == A->nb_rows_global && A->window == n &&
                A->own_offset == 0 && (!sell_r1 || A->R == 1),
            EIG_ERR_SHAPE, std::string(who) + ": square single-rank matrix required");
}

}  // namespace eigmi

using namespace eigmi;

// M^-1 B by the Chebyshev-Jacobi semi-iteration (the block Lanczos operator's inner solve).
extern "C" int eig_mass_solve_mv8(eig_mat_t M, int64_t m, int degree, double lmin, double lmax, const double *B,
                                  double *X)
{
  return guard(M ? M->ctx : nullptr, [&] {
    EIG_CHECK(M && B && X && m > 0 && m % 8 == 0 && degree >= 1 && lmin > 0.0 && lmax > lmin, EIG_ERR_ARG,
              "eig_mass_solve_mv8: bad argument");
    EIG_CHECK(M->br == M->bc && M->br >= 1 && M->br <= 4 && M->nb_rows_global == M->nb_cols &&
                  (M->br == 1 || !M->ctx->distributed()),
              EIG_ERR_BLOCKSIZE,
              "eig_mass_solve_mv8: square matrix of FieldMatrix<double,b,b>, b = 1..4 (b > 1: one rank)");
    EIG_CHECK(X != B, EIG_ERR_ARG, "eig_mass_solve_mv8: X must not alias B (B is read by every step)");
    eig_ctx_t ctx = M->ctx;
    EIG_HIP(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const size_t bytes = (size_t)M->window * m * sizeof(double);
    DevBuf dinv((size_t)std::max<i64>(M->nb_rows * M->br, 1) * sizeof(double)), Xb(bytes), Xc(bytes);
    launch_diag_inv(*M, dinv.d(), s);
    EIG_HIP(hipMemsetAsync(X, 0, bytes, s));
    double *res = cheb_solve(*M, m, degree, lmin, lmax, B, dinv.d(), X, Xb.d(), Xc.d(), s);
    if (res != X) EIG_HIP(hipMemcpyAsync(X, res, bytes, hipMemcpyDeviceToDevice, s));
    EIG_HIP(hipStreamSynchronize(s));
  });
}

extern "C" int eig_panel_update_mv8(eig_ctx_t ctx, int64_t n, int64_t m1, int64_t m2, const double *Q, const double *S,
                                    double alpha, double beta, double *Y)
{
  return guard(ctx, [&] {
    EIG_CHECK(ctx && Q && S && Y && n >= 0 && m1 >= 0 && m1 % 8 == 0 && m2 % 8 == 0 && m2 >= 8 && m2 <= 32,
              EIG_ERR_ARG, "eig_panel_update_mv8: m1 % 8 == 0, m2 in {8,16,24,32}");
    EIG_HIP(hipSetDevice(ctx->device));
    launch_panel_update(n, n, n, m1, m2, Q, S, alpha, beta, Y, ctx->stream);
  });
}

extern "C" int eig_panel_gram_mv8(eig_ctx_t ctx, int64_t n, int64_t m1, int64_t m2, const double *Q1, const double *Q2,
                                  double *G)
{
  return guard(ctx, [&] {
    EIG_CHECK(ctx && Q1 && Q2 && G && n >= 0 && m1 > 0 && m2 > 0 && m1 % 8 == 0 && m2 % 8 == 0, EIG_ERR_ARG,
              "eig_panel_gram_mv8: bad argument");
    EIG_HIP(hipSetDevice(ctx->device));
    launch_panel_gram(ctx, n, n, m1, m2, Q1, Q2, G, ctx->stream);
  });
}
