// slice.cpp -- interior eigenpairs of a symmetric A in a window [a, b] by Chebyshev-filtered subspace
// iteration, one rank, and the filter's own entry points.
//
// Filter (filter_host.h): p(A) X for the Jackson-damped Chebyshev expansion p of the window's indicator,
// evaluated by Clenshaw in `degree` fused product steps (launch_filt_step): step k gathers b_{k+1}, reads X
// and overwrites b_{k+2} with b_k, so two n x m panels alternate and b_d = gamma_d X is never formed.
//
// Driver state: X (n x m Ritz vectors, orthonormal), and three more panels Y, W, AX.  One iteration:
//   1. Y = p(A) X                                   (degree launches of the filter step; W is its second panel)
//   2. CholQR2 of Y in place (mcholqr2_mv, M = I)   a non-positive pivot: EIG_ERR_BREAKDOWN
//   3. W = A Y, H = Y^T W (panel Gram), symmetrised, sym_eig on the host: theta ascending, S
//   4. X = Y S, AX = W S (panel updates)
//   5. Y = AX - X diag(theta) with the column sums ||r_j||^2, ||x_j||^2 (k_lobpcg_resid, MX = X)
// The pairs with theta in [a, b] are accepted; the step stops when there is at least one and every one has
// ||r_j|| <= tol max(|theta_j|, |a|, |b|) ||x_j|| (subspace_host.h window_converged).  CholQR2, the small
// Rayleigh-Ritz read-back, the residual sums and the eigenvector copy-out are subspace.h's.
#include <cmath>
#include <cstring>
#include <vector>

#include "filter_host.h"
#include "subspace.h"

using namespace eigmi;

struct eig_slice_s {
  eig_mat_s *A = nullptr;
  int m = 8;
  i64 n = 0;
  double a = 0.0, b = 0.0;
  FilterWindow win;
  std::vector<double> gamma;  // gamma_0 .. gamma_d
  std::vector<double> theta, rr, xx;  // Ritz values (ascending), ||r_j||^2, ||x_j||^2 of the last iteration
  long long iters = 0, cholqr_recomputed = 0;
  DevBuf *X = nullptr, *Y = nullptr, *W = nullptr, *AX = nullptr, *small = nullptr, *chol = nullptr;
  ~eig_slice_s()
  {
    for (DevBuf *d : {X, Y, W, AX, small, chol}) delete d;
  }
  size_t panel() const { return (size_t)n * m; }
  // small: [H m^2][S m^2][cholqr 2 m^2][theta m][sums 2 m]
  double *Hd() const { return small->d(); }
  double *Sd() const { return Hd() + (size_t)m * m; }
  double *Qd() const { return Sd() + (size_t)m * m; }
  double *theta_d() const { return Qd() + (size_t)2 * m * m; }
  double *sums_d() const { return theta_d() + m; }
  int degree() const { return (int)gamma.size() - 1; }
};

namespace {

void check_filter_matrix(const eig_mat_s *A, const char *who)
{
  check_square_single_rank(A, who, ": 1x1 blocks or square blocks FieldMatrix<double,b,b> with b = 2..4", true);
}

// Y = p(A) X: step k (k = d - 1 .. 0) writes panel (d - 1 - k) % 2 of {P0, P1}, chosen so that the last
// step (k = 0) lands in Y.  X, Y, W distinct; returns the number of kernel launches.
long long apply_filter(const eig_mat_s &A, i64 m, const std::vector<double> &gamma, const FilterWindow &win,
                       const double *X, double *Y, double *W, hipStream_t s)
{
  const int d = (int)gamma.size() - 1;
  double *P[2];
  P[(d - 1) % 2] = Y;
  P[d % 2] = W;
  const double *cur = X;
  for (int k = d - 1; k >= 0; --k)
  {
    double *out = P[(d - 1 - k) % 2];
    const FiltScalars f = filter_step_scalars(gamma, win, k);
    launch_filt_step(A, m, cur, out, X, f.s1, f.s0, f.s2, f.g, s);
    cur = out;
  }
  return (long long)d * filt_step_launches(A, m);
}

bool cholqr(eig_slice_s &w, double *Z)
{
  const CholQr2 q = cholqr_args(w.A->ctx, nullptr, w.m, w.n, w.n, 0, nullptr, w.Qd(), w.chol->d(), false);
  std::vector<double> R;
  return mcholqr2_mv(q, Z, Z, R, w.cholqr_recomputed);
}

// R = AXp - X diag(theta) into `dst`, the column sums to the host
void residual(eig_slice_s &w, const double *AXp, double *dst, hipStream_t s)
{
  std::vector<double> sums;
  residual_sums(w.A->ctx, w.n, w.n, w.m, AXp, w.X->d(), w.theta_d(), dst, w.sums_d(), sums, s);
  w.rr.assign(sums.begin(), sums.begin() + w.m);
  w.xx.assign(sums.begin() + w.m, sums.end());
}

bool accepted(const eig_slice_s &w, int j) { return window_accept(w.theta[j], w.a, w.b); }

int in_window(const eig_slice_s &w)
{
  int c = 0;
  for (int j = 0; j < w.m; ++j) c += accepted(w, j);
  return c;
}

bool all_converged(const eig_slice_s &w, double tol) { return window_converged(w.theta, w.rr, w.xx, w.a, w.b, tol); }

long long iterate(eig_slice_s &w, hipEvent_t *e)
{
  eig_ctx_t ctx = w.A->ctx;
  hipStream_t s = ctx->stream;
  const int m = w.m;
  const i64 n = w.n;
  double *X = w.X->d(), *Y = w.Y->d(), *W = w.W->d(), *AX = w.AX->d();
  EIG_HIP(hipEventRecord(e[0], s));
  const long long launches = apply_filter(*w.A, m, w.gamma, w.win, X, Y, W, s);
  EIG_HIP(hipEventRecord(e[1], s));
  EIG_CHECK(cholqr(w, Y), EIG_ERR_BREAKDOWN,
            "eig_slice_step: the filtered block has no positive-definite Gram (CholQR2 pivot <= 0)");
  EIG_HIP(hipEventRecord(e[2], s));
  launch_spmm_mv8(*w.A, m, Y, W, s);
  launch_panel_gram(ctx, n, n, m, m, Y, W, w.Hd(), s);
  std::vector<double> S;
  small_ritz(m, w.Hd(), m, EIG_WHICH_SA, w.theta, S, s);  // theta ascending, column j of S = eigenvector j
  upload(S, w.Sd(), s);
  launch_panel_update(n, n, n, m, m, Y, w.Sd(), 1.0, 0.0, X, s);
  launch_panel_update(n, n, n, m, m, W, w.Sd(), 1.0, 0.0, AX, s);
  upload(w.theta, w.theta_d(), s);
  EIG_HIP(hipEventRecord(e[3], s));
  residual(w, AX, Y, s);
  EIG_HIP(hipEventRecord(e[4], s));
  return launches;
}

}  // namespace

extern "C" int eig_filter_degree(double a, double b, double lmin, double lmax, int degree, int *degree_out)
{
  return guard(nullptr, [&] {
    EIG_CHECK(degree >= 0 && degree_out, EIG_ERR_ARG, "eig_filter_degree: degree >= 2, or 0 for the default");
    std::vector<double> g;
    *degree_out = filter_coefs(a, b, lmin, lmax, degree, g);
  });
}

extern "C" int eig_filter_coefs(double a, double b, double lmin, double lmax, int degree, double *gamma_host)
{
  return guard(nullptr, [&] {
    EIG_CHECK(degree >= 0 && gamma_host, EIG_ERR_ARG, "eig_filter_coefs: degree >= 2, or 0 for the default");
    std::vector<double> g;
    filter_coefs(a, b, lmin, lmax, degree, g);
    std::memcpy(gamma_host, g.data(), g.size() * sizeof(double));
  });
}

extern "C" int eig_filter_step_mv8(eig_mat_t A, int64_t m, const double *Xk, double *Xold, const double *B,
                                   double s1, double s0, double s2, double g)
{
  return guard(A ? A->ctx : nullptr, [&] {
    EIG_CHECK(A && Xk && Xold && B, EIG_ERR_ARG, "eig_filter_step_mv8: null argument");
    EIG_CHECK(m >= 0 && m % 8 == 0, EIG_ERR_ARG, "eig_filter_step_mv8: m must be a multiple of 8");
    check_filter_matrix(A, "eig_filter_step_mv8");
    DeviceGuard dg(A->ctx->device);
    if (m > 0) launch_filt_step(*A, m, Xk, Xold, B, s1, s0, s2, g, A->ctx->stream);
  });
}

extern "C" int eig_filter_mv8(eig_mat_t A, int64_t m, double a, double b, double lmin, double lmax, int degree,
                              const double *X, double *Y, double *work)
{
  return guard(A ? A->ctx : nullptr, [&] {
    EIG_CHECK(A && X && Y && work && X != Y && X != work && Y != work, EIG_ERR_ARG,
              "eig_filter_mv8: X, Y and work must be three distinct panels");
    EIG_CHECK(m >= 0 && m % 8 == 0 && degree >= 0, EIG_ERR_ARG,
              "eig_filter_mv8: m a multiple of 8, degree >= 2 or 0 for the default");
    check_filter_matrix(A, "eig_filter_mv8");
    std::vector<double> gamma;
    filter_coefs(a, b, lmin, lmax, degree, gamma);
    const FilterWindow win = filter_window(a, b, lmin, lmax);
    DeviceGuard dg(A->ctx->device);
    if (m > 0) apply_filter(*A, m, gamma, win, X, Y, work, A->ctx->stream);
  });
}

extern "C" int eig_spectrum_bounds(eig_mat_t A, int steps, unsigned seed, double *lmin, double *lmax)
{
  return guard(A ? A->ctx : nullptr, [&] {
    EIG_CHECK(A && lmin && lmax && steps >= 1, EIG_ERR_ARG, "eig_spectrum_bounds: steps >= 1 required");
    eig_ctx_t ctx = A->ctx;
    eig_lanczos_t ws = nullptr;
    // (the workspace entry points set the context's error themselves: pass their status on)
    int rc = eig_lanczos_create(A, steps, nullptr, seed, &ws);
    if (rc != EIG_OK) throw Error(rc, ctx->last_error);
    std::vector<double> alpha((size_t)steps), beta((size_t)steps + 1);
    int k = 0;
    rc = eig_lanczos_step(ws, steps, 0, nullptr);
    if (rc == EIG_OK) rc = eig_lanczos_tridiag(ws, &k, alpha.data(), beta.data());
    const std::string msg = ctx->last_error;
    (void)eig_lanczos_destroy(ws);
    if (rc != EIG_OK) throw Error(rc, msg);
    EIG_CHECK(k >= 1, EIG_ERR_BREAKDOWN, "eig_spectrum_bounds: no Lanczos step was taken");
    lanczos_bounds(k, alpha.data(), beta.data(), *lmin, *lmax);
  });
}

extern "C" int eig_filter_count(eig_mat_t A, double a, double b, double lmin, double lmax, int degree, int nvec,
                                unsigned seed, double *estimate)
{
  return guard(A ? A->ctx : nullptr, [&] {
    EIG_CHECK(A && estimate && nvec >= 8 && nvec % 8 == 0, EIG_ERR_ARG,
              "eig_filter_count: nvec must be a positive multiple of 8");
    check_filter_matrix(A, "eig_filter_count");
    eig_ctx_t ctx = A->ctx;
    const i64 n = A->nb_rows * A->br;
    DeviceGuard dg(ctx->device);
    DevBuf Z((size_t)n * nvec * sizeof(double)), Y(Z.bytes()), W(Z.bytes()), dp((size_t)nvec * sizeof(double));
    int rc = eig_random_mv8(ctx, n, nvec, seed, Z.d());
    if (rc == EIG_OK) rc = eig_filter_mv8(A, nvec, a, b, lmin, lmax, degree, Z.d(), Y.d(), W.d());
    if (rc == EIG_OK) rc = eig_dot_diag_mv8(ctx, n, nvec, Z.d(), Y.d(), dp.d());
    if (rc != EIG_OK) throw Error(rc, ctx->last_error);
    std::vector<double> h((size_t)nvec);
    download(h, dp.d(), ctx->stream);
    double sum = 0.0;
    for (double v : h) sum += v;
    *estimate = sum / nvec;
  });
}

extern "C" int eig_slice_create(eig_mat_t A, double a, double b, double lmin, double lmax, int block, int degree,
                                const double *X0, unsigned seed, eig_slice_t *out)
{
  return guard(A ? A->ctx : nullptr, [&] {
    EIG_CHECK(A && out && block >= 8 && block <= 32 && block % 8 == 0, EIG_ERR_ARG,
              "eig_slice_create: A, ws and block in {8, 16, 24, 32} required");
    EIG_CHECK(degree >= 0, EIG_ERR_ARG, "eig_slice_create: degree >= 2, or 0 for the default");
    check_filter_matrix(A, "eig_slice_create");
    const i64 n = A->nb_rows * A->br;
    EIG_CHECK((i64)4 * block <= n, EIG_ERR_SHAPE, "eig_slice_create: 4 * block exceeds the matrix size");
    std::vector<double> gamma;
    filter_coefs(a, b, lmin, lmax, degree, gamma);
    eig_ctx_t ctx = A->ctx;
    DeviceGuard dg(ctx->device);
    hipStream_t s = ctx->stream;
    auto *w = new eig_slice_s();
    try
    {
      const int m = block;
      w->A = A;
      w->m = m;
      w->n = n;
      w->a = a;
      w->b = b;
      w->win = filter_window(a, b, lmin, lmax);
      w->gamma = gamma;
      w->theta.assign(m, 0.0);
      const size_t bytes = w->panel() * sizeof(double);
      w->X = new DevBuf(bytes);
      w->Y = new DevBuf(bytes);
      w->W = new DevBuf(bytes);
      w->AX = new DevBuf(bytes);
      w->small = new DevBuf(((size_t)4 * m * m + 3 * m) * sizeof(double));
      w->chol = new DevBuf((size_t)2 * m * m * sizeof(double) + 64);
      if (X0)
        EIG_HIP(hipMemcpyAsync(w->X->d(), X0, bytes, hipMemcpyDeviceToDevice, s));
      else
        random_block(ctx, n, m, seed, w->X->d());
      EIG_CHECK(cholqr(*w, w->X->d()), EIG_ERR_BREAKDOWN, "eig_slice_create: the start block is not of full rank");
    }
    catch (...)
    {
      delete w;
      throw;
    }
    *out = w;
  });
}

extern "C" int eig_slice_step(eig_slice_t w, int max_iters, double tol, int *iters_done, int *converged,
                              eig_slice_timing *timing)
{
  return guard(w ? w->A->ctx : nullptr, [&] {
    EIG_CHECK(w && max_iters >= 0 && tol >= 0.0, EIG_ERR_ARG, "eig_slice_step: max_iters >= 0, tol >= 0 required");
    eig_ctx_t ctx = w->A->ctx;
    DeviceGuard dg(ctx->device);
    hipStream_t s = ctx->stream;
    TimingEvents ev(5);
    if (iters_done) *iters_done = 0;
    if (converged) *converged = 0;
    if (timing) std::memset(timing, 0, sizeof(*timing));
    int it = 0;
    long long launches = 0;
    // (a workspace that already meets the tolerance takes no iteration)
    bool conv = tol > 0.0 && all_converged(*w, tol);
    while (!conv && it < max_iters)
    {
      launches += iterate(*w, ev.data());
      ++w->iters;
      ++it;
      if (iters_done) *iters_done = it;
      if (timing)
      {
        EIG_HIP(hipEventSynchronize(ev[4]));
        float t[4];
        for (int q = 0; q < 4; ++q) EIG_HIP(hipEventElapsedTime(&t[q], ev[q], ev[q + 1]));
        timing->filter_ms += t[0];
        timing->orth_ms += t[1];
        timing->rr_ms += t[2];
        timing->resid_ms += t[3];
        timing->total_ms += t[0] + t[1] + t[2] + t[3];
      }
      conv = tol > 0.0 && all_converged(*w, tol);
    }
    EIG_HIP(hipStreamSynchronize(s));
    if (converged) *converged = conv ? 1 : 0;
    if (timing)
    {
      timing->iters = it;
      timing->filter_launches = launches;
      timing->degree = w->degree();
      timing->in_window = w->rr.empty() ? 0 : in_window(*w);
      timing->saturated = !w->rr.empty() && in_window(*w) == w->m ? 1 : 0;
      timing->cholqr_recomputed = w->cholqr_recomputed;
    }
  });
}

extern "C" int eig_slice_ritz(eig_slice_t w, int *count, double *eval_host, double *evec_host, double *resid_host)
{
  return guard(w ? w->A->ctx : nullptr, [&] {
    EIG_CHECK(w && count, EIG_ERR_ARG, "eig_slice_ritz: ws and count required");
    eig_ctx_t ctx = w->A->ctx;
    DeviceGuard dg(ctx->device);
    hipStream_t s = ctx->stream;
    const int m = w->m;
    const i64 n = w->n;
    std::vector<int> idx;
    if (!w->rr.empty())
      for (int j = 0; j < m; ++j)
        if (accepted(*w, j)) idx.push_back(j);
    *count = (int)idx.size();
    if (idx.empty()) return;
    if (eval_host)
      for (size_t q = 0; q < idx.size(); ++q) eval_host[q] = w->theta[idx[q]];
    if (resid_host)
    {
      // fresh products (W and Y are scratch between iterations), not the carried A X
      launch_spmm_mv8(*w->A, m, w->X->d(), w->W->d(), s);
      residual(*w, w->W->d(), w->Y->d(), s);
      for (size_t q = 0; q < idx.size(); ++q) resid_host[q] = std::sqrt(w->rr[idx[q]]);
    }
    copy_evecs(ctx, w->X->d(), n, 0, n, (int)idx.size(), idx.data(), nullptr, evec_host);
  });
}

extern "C" int eig_slice_destroy(eig_slice_t w)
{
  return w ? destroy_workspace(w, w->A->ctx) : EIG_OK;
}
