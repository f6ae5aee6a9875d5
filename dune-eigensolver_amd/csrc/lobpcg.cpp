// lobpcg.cpp -- LOBPCG for the symmetric-definite pencil K x = lambda M x (M = NULL: M = I), the
// smallest (or, without a preconditioner, largest) end, one rank.
//
// State: three multivectors S = [X | W | P], KS and MS (n x 3 m each, MultiVector<double,8>
// layout, so X, W and P are slices of m / 8 column blocks and one panel call sees all of S; M = NULL:
// MS is S) and the Ritz values theta[m].  S is M-orthonormal at every Rayleigh-Ritz, so the small
// problem is a standard one and X' = S C_x, P' = S C_p with orthonormal [C_x C_p] need no further
// device pass.  One iteration:
//   1. R = KX - MX diag(theta) and the column sums ||r_j||^2, ||(MX)_j||^2 (k_lobpcg_resid); the host
//      tests ||r_j|| <= tol |theta_j| ||M x_j|| for j < nev
//   2. W = T R: none, `degree` Chebyshev-Jacobi steps on A_p (cheb_solve), or `cycles` multigrid
//      iterations (mg_apply) -- a search direction only, so its accuracy does not enter the answer
//   3. two classical Gram-Schmidt passes of W against [X P] in the M-inner product with the carried
//      MX, MP (panel Gram + panel update; no M SpMM)
//   4. M-CholQR2 of W (subspace.h mcholqr2_mv; M W carried out of it), K W
//   5. H = S^T K S (panel Gram), symmetrised, sym_eig on the host: C_x = the m wanted eigenvectors (small_ritz)
//   6. C_p = C_x with its X rows zeroed, orthogonalised twice against C_x, Householder QR
//      (subspace_host.h search_coefficients)
//   7. [X' P'] = S [C_x C_p] on S, KS and MS (k_lobpcg_update)
// A non-positive pivot in 4., or an S that is not M-orthonormal to kOrthTol after 4. (checked by one panel
// Gram S^T M S), redoes the iteration without P; without P it is EIG_ERR_BREAKDOWN.
// The transfers, read-backs and checks shared with block Lanczos and slicing are subspace.h's, the host
// arithmetic of 1., 5., 6. and the orthonormality test subspace_host.h's.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "subspace.h"

using namespace eigmi;

enum { kPrecNone = 0, kPrecCheb = 1, kPrecMg = 2 };
// max |S^T M S - I| an iteration may enter its Rayleigh-Ritz with: CholQR2 delivers ~1e-14, and a deviation
// shows at its own size in the Ritz values, which the tests hold to 1e-10
constexpr double kOrthTol = 1e-10;

struct eig_lobpcg_s {
  eig_mat_s *K = nullptr, *M = nullptr;
  int m = 8, which = EIG_WHICH_SA;
  i64 n = 0;  // scalar rows = leading dimension of every multivector (one rank: window = n, own = 0)
  int prec = kPrecNone;
  eig_mat_s *Ap = nullptr;
  int degree = 0, cycles = 0;
  double lmin = 0.0, lmax = 0.0;
  eig_mg_s *mg = nullptr;
  bool has_p = false;
  long long iters = 0, cholqr_recomputed = 0, p_dropped = 0, orth_rejected = 0;
  double orth_dev = 0.0;  // largest accepted max |S^T M S - I|
  std::vector<double> theta;
  DevBuf *S = nullptr, *KS = nullptr, *MS = nullptr;
  DevBuf *Rb = nullptr, *Ta = nullptr, *Tb = nullptr, *dinv = nullptr;  // preconditioner input and scratch
  DevBuf *small = nullptr;  // Gram panels, coefficients, theta, sums
  DevBuf *chol = nullptr;
  ~eig_lobpcg_s()
  {
    for (DevBuf *d : {S, KS, MS, Rb, Ta, Tb, dinv, small, chol}) delete d;
  }
  size_t slice() const { return (size_t)n * m; }  // doubles per slice
  double *X(DevBuf *f) const { return f->d(); }
  double *W(DevBuf *f) const { return f->d() + slice(); }
  double *P(DevBuf *f) const { return f->d() + 2 * slice(); }
  DevBuf *MSf() const { return M ? MS : S; }
  // small: [H 9 m^2][C 6 m^2][G 2 m^2][cholqr 2 m^2][theta m][sums 2 m]
  double *Hd() const { return small->d(); }
  double *Cd() const { return Hd() + (size_t)9 * m * m; }
  double *Gd() const { return Cd() + (size_t)6 * m * m; }
  double *Qd() const { return Gd() + (size_t)2 * m * m; }
  double *theta_d() const { return Qd() + (size_t)2 * m * m; }
  double *sums_d() const { return theta_d() + m; }
};

namespace {

bool cholqr(eig_lobpcg_s &w, double *Z, double *MZ)
{
  const CholQr2 q = cholqr_args(w.K->ctx, w.M, w.m, w.n, w.n, 0, MZ, w.Qd(), w.chol->d(), true);
  std::vector<double> R;
  return mcholqr2_mv(q, Z, Z, R, w.cholqr_recomputed);
}

// R = KX - MX diag(theta) into `dst`; sums[j] = ||r_j||^2, sums[m + j] = ||(MX)_j||^2 on the host
void residual(eig_lobpcg_s &w, const double *KX, const double *MX, double *dst, std::vector<double> &sums,
              hipStream_t s)
{
  residual_sums(w.K->ctx, w.n, w.n, w.m, KX, MX, w.theta_d(), dst, w.sums_d(), sums, s);
}

// where the residual goes: straight into W without a preconditioner, else the preconditioner's input
double *res_buf(const eig_lobpcg_s &w) { return w.prec == kPrecNone ? w.W(w.S) : w.Rb->d(); }

// Steps 2..7 of one iteration on the residual in res_buf(w); false: the CholQR of W met a
// non-positive pivot, or S = [X W P] is not M-orthonormal to kOrthTol (X, KX, MX and theta are untouched)
bool iterate(eig_lobpcg_s &w, bool use_p, hipEvent_t *e)
{
  eig_ctx_t ctx = w.K->ctx;
  hipStream_t s = ctx->stream;
  const int m = w.m, kb = use_p ? 3 : 2;
  const i64 n = w.n;
  double *Wd = w.W(w.S);
  if (w.prec == kPrecCheb)
  {
    double *r = cheb_solve(*w.Ap, m, w.degree, w.lmin, w.lmax, w.Rb->d(), w.dinv->d(), Wd, w.Ta->d(), w.Tb->d(), s);
    if (r != Wd) EIG_HIP(hipMemcpyAsync(Wd, r, w.slice() * sizeof(double), hipMemcpyDeviceToDevice, s));
  }
  else if (w.prec == kPrecMg)
    mg_apply(*w.mg, m, w.Rb->d(), Wd, w.cycles);
  EIG_HIP(hipEventRecord(e[2], s));
  DevBuf *MSf = w.MSf();
  double *G0 = w.Gd(), *G1 = G0 + (size_t)m * m;
  for (int pass = 0; pass < 2; ++pass)
  {
    launch_panel_gram(ctx, n, n, m, m, w.X(MSf), Wd, G0, s);
    if (use_p) launch_panel_gram(ctx, n, n, m, m, w.P(MSf), Wd, G1, s);
    launch_panel_update(n, n, n, m, m, w.X(w.S), G0, -1.0, 1.0, Wd, s);
    if (use_p) launch_panel_update(n, n, n, m, m, w.P(w.S), G1, -1.0, 1.0, Wd, s);
  }
  if (!cholqr(w, Wd, w.W(MSf))) return false;
  const int N = kb * m;
  {
    // The Rayleigh-Ritz below is a standard eigenproblem only while S^T M S = I: a CholQR2 of a W that is
    // numerically inside span [X P] returns without a failed pivot and leaves S rank deficient, whose
    // null vectors are Ritz vectors of value 0 -- the smallest end would select them and X would collapse.
    // So the invariant is checked (one more panel Gram, with the carried M S) and a miss counts as a
    // failed orthonormalisation.
    launch_panel_gram(ctx, n, n, N, N, w.S->d(), MSf->d(), w.Hd(), s);
    std::vector<double> G((size_t)N * N);
    download(G, w.Hd(), s);
    const double dev = orth_deviation(N, G);
    if (!(dev <= kOrthTol))
    {
      ++w.orth_rejected;
      return false;
    }
    w.orth_dev = std::max(w.orth_dev, dev);
  }
  EIG_HIP(hipEventRecord(e[3], s));
  launch_spmm_mv8(*w.K, m, Wd, w.W(w.KS), s);
  EIG_HIP(hipEventRecord(e[4], s));
  launch_panel_gram(ctx, n, n, N, N, w.S->d(), w.KS->d(), w.Hd(), s);
  std::vector<double> Cx, C;
  small_ritz(N, w.Hd(), m, w.which, w.theta, Cx, s);
  search_coefficients(N, m, Cx, C);
  upload(C, w.Cd(), s);
  launch_lobpcg_update(ctx, n, n, m, kb, w.S->d(), w.KS->d(), w.M ? w.MS->d() : nullptr, w.Cd(), s);
  upload(w.theta, w.theta_d(), s);
  EIG_HIP(hipEventRecord(e[5], s));
  return true;
}

void check_matrix(const eig_mat_s *A, const eig_mat_s *K, const char *what)
{
  EIG_CHECK(A->ctx == K->ctx, EIG_ERR_ARG, std::string(what) + " must share K's context");
  EIG_CHECK(A->br == A->bc && A->br == K->br, EIG_ERR_BLOCKSIZE,
            std::string(what) + " needs K's square blocks, FieldMatrix<double,b,b> with b = 1..4");
  EIG_CHECK(A->nb_rows == K->nb_rows && A->nb_cols == K->nb_cols && A->window == K->window, EIG_ERR_SHAPE,
            std::string(what) + " must have K's rows and columns");
}

}  // namespace

extern "C" int eig_lobpcg_create(eig_mat_t K, eig_mat_t M, int block, int which, const double *X0, unsigned seed,
                                 eig_lobpcg_t *out)
{
  return guard(K ? K->ctx : nullptr, [&] {
    EIG_CHECK(K && out && block >= 8 && block <= 32 && block % 8 == 0, EIG_ERR_ARG,
              "eig_lobpcg_create: K, ws and block in {8, 16, 24, 32} required");
    EIG_CHECK(which == EIG_WHICH_SA || which == EIG_WHICH_LA, EIG_ERR_ARG, "eig_lobpcg_create: bad `which`");
    check_square_single_rank(K, "eig_lobpcg_create", ": square blocks FieldMatrix<double,b,b> with b = 1..4", false);
    if (M) check_matrix(M, K, "eig_lobpcg_create: M");
    const i64 n = K->nb_rows * K->br;
    EIG_CHECK((i64)4 * block <= n, EIG_ERR_SHAPE, "eig_lobpcg_create: 4 * block exceeds the matrix size");
    eig_ctx_t ctx = K->ctx;
    EIG_HIP(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    auto *w = new eig_lobpcg_s();
    try
    {
      const int m = block;
      w->K = K;
      w->M = M;
      w->m = m;
      w->which = which;
      w->n = n;
      const size_t fam = 3 * w->slice() * sizeof(double);
      w->S = new DevBuf(fam);
      w->KS = new DevBuf(fam);
      if (M) w->MS = new DevBuf(fam);
      w->small = new DevBuf(((size_t)19 * m * m + 3 * m) * sizeof(double));
      w->chol = new DevBuf((size_t)2 * m * m * sizeof(double) + 64);
      for (DevBuf *d : {w->S, w->KS, w->MS})
        if (d) EIG_HIP(hipMemsetAsync(d->d(), 0, d->bytes(), s));
      if (X0)
        EIG_HIP(hipMemcpyAsync(w->S->d(), X0, w->slice() * sizeof(double), hipMemcpyDeviceToDevice, s));
      else
        random_block(ctx, n, m, seed, w->S->d());
      EIG_CHECK(cholqr(*w, w->X(w->S), w->X(w->MSf())), EIG_ERR_BREAKDOWN,
                "eig_lobpcg_create: the start block is not of full rank in the M-inner product");
      launch_spmm_mv8(*K, m, w->X(w->S), w->X(w->KS), s);
      launch_panel_gram(ctx, n, n, m, m, w->X(w->S), w->X(w->KS), w->Hd(), s);
      std::vector<double> Cx;
      small_ritz(m, w->Hd(), m, which, w->theta, Cx, s);
      upload(Cx, w->Cd(), s);
      for (DevBuf *d : {w->S, w->KS, w->MS})
        if (d) launch_panel_update(n, n, n, m, m, d->d(), w->Cd(), 1.0, 0.0, d->d(), s);
      upload(w->theta, w->theta_d(), s);
    }
    catch (...)
    {
      delete w;
      throw;
    }
    *out = w;
  });
}

extern "C" int eig_lobpcg_precond_cheb(eig_lobpcg_t w, eig_mat_t Ap, int degree, double lmin, double lmax)
{
  return guard(w ? w->K->ctx : nullptr, [&] {
    EIG_CHECK(w && degree >= 1 && lmin > 0.0 && lmax > lmin, EIG_ERR_ARG,
              "eig_lobpcg_precond_cheb: degree >= 1 and 0 < lmin < lmax required");
    EIG_CHECK(w->which == EIG_WHICH_SA, EIG_ERR_ARG,
              "eig_lobpcg_precond_cheb: a preconditioner serves the smallest end only (EIG_WHICH_SA)");
    if (!Ap) Ap = w->K;
    check_matrix(Ap, w->K, "eig_lobpcg_precond_cheb: Ap");
    eig_ctx_t ctx = w->K->ctx;
    EIG_HIP(hipSetDevice(ctx->device));
    const size_t bytes = w->slice() * sizeof(double);
    if (!w->Rb) w->Rb = new DevBuf(bytes);
    if (!w->Ta) w->Ta = new DevBuf(bytes);
    if (!w->Tb) w->Tb = new DevBuf(bytes);
    if (!w->dinv) w->dinv = new DevBuf((size_t)w->n * sizeof(double));
    launch_diag_inv(*Ap, w->dinv->d(), ctx->stream);
    w->Ap = Ap;
    w->degree = degree;
    w->lmin = lmin;
    w->lmax = lmax;
    w->mg = nullptr;
    w->prec = kPrecCheb;
  });
}

extern "C" int eig_lobpcg_precond_mg(eig_lobpcg_t w, eig_mg_t mg, int cycles)
{
  return guard(w ? w->K->ctx : nullptr, [&] {
    EIG_CHECK(w && mg && cycles >= 1, EIG_ERR_ARG, "eig_lobpcg_precond_mg: mg and cycles >= 1 required");
    EIG_CHECK(w->which == EIG_WHICH_SA, EIG_ERR_ARG,
              "eig_lobpcg_precond_mg: a preconditioner serves the smallest end only (EIG_WHICH_SA)");
    const eig_mat_s *A = mg_matrix(*mg);
    EIG_CHECK(A->ctx == w->K->ctx && A->nb_rows * A->br == w->n && mg_max_cols(*mg) >= w->m, EIG_ERR_ARG,
              "eig_lobpcg_precond_mg: mg must be of K's context and size with max_cols >= block");
    EIG_HIP(hipSetDevice(w->K->ctx->device));
    if (!w->Rb) w->Rb = new DevBuf(w->slice() * sizeof(double));
    w->mg = mg;
    w->cycles = cycles;
    w->prec = kPrecMg;
  });
}

extern "C" int eig_lobpcg_step(eig_lobpcg_t w, int max_iters, int nev, double tol, int *iters_done, int *converged,
                               eig_lobpcg_timing *timing)
{
  return guard(w ? w->K->ctx : nullptr, [&] {
    EIG_CHECK(w && max_iters >= 0 && nev >= 1 && nev <= w->m && tol >= 0.0, EIG_ERR_ARG,
              "eig_lobpcg_step: max_iters >= 0, 1 <= nev <= block, tol >= 0 required");
    eig_ctx_t ctx = w->K->ctx;
    EIG_HIP(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    TimingEvents ev(6);
    if (iters_done) *iters_done = 0;
    if (converged) *converged = 0;
    if (timing) std::memset(timing, 0, sizeof(*timing));
    std::vector<double> sums;
    int it = 0;
    bool conv = false;
    for (;;)
    {
      if (tol == 0.0 && it == max_iters) break;
      EIG_HIP(hipEventRecord(ev[0], s));
      residual(*w, w->X(w->KS), w->X(w->MSf()), res_buf(*w), sums, s);
      EIG_HIP(hipEventRecord(ev[1], s));
      if (tol > 0.0)
      {
        conv = lobpcg_converged(sums, w->theta, w->m, nev, tol);
        if (conv || it == max_iters) break;
      }
      if (!iterate(*w, w->has_p, ev.data()))
      {
        EIG_CHECK(w->has_p, EIG_ERR_BREAKDOWN,
                  "LOBPCG: W has no positive-definite M-Gram, or [X W] is not M-orthonormal after CholQR2");
        // redo the iteration without P (W was overwritten: the residual again)
        w->has_p = false;
        ++w->p_dropped;
        EIG_HIP(hipEventRecord(ev[0], s));
        residual(*w, w->X(w->KS), w->X(w->MSf()), res_buf(*w), sums, s);
        EIG_HIP(hipEventRecord(ev[1], s));
        EIG_CHECK(iterate(*w, false, ev.data()), EIG_ERR_BREAKDOWN,
                  "LOBPCG: W has no positive-definite M-Gram, or [X W] is not M-orthonormal after CholQR2 (without P too)");
      }
      w->has_p = true;
      ++w->iters;
      ++it;
      if (iters_done) *iters_done = it;
      if (timing)
      {
        EIG_HIP(hipEventSynchronize(ev[5]));
        float t[5];
        for (int q = 0; q < 5; ++q) EIG_HIP(hipEventElapsedTime(&t[q], ev[q], ev[q + 1]));
        timing->resid_ms += t[0];
        timing->precond_ms += t[1];
        timing->orth_ms += t[2];
        timing->spmm_ms += t[3];
        timing->rr_ms += t[4];
        timing->total_ms += t[0] + t[1] + t[2] + t[3] + t[4];
      }
    }
    EIG_HIP(hipStreamSynchronize(s));
    if (converged) *converged = conv ? 1 : 0;
    if (timing)
    {
      timing->iters = it;
      timing->cholqr_recomputed = w->cholqr_recomputed;
      timing->p_dropped = w->p_dropped;
      timing->orth_rejected = w->orth_rejected;
      timing->orth_dev = w->orth_dev;
    }
  });
}

extern "C" int eig_lobpcg_ritz(eig_lobpcg_t w, int nev, double *eval_host, double *evec_host, double *resid_host)
{
  return guard(w ? w->K->ctx : nullptr, [&] {
    EIG_CHECK(w && eval_host && nev >= 1 && nev <= w->m, EIG_ERR_ARG, "eig_lobpcg_ritz: 1 <= nev <= block required");
    eig_ctx_t ctx = w->K->ctx;
    EIG_HIP(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const int m = w->m;
    const i64 n = w->n;
    for (int j = 0; j < nev; ++j) eval_host[j] = w->theta[j];
    if (resid_host)
    {
      // fresh products (the W slices are scratch between iterations), not the carried KX, MX
      launch_spmm_mv8(*w->K, m, w->X(w->S), w->W(w->KS), s);
      if (w->M) launch_spmm_mv8(*w->M, m, w->X(w->S), w->W(w->MS), s);
      std::vector<double> sums;
      residual(*w, w->W(w->KS), w->M ? w->W(w->MS) : w->X(w->S), res_buf(*w), sums, s);
      for (int j = 0; j < nev; ++j) resid_host[j] = std::sqrt(sums[j]);
    }
    copy_evecs(ctx, w->S->d(), n, 0, n, nev, nullptr, nullptr, evec_host);
  });
}

extern "C" int eig_lobpcg_destroy(eig_lobpcg_t w)
{
  return w ? destroy_workspace(w, w->K->ctx) : EIG_OK;
}

extern "C" int eig_lobpcg_resid_mv8(eig_ctx_t ctx, int64_t n, int64_t m, const double *KX, const double *MX,
                                    const double *theta, double *R, double *sums)
{
  return guard(ctx, [&] {
    EIG_CHECK(ctx && KX && MX && theta && R && sums && n > 0 && m >= 8 && m <= 32 && m % 8 == 0, EIG_ERR_ARG,
              "eig_lobpcg_resid_mv8: n > 0, m in {8,16,24,32}");
    EIG_HIP(hipSetDevice(ctx->device));
    launch_lobpcg_resid(ctx, n, n, m, KX, MX, theta, R, sums, ctx->stream);
  });
}

extern "C" int eig_lobpcg_update_mv8(eig_ctx_t ctx, int64_t n, int64_t m, int kb, double *S, const double *C)
{
  return guard(ctx, [&] {
    EIG_CHECK(ctx && S && C && n > 0 && m >= 8 && m <= 32 && m % 8 == 0 && (kb == 2 || kb == 3), EIG_ERR_ARG,
              "eig_lobpcg_update_mv8: n > 0, m in {8,16,24,32}, kb in {2,3}");
    EIG_HIP(hipSetDevice(ctx->device));
    launch_lobpcg_update(ctx, n, n, m, kb, S, nullptr, nullptr, C, ctx->stream);
  });
}
