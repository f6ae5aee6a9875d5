// shift_invert.cpp -- the Krylov drivers on OP = (A - sigma B)^-1 B over exported LU factors: thick-restart
// Lanczos, one-vector and block (eig_shift_invert_solve[_ex] / _adaptive), and Arnoldi with Krylov-Schur restarts
// (eig_arnoldi_shift_invert).  The one-vector paths share KrylovWs; their host arithmetic is krylov_host.cpp.
#include "inverse_common.h"
#include "subspace_host.h"

using namespace eigmi;

// ============================================================================================
// computeGenSymShiftInvertMinMagnitude (arpack_geneo_wrapper.hh:581-658): thick-restart Lanczos
// in the B-inner product on OP = (A - sigma B)^-1 B, "LM" 
// ============================================================================================
namespace {

// Host copy of A - sigma B on A's pattern (pattern(B) within pattern(A); ashiftb.axpy(-sigma, b_),
// arpack_geneo_wrapper.hh:599-600).  B null: the identity.
HostCsr shifted_copy(eig_mat_s &A, eig_mat_s *B, double sigma)
{
  HostCsr a, b;
  mat_download_bcsr(A, a.rp, a.c, a.v);
  if (!B)
    pattern_shift_diag(0, A.nb_rows, A.br, a, -sigma, "shift-invert");
  else if (sigma != 0.0)
  {
    mat_download_bcsr(*B, b.rp, b.c, b.v);
    pattern_axpy(0, A.nb_rows, A.br, a, -sigma, b, "shift-invert");
  }
  return a;
}

// blocks: square blocks 1..4 (the symmetric driver, like the reference's, needs only mv and the
// factorisation); B then has A's block size
void shift_invert_check(eig_mat_t A, eig_mat_t B, bool blocks = false)
{
  check_inverse_matrix(A, "computeGenSymShiftInvertMinMagnitude", blocks);
  if (B)
  {
    check_inverse_matrix(B, "computeGenSymShiftInvertMinMagnitude", blocks);
    EIG_CHECK(B->br == A->br, EIG_ERR_BLOCKSIZE, "shift-invert: A and B block sizes differ");
    EIG_CHECK(B->ctx == A->ctx && B->nb_rows == A->nb_rows, EIG_ERR_SHAPE, "shift-invert: A and B sizes differ");
  }
}

// The factorisation of A - sigma B (arpack_geneo_wrapper.hh:597-601): the caller's, or a host one.
void shift_invert_factor(eig_mat_t A, eig_mat_t B, eig_lu_t lu, double sigma, LuRef &F)
{
  EIG_HIP(hipSetDevice(A->ctx->device));
  select_factors(*A, lu, A->nb_rows * A->br, "shift-invert: factorisation size differs from A", F, [&] {
    EIG_HIP(hipStreamSynchronize(A->ctx->stream));
    return shifted_copy(*A, B, sigma);
  });
}

// Device workspace of a one-vector Krylov driver on OP: the basis V (m + 1 columns of n scalar rows,
// column-major) and, in the B-inner product (bip), BV = B V -- else BV is V itself; the work vectors; the
// per-extension coefficient rows.  The members queue on the context's stream.
struct KrylovWs {
  eig_ctx_t ctx;
  hipStream_t s;
  eig_mat_t B;  // OP's B (null: the identity)
  eig_lu_t lu;  // factors of A - sigma B
  const i64 n;
  const int m;
  const bool bip;
  const i64 cstride;  // extension_stride(m)
  DevBuf Vb, BVb, Wb, BWb, X8b, Y8b, Tb, cb, coefb;
  double *V, *BV, *W, *BW, *cd, *sc;
  std::vector<double> coefh;

  KrylovWs(eig_ctx_t ctx_, eig_mat_t B_, eig_lu_t lu_, i64 n_, int m_, bool bip_)
      : ctx(ctx_), s(ctx_->stream), B(B_), lu(lu_), n(n_), m(m_), bip(bip_), cstride(extension_stride(m_)),
        Vb((size_t)(m + 1) * n * 8), BVb(bip ? (size_t)(m + 1) * n * 8 : 8), Wb(n * 8), BWb(n * 8), X8b(n * 64),
        Y8b(n * 64), Tb((size_t)2 * (m + 1) * n * 8), cb((size_t)(m + 8) * 8 * 2), coefb((size_t)m * cstride * 8),
        V(Vb.d()), BV(bip ? BVb.d() : Vb.d()), W(Wb.d()), BW(BWb.d()), cd(cb.d()), sc(cd + m + 8),
        coefh((size_t)m * cstride)
  {
    EIG_HIP(hipMemsetAsync(X8b.d(), 0, n * 64, s));
  }

  void bmul(const double *x, double *y)  // y = B x
  {
    if (B) launch_spmv(*B, x, y, nullptr, 0, B->nslices, s);
    else if (y != x) EIG_HIP(hipMemcpyAsync(y, x, n * 8, hipMemcpyDeviceToDevice, s));
  }
  double dot(const double *x, const double *y)
  {
    launch_dot(n, x, y, sc, 0, s, ctx->red);
    double h = 0.0;
    EIG_HIP(hipMemcpyAsync(&h, sc, 8, hipMemcpyDeviceToHost, s));
    EIG_HIP(hipStreamSynchronize(s));
    return h;
  }
  void solve(const double *bx, double *y)  // y = (A - sigma B)^-1 bx (column 0 of the 8-wide solve)
  {
    double *X8 = X8b.d(), *Y8 = Y8b.d();
    EIG_HIP(hipMemcpy2DAsync(X8, 64, bx, 8, 8, n, hipMemcpyDeviceToDevice, s));
    lu_inverse_device(lu, 8, X8, Y8, s);
    EIG_HIP(hipMemcpy2DAsync(y, 8, Y8, 64, 8, n, hipMemcpyDeviceToDevice, s));
  }
  void upload(const double *c, int count) { EIG_HIP(hipMemcpyAsync(cd, c, (size_t)count * 8, hipMemcpyHostToDevice, s)); }

  // Start vector: mt19937(seed) normal numbers, put into range(OP) when `into_range` (ARPACK's dgetv0 in the
  // generalised modes: a singular B leaves no null(B) components).  Returns (v, B v); start_scale normalises.
  double start(unsigned seed, bool into_range)
  {
    std::vector<double> h(n);
    host_random_normal(n, seed, h.data());
    EIG_HIP(hipMemcpyAsync(W, h.data(), n * 8, hipMemcpyHostToDevice, s));
    if (into_range)
    {
      bmul(W, BW);
      solve(BW, V);
    }
    else
      EIG_HIP(hipMemcpyAsync(V, W, n * 8, hipMemcpyDeviceToDevice, s));
    if (bip) bmul(V, BV);
    return dot(V, BV);
  }
  void start_scale(double norm)
  {
    launch_scal(n, 1.0 / norm, V, s);
    if (bip) launch_scal(n, 1.0 / norm, BV, s);
  }

  // Extend the factorisation from k to m vectors: for column j, W = OP applied to operand(j) (the device
  // vector B v_j, however the driver obtains it), CGS2 / DGKS against v_0 .. v_j in the inner product,
  // v_{j+1} = W / ||W||.  The coefficients and squared norms stay on the device and are read back once, at the
  // end: the steps queue without a host round trip, a breakdown is reported after them.  row(j) is column j's.
  template <class Operand>
  void extend(int k, Operand operand)
  {
    double *coef = coefb.d();
    for (int j = k; j < m; ++j)
    {
      double *cj = coef + (i64)j * cstride;
      solve(operand(j), W);  // the reverse-communication product
      for (int pass = 0; pass < 2; ++pass)
      {
        launch_gemv_t(n, j + 1, BV, n, W, cj + pass * (m + 1), 0, s, ctx->red);
        launch_gemv_n_sub(n, j + 1, V, n, cj + pass * (m + 1), nullptr, W, s);
      }
      if (bip) bmul(W, BW);
      launch_dot(n, W, bip ? BW : W, cj + 2 * (m + 1), 0, s, ctx->red);  // beta_j^2
      double *vn = V + (i64)(j + 1) * n;
      EIG_HIP(hipMemcpyAsync(vn, W, n * 8, hipMemcpyDeviceToDevice, s));
      launch_scal_dev(n, cj + 2 * (m + 1), true, vn, s);  // 1 / sqrt(beta_j^2)
      if (bip)
      {
        double *bvn = BV + (i64)(j + 1) * n;
        EIG_HIP(hipMemcpyAsync(bvn, BW, n * 8, hipMemcpyDeviceToDevice, s));
        launch_scal_dev(n, cj + 2 * (m + 1), true, bvn, s);
      }
    }
    EIG_HIP(hipMemcpyAsync(coefh.data() + (size_t)k * cstride, coef + (i64)k * cstride,
                           (size_t)(m - k) * cstride * 8, hipMemcpyDeviceToHost, s));
    EIG_HIP(hipStreamSynchronize(s));
  }
  const double *row(int j) const { return coefh.data() + (size_t)j * cstride; }

  // Restart: V <- V Z (Z m x kk row-major on the host), v_kk <- v_m; the same for BV (bip)
  void rotate(int kk, const std::vector<double> &Z)
  {
    double *Tmp = Tb.d();
    std::vector<double> col(m);
    for (int q = 0; q < kk; ++q)
    {
      for (int i = 0; i < m; ++i) col[i] = Z[(size_t)i * kk + q];
      upload(col.data(), m);
      launch_gemv_n_set(n, m, V, n, cd, nullptr, Tmp + (i64)q * n, s);
      if (bip) launch_gemv_n_set(n, m, BV, n, cd, nullptr, Tmp + (i64)(kk + q) * n, s);
      EIG_HIP(hipStreamSynchronize(s));
    }
    for (int t = 0; t < (bip ? 2 : 1); ++t)  // V, then BV from the second kk columns of Tmp
    {
      double *Q = t ? BV : V;
      EIG_HIP(hipMemcpyAsync(Q, Tmp + (i64)t * kk * n, (size_t)kk * n * 8, hipMemcpyDeviceToDevice, s));
      EIG_HIP(hipMemcpyAsync(Q + (i64)kk * n, Q + (i64)m * n, n * 8, hipMemcpyDeviceToDevice, s));
    }
  }
};

// One computeGenSymShiftInvertMinMagnitude solve (ARSymGenEig 'S' mode, "LM") with the factors F.
void shift_invert_core(eig_mat_t A, eig_mat_t B, const LuRef &F, double sigma, int nev, int ncv, double tol, int maxit,
                       unsigned seed, double *eval_host, double *evec_host, int *restarts)
{
  eig_ctx_t ctx = A->ctx;
  EIG_HIP(hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  const i64 n = A->nb_rows * A->br;  // scalar rows (square blocks 1..4: only mv and the factors are used)
  ncv = arpack_ncv(n, nev, ncv);
  EIG_CHECK(nev < ncv && ncv <= n && ncv <= 500, EIG_ERR_ARG, "shift-invert: need nev < ncv <= min(n, 500)");
  tol = arpack_tol(tol);
  maxit = arpack_maxit(nev, maxit);
  const int m = ncv;
  // basis V and BV (= B V; V itself when B is NULL)
  KrylovWs ws(ctx, B, F.lu, n, m, B != nullptr);
  ws.start_scale(std::sqrt(ws.start(seed, true)));  // B-normalised
  std::vector<double> T((size_t)m * m, 0.0), ctot(m + 1), th, Y, Z;
  int k = 0, nrestart = 0;
  double betam = 0.0;
  std::vector<int> ord;
  for (;;)
  {
    // extend the Lanczos factorisation from k to m vectors: w = (A - sigma B)^-1 (B v_j) from the stored B v_j
    ws.extend(k, [&](int j) { return ws.BV + (i64)j * n; });
    for (int j = k; j < m; ++j)
    {
      betam = extension_column(m, j, ws.row(j), ctot,
                               "shift-invert Lanczos: invariant subspace reached (choose ncv < n or another seed)");
      for (int i = 0; i <= j; ++i) T[(size_t)i * m + j] = T[(size_t)j * m + i] = ctot[i];
      if (j + 1 < m) T[(size_t)(j + 1) * m + j] = T[(size_t)j * m + (j + 1)] = betam;
    }
    sym_eig(m, T, th, Y);
    // "LM" on OP: the nev Ritz values of largest magnitude (eigenvalues of the pencil nearest sigma)
    order_largest_magnitude(th, ord);
    bool conv = true;
    for (int q = 0; q < nev; ++q)
      if (std::fabs(betam * Y[(size_t)(m - 1) * m + ord[q]]) > tol * std::fabs(th[ord[q]])) conv = false;
    if (conv || nrestart >= maxit) break;
    // thick restart: keep kk Ritz vectors of largest |theta|, then the residual vector
    const int kk = thick_restart_size(m, nev);
    Z.resize((size_t)m * kk);
    for (int i = 0; i < m; ++i)
      for (int q = 0; q < kk; ++q) Z[(size_t)i * kk + q] = Y[(size_t)i * m + ord[q]];
    ws.rotate(kk, Z);
    std::fill(T.begin(), T.end(), 0.0);
    for (int q = 0; q < kk; ++q) T[(size_t)q * m + q] = th[ord[q]];
    k = kk;
    ++nrestart;
  }
  // eigenpairs of the pencil: lambda = sigma + 1 / theta, sorted ascending (:636-648)
  std::vector<int> idx(nev);
  std::iota(idx.begin(), idx.end(), 0);
  std::vector<double> lam(nev);
  for (int i = 0; i < nev; ++i) lam[i] = sigma + 1.0 / th[ord[i]];
  std::stable_sort(idx.begin(), idx.end(), [&](int a, int b) { return lam[a] < lam[b]; });
  for (int i = 0; i < nev; ++i) eval_host[i] = lam[idx[i]];
  if (evec_host)
  {
    // purified Ritz vectors (ARPACK dseupd for the spectral-transformation modes): x = OP(V y) /
    // theta = V y + (beta_m y_m / theta) v_m.  B = I: that linear combination.  Generalised: the
    // operator applied explicitly to B V y = BV y, x = (A - sigma B)^-1 (BV y) / theta, then
    // B-normalised -- with a singular B (the harness's partition-of-unity B) the basis picks up
    // null(B) components through the projections that the B-inner products never see and that
    // grow over thick restarts; OP maps into range(OP), where they cannot live.
    std::vector<double> coef(m + 1);
    double *W = ws.W, *BW = ws.BW;
    for (int q = 0; q < nev; ++q)
    {
      const int col = ord[idx[q]];
      for (int i = 0; i < m; ++i) coef[i] = Y[(size_t)i * m + col];
      coef[m] = betam * Y[(size_t)(m - 1) * m + col] / th[col];
      ws.upload(coef.data(), m + 1);
      if (!B)
        launch_gemv_n_set(n, m + 1, ws.V, n, ws.cd, nullptr, W, s);
      else
      {
        launch_gemv_n_set(n, m, ws.BV, n, ws.cd, nullptr, BW, s);
        ws.solve(BW, W);
        ws.bmul(W, BW);
        const double xb = ws.dot(W, BW);
        EIG_CHECK(xb > 0.0, EIG_ERR_BREAKDOWN, "shift-invert: purified Ritz vector has no B-norm");
        launch_scal(n, 1.0 / std::sqrt(xb), W, s);
      }
      EIG_HIP(hipMemcpyAsync(evec_host + (i64)q * n, W, n * 8, hipMemcpyDeviceToHost, s));
      EIG_HIP(hipStreamSynchronize(s));
    }
  }
  if (restarts) *restarts = nrestart;
}

// Block variant (EIG_SI_BLOCK, the default where the basis fits): the same OP, the same wanted
// pairs and the same B-inner product, by block Lanczos with Krylov-Schur (thick) restarts on p
// columns at once.  Why: one application of OP is the block-inverse triangular solve, a chain over
// the factor's 64-row blocks that one workgroup walks per 8 columns -- latency-bound, so p = 16
// columns cost what one column costs (two chains side by side), and a block Krylov space reaches
// the wanted pairs in a fraction of the applications the one-vector recurrence needs (nev = 8 on
// the 200^2 GenEO pencil: 44 applications -> 8).  Basis V (c columns, MultiVector<double,8>
// blocks) and BV = B V; per block step, with V_a the last p columns:
//     W = OP(B V_a);  H = (B V)^T W, W -= V H  (twice: CGS2 in the B-inner product);
//     W = F R (CholQR2 in the B-inner product);  T(:, a) = H, T(next, a) = R.
// Rayleigh-Ritz on T; the residual of Ritz pair i is ||R y_i(a)|| (V_next is B-orthonormal), so the
// convergence test is ||R y_i(a)|| <= tol |theta_i|.  Restart: U = V Y(:, kept) (kk Ritz vectors of
// largest |theta|), T = diag(theta_kept) coupled to F by C = R Y(a, kept) -- again a block Krylov
// decomposition OP [U F] = [U F] T + ..., extended from F.  Eigenvectors purified like the one-vector
// path: x = OP(B V y) / theta, B-normalised (one block solve for all of them).
struct SiBlockShape {
  int nw, p, kk, cmax;
};

SiBlockShape si_block_shape(int nev, int ncv)
{
  SiBlockShape g;
  g.nw = (nev + 7) / 8 * 8;
  g.p = std::max(16, g.nw);
  g.kk = std::max((nev + (nev + 1) / 2 + 7) / 8 * 8, 3 * g.p);
  g.cmax = std::max(g.kk + 3 * g.p, (ncv + 7) / 8 * 8);
  return g;
}

// the block method's reductions within the context's tickets: the projection Gram (cmax x p, partials
// in a buffer sized for the launch), the CholQR Gram (p x p) and the purified vectors' B-norms
// (the projection Gram goes in row slices of 64 when it is larger: see gram_rows)
bool si_block_fits(const SiBlockShape &g)
{
  return gram_mv8_chunks(64, g.p) <= kNumTickets && gram_mv8_chunks(g.p, g.p) <= kNumTickets &&
         g.nw / 8 <= kNumTickets;
}

// H (c x p, row i at H + i p) = Q1(:, 0 .. c)^T Q2: one launch where its output chunks fit the
// tickets, else row slices (each a multiple of 64 rows) in stream order
void gram_rows(eig_ctx_t ctx, i64 n, int c, int p, const double *Q1, const double *Q2, double *H, hipStream_t s)
{
  int rc = c;
  while (gram_mv8_chunks(rc, p) > kNumTickets) rc = std::max(64, (rc / 2 + 63) / 64 * 64);
  for (int r0 = 0; r0 < c; r0 += rc)
    launch_gram_panel(ctx, n, n, std::min(rc, c - r0), p, Q1 + (i64)r0 * n, Q2, H + (size_t)r0 * p, s);
}

void shift_invert_block_core(eig_mat_t A, eig_mat_t B, const LuRef &F, double sigma, int nev, int ncv, double tol,
                             int maxit, unsigned seed, double *eval_host, double *evec_host, int *restarts)
{
  eig_ctx_t ctx = A->ctx;
  EIG_HIP(hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  const i64 n = A->nb_rows;
  const SiBlockShape g = si_block_shape(nev, ncv);
  const int p = g.p, kk = g.kk, cmax = g.cmax, cap = cmax + p;
  EIG_CHECK(nev < n && cap <= n, EIG_ERR_ARG, "shift-invert (block): the block basis does not fit n");
  EIG_CHECK(si_block_fits(g), EIG_ERR_ARG, "shift-invert (block): nev too large for the block method (use EIG_SI_SINGLE)");
  tol = arpack_tol(tol);
  maxit = arpack_maxit(nev, maxit);
  const int wk = std::max(kk, g.nw);
  DevBuf Vb((size_t)cap * n * 8), BVb(B ? (size_t)cap * n * 8 : 8), W1b((size_t)p * n * 8), W2b((size_t)p * n * 8),
      BWb((size_t)p * n * 8), Ub((size_t)wk * n * 8), Hb((size_t)cap * std::max(p, wk) * 8);
  double *V = Vb.d(), *BV = B ? BVb.d() : V, *W = W1b.d(), *Wt = W2b.d(), *BW = BWb.d(), *U = Ub.d(), *dH = Hb.d();
  auto bmul = [&](const double *x, double *y, int cols) {  // y = B x (cols columns)
    if (B) launch_spmm_mv8(*B, cols, x, y, s);
    else if (y != x) EIG_HIP(hipMemcpyAsync(y, x, (size_t)cols * n * 8, hipMemcpyDeviceToDevice, s));
  };
  // y (q columns) = x (px columns) M, M px x q row-major on the host
  std::vector<double> mneg;
  auto mul_small = [&](const double *x, int px, const std::vector<double> &M, int q, double *y) {
    mneg.resize((size_t)px * q);
    for (size_t k = 0; k < mneg.size(); ++k) mneg[k] = -M[k];
    EIG_HIP(hipMemcpyAsync(dH, mneg.data(), mneg.size() * 8, hipMemcpyHostToDevice, s));
    EIG_HIP(hipMemsetAsync(y, 0, (size_t)q * n * 8, s));
    for (int i = 0; i < px / 8; ++i) launch_project(n, q, x + (i64)i * 8 * n, y, dH + (size_t)i * 8 * q, s);
    EIG_HIP(hipStreamSynchronize(s));  // (mneg is reused by the next call)
  };
  // OP on p columns: y = (A - sigma B)^-1 bx (bx is consumed as the solve's scratch)
  auto op = [&](double *bx, double *y, int cols) { lu_inverse_device(F.lu, cols, bx, y, s); };
  // W (p columns, scratch Wt) -> B-orthonormal F at dst / bdst with W = F R; false on a rank loss
  std::vector<double> G((size_t)p * p), R((size_t)p * p), Ri((size_t)p * p), Rtot((size_t)p * p);
  auto bortho = [&](double *dst, double *bdst) -> bool {
    std::fill(Rtot.begin(), Rtot.end(), 0.0);
    for (int i = 0; i < p; ++i) Rtot[(size_t)i * p + i] = 1.0;
    for (int pass = 0; pass < 2; ++pass)
    {
      double *bw = B ? BW : W;
      bmul(W, bw, p);
      launch_gram_panel(ctx, n, n, p, p, W, bw, dH, s);
      EIG_HIP(hipMemcpyAsync(G.data(), dH, G.size() * 8, hipMemcpyDeviceToHost, s));
      EIG_HIP(hipStreamSynchronize(s));
      for (int i = 0; i < p; ++i)
        for (int j = i + 1; j < p; ++j) G[(size_t)j * p + i] = G[(size_t)i * p + j];
      if (!chol_upper(p, G.data(), R.data())) return false;
      tri_upper_inv(p, R.data(), Ri.data());
      mul_small(W, p, Ri, p, Wt);
      std::swap(W, Wt);
      std::vector<double> Rn((size_t)p * p, 0.0);  // Rtot = R Rtot
      for (int i = 0; i < p; ++i)
        for (int k = i; k < p; ++k)
          for (int j = k; j < p; ++j) Rn[(size_t)i * p + j] += R[(size_t)i * p + k] * Rtot[(size_t)k * p + j];
      Rtot.swap(Rn);
    }
    EIG_HIP(hipMemcpyAsync(dst, W, (size_t)p * n * 8, hipMemcpyDeviceToDevice, s));
    bmul(dst, bdst, p);
    return true;
  };
  // start block: normal numbers put into the range of OP (dgetv0 for the generalised modes), then
  // B-orthonormalised
  {
    launch_fill_normal((i64)p * n, seed, Wt, s);
    bmul(Wt, BW, p);
    op(BW, W, p);
    EIG_CHECK(bortho(V, BV), EIG_ERR_BREAKDOWN, "shift-invert (block): start block is rank deficient");
  }
  std::vector<double> T((size_t)cap * cap, 0.0), th, Y, Hh, Ht, Tc;
  int c = p, nrestart = 0;
  std::vector<int> ord;
  for (;;)
  {
    // apply OP to the active block V(:, a .. c), project, B-orthonormalise: F = V(:, c .. c + p)
    const int a = c - p;
    EIG_HIP(hipMemcpyAsync(BW, BV + (i64)a * n, (size_t)p * n * 8, hipMemcpyDeviceToDevice, s));
    op(BW, W, p);
    Ht.assign((size_t)c * p, 0.0);
    for (int pass = 0; pass < 2; ++pass)  // CGS2 against V(:, 0 .. c) in the B-inner product
    {
      gram_rows(ctx, n, c, p, BV, W, dH, s);
      for (int i = 0; i < c / 8; ++i) launch_project(n, p, V + (i64)i * 8 * n, W, dH + (size_t)i * 8 * p, s);
      Hh.resize((size_t)c * p);
      EIG_HIP(hipMemcpyAsync(Hh.data(), dH, Hh.size() * 8, hipMemcpyDeviceToHost, s));
      EIG_HIP(hipStreamSynchronize(s));
      for (size_t k = 0; k < Hh.size(); ++k) Ht[k] += Hh[k];
    }
    for (int i = 0; i < c; ++i)
      for (int j = 0; j < p; ++j) T[(size_t)i * cap + a + j] = T[(size_t)(a + j) * cap + i] = Ht[(size_t)i * p + j];
    EIG_CHECK(bortho(V + (i64)c * n, BV + (i64)c * n), EIG_ERR_BREAKDOWN,
              "shift-invert (block): invariant subspace reached (choose another seed or the one-vector solver)");
    // Rayleigh-Ritz on the c columns: at the end of the first cycle, then after every application
    // (stop as soon as the wanted pairs converged).  Inside the first cycle the wanted pairs have not
    // converged in any run seen, and the host eigen-solve of T costs O(c^3) (~1-2 ms at c = 64-96).
    auto join = [&] {  // F joins the basis: T(c .. c + p, a .. c) = R
      for (int i = 0; i < p; ++i)
        for (int j = 0; j < p; ++j)
          T[(size_t)(c + i) * cap + a + j] = T[(size_t)(a + j) * cap + c + i] = Rtot[(size_t)i * p + j];
      c += p;
    };
    if (nrestart == 0 && c + p <= cmax)
    {
      join();
      continue;
    }
    Tc.resize((size_t)c * c);
    for (int i = 0; i < c; ++i)
      for (int j = 0; j < c; ++j) Tc[(size_t)i * c + j] = T[(size_t)i * cap + j];
    sym_eig(c, Tc, th, Y);  // Y[i * c + j]: component i of Ritz vector j
    // "LM" on OP: the Ritz values of largest magnitude (eigenvalues of the pencil nearest sigma)
    order_largest_magnitude(th, ord);
    // coupling of the Ritz vectors to F: C(:, j) = R y_j(a .. a + p)
    auto coupling = [&](int j, int i) {
      double v = 0.0;
      for (int k = i; k < p; ++k) v += Rtot[(size_t)i * p + k] * Y[(size_t)(a + k) * c + j];
      return v;
    };
    bool conv = c >= std::min(nev + 1, cmax);
    for (int q = 0; q < nev && conv; ++q)
    {
      double r2 = 0.0;
      for (int i = 0; i < p; ++i)
      {
        const double v = coupling(ord[q], i);
        r2 += v * v;
      }
      if (std::sqrt(r2) > tol * std::fabs(th[ord[q]])) conv = false;
    }
    if (conv) break;
    if (c + p <= cmax)
    {
      join();
      continue;
    }
    if (nrestart >= maxit) break;
    // thick restart: U = V Y(:, kept), F moves behind it, T = diag(theta_kept) + the coupling C
    {
      std::vector<double> Ysel((size_t)c * kk);
      for (int r = 0; r < c; ++r)
        for (int q = 0; q < kk; ++q) Ysel[(size_t)r * kk + q] = Y[(size_t)r * c + ord[q]];
      mul_small(V, c, Ysel, kk, U);
      EIG_HIP(hipMemcpyAsync(V, U, (size_t)kk * n * 8, hipMemcpyDeviceToDevice, s));
      EIG_HIP(hipMemcpyAsync(V + (i64)kk * n, V + (i64)c * n, (size_t)p * n * 8, hipMemcpyDeviceToDevice, s));
      if (B)
      {
        EIG_HIP(hipMemcpyAsync(BV + (i64)kk * n, BV + (i64)c * n, (size_t)p * n * 8, hipMemcpyDeviceToDevice, s));
        bmul(V, BV, kk);
      }
      std::fill(T.begin(), T.end(), 0.0);
      for (int q = 0; q < kk; ++q)
      {
        T[(size_t)q * cap + q] = th[ord[q]];
        for (int i = 0; i < p; ++i) T[(size_t)(kk + i) * cap + q] = T[(size_t)q * cap + kk + i] = coupling(ord[q], i);
      }
      c = kk + p;
      ++nrestart;
    }
  }
  // eigenpairs of the pencil: lambda = sigma + 1 / theta, ascending (:636-648)
  std::vector<int> idx(nev);
  std::iota(idx.begin(), idx.end(), 0);
  std::vector<double> lam(nev);
  for (int q = 0; q < nev; ++q) lam[q] = sigma + 1.0 / th[ord[q]];
  std::stable_sort(idx.begin(), idx.end(), [&](int x, int y) { return lam[x] < lam[y]; });
  for (int q = 0; q < nev; ++q) eval_host[q] = lam[idx[q]];
  if (evec_host)
  {
    const int nw = g.nw;
    std::vector<double> Ysel((size_t)c * nw, 0.0);
    for (int q = 0; q < nev; ++q)
    {
      const int j = ord[idx[q]];
      for (int r = 0; r < c; ++r) Ysel[(size_t)r * nw + q] = Y[(size_t)r * c + j] / th[j];
    }
    mul_small(BV, c, Ysel, nw, U);  // B V y / theta
    op(U, W, nw);                   // x = OP(B V y) / theta
    double *bw = B ? BW : W;
    bmul(W, bw, nw);
    launch_dot_diag_mv8(n, nw, W, bw, dH, 0, s, ctx->red);
    std::vector<double> xb(nw), h((size_t)nw * n);
    EIG_HIP(hipMemcpyAsync(xb.data(), dH, nw * 8, hipMemcpyDeviceToHost, s));
    EIG_HIP(hipMemcpyAsync(h.data(), W, h.size() * 8, hipMemcpyDeviceToHost, s));
    EIG_HIP(hipStreamSynchronize(s));
    for (int q = 0; q < nev; ++q)
    {
      EIG_CHECK(xb[q] > 0.0, EIG_ERR_BREAKDOWN, "shift-invert: purified Ritz vector has no B-norm");
      mv8_column(h.data(), n, 0, n, q, 1.0 / std::sqrt(xb[q]), evec_host + (i64)q * n);
    }
  }
  if (restarts) *restarts = nrestart;
}

// EIG_SI_AUTO: the block solver where its basis (cmax + p columns) is at most a quarter of n
bool si_use_block(i64 n, int nev, int ncv, int flags)
{
  if (flags & EIG_SI_SINGLE) return false;
  if (flags & EIG_SI_BLOCK) return true;
  const SiBlockShape g = si_block_shape(nev, ncv);
  // the basis within n / 4, and the reductions within the tickets
  return (i64)(g.cmax + g.p) * 4 <= n && si_block_fits(g);
}

void shift_invert_run(eig_mat_t A, eig_mat_t B, const LuRef &F, double sigma, int nev, int ncv, double tol, int maxit,
                      unsigned seed, double *eval_host, double *evec_host, int *restarts, int flags)
{
  // blocked matrices: the one-vector method (mv and the factors only); the block method's panel kernels are
  // FieldMatrix<..,1,1> code (eig_shift_invert_solve_ex has refused EIG_SI_BLOCK on them)
  const bool block = A->br == 1 && si_use_block(A->nb_rows, nev, ncv, flags);
  (block ? shift_invert_block_core : shift_invert_core)(A, B, F, sigma, nev, ncv, tol, maxit, seed, eval_host,
                                                        evec_host, restarts);
}

}  // namespace

extern "C" int eig_shift_invert_solve_ex(eig_mat_t A, eig_mat_t B, eig_lu_t lu, double sigma, int nev, int ncv,
                                         double tol, int maxit, unsigned seed, double *eval_host, double *evec_host,
                                         int *restarts, int flags)
{
  return guard(A ? A->ctx : nullptr, [&] {
    EIG_CHECK(A && eval_host && nev > 0, EIG_ERR_ARG, "eig_shift_invert_solve: bad argument");
    EIG_CHECK((flags & ~(EIG_SI_SINGLE | EIG_SI_BLOCK)) == 0 && flags != (EIG_SI_SINGLE | EIG_SI_BLOCK), EIG_ERR_ARG,
              "eig_shift_invert_solve_ex: unknown flags");
    shift_invert_check(A, B, true);
    EIG_CHECK(A->br == 1 || !(flags & EIG_SI_BLOCK), EIG_ERR_BLOCKSIZE,
              "shift-invert (block): only implemented for FieldMatrix<..,1,1> (use EIG_SI_AUTO / EIG_SI_SINGLE)");
    LuRef F;
    shift_invert_factor(A, B, lu, sigma, F);
    shift_invert_run(A, B, F, sigma, nev, ncv, tol, maxit, seed, eval_host, evec_host, restarts, flags);
  });
}

extern "C" int eig_shift_invert_solve(eig_mat_t A, eig_mat_t B, eig_lu_t lu, double sigma, int nev, int ncv,
                                      double tol, int maxit, unsigned seed, double *eval_host, double *evec_host,
                                      int *restarts)
{
  return eig_shift_invert_solve_ex(A, B, lu, sigma, nev, ncv, tol, maxit, seed, eval_host, evec_host, restarts,
                                   EIG_SI_AUTO);
}

// computeGenSymShiftInvertMinMagnitudeAdaptive (arpack_geneo_wrapper.hh:661-774): solve with nev =
// initial_nev; while the largest returned eigenvalue is below `threshold` and nev < max_nev, grow
// nev to min(max_nev, int(nev * 1.3)) (:770; the comment at :665 says 50 %, the code 1.3) and solve
// again from the same start (ARPACK++'s default initial guess each pass).  One factorisation of
// A - sigma B serves every pass.  ncv = 0 (auto) and maxit = nIterationsMax_ * nev as the reference.
extern "C" int eig_shift_invert_adaptive(eig_mat_t A, eig_mat_t B, eig_lu_t lu, double sigma, double threshold,
                                         int initial_nev, int max_nev, double tol, int maxit_per_nev, unsigned seed,
                                         double *eval_host, double *evec_host, int *nev_out, int *passes)
{
  return guard(A ? A->ctx : nullptr, [&] {
    EIG_CHECK(A && eval_host && nev_out && initial_nev > 0 && max_nev > 0, EIG_ERR_ARG,
              "eig_shift_invert_adaptive: bad argument");
    // (arpack_geneo_wrapper.hh:693-694: "initial_nev too large")
    EIG_CHECK(initial_nev <= max_nev, EIG_ERR_ARG, "eig_shift_invert_adaptive: initial_nev too large");
    shift_invert_check(A, B, true);
    LuRef F;
    shift_invert_factor(A, B, lu, sigma, F);
    int nev = initial_nev, pass = 0;
    for (;;)
    {
      const int maxit = maxit_per_nev > 0 ? maxit_per_nev * nev : 0;
      shift_invert_run(A, B, F, sigma, nev, 0, tol, maxit, seed, eval_host, evec_host, nullptr, EIG_SI_AUTO);
      ++pass;
      if (eval_host[nev - 1] >= threshold || nev >= max_nev) break;
      // (:770; for nev <= 3, int(nev * 1.3) == nev and the reference would solve the same problem
      // forever -- there nev grows by one instead; from nev = 4 on the sequences are identical)
      nev = std::min(max_nev, std::max(nev + 1, (int)(nev * 1.3)));
    }
    *nev_out = nev;
    if (passes) *passes = pass;
  });
}

// ============================================================================================
// Non-symmetric modes (arpack_geneo_wrapper.hh:428-578): computeStdNonSymMinMagnitude
// (ARNonSymStdEig on OP = (A - sigma B)^-1 B, "LM", lambda = sigma + 1 / Re(nu)) and
// computeGenNonSymShiftInvertMinMagnitude (ARNonSymGenEig, real shift-invert mode: the same OP in
// the B-inner product, lambda = sigma + 1 / nu).  ARPACK's dnaupd restarts implicitly with exact
// shifts; here the restart is Stewart's Krylov-Schur in its eigenvector-basis form: the projected
// matrix G of the Krylov decomposition  OP V = V G + f c^T  has its wanted eigenvectors (real and
// imaginary parts of complex pairs) orthonormalised into Z (m x kk); span(Z) is G-invariant, so
// OP (V Z) = (V Z)(Z^T G Z) + f (Z^T c)^T is again a Krylov decomposition, extended by Arnoldi
// steps (CGS2 in the chosen inner product) back to m vectors.  The same wanted Ritz values as
// ARPACK's restart filter (the polynomial with the unwanted Ritz values as roots annihilates the
// complement of span(Z)); convergence: ||f|| |c^T y| <= tol |nu| (dnaupd's Ritz estimate).
// ============================================================================================
namespace {

void arnoldi_core(eig_mat_t A, eig_mat_t B, const LuRef &F, double sigma, int nev, int ncv, double tol, int maxit,
                  unsigned seed, bool gen, double *eval_re, double *eval_im, double *evec_host, int *restarts)
{
  typedef std::complex<double> C;
  eig_ctx_t ctx = A->ctx;
  EIG_HIP(hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  const i64 n = A->nb_rows;
  ncv = arpack_ncv(n, nev, ncv);
  EIG_CHECK(nev + 2 <= ncv && ncv <= n && ncv <= 500, EIG_ERR_ARG, "Arnoldi: need nev + 2 <= ncv <= min(n, 500)");
  tol = arpack_tol(tol);
  maxit = arpack_maxit(nev, maxit);
  const int m = ncv;
  KrylovWs ws(ctx, B, F.lu, n, m, gen && B);  // the generalised mode: the B-inner product
  // the generalised mode puts the start vector into range(OP) first (dgetv0 for mode 3)
  const double nb = std::sqrt(std::max(0.0, ws.start(seed, gen)));
  EIG_CHECK(nb > 0.0, EIG_ERR_BREAKDOWN, "Arnoldi: zero start vector");
  ws.start_scale(nb);
  std::vector<double> G((size_t)m * m, 0.0), cvec, ctot(m + 1), Z;
  std::vector<C> w, Y;
  std::vector<int> ord;
  std::vector<std::pair<int, bool>> units;
  double beta = 0.0;
  int k = 0, nrestart = 0;
  for (;;)
  {
    // extend the Krylov decomposition from k to m vectors (Arnoldi steps): W = OP v_j, B v_j formed in BW
    ws.extend(k, [&](int j) {
      ws.bmul(ws.V + (i64)j * n, ws.BW);
      return ws.BW;
    });
    for (int j = k; j < m; ++j)
    {
      if (j > 0)
        for (int i = 0; i < j; ++i) G[(size_t)j * m + i] = beta * cvec[i];
      beta = extension_column(m, j, ws.row(j), ctot, "Arnoldi: invariant subspace reached (choose ncv < n or another seed)");
      for (int i = 0; i <= j; ++i) G[(size_t)i * m + j] = ctot[i];
      cvec.assign(j + 1, 0.0);
      cvec[j] = 1.0;
    }
    EIG_CHECK(gen_eig(m, G, w, Y), EIG_ERR_BREAKDOWN, "Arnoldi: QR iteration of the projected matrix failed");
    // "LM": largest |nu| first (conjugate partners keep their relative order)
    order_largest_magnitude(w, ord);
    auto resid = [&](int q) {
      C r = 0.0;
      for (int i = 0; i < m; ++i) r += cvec[i] * Y[(size_t)i * m + q];
      return beta * std::abs(r);
    };
    bool conv = true;
    for (int i = 0; i < nev; ++i)
      if (resid(ord[i]) > tol * std::abs(w[ord[i]])) conv = false;
    if (conv || nrestart >= maxit) break;
    // Krylov-Schur restart: G <- Z^T G Z, c <- Z^T c; V <- V Z, v_kk <- v_m
    int kk = 0;
    krylov_schur_restart(m, nev, G, cvec, w, Y, ord, kk, Z, units);
    ws.rotate(kk, Z);
    k = kk;
    ++nrestart;
  }
  // eigenvalues of the original problem, ascending by real part (:484-498, :556-571)
  std::vector<C> lam(nev);
  for (int i = 0; i < nev; ++i)
  {
    const C nu = w[ord[i]];
    lam[i] = gen ? C(sigma) + 1.0 / nu : C(sigma + 1.0 / nu.real(), (C(sigma) + 1.0 / nu).imag());
  }
  std::vector<int> idx(nev);
  std::iota(idx.begin(), idx.end(), 0);
  std::stable_sort(idx.begin(), idx.end(), [&](int a, int b) { return lam[a].real() < lam[b].real(); });
  for (int i = 0; i < nev; ++i)
  {
    eval_re[i] = lam[idx[i]].real();
    if (eval_im) eval_im[i] = lam[idx[i]].imag();
  }
  if (evec_host)
  {
    // x = V y, unit 2-norm as a complex vector; ARPACK's raw storage of a conjugate pair: the real
    // part for the member with Im(nu) > 0, the imaginary part for its partner
    std::vector<double> coef(m);
    double *W = ws.W, *BW = ws.BW;
    for (int q = 0; q < nev; ++q)
    {
      const int e = ord[idx[q]];
      const bool cplx = w[e].imag() != 0.0;
      int ey = e;
      if (cplx && w[e].imag() < 0.0)
        for (int i = 0; i < m; ++i)
          if (w[i] == std::conj(w[e])) ey = i;
      double nr2 = 0.0;
      for (int part = 0; part < (cplx ? 2 : 1); ++part)
      {
        for (int i = 0; i < m; ++i)
          coef[i] = part == 0 ? Y[(size_t)i * m + ey].real() : Y[(size_t)i * m + ey].imag();
        ws.upload(coef.data(), m);
        launch_gemv_n_set(n, m, ws.V, n, ws.cd, nullptr, part == 0 ? W : BW, s);
        nr2 += ws.dot(part == 0 ? W : BW, part == 0 ? W : BW);
      }
      double *x = (cplx && w[e].imag() < 0.0) ? BW : W;
      launch_scal(n, 1.0 / std::sqrt(nr2), x, s);
      EIG_HIP(hipMemcpyAsync(evec_host + (i64)q * n, x, n * 8, hipMemcpyDeviceToHost, s));
      EIG_HIP(hipStreamSynchronize(s));
    }
  }
  if (restarts) *restarts = nrestart;
}

}  // namespace

extern "C" int eig_arnoldi_shift_invert(eig_mat_t A, eig_mat_t B, eig_lu_t lu, double sigma, int nev, int ncv,
                                        double tol, int maxit, unsigned seed, int mode, double *eval_re,
                                        double *eval_im, double *evec_host, int *restarts)
{
  return guard(A ? A->ctx : nullptr, [&] {
    EIG_CHECK(A && eval_re && nev > 0, EIG_ERR_ARG, "eig_arnoldi_shift_invert: bad argument");
    EIG_CHECK(mode == EIG_ARNOLDI_STD || mode == EIG_ARNOLDI_GEN, EIG_ERR_ARG, "eig_arnoldi_shift_invert: bad mode");
    shift_invert_check(A, B);
    LuRef F;
    shift_invert_factor(A, B, lu, sigma, F);
    arnoldi_core(A, B, F, sigma, nev, ncv, tol, maxit, seed, mode == EIG_ARNOLDI_GEN, eval_re, eval_im, evec_host,
                 restarts);
  });
}
