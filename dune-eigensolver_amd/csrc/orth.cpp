// orth.cpp -- orthonormalisation of MultiVector<double,8> blocks, host side: which of the kernels of
// k_orth.hip a call takes (column MGS in five forms, CholQR, B-Gram-Schmidt), the tall-skinny Gram with
// its allreduce, the look-ahead MGS's state on a context, and the C entry points for all of it.  No
// kernel is launched from here directly: every launch goes through a launch_* of k_orth.hip / k_mv8.hip /
// k_blas.hip.
#include <algorithm>
#include <cstdlib>

#include "internal.h"

using namespace eigmi;

namespace eigmi {

// ============================================================================================
// the look-ahead MGS on a context
// ============================================================================================
int mgs_lookahead_default()
{
  static const int L = [] {
    const char *e = std::getenv("EIGMI_MGS_LOOKAHEAD");
    const int v = e ? std::atoi(e) : kMgsLookaheadDefault;
    return std::min(8, std::max(1, v));
  }();
  return L;
}

namespace {
struct MgsLaBuffer {  // the device layout behind MgsLaState
  double Sfin[64];
  unsigned st[64];
};
}  // namespace

MgsLaState mgs_lookahead_state(eig_ctx_t ctx, hipStream_t s)
{
  const bool fresh = (int)ctx->pool.size() <= kSlotMgsLa || ctx->pool[kSlotMgsLa].second < sizeof(MgsLaBuffer);
  MgsLaBuffer *buf = (MgsLaBuffer *)ctx_buffer(ctx, kSlotMgsLa, sizeof(MgsLaBuffer));
  if (fresh) EIG_HIP(hipMemsetAsync(buf, 0, sizeof(MgsLaBuffer), s));  // (the state words start clear)
  return MgsLaState{buf->Sfin, buf->st};
}

int *mgs_err_word(eig_ctx_t ctx)
{
  MgsCtx &g = ctx->mgs;
  if (!g.err_host)
  {
    EIG_HIP(hipHostMalloc(reinterpret_cast<void **>(&g.err_host), sizeof(int), hipHostMallocMapped));
    *g.err_host = 0;
    EIG_HIP(hipHostGetDevicePointer(reinterpret_cast<void **>(&g.err_dev), g.err_host, 0));
  }
  return g.err_dev;
}

void mgs_release(eig_ctx_t ctx)
{
  if (ctx->mgs.err_host) (void)hipHostFree(ctx->mgs.err_host);
}

// read passes of the last look-ahead call on this context (diagnostics; synchronises the stream):
// -1 none finished, -2 the last launch's grid barrier timed out
int mgs_lookahead_passes(eig_ctx_t ctx)
{
  const MgsLaState state = mgs_lookahead_state(ctx, ctx->stream);
  unsigned w[64] = {};
  EIG_HIP(hipMemcpyAsync(w, state.st, sizeof(w), hipMemcpyDeviceToHost, ctx->stream));
  EIG_HIP(hipStreamSynchronize(ctx->stream));
  if (ctx->mgs.err_host && *reinterpret_cast<volatile int *>(ctx->mgs.err_host)) return -2;
  return (w[kMgsLaLast] & kMgsLaWritten) ? (int)((w[kMgsLaLast] >> 8) & 255u) : -1;
}

void mgs_lookahead_check(eig_ctx_t ctx)
{
  // (called after a synchronisation of the stream: the word is host memory, no copy, no launch)
  if (!ctx->mgs.la_armed) return;
  ctx->mgs.la_armed = false;
  volatile int *e = ctx->mgs.err_host;
  if (!e || !*e) return;
  *e = 0;
  EIG_CHECK(false, EIG_ERR_HIP,
            "orthonormalize_blocked: a look-ahead MGS grid barrier timed out (workgroups not co-resident); "
            "the block was poisoned with NaN");
}

// ============================================================================================
// device-pointer helpers shared with the drivers
// ============================================================================================
// G (m1 x m2 row-major) = Q1^T Q2, tiled so that one launch stays within the ticket pool.
void gram_device(eig_ctx_t ctx, i64 n, i64 m1, i64 m2, const double *Q1, const double *Q2, double *G)
{
  if (gram_mv8_chunks(m1, m2) <= 48)
  {
    launch_gram_mv8(n, m1, m2, Q1, Q2, G, 0, ctx->stream, ctx->red);
  }
  else
  {
    // row panels of Q1 (32 columns each) against all of Q2; write into a temp then scatter
    EIG_CHECK(gram_mv8_chunks(32, m2) <= 48, EIG_ERR_ARG, "gram: Q2 too wide (> 1536 columns)");
    double *tmp = (double *)ctx_buffer(ctx, kSlotGramRows, (size_t)32 * m2 * sizeof(double));
    for (i64 r = 0; r < m1; r += 32)
    {
      const i64 mr = std::min<i64>(32, m1 - r);
      launch_gram_mv8(n, mr, m2, Q1 + r * n, Q2, tmp, 0, ctx->stream, ctx->red);
      EIG_HIP(hipMemcpyAsync(G + r * m2, tmp, mr * m2 * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
    }
  }
  allreduce_sum(ctx, G, m1 * m2, ctx->stream);
}

void spmm_dot_gram_device(const eig_mat_s &A, const double *X, double *Y, double *dp, double *gram)
{
  eig_ctx_t ctx = A.ctx;
  if (launch_spmm_dot_gram_mv8(A, 8, X, Y, dp, gram, ctx->stream, ctx->red)) return;
  // no fused kernel on this image: the product with its dots, then the panel Gram of the block
  launch_spmm_dot_mv8(A, 8, X, Y, dp, ctx->stream, ctx->red);
  gram_device(ctx, A.nb_rows * A.br, 8, 8, Y, Y, gram);  // scalar rows
}

void orthonormalize_device(eig_ctx_t ctx, i64 n, i64 m, double *Q, int variant, const double *gram0)
{
  const int flags = variant & (EIG_ORTHO_GRID | EIG_ORTHO_NO_COOP | EIG_ORTHO_ONE_WG);
  const int la = (variant >> EIG_ORTHO_LOOKAHEAD_SHIFT) & 15;  // EIG_ORTHO_LOOKAHEAD(L); 0: the default
  const int L = la ? std::min(la, 8) : mgs_lookahead_default();
  variant &= 0xff;
  hipStream_t s = ctx->stream;
  double *S = (double *)ctx_buffer(ctx, kSlotOrthS, 64 * sizeof(double));
  double *U = S + 0;  // reused: Ssum for MGS, Gram for CholQR
  double *U2 = (double *)ctx_buffer(ctx, kSlotOrthU, 64 * sizeof(double));
  double *Sg = nullptr;
  if (m > 8) Sg = (double *)ctx_buffer(ctx, kSlotOrthProj, (size_t)8 * m * sizeof(double));
  // One rank: the kernels that run the whole column MGS of a block on the device, in the order they are
  // tried.  A launch_* that does not take the block returns false having launched nothing that writes it.
  const bool one_rank = !ctx->distributed();
  const bool grid = (flags & EIG_ORTHO_GRID) != 0;
  auto mgs_one_rank = [&](double *Qb, bool first) {
    // 1. the look-ahead whose first read pass is the Gram the caller's product summed
    if (first && gram0 && L == 8 && launch_mgs_lookahead_gram(ctx, n, Qb, gram0, s)) return true;
    // 2. one workgroup (EIG_ORTHO_ONE_WG, n <= 4096)
    if ((flags & EIG_ORTHO_ONE_WG) && !grid && launch_mgs_small(n, Qb, s)) return true;
    // 3. the cooperative launch (EIGMI_MGS_COOP)
    if (!grid && launch_mgs_coop(ctx, n, Qb, S, s)) return true;
    // 4. the look-ahead (L > 1)
    return launch_mgs_lookahead(ctx, n, Qb, L, !(flags & EIG_ORTHO_NO_COOP), s);
  };
  for (i64 bk = 0; bk < m; bk += 8)
  {
    double *Qb = Q + bk * n;
    if (variant == EIG_ORTHO_MGS)
    {
      if (!(one_rank && mgs_one_rank(Qb, bk == 0)))
      {
        // 5. one launch per pass, the sums allreduced between them (any number of ranks)
        for (int k = 0; k <= 8; ++k)
        {
          launch_mgs_pass(n, Qb, k, S, 0, s, ctx->red);
          if (k < 8) allreduce_sum(ctx, S + 8 * k, 8, s);
        }
      }
    }
    else
    {
      // 6. CholQR
      gram_device(ctx, n, 8, 8, Qb, Qb, U);
      launch_cholqr_factor(U, U2, nullptr, 0, s);
      launch_apply_upper(n, Qb, U2, s);
    }
    const i64 mrest = m - bk - 8;
    if (mrest > 0 && variant == EIG_ORTHO_CHOLQR_SPLIT)
    {
      // orthonormalize_avx2_b8 (kernels_avx2.hh:255-381): columns 0-3 of Q_bk first, then 4-7
      // against the updated later blocks.  Each half is the full 8 x mrest Gram with the other
      // half's rows zeroed: those add 0 * q_k, which leaves every entry exactly as it was.
      for (int h = 0; h < 2; ++h)
      {
        gram_device(ctx, n, 8, mrest, Qb, Qb + 8 * n, Sg);
        EIG_HIP(hipMemsetAsync(Sg + (h ? 0 : 4 * mrest), 0, (size_t)4 * mrest * sizeof(double), s));
        launch_project(n, mrest, Qb, Qb + 8 * n, Sg, s);
      }
    }
    else if (mrest > 0)
    {
      gram_device(ctx, n, 8, mrest, Qb, Qb + 8 * n, Sg);
      launch_project(n, mrest, Qb, Qb + 8 * n, Sg, s);
    }
  }
}

// B_orthonormalize_blocked (kernels_cpp.hh:356-591) on the device; *norm (device) receives the
// max off-diagonal R coefficient.
void b_orthonormalize_device(eig_mat_s &B, i64 m, double *Q, double *norm)
{
  eig_ctx_t ctx = B.ctx;
  hipStream_t s = ctx->stream;
  const i64 n = B.nb_rows;
  double *P = (double *)ctx_buffer(ctx, kSlotBOrthP, (size_t)n * 8 * sizeof(double));
  double *G = (double *)ctx_buffer(ctx, kSlotOrthS, 64 * sizeof(double));
  double *U = (double *)ctx_buffer(ctx, kSlotOrthU, 64 * sizeof(double));
  double *Sg = m > 8 ? (double *)ctx_buffer(ctx, kSlotOrthProj, (size_t)8 * m * sizeof(double)) : nullptr;
  EIG_HIP(hipMemsetAsync(norm, 0, sizeof(double), s));
  for (i64 bk = 0; bk < m; bk += 8)
  {
    double *Qb = Q + bk * n;
    launch_spmm_mv8(B, 8, Qb, P, s);                   // P = B Q_bk          (:378-395)
    gram_device(ctx, n, 8, 8, P, Qb, G);               // s = P^T Q_bk        (:450-456)
    launch_cholqr_factor(G, U, norm, 1, s);            // mirror upper, norm, U (:457-526)
    launch_apply_upper(n, Qb, U, s);                   // Q_bk := Q_bk U      (:528-539)
    launch_apply_upper(n, P, U, s);                    // P := P U            (:540-552)
    const i64 mrest = m - bk - 8;
    if (mrest > 0)
    {
      gram_device(ctx, n, 8, mrest, P, Qb + 8 * n, Sg);  // S = P^T Q_bj     (:559-565)
      launch_max_offdiag(Sg, 8, mrest, false, norm, s);  // norm (:566-568)
      launch_project(n, mrest, Qb, Qb + 8 * n, Sg, s);   // Q_bj -= Q_bk S   (:570-584)
    }
  }
}

}  // namespace eigmi

// ============================================================================================
// C entry points
// ============================================================================================
extern "C" int eig_gram_mv8(eig_ctx_t ctx, int64_t n, int64_t m1, int64_t m2, const double *Q1, const double *Q2,
                            double *G)
{
  return guard(ctx, [&] {
    EIG_CHECK(ctx && Q1 && Q2 && G && n >= 0, EIG_ERR_ARG, "eig_gram_mv8: bad argument");
    EIG_MV8_CHECK(m1);
    EIG_MV8_CHECK(m2);
    DeviceGuard dg(ctx->device);
    if (m1 > 0 && m2 > 0) gram_device(ctx, n, m1, m2, Q1, Q2, G);
  });
}

extern "C" int eig_orthonormalize_mv8(eig_ctx_t ctx, int64_t n, int64_t m, double *Q, int variant)
{
  return guard(ctx, [&] {
    EIG_CHECK(ctx && Q && n >= 0, EIG_ERR_ARG, "eig_orthonormalize_mv8: bad argument");
    const int v = variant & 0xff;
    EIG_CHECK(v == EIG_ORTHO_MGS || v == EIG_ORTHO_CHOLQR || v == EIG_ORTHO_CHOLQR_SPLIT, EIG_ERR_ARG,
              "unknown variant");
    EIG_CHECK((variant & ~(0xff | EIG_ORTHO_GRID | EIG_ORTHO_NO_COOP | EIG_ORTHO_ONE_WG | (15 << EIG_ORTHO_LOOKAHEAD_SHIFT))) == 0 &&
                  ((variant >> EIG_ORTHO_LOOKAHEAD_SHIFT) & 15) <= 8,
              EIG_ERR_ARG, "unknown variant flags");
    EIG_MV8_CHECK(m);
    DeviceGuard dg(ctx->device);
    orthonormalize_device(ctx, n, m, Q, variant);
  });
}

extern "C" int eig_orthonormalize_gram_mv8(eig_ctx_t ctx, int64_t n, int64_t m, double *Q, const double *gram)
{
  return guard(ctx, [&] {
    EIG_CHECK(ctx && Q && gram && n >= 0, EIG_ERR_ARG, "eig_orthonormalize_gram_mv8: bad argument");
    EIG_MV8_CHECK(m);
    DeviceGuard dg(ctx->device);
    orthonormalize_device(ctx, n, m, Q, EIG_ORTHO_MGS, gram);
  });
}

extern "C" int eig_spmm_dot_gram_mv8(eig_mat_t mat, int64_t m, const double *Qin, double *Qout, double *dp,
                                     double *gram)
{
  return guard(mat ? mat->ctx : nullptr, [&] {
    EIG_CHECK(mat && Qin && Qout && dp && gram, EIG_ERR_ARG, "eig_spmm_dot_gram_mv8: bad argument");
    EIG_CHECK(m == 8, EIG_ERR_SHAPE, "eig_spmm_dot_gram_mv8: one 8-column block (m = 8)");
    EIG_CHECK(mat->br == 1 && mat->bc == 1, EIG_ERR_BLOCKSIZE,
              "matmul_sparse_tallskinny_blocked: only implemented for FieldMatrix<..,1,1>");
    DeviceGuard dg(mat->ctx->device);
    spmm_dot_gram_device(*mat, Qin, Qout, dp, gram);
  });
}

extern "C" int eig_orthonormalize_passes(eig_ctx_t ctx, int *passes)
{
  return guard(ctx, [&] {
    EIG_CHECK(ctx && passes, EIG_ERR_ARG, "eig_orthonormalize_passes: null argument");
    DeviceGuard dg(ctx->device);
    *passes = mgs_lookahead_passes(ctx);
  });
}

extern "C" int eig_orthonormalize_naive(eig_ctx_t ctx, int64_t n, int64_t m, double *Q)
{
  return guard(ctx, [&] {
    EIG_CHECK(ctx && Q && n >= 0 && m >= 0, EIG_ERR_ARG, "eig_orthonormalize_naive: bad argument");
    EIG_CHECK(m <= 512, EIG_ERR_ARG, "eig_orthonormalize_naive: at most 512 columns");
    DeviceGuard dg(ctx->device);
    hipStream_t s = ctx->stream;
    double *d = (double *)ctx_buffer(ctx, kSlotNaiveDots, (size_t)(m + 1) * sizeof(double));
    // kernels_cpp.hh:128-154: normalise q_k, then q_j -= (q_k . q_j) q_k for every j > k.
    for (i64 k = 0; k < m; ++k)
    {
      double *qk = Q + k * n;
      launch_nrm2sq(n, qk, d + m, 0, s, ctx->red);
      allreduce_sum(ctx, d + m, 1, s);
      launch_scal_dev(n, d + m, true, qk, s);
      const i64 rest = m - k - 1;
      for (i64 j0 = 0; j0 < rest; j0 += 8 * 48)
      {
        const int kk = (int)std::min<i64>(rest - j0, 8 * 48);
        launch_gemv_t(n, kk, Q + (k + 1 + j0) * n, n, qk, d + j0, 0, s, ctx->red);
      }
      allreduce_sum(ctx, d, rest, s);
      // q_j -= d_j q_k : rank-1 update, one axpy per column (same rounding as the reference)
      for (i64 j = 0; j < rest; ++j) launch_axpy_dev(n, d + j, -1.0, qk, Q + (k + 1 + j) * n, s);
    }
  });
}

extern "C" int eig_b_orthonormalize_mv8(eig_mat_t B, int64_t m, double *Q, double *norm)
{
  return guard(B ? B->ctx : nullptr, [&] {
    EIG_CHECK(B && Q && norm, EIG_ERR_ARG, "eig_b_orthonormalize_mv8: null argument");
    EIG_CHECK(B->br == 1 && B->bc == 1, EIG_ERR_BLOCKSIZE,
              "B_orthonormalize_blocked: only implemented for FieldMatrix<..,1,1>");
    EIG_MV8_CHECK(m);
    EIG_CHECK(!B->ctx->distributed(), EIG_ERR_ARG, "eig_b_orthonormalize_mv8: single rank only");
    DeviceGuard dg(B->ctx->device);
    b_orthonormalize_device(*B, m, Q, norm);
  });
}

extern "C" double eig_flops_orthonormalize(int64_t n, int64_t m)
{
  // kernels_cpp.hh:98-106
  double f = 0.0;
  for (i64 k = m; k > 0; k--) f += 2.0 * n + n + (k - 1) * 4.0 * n;
  return f;
}

extern "C" double eig_bytes_orthonormalize_blocked(int64_t n, int64_t m, int b)
{
  // kernels_cpp.hh:157-175
  double c = 0.0;
  for (i64 bk = 0; bk < m; bk += b)
  {
    for (int k = b; k > 0; k--) c += (double)n * k + (double)n * (1 + (k - 1) + 1);
    for (i64 bj = bk + b; bj < m; bj += b) c += 5.0 * b * n;
  }
  return c * 8;
}
