// subspace.h -- what the block eigensolvers (blanczos.cpp, lobpcg.cpp, slice.cpp), the multigrid (mg.cpp) and
// the dense-block drivers (drivers.cpp) share on the launching side; their host arithmetic is subspace_host.h.
#pragma once
#include "internal.h"
#include "subspace_host.h"

namespace eigmi {

// Exchange the ghost rows of every column block of a window-layout multivector.
void halo_mv(const eig_mat_s &A, double *X, i64 m, hipStream_t s);
// Chebyshev-Jacobi semi-iteration (subspace_host.h ChebJacobi) for M X = Bv, `degree` steps on the spectrum
// bounds [lmin, lmax] of diag(M)^-1 M, from X = 0: x_1 = gamma D^-1 b, then degree - 1 fused steps.  Returns
// the buffer (Xa, Xb or Xc) that holds x_degree.  Error in the D-norm <= 2 rho^degree,
// rho = (sqrt(kappa) - 1) / (sqrt(kappa) + 1), kappa = lmax / lmin.
// Xc (optional third buffer): on the box kernel x_{k+1} goes to a buffer of its own instead of over
// the x_{k-1} it reads (interleaved A/B at 256^3: 4.23 vs 4.28 ms per launch; box-to-box spread of
// the same launch is 4.2-4.8 ms).
double *cheb_solve(eig_mat_s &M, i64 m, int degree, double lmin, double lmax, const double *Bv, const double *dinv,
                   double *Xa, double *Xb, double *Xc, hipStream_t s);

// CholQR2 in the M-inner product (block Lanczos, LOBPCG and spectrum slicing): Z (b columns) = Vdst R with
// Vdst M-orthonormal, R (b x b upper, row-major) to the host in Rtot.  Vdst may equal Z.  M == nullptr is
// M = I (MZ unused).  finish_mz: MZ = M Vdst on return (the factors applied to M Z as to Z; the fused
// b = 32 middle step, which never stores M Z R0^-1, is then not taken).  `recomputed` counts second
// passes that recomputed M Z.  False on a non-positive pivot (Vdst is then not usable).
// The b x b factorisations run on the device (k_chol_small: the host chol_upper / tri_upper_inv arithmetic);
// two host round trips: R0 in the middle to pick the second pass (cholqr_reuse), R and the breakdown flag at
// the end.  The pick is a heuristic: the spread of R0's diagonal is only a lower bound on cond(R0), so an
// ill-conditioned block with an even diagonal can still take the reuse path (its second pass then restores
// M-orthonormality to ~eps cond(Z) instead of ~eps).
struct CholQr2 {
  eig_mat_s *M = nullptr;
  eig_ctx_t ctx = nullptr;
  int b = 0;
  i64 n = 0, ld = 0, own = 0;
  double *MZ = nullptr;     // b columns, window layout
  double *small = nullptr;  // 2 b b doubles: Gram, inverse factor
  double *chol = nullptr;   // 2 b b doubles + 64 bytes: R, Rtot and the flag
  bool finish_mz = false;
};
inline CholQr2 cholqr_args(eig_ctx_t ctx, eig_mat_s *M, int b, i64 n, i64 ld, i64 own, double *MZ, double *small,
                           double *chol, bool finish_mz)
{
  return CholQr2{M, ctx, b, n, ld, own, MZ, small, chol, finish_mz};
}
bool mcholqr2_mv(const CholQr2 &q, double *Z, double *Vdst, std::vector<double> &Rtot, long long &recomputed);

// h -> d / d -> h (h.size() doubles) on s, then a stream synchronisation: h is pageable and may go out of scope
void upload(const std::vector<double> &h, double *d, hipStream_t s);
void download(std::vector<double> &h, const double *d, hipStream_t s);
// `count` timing events, destroyed with the holder
struct TimingEvents {
  std::vector<hipEvent_t> ev;
  TimingEvents() = default;
  explicit TimingEvents(size_t count);
  ~TimingEvents();
  TimingEvents(const TimingEvents &) = delete;
  TimingEvents &operator=(const TimingEvents &) = delete;
  hipEvent_t *data() { return ev.data(); }
  hipEvent_t operator[](size_t i) const { return ev[i]; }
};
// H (N x N, row-major, device) read back, then ritz_select: the m wanted eigenpairs in the order of `which`
void small_ritz(int N, const double *Hdev, int m, int which, std::vector<double> &theta, std::vector<double> &Cx,
                hipStream_t s);
// R = KX - MX diag(theta) into `dst` (launch_lobpcg_resid) and its 2 m column sums read back from sums_d:
// sums[j] = ||r_j||^2, sums[m + j] = ||(MX)_j||^2
void residual_sums(eig_ctx_t ctx, i64 n, i64 ld, i64 m, const double *KX, const double *MX, const double *theta_d,
                   double *dst, double *sums_d, std::vector<double> &sums, hipStream_t s);
// evec_host[q][r] = scale[q] * Q(r, cols[q]) for q < nev, r < n: Q a device multivector of
// MultiVector<double,8> blocks ld rows apart with its owned rows at `own`.  cols == nullptr: columns 0 .. nev - 1;
// scale == nullptr: 1.  evec_host == nullptr: nothing.  Synchronises the stream.
void copy_evecs(eig_ctx_t ctx, const double *Q, i64 ld, i64 own, i64 n, int nev, const int *cols, const double *scale,
                double *evec_host);
// Q (n x m, single rank) = mt19937(seed) normals in MultiVector fill order (block, row, col) = the flat order
// (eig_random_mv8; eigensolver.hh:50-55 / :137-142 / :222-227)
void random_block(eig_ctx_t ctx, i64 n, i64 m, unsigned seed, double *Q);
// A on one rank (EIG_ERR_ARG), of square blocks 1..4 (EIG_ERR_BLOCKSIZE, `who` + `blocks_text`), square with
// window = its scalar rows (EIG_ERR_SHAPE); sell_r1: and a SELL image of one row per lane
void check_square_single_rank(const eig_mat_s *A, const char *who, const char *blocks_text, bool sell_r1);
// the body of a workspace's destroy entry point: the context's stream drained, then the workspace deleted
template <class W>
int destroy_workspace(W *w, eig_ctx_t ctx)
{
  (void)hipSetDevice(ctx->device);
  (void)hipStreamSynchronize(ctx->stream);
  delete w;
  return EIG_OK;
}

}  // namespace eigmi
