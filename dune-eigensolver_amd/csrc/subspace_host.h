// subspace_host.h -- host arithmetic shared by the block eigensolvers (blanczos.cpp, lobpcg.cpp, slice.cpp)
// and the Chebyshev-Jacobi users (subspace.cpp cheb_solve, mg.cpp).  No device code, no HIP header and no
// context: host tests compile subspace_host.cpp with dense.cpp alone and need no GPU.
#pragma once
#include <cstdint>
#include <vector>

#include "../../include/eigmi.h"

namespace eigmi {

// H (N x N, row-major) <- (H + H^T) / 2
void symmetrise(int N, std::vector<double> &H);
// H symmetrised and diagonalised (sym_eig): the m wanted eigenpairs, theta in the order of `which` (EIG_WHICH_SA
// ascending, EIG_WHICH_LA descending), Cx (N x m, row-major) their eigenvectors
void ritz_select(int N, std::vector<double> &H, int m, int which, std::vector<double> &theta, std::vector<double> &Cx);
// Q (N x m, row-major) = the orthonormal factor of A's Householder QR (A: N x m, N >= m, overwritten)
void householder_q(int N, int m, std::vector<double> &A, std::vector<double> &Q);
// LOBPCG's C = [C_x C_p] (N x 2 m, row-major): C_p = C_x with its X rows (the first m) zeroed, orthogonalised
// twice against C_x, then orthonormalised
void search_coefficients(int N, int m, const std::vector<double> &Cx, std::vector<double> &C);
// The block tridiagonal T (k b x k b, row-major) of k block Lanczos steps: A holds A_j (b x b), B holds
// B_{j+1} (b x b, upper) per step; T_{j+1,j} = B_{j+1}, T_{j,j+1} = B_{j+1}^T (B of the last step is not read)
std::vector<double> block_tridiag(int b, int k, const std::vector<double> &A, const std::vector<double> &B);
// Shift-invert selection: pick = the nev Ritz values th of OP = (K - sigma M)^-1 M of largest |th| (the
// eigenvalues nearest sigma), ordered by lambda = sigma + 1 / th ascending (EIG_WHICH_SA) or descending (LA);
// th is overwritten by lambda (th == 0: HUGE_VAL).  Both sorts are stable.
void si_ritz_order(std::vector<double> &th, double sigma, int nev, int which, std::vector<int> &pick);
// LOBPCG: ||r_j|| <= tol |theta_j| ||M x_j|| for every j < nev, from sums[j] = ||r_j||^2, sums[m + j] = ||(M x)_j||^2
bool lobpcg_converged(const std::vector<double> &sums, const std::vector<double> &theta, int m, int nev, double tol);
// Spectrum slicing: a pair is accepted when theta lies in [a, b]; the window has converged when it holds at
// least one accepted pair and every accepted one has ||r_j|| <= tol max(|theta_j|, |a|, |b|) ||x_j||
// (rr[j] = ||r_j||^2, xx[j] = ||x_j||^2; no residuals yet, rr empty: false)
inline bool window_accept(double theta, double a, double b) { return theta >= a && theta <= b; }
bool window_converged(const std::vector<double> &theta, const std::vector<double> &rr, const std::vector<double> &xx,
                      double a, double b, double tol);
// max |G - I| of an N x N Gram; a NaN entry counts as a miss (HUGE_VAL)
double orth_deviation(int N, const std::vector<double> &G);

// Scalars of the Chebyshev-Jacobi semi-iteration (Golub-Varga three-term form) on the spectrum bounds
// [lmin, lmax] of D^-1 A: x_1 = gamma D^-1 b, x_{k+1} = omega_{k+1} (x_k + gamma D^-1 (b - A x_k) - x_{k-1}) + x_{k-1}
struct ChebJacobi {
  double gamma, mu;
  ChebJacobi(double lmin, double lmax) : gamma(2.0 / (lmin + lmax)), mu((lmax - lmin) / (lmax + lmin)) {}
  double omega1() const { return 1.0 / (1.0 - 0.5 * mu * mu); }
  double next(double omega) const { return 1.0 / (1.0 - 0.25 * mu * mu * omega); }  // omega_{k+1} from omega_k
};

// R0 diagonal spread beyond which CholQR2's second pass recomputes M Z instead of reusing (M Z) R0^-1
constexpr double kCholQrReuseCond = 1e4;
// whether the first factor R0 (b x b, row-major) allows the reuse: every pivot non-zero and
// max |r_ii| <= kCholQrReuseCond min |r_ii|
bool cholqr_reuse(int b, const std::vector<double> &R0);
// out[r] = scale * column j of a host copy h of MultiVector<double,8> blocks: column blocks of 8, ld rows
// apart, owned rows (n of them) from row `own` -- h[((j / 8) ld + own + r) 8 + j % 8]
void mv8_column(const double *h, int64_t ld, int64_t own, int64_t n, int j, double scale, double *out);

}  // namespace eigmi
