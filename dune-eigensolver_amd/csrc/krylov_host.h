// krylov_host.h -- host arithmetic shared by the shift-invert Lanczos and Arnoldi drivers (shift_invert.cpp) and
// the inverse-iteration drivers (drivers.cpp).  No device code and no HIP runtime call: host tests compile
// krylov_host.cpp (with dense.cpp) and no GPU.
#pragma once
#include "internal.h"

#include <algorithm>
#include <cmath>
#include <complex>
#include <numeric>
#include <utility>
#include <vector>

namespace eigmi {

// Host block-CSR copy of a matrix (mat_download_bcsr's layout: ascending columns per row; block q is b x b
// values, row-major, at v[q * b * b]).
struct HostCsr {
  std::vector<i64> rp;
  std::vector<i32> c;
  std::vector<double> v;
};
// Pattern updates of A's copy on block rows [r0, r1).  alpha = 0 touches and checks nothing.  EIG_ERR_SHAPE
// texts: "<who>: pattern(B) must be contained in pattern(A)", "<who>: A has no diagonal entry".
// A += alpha B on A's pattern:
void pattern_axpy(i64 r0, i64 r1, int b, HostCsr &A, double alpha, const HostCsr &B, const char *who);
// alpha onto the diagonal entries of the diagonal blocks:
void pattern_shift_diag(i64 r0, i64 r1, int b, HostCsr &A, double alpha, const char *who);

// ARPACK++ defaults: ncv = 0 (auto), tol = 0 (machine precision), maxit = 0 (100 nev)
inline int arpack_ncv(i64 n, int nev, int ncv) { return ncv > 0 ? ncv : (int)std::min<i64>(n, std::max(2 * nev + 1, 20)); }
inline double arpack_tol(double tol) { return tol > 0.0 ? tol : 2.220446049250313e-16; }
inline int arpack_maxit(int nev, int maxit) { return maxit > 0 ? maxit : 100 * nev; }

// Read-back row of an extension column (basis of m vectors): the two CGS passes' coefficients (m + 1 each), ||w||^2
inline i64 extension_stride(int m) { return 2 * (i64)(m + 1) + 1; }
// Column j from its row: ctot[0 .. j] = the two passes summed (ctot has m + 1 entries), returns beta_j;
// beta_j <= 1e-14 max|ctot| throws EIG_ERR_BREAKDOWN with the text `breakdown`.
double extension_column(int m, int j, const double *row, std::vector<double> &ctot, const char *breakdown);

// "LM": ord = the indices of w, largest |w| first (stable: equal moduli, so conjugate partners, keep their order)
template <class T>
void order_largest_magnitude(const std::vector<T> &w, std::vector<int> &ord)
{
  ord.resize(w.size());
  std::iota(ord.begin(), ord.end(), 0);
  std::stable_sort(ord.begin(), ord.end(), [&](int a, int b) { return std::abs(w[a]) > std::abs(w[b]); });
}
// vectors a thick restart keeps of a basis of m
inline int thick_restart_size(int m, int nev) { return std::min(m - 2, nev + (m - nev) / 2); }

// Krylov-Schur restart of the Arnoldi driver (shift_invert.cpp "Non-symmetric modes") on the decomposition
// OP V = V G + f cvec^T (G m x m row-major; its eigenpairs (w, Y) as gen_eig returns them, in "LM" order
// `ord`): the kept units (eigenvalue index, complex pair), kk columns in all; Z (m x kk row-major), their
// real and imaginary parts orthonormalised; G <- Z^T G Z (leading kk x kk of the m x m array), cvec <- Z^T cvec.
void krylov_schur_restart(int m, int nev, std::vector<double> &G, std::vector<double> &cvec,
                          const std::vector<std::complex<double>> &w, const std::vector<std::complex<double>> &Y,
                          const std::vector<int> &ord, int &kk, std::vector<double> &Z,
                          std::vector<std::pair<int, bool>> &units);

}  // namespace eigmi
