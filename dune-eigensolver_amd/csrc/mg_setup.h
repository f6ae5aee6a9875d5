// mg_setup.h -- host setup of the geometric multigrid hierarchy (mg.cpp uploads what this builds): the node
// coarsening rule, the Galerkin operator P^T A P on b x b blocks, the smoother data of a level (scalar or block
// Jacobi with its Gershgorin bound) and the coarsest level's spectrum bounds.  Plain host arithmetic: no device
// code, no HIP runtime call and no context, so host tests compile mg_setup.cpp (with dense.cpp) and need no GPU.
#pragma once
#include "internal.h"

#include <vector>

namespace eigmi {

// largest coarsest level (scalar rows) whose preconditioned spectrum is computed densely on the host
constexpr i64 kMgMaxCoarse = 1024;

// Host block-CSR of one level (mat_download_bcsr's layout: block rows with ascending block columns, block q
// is b x b values, row-major, at val[q * b * b]).
struct MgCsr {
  std::vector<i64> rp;
  std::vector<i32> col;
  std::vector<double> val;
};

// A level is the last one at <= 64 nodes or a direction below 3 nodes.
inline bool mg_last_level(const int *dim)
{
  return (i64)dim[0] * dim[1] * dim[2] <= 64 || dim[0] < 3 || dim[1] < 3 || dim[2] < 3;
}
// Scalar rows (nodes * b) of the coarsest level that nx x ny x nz nodes coarsen to.
i64 mg_coarsest_rows(int nx, int ny, int nz, int b);

// A_c = (P (x) I_b)^T A (P (x) I_b), P trilinear from the coarse nodes at the odd fine indices (cd = fd / 2), on
// the 27-point coarse stencil with a b x b block per slot.  Coarse rows are computed independently (threads over
// coarse nodes), each gathering its fine rows in z, y, x order; then mirrored, so that A_c is bitwise symmetric:
// block (J, I), J < I, is the transpose of the block computed for (I, J), and a diagonal block's lower triangle
// comes from its upper.  EIG_ERR_ARG when A couples nodes more than one grid step apart.
void mg_galerkin(const MgCsr &A, int b, const int *fd, const int *cd, MgCsr &Ac);

// Scalar Jacobi (b = 1): the Gershgorin bound max_r sum_c |a_rc| / a_rr of D^-1 A.  EIG_ERR_BREAKDOWN for a
// non-positive diagonal entry.
double mg_gershgorin(const MgCsr &A, i64 n);
// Block Jacobi: dinv = the inverses of the nb diagonal blocks (b x b row-major each, bitwise symmetric) and the
// block Gershgorin bound max_I sum_J ||L_I^-1 A_IJ L_J^-T||_2 of D^-1 A, D_I = L_I L_I^T (the 2-norm from
// sym_eig).  EIG_ERR_BREAKDOWN for a diagonal block that is missing or not positive definite.
double mg_block_jacobi(const MgCsr &A, i64 nb, int b, std::vector<double> &dinv);

// Exact spectrum bounds of D^-1 A on a small level: the dense symmetric eigenvalues of L^-1 A L^-T with D = L L^T
// the block diagonal (b = 1: D^-1/2 A D^-1/2).  EIG_ERR_BREAKDOWN when the level is not positive definite.
void mg_spectrum_bounds(const MgCsr &A, i64 nb, int b, double &lo, double &hi);

// Chebyshev degree that solves the coarsest level to 1e-15 on the bounds [clo, chi] (1 .. 2000).
int mg_coarse_degree(double clo, double chi);

}  // namespace eigmi
