// amg_setup.h -- host setup of the smoothed-aggregation algebraic multigrid hierarchy (mg.cpp uploads what this
// builds): strength of connection, the three-pass aggregation, the smoothed prolongator P = (I - omega D^-1 A) T
// with its explicit transpose, the Galerkin operator P^T (A P) and the stopping rule.  1 x 1 blocks, symmetric
// positive definite matrices.  Plain host arithmetic like mg_setup.*: no device code, no HIP runtime call and no
// context, so host tests compile amg_setup.cpp (with mg_setup.cpp and dense.cpp) and need no GPU.
#pragma once
#include "mg_setup.h"

#include <vector>

namespace eigmi {

constexpr i64 kAmgCoarsestRows = 256;  // a level of at most this many rows is the coarsest
constexpr int kAmgMaxLevels = 16;

// Aggregates of the n x n matrix A (CSR, ascending columns) at the strength threshold theta_l: entry j != i of
// row i is strong when fabs(a_ij) >= theta_l * sqrt(a_ii * a_jj).  Three serial passes over the rows in ascending
// order:
//   1. an unaggregated row with at least one strong neighbour, all of them unaggregated, founds an aggregate of
//      itself and those neighbours;
//   2. each remaining row joins the aggregate, as it stood after pass 1, of its strongest aggregated strong
//      neighbour (largest fabs(a_ij), ties to the lowest column);
//   3. each row still left founds an aggregate of itself and its still unaggregated strong neighbours (a row
//      without a strong neighbour becomes a singleton).
// agg[i] in [0, returned count).  EIG_ERR_BREAKDOWN for a non-positive (or missing) diagonal entry.
i64 amg_aggregate(i64 n, const i64 *rp, const i32 *col, const double *val, double theta_l, std::vector<i64> &agg);

// P = (I - omega D^-1 A) T, T[i, agg(i)] = 1, omega = 4 / (3 lmax): n x nc CSR with ascending columns, exact zeros
// dropped.  Row i: acc[agg(j)] += (omega / a_ii) * a_ij over the stored j in turn, then P[i, J] = T[i, J] - acc[J].
void amg_prolongator(const MgCsr &A, i64 n, const std::vector<i64> &agg, i64 nc, double lmax, MgCsr &P);

// PT = P^T (nc x n CSR, ascending columns), values copied.
void amg_transpose(const MgCsr &P, i64 n, i64 nc, MgCsr &PT);

// A_c = P^T (A P): AP row i = sum over the stored j of row i of A, in turn, of a_ij * P[j, :]; A_c row I = sum over
// the stored k of row I of PT, in turn, of PT[I, k] * AP[k, :] (threads over rows; a row's sums never depend on the
// thread count).  Then mirrored from its upper triangle like mg_galerkin, so A_c is bitwise symmetric, and exact
// zeros dropped.
void amg_galerkin(const MgCsr &A, const MgCsr &P, const MgCsr &PT, i64 n, i64 nc, MgCsr &Ac);

struct AmgHierarchy {
  std::vector<MgCsr> A;       // A[0] the fine matrix .. A.back() the coarsest
  std::vector<MgCsr> P, PT;   // P[l]: rows(l) x rows(l + 1); one fewer than A
  std::vector<i64> rows;      // rows per level
  std::vector<double> lmax;   // Gershgorin bound of D^-1 A per level
  double clo = 0.0, chi = 0.0;  // coarsest: spectrum bounds of D^-1 A, widened by 0.999 / 1.001
  int cdeg = 0;                 // coarsest: Chebyshev degree (mg_coarse_degree)
};

// The hierarchy of A0 (n rows): theta_l = theta * 0.5^l per level.  A level of <= kAmgCoarsestRows rows is the
// coarsest; one that coarsens by less than a factor 2 (or the kAmgMaxLevels-th) is the coarsest when it has <=
// kMgMaxCoarse rows, else EIG_ERR_ARG with the level sizes reached in the message.  EIG_ERR_BREAKDOWN for a
// non-positive diagonal entry or a coarsest level that is not positive definite.
void amg_build(MgCsr A0, i64 n, double theta, AmgHierarchy &H);

}  // namespace eigmi
