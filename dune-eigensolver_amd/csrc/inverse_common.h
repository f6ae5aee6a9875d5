// inverse_common.h -- private to the drivers that apply LU factors (drivers.cpp: StandardInverse /
// GeneralizedInverse; shift_invert.cpp: the shift-invert Lanczos and Arnoldi drivers): the checks on their
// matrices and the choice between the caller's factors and a host factorisation.
#pragma once
#include "krylov_host.h"

namespace eigmi {

// The factors the inverse drivers apply: the caller's, or a host factorisation (owned).
struct LuRef {
  eig_lu_t lu = nullptr;
  bool owned = false;
  ~LuRef()
  {
    if (owned) eig_lu_destroy(lu);
  }
};

// F = the caller's factors `lu`, or (lu null) a host factorisation of csr() -- a host copy with A's shape,
// assembled only then -- and in either case of n scalar rows, else EIG_ERR_SHAPE with the text `mismatch`.
template <class Csr>
void select_factors(eig_mat_s &A, eig_lu_t lu, i64 n, const char *mismatch, LuRef &F, Csr csr)
{
  F.lu = lu;
  if (!lu)
  {
    const HostCsr &h = csr();
    const int rc = eig_lu_create_bcsr(A.ctx, A.nb_rows, A.br, h.rp.data(), h.c.data(), h.v.data(), &F.lu);
    EIG_CHECK(rc == EIG_OK, rc, std::string("LU factorisation: ") + eig_last_error(A.ctx));
    F.owned = true;
  }
  EIG_CHECK(lu_size(F.lu) == n, EIG_ERR_SHAPE, mismatch);
}

// blocks: the caller runs on square blocks 1..4 (StandardInverse, the symmetric shift-invert
// drivers); the others keep the reference's FieldMatrix<..,1,1> restriction
inline void check_inverse_matrix(const eig_mat_s *A, const char *who, bool blocks = false)
{
  EIG_CHECK(A->br == A->bc, EIG_ERR_ARG, std::string(who) + ": blocks of input matrix must be square");
  EIG_CHECK(blocks || A->br == 1, EIG_ERR_BLOCKSIZE,
            "matmul_sparse_tallskinny_blocked: only implemented for FieldMatrix<..,1,1>");
  EIG_CHECK(!A->ctx->distributed(), EIG_ERR_ARG, std::string(who) + ": single rank only");
  EIG_CHECK(A->nb_rows == A->nb_cols, EIG_ERR_SHAPE, std::string(who) + ": square matrix required");
}

}  // namespace eigmi
