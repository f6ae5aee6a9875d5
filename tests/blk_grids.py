"""Blocked (b x b) box-stencil matrices on nx x ny x nz node grids -- test infrastructure only (imported like
box_grids.py).  A = kron(Ka, C1) + kron(Kb, C2) with Ka the 7-point and Kb the 27-point "edge" matrix of
box_grids.box_matrix (both SPD: symmetric, strictly diagonally dominant, positive diagonal) and C1, C2 two SPD
b x b matrices that do not commute: A is SPD, its blocks couple all components, and it is no single Kronecker
product (no common eigenbasis of the components that a smoother could get right by accident).  Node-major rows
(scalar row = node * b + component), block columns ascending."""
import numpy as np
import scipy.sparse as sp

import box_grids
import oracle


def couplings(b):
    """Two non-commuting SPD b x b matrices: the tridiagonal [1, 2, 1]-like T (spectrum inside (0, 4)) and a
    diagonal-plus-rank-one matrix."""
    C1 = 2.0 * np.eye(b) + np.diag(np.ones(b - 1), 1) + np.diag(np.ones(b - 1), -1)
    v = np.arange(1.0, b + 1.0)
    C2 = np.diag(1.0 + 0.5 * np.arange(b)) + 0.25 * np.outer(v, v)
    assert np.abs(C1 @ C2 - C2 @ C1).max() > 0.1
    assert np.linalg.eigvalsh(C1)[0] > 0 and np.linalg.eigvalsh(C2)[0] > 0
    return C1, C2


def to_blocked(S, b):
    """scipy matrix of the scalar expansion -> oracle.CSR with b x b blocks (ascending block columns)."""
    B = sp.bsr_matrix(S, blocksize=(b, b))
    B.sort_indices()
    return oracle.CSR(B.shape[0] // b, B.indptr.astype(np.int64), B.indices.astype(np.int32),
                      np.ascontiguousarray(B.data, dtype=np.float64).reshape(-1), b, b)


def expand(A):
    """Scalar expansion of a blocked oracle.CSR as scipy CSR."""
    n = A.nrows * A.br
    S = sp.bsr_matrix((A.val.reshape(-1, A.br, A.bc), A.col, A.rowptr), shape=(n, A.nrows * A.bc)).tocsr()
    S.sort_indices()
    return S


def blk_matrix(dims, b, seed=0):
    """-> (oracle.CSR with b x b blocks, scipy CSR of its scalar expansion)."""
    Ka = box_grids.to_scipy(box_grids.box_matrix(dims, "p7", "edge", seed))
    Kb = box_grids.to_scipy(box_grids.box_matrix(dims, "full27", "edge", seed + 1))
    C1, C2 = couplings(b)
    S = (sp.kron(Ka, C1) + sp.kron(Kb, C2)).tocsr()
    A = to_blocked(S, b)
    return A, expand(A)


def two_step_matrix(dims, b):
    """A blocked SPD matrix that couples nodes two grid steps apart in x (not a box stencil on `dims`)."""
    n = dims[0] * dims[1] * dims[2]
    x = np.arange(n) % dims[0]
    i = np.arange(n)[x + 2 < dims[0]]
    K = sp.csr_matrix((np.full(i.size, -1.0), (i, i + 2)), shape=(n, n))
    K = (K + K.T + 4.0 * sp.identity(n)).tocsr()
    A = to_blocked(sp.kron(K, couplings(b)[0]).tocsr(), b)
    return A
