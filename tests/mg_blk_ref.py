"""numpy restatement of the multigrid inner solve on square blocks b x b (dune-eigensolver_amd/csrc/mg_setup.cpp,
mg.cpp, k_mg.hip, k_mv8.hip) -- test infrastructure only.  It is tests/mg_ref.py with P (x) I_b and block Jacobi:
coarsening by nodes (odd-index coarse nodes, trilinear P per node, identity on the b components), Galerkin
P^T A P mirrored from its upper triangle, the Chebyshev recurrence of mg_ref.cheb_solve with D the block diagonal
(z = D_I^-1 (b - A x) per node), lmax the block Gershgorin bound max_I sum_J ||L_I^-1 A_IJ L_J^-T||_2 with
D_I = L_I L_I^T, levels until <= 64 nodes or a direction below 3 nodes, the coarsest level solved by the same
recurrence on the exact spectrum of L^-1 A L^-T.  Double precision with another rounding order, so results agree
with the device to the restatement's own sensitivity (tests/test_mg_blk_ref.py), not bitwise.

Matrices are scipy CSR of the scalar expansion (node-major: scalar row = node * b + component)."""
import numpy as np
import scipy.sparse as sp

import mg_ref


def diag_blocks(A, b):
    """(nodes, b, b): the diagonal blocks of the scalar-expanded A."""
    B = A.tobsr((b, b))
    B.sort_indices()
    nb = B.shape[0] // b
    rows = np.repeat(np.arange(nb), np.diff(B.indptr))
    on = B.indices == rows
    D = np.zeros((nb, b, b))
    D[rows[on]] = B.data[on]
    return D


def block_inverse(A, b):
    """The block-diagonal D^-1 as a sparse matrix (each block symmetrised bitwise) and L_I^-1 per node."""
    D = diag_blocks(A, b)
    L = np.linalg.cholesky(D)  # raises LinAlgError for a block that is not positive definite
    Li = np.linalg.inv(L)
    Dinv = np.einsum("nki,nkj->nij", Li, Li)
    Dinv = 0.5 * (Dinv + Dinv.transpose(0, 2, 1))
    nb = D.shape[0]
    return sp.bsr_matrix((Dinv, np.arange(nb), np.arange(nb + 1)), shape=A.shape).tocsr(), Li


def block_gershgorin(A, b, Li):
    """max_I sum_J ||L_I^-1 A_IJ L_J^-T||_2"""
    B = A.tobsr((b, b))
    nb = B.shape[0] // b
    rows = np.repeat(np.arange(nb), np.diff(B.indptr))
    N = Li[rows] @ B.data @ Li[B.indices].transpose(0, 2, 1)
    return float(np.bincount(rows, weights=np.linalg.norm(N, 2, axis=(1, 2)), minlength=nb).max())


def last_level(dims):
    return dims[0] * dims[1] * dims[2] <= 64 or min(dims) < 3


def level_dims(dims):
    """The node grids of the hierarchy on `dims`."""
    out = [tuple(dims)]
    while not last_level(out[-1]):
        out.append(tuple(d // 2 for d in out[-1]))
    return out


def cheb_solve(A, Dinv, rhs, degree, lmin, lmax):
    """mg_ref.cheb_solve with the block-diagonal D^-1 (a sparse matrix) in place of the scalar 1 / a_ii."""
    gamma = 2.0 / (lmin + lmax)
    mu = (lmax - lmin) / (lmax + lmin)
    xa = gamma * (Dinv @ rhs)
    if degree <= 1:
        return xa
    xb = np.zeros_like(rhs)
    omega = 1.0
    for k in range(1, degree):
        omega = 1.0 / (1.0 - 0.5 * mu * mu) if k == 1 else 1.0 / (1.0 - 0.25 * mu * mu * omega)
        xn = omega * (xa + gamma * (Dinv @ (rhs - A @ xa)) - xb) + xb
        xb, xa = xa, xn
    return xa


class Multigrid:
    def __init__(self, A, dims, b, smooth_degree=2, smooth_ratio=10.0):
        self.nu, self.ratio, self.b = smooth_degree, smooth_ratio, b
        self.levels = []
        A = A.tocsr()
        dims = tuple(dims)
        assert dims[0] * dims[1] * dims[2] * b == A.shape[0]
        Ib = sp.identity(b, format="csr")
        while True:
            Dinv, Li = block_inverse(A, b)
            lev = {"A": A, "Dinv": Dinv, "dims": dims, "lmax": block_gershgorin(A, b, Li)}
            self.levels.append(lev)
            if last_level(dims):
                nb = Li.shape[0]
                Lh = sp.bsr_matrix((Li, np.arange(nb), np.arange(nb + 1)), shape=A.shape).toarray()
                S = Lh @ A.toarray() @ Lh.T
                w = np.linalg.eigvalsh(0.5 * (S + S.T))
                lev["clo"], lev["chi"] = w[0] * 0.999, w[-1] * 1.001
                kappa = lev["chi"] / lev["clo"]
                rho = (np.sqrt(kappa) - 1) / (np.sqrt(kappa) + 1)
                lev["cdeg"] = min(max(int(np.ceil(np.log(0.5e-15) / np.log(rho))) if rho > 0 else 1, 1), 2000)
                break
            Pn, cd = mg_ref.prolongation(dims)
            P = sp.kron(Pn, Ib).tocsr()
            lev["P"] = P
            A = mg_ref.mirror_upper((P.T @ A @ P).tocsr())
            dims = cd

    def info(self):
        L = self.levels[-1]
        return {"levels": len(self.levels), "coarse_rows": L["A"].shape[0], "coarse_degree": L["cdeg"],
                "lmax_fine": self.levels[0]["lmax"]}

    def vcycle(self, l, rhs):
        L = self.levels[l]
        if l + 1 == len(self.levels):
            return cheb_solve(L["A"], L["Dinv"], rhs, L["cdeg"], L["clo"], L["chi"])
        lo, hi = L["lmax"] / self.ratio, L["lmax"]
        x = cheb_solve(L["A"], L["Dinv"], rhs, self.nu, lo, hi)
        r = rhs - L["A"] @ x
        x = x + L["P"] @ self.vcycle(l + 1, L["P"].T @ r)
        r = rhs - L["A"] @ x
        return x + cheb_solve(L["A"], L["Dinv"], r, self.nu, lo, hi)

    def solve(self, rhs, cycles):
        A = self.levels[0]["A"]
        r = rhs.copy()
        x = None
        for it in range(cycles):
            e = self.vcycle(0, r)
            x = e if x is None else x + e
            if it + 1 < cycles:
                r = r - A @ e
        return x
