"""The eigen drivers on blocked matrices (BCRSMatrix<FieldMatrix<double,3,3>>, single rank):
StandardInverse and computeGenSymShiftInvertMinMagnitude run with n = nb_rows * br on the blocked
SpMM (k_spmm_blk_mv8), BCRSMatrix::mv and the factorisation of the blocked matrix.  The reference's
subspace iterations throw on blocks ("only implemented for FieldMatrix<..,1,1>"); its shift-invert
wrapper does not.  StandardLargest keeps the reference's refusal (tests/test_gpu_drivers.py pins it).

References: the oracle restatements of the drivers on the matrix's scalar expansion (the blocked
product is bitwise the 1x1 product on it, tests/test_gpu_blocked_spmm.py) and numpy's dense
eigensolver.

Matrix: the scaling S A S of A = q1elast(5) (125 block rows, n = 375), s_i = 1 + 0.25 sin(1.7 i), which is bitwise symmetric with a simple spectrum (smallest
four eigenvalues 0.38255, 0.67736, 0.68372, 0.70662, relative gaps >= 0.9 %) -- the plain q1elast
spectrum is heavily degenerate, which makes a one-vector Lanczos comparison depend on rounding.
The drivers that stay FieldMatrix<..,1,1>-only are asserted to refuse blocks."""
import numpy as np
import pytest

import eigmi
import oracle
from test_gpu_blocked_spmm import expand

pytestmark = pytest.mark.gpu

_cache = {}


def mats():
    """S A S and B (blocked oracle.CSR), the expansion of S A S and the dense spectra; built once."""
    if not _cache:
        A = oracle.q1elast(5)
        n = A.n
        s = 1.0 + 0.25 * np.sin(1.7 * np.arange(n))
        I = np.repeat(np.arange(A.nrows), np.diff(A.rowptr))
        J = A.col.astype(np.int64)
        r = np.arange(3)
        srow = s[(I[:, None] * 3 + r)][:, :, None]   # (nnzb, 3, 1)
        scol = s[(J[:, None] * 3 + r)][:, None, :]   # (nnzb, 1, 3)
        S = oracle.CSR(A.nrows, A.rowptr, A.col, (A.val.reshape(-1, 3, 3) * (srow * scol)).reshape(-1), 3, 3)
        ES = expand(S.rowptr, S.col, S.val, 3)
        DS = ES.to_scipy().toarray()
        assert np.array_equal(DS, DS.T)
        # B: block diagonal, block I = (1 + 0.1 (I mod 3)) [[2, .5, 0], [.5, 2, .5], [0, .5, 2]]
        T = np.array([[2.0, 0.5, 0.0], [0.5, 2.0, 0.5], [0.0, 0.5, 2.0]])
        bval = ((1.0 + 0.1 * (np.arange(A.nrows) % 3))[:, None, None] * T).reshape(-1)
        B = oracle.CSR(A.nrows, np.arange(A.nrows + 1, dtype=np.int64), np.arange(A.nrows, dtype=np.int32), bval, 3, 3)
        DB = expand(B.rowptr, B.col, B.val, 3).to_scipy().toarray()
        L = np.linalg.cholesky(DB)
        Li = np.linalg.inv(L)
        _cache.update(S=S, ES=ES, DS=DS, B=B, DB=DB, wS=np.linalg.eigvalsh(DS),
                      wG=np.linalg.eigvalsh(Li @ DS @ Li.T))
    return _cache


def up(ctx, A):
    return eigmi.Matrix.from_bcsr(ctx, A.rowptr, A.col, A.val, A.br, A.bc)


# ------------------------------------------------------------------------------ StandardInverse
def test_standard_inverse_vs_oracle(ctx):
    """10 fixed iterations with exported factors of the blocked matrix against the oracle driver on
    the expansion with those factors: the same counter, values to rtol 1e-12 (the bar of
    tests/test_inverse.py::test_standard_inverse_vs_oracle)."""
    d = mats()
    S = d["S"]
    M = up(ctx, S)
    lu = eigmi.LU.from_bcsr(ctx, S.rowptr, S.col, S.val, br=3)
    f = oracle.LU(**lu.export())
    assert f.n == 375
    ev, _, it = eigmi.standard_inverse(M, 0.0, 0.0, 10, 4, 123, lu=lu)
    rev, _, rit = oracle.standard_inverse(d["ES"], f, 0.0, 0.0, 10, 4, 123)
    print(f"blocked StandardInverse 10 iterations: max rel |ev - ev_ref| = {np.abs(ev / rev - 1).max():.2e}")
    assert it == rit
    assert np.allclose(ev, rev, rtol=1e-12, atol=0)
    lu.close()
    M.close()


def test_standard_inverse_factors_itself(ctx):
    """without `lu` the driver downloads and factors the blocked matrix; converged (tol 1e-10) it
    reaches the dense smallest eigenvalues to 1e-8 absolute (tests/test_inverse.py's bar)."""
    d = mats()
    M = up(ctx, d["S"])
    ev, _, it = eigmi.standard_inverse(M, 0.0, 1e-10, 1000, 4, 123)
    exact = d["wS"][:4]
    print(f"blocked StandardInverse tol 1e-10: {it} iterations, max |ev - dense| = "
          f"{np.abs(np.sort(ev) - exact).max():.2e}")
    assert np.allclose(exact, [0.38255, 0.67736, 0.68372, 0.70662], rtol=0, atol=1e-5)
    assert np.allclose(np.sort(ev)[:4], exact, rtol=0, atol=1e-8)
    M.close()


# ----------------------------------------------------------------------------------- shift-invert
@pytest.mark.parametrize("sigma", [0.0, 0.3])
def test_shift_invert_standard(ctx, sigma):
    """nev = 4 on blocked S A S; sigma = 0.3 (below the spectrum: the pivot-free LU is valid) goes
    through the blocked diagonal shift of the host copy.  Values within 1e-10 relative of the dense
    ones (tests/test_shift_invert.py's bar), residuals ||A y - lambda y|| <= 1e-9 lambda ||y||."""
    d = mats()
    M = up(ctx, d["S"])
    ev, X, _ = eigmi.shift_invert_solve(M, 4, sigma=sigma)
    exact = d["wS"][:4]
    res = [np.linalg.norm(d["DS"] @ x - lam * x) / (lam * np.linalg.norm(x)) for lam, x in zip(ev, X)]
    print(f"blocked shift-invert sigma {sigma}: max rel |ev - dense| = {np.abs(ev / exact - 1).max():.2e}, "
          f"max residual {max(res):.2e}")
    assert np.allclose(ev, exact, rtol=1e-10, atol=0)
    assert max(res) <= 1e-9
    M.close()


@pytest.mark.parametrize("sigma", [0.0, 0.2])
def test_shift_invert_generalised(ctx, sigma):
    """B block diagonal (3x3 blocks): the four smallest eigenvalues of the pencil against dense
    eigvalsh(L^-1 A L^-T), L = chol(B) (0.26125, 0.45649, 0.46043, 0.47310), within 1e-10 relative;
    B-normalised vectors to 1e-12.  sigma = 0.2 (below the pencil's spectrum) subtracts sigma B
    blockwise in the host copy."""
    d = mats()
    M, MB = up(ctx, d["S"]), up(ctx, d["B"])
    ev, X, _ = eigmi.shift_invert_solve(M, 4, sigma=sigma, B=MB)
    exact = d["wG"][:4]
    bn = np.array([x @ d["DB"] @ x for x in X])
    print(f"blocked generalised shift-invert sigma {sigma}: max rel |ev - dense| = {np.abs(ev / exact - 1).max():.2e}, "
          f"max |x^T B x - 1| = {np.abs(bn - 1).max():.2e}")
    assert np.allclose(exact, [0.26125, 0.45649, 0.46043, 0.47310], rtol=0, atol=1e-5)
    assert np.allclose(ev, exact, rtol=1e-10, atol=0)
    assert np.abs(bn - 1).max() <= 1e-12
    M.close(), MB.close()


def test_shift_invert_block_method_refused(ctx):
    d = mats()
    M = up(ctx, d["S"])
    with pytest.raises(eigmi.EigShapeError) as e:
        eigmi.shift_invert_solve(M, 4, sigma=0.0, method="block")
    assert e.value.code == eigmi.EIG_ERR_BLOCKSIZE
    ev, _, _ = eigmi.shift_invert_solve(M, 4, sigma=0.0, method="single", want_evec=False)
    assert np.allclose(ev, d["wS"][:4], rtol=1e-10, atol=0)
    M.close()


# ---------------------------------------------------------------------------------- scope boundary
def test_still_refused_on_blocks(ctx):
    """out of scope, pinned: the Lanczos solver, StandardLargest, GeneralizedInverse and
    B_orthonormalize_blocked keep EIG_ERR_BLOCKSIZE on a 3x3 matrix"""
    d = mats()
    M, MB = up(ctx, d["S"]), up(ctx, d["B"])
    Q, norm = ctx.zeros(375 * 8), ctx.zeros(1)
    for call in (lambda: eigmi.lanczos_solve(M, 4, 20),
                 lambda: eigmi.standard_largest(M, 0.0, 1e-3, 10, 4),
                 lambda: eigmi.generalized_inverse(M, MB, 0.0, 0.0, 1e-8, 20, 4),
                 lambda: eigmi.b_orthonormalize_mv8(MB, 8, Q, norm)):
        with pytest.raises(eigmi.EigShapeError) as e:
            call()
        assert e.value.code == eigmi.EIG_ERR_BLOCKSIZE
    M.close(), MB.close()
