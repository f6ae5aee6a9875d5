"""Block Lanczos for K x = lambda M x and the Chebyshev-Jacobi mass solve on blocked pencils
(BCRSMatrix<FieldMatrix<double,b,b>>, b = 2, 3, 4, one rank): eig_blanczos_* and eig_mass_solve_mv8
with n = nb_rows * b scalar rows, the products on k_spmm_blk_mv8, the Chebyshev step on
k_spmm_blk_mv8_cheb (k_mv8.hip) with point Jacobi on the scalar diagonal of the diagonal blocks
(k_diag_inv_blk).

References: the numpy restatements the 1x1 tests use (oracle.cheb_solve, oracle.block_lanczos_gen) on
the SCALAR EXPANSION of the blocked matrices (expand, tests/test_gpu_blocked_spmm.py: the blocked
product is bitwise the 1x1 product on it), and dense scipy.linalg.eigh / numpy.linalg.solve.  The bars
are those of tests/test_block_lanczos.py: mass solve 1e-13 relative (max norm) to the restatement and
1e-12 to the dense solve at degree 36, eigenvalues of T 1e-9 relative to the restatement's, converged
Ritz values 1e-9 (largest end) / 1e-8 (shift-invert, smallest end) relative to dense.

Pencils: spd_pencil(b) on 130 block rows (3 slices, the last with 2 rows; 1..10 blocks per row), K
strictly diagonally dominant with normal off-diagonal blocks, M = scaled tridiag(0.5, 2, 0.5) diagonal
blocks plus 0.03 * normal off-diagonal blocks; both bitwise symmetric.  The Chebyshev bounds passed are
0.95 lambda_min and 1.05 lambda_max of D^-1/2 . D^-1/2 (dense eigvalsh).  The CPU test below pins the
inputs' conditions -- with this file's construction (the draw order is this file's own)
    spec(D^-1 M) = [0.69, 1.32] / [0.57, 1.42] / [0.53, 1.47],
    spec(D^-1 K) = [0.36, 1.63] / [0.45, 1.63] / [0.36, 1.69]      for b = 2 / 3 / 4
-- and that the restatements themselves reach the dense answers to <= 1e-12, so the bars above hold
with orders of margin on the reference alone.  The elasticity cases take M = D + 0.3 (A - D) from
oracle.q1elast (D the scalar diagonal): q1elast(5) has a ragged last slice (61 rows), q1elast(16) has
64 slices, from which the kernels walk the XCD shares.

Every GPU test that builds a blocked BlockLanczos or calls mass_solve_mv8 on blocks fails with
EIG_ERR_BLOCKSIZE without the blocked path."""
import numpy as np
import pytest

import eigmi
import oracle
from test_block_lanczos import _cheb_degree
from test_gpu_blocked_spmm import expand

_cache = {}


def spd_pencil(b, nb=130, seed=2):
    """(K, M) blocked oracle.CSR on one pattern: the diagonal block plus 0..4 partners among the next 24
    block rows, mirrored."""
    prng = np.random.default_rng(seed + 100)
    part = [set() for _ in range(nb)]
    for I in range(nb):
        k = int(prng.integers(0, 5))
        cand = np.arange(I + 1, min(nb, I + 25))
        for J in (prng.choice(cand, min(k, cand.size), replace=False) if k and cand.size else []):
            part[I].add(int(J))
            part[int(J)].add(I)
    cols = [sorted(part[I] | {I}) for I in range(nb)]
    rowptr = np.zeros(nb + 1, np.int64)
    rowptr[1:] = np.cumsum([len(c) for c in cols])
    col = np.concatenate(cols).astype(np.int32)
    pos = {(I, J): rowptr[I] + k for I in range(nb) for k, J in enumerate(cols[I])}
    rng = np.random.default_rng(seed)
    kv, mv = np.zeros((col.size, b, b)), np.zeros((col.size, b, b))
    for I in range(nb):
        for J in cols[I]:
            if J > I:
                G = rng.standard_normal((b, b))
                kv[pos[I, J]], kv[pos[J, I]] = G, G.T.copy()
                H = 0.03 * rng.standard_normal((b, b))
                mv[pos[I, J]], mv[pos[J, I]] = H, H.T.copy()
    T = 2.0 * np.eye(b) + 0.5 * (np.eye(b, k=1) + np.eye(b, k=-1))
    for I in range(nb):
        G = rng.standard_normal((b, b))
        kv[pos[I, I]] = G + G.T
        rs = np.abs(kv[rowptr[I]:rowptr[I + 1]]).sum(axis=(0, 2))  # abs sum of each whole scalar row
        kv[pos[I, I]] += np.diag(rs + 1.0 + 0.37 * np.arange(b))
        mv[pos[I, I]] = (1.0 + 0.1 * (I % 3)) * T
    return (oracle.CSR(nb, rowptr, col, kv.reshape(-1), b, b), oracle.CSR(nb, rowptr, col, mv.reshape(-1), b, b))


def damped(A, theta=0.3):
    """D + theta (A - D), D the scalar diagonal of the blocked matrix A: same pattern, symmetric with A."""
    b = A.br
    v = theta * A.val.reshape(-1, b, b)
    I = np.repeat(np.arange(A.nrows), np.diff(A.rowptr))
    dg = np.nonzero(A.col == I)[0]
    r = np.arange(b)
    v[dg[:, None], r, r] = A.val.reshape(-1, b, b)[dg[:, None], r, r]
    return oracle.CSR(A.nrows, A.rowptr, A.col, v.reshape(-1), b, b)


def jacobi_spectrum(D):
    d = 1.0 / np.sqrt(np.diag(D))
    w = np.linalg.eigvalsh(D * d[:, None] * d[None, :])
    return w[0], w[-1]


def pencil(b):
    """the blocked pair, its expansions (oracle.CSR, scipy and dense), the Jacobi-scaled spectra and the
    dense eigenvalues; built once per session and left unchanged"""
    if b not in _cache:
        import scipy.linalg as sl
        K, M = spd_pencil(b)
        EK, EM = expand(K.rowptr, K.col, K.val, b), expand(M.rowptr, M.col, M.val, b)
        SK, SM = EK.to_scipy(), EM.to_scipy()
        DK, DM = SK.toarray(), SM.toarray()
        _cache[b] = dict(K=K, M=M, EK=EK, EM=EM, SK=SK, SM=SM, DK=DK, DM=DM, specK=jacobi_spectrum(DK),
                         specM=jacobi_spectrum(DM), exact=sl.eigh(DK, DM, eigvals_only=True))
    return _cache[b]


def bounds(spec):
    return 0.95 * spec[0], 1.05 * spec[1]


def rhs(n, m, seed):
    return np.random.default_rng(seed).standard_normal((n, m))


def up(ctx, A):
    return eigmi.Matrix.from_bcsr(ctx, A.rowptr, A.col, A.val, A.br, A.bc)


def relmax(X, R):
    return np.max(np.abs(X - R)) / np.max(np.abs(R))


# ------------------------------------------------------------------------------------ CPU: the inputs
def test_pencils_and_restatements_cpu():
    """the inputs' conditions, wherever the suite runs: pattern, bitwise symmetry, the Jacobi-scaled
    spectra (two digits), and the restatements against dense solve / eigh to <= 1e-12"""
    table = {2: ((0.69, 1.32), (0.36, 1.63)), 3: ((0.57, 1.42), (0.45, 1.63)), 4: ((0.53, 1.47), (0.36, 1.69))}
    for b in (2, 3, 4):
        d = pencil(b)
        cnt = np.diff(d["K"].rowptr)
        assert d["K"].nrows == 130 and cnt.min() == 1 and cnt.max() == 10
        assert np.array_equal(d["DK"], d["DK"].T) and np.array_equal(d["DM"], d["DM"].T)
        assert np.allclose(d["specM"], table[b][0], rtol=0, atol=5e-3), d["specM"]
        assert np.allclose(d["specK"], table[b][1], rtol=0, atol=5e-3), d["specK"]
        lo, hi = bounds(d["specM"])
        n = d["K"].n
        for m in (8, 24, 32):
            B = rhs(n, m, 10 * b + m)
            e = relmax(oracle.cheb_solve(d["SM"], B, 36, lo, hi), np.linalg.solve(d["DM"], B))
            assert e <= 1e-12, (b, m, e)
        V0 = oracle.mv_to_cols(oracle.random_mv8(n, 8, 123), n, 8)
        T, _ = oracle.block_lanczos_gen(d["SK"], d["SM"], V0, 24, 36, lo, hi)
        top = d["exact"][::-1][:4]
        e = np.max(np.abs(np.linalg.eigvalsh(T)[::-1][:4] - top) / top)
        print(f"b = {b}: restatement's 4 largest Ritz values vs dense eigh: {e:.2e}")
        assert e <= 1e-12, (b, e)


# ------------------------------------------------------------------------------------- mass solve
def device_mass_solve(ctx, A, B, degree, lo, hi):
    n, m = B.shape
    M = up(ctx, A)
    dB, dX = ctx.array(oracle.cols_to_mv(B)), ctx.zeros(n * m)
    eigmi.mass_solve_mv8(M, m, degree, dB, dX, lo, hi)
    X = oracle.mv_to_cols(dX.get(), n, m)
    dB.free(), dX.free()
    M.close()
    return X


@pytest.mark.gpu
@pytest.mark.parametrize("m", [8, 24, 40])  # 1; 3 (a partly filled group of 4, two groups of 2); 5 column blocks
@pytest.mark.parametrize("b", [2, 3, 4])
def test_mass_solve(ctx, b, m):
    d = pencil(b)
    n = d["M"].n
    lo, hi = bounds(d["specM"])
    B = rhs(n, m, 10 * b + m)
    X = device_mass_solve(ctx, d["M"], B, 36, lo, hi)
    Xo = oracle.cheb_solve(d["SM"], B, 36, lo, hi)
    Xe = np.linalg.solve(d["DM"], B)
    X1 = device_mass_solve(ctx, d["EM"], B, 36, lo, hi)  # the expansion as a 1x1 matrix
    print(f"b = {b}, m = {m}: vs restatement {relmax(X, Xo):.2e}, vs dense {relmax(X, Xe):.2e}, "
          f"vs the 1x1 device solve {relmax(X, X1):.2e} (bitwise: {np.array_equal(X, X1)})")
    assert relmax(X, Xo) <= 1e-13
    assert relmax(X, Xe) <= 1e-12
    assert relmax(X, X1) <= 1e-13


@pytest.mark.gpu
def test_mass_solve_ragged_elasticity_slice(ctx):
    """M = D + 0.3 (A - D) of q1elast(5): 125 block rows, the last slice with 61; spec(D^-1 M) =
    0.7 + 0.3 spec(D^-1 A) lies in the default bounds [0.5, 2.5]"""
    A = oracle.q1elast(5)
    Mh = damped(A)
    E = expand(Mh.rowptr, Mh.col, Mh.val, 3)
    DM = E.to_scipy().toarray()
    assert np.array_equal(DM, DM.T)
    lo, hi = jacobi_spectrum(DM)
    assert 0.5 < lo and hi < 2.5
    B = rhs(Mh.n, 32, 5)
    X = device_mass_solve(ctx, Mh, B, 36, 0.5, 2.5)
    Xo = oracle.cheb_solve(E.to_scipy(), B, 36)
    Xe = np.linalg.solve(DM, B)
    print(f"q1elast(5) mass solve: vs restatement {relmax(X, Xo):.2e}, vs dense {relmax(X, Xe):.2e}")
    assert relmax(X, Xo) <= 1e-13
    assert relmax(X, Xe) <= 1e-12


@pytest.mark.gpu
def test_mass_solve_xcd_share_schedule(ctx):
    """q1elast(16): 4,096 block rows = 64 slices, from which the blocked kernels walk the XCD shares;
    8 Chebyshev steps on [0.668, 1.531] against the restatement (no convergence claim at degree 8)"""
    Mh = damped(oracle.q1elast(16))
    E = expand(Mh.rowptr, Mh.col, Mh.val, 3)
    assert Mh.nrows == 4096 and Mh.n == 12288
    B = rhs(Mh.n, 32, 16)
    X = device_mass_solve(ctx, Mh, B, 8, 0.668, 1.531)
    Xo = oracle.cheb_solve(E.to_scipy(), B, 8, 0.668, 1.531)
    print(f"q1elast(16) 8 Chebyshev steps: vs restatement {relmax(X, Xo):.2e}")
    assert relmax(X, Xo) <= 1e-13


# ----------------------------------------------------------------------------------- block Lanczos
def t_error(bl, d, n, block, steps, lo, hi):
    V0 = oracle.mv_to_cols(oracle.random_mv8(n, block, 123), n, block)
    Tref, _ = oracle.block_lanczos_gen(d["SK"], d["SM"], V0, steps, 36, lo, hi)
    th, thr = np.linalg.eigvalsh(bl.tmatrix()), np.linalg.eigvalsh(Tref)
    return np.max(np.abs(th - thr) / np.abs(thr))


@pytest.mark.gpu
@pytest.mark.parametrize("b", [2, 3, 4])
def test_block_lanczos_largest(ctx, b):
    d = pencil(b)
    n, block, steps = d["K"].n, 8, 24
    lo, hi = bounds(d["specM"])
    K, M = up(ctx, d["K"]), up(ctx, d["M"])
    bl = eigmi.BlockLanczos(K, M, block=block, max_steps=steps, degree=36, lmin=lo, lmax=hi, seed=123)
    t = bl.step(steps)
    assert t.steps == steps and t.cheb_launches == steps * 35  # one blocked launch per Chebyshev step
    et = t_error(bl, d, n, block, steps, lo, hi)
    ev, Y, res = bl.ritz(4, eigmi.WHICH_LA, want_evec=True)
    top = d["exact"][::-1][:4]
    ee = np.max(np.abs(ev - top) / top)
    G = Y @ (d["DM"] @ Y.T)
    # the host's residuals ||K y - theta M y|| on the returned vectors.  These Ritz pairs have converged,
    # so the residuals are rounding-sized (1e-13 .. 1e-9, against ||K y|| ~ 10): a product with another
    # summation order (a dense matmul) moves them by ~3e-16 absolute = 1e-3 relative.  The products are
    # therefore the oracle's on the expansions -- the order of the device's blocked product, bitwise
    Ymv = oracle.cols_to_mv(np.ascontiguousarray(np.hstack([Y.T, np.zeros((n, 4))])))
    KY = oracle.mv_to_cols(oracle.spmm_mv8(d["EK"], Ymv, 8), n, 8)[:, :4]
    MY = oracle.mv_to_cols(oracle.spmm_mv8(d["EM"], Ymv, 8), n, 8)[:, :4]
    host_res = np.linalg.norm(KY - MY * ev[None, :], axis=0)
    print(f"b = {b}: eig(T) vs restatement {et:.2e}, 4 largest vs dense {ee:.2e}, "
          f"M-orthonormality {np.max(np.abs(G - np.eye(4))):.2e}, residuals {res} vs the host's: "
          f"{np.max(np.abs(res / host_res - 1)):.2e}")
    assert et <= 1e-9
    assert ee <= 1e-9
    assert np.max(np.abs(G - np.eye(4))) <= 1e-9
    assert np.allclose(res, host_res, rtol=1e-6, atol=0)
    bl.close()
    K.close(), M.close()


@pytest.mark.gpu
def test_block_lanczos_block32(ctx):
    """block 32, 6 steps on 3x3 blocks: the panels' widest case, T against the restatement"""
    d = pencil(3)
    n, block, steps = d["K"].n, 32, 6
    lo, hi = bounds(d["specM"])
    K, M = up(ctx, d["K"]), up(ctx, d["M"])
    bl = eigmi.BlockLanczos(K, M, block=block, max_steps=steps, degree=36, lmin=lo, lmax=hi, seed=123)
    bl.step(steps)
    et = t_error(bl, d, n, block, steps, lo, hi)
    print(f"b = 3, block 32: eig(T) vs restatement {et:.2e}")
    assert et <= 1e-9
    bl.close()
    K.close(), M.close()


@pytest.mark.gpu
def test_shift_invert_smallest(ctx):
    """(K - sigma M)^-1 M at sigma = 0 on 3x3 blocks, Ks = K solved by Chebyshev-Jacobi on K (degree
    for 1e-13): the 4 smallest eigenvalues, ascending, within 1e-8 relative of dense eigh"""
    d = pencil(3)
    lo, hi = bounds(d["specK"])
    deg = _cheb_degree(lo, hi, 1e-13)
    K, M = up(ctx, d["K"]), up(ctx, d["M"])
    bl = eigmi.BlockLanczos(K, M, block=8, max_steps=12, degree=deg, lmin=lo, lmax=hi, seed=123, Ks=K, sigma=0.0)
    bl.step(12)
    ev, _, _ = bl.ritz(4, eigmi.WHICH_SA)
    e = np.max(np.abs(ev - d["exact"][:4]) / d["exact"][:4])
    print(f"shift-invert on 3x3 blocks, degree {deg}: 4 smallest vs dense {e:.2e}")
    assert np.all(np.diff(ev) >= 0)
    assert e <= 1e-8
    bl.close()
    K.close(), M.close()


# ---------------------------------------------------------------------------------------- refusals
@pytest.mark.gpu
def test_refusals(ctx):
    nb = 130
    rowptr, col = np.arange(nb + 1, dtype=np.int64), np.arange(nb, dtype=np.int32)
    K23 = eigmi.Matrix.from_bcsr(ctx, rowptr, col, np.ones(nb * 6), 2, 3, ncols_blocks=nb)
    with pytest.raises(eigmi.EigShapeError) as e:  # rectangular blocks
        eigmi.BlockLanczos(K23, K23, block=8, max_steps=2)
    assert e.value.code == eigmi.EIG_ERR_BLOCKSIZE
    K23.close()
    d = pencil(3)
    K, M, M1 = up(ctx, d["K"]), up(ctx, d["M"]), up(ctx, d["EM"])
    with pytest.raises(eigmi.EigShapeError) as e:  # 3x3 K with the 1x1 M of the same n
        eigmi.BlockLanczos(K, M1, block=8, max_steps=2)
    assert e.value.code == eigmi.EIG_ERR_BLOCKSIZE
    B = ctx.zeros(d["M"].n * 8)
    with pytest.raises(eigmi.EigError) as e:  # X aliasing B: B is read by every step
        eigmi.mass_solve_mv8(M, 8, 4, B, B)
    assert e.value.code == eigmi.EIG_ERR_ARG
    B.free()
    K.close(), M.close(), M1.close()
