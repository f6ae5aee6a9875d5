"""The geometric multigrid on square blocks b = 2..4 (csrc/mg.cpp, mg_setup.cpp, k_mg.hip, k_mv8.hip) and the
residual entry point eig_resid_mv8, on the device.

eig_resid_mv8 on blocks is the residual epilogue on k_spmm_blk_mv8's row sums: bitwise B minus the oracle product on
the matrix's scalar expansion (tests/test_gpu_blocked_spmm.py expand), run to run bitwise equal; on a 1x1 matrix
within (row length + 1) 2.2e-16 (|A| |X| + |B|) (another summation order per kernel).

Solve parity against tests/mg_blk_ref.py on the grids of tests/test_mg_blk_ref.py GRIDS, 1 and 3 cycles.  Bar:
1e-12 max|R|, the bar of tests/test_multigrid.py, which holds while the restatement's own sensitivity to a one-ulp
perturbation of B stays <= 1e-14 (asserted here; measured 4e-16 .. 7e-16 on every grid, test_mg_blk_ref.py prints
it); a grid above that would take 100 x its measured sensitivity, the rule of tests/test_gpu_lobpcg.py."""
import numpy as np
import pytest

import blk_grids
import box_grids
import eigmi
import oracle
from test_gpu_blocked_spmm import expand
from test_mg_blk_ref import GRIDS, RATIO, grid_case, rhs, sensitivity

pytestmark = pytest.mark.gpu

_cache = {}


def _mv(ctx, X):
    return ctx.array(oracle.cols_to_mv(np.ascontiguousarray(X)))


def _cols(d, n, m):
    return oracle.mv_to_cols(d.get(), n, m)


def _blocked(ctx, A):
    return eigmi.Matrix.from_bcsr(ctx, A.rowptr, A.col, A.val, A.br, A.bc)


def resid_case(name):
    """(blocked oracle.CSR, its scalar expansion as oracle.CSR), built once and left unchanged."""
    if name not in _cache:
        A = {"q1elast5": lambda: oracle.q1elast(5), "blk2": lambda: blk_grids.blk_matrix((17, 9, 5), 2, 3)[0],
             "blk4": lambda: blk_grids.blk_matrix((17, 9, 5), 4, 4)[0]}[name]()
        _cache[name] = (A, expand(A.rowptr, A.col, A.val, A.br))
    return _cache[name]


# ------------------------------------------------------------------------------------- eig_resid_mv8
@pytest.mark.parametrize("name", ["q1elast5", "blk2", "blk4"])
@pytest.mark.parametrize("m", [8, 24, 32])  # 24: a partial column-block group (4 per workgroup for b <= 3, 2 for b = 4)
def test_resid_blocked_bitwise(ctx, name, m):
    A, E = resid_case(name)
    n = A.n
    Xh, Bh = oracle.random_mv8(n, m, 7), oracle.random_mv8(n, m, 8)
    want = Bh - oracle.spmm_mv8(E, Xh, m)
    M = _blocked(ctx, A)
    assert M.kernel("spmm8") == "k_spmm_blk_mv8"
    dX, dB = ctx.array(Xh), ctx.array(Bh)
    out = []
    for _ in range(2):
        dR = ctx.zeros(n * m)
        eigmi.resid_mv8(M, m, dX, dB, dR)
        out.append(dR.get())
        dR.free()
    assert np.array_equal(out[0], want)
    assert np.array_equal(out[0], out[1])
    eigmi.resid_mv8(M, m, dX, dB, dB)  # R may be B
    assert np.array_equal(dB.get(), want)
    assert np.array_equal(dX.get(), Xh)
    M.close()


def test_resid_scalar_within_rounding(ctx):
    dims, m = (17, 9, 5), 16
    A = box_grids.box_matrix(dims, "full27", "edge", 2)
    S = box_grids.to_scipy(A)
    n = A.n
    rng = np.random.default_rng(9)
    X, B = rng.standard_normal((n, m)), rng.standard_normal((n, m))
    M = eigmi.Matrix.from_bcsr(ctx, A.rowptr, A.col, A.val)
    dX, dB, dR = _mv(ctx, X), _mv(ctx, B), ctx.zeros(n * m)
    eigmi.resid_mv8(M, m, dX, dB, dR)
    R = _cols(dR, n, m)
    bar = (np.diff(A.rowptr).max() + 1) * 2.2e-16 * (abs(S) @ np.abs(X) + np.abs(B))
    err = np.abs(R - (B - S @ X))
    print(f"eig_resid_mv8 1x1 {dims}: max error / bar = {(err / bar).max():.3f}")
    assert np.all(err <= bar)
    M.close()


def test_resid_refuses_aliased_x(ctx):
    A, _ = resid_case("blk2")
    M = _blocked(ctx, A)
    dX, dB = ctx.array(oracle.random_mv8(A.n, 8, 1)), ctx.array(oracle.random_mv8(A.n, 8, 2))
    with pytest.raises(eigmi.EigError) as e:
        eigmi.resid_mv8(M, 8, dX, dB, dX)
    assert e.value.code == eigmi.EIG_ERR_ARG
    M.close()


@pytest.mark.parametrize("name", ["q1elast5", "blk4"])
def test_resid_reads_only_stored_blocks(ctx, name):
    """+Inf in X at a block column that the witness block row does not store leaves the witness's rows of R finite
    and bitwise what they were (the idea of tests/test_gpu_poison.py): a product that gathered a padding entry or
    a neighbour's column would turn them into Inf or NaN."""
    A, E = resid_case(name)
    b, n, m = A.br, A.n, 24
    Xh, Bh = oracle.random_mv8(n, m, 11), oracle.random_mv8(n, m, 12)
    want = oracle.mv_to_cols(Bh - oracle.spmm_mv8(E, Xh, m), n, m)
    M = _blocked(ctx, A)
    dB = ctx.array(Bh)
    for I in (0, A.nrows // 2, A.nrows - 1):
        stored = set(A.col[A.rowptr[I]:A.rowptr[I + 1]].tolist())
        J = next(j for j in range(A.nrows - 1, -1, -1) if j not in stored)
        X = oracle.mv_to_cols(Xh, n, m).copy()
        X[J * b:(J + 1) * b] = np.inf
        dX, dR = _mv(ctx, X), ctx.zeros(n * m)
        eigmi.resid_mv8(M, m, dX, dB, dR)
        R = _cols(dR, n, m)
        assert np.all(np.isfinite(R[I * b:(I + 1) * b])), (I, J)
        assert np.array_equal(R[I * b:(I + 1) * b], want[I * b:(I + 1) * b])
        dX.free(), dR.free()
    M.close()


# ------------------------------------------------------------------------------------- solve
@pytest.mark.parametrize("name", sorted(GRIDS))
def test_solve_matches_restatement(ctx, name):
    dims, b, nu, m = GRIDS[name]
    A, S, ref = grid_case(name)
    n = S.shape[0]
    dK = _blocked(ctx, A)
    mg = eigmi.Multigrid(dK, dims, max_cols=m, smooth_degree=nu, smooth_ratio=RATIO)
    info, want = mg.info(), ref.info()
    print(f"multigrid {name} b={b}: device {info}, restatement {want}")
    assert info["levels"] == want["levels"] and info["coarse_rows"] == want["coarse_rows"]
    assert info["coarse_degree"] == want["coarse_degree"]
    assert abs(info["lmax_fine"] - want["lmax_fine"]) <= 1e-13 * want["lmax_fine"]
    B = rhs(n, m)
    dB, dX = _mv(ctx, B), ctx.zeros(n * m)
    for cycles in (1, 3):
        sens = sensitivity(name, cycles)
        assert sens <= 1e-14, sens  # the condition under which the 1e-12 bar holds
        mg.solve(m, dB, dX, cycles)
        X = _cols(dX, n, m)
        R = ref.solve(B, cycles)
        dev = np.abs(X - R).max() / np.abs(R).max()
        print(f"multigrid {name} b={b} nu={nu} m={m} cycles={cycles}: |X - R|.max() / |R|.max() = {dev:.2e} "
              f"(restatement sensitivity {sens:.2e})")
        assert np.abs(X - R).max() <= 1e-12 * np.abs(R).max(), (cycles, dev)
    mg.close()
    dK.close()


def test_solve_is_symmetric(ctx):
    """Restriction is exactly P^T, D^-1 is stored bitwise symmetric and the post-smoother is the adjoint of the
    pre-smoother, so B^T S_6 B is symmetric to rounding."""
    name, m = "66x9x17", 8
    dims, b, nu, _ = GRIDS[name]
    A, S, _ = grid_case(name)
    n = S.shape[0]
    dK = _blocked(ctx, A)
    mg = eigmi.Multigrid(dK, dims, max_cols=8, smooth_degree=nu, smooth_ratio=RATIO)
    B = rhs(n, m)
    dB, dX = _mv(ctx, B), ctx.zeros(n * m)
    mg.solve(m, dB, dX, 6)
    G = B.T @ _cols(dX, n, m)
    assert np.all(np.isfinite(G))
    assert np.abs(G - G.T).max() <= 1e-13 * np.abs(G).max(), np.abs(G - G.T).max() / np.abs(G).max()
    mg.close()
    dK.close()


def test_reported_residual(ctx):
    name, m = "40x24x10", 8
    dims, b, nu, _ = GRIDS[name]
    A, S, _ = grid_case(name)
    n = S.shape[0]
    dK = _blocked(ctx, A)
    mg = eigmi.Multigrid(dK, dims, max_cols=8, smooth_degree=nu, smooth_ratio=RATIO)
    B = rhs(n, m)
    dB, dX = _mv(ctx, B), ctx.zeros(n * m)
    r = mg.solve(m, dB, dX, 2, resid=True)
    X = _cols(dX, n, m)
    host = (np.linalg.norm(B - S @ X, axis=0) / np.linalg.norm(B, axis=0)).max()
    print(f"multigrid {name}: reported residual after 2 cycles {r:.6e}, host {host:.6e}")
    assert 0 < r < 1 and abs(r - host) <= 1e-9 * host
    mg.close()
    dK.close()


def test_refusals(ctx):
    dims = (5, 4, 3)
    A, _ = blk_grids.blk_matrix(dims, 2, 1)
    dA = _blocked(ctx, A)
    with pytest.raises(eigmi.EigShapeError) as e:  # nx ny nz != block rows
        eigmi.Multigrid(dA, (5, 4, 4))
    assert e.value.code == eigmi.EIG_ERR_SHAPE
    with pytest.raises(eigmi.EigShapeError) as e:  # the scalar extents are not the node extents
        eigmi.Multigrid(dA, (10, 4, 3))
    assert e.value.code == eigmi.EIG_ERR_SHAPE
    # rectangular blocks: 60 x 60 blocks of 2 x 3
    n = 60
    R = eigmi.Matrix.from_bcsr(ctx, np.arange(n + 1, dtype=np.int64), np.arange(n, dtype=np.int32), np.ones(n * 6), 2, 3)
    with pytest.raises(eigmi.EigShapeError) as e:
        eigmi.Multigrid(R, dims)
    assert e.value.code == eigmi.EIG_ERR_BLOCKSIZE
    # nodes two grid steps apart
    T = blk_grids.two_step_matrix((9, 3, 3), 3)
    dT = _blocked(ctx, T)
    with pytest.raises(eigmi.EigError) as e:
        eigmi.Multigrid(dT, (9, 3, 3))
    assert e.value.code == eigmi.EIG_ERR_ARG and "one grid step" in str(e.value)
    # a diagonal block that is not positive definite
    val = A.val.copy().reshape(-1, 2, 2)
    k = int(A.rowptr[7] + np.searchsorted(A.col[A.rowptr[7]:A.rowptr[8]], 7))
    val[k] = [[1.0, 2.0], [2.0, 1.0]]
    dN = eigmi.Matrix.from_bcsr(ctx, A.rowptr, A.col, val.reshape(-1), 2, 2)
    with pytest.raises(eigmi.EigError) as e:
        eigmi.Multigrid(dN, dims)
    assert e.value.code == eigmi.EIG_ERR_BREAKDOWN
    for h in (dA, R, dT, dN):
        h.close()
