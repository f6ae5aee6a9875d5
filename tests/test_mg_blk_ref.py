"""The numpy restatement of the blocked multigrid (tests/mg_blk_ref.py) against its own definition, on the CPU:
its coarse operators are P^T A P and bitwise symmetric, the node-count stopping rule gives the stated levels, a
V-cycle contracts, and its sensitivity to a one-ulp perturbation of B -- the figure that decides the parity bar of
tests/test_gpu_mg_blocked.py -- is printed for every grid that file uses.

GRIDS (shared with the GPU tests; built once, left unchanged): name -> (dims, b, nu, m).  The smoothing ratio
is 5 everywhere."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

import blk_grids
import lobpcg_ref as lr
import mg_blk_ref
import mg_ref

RATIO = 5.0
GRIDS = {
    "66x9x17": ((66, 9, 17), 3, 2, 32),    # fx straddles the 64-x workgroup by two
    "130x12x20": ((130, 12, 20), 3, 2, 8),  # cx = 65 and 32: several restriction blocks per line
    "40x24x10": ((40, 24, 10), 2, 3, 24),
    "17x40x12": ((17, 40, 12), 4, 1, 8),    # y is the long direction
    "q1s-12": ((12, 12, 12), 3, 2, 32),
}


@functools.lru_cache(maxsize=None)
def grid_case(name):
    """-> (blocked oracle.CSR, scipy CSR of its scalar expansion, restatement Multigrid)."""
    dims, b, nu, _ = GRIDS[name]
    if name == "q1s-12":
        A = lr.scaled_q1elast(12)[0]
        S = blk_grids.expand(A)
    else:
        A, S = blk_grids.blk_matrix(dims, b, seed=sum(dims))
    return A, S, mg_blk_ref.Multigrid(S, dims, b, nu, RATIO)


def rhs(n, m, seed=5):
    return np.random.default_rng(seed).standard_normal((n, m))


@functools.lru_cache(maxsize=None)
def sensitivity(name, cycles):
    """max |S(B') - S(B)| / max |S(B)| for B' = B with every entry moved by one ulp (random direction), 8 columns."""
    _, S, mg = grid_case(name)
    B = rhs(S.shape[0], 8)
    sign = np.where(np.random.default_rng(6).random(B.shape) < 0.5, -1.0, 1.0)
    B1 = np.nextafter(B, sign * np.inf)
    X, X1 = mg.solve(B, cycles), mg.solve(B1, cycles)
    return float(np.abs(X1 - X).max() / np.abs(X).max())


def test_level_dims_and_rows():
    assert mg_blk_ref.level_dims((66, 9, 17)) == [(66, 9, 17), (33, 4, 8), (16, 2, 4)]
    assert [3 * x * y * z for x, y, z in mg_blk_ref.level_dims((66, 9, 17))] == [30294, 3168, 384]
    assert mg_blk_ref.level_dims((17, 40, 12)) == [(17, 40, 12), (8, 20, 6), (4, 10, 3), (2, 5, 1)]
    mg = grid_case("66x9x17")[2]
    assert [L["dims"] for L in mg.levels] == mg_blk_ref.level_dims((66, 9, 17))
    assert [L["A"].shape[0] for L in mg.levels] == [30294, 3168, 384]
    assert mg.info()["levels"] == 3 and mg.info()["coarse_rows"] == 384


@pytest.mark.parametrize("name", ["66x9x17", "17x40x12"])
def test_coarse_operators_are_galerkin_and_symmetric(name):
    dims, b, _, _ = GRIDS[name]
    mg = grid_case(name)[2]
    for F, C in zip(mg.levels[:-1], mg.levels[1:]):
        Pn, cd = mg_ref.prolongation(F["dims"])
        assert cd == C["dims"]
        P = sp.kron(Pn, sp.identity(b)).tocsr()
        assert (abs(P - F["P"])).max() == 0.0
        G = (P.T @ F["A"] @ P).tocsr()
        assert abs(G - C["A"]).max() <= 1e-14 * abs(G).max()
        assert abs(C["A"] - C["A"].T).max() == 0.0
        assert np.diff(C["A"].tobsr((b, b)).indptr).max() <= 27


def test_block_inverse_and_bound():
    dims, b, _, _ = GRIDS["17x40x12"]
    L = grid_case("17x40x12")[2].levels[1]
    A, Dinv = L["A"], L["Dinv"]
    D = sp.block_diag(list(mg_blk_ref.diag_blocks(A, b))).tocsr()
    assert abs(Dinv @ D - sp.identity(A.shape[0])).max() <= 1e-13
    assert abs(Dinv - Dinv.T).max() == 0.0
    lam = np.linalg.eigvals((Dinv @ A).toarray()).real.max()
    print(f"17x40x12 level 1: block Gershgorin bound {L['lmax']:.4f}, dense lambda_max {lam:.4f}")
    assert L["lmax"] >= lam


def test_restatement_contracts_on_q1s12():
    """The residual contraction per V-cycle (nu = 2, ratio 5) on the scaled q1elast(12): printed, asserted only
    finite and < 1 (measured 0.44 with the prototype)."""
    _, S, mg = grid_case("q1s-12")
    B = rhs(S.shape[0], 8)
    r0 = np.linalg.norm(B, axis=0)
    r = [np.linalg.norm(B - S @ mg.solve(B, c), axis=0) / r0 for c in (1, 2, 3, 4)]
    fac = [float((r[i + 1] / r[i]).max()) for i in range(3)]
    print(f"q1s-12 residual after 1..4 cycles {[float(x.max()) for x in r]}, contraction per cycle {fac}")
    assert np.all(np.isfinite(fac)) and max(fac) < 1.0 and float(r[0].max()) < 1.0


@pytest.mark.parametrize("name", sorted(GRIDS))
def test_print_sensitivity(name):
    s1, s3 = sensitivity(name, 1), sensitivity(name, 3)
    print(f"mg_blk_ref sensitivity to one ulp of B on {name}: {s1:.2e} (1 cycle), {s3:.2e} (3 cycles)")
    assert np.isfinite(s1) and np.isfinite(s3)
