"""LOBPCG and the shift-invert block Lanczos on a 3x3-blocked pencil with the blocked multigrid as the inner solve
(eig_lobpcg_precond_mg / eig_blanczos_create_si_mg on a Multigrid built on blocks), on the device.

Problem: the scaled q1elast(N) and block-diagonal B of tests/lobpcg_ref.py (scaled_q1elast), N = 12 for LOBPCG
(block 8 and 16, nev 4, tol 1e-8, one V-cycle per iteration, smoother degree 2, ratio 5) and N = 8 for the block
Lanczos.  Bars: eigenvalues within 1e-10 relative of the dense reference, residuals <= 1e-8 theta ||M y||,
Y^T M Y - I <= 1e-12, iterations <= the count of the restatement (lobpcg_ref.Lobpcg with one V-cycle of
mg_blk_ref, re-run here, no literal count) + max(2, 10 %), and <= the count of the device's own run with
Chebyshev-Jacobi degree 4.  Block Lanczos: the 4 smallest within 1e-8 of dense, the bar of
tests/test_multigrid.py::test_shift_invert_smallest_p1_multigrid, with the smallest cycle count at which the
restatement's residual is <= 1e-12."""
import functools
import math

import numpy as np
import pytest
import scipy.linalg as sl

import eigmi
import lobpcg_ref as lr
import mg_blk_ref

pytestmark = pytest.mark.gpu

NEV = 4


@functools.lru_cache(maxsize=None)
def problem(N):
    """-> dict(blocked pair, K, M (scalar expansions), dense eigenvalues, restatement multigrid); built once."""
    S, B = lr.scaled_q1elast(N)
    K, M = lr.expand3(S), lr.expand3(B)
    exact = sl.eigh(K.toarray(), M.toarray(), eigvals_only=True, subset_by_index=(0, NEV - 1))
    return dict(blocked=(S, B), K=K, M=M, exact=exact, mg=mg_blk_ref.Multigrid(K, (N, N, N), 3, 2, 5.0))


@functools.lru_cache(maxsize=None)
def ref_count(N, m):
    p = problem(N)
    s = lr.Lobpcg(p["K"], p["M"], m, precond=lr.vcycles(p["mg"], 1))
    it, conv = s.step(500, NEV, 1e-8)
    assert conv
    return it


def _device(ctx, N):
    return [eigmi.Matrix.from_bcsr(ctx, A.rowptr, A.col, A.val, 3, 3) for A in problem(N)["blocked"]]


@pytest.mark.parametrize("m", [8, 16])
def test_lobpcg_one_vcycle_on_blocks(ctx, m):
    N, tol = 12, 1e-8
    p = problem(N)
    K, M, exact = p["K"], p["M"], p["exact"]
    dK, dM = _device(ctx, N)
    mg = eigmi.Multigrid(dK, (N, N, N), max_cols=m, smooth_degree=2, smooth_ratio=5.0)
    s = eigmi.Lobpcg(dK, dM, block=m)
    s.precond_mg(mg, 1)
    it, conv, t = s.step(500, NEV, tol)
    ev, Y, res = s.ritz(NEV, want_evec=True)
    Y = Y.T
    MY = M @ Y
    G = Y.T @ MY
    g = lr.gershgorin_lmax(K)
    c = eigmi.Lobpcg(dK, dM, block=m)
    c.precond_cheb(4, g / 10.0, g)
    it_cheb, conv_cheb, t_cheb = c.step(500, NEV, tol)
    count = ref_count(N, m)
    print(f"lobpcg q1s-{N} m={m} one V-cycle on blocks: {it} iterations (restatement {count}, Chebyshev-Jacobi degree 4 "
          f"{it_cheb}), max rel |ev - exact| = {np.abs(ev / exact - 1).max():.2e}, max residual / (theta |M y|) = "
          f"{(res / (np.abs(ev) * np.linalg.norm(MY, axis=0))).max():.2e}, |Y^T M Y - I| = "
          f"{np.abs(G - np.eye(NEV)).max():.2e}, device {t.total_ms:.1f} ms (Chebyshev {t_cheb.total_ms:.1f} ms)")
    assert conv and conv_cheb
    assert np.abs(ev / exact - 1).max() <= 1e-10
    assert np.all(res <= tol * np.abs(ev) * np.linalg.norm(MY, axis=0))
    assert np.abs(G - np.eye(NEV)).max() <= 1e-12
    assert it <= count + max(2, math.ceil(0.1 * count))
    assert it <= it_cheb
    for h in (s, c, mg, dK, dM):
        h.close()


def test_block_lanczos_shift_invert_on_blocks(ctx):
    N, m = 8, 8
    p = problem(N)
    K, exact, ref = p["K"], p["exact"], p["mg"]
    # the smallest cycle count at which the restatement solves to 1e-12 (mg_blk_ref.Multigrid.solve's iteration)
    B = np.random.default_rng(2).standard_normal((K.shape[0], m))
    x, r, cycles = np.zeros_like(B), B.copy(), 0
    while np.max(np.linalg.norm(B - K @ x, axis=0) / np.linalg.norm(B, axis=0)) > 1e-12:
        e = ref.vcycle(0, r)
        x, r, cycles = x + e, r - K @ e, cycles + 1
        assert cycles < 200
    dK, dM = _device(ctx, N)
    mg = eigmi.Multigrid(dK, (N, N, N), max_cols=m, smooth_degree=2, smooth_ratio=5.0)
    steps = 16
    bl = eigmi.BlockLanczos(dK, dM, block=m, max_steps=steps, Ks=dK, sigma=0.0, mg=mg, cycles=cycles)
    bl.step(steps)
    ev, _, res = bl.ritz(NEV, eigmi.WHICH_SA)
    print(f"SI block Lanczos q1s-{N} on blocks, {cycles} multigrid cycles per solve: {ev} (dense {exact}), residuals {res}")
    assert np.all(np.diff(ev) >= 0)
    assert np.max(np.abs(ev - exact) / exact) <= 1e-8, (ev, exact)
    for h in (bl, mg, dK, dM):
        h.close()
