"""LOBPCG on the device (csrc/lobpcg.cpp, k_lobpcg.hip; include/eigmi.h eig_lobpcg_*) against the
numpy restatement tests/lobpcg_ref.py and dense / ARPACK / analytic spectra.

Kernel bars: k_lobpcg_resid's R is bitwise numpy's KX - MX * theta and its sums hold 1e-13 relative
(the bar of dot_diag); k_lobpcg_update holds 1e-13 (|S| @ |C|).max() (the bar of test_panel_update).

Fixed-iteration parity: after 3, 6 and 10 forced iterations from the same uploaded start block the m
Ritz values agree with the restatement to 100 x its measured one-ulp sensitivity
(tests/test_lobpcg_ref.py SENSITIVITY: 3e-14 / 2e-13 / 4e-12 for Jacobi m = 8, one V-cycle m = 8 and
m = 32, so the bars are 3e-12 / 2e-11 / 4e-10): 100 because the device sums every Gram in another order.
The restatement's preconditioner is tests/mg_ref.py, tied to the device's multigrid to 1e-12 by
test_multigrid.py::test_mg_solve_matches_restatement.

Converged answers (nev = 4, tol 1e-8): eigenvalues within 1e-10 relative, returned residuals <= 1e-8
theta ||M y|| and equal to host-computed ones to 1e-6 relative, Y^T M Y - I <= 1e-12, iterations <=
the restatement's count + max(2, 10 %)."""
import functools
import math
import threading

import numpy as np
import pytest
import scipy.sparse as sp

import eigmi
import lobpcg_ref as lr
import oracle
from test_lobpcg_ref import NEV, PARITY_CASES, SENSITIVITY, dense_reference, redo_case, start_block, which_of

pytestmark = pytest.mark.gpu


def _upload(ctx, A):
    A = A.tocsr()
    A.sort_indices()
    return eigmi.Matrix.from_bcsr(ctx, A.indptr.astype(np.int64), A.indices.astype(np.int32), A.data)


def _mv(ctx, X):
    return ctx.array(oracle.cols_to_mv(np.ascontiguousarray(X)))


def _cols(d, n, m):
    return oracle.mv_to_cols(d.get(), n, m)


# ------------------------------------------------------------------------------------- kernels
@pytest.mark.parametrize("n", [61, 130, 4099])
@pytest.mark.parametrize("m", [8, 32])
def test_resid_kernel(ctx, n, m):
    rng = np.random.default_rng(n + m)
    KX, MX, th = rng.standard_normal((n, m)), rng.standard_normal((n, m)), rng.standard_normal(m)
    dK, dM, dT = _mv(ctx, KX), _mv(ctx, MX), ctx.array(th)
    out = []
    for _ in range(2):
        dR, dS = ctx.zeros(n * m), ctx.zeros(2 * m)
        eigmi.lobpcg_resid_mv8(ctx, n, m, dK, dM, dT, dR, dS)
        out.append((_cols(dR, n, m), dS.get()))
    R = KX - MX * th
    assert np.array_equal(out[0][0], R)
    ref = np.concatenate([(R * R).sum(axis=0), (MX * MX).sum(axis=0)])
    print(f"lobpcg resid n={n} m={m}: max rel sum error {np.abs(out[0][1] / ref - 1).max():.2e}")
    assert np.abs(out[0][1] - ref).max() <= 1e-13 * np.abs(ref).max() and np.abs(out[0][1] / ref - 1).max() <= 1e-13
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])


@pytest.mark.parametrize("n", [61, 130, 4099])
@pytest.mark.parametrize("m", [8, 16, 24, 32])
@pytest.mark.parametrize("kb", [2, 3])
def test_update_kernel(ctx, n, m, kb):
    rng = np.random.default_rng(n + m + kb)
    S = rng.standard_normal((n, 3 * m))
    if kb == 2:
        S[:, 2 * m:] = np.nan  # the P slice is written, never read
    C = rng.standard_normal((kb * m, 2 * m))
    dC = ctx.array(C)
    out = []
    for _ in range(2):
        dS = _mv(ctx, S)
        eigmi.lobpcg_update_mv8(ctx, n, m, kb, dS, dC)
        out.append(_cols(dS, n, 3 * m))
    got = out[0]
    B = S[:, :kb * m]
    bar = 1e-13 * (np.abs(B) @ np.abs(C)).max()
    err = max(np.abs(got[:, :m] - B @ C[:, :m]).max(), np.abs(got[:, 2 * m:] - B @ C[:, m:]).max())
    print(f"lobpcg update n={n} m={m} kb={kb}: max error {err:.2e} (bar {bar:.2e})")
    assert np.all(np.isfinite(got)) and err <= bar
    assert np.array_equal(got[:, m:2 * m], S[:, m:2 * m])
    assert np.array_equal(out[0], out[1])


def test_kernels_past_one_pass_per_wave(ctx):
    """The sizes above give every wave of k_lobpcg_update at most one 16-row tile and every lane of
    k_lobpcg_resid at most one row per column block; here a wave takes two or three tiles (the loads of
    the next tile issued before the MFMAs of this one: n = 40,000 > 16 x 4 x 256) and the residual's grid
    is at its cap with several rows per lane (n = 70,000 > 64 x 1024)."""
    test_update_kernel(ctx, 40000, 32, 3)
    test_update_kernel(ctx, 40000, 8, 2)
    test_resid_kernel(ctx, 70000, 8)


# ------------------------------------------------------------------------------------- drivers
def _device_solver(ctx, name, m, X0=None, seed=123, keep=None):
    """The device Lobpcg of lobpcg_ref.problem(name); the handles it needs alive go into `keep`."""
    p = lr.problem(name)
    if p["blocked"] is not None:
        dK, dM = [eigmi.Matrix.from_bcsr(ctx, A.rowptr, A.col, A.val, A.br, A.bc) for A in p["blocked"]]
    else:
        dK, dM = _upload(ctx, p["K"]), (_upload(ctx, p["M"]) if p["M"] is not None else None)
    which = eigmi.WHICH_LA if which_of(name) == "LA" else eigmi.WHICH_SA
    dX = _mv(ctx, X0) if X0 is not None else None
    s = eigmi.Lobpcg(dK, dM, block=m, which=which, X0=dX, seed=seed)
    mg = None
    if "mg" in p:
        mg = eigmi.Multigrid(dK, p["dims"], max_cols=32, smooth_degree=2, smooth_ratio=5.0)
        s.precond_mg(mg, 1)
    elif p["T"] is not None:
        s.precond_cheb(p["degree"], p["lmin"], p["lmax"])
    if keep is not None:
        keep.extend([s, mg, dK, dM])
    return s


def _close(keep):
    for h in keep:
        if h is not None:
            h.close()


@pytest.mark.parametrize("name,m", PARITY_CASES)
def test_fixed_iteration_parity(ctx, name, m):
    p = lr.problem(name)
    X0 = start_block(name, m)
    ref = lr.Lobpcg(p["K"], p["M"], m, X0=X0, precond=p["T"])
    keep = []
    dev = _device_solver(ctx, name, m, X0=X0, keep=keep)
    bar = 100 * SENSITIVITY[name, m]
    done = 0
    for k in (3, 6, 10):
        ref.step(k - done, NEV, 0.0)
        it, conv, _ = dev.step(k - done, NEV, 0.0)
        assert it == k - done and not conv
        done = k
        th = dev.ritz(m, want_resid=False)[0]
        d = np.abs(th / ref.theta - 1).max()
        print(f"lobpcg parity {name} m={m} after {k} iterations: max rel |theta - ref| = {d:.2e} (bar {bar:.1e})")
        assert d <= bar
    _close(keep)


@functools.lru_cache(maxsize=None)
def _ref_count(name, m, tol):
    p = lr.problem(name)
    s = lr.Lobpcg(p["K"], p["M"], m, which_of(name), precond=p["T"])
    it, conv = s.step(500, NEV, tol)
    assert conv
    return it


def _exact(name):
    if name.startswith("lap2d"):
        return np.sort(oracle.eig_laplace2d(lr.problem(name)["N"]))[:NEV]
    return dense_reference(name)


def _check_converged(ctx, name, m, tol):
    p = lr.problem(name)
    K, M = p["K"], p["M"]
    keep = []
    dev = _device_solver(ctx, name, m, keep=keep)
    it, conv, t = dev.step(500, NEV, tol)
    ev, Y, res = dev.ritz(NEV, want_evec=True)
    Y = Y.T
    MY = M @ Y if M is not None else Y
    host = np.linalg.norm(K @ Y - MY * ev, axis=0)
    exact, count = _exact(name), _ref_count(name, m, tol)
    G = Y.T @ MY
    print(f"lobpcg {name} m={m} tol={tol:g}: {it} iterations (restatement {count}), max rel |ev - exact| = "
          f"{np.abs(ev / exact - 1).max():.2e}, max residual / (theta |M y|) = "
          f"{(res / (np.abs(ev) * np.linalg.norm(MY, axis=0))).max():.2e}, |Y^T M Y - I| = "
          f"{np.abs(G - np.eye(NEV)).max():.2e}, {t.total_ms / max(it, 1):.2f} ms per iteration")
    assert conv
    assert np.abs(ev / exact - 1).max() <= 1e-10
    assert np.all(res <= tol * np.abs(ev) * np.linalg.norm(MY, axis=0))
    assert np.all(np.abs(res - host) <= 1e-6 * host)
    assert np.abs(G - np.eye(NEV)).max() <= 1e-12
    assert it <= count + max(2, math.ceil(0.1 * count))
    _close(keep)


@pytest.mark.parametrize("name,m", [("p1-12-jacobi", 8), ("p1-24-mg", 32), ("lap2d-64-cheb8", 16), ("q1s-5-cheb4", 8)])
def test_converged_answers(ctx, name, m):
    _check_converged(ctx, name, m, 1e-8)


def test_tight_tolerance_with_one_vcycle(ctx):
    """tol 1e-11 at N = 24 with one V-cycle per iteration: the pencil residual the shift-invert block
    Lanczos tests hold only to 1e-5."""
    _check_converged(ctx, "p1-24-mg", 32, 1e-11)


def test_largest_end_warm_start_and_reproducibility(ctx):
    name = "p1-8-none"
    keep = []
    a = _device_solver(ctx, name, 8, keep=keep)
    it, conv, _ = a.step(500, NEV, 1e-8)
    ev, Y, _ = a.ritz(8, want_evec=True)
    exact = dense_reference(name)
    assert conv and np.all(np.diff(ev[:NEV]) <= 0)
    assert np.abs(ev[:NEV] / exact - 1).max() <= 1e-10
    b = _device_solver(ctx, name, 8, keep=keep)
    b.step(500, NEV, 1e-8)
    assert np.array_equal(b.ritz(8, want_resid=False)[0], ev)
    c = _device_solver(ctx, name, 8, X0=Y.T, keep=keep)
    assert c.step(500, NEV, 1e-8)[:2] == (0, True)
    _close(keep)


# -------------------------------------------------------------------------------------- errors
def test_refusals(ctx):
    K, M = oracle.p1_kuhn(6)
    dK, dM = _upload(ctx, K), _upload(ctx, M)
    A = oracle.q1elast(3)
    dA = eigmi.Matrix.from_bcsr(ctx, A.rowptr, A.col, A.val, 3, 3)

    def code(f):
        with pytest.raises(eigmi.EigError) as e:
            f()
        return e.value.code

    # differing blocks (3x3 K, 1x1 M of other rows) and rectangular blocks
    assert code(lambda: eigmi.Lobpcg(dA, dM)) == eigmi.EIG_ERR_BLOCKSIZE
    R = eigmi.Matrix.from_bcsr(ctx, np.arange(9, dtype=np.int64), np.arange(8, dtype=np.int32), np.ones(16), 2, 1)
    assert code(lambda: eigmi.Lobpcg(R)) == eigmi.EIG_ERR_BLOCKSIZE
    assert code(lambda: eigmi.Lobpcg(dK, dM, block=64)) == eigmi.EIG_ERR_ARG
    small = _upload(ctx, sp.identity(24).tocsr())
    assert code(lambda: eigmi.Lobpcg(small, block=8)) == eigmi.EIG_ERR_SHAPE
    la = eigmi.Lobpcg(dK, dM, block=8, which=eigmi.WHICH_LA)
    mg8 = eigmi.Multigrid(dK, (6, 6, 6), max_cols=8)
    assert code(lambda: la.precond_cheb(2, 0.2, 2.0)) == eigmi.EIG_ERR_ARG
    assert code(lambda: la.precond_mg(mg8, 1)) == eigmi.EIG_ERR_ARG
    sa = eigmi.Lobpcg(dK, dM, block=16)
    assert code(lambda: sa.precond_mg(mg8, 1)) == eigmi.EIG_ERR_ARG  # max_cols < block
    K8 = _upload(ctx, oracle.p1_kuhn(8)[0])
    mg_other = eigmi.Multigrid(K8, (8, 8, 8), max_cols=16)
    assert code(lambda: sa.precond_mg(mg_other, 1)) == eigmi.EIG_ERR_ARG  # another size
    ctx2 = eigmi.Context(0)  # another context: the same matrix and grid, max_cols wide enough
    K2 = _upload(ctx2, K)
    mg_ctx2 = eigmi.Multigrid(K2, (6, 6, 6), max_cols=16)
    assert code(lambda: sa.precond_mg(mg_ctx2, 1)) == eigmi.EIG_ERR_ARG
    for h in (mg_ctx2, K2, ctx2, la, sa, mg8, mg_other, K8, small, R, dA, dK, dM):
        h.close()


def test_refuses_distributed_context(ctx):
    """Two loopback ranks, each with half the rows of a 2-D Laplacian: EIG_ERR_ARG on both."""
    A, P = oracle.laplace2d(16), 2
    hub = eigmi.loopback_create(P)
    out = [None] * P

    def rank(r):
        rc = eigmi.Context(0)
        try:
            rc.comm_init_loopback(hub, r)
            b, e = A.n * r // P, A.n * (r + 1) // P
            lo, hi = A.rowptr[b], A.rowptr[e]
            M = eigmi.Matrix.from_rows(rc, A.n, b, A.rowptr[b:e + 1] - lo, A.col[lo:hi], A.val[lo:hi])
            try:
                eigmi.Lobpcg(M, block=8)
                out[r] = "accepted"
            except eigmi.EigError as err:
                out[r] = err.code
            M.close()
        except Exception as err:  # noqa: BLE001 -- reported below
            out[r] = repr(err)
        finally:
            rc.close()

    th = [threading.Thread(target=rank, args=(r,)) for r in range(P)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    eigmi.loopback_destroy(hub)
    assert out == [eigmi.EIG_ERR_ARG] * P, out


def test_iteration_is_redone_without_p(ctx):
    """tests/test_lobpcg_ref.py redo_case: the second iteration's W lies numerically inside span [X P], so
    it fails (a failed pivot, or the check of S^T S = I) and is redone on [X W]; the run goes on with the
    exact eigenvalues and an orthonormal X instead of a collapsed block."""
    K, X0 = redo_case()
    dK = _upload(ctx, K)
    s = eigmi.Lobpcg(dK, None, block=8, X0=_mv(ctx, X0))
    it, conv, t = s.step(3, NEV, 0.0)
    ev, Y, _ = s.ritz(8, want_evec=True)
    print(f"lobpcg redo case: p_dropped {t.p_dropped}, orth_rejected {t.orth_rejected}, orth_dev {t.orth_dev:.1e}")
    assert it == 3 and t.p_dropped >= 1
    assert np.abs(ev - np.arange(1.0, 9.0)).max() <= 1e-12
    assert np.abs(Y @ Y.T - np.eye(8)).max() <= 1e-12
    s.close()
    dK.close()


def test_blocked_problem_is_the_blocked_drivers_pair(ctx):
    """lobpcg_ref.scaled_q1elast builds the matrices of tests/test_gpu_blocked_drivers.py itself."""
    from test_gpu_blocked_drivers import mats
    d, p = mats(), lr.problem("q1s-5-cheb4")
    assert np.array_equal(p["K"].toarray(), d["DS"]) and np.array_equal(p["M"].toarray(), d["DB"])


def test_forced_breakdown_is_a_status(ctx):
    """K = diag(1..64), M = NULL, X0 = the first 8 unit vectors, tol = 0, 2 iterations: the residual is
    exactly zero, so W = 0 and its Gram has no positive pivot: EIG_ERR_BREAKDOWN, and the workspace is
    destroyed cleanly; the context still works afterwards."""
    dK = _upload(ctx, sp.diags(np.arange(1.0, 65.0)).tocsr())
    s = eigmi.Lobpcg(dK, None, block=8, X0=_mv(ctx, np.eye(64)[:, :8]))
    with pytest.raises(eigmi.EigError) as e:
        s.step(2, NEV, 0.0)
    assert e.value.code == eigmi.EIG_ERR_BREAKDOWN
    s.close()
    x = ctx.array(np.arange(8.0))
    assert np.array_equal(x.get(), np.arange(8.0))
    dK.close()
