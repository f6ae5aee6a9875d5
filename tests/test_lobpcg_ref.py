"""CPU tests of tests/lobpcg_ref.py, the numpy restatement of LOBPCG (csrc/lobpcg.cpp): it is the
reference of tests/test_gpu_lobpcg.py, so its own answers, iteration counts and sensitivity are
pinned here.

Answers: nev = 4, tol 1e-8 against dense scipy.linalg.eigh(K, M) to 1e-10 relative, X^T M X - I <=
1e-12, true residuals ||K x - theta M x|| <= tol theta ||M x||.

Iteration counts (nev = 4; printed by test_answers_and_iteration_counts, the reference of the GPU
tests' iteration bars):
    p1-8-jacobi   m 8   tol 1e-8   42        p1-12-jacobi    m 8   tol 1e-8   63
    p1-8-mg       m 8   tol 1e-8   13        p1-12-mg        m 8   tol 1e-8   13
    p1-12-mg      m 32  tol 1e-8    9        lap2d-64-cheb8  m 16  tol 1e-8   28
    q1s-5-cheb4   m 8   tol 1e-8   29        p1-24-mg        m 32  tol 1e-8   10
    p1-24-mg      m 32  tol 1e-11  12        p1-8-none (LA)  m 8   tol 1e-8   56
(jacobi: Chebyshev-Jacobi degree 1 = Jacobi up to a factor; mg: one V-cycle of tests/mg_ref.py; see
lobpcg_ref.problem.)

Sensitivity: the relative change of the m Ritz values after 3, 6 and 10 forced iterations when
every entry of the start block moves by one ulp (up or down at random).  Measured here after 3 / 6 /
10 iterations:
    p1-12-jacobi m 8    1.1e-14  1.2e-14  2.5e-14
    p1-12-mg     m 8    7.3e-15  6.0e-15  1.5e-13
    p1-12-mg     m 32   1.5e-14  6.7e-15  3.3e-12
(the largest figures belong to the upper Ritz values of the block, which sit in the dense part of the
spectrum and are far from converged when the lowest ones already are).  SENSITIVITY below holds each
case's ceiling, asserted to hold and to stay below 1e-11.  The GPU parity bar is 100 x SENSITIVITY
(the device sums every Gram in another order)."""
import numpy as np
import pytest
import scipy.linalg as sl

import lobpcg_ref as lr

# name, block, tol, the count recorded above
CASES = [("p1-8-jacobi", 8, 1e-8, 42), ("p1-12-jacobi", 8, 1e-8, 63), ("p1-8-mg", 8, 1e-8, 13),
         ("p1-12-mg", 8, 1e-8, 13), ("p1-12-mg", 32, 1e-8, 9), ("lap2d-64-cheb8", 16, 1e-8, 28),
         ("q1s-5-cheb4", 8, 1e-8, 29), ("p1-24-mg", 32, 1e-8, 10), ("p1-24-mg", 32, 1e-11, 12),
         ("p1-8-none", 8, 1e-8, 56)]
NEV = 4
SENSITIVITY = {("p1-12-jacobi", 8): 3e-14, ("p1-12-mg", 8): 2e-13, ("p1-12-mg", 32): 4e-12}
PARITY_CASES = sorted(SENSITIVITY)


def which_of(name):
    return "LA" if name.endswith("-none") else "SA"


def dense_reference(name, nev=NEV):
    p = lr.problem(name)
    if "exact" not in p:
        n = p["K"].shape[0]
        if n > 5000:  # p1-24: no dense solve at 13,824 rows; ARPACK shift-invert with an exact factorisation
            import scipy.sparse.linalg as ssl
            p["exact"] = np.sort(ssl.eigsh(p["K"], k=nev, M=p["M"], sigma=0.0, which="LM", tol=1e-14,
                                           v0=np.ones(n), return_eigenvectors=False))
        else:
            w = sl.eigh(p["K"].toarray(), p["M"].toarray() if p["M"] is not None else None, eigvals_only=True)
            p["exact"] = w[::-1][:nev] if which_of(name) == "LA" else w[:nev]
    return p["exact"]


def start_block(name, m, seed=7):
    n = lr.problem(name)["K"].shape[0]
    return np.random.default_rng(seed).standard_normal((n, m))


@pytest.mark.parametrize("name,m,tol,recorded", CASES, ids=["%s-m%d-%g" % c[:3] for c in CASES])
def test_answers_and_iteration_counts(name, m, tol, recorded):
    p = lr.problem(name)
    s = lr.Lobpcg(p["K"], p["M"], m, which_of(name), precond=p["T"])
    it, conv = s.step(500, NEV, tol)
    ev, Y, res = s.ritz(NEV)
    exact = dense_reference(name)
    MY = p["M"] @ Y if p["M"] is not None else Y
    G = s.X.T @ (p["M"] @ s.X if p["M"] is not None else s.X)
    rel = res / (np.abs(ev) * np.linalg.norm(MY, axis=0))
    print(f"lobpcg_ref {name} m={m} tol={tol:g}: {it} iterations (recorded {recorded}), "
          f"max rel |ev - exact| = {np.abs(ev / exact - 1).max():.2e}, |X^T M X - I| = "
          f"{np.abs(G - np.eye(m)).max():.2e}, max residual / (theta |M x|) = {rel.max():.2e}")
    assert conv
    assert np.abs(ev / exact - 1).max() <= 1e-10
    assert np.abs(G - np.eye(m)).max() <= 1e-12
    assert np.all(rel <= tol)
    # the recorded counts are the GPU tests' reference: they move by an iteration at most with the BLAS
    assert abs(it - recorded) <= 1


@pytest.mark.parametrize("name,m", PARITY_CASES)
def test_sensitivity_to_one_ulp(name, m):
    p = lr.problem(name)
    X0 = start_block(name, m)
    rng = np.random.default_rng(11)
    X1 = np.nextafter(X0, np.where(rng.random(X0.shape) < 0.5, -np.inf, np.inf))
    a = lr.Lobpcg(p["K"], p["M"], m, X0=X0, precond=p["T"])
    b = lr.Lobpcg(p["K"], p["M"], m, X0=X1, precond=p["T"])
    done, worst = 0, 0.0
    for k in (3, 6, 10):
        a.step(k - done, NEV, 0.0)
        b.step(k - done, NEV, 0.0)
        done = k
        d = np.abs(b.theta / a.theta - 1).max()
        worst = max(worst, d)
        print(f"lobpcg_ref sensitivity {name} m={m} after {k} iterations: {d:.2e}")
    assert worst <= SENSITIVITY[name, m] < 1e-11


def test_forced_breakdown_and_warm_start():
    """K = diag(1..64), X0 = the first 8 unit vectors: the residual is exactly zero, W = 0, Breakdown.
    A run restarted from its converged X converges after 0 iterations."""
    import scipy.sparse as sp
    s = lr.Lobpcg(sp.diags(np.arange(1.0, 65.0)).tocsr(), None, 8, X0=np.eye(64)[:, :8])
    with pytest.raises(lr.Breakdown):
        s.step(2, 4, 0.0)
    p = lr.problem("p1-8-mg")
    a = lr.Lobpcg(p["K"], p["M"], 8, precond=p["T"])
    assert a.step(100, NEV, 1e-8)[1]
    b = lr.Lobpcg(p["K"], p["M"], 8, X0=a.X, precond=p["T"])
    assert b.step(100, NEV, 1e-8) == (0, True)


def redo_case(eps=1e-3):
    """K = diag(1..64), M = None, block 8, X0 = e_1..e_8 plus eps times random multiples of e_9..e_16:
    every vector of the run stays in the first 16 coordinates.  Iteration 1's [X W] spans them all, so its
    Rayleigh-Ritz returns X = e_1..e_8 and P = a basis of e_9..e_16 to rounding; iteration 2's residual is
    rounding noise inside span [X P], its W is what two Gram-Schmidt passes leave of it, and [X W P] cannot
    be orthonormal: the iteration must be redone on [X W]."""
    import scipy.sparse as sp
    X0 = np.eye(64)[:, :8].copy()
    X0[8:16, :] = eps * np.random.default_rng(3).standard_normal((8, 8))
    return sp.diags(np.arange(1.0, 65.0)).tocsr(), X0


def test_iteration_is_redone_without_p():
    """The redo path: the second iteration fails (failed pivot or S^T S != I) and is redone without P; the
    run goes on with X orthonormal and the exact eigenvalues.  Without the check of S^T M S = I the
    rank-deficient S would hand the Rayleigh-Ritz null vectors as Ritz vectors of value 0."""
    K, X0 = redo_case()
    s = lr.Lobpcg(K, None, 8, X0=X0)
    assert s.step(3, NEV, 0.0) == (3, False)
    print(f"lobpcg_ref redo case: p_dropped {s.p_dropped}, orth_rejected {s.orth_rejected}, orth_dev {s.orth_dev:.1e}")
    assert s.p_dropped >= 1
    assert np.abs(s.theta - np.arange(1.0, 9.0)).max() <= 1e-12
    assert np.abs(s.X.T @ s.X - np.eye(8)).max() <= 1e-12
