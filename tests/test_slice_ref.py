"""CPU checks of the spectrum-slicing restatement (tests/slice_ref.py) and of the library's host-only filter
entry points against it: the Clenshaw filter against V p(Lambda) V^T X from a dense eigh, eig_filter_coefs
against the restatement, the refusals, and the restatement driver on the end-to-end cases of
tests/test_gpu_slice.py (which takes CASES from here).

The driver cases: windows at gap midpoints of the dense spectrum of the project's generated matrices, found
by a search for windows of 0.015 .. 0.05 of the range whose end gaps are large against their width.  At
tol 1e-8, degree 80 on [lmin, lmax] = [0, 13] the restatement took
    kind 8 (variable-coefficient 7-point), N = 10, eigenvalues 10..16: 4 iterations at block 24, 3 at block 32
    kind 8, N = 16, eigenvalues 4..10:                                 6 iterations at block 24, 4 at block 32
    q1elast N = 6 (3x3 blocks), eigenvalues 469..474:                  7 iterations at block 24, 6 at block 32
(block 16 needed 10 and 15 on the first and the last: under the cap only for the first), so the cap of 12 holds
with room.  Kind 8 appears at two sizes because its GPU case on the box image needs a grid of at least
16 x 8 x 3 rows (the box kernels' tile): N = 10 runs on the SELL kernels only, N = 16 is the smallest cube
the box image takes."""
import numpy as np
import pytest

import eigmi
import oracle
import slice_ref as sr

MAX_ITERS = 12
TOL = 1e-8
LMIN, LMAX = 0.0, 13.0   # encloses the three spectra (largest eigenvalues 12.37, 12.76 and 12.62)
DEGREE = 80
# name -> (first eigenvalue index, count, block)
CASES = {"var10": (10, 7, 24), "var16": (4, 7, 32), "q1elast6": (469, 6, 32)}
SATURATED = ("var10", 7, 10, 8)  # matrix, first index, count, block: 10 eigenvalues, a block of 8

_CACHE = {}


def matrix(name):
    """(oracle.CSR, scipy CSR of its scalar expansion, ascending dense eigenvalues); built once."""
    if name not in _CACHE:
        if name.startswith("var"):
            rp, c, v = eigmi.gen_matrix(eigmi.GEN_VARCOEF3D, int(name[3:]))
            A = oracle.CSR(rp.size - 1, rp, c, v)
        else:
            A = oracle.q1elast(6)
        S = A.to_scipy().tocsr()
        _CACHE[name] = (A, S, np.linalg.eigvalsh(S.toarray()))
    return _CACHE[name]


def window(lam, i0, cnt):
    """[a, b] at the midpoints of the gaps below eigenvalue i0 and above eigenvalue i0 + cnt - 1."""
    return 0.5 * (lam[i0 - 1] + lam[i0]), 0.5 * (lam[i0 + cnt - 1] + lam[i0 + cnt])


def start_block(n, block, seed=123):
    return oracle.mv_to_cols(oracle.random_mv8(n, block, seed), n, block)


def check_eigenvalues(theta, lam, i0, cnt, a, b, tol=TOL):
    want = lam[i0:i0 + cnt]
    assert theta.size == cnt, (theta, want)
    err = np.abs(np.sort(theta) - want)
    bound = tol * np.maximum(np.abs(want), max(abs(a), abs(b)))
    print("eigenvalue errors", err.max(), "bound", bound.min())
    assert np.all(err <= bound), (err, bound)


@pytest.mark.parametrize("degree", [20, 80, 200])
def test_filter_matches_dense_function(degree):
    _, S, lam = matrix("var10")
    D = S.toarray()
    w, V = np.linalg.eigh(D)
    a, b = window(lam, 10, 7)
    X = np.random.default_rng(degree).standard_normal((lam.size, 8))
    gam = sr.filter_coefs(a, b, LMIN, LMAX, degree)
    c, e, _, _ = sr.filter_window(a, b, LMIN, LMAX)
    ref = V @ (sr.filter_poly(gam, (w - c) / e)[:, None] * (V.T @ X))
    got = sr.apply_filter(S, X, a, b, LMIN, LMAX, degree)
    err = np.abs(got - ref).max()
    print("degree", degree, "error", err, "scale", np.abs(ref).max())
    assert err <= 1e-12 * np.abs(ref).max()
    # the filter is the window's indicator up to the Jackson kernel's resolution: ~1 inside, ~0 far outside
    p = sr.filter_poly(gam, (lam - c) / e)
    assert p.min() > -1e-12 and p.max() < 1.0 + 1e-12


@pytest.mark.parametrize("args", [(0.9, 1.2, 0.0, 13.0, 80), (4.0, 4.5, -2.0, 15.0, 200), (-1.0, 0.5, 0.0, 13.0, 20),
                                  (12.0, 20.0, 0.0, 13.0, 2), (5.0, 5.1, 0.0, 13.0, 0)])
def test_library_coefficients_match_restatement(args):
    a, b, lmin, lmax, d = args
    gam = eigmi.filter_coefs(a, b, lmin, lmax, d)
    ref = sr.filter_coefs(a, b, lmin, lmax, d)
    assert gam.size == ref.size == eigmi.filter_degree(a, b, lmin, lmax, d) + 1
    if d == 0:
        assert gam.size - 1 == sr.default_degree(a, b, lmin, lmax)
    print("max coefficient difference", np.abs(gam - ref).max())
    assert np.abs(gam - ref).max() <= 1e-15
    _, _, ta, tb = sr.filter_window(a, b, lmin, lmax)
    # gamma_0 = (theta_a - theta_b) / pi exactly as computed: the Jackson factor g_0 is 1 without rounding.  Here
    # for the restatement; for the library with its own arccos (an ulp from numpy's at some arguments) in
    # tests/cpp/filter_host_test.cc
    assert ref[0] == (ta - tb) / np.pi


def test_default_degree_rule():
    # resolution pi / (d + 2) at a quarter of the angular width, clamped to [20, 2000]
    for a, b in ((0.9, 1.2), (5.0, 5.1), (6.0, 6.001), (0.0, 13.0)):
        _, _, ta, tb = sr.filter_window(a, b, LMIN, LMAX)
        d = eigmi.filter_degree(a, b, LMIN, LMAX, 0)
        assert d == sr.default_degree(a, b, LMIN, LMAX) == int(min(2000, max(20, np.ceil(4 * np.pi / (ta - tb)) - 2)))
    assert eigmi.filter_degree(6.0, 6.001, LMIN, LMAX, 0) == 2000 and eigmi.filter_degree(0.0, 13.0, LMIN, LMAX, 0) == 20
    assert eigmi.filter_degree(0.9, 1.2, LMIN, LMAX, 57) == 57


@pytest.mark.parametrize("args", [(1.2, 0.9, 0.0, 13.0, 80),    # a > b
                                  (1.0, 1.0, 0.0, 13.0, 80),    # a == b
                                  (14.0, 15.0, 0.0, 13.0, 80),  # window above the spectrum bounds
                                  (-3.0, -1.0, 0.0, 13.0, 80),  # window below them
                                  (0.9, 1.2, 13.0, 0.0, 80),    # lmin > lmax
                                  (0.9, 1.2, 0.0, 13.0, 1),     # degree 1
                                  (0.9, 1.2, 0.0, 13.0, -4),    # negative degree
                                  (0.9, float("nan"), 0.0, 13.0, 80)])
def test_refusals(args):
    with pytest.raises(eigmi.EigError) as e:
        eigmi.filter_coefs(*args)
    assert e.value.code == eigmi.EIG_ERR_ARG
    with pytest.raises(eigmi.EigError):
        eigmi.filter_degree(*args)
    if args[4] >= 0:
        with pytest.raises(ValueError):
            sr.filter_coefs(*args)


def test_window_is_clamped_into_the_bounds():
    assert np.array_equal(eigmi.filter_coefs(-5.0, 1.0, 0.0, 13.0, 40), eigmi.filter_coefs(0.0, 1.0, 0.0, 13.0, 40))
    assert np.array_equal(eigmi.filter_coefs(12.0, 99.0, 0.0, 13.0, 40), eigmi.filter_coefs(12.0, 13.0, 0.0, 13.0, 40))


def test_step_scalars_reproduce_clenshaw():
    """The folded first two steps (no b_d, no b_{d+1}) give the textbook recurrence."""
    _, S, lam = matrix("var10")
    a, b = window(lam, 10, 7)
    for d in (2, 3, 4, 17):
        gam = sr.filter_coefs(a, b, LMIN, LMAX, d)
        c, e, _, _ = sr.filter_window(a, b, LMIN, LMAX)
        X = np.random.default_rng(d).standard_normal((lam.size, 3))
        Ah = lambda V: (S @ V - c * V) / e  # noqa: E731
        b1, b2 = np.zeros_like(X), np.zeros_like(X)
        for k in range(d, 0, -1):
            b1, b2 = gam[k] * X + 2.0 * Ah(b1) - b2, b1
        ref = gam[0] * X + Ah(b1) - b2
        got = sr.apply_filter(S, X, a, b, LMIN, LMAX, d)
        assert np.abs(got - ref).max() <= 1e-13 * max(1.0, np.abs(ref).max())


@pytest.mark.parametrize("name", sorted(CASES))
def test_restatement_driver(name):
    _, S, lam = matrix(name)
    i0, cnt, block = CASES[name]
    a, b = window(lam, i0, cnt)
    r = sr.slice_solve(S, start_block(lam.size, block), a, b, LMIN, LMAX, DEGREE, TOL, MAX_ITERS)
    print(name, "window", a, b, "iterations", r["iters"], "converged", r["converged"])
    assert r["converged"] and r["iters"] <= MAX_ITERS and not r["saturated"]
    check_eigenvalues(r["theta"][r["accepted"]], lam, i0, cnt, a, b)
    X = r["X"]
    assert np.abs(X.T @ X - np.eye(block)).max() <= 1e-12


def test_restatement_saturates_on_a_small_block():
    name, i0, cnt, block = SATURATED
    _, S, lam = matrix(name)
    a, b = window(lam, i0, cnt)
    r = sr.slice_solve(S, start_block(lam.size, block), a, b, LMIN, LMAX, DEGREE, 0.0, 6)
    assert r["iters"] == 6 and not r["converged"] and r["saturated"] and r["accepted"].sum() == block < cnt


def test_lanczos_bounds_enclose_the_spectrum():
    """theta_min - beta_k, theta_max + beta_k from 30 steps enclose the dense spectrum on the driver matrices."""
    for name in sorted(CASES):
        _, S, lam = matrix(name)
        S.sort_indices()
        A = oracle.CSR(S.shape[0], S.indptr.astype(np.int64), S.indices.astype(np.int32), S.data.copy())  # scalar rows
        _, al, be = oracle.lanczos(A, oracle.random_vec(A.n, 123), 30)
        lo, hi = sr.spectrum_bounds(al, be)
        print(name, "bounds", lo, hi, "spectrum", lam[0], lam[-1])
        assert lo <= lam[0] and hi >= lam[-1]


def test_count_estimate_within_four_sigma():
    _, S, lam = matrix("var10")
    a, b = window(lam, 10, 7)
    nvec = 32
    Z = start_block(lam.size, nvec, seed=7)
    est = sr.count_estimate(S, Z, a, b, LMIN, LMAX, DEGREE)
    c, e, _, _ = sr.filter_window(a, b, LMIN, LMAX)
    p = sr.filter_poly(sr.filter_coefs(a, b, LMIN, LMAX, DEGREE), (lam - c) / e)
    print("estimate", est, "trace", p.sum(), "bound", 4 * np.sqrt(2 * np.sum(p * p) / nvec))
    assert abs(est - p.sum()) <= 4 * np.sqrt(2 * np.sum(p * p) / nvec)
