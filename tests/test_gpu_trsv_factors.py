"""eig_inverse_mv8 (csrc/k_trsv.hip) on general LU factors in the exported form -- P != Q,
unsymmetric patterns, sparse rows with far entries, empty rows, crafted widths and distances
(tests/lu_factors.py) -- through each of its three device paths, and every time the test asserts
with eig_lu_solver_info WHICH path ran:

  staged    k_tsolve_staged.  A factor that fits the staged image also fits the block-inverse
            image, which is then the default, so the staged kernel is forced by construction:
            pivots 1e-3 and 1e3 in one 64-row block of U fail the kBinvCond gate (n = 1: the pivot
            1e-5 beside the identity padding of the block).  Bitwise the reference arithmetic
            (oracle.inverse_mv8), bitwise k_tsolve on the same factors, and within the
            backward-error bound of lu_factors.residual_ratio.
  csr       k_tsolve: factors the staged image does not admit (a row of 129 outside entries, an
            entry 5 blocks away) or that reach past both images (9 blocks).  Bitwise + the bound.
  blockinv  k_binv_z + k_binv_chain / k_binv_chain16 on benign factors (pivots in [1, 2]) for every
            chain template and different coupled-block counts in L and U: the constructed counts
            exactly, and within BINV_RTOL of the reference arithmetic.

The oracle is anchored on the same factor sets in tests/test_trsv_factors.py (CPU)."""
import numpy as np
import pytest

import eigmi
import lu_factors as F
from lu_factors import BINV_RTOL

pytestmark = pytest.mark.gpu


def _names(kind):
    return sorted(k for k, c in F.CASES.items() if c["expect"][0] == kind)


@pytest.fixture
def factor(ctx, name):
    """The case's factors on the device, closed whether the test passes or not."""
    lu = eigmi.LU.from_factors(ctx, **F.case(name)[0])
    yield lu
    lu.close()


def _solve(ctx, lu, X, n, m, kind=None):
    """One solve on a fresh copy of X (Qin is scratch afterwards) -> (result, kernel that ran)."""
    din, dout = ctx.array(X), ctx.zeros(n * m)
    lu.set_solver(kind)
    try:
        used = lu.solver_info()[0]
        lu.inverse_mv8(m, din, dout)
    finally:
        lu.set_solver(None)
    return dout.get(), used


def _against_reference(name, out, ref):
    if F.CASES[name]["check"] == "rounding":  # L rows given descending are sorted at upload
        assert np.abs(out - ref).max() <= 1e-13 * np.abs(ref).max()
    else:
        assert np.array_equal(out, ref), "not bitwise the reference arithmetic"


@pytest.mark.parametrize("name", _names("staged"))
def test_staged_kernel(ctx, factor, name):
    d, X, m, ref = F.case(name)
    n, lu = d["Lp"].size - 1, factor
    assert lu.solver_info() == F.CASES[name]["expect"]  # ("staged", gd_L, gd_U) before any solve
    out, used = _solve(ctx, lu, X, n, m)
    assert used == "staged" and lu.solver_info()[0] == "staged"
    _against_reference(name, out, ref)
    out_csr, used_csr = _solve(ctx, lu, X, n, m, "csr")
    assert used_csr == "csr"
    assert np.array_equal(out, out_csr), "k_tsolve_staged and k_tsolve differ"
    ratio = F.residual_ratio(d, X, out, m)
    print(f"{name}: kernel {used}, n {n}, m {m}, residual / bound {ratio:.3f} (k_tsolve: bitwise the same)")
    assert ratio <= 1.0


@pytest.mark.parametrize("name", _names("csr"))
def test_csr_kernel(ctx, factor, name):
    d, X, m, ref = F.case(name)
    n, lu = d["Lp"].size - 1, factor
    assert lu.solver_info() == F.CASES[name]["expect"]
    out, used = _solve(ctx, lu, X, n, m)
    assert used == "csr"
    _against_reference(name, out, ref)
    # asking for the staged kernel on a factor its image does not admit still runs k_tsolve
    out_st, used_st = _solve(ctx, lu, X, n, m, "staged")
    assert used_st == "csr" and np.array_equal(out_st, ref)
    ratio = F.residual_ratio(d, X, out, m)
    print(f"{name}: kernel {used}, n {n}, m {m}, residual / bound {ratio:.3f}")
    assert ratio <= 1.0


@pytest.mark.parametrize("name", _names("blockinv"))
def test_blockinv_chain(ctx, factor, name):
    d, X, m, ref = F.case(name)
    n, lu = d["Lp"].size - 1, factor
    info = lu.solver_info()
    assert info == F.CASES[name]["expect"]  # ("blockinv", gd_L, gd_U) exactly as constructed
    out, used = _solve(ctx, lu, X, n, m)
    assert used == "blockinv"
    err = np.abs(out - ref).max() / np.abs(ref).max()
    print(f"{name}: kernel {used}, coupled {info[1]}/{info[2]}, n {n}, m {m}, vs reference arithmetic {err:.2e}, "
          f"residual / bound {F.residual_ratio(d, X, out, m):.3f}")
    assert err <= BINV_RTOL
    # the same benign factors through k_tsolve (the staged request takes it beside a block-inverse image)
    for kind in ("csr", "staged"):
        out_k, used_k = _solve(ctx, lu, X, n, m, kind)
        assert used_k == "csr" and np.array_equal(out_k, ref)
