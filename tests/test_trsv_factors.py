"""The factor sets of tests/test_gpu_trsv_factors.py on the CPU (tests/lu_factors.py builds them).

The device result of eig_inverse_mv8 is compared bitwise with oracle.inverse_mv8, so the oracle
itself is anchored here on every one of those sets, independently of it: in numpy.longdouble its
output y satisfies the backward-error bound of two substitutions plus the row scaling,
    |L (U y) - b| <= (w_L + w_U + 3) 2^-53 |L| |U| |y| + 2^-53 |b|      (elementwise)
(w: the largest stored row width; derived, not measured -- the oracle alone reaches at most 0.24
of it).  The generator's own promises and the kernel each case expects from the device are checked
against Python restatements of the upload's admission rules."""
import numpy as np
import pytest

import lu_factors as F
import oracle


@pytest.mark.parametrize("name", sorted(F.CASES) + sorted(F.EXTRA))
def test_oracle_residual_bound(name):
    d, X, m, ref = F.case(name)
    assert np.all(np.isfinite(ref))
    ratio = F.residual_ratio(d, X, ref, m)
    print(f"{name}: oracle residual / bound {ratio:.3f}")
    assert ratio <= 1.0


def test_residual_bound_has_teeth():
    """One entry of the result off by 1e-12 relative, or one factor entry ignored, breaks the bound."""
    d, X, m, ref = F.case("staged_dist4")
    out = ref.copy()
    k = int(np.argmax(np.abs(out)))
    out[k] *= 1 + 1e-12
    assert F.residual_ratio(d, X, out, m) > 1.0
    d2 = dict(d, Lx=d["Lx"].copy())
    d2["Lx"][int(d["Lp"][-2])] = 0.0  # the first entry of the last row (4 blocks back)
    assert d["Lp"][-1] - d["Lp"][-2] > 1
    out2, _ = oracle.inverse_mv8(oracle.LU(**d2), X, m)
    assert F.residual_ratio(d, X, out2, m) > 1.0


@pytest.mark.parametrize("name", sorted(F.CASES))
def test_factor_form_and_expected_kernel(name):
    """The exported form (umfpacktools.hh contract), contractivity, and the kernel the GPU test
    asserts: F.expected_solver restates the admission rules of trsv_upload."""
    d, _, _, _ = F.case(name)
    kw, expect = F.CASES[name]["kw"], F.CASES[name]["expect"]
    n = d["Lp"].size - 1
    assert n == kw["n"]
    assert np.array_equal(d["Lj"][d["Lp"][1:] - 1], np.arange(n)) and np.all(d["Lx"][d["Lp"][1:] - 1] == 1.0)
    assert np.array_equal(d["Ui"][d["Up"][1:] - 1], np.arange(n))
    L, U = F.dense_factors(d)
    assert np.all(np.triu(L, 1) == 0) and np.all(np.tril(U, -1) == 0)
    assert np.all(np.abs(np.tril(L, -1)).sum(1) <= 0.5 * (1 + 1e-12))
    assert np.all(np.abs(np.triu(U, 1)).sum(1) <= 0.5 * np.abs(np.diag(U)) * (1 + 1e-12))
    assert sorted(d["P"]) == list(range(n)) and sorted(d["Q"]) == list(range(n))
    assert n == 1 or not np.array_equal(d["P"], d["Q"])
    assert d["Rs"].min() >= 0.5 and d["Rs"].max() <= 2.0
    assert F.expected_solver(d) == expect
    est = F.gate_estimate(d)
    if expect[0] == "blockinv":
        assert est <= 256.0  # pivots in [1, 2], contractive: max |D| <= 2, max |inv D| <= 2
    elif name != "csr_9_1" and not name.startswith("csr_reach9"):
        # refused by the pivots, whatever the other entries (n = 1: 64 * 1 * 1e5, the 1 from the padding)
        assert est >= (6.4e6 if n == 1 else 6.4e7) * (1 - 1e-12) > F.BINV_COND


def test_crafted_rows_are_what_they_claim():
    def l_outside(d, i):
        c = d["Lj"][d["Lp"][i]:d["Lp"][i + 1] - 1]
        return c[c // F.TB != i // F.TB]

    def u_outside(d, i):
        c = np.repeat(np.arange(d["Up"].size - 1), np.diff(d["Up"]))[d["Ui"] == i]
        return c[c // F.TB != i // F.TB]

    d = F.case("staged_widths")[0]
    for r, w in enumerate((0, 1, 7, 8, 9, 120, 127, 128)):
        assert l_outside(d, 4 * F.TB + r).size == w and u_outside(d, F.TB + r).size == w
    d = F.case("staged_width0_block")[0]
    assert all(l_outside(d, i).size == 0 and u_outside(d, i).size == 0 for i in range(3 * F.TB, 4 * F.TB))
    assert l_outside(d, 4 * F.TB).size == 128 and u_outside(d, 2 * F.TB).size == 128
    d = F.case("staged_dist4")[0]
    n = d["Lp"].size - 1
    for i in range(n):
        assert np.all(i // F.TB - l_outside(d, i) // F.TB == 4) and np.all(u_outside(d, i) // F.TB - i // F.TB == 4)
    d = F.case("staged_dist_mix")[0]
    dl = np.concatenate([i // F.TB - l_outside(d, i) // F.TB for i in range(d["Lp"].size - 1)])
    assert set(dl) == {1, 2, 3, 4}
    d = F.case("csr_reach9_m8")[0]
    for base, lo in ((8 * F.TB, l_outside), (0, u_outside)):
        for r, w in ((1, 31), (2, 32), (3, 33), (4, 65)):
            c = lo(d, base + r)
            near = np.abs(c // F.TB - base // F.TB) <= 3
            assert c.size == w and 0 < near.sum() < w  # ring and global reads in one row
    assert l_outside(d, 9).size == 0 and d["Lp"][10] - d["Lp"][9] == 1  # an empty row
    d = F.case("staged_l_descending")[0]
    c = d["Lj"][d["Lp"][-2]:d["Lp"][-1] - 1]
    assert c.size > 1 and np.all(np.diff(c) < 0)
    d = F.case("staged_u_shuffled")[0]
    asc = [np.all(np.diff(d["Ui"][d["Up"][j]:d["Up"][j + 1] - 1]) > 0) for j in range(d["Up"].size - 1)]
    assert not all(asc)
