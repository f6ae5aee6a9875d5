"""eig_amg_aggregate (csrc/amg_setup.cpp through the C ABI, host-only) returns exactly the aggregates of the numpy
restatement tests/amg_ref.py -- the same three passes written down twice -- on a scrambled 12^3 Poisson matrix, a
2-D 5-point 24^2, the variable-coefficient P1 stiffness (kind 9) at N = 8 and a matrix with an isolated diagonal
row; and the restatement's hierarchy is what DESIGN.md 4d says it is."""
import numpy as np
import pytest
import scipy.sparse as sp

import amg_ref
import eigmi


def _scipy(rp, c, v):
    return sp.csr_matrix((v, c, rp), shape=(rp.size - 1, rp.size - 1))


def _isolated():
    """A 2-D 5-point 9^2 whose row 40 is cut off (its diagonal only), theta_l above some of its varying entries."""
    rp, c, v = eigmi.gen_matrix(eigmi.GEN_LAPLACE2D, 9)
    A = _scipy(rp, c, v).tolil()
    rng = np.random.default_rng(5)
    for i, j in zip(*sp.triu(A, 1).nonzero()):
        A[i, j] = A[j, i] = -rng.uniform(0.2, 1.0)
    for j in A.rows[40][:]:
        if j != 40:
            A[40, j] = 0.0
            A[j, 40] = 0.0
    A = A.tocsr()
    A.eliminate_zeros()
    A.sort_indices()
    assert A.indptr[41] - A.indptr[40] == 1
    return A.indptr.astype(np.int64), A.indices.astype(np.int32), A.data


CASES = {
    "poisson12-scrambled": lambda: eigmi.scrambled_rcm(*eigmi.gen_matrix(eigmi.GEN_POISSON3D, 12)),
    "laplace2d-24": lambda: eigmi.gen_matrix(eigmi.GEN_LAPLACE2D, 24),
    "p1var-8": lambda: eigmi.gen_matrix(9, 8),
    "isolated-row": _isolated,
}


@pytest.mark.parametrize("name", sorted(CASES))
@pytest.mark.parametrize("theta", [0.08, 0.02, 0.2])
def test_aggregate_equals_restatement(name, theta):
    rp, c, v = CASES[name]()
    agg, na = eigmi.amg_aggregate(rp, c, v, theta)
    ref, nref = amg_ref.aggregate(rp, c, v, theta)
    n = rp.size - 1
    print(f"{name} theta {theta}: {n} rows -> {na} aggregates")
    assert na == nref and np.array_equal(agg, ref)
    assert agg.min() == 0 and agg.max() == na - 1 and np.unique(agg).size == na  # every row in one, none empty
    if name == "isolated-row":
        assert np.count_nonzero(agg == agg[40]) == 1


def test_aggregate_refusals():
    rp, c, v = eigmi.gen_matrix(eigmi.GEN_LAPLACE2D, 6)
    bad = v.copy()
    bad[np.nonzero(c[rp[7]:rp[8]] == 7)[0][0] + rp[7]] = 0.0
    with pytest.raises(eigmi.EigError) as e:
        eigmi.amg_aggregate(rp, c, bad, 0.08)
    assert e.value.code == eigmi.EIG_ERR_BREAKDOWN
    with pytest.raises(eigmi.EigError) as e:
        eigmi.amg_aggregate(rp, c, v, -1.0)
    assert e.value.code == eigmi.EIG_ERR_ARG
    cc = c.copy()
    cc[3] = 36
    with pytest.raises(eigmi.EigError) as e:
        eigmi.amg_aggregate(rp, cc, v, 0.08)
    assert e.value.code == eigmi.EIG_ERR_SHAPE


def test_restatement_hierarchy():
    """The restatement on the scrambled 16^3 Poisson matrix: three levels, each coarse operator P^T A P to rounding
    and bitwise symmetric, theta halved per level (a constant theta stalls on the second level), theta above 1/6
    refused, and the V-cycle contracts (below 0.1 after one cycle, below 0.35 per cycle after that; unsmoothed
    aggregation: above 0.5 per cycle)."""
    rp, c, v = eigmi.scrambled_rcm(*eigmi.gen_matrix(eigmi.GEN_POISSON3D, 16))
    A = _scipy(rp, c, v)
    mg = amg_ref.Amg(A, 0.08, 2, 5.0)
    rows = mg.rows()
    assert len(rows) == 3 and rows[0] == 4096 and rows[2] <= 256 and mg.complexity() < 1.8, (rows, mg.complexity())
    for f, g in zip(mg.levels[:-1], mg.levels[1:]):
        G = (f["P"].T @ f["A"] @ f["P"]).toarray()
        assert np.abs(g["A"].toarray() - G).max() <= 1e-14 * np.abs(G).max()
        assert (g["A"] != g["A"].T).nnz == 0
    # constant theta on the second level: less than a factor 2
    _, nc1 = amg_ref.aggregate(mg.levels[1]["A"].indptr, mg.levels[1]["A"].indices, mg.levels[1]["A"].data, 0.08)
    _, nc1h = amg_ref.aggregate(mg.levels[1]["A"].indptr, mg.levels[1]["A"].indices, mg.levels[1]["A"].data, 0.04)
    print("level 1:", rows[1], "rows ->", nc1, "aggregates at theta 0.08,", nc1h, "at 0.04")
    assert nc1h == rows[2] and nc1 > nc1h
    with pytest.raises(ValueError):
        amg_ref.Amg(A, 0.2)
    B = np.random.default_rng(0).standard_normal((4096, 2))
    nb = np.linalg.norm(B, axis=0)
    r = [(np.linalg.norm(B - A @ mg.solve(B, k), axis=0) / nb).max() for k in (1, 6, 8)]
    plain = amg_ref.Amg(A, 0.08, 2, 5.0, smoothed=False)
    q = [(np.linalg.norm(B - A @ plain.solve(B, k), axis=0) / nb).max() for k in (6, 8)]
    print("residual after 1 / 6 / 8 cycles:", r, "per cycle", (r[2] / r[1]) ** 0.5, "| unsmoothed P per cycle",
          (q[1] / q[0]) ** 0.5)
    assert r[0] < 0.1 and (r[2] / r[1]) ** 0.5 < 0.35 < 0.5 < (q[1] / q[0]) ** 0.5
