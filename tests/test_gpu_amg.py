"""Smoothed-aggregation AMG on the device (csrc/amg_setup.cpp, k_amg.hip, mg.cpp; include/eigmi.h eig_amg_create)
against the numpy restatement tests/amg_ref.py, on matrices no box grid describes: the scrambled + reverse
Cuthill-McKee 7-point Poisson at 16^3 and 24^3, the variable-coefficient 7-point (kind 8) at 16^3 scrambled the same
way, and the variable-coefficient P1 stiffness (kind 9) at 12^3 as generated (a hierarchy from the matrix alone must
also work where a geometric one would).

Bars: the hierarchy (levels, rows and stored entries per level, the coarse degree) is the restatement's exactly --
the host setup sums in the restatement's order (tests/test_amg_aggregate.py holds the aggregates bitwise);
eig_mg_solve agrees with the restatement to 1e-12 relative to max|R| (tests/test_multigrid.py's bar: only the device's
rounding order differs) at m = 8, 24 and 32 columns and 1 and 6 cycles; B^T S_6 B is symmetric to 1e-13; the residual
after 8 cycles is within a factor 2 of the restatement's own.

The transfer kernels alone against scipy's P @ Xc and P^T @ Rf to 1e-14 relative to max|reference|, on guarded
buffers (tests/poison.py: NaN around the inputs, a sentinel around the outputs), with +Inf / NaN in panel rows chosen
so that rows which do not store them have a false address there (column 0, the last column, the row's own index), at
shapes with a ragged last wave (rows not a multiple of 16), more rows than one pass of the grid, and a one-row coarse
level."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

import amg_ref
import eigmi
import oracle
import poison

pytestmark = pytest.mark.gpu

THETA, NU, RATIO = 0.08, 2, 5.0
MATRICES = {"poisson16": (eigmi.GEN_POISSON3D, 16, True), "poisson24": (eigmi.GEN_POISSON3D, 24, True),
            "var7-16": (8, 16, True), "p1var-12": (9, 12, False)}


@functools.lru_cache(maxsize=None)
def _problem(name):
    """(K, restatement, B (n x 32), {cycles: restatement's S_cycles B})"""
    kind, N, scramble = MATRICES[name]
    rp, c, v = eigmi.gen_matrix(kind, N)
    if scramble:
        rp, c, v = eigmi.scrambled_rcm(rp, c, v)
    K = sp.csr_matrix((v, c, rp), shape=(rp.size - 1, rp.size - 1))
    ref = amg_ref.Amg(K, THETA, NU, RATIO)
    B = np.random.default_rng(N).standard_normal((K.shape[0], 32))
    return K, ref, B, {cycles: ref.solve(B, cycles) for cycles in (1, 6, 8)}


def _upload(ctx, A):
    A = A.tocsr()
    A.sort_indices()
    return eigmi.Matrix.from_bcsr(ctx, A.indptr.astype(np.int64), A.indices.astype(np.int32), A.data)


def _mv(ctx, X):
    return ctx.array(oracle.cols_to_mv(np.ascontiguousarray(X)))


def _cols(d, n, m):
    return oracle.mv_to_cols(d.get(), n, m)


@pytest.mark.parametrize("name", sorted(MATRICES))
def test_hierarchy_is_the_restatements(ctx, name):
    K, ref, _, _ = _problem(name)
    dK = _upload(ctx, K)
    mg = eigmi.Multigrid.amg(dK, THETA, max_cols=8, smooth_degree=NU, smooth_ratio=RATIO)
    info = mg.info()
    lev = [mg.level_info(l) for l in range(info["levels"])]
    print(f"amg {name}: rows {[L['rows'] for L in lev]}, nnz {[L['nnz'] for L in lev]}, complexity "
          f"{mg.complexity():.3f}, coarse degree {info['coarse_degree']}")
    assert info["levels"] == len(ref.levels) >= 2
    assert [L["rows"] for L in lev] == ref.rows() and [L["nnz"] for L in lev] == ref.nnz()
    assert [L["lmax"] for L in lev] == [L["lmax"] for L in ref.levels]
    assert info["coarse_rows"] == ref.rows()[-1] and info["coarse_degree"] == ref.levels[-1]["cdeg"]
    assert info["lmax_fine"] == ref.levels[0]["lmax"] and mg.complexity() == ref.complexity()
    with pytest.raises(eigmi.EigError) as e:
        mg.level_info(info["levels"])
    assert e.value.code == eigmi.EIG_ERR_ARG
    mg.close()
    dK.close()


@pytest.mark.parametrize("m", [8, 24, 32])
@pytest.mark.parametrize("name", sorted(MATRICES))
def test_solve_matches_restatement(ctx, name, m):
    K, ref, B32, R32 = _problem(name)
    n = K.shape[0]
    dK = _upload(ctx, K)
    mg = eigmi.Multigrid.amg(dK, THETA, max_cols=32, smooth_degree=NU, smooth_ratio=RATIO)
    B = np.ascontiguousarray(B32[:, :m])
    dB, dX = _mv(ctx, B), ctx.zeros(n * m)
    for cycles in (1, 6):
        mg.solve(m, dB, dX, cycles)
        X, R = _cols(dX, n, m), R32[cycles][:, :m]
        dev = np.abs(X - R).max() / np.abs(R).max()
        print(f"amg {name} m={m} cycles={cycles}: |X - R|.max() / |R|.max() = {dev:.2e}")
        assert np.all(np.isfinite(X)) and dev <= 1e-12, (cycles, dev)
    mg.close()
    dK.close()


@pytest.mark.parametrize("name", sorted(MATRICES))
def test_symmetric_and_converges_like_the_restatement(ctx, name):
    K, ref, B32, R32 = _problem(name)
    n, m = K.shape[0], 8
    dK = _upload(ctx, K)
    mg = eigmi.Multigrid.amg(dK, THETA, max_cols=8, smooth_degree=NU, smooth_ratio=RATIO)
    B = np.ascontiguousarray(B32[:, :m])
    dB, dX = _mv(ctx, B), ctx.zeros(n * m)
    mg.solve(m, dB, dX, 6)
    G = B.T @ _cols(dX, n, m)
    asym = np.abs(G - G.T).max() / np.abs(G).max()
    r8 = mg.solve(m, dB, dX, 8, resid=True)
    Rr = B - K @ R32[8][:, :m]
    ref8 = (np.linalg.norm(Rr, axis=0) / np.linalg.norm(B, axis=0)).max()
    print(f"amg {name}: |G - G^T| / |G| = {asym:.2e}; residual after 8 cycles {r8:.3e} (restatement {ref8:.3e})")
    assert np.all(np.isfinite(G)) and asym <= 1e-13
    assert ref8 < 1e-4  # (the restatement itself contracts: about 0.3 per cycle)
    assert 0.5 * ref8 <= r8 <= 2.0 * ref8
    mg.close()
    dK.close()


def test_refusals(ctx):
    def code(f):
        with pytest.raises(eigmi.EigError) as e:
            f()
        return e.value, e.value.code

    K = _problem("poisson16")[0]
    dK = _upload(ctx, K)
    # theta above the 7-point stencil's strength 1/6: no strong entry, 4096 -> 4096, a status and not a loop
    err, c = code(lambda: eigmi.Multigrid.amg(dK, 0.2))
    assert c == eigmi.EIG_ERR_ARG and "4096 -> 4096" in str(err)
    assert code(lambda: eigmi.Multigrid.amg(dK, -0.1))[1] == eigmi.EIG_ERR_ARG
    assert code(lambda: eigmi.Multigrid.amg(dK, 0.08, max_cols=12))[1] == eigmi.EIG_ERR_ARG
    A = oracle.q1elast(3)
    dA = eigmi.Matrix.from_bcsr(ctx, A.rowptr, A.col, A.val, 3, 3)
    assert code(lambda: eigmi.Multigrid.amg(dA))[1] == eigmi.EIG_ERR_BLOCKSIZE
    R = eigmi.Matrix.from_bcsr(ctx, np.arange(9, dtype=np.int64), np.arange(8, dtype=np.int32), np.ones(8), 1, 1,
                               ncols_blocks=12)
    assert code(lambda: eigmi.Multigrid.amg(R))[1] == eigmi.EIG_ERR_ARG  # 8 x 12
    R.close()
    bad = K.copy().tolil()
    bad[7, 7] = -1.0
    dBad = _upload(ctx, bad.tocsr())
    assert code(lambda: eigmi.Multigrid.amg(dBad))[1] == eigmi.EIG_ERR_BREAKDOWN
    # a geometric hierarchy answers eig_mg_level_info as well
    Kg = oracle.p1_kuhn(12)[0]
    dKg = _upload(ctx, Kg)
    g = eigmi.Multigrid(dKg, (12, 12, 12), max_cols=8)
    assert [g.level_info(l)["rows"] for l in range(g.info()["levels"])] == [1728, 216, 27]
    assert g.level_info(0)["nnz"] == Kg.nnz and g.level_info(0)["lmax"] == g.info()["lmax_fine"]
    for h in (g, dKg, dBad, dA, dK):
        h.close()


# ------------------------------------------------------------------------------------- transfers
def _random_op(nrows, ncols, per_row, seed):
    """nrows x ncols CSR, 1 .. per_row distinct ascending columns per row (row 3 empty when there is one)."""
    rng = np.random.default_rng(seed)
    rp, col = [0], []
    for i in range(nrows):
        k = 0 if i == 3 else int(rng.integers(1, min(per_row, ncols) + 1))
        col.extend(sorted(rng.choice(ncols, size=k, replace=False).tolist()))
        rp.append(len(col))
    return sp.csr_matrix((rng.uniform(-1.0, 1.0, len(col)), np.asarray(col, np.int32), np.asarray(rp, np.int64)),
                         shape=(nrows, ncols))


@functools.lru_cache(maxsize=None)
def _operators():
    """name -> (P, whether a poison set is asked for).  Real prolongators (level 0: 4096 x 513, level 1: 513 x 66,
    513 = 32 * 16 + 1) and synthetic shapes: ragged rows, 70,001 rows (more than one pass of the capped grid at
    m = 32 would need 262,144; more than one workgroup row range anyway), a one-row coarse level."""
    ref = _problem("poisson16")[1]
    return {"P0": (ref.levels[0]["P"], True), "P1": (ref.levels[1]["P"], True),
            "ragged-1003x77": (_random_op(1003, 77, 9, 1), True), "wide-77x1003": (_random_op(77, 1003, 40, 2), True),
            "long-70001x300": (_random_op(70001, 300, 5, 3), True),
            "one-coarse-row-37x1": (sp.csr_matrix(np.linspace(0.5, 1.5, 37)[:, None]), False)}


def _poison_rows(Op, want):
    """Panel rows (columns of Op) to poison: tests/poison.py's greedy set for the false addresses of a gather on
    explicit columns -- column 0, the last column, the row's own index -- capped at a fifth of the rows tainted."""
    if not want:
        return np.zeros(0, np.int64)
    A = oracle.CSR(Op.shape[0], Op.indptr.astype(np.int64), Op.indices.astype(np.int32), Op.data)
    fa = poison.false_addresses(A, "sell", sell=True, ncols=Op.shape[1])
    return poison.poison_set(A, fa, ncols=Op.shape[1], want=4)


def _transfer(ctx, Op, m, add, seed):
    Op = sp.csr_matrix(Op)
    Op.sort_indices()
    nr, nc = Op.shape
    rng = np.random.default_rng(seed)
    Xin, X0 = rng.standard_normal((nc, m)), rng.standard_normal((nr, m))
    return Op, nr, nc, Xin, X0


@pytest.mark.parametrize("m", [8, 32])
@pytest.mark.parametrize("direction", ["prolong", "restrict"])
@pytest.mark.parametrize("name", ["P0", "P1", "ragged-1003x77", "wide-77x1003", "long-70001x300", "one-coarse-row-37x1"])
def test_transfer_kernels(ctx, name, direction, m):
    P, want_poison = _operators()[name]
    add = direction == "prolong"
    Op, nr, nc, Xin, X0 = _transfer(ctx, P if add else P.T.tocsr(), m, add, len(name) + m)
    J = _poison_rows(Op, want_poison)
    Xin[J, :] = poison.poison_values(len(J))[:, None]  # +Inf, NaN, +Inf, ... in every column of those panel rows
    with np.errstate(invalid="ignore"):
        ref = Op @ Xin
        if add:
            ref = X0 + ref
    stores_poison = np.zeros(nr, bool)
    stores_poison[np.repeat(np.arange(nr), np.diff(Op.indptr))[np.isin(Op.indices, J)]] = True
    assert np.array_equal(~np.isfinite(ref).all(axis=1), stores_poison)
    if want_poison:
        assert 0 < stores_poison.mean() <= 0.25, stores_poison.mean()
    din = poison.guarded(ctx, oracle.cols_to_mv(Xin))
    dout = poison.Guarded(ctx, nr * m, 512, poison.SENTINEL, host=oracle.cols_to_mv(X0) if add else None)
    eigmi.amg_transfer_mv8(ctx, Op.indptr, Op.indices, Op.data, nc, m, din, dout, add=add)
    whole = dout.whole()
    got = oracle.mv_to_cols(dout.payload(whole), nr, m)
    assert din.intact()
    assert poison.untouched(whole, dout.outside(slice(0, nr * m)))  # nothing but the rows of the output written
    fin = np.isfinite(ref)
    assert np.array_equal(np.isfinite(got), fin), "a poisoned panel row reached (or missed) a row's sum"
    err = np.abs(got[fin] - ref[fin]).max() / np.abs(ref[fin]).max()
    print(f"amg {direction} {name} m={m}: {nr} x {nc}, {len(J)} poisoned panel rows, {int(stores_poison.sum())} rows "
          f"store one; max |got - ref| / max|ref| = {err:.1e}, bitwise {np.array_equal(got[fin], ref[fin])}")
    assert err <= 1e-14
    din.free()
    dout.free()


def test_transfer_refusals(ctx):
    P = _operators()["ragged-1003x77"][0]
    din, dout = ctx.zeros(77 * 8), ctx.zeros(1003 * 8)
    bad = P.indices.copy()
    bad[5] = 77
    with pytest.raises(eigmi.EigError) as e:
        eigmi.amg_transfer_mv8(ctx, P.indptr, bad, P.data, 77, 8, din, dout)
    assert e.value.code == eigmi.EIG_ERR_SHAPE
    with pytest.raises(eigmi.EigError) as e:
        eigmi.amg_transfer_mv8(ctx, P.indptr, P.indices, P.data, 77, 12, din, dout)
    assert e.value.code == eigmi.EIG_ERR_ARG
