"""GPU tests of the spectrum-slicing solver: the fused filter step (eig_filter_step_mv8) on every kernel that
carries its epilogue, against the numpy restatement (tests/slice_ref.py); stored entries only (poison at the
false addresses, tests/poison.py); the whole filter at degree 80; the driver end to end on the cases fixed by
tests/test_slice_ref.py; eig_spectrum_bounds and eig_filter_count.

The driver's box-image case is kind 8 at N = 16, not N = 10: the box kernels need a grid of at least
16 x 8 x 3 rows, so the 10^3 grid runs on the SELL kernels whatever the flags (tests/test_slice_ref.py)."""
import numpy as np
import pytest

import blk_grids
import box_grids
import eigmi
import oracle
import poison
import slice_ref as sr
from test_slice_ref import CASES, DEGREE, LMAX, LMIN, MAX_ITERS, SATURATED, TOL, check_eigenvalues, matrix, window

STEP_TOL = 1e-12
SCALARS = (0.3125, -0.71, -1.0, 0.113)  # s1, s0, s2, g of the general step (no value special to any term)


def upload(ctx, A, flags=0):
    return eigmi.Matrix.from_bcsr(ctx, A.rowptr, A.col, A.val, A.br, A.bc, flags=flags)


def kernel_at(M, m):
    """The kernel eig_mat_kernel_info names for the filter step at m columns: "filt8" is the m = 8 launch,
    "filt32" the m % 32 == 0 one; it names no other width (None)."""
    return M.kernel("filt8") if m == 8 else M.kernel("filt32") if m % 32 == 0 else None


def step_check(ctx, M, S, m, want, seed=5):
    """One fused step on M against the restatement on the scipy matrix S: the general step, then the
    s2 = 0 flavour on an output buffer full of NaN (it must not be read).  want: the kernel named for this
    width (m = 8 or m % 32 == 0), or None for a width in between."""
    n = S.shape[0]
    assert M.info.n == n and kernel_at(M, m) == want, (kernel_at(M, m), want)
    rng = np.random.default_rng(seed + m)
    Xk, Xo, B = (rng.standard_normal((n, m)) for _ in range(3))
    dXk, dB = ctx.array(oracle.cols_to_mv(Xk)), ctx.array(oracle.cols_to_mv(B))
    dXo = ctx.array(oracle.cols_to_mv(Xo))
    s1, s0, s2, g = SCALARS
    eigmi.filter_step_mv8(M, m, dXk, dXo, dB, s1, s0, s2, g)
    got = oracle.mv_to_cols(dXo.get(), n, m)
    ref = sr.filt_step(S, Xk, Xo, B, s1, s0, s2, g)
    err = np.abs(got - ref).max()
    print(f"[filt] {want or M.kernel('filt32')} n {n} m {m}: step error {err:.3e} of {np.abs(ref).max():.3e}")
    assert err <= STEP_TOL * np.abs(ref).max()
    dXo.upload(np.full(n * m, np.nan))
    eigmi.filter_step_mv8(M, m, dXk, dXo, dB, s1, s0, 0.0, g)
    got = oracle.mv_to_cols(dXo.get(), n, m)
    ref = sr.filt_step(S, Xk, None, B, s1, s0, 0.0, g)
    assert np.isfinite(got).all(), "the s2 = 0 flavour read its output buffer"
    assert np.abs(got - ref).max() <= STEP_TOL * np.abs(ref).max()
    assert np.array_equal(dXk.get(), oracle.cols_to_mv(Xk)) and np.array_equal(dB.get(), oracle.cols_to_mv(B))
    for d in (dXk, dXo, dB):
        d.free()


# ---- one step ----

@pytest.mark.gpu
def test_step_sell_explicit_columns(ctx):
    """SELL forced (EIG_MAT_NO_MARCH), kind 8 at N = 9 scrambled + RCM: 729 rows = 11 slices and a 25-row tail,
    explicit columns; m = 8 (k_sell_mv8g), 24 and 32 (k_sell_mv8q with 3 and 4 column blocks)."""
    rp, c, v = eigmi.gen_matrix(eigmi.GEN_VARCOEF3D, 9)
    rp, c, v = eigmi.scrambled_rcm(rp, c, v, 123)
    A = oracle.CSR(rp.size - 1, rp, c, v)
    M = upload(ctx, A, flags=eigmi.MAT_NO_MARCH)
    info = M.info
    assert info.n == 729 and info.nslices == 12 and info.stencil_slices < info.nslices
    S = A.to_scipy().tocsr()
    # (m = 16 and 24 are k_sell_mv8q launches of 2 and 3 column blocks: no op of eig_mat_kernel_info names them)
    for m, want in ((8, "k_sell_mv8g_filt"), (16, None), (24, None), (32, "k_sell_mv8q_filt")):
        step_check(ctx, M, S, m, want)
    M.close()


@pytest.mark.gpu
def test_step_sell_tiny(ctx):
    """SELL forced, kind 8 at N = 3: 27 rows < one 64-row slice (a stencil slice: the mask path)."""
    rp, c, v = eigmi.gen_matrix(eigmi.GEN_VARCOEF3D, 3)
    A = oracle.CSR(rp.size - 1, rp, c, v)
    M = upload(ctx, A, flags=eigmi.MAT_NO_MARCH)
    assert M.info.n == 27 and M.info.nslices == 1
    S = A.to_scipy().tocsr()
    step_check(ctx, M, S, 8, "k_sell_mv8g_filt")
    step_check(ctx, M, S, 32, "k_sell_mv8q_filt")
    M.close()


@pytest.mark.gpu
@pytest.mark.parametrize("values", ["const", "edge"])
@pytest.mark.parametrize("dims,shape", [((33, 9, 4), "p7"), ((16, 23, 5), "kuhn15"), ((40, 8, 3), "nine")],
                         ids=["33x9x4-p7", "16x23x5-kuhn15", "40x8x3-nine"])
def test_step_box(ctx, dims, shape, values):
    """Non-cubic grids of tests/box_grids.py (sizes of tests/test_gpu_box_noncubic.py): constant values on the
    row-class kernel (m = 8, 16, 32), one value per edge on the box image (m = 32: k_box_mv32, and with
    EIG_TUNE_BOX_COLS = 16 the two 16-column halves of k_box_mv16p; m = 8 has no box-image kernel and takes
    k_sell_mv8g).  "nine" is the runtime-offset form of all three kernels."""
    A = box_grids.box_matrix(dims, shape, values, seed=sum(dims) + 3)
    S = box_grids.to_scipy(A)
    M = upload(ctx, A)
    if values == "const":
        for m in (8, 16, 32):
            step_check(ctx, M, S, m, None if m == 16 else "k_boxc_mv8_filt")
    else:
        step_check(ctx, M, S, 8, "k_sell_mv8g_filt")
        step_check(ctx, M, S, 32, "k_box_mv32_filt")
        step_check(ctx, M, S, 64, "k_box_mv32_filt")
        M.tune(box_cols=16)
        step_check(ctx, M, S, 32, "k_box_mv16p_filt")
        M.tune(box_cols=0)
    M.close()


@pytest.mark.gpu
@pytest.mark.parametrize("b", [2, 3, 4])
def test_step_blocked(ctx, b):
    """Blocks b = 2, 3, 4 of tests/blk_grids.py on 9 x 5 x 4 nodes (180 block rows: two slices and a tail),
    m = 8 and 24 (one and two workgroup rows of column blocks at b = 4)."""
    A, S = blk_grids.blk_matrix((9, 5, 4), b, seed=b)
    M = upload(ctx, A)
    assert M.info.br == b
    assert M.kernel("filt8") == M.kernel("filt32") == "k_spmm_blk_mv8_filt"
    for m in (8, 24):
        step_check(ctx, M, S, m, "k_spmm_blk_mv8_filt" if m == 8 else None)
    M.close()


# ---- stored entries only ----

def poison_check(ctx, M, A, S, J, m, note):
    """The step with +Inf / NaN in Xk at the (block) rows J, columns 3 and m - 3: a row is reached when it stores a
    column of J (its own entry is such a column: every row here stores its diagonal).  Reached entries come out
    non-finite, every other entry bitwise as in the clean run -- a false address in the sum would show as NaN."""
    n = S.shape[0]
    rng = np.random.default_rng(17)
    Xc, Xo, B = (rng.standard_normal((n, m)) for _ in range(3))
    cols = (3, m - 3)
    rows = np.asarray(J) * A.bc + (A.bc - 1)
    Xp = Xc.copy()
    for col in cols:
        Xp[rows, col] = poison.poison_values(rows.size)
    reached = np.zeros((n, m), bool)
    t = np.repeat(poison.tainted_rows(A, set(J.tolist())), A.br)
    for col in cols:
        reached[t, col] = True
    assert 0 < t.mean() <= 0.3
    dB = ctx.array(oracle.cols_to_mv(B))
    got = {}
    for key, X in (("clean", Xc), ("poisoned", Xp)):
        dX = poison.guarded(ctx, oracle.cols_to_mv(X))
        dO = poison.guarded(ctx, oracle.cols_to_mv(Xo))
        eigmi.filter_step_mv8(M, m, dX.vec, dO.vec, dB, *SCALARS)
        whole = dO.whole()
        assert np.array_equal(whole.view(np.uint64)[dO.outside(slice(0, n * m))],
                              dO.image.view(np.uint64)[dO.outside(slice(0, n * m))]), (note, "write outside the panel")
        assert dX.intact(), (note, "Xk written")
        got[key] = oracle.mv_to_cols(dO.payload(whole).copy(), n, m)
        dX.free()
        dO.free()
    dB.free()
    gc, gp = got["clean"], got["poisoned"]
    ref = sr.filt_step(S, Xc, Xo, B, *SCALARS)
    assert np.isfinite(gc).all() and np.abs(gc - ref).max() <= STEP_TOL * np.abs(ref).max()
    assert np.array_equal(gp[~reached].view(np.uint64), gc[~reached].view(np.uint64)), \
        (note, "poison outside the rows that store it", np.argwhere(~reached & ~np.isfinite(gp))[:8].tolist())
    assert not np.isfinite(gp[reached]).any(), (note, "a row that stores a poisoned column came out finite")
    print(f"[filt] poison {note}: |J| = {len(J)}, {int(t.sum())} of {n} rows reached")


@pytest.mark.gpu
@pytest.mark.parametrize("kernel", ["k_sell_mv8q_filt", "k_box_mv32_filt", "k_boxc_mv8_filt"])
def test_step_reads_stored_entries_only(ctx, kernel):
    """The 33 x 9 x 4 grid (7-point): the SELL kernel (EIG_MAT_NO_MARCH), the box-image kernel (one value per
    edge) and the row-class kernel (constant values); poison at the clamped positions of the neighbours a
    boundary row does not store, at column 0 and the last column (poison.false_addresses / poison_set)."""
    dims = (33, 9, 4)
    A = box_grids.box_matrix(dims, "p7", "const" if kernel == "k_boxc_mv8_filt" else "edge", seed=sum(dims) + 5)
    fa = poison.false_addresses(A, dims)
    if kernel == "k_sell_mv8q_filt":
        fa.update(poison.false_addresses(A, "sell", sell=True))
    J = poison.poison_set(A, fa)
    share, least, ok = poison.conditions(A, fa, J)
    assert ok, (share, least)
    M = upload(ctx, A, flags=eigmi.MAT_NO_MARCH if kernel == "k_sell_mv8q_filt" else 0)
    assert M.kernel("filt32") == kernel
    poison_check(ctx, M, A, box_grids.to_scipy(A), J, 32, kernel)
    M.close()


@pytest.mark.gpu
def test_step_blocked_reads_stored_entries_only(ctx):
    """k_spmm_blk_mv8_filt, b = 3 on 9 x 5 x 4 nodes: poison in the last component of the block columns J."""
    A, S = blk_grids.blk_matrix((9, 5, 4), 3, seed=3)
    fa = poison.false_addresses(A, "sell", sell=True)
    J = poison.poison_set(A, fa, A.nrows)
    M = upload(ctx, A)
    assert M.kernel("filt8") == "k_spmm_blk_mv8_filt"
    poison_check(ctx, M, A, S, J, 24, "k_spmm_blk_mv8_filt")
    M.close()


# ---- the whole filter ----

def filter_check(ctx, M, S, m, a, b, lmin, lmax, want):
    n = S.shape[0]
    assert kernel_at(M, m) == want
    X = np.random.default_rng(m).standard_normal((n, m))
    dX, dY, dW = ctx.array(oracle.cols_to_mv(X)), ctx.zeros(n * m), ctx.zeros(n * m)
    eigmi.filter_mv8(M, m, a, b, lmin, lmax, DEGREE, dX, dY, dW)
    got = oracle.mv_to_cols(dY.get(), n, m)
    ref = sr.apply_filter(S, X, a, b, lmin, lmax, DEGREE)
    err = np.abs(got - ref).max()
    print(f"[filt] {want} filter degree {DEGREE}: error {err:.3e} of {np.abs(ref).max():.3e}")
    assert err <= STEP_TOL * np.abs(ref).max()
    assert np.array_equal(dX.get(), oracle.cols_to_mv(X))
    for d in (dX, dY, dW):
        d.free()


@pytest.mark.gpu
def test_filter_sell(ctx):
    A, S, lam = matrix("var10")
    M = upload(ctx, A, flags=eigmi.MAT_NO_MARCH)
    a, b = window(lam, *CASES["var10"][:2])
    filter_check(ctx, M, S, 24, a, b, LMIN, LMAX, None)  # (the driver case's width: k_sell_mv8q, 3 column blocks)
    filter_check(ctx, M, S, 8, a, b, LMIN, LMAX, "k_sell_mv8g_filt")
    M.close()


@pytest.mark.gpu
def test_filter_box(ctx):
    dims = (33, 9, 4)
    A = box_grids.box_matrix(dims, "p7", "edge", seed=11)
    S = box_grids.to_scipy(A)
    M = upload(ctx, A)
    hi = float(np.abs(S).sum(axis=1).max())  # Gershgorin
    filter_check(ctx, M, S, 32, 0.30 * hi, 0.36 * hi, 0.0, hi, "k_box_mv32_filt")
    M.close()


@pytest.mark.gpu
def test_filter_blocked(ctx):
    A, S, lam = matrix("q1elast6")
    M = upload(ctx, A)
    a, b = window(lam, *CASES["q1elast6"][:2])
    filter_check(ctx, M, S, 8, a, b, LMIN, LMAX, "k_spmm_blk_mv8_filt")
    M.close()


# ---- the driver ----

_REF = {}


def reference_run(name):
    if name not in _REF:
        _, S, lam = matrix(name)
        i0, cnt, block = CASES[name]
        a, b = window(lam, i0, cnt)
        X0 = oracle.mv_to_cols(oracle.random_mv8(lam.size, block, 123), lam.size, block)
        _REF[name] = sr.slice_solve(S, X0, a, b, LMIN, LMAX, DEGREE, TOL, MAX_ITERS)
    return _REF[name]


DRIVER = {"var10": (eigmi.MAT_NO_MARCH, "k_sell_mv8q_filt"), "var16": (0, "k_box_mv32_filt"),
          "q1elast6": (0, "k_spmm_blk_mv8_filt")}


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_driver(ctx, name):
    A, S, lam = matrix(name)
    i0, cnt, block = CASES[name]
    a, b = window(lam, i0, cnt)
    flags, want = DRIVER[name]
    M = upload(ctx, A, flags=flags)
    assert M.kernel("filt32") == want
    ref = reference_run(name)
    assert ref["converged"]
    sl = eigmi.Slice(M, a, b, LMIN, LMAX, block=block, degree=DEGREE, seed=123)
    it, conv, t = sl.step(MAX_ITERS, TOL)
    print(f"[slice] {name}: {it} iterations (restatement {ref['iters']}), in window {t.in_window}, "
          f"filter {t.filter_ms:.2f} ms orth {t.orth_ms:.2f} rr {t.rr_ms:.2f} resid {t.resid_ms:.2f}")
    assert conv and abs(it - ref["iters"]) <= 1 and it <= MAX_ITERS
    assert t.iters == it and t.degree == DEGREE and t.in_window == cnt and t.saturated == 0
    ev, X, res = sl.ritz(want_evec=True, want_resid=True)
    check_eigenvalues(ev, lam, i0, cnt, a, b)
    assert np.all(np.diff(ev) >= 0)
    X = X.T  # (n, count)
    host = np.linalg.norm(S @ X - X * ev, axis=0)
    print("[slice] residuals", res.max(), "host", host.max())
    assert np.abs(res - host).max() <= 1e-12 * LMAX
    assert np.all(res <= TOL * np.maximum(np.abs(ev), max(abs(a), abs(b))) * (1.0 + 1e-4))  # (fresh products)
    assert np.abs(X.T @ X - np.eye(cnt)).max() <= 1e-12
    # a converged workspace takes no further iteration
    it2, conv2, _ = sl.step(MAX_ITERS, TOL)
    assert it2 == 0 and conv2
    sl.close()
    M.close()


@pytest.mark.gpu
def test_driver_saturates_on_a_small_block(ctx):
    name, i0, cnt, block = SATURATED
    A, S, lam = matrix(name)
    a, b = window(lam, i0, cnt)
    M = upload(ctx, A, flags=eigmi.MAT_NO_MARCH)
    sl = eigmi.Slice(M, a, b, LMIN, LMAX, block=block, degree=DEGREE, seed=123)
    it, conv, t = sl.step(6, 0.0)
    assert it == 6 and not conv and t.saturated == 1 and t.in_window == block < cnt
    ev, _, _ = sl.ritz(want_resid=False)
    assert ev.size == block and np.all((ev >= a) & (ev <= b))
    sl.close()
    M.close()


@pytest.mark.gpu
def test_driver_refusals(ctx):
    A, S, lam = matrix("var10")
    M = upload(ctx, A)
    for block in (0, 12, 40):
        with pytest.raises(eigmi.EigError) as e:
            eigmi.Slice(M, 1.0, 2.0, LMIN, LMAX, block=block)
        assert e.value.code == eigmi.EIG_ERR_ARG
    for a, b, d in ((2.0, 1.0, 80), (14.0, 15.0, 80), (1.0, 2.0, 1)):
        with pytest.raises(eigmi.EigError) as e:
            eigmi.Slice(M, a, b, LMIN, LMAX, block=8, degree=d)
        assert e.value.code == eigmi.EIG_ERR_ARG
    M.close()
    rp, c, v = eigmi.gen_matrix(eigmi.GEN_VARCOEF3D, 3)
    Ms = eigmi.Matrix.from_bcsr(ctx, rp, c, v)
    with pytest.raises(eigmi.EigShapeError) as e:  # 4 * block > n
        eigmi.Slice(Ms, 1.0, 2.0, LMIN, LMAX, block=8)
    assert e.value.code == eigmi.EIG_ERR_SHAPE
    x = ctx.zeros(27 * 8)
    with pytest.raises(eigmi.EigError) as e:  # the output buffer is x_k
        eigmi.filter_step_mv8(Ms, 8, x, x, x, 1.0, 0.0, 0.0, 0.0)
    assert e.value.code == eigmi.EIG_ERR_ARG
    Ms.close()
    R = oracle.CSR(4, np.array([0, 1, 2, 3, 4], np.int64), np.zeros(4, np.int32), np.ones(4 * 6), 2, 3)
    Mr = eigmi.Matrix.from_bcsr(ctx, R.rowptr, R.col, R.val, 2, 3, ncols_blocks=4)
    with pytest.raises(eigmi.EigShapeError) as e:  # rectangular blocks
        eigmi.Slice(Mr, 1.0, 2.0, LMIN, LMAX, block=8)
    assert e.value.code == eigmi.EIG_ERR_BLOCKSIZE
    Mr.close()


# ---- bounds and counts ----

@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_spectrum_bounds(ctx, name):
    A, _, lam = matrix(name)
    M = upload(ctx, A)
    lo, hi = eigmi.spectrum_bounds(M, 30, 123)
    al, be, _ = eigmi.lanczos_run(M, 30, seed=123)
    rlo, rhi = sr.spectrum_bounds(al, be)
    print(f"[slice] {name}: bounds {lo} {hi}, formula {rlo} {rhi}, spectrum {lam[0]} {lam[-1]}")
    assert abs(lo - rlo) <= 1e-14 and abs(hi - rhi) <= 1e-14
    assert lo <= lam[0] and hi >= lam[-1]
    M.close()


@pytest.mark.gpu
def test_filter_count(ctx):
    A, _, lam = matrix("var10")
    a, b = window(lam, *CASES["var10"][:2])
    M = upload(ctx, A)
    nvec = 32
    est = eigmi.filter_count(M, a, b, LMIN, LMAX, DEGREE, nvec, 7)
    c, e, _, _ = sr.filter_window(a, b, LMIN, LMAX)
    p = sr.filter_poly(sr.filter_coefs(a, b, LMIN, LMAX, DEGREE), (lam - c) / e)
    bound = 4 * np.sqrt(2 * np.sum(p * p) / nvec)
    print(f"[slice] count estimate {est:.3f}, trace p(A) {p.sum():.3f}, bound {bound:.3f}, eigenvalues in the window "
          f"{CASES['var10'][1]}")
    assert abs(est - p.sum()) <= bound
    M.close()
