"""Sparse products read only the entries a row stores, and write only the rows they own.

Every product kernel is pinned bitwise to the reference row loop elsewhere -- on finite x, where a
"not stored" operand is 0.0 and a stray read gives 0 * finite = 0.  Here x (or single entries X[j, c] of a
multivector, or of the Chebyshev right-hand side B) carries +Inf / NaN at a poison set J built by
tests/poison.py: rows that store a column of J are TAINTED (non-finite in the reference too), WITNESS rows
are untainted but have one of their false addresses -- the clamped position of an offset they do not
store (by grid face on the box grids), column 0, the last column, their own index -- in J.  Bars:

    isfinite(got) == isfinite(ref) everywhere, got bitwise ref where ref is finite
    (a leak makes a witness NaN; a kernel that skips a stored NaN makes a tainted row finite);
    every buffer has 512 guard doubles on either side (NaN around inputs, one sentinel bit pattern over
    outputs): inputs come back bit for bit, outputs hold the sentinel everywhere but the owned rows.

References: oracle.csr_mv (BCRSMatrix::mv), oracle.spmm_mv8 (matmul_sparse_tallskinny_blocked), both on the
poisoned input; for the Chebyshev step oracle.cheb_solve's reach set.  The helper's CPU tests assert, for every
matrix the GPU tests use: at most 25 % of the rows tainted, at least 2 witnesses per face / missing offset / SELL
address, and that the reference itself keeps every witness finite and every tainted row non-finite.

What the cases cannot reach, and one that is split:
  * k_spmm_mv8 is launched only for images of more than one row per lane, and every image is built with one
    (api.cpp "A.R = 1"): the SELL multivector product runs k_sell_mv8g (m = 8) and k_sell_mv8q (m >= 16).
  * the pipelined 2-line bodies march the fused step's pair vector only (march_plan.cpp: "can = fused && ...");
    eig_mv under EIG_TUNE_CACHE 64 / 80 runs the plain upward / downward body.
  * case 1 wants the own index of EVERY diagonal-less and empty row poisoned; each such column is stored by
    about 36 rows, so one launch with all of them taints the whole matrix.  They are poisoned in batches
    (poison.batches), every batch within the 25 % cap, every one of them poisoned in some launch.
"""
import threading

import numpy as np
import pytest

import box_grids
import eigmi
import oracle
import poison
from test_gpu_blocked_blanczos import damped, pencil
from test_gpu_blocked_spmm import expand
from test_gpu_blocked_spmm import random_bcsr as random_blocks
from test_gpu_sell_cpf import _ragged
from test_gpu_spmv import random_bcsr
from test_gpu_sym import band_matrix

BOX_GRIDS = [(33, 9, 4), (40, 8, 3), (16, 23, 5), (70, 12, 9)]
BOX_SHAPES = ["p7", "kuhn15", "nine"]
L2_GRIDS = [(64, 4, 6), (128, 2, 5), (64, 6, 9)]
GEO_GRIDS = [(64, 6, 9), (128, 9, 5)]
KUHN_GRIDS = {(64, 10, 7): 16, (64, 12, 6): 20, (128, 9, 5): 16}
SLAB_GRID, SLAB_RANKS = (64, 4, 15), 3
BLOCKS = [(2, 2), (3, 3), (4, 4), (2, 3), (4, 1)]


def gname(d):
    return "x".join(map(str, d))


# ---- the matrices and their poison sets: built once, shared, never modified ----

def _ragged_holes(square):
    """ragged3000 of test_gpu_sell_cpf.py without the diagonal entry of every 13th row, every row r % 17 == 5
    emptied, and (not square) 37 columns more than rows that no row references."""
    rp, c, v = _ragged()
    n = rp.size - 1
    r = np.repeat(np.arange(n), np.diff(rp))
    keep = ~((r % 13 == 0) & (c == r)) & (r % 17 != 5)
    rowptr = np.zeros(n + 1, np.int64)
    np.cumsum(np.bincount(r[keep], minlength=n), out=rowptr[1:])
    A = oracle.CSR(n, rowptr, c[keep].copy(), v[keep].copy())
    ncols = n if square else n + 37
    fa = poison.false_addresses(A, "sell", sell=True, ncols=ncols)
    extra = list(range(n, ncols)) + np.random.default_rng(41).choice(n, 8, replace=False).tolist()
    J = poison.poison_set(A, fa, ncols, extra=extra)
    holes = np.nonzero((np.arange(n) % 13 == 0) | (np.arange(n) % 17 == 5))[0]
    own = [int(h) for h in holes if h not in set(J.tolist())]
    return dict(A=A, ncols=ncols, fa=fa, J=J, batches=poison.batches(A, own, J.tolist()), holes=holes)


def _box(dims, shape, values, seed):
    A = box_grids.box_matrix(dims, shape, values, seed=seed)
    fa = poison.false_addresses(A, dims)
    return dict(A=A, ncols=A.n, fa=fa, J=poison.poison_set(A, fa), dims=dims)


def _band(A, sell=False, slices=False, offsets=None):
    fa = poison.false_addresses(A, offsets, sell=sell)
    if slices:
        fa.update(poison.slice_addresses(A))
    return dict(A=A, ncols=A.nrows, fa=fa, J=poison.poison_set(A, fa))


def _sell(A, ncols=None, slices=False):
    ncols = A.nrows if ncols is None else ncols
    fa = poison.false_addresses(A, "sell", sell=True, ncols=ncols)
    if slices:
        fa.update(poison.slice_addresses(A))
    return dict(A=A, ncols=ncols, fa=fa, J=poison.poison_set(A, fa, ncols))


def _slab():
    """The slab grid: J additionally holds entries in planes 4, 5, 9, 10 -- the planes on either side of the
    two cuts -- so the halo exchange carries poison into the ghosts."""
    dims = SLAB_GRID
    A = box_grids.box_matrix(dims, "p7", "edge", seed=sum(dims))
    D = dims[0] * dims[1]
    fa = poison.false_addresses(A, dims)
    extra = [p * D + 37 + 11 * k for k, p in enumerate((4, 5, 9, 10))]
    return dict(A=A, ncols=A.n, fa=fa, J=poison.poison_set(A, fa, extra=extra), dims=dims, halo=extra)


def _mixed():
    rp, c, v = eigmi.gen_matrix(eigmi.GEN_POISSON3D, 48)
    rp, c, v = eigmi.scrambled_rcm(rp, c, v, 123)
    return _sell(oracle.CSR(rp.size - 1, rp, c, v), slices=True)


def _blocked(name):
    if name == "q1elast5":
        return oracle.q1elast(5)
    if name == "q1elast5_damped":
        return damped(oracle.q1elast(5))
    if name.startswith("rand"):
        return random_blocks(int(name[4:]))
    return pencil(int(name[-1]))["M"]  # "massN": the SPD mass matrix of test_gpu_blocked_blanczos.py


BUILDERS = {"ragged_holes": lambda: _ragged_holes(False), "ragged_holes_sq": lambda: _ragged_holes(True),
            "poisson16_sell": lambda: _band(oracle.poisson3d(16), sell=True, slices=True, offsets=(16, 16, 16)),
            "poisson48_rcm_mixed": _mixed,
            "band_u8": lambda: _band(band_matrix(5000, [0, 1, 7, 130], 1)),
            "band_u32": lambda: _band(band_matrix(4100, [0, 1, 2, 3, 5, 8, 13, 21, 34, 55, 89, 144], 3, drop=0.1)),
            "laplace64": lambda: _band(oracle.laplace2d(64)),
            "laplace64_neumann": lambda: _band(oracle.laplace2d(64, "neumann")),
            "slab": _slab}
for _br, _bc in BLOCKS:
    BUILDERS[f"blocks_{_br}x{_bc}"] = (lambda br=_br, bc=_bc:
                                       _sell(random_bcsr(300, 257, br, bc, 0.03, 100 * br + bc), ncols=257))
for _d in GEO_GRIDS:
    BUILDERS[f"p7_const_{gname(_d)}"] = lambda d=_d: _box(d, "p7", "const", sum(d))
for _d in sorted(set(GEO_GRIDS + L2_GRIDS)):
    BUILDERS[f"p7_edge_{gname(_d)}"] = lambda d=_d: _box(d, "p7", "edge", sum(d) + 1)
for _d in KUHN_GRIDS:
    BUILDERS[f"kuhn15_edge_{gname(_d)}"] = lambda d=_d: _box(d, "kuhn15", "edge", sum(d))
for _d in BOX_GRIDS:
    for _s in BOX_SHAPES:
        for _v in ("const", "edge"):
            BUILDERS[f"{_s}_{_v}_{gname(_d)}"] = lambda d=_d, s=_s, v=_v: _box(d, s, v, sum(d) + 5)
for _n in ("q1elast5", "rand2", "rand3", "rand4", "q1elast5_damped", "mass2", "mass4"):
    BUILDERS[_n] = lambda n=_n: _sell(_blocked(n))

_CASES = {}


def case(name):
    if name not in _CASES:
        _CASES[name] = BUILDERS[name]()
    return _CASES[name]


def scalar(A):
    """The scalar expansion of a square-blocked matrix (what oracle.spmm_mv8 takes), A itself for 1x1."""
    return A if A.br == 1 else expand(A.rowptr, A.col, A.val, A.br)


def comp_of(A):
    return A.bc - 1  # the scalar component of a block column that carries the poison


# ---- the helper (CPU) ----

def test_layout_keeps_guards_and_alignment():
    for base in (0, 8, 256, 4096, 4096 * 7 + 8 * 511, 0x7F00_0000_1238):
        for n in (0, 1, 511, 512, 3037):
            for guard in (0, 512, 700):
                lead, total = poison.layout(base, n, guard)
                assert lead >= guard and (base + 8 * lead) % 4096 == 0
                assert total - lead - n >= guard and total == poison.layout(0, n, guard)[1]


def test_sentinel_and_untouched():
    s = np.array([poison.SENTINEL]).view(np.float64)
    assert np.isnan(s[0]) and (int(poison.SENTINEL) >> 51) & 1  # quiet
    whole = np.full(16, poison.SENTINEL, np.uint64).view(np.float64)
    mask = np.ones(16, bool)
    mask[4:8] = False
    whole[4:8] = 1.0
    assert poison.untouched(whole, mask)
    whole[9] = np.nan  # another NaN is not the sentinel: compared as bits
    assert not poison.untouched(whole, mask)


def test_comparison_catches_leaks_and_dropped_terms():
    ref = np.array([1.0, np.inf, np.nan, -0.0, 2.0])
    poison.assert_rows_only(np.array([1.0, np.nan, np.inf, -0.0, 2.0]), ref)  # any non-finite for a non-finite
    for bad in ([np.nan, np.inf, np.nan, -0.0, 2.0],   # a leak
                [1.0, 3.0, np.nan, -0.0, 2.0],          # a stored non-finite term dropped
                [1.0, np.inf, np.nan, 0.0, 2.0],        # +0 for -0: not bitwise
                [1.0, np.inf, np.nan, -0.0, 2.0000000000000004]):
        with pytest.raises(AssertionError):
            poison.assert_rows_only(np.array(bad), ref)


def test_false_addresses_small_box():
    """On a 4 x 3 x 3 box: by face, exactly the out-of-grid neighbours' clamped positions."""
    dims = (4, 3, 3)
    A = box_grids.box_matrix(dims, "p7", "const")
    fa = poison.false_addresses(A, dims)
    nx, ny, nz = dims
    _, x, y, z = box_grids.coords(dims)
    want = {"x-": (x == 0, -1), "x+": (x == nx - 1, 1), "y-": (y == 0, -nx), "y+": (y == ny - 1, nx),
            "z-": (z == 0, -nx * ny), "z+": (z == nz - 1, nx * ny)}
    for f, (on, d) in want.items():
        r = np.nonzero(on)[0]
        a = np.clip(r + d, 0, A.n - 1)
        keep = np.array([a[i] not in A.col[A.rowptr[r[i]]:A.rowptr[r[i] + 1]] for i in range(r.size)])
        got = sorted(zip(fa[f][0].tolist(), fa[f][1].tolist()))
        assert got == sorted(zip(r[keep].tolist(), a[keep].tolist())), f
    s = poison.false_addresses(A, "sell", sell=True)
    assert set(s) == {"first", "last", "own"} and s["own"][0].size == 0  # every row stores its diagonal
    assert 0 not in s["first"][0] and 1 not in s["first"][0] and 2 in s["first"][0]


@pytest.mark.parametrize("name", sorted(BUILDERS))
def test_poison_set_conditions(name):
    """Every matrix the GPU tests use: J holds the clamp targets; at most 25 % of the rows tainted; at least
    2 witnesses per face / missing offset / SELL address; and on the reference itself every witness is finite
    and every tainted row non-finite (so a pass of the GPU comparison means something)."""
    c = case(name)
    A, J, fa = c["A"], c["J"], c["fa"]
    assert 0 in J and c["ncols"] - 1 in J and np.array_equal(J, np.unique(J))
    sets = [J] + [np.unique(np.concatenate([J, b])) for b in c.get("batches", [])]
    if "batches" in c:
        assert np.array_equal(np.sort(np.concatenate([np.asarray(b) for b in c["batches"]] + [J[np.isin(J, c["holes"])]])),
                              c["holes"])  # every hole's own index is poisoned in some launch
    for Jk in sets:
        share, least, ok = poison.conditions(A, fa, Jk, c["ncols"])
        assert ok, (name, share, least, {k: len(v) for k, v in poison.witnesses(A, fa, Jk, c["ncols"]).items()})
    share, least, _ = poison.conditions(A, fa, J, c["ncols"])
    print(f"{name}: {A.nrows} rows, |J| = {J.size}, tainted {100 * share:.1f} %, least witnesses per key {least}, "
          f"{len(sets)} launch set(s)")
    x = poison.poisoned(np.random.default_rng(5).standard_normal(c["ncols"] * A.bc), J, A.bc, comp_of(A))
    ref = oracle.csr_mv(A, x).reshape(A.nrows, A.br)
    t = poison.tainted_rows(A, J)
    assert not np.isfinite(ref[t]).any() and np.isfinite(ref[~t]).all()
    for k, w in poison.witnesses(A, fa, J, c["ncols"]).items():
        assert np.isfinite(ref[w]).all(), k


@pytest.mark.parametrize("name", ["p7_edge_33x9x4", "kuhn15_edge_64x10x7", "band_u32", "ragged_holes", "poisson16_sell"])
def test_careless_product_is_caught(name):
    """What the witnesses are for, on the host: a product that multiplies the operand at a key's false addresses
    by an exact zero instead of leaving it out (0 * x[a] added to the row) differs from the reference at every
    witness of that key -- and the comparison says so -- while the reference itself passes."""
    c = case(name)
    A, J, fa = c["A"], c["J"], c["fa"]
    x = poison.poisoned(np.random.default_rng(8).standard_normal(c["ncols"]), J)
    ref = oracle.csr_mv(A, x)
    poison.assert_rows_only(ref.copy(), ref)
    wit = poison.witnesses(A, fa, J, c["ncols"])
    for k, (r, a) in fa.items():
        if not r.size:
            continue
        leaky = ref.copy()
        with np.errstate(invalid="ignore"):
            np.add.at(leaky, r, 0.0 * x[a])
        bad = poison.leaks(leaky, ref)
        assert wit[k].size >= 2 and np.isin(wit[k], bad).all(), k
        with pytest.raises(AssertionError):
            poison.assert_rows_only(leaky, ref)


def test_batches_respect_the_cap():
    c = case("ragged_holes")
    assert len(c["batches"]) > 1
    for b in c["batches"]:
        assert poison.tainted_rows(c["A"], set(c["J"].tolist()) | set(b)).mean() <= 0.25


# ---- the kernels ----

def report(family, c, kernels, J=None):
    """One line per case for the log: the kernels asserted, the tainted share, the witnesses."""
    A = c["A"]
    J = c["J"] if J is None else J
    share, least, _ = poison.conditions(A, c["fa"], J, c["ncols"])
    w = poison.witnesses(A, c["fa"], J, c["ncols"])
    rows = np.unique(np.concatenate(list(w.values()))).size if w else 0
    print(f"[poison] {family}: {kernels}; {A.nrows} rows, |J| = {len(J)}, tainted {100 * share:.1f} %, "
          f"{rows} witness rows over {sum(1 for k in w if c['fa'][k][0].size)} keys, at least {least} per key")


def upload(ctx, c, flags=0):
    A = c["A"]
    return eigmi.Matrix.from_bcsr(ctx, A.rowptr, A.col, A.val, A.br, A.bc, ncols_blocks=c["ncols"], flags=flags)


class MvRun:
    """eig_mv on guarded x and y for one matrix: x uploaded once per poison set, y reset to the sentinel
    before every launch."""

    def __init__(self, ctx, M, c, J=None, seed=3):
        A = c["A"]
        info = M.info
        self.M, self.n, self.own, self.window = M, int(info.n), int(info.own_offset), int(info.window)
        nx = c["ncols"] * A.bc
        assert self.own == 0 and self.window >= nx and self.n == A.n
        xh = np.full(self.window, np.nan)  # (window entries past the columns, if any, belong to no row)
        xh[:nx] = poison.poisoned(np.random.default_rng(seed).standard_normal(nx), c["J"] if J is None else J, A.bc,
                                  comp_of(A))
        self.ref = oracle.csr_mv(A, xh[:nx])
        self.x = poison.guarded(ctx, xh)
        self.y = poison.guarded_out(ctx, max(self.window, self.n))
        self.launches = 0

    def check(self, what):
        self.y.reset()
        self.M.mv(self.x.vec, self.y.vec)
        self.launches += 1
        whole = self.y.whole()
        poison.assert_rows_only(self.y.payload(whole)[:self.n], self.ref, what)
        assert poison.untouched(whole, self.y.outside(slice(0, self.n))), (what, "write outside the owned rows")
        assert self.x.intact(), (what, "x written")

    def free(self):
        print(f"[poison]   eig_mv: {self.launches} launches checked, {int((~np.isfinite(self.ref)).sum())} of {self.n} "
              "rows non-finite in the reference and on the device")
        self.x.free()
        self.y.free()


@pytest.mark.gpu
def test_sell_explicit_columns(ctx):
    """Case 1: k_spmv_b1 on explicit slices (46 full and a partial one), EIG_TUNE_SELL_CPF 0 and 1; rows without
    a diagonal, empty rows, 37 columns no row references.  J: the clamp targets, the 37 unreferenced columns, 8
    seeded columns, the greedy picks -- then, in batches under the 25 % cap, the own index of every diagonal-less
    and every empty row."""
    c = case("ragged_holes")
    M = upload(ctx, c, flags=eigmi.MAT_NO_BAND)
    info = M.info
    assert M.kernel("spmv") == "k_spmv_b1" and info.sym_offsets == 0 and info.stencil_slices == 0
    assert info.nslices == 47 and info.ncols == c["ncols"] == 3037
    for k, extra in enumerate([[]] + c["batches"]):
        run = MvRun(ctx, M, c, np.unique(np.concatenate([c["J"], np.asarray(extra, np.int64)])))
        for cpf in (0, 1):
            M.tune(sell_cpf=cpf)
            run.check(("batch", k, "cpf", cpf))
        run.free()
    report(f"1 SELL explicit ({1 + len(c['batches'])} poison sets, the first)", c, "k_spmv_b1, sell_cpf 0 / 1")
    M.close()


@pytest.mark.gpu
@pytest.mark.parametrize("br,bc", BLOCKS)
def test_sell_blocks(ctx, br, bc):
    """Case 2: k_spmv_blk (k_spmv_b1 for no blocks at all) on 300 x 257 block rows with empty rows; one scalar
    component of each poisoned block column carries the poison."""
    c = case(f"blocks_{br}x{bc}")
    M = upload(ctx, c)
    assert M.kernel("spmv") == "k_spmv_blk" and (M.info.br, M.info.bc) == (br, bc)
    run = MvRun(ctx, M, c)
    run.check((br, bc))
    run.free()
    report(f"2 SELL blocks {br}x{bc}", c, M.kernel("spmv"))
    M.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["poisson16_sell", "poisson48_rcm_mixed"])
def test_sell_stencil_slices(ctx, name):
    """Case 3: the SELL image's stencil slices (8 offsets and a row mask per slice) -- poisson3d(16), every
    slice a stencil slice, and the scrambled + RCM 48^3 image where they sit beside explicit slices.  False
    addresses: by grid face (poisson16), per slice the slice's offsets a row does not store, and column 0, the
    last column."""
    c = case(name)
    M = upload(ctx, c, flags=eigmi.MAT_NO_BAND)
    info = M.info
    assert M.kernel("spmv") == "k_spmv_b1" and info.sym_offsets == 0
    if name == "poisson16_sell":
        assert info.stencil_slices == info.nslices > 0
    else:
        assert 0 < info.stencil_slices < info.nslices
    run = MvRun(ctx, M, c)
    for cpf in (0, 1):
        M.tune(sell_cpf=cpf)
        run.check((name, cpf))
    run.free()
    report(f"3 SELL stencil slices {name}", c, f"k_spmv_b1, {info.stencil_slices} of {info.nslices} slices stencil")
    M.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["band_u8", "band_u32", "laplace64", "laplace64_neumann"])
def test_band_row_kernels(ctx, name):
    """Case 4: the band image's row kernels (rows_dot_stencil / sym_span gate the accumulation by the row
    mask): u8 and u32 masks; the 2-D Laplacians with EIG_MAT_NO_MARCH (they march otherwise -- that launch is
    checked as well).  One key per offset of the band."""
    c = case(name)
    lap = name.startswith("laplace")
    M = upload(ctx, c, flags=eigmi.MAT_NO_MARCH if lap else 0)
    info = M.info
    assert info.sym_offsets > 0 and info.sym_mask_bytes == (4 if name == "band_u32" else 1)
    assert M.kernel("spmv") == "k_spmv_b1" and info.march_variant_mv == -1
    run = MvRun(ctx, M, c)
    run.check(name)
    report(f"4 band rows {name}", c, f"k_spmv_b1 on the band image, {info.sym_offsets} offsets"
           + (", and k_spmv_march" if lap else ""))
    M.close()
    if lap:
        M = upload(ctx, c)
        assert M.kernel("spmv") == "k_spmv_march"
        run.M = M
        run.check((name, "march"))
        M.close()
    run.free()


@pytest.mark.gpu
@pytest.mark.parametrize("dims", GEO_GRIDS, ids=gname)
def test_march_uniform_mask_free(ctx, dims):
    """Case 5a: the mask-free geometric march on uniform bands (march_rows_geo2, variants 7 / 8 / 9: missing
    neighbours read as exact zeros through zero-record buffer descriptors), constant 7-point values."""
    c = case(f"p7_const_{gname(dims)}")
    M = upload(ctx, c)
    assert M.info.sym_uniform == 2 and M.kernel("spmv") == "k_spmv_march"
    run = MvRun(ctx, M, c)
    for pf, variant in ((0, 7), (6, 7), (7, 8), (8, 9)):
        for runs in (0, 2, 3):
            M.tune(runs, march_prefetch=pf)
            assert M.info.march_variant_mv == variant, (pf, runs)
            run.check((pf, runs))
    run.free()
    report(f"5a uniform march {gname(dims)}", c, "k_spmv_march variants 7 / 8 / 9")
    M.close()


@pytest.mark.gpu
@pytest.mark.parametrize("dims", GEO_GRIDS, ids=gname)
def test_march_value_variants(ctx, dims):
    """Case 5b: the value march on one value per grid edge: variant 15 and the prefetch variants 10, 11, 14, 18."""
    c = case(f"p7_edge_{gname(dims)}")
    M = upload(ctx, c)
    assert M.info.sym_geo == 1 and M.info.sym_uniform == 0 and M.kernel("spmv") == "k_spmv_march"
    run = MvRun(ctx, M, c)
    for pf, variant in ((13, 15), (9, 10), (10, 11), (12, 14), (15, 18)):
        for runs in (0, 2, 3):
            M.tune(runs, march_prefetch=pf)
            assert M.info.march_variant_mv == variant, (pf, runs)
            run.check((pf, runs))
    run.free()
    report(f"5b value march {gname(dims)}", c, "k_spmv_march variants 15 / 10 / 11 / 14 / 18")
    M.close()


@pytest.mark.gpu
@pytest.mark.parametrize("dims", L2_GRIDS, ids=gname)
def test_march_two_lines(ctx, dims):
    """Case 5c: the 2-line bodies of variants 22 / 23 (EIG_TUNE_MARCH_PREFETCH 16 / 17), plane runs 0, 2, 3,
    EIG_TUNE_CACHE 8 (up), 16 (down), 64 and 80 (up / down with the pipeline bit: eig_mv has no pipelined body,
    see the module docstring).  ny = 2 leaves neither gathered line; nx = 128 lets the edge lanes cross x runs."""
    c = case(f"p7_edge_{gname(dims)}")
    M = upload(ctx, c)
    run = MvRun(ctx, M, c)
    for pf, variant in ((16, 22), (17, 23)):
        for runs in (0, 2, 3):
            for cache in (8, 16, 64, 80):
                M.tune(runs, march_prefetch=pf, cache=cache)
                info = M.info
                assert info.march_variant_mv == variant and M.kernel("spmv") == "k_spmv_march", (pf, runs, cache)
                run.check((pf, runs, cache))
    run.free()
    report(f"5c two-line march {gname(dims)}", c, "k_spmv_march variants 22 / 23, up and down")
    M.close()


@pytest.mark.gpu
@pytest.mark.parametrize("dims", list(KUHN_GRIDS), ids=gname)
def test_march_kuhn(ctx, dims):
    """Case 5d: the Kuhn 15-point marches 16 / 20 / 12 (the pack, the pack with the line exchange in LDS, the
    band arrays), one value per grid edge."""
    c = case(f"kuhn15_edge_{gname(dims)}")
    M = upload(ctx, c)
    auto = KUHN_GRIDS[dims]
    assert M.info.sym_offsets == 15 and M.kernel("spmv") == "k_spmv_march"
    run = MvRun(ctx, M, c)
    for pf, variant in ((0, auto), (13, 16), (14, 12)):
        for runs in (0, 3):
            M.tune(runs, march_prefetch=pf)
            assert M.info.march_variant_mv == variant, (pf, runs)
            run.check((pf, runs))
    run.free()
    report(f"5d Kuhn march {gname(dims)}", c, f"k_spmv_march variants {auto} / 16 / 12")
    M.close()


class MmRun:
    """A multivector product on guarded Q and Y with single entries X[j, c] poisoned: c in the first 8-column
    block and in the last.  Every other column must be bitwise the clean reference in every row."""

    def __init__(self, ctx, c, m, seed=7):
        A = c["A"]
        E = scalar(A)
        n = self.n = E.n
        self.m = m
        Qh = oracle.random_mv8(n, m, seed)
        self.cols = (3, 5) if m == 8 else (3, m - 8 + 5)
        rows = c["J"] * A.bc + comp_of(A)
        entries = [(int(j), col) for col in self.cols for j in rows]
        Qp = poison.mv_poison(n, m, Qh, entries)
        self.ref = oracle.spmm_mv8(E, Qp, m)
        clean = oracle.mv_to_cols(oracle.spmm_mv8(E, Qh, m), n, m)
        rc = oracle.mv_to_cols(self.ref, n, m)
        self.others = np.setdiff1d(np.arange(m), self.cols)
        assert np.array_equal(rc[:, self.others], clean[:, self.others]) and np.isfinite(clean).all()
        assert not np.isfinite(rc[:, self.cols]).all()
        self.clean = clean
        self.Q = poison.guarded(ctx, Qp)
        self.Y = poison.guarded_out(ctx, n * m)

    def check(self, M, what, op=eigmi.spmm_mv8):
        self.Y.reset()
        op(M, self.m, self.Q.vec, self.Y.vec)
        whole = self.Y.whole()
        got = self.Y.payload(whole)
        poison.assert_rows_only(got, self.ref, what)
        gc = oracle.mv_to_cols(got, self.n, self.m)
        assert np.array_equal(gc[:, self.others], self.clean[:, self.others]), (what, "leak across columns")
        assert poison.untouched(whole, self.Y.outside(slice(0, self.n * self.m))), (what, "write outside Y")
        assert self.Q.intact(), (what, "Q written")

    def free(self):
        self.Q.free()
        self.Y.free()


@pytest.mark.gpu
@pytest.mark.parametrize("shape", BOX_SHAPES)
@pytest.mark.parametrize("dims", BOX_GRIDS, ids=gname)
def test_box_kernels(ctx, dims, shape):
    """Case 6: k_boxc_mv8 (zero halo rows and zero class entries, SHAPE != 0) at m = 8, 24 on constant values;
    k_box_mv32 / k_box_mv16p at m = 32 with EIG_TUNE_BOX_SEGS in {1, nz} and EIG_TUNE_BOX_MAP in {0, 1} on the
    same matrix under EIG_MAT_NO_CLASS and on one value per grid edge."""
    nz = dims[2]
    cc, ce = case(f"{shape}_const_{gname(dims)}"), case(f"{shape}_edge_{gname(dims)}")
    M = upload(ctx, cc)
    assert M.kernel("spmm8") == "k_boxc_mv8" and M.kernel("spmm32") == "k_boxc_mv8"
    for m in (8, 24):
        run = MmRun(ctx, cc, m)
        for segs in (1, nz):
            M.tune(box_segs=segs)
            run.check(M, ("class", m, segs))
        run.free()
    M.close()
    for c, flags in ((cc, eigmi.MAT_NO_CLASS), (ce, 0)):
        M = upload(ctx, c, flags=flags)
        run = MmRun(ctx, c, 32)
        for cols, kern in ((32, "k_box_mv32"), (16, "k_box_mv16p")):
            for segs in (1, nz):
                for xmap in (0, 1):
                    M.tune(box_cols=cols, box_segs=segs, box_map=xmap)
                    assert M.kernel("spmm32") == kern
                    run.check(M, (kern, flags, segs, xmap))
        run.free()
        M.close()
    report(f"6 box kernels {shape} {gname(dims)}", cc, "k_boxc_mv8, k_box_mv32, k_box_mv16p")


@pytest.mark.gpu
def test_sell_multivector(ctx):
    """Case 7a: the SELL multivector product on the case-1 matrix made square: k_sell_mv8g (m = 8) and
    k_sell_mv8q (m = 16: one pass of two column blocks; m = 40: a pass of four and a pass of one).
    (k_spmm_mv8 is not reachable: see the module docstring.)"""
    c = case("ragged_holes_sq")
    M = upload(ctx, c, flags=eigmi.MAT_NO_BAND)
    assert M.kernel("spmm8") == "k_sell_mv8g" and M.info.rows_per_lane == 1 and M.info.stencil_slices == 0
    for m in (8, 16, 40):
        run = MmRun(ctx, c, m)
        run.check(M, m)
        run.free()
    report("7a SELL multivector", c, "k_sell_mv8g (m = 8), k_sell_mv8q (m = 16, 40)")
    M.close()
    # ... and its stencil-slice instantiation (k_sell_mv8g / k_sell_mv8q <STENCIL = true>)
    c = case("poisson16_sell")
    M = upload(ctx, c, flags=eigmi.MAT_NO_BAND | eigmi.MAT_NO_MARCH)
    assert M.kernel("spmm8") == "k_sell_mv8g" and M.info.stencil_slices == M.info.nslices
    for m in (8, 24):
        run = MmRun(ctx, c, m)
        run.check(M, ("stencil", m))
        run.free()
    M.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["q1elast5", "rand2", "rand3", "rand4"])
def test_blocked_multivector(ctx, name):
    """Case 7b: k_spmm_blk_mv8 for b = 2, 3, 4 on q1elast(5) (3 x 3) and the random pattern of
    test_gpu_blocked_spmm.py, against oracle.spmm_mv8 on the scalar expansion."""
    c = case(name)
    M = upload(ctx, c)
    assert M.kernel("spmm8") == "k_spmm_blk_mv8"
    for m in (8, 24):
        run = MmRun(ctx, c, m)
        run.check(M, (name, m), op=eigmi.spmm_blk_mv8)
        run.free()
    report(f"7b blocked multivector {name} (b = {c['A'].br})", c, "k_spmm_blk_mv8")
    M.close()


def _cheb_check(ctx, M, c, m, lo, hi, kernel_note):
    """eig_mass_solve_mv8 of degree 1, 2, 3 with poison in B.  R = the entries where the restatement
    (oracle.cheb_solve) on the poisoned B is non-finite or differs bitwise from the restatement on the clean B:
    what the poison may reach in degree - 1 hops.  Outside R the device's poisoned run is bitwise its clean
    run; inside R it is non-finite wherever the restatement is."""
    A = c["A"]
    E = scalar(A)
    S = E.to_scipy()
    n = E.n
    Bc = np.random.default_rng(29).standard_normal((n, m))
    rows = c["J"] * A.bc + comp_of(A)
    cols = (3, m - 8 + 5)
    Bp = Bc.copy()
    for col in cols:
        Bp[rows, col] = poison.poison_values(rows.size)
    dB = {k: poison.guarded(ctx, oracle.cols_to_mv(B)) for k, B in (("clean", Bc), ("poisoned", Bp))}
    X = poison.guarded_out(ctx, n * m)
    for degree in (1, 2, 3):
        with np.errstate(all="ignore"):
            rc, rp = oracle.cheb_solve(S, Bc, degree, lo, hi), oracle.cheb_solve(S, Bp, degree, lo, hi)
        R = ~np.isfinite(rp) | (rp.view(np.uint64) != rc.view(np.uint64))
        assert np.isfinite(rc).all() and 0 < R.mean() < 0.9 and not R[:, np.setdiff1d(np.arange(m), cols)].any()
        got = {}
        for k in ("clean", "poisoned"):
            X.reset()
            eigmi.mass_solve_mv8(M, m, degree, dB[k].vec, X.vec, lo, hi)
            whole = X.whole()
            assert poison.untouched(whole, X.outside(slice(0, n * m))), (kernel_note, degree, k, "write outside X")
            assert dB[k].intact(), (kernel_note, degree, k, "B written")
            got[k] = oracle.mv_to_cols(X.payload(whole), n, m).copy()
        gc, gp = got["clean"], got["poisoned"]
        assert np.isfinite(gc).all()
        out = ~R
        assert np.array_equal(gp[out].view(np.uint64), gc[out].view(np.uint64)), \
            (kernel_note, degree, "poison outside the reach set", np.argwhere(out & ~np.isfinite(gp))[:8].tolist())
        nf = ~np.isfinite(rp)
        assert not np.isfinite(gp[nf]).any(), (kernel_note, degree, "a reached entry came out finite")
        print(f"[poison]   {kernel_note} degree {degree}: reach set {int(R.sum())} of {R.size} entries, non-finite "
              f"{int(nf.sum())} in the restatement, {int((~np.isfinite(gp)).sum())} on the device")
    for b in dB.values():
        b.free()
    X.free()


@pytest.mark.gpu
@pytest.mark.parametrize("kernel", ["k_boxc_mv8_cheb", "k_box_mv32_cheb", "k_sell_mv8q_cheb"])
def test_chebyshev_step(ctx, kernel):
    """Case 8: one Chebyshev-Jacobi step fused into the product, on the 33 x 9 x 4 grid (7-point): the row-class
    kernel (constant values), the box-image kernel (one value per edge) and the SELL kernel (EIG_MAT_NO_MARCH),
    m = 32, fixed bounds (the recurrence is the point, not its convergence)."""
    dims = BOX_GRIDS[0]
    c = case(f"p7_{'const' if kernel == 'k_boxc_mv8_cheb' else 'edge'}_{gname(dims)}")
    M = upload(ctx, c, flags=eigmi.MAT_NO_MARCH if kernel == "k_sell_mv8q_cheb" else 0)
    assert M.kernel("cheb32") == kernel
    _cheb_check(ctx, M, c, 32, 0.1, 2.0, kernel)
    report("8 Chebyshev step", c, kernel)
    M.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["mass2", "q1elast5_damped", "mass4"])
def test_chebyshev_step_blocked(ctx, name):
    """Case 8, blocks: k_spmm_blk_mv8_cheb for b = 2, 3, 4 (the mass matrices of test_gpu_blocked_blanczos.py;
    eig_mat_kernel_info names no blocked Chebyshev kernel, the blocked product's name stands for the image)."""
    c = case(name)
    M = upload(ctx, c)
    assert M.kernel("spmm8") == "k_spmm_blk_mv8" and M.info.br == c["A"].br > 1
    _cheb_check(ctx, M, c, 24, 0.5, 2.5, name)
    report(f"8 Chebyshev step {name} (b = {c['A'].br})", c, "k_spmm_blk_mv8_cheb")
    M.close()


@pytest.mark.gpu
def test_slabs(ctx):
    """Case 9: the 64 x 4 x 15 grid as 3 z-slabs over the loopback transport, variant 22, set up as
    test_gpu_march_direction.py::test_downward_on_slabs; EIG_TUNE_HALO 0 and 1, marching up (8) and down (16).
    J also holds entries in planes 4, 5, 9, 10, so the exchange carries Inf / NaN into the ghost planes.  Owned
    rows against the global reference; y outside the owned rows, and the guards of x and y, untouched (x's
    ghost entries are the exchange's to write: eigmi.h, eig_mv)."""
    c = case("slab")
    A, J, P = c["A"], c["J"], SLAB_RANKS
    D, nz = SLAB_GRID[0] * SLAB_GRID[1], SLAB_GRID[2]
    assert all(h in J for h in c["halo"])
    xh = poison.poisoned(np.random.default_rng(31).standard_normal(A.n), J)
    ref = oracle.csr_mv(A, xh)
    hub = eigmi.loopback_create(P)
    out = [None] * P

    def rank(r):
        rc = eigmi.Context(0)
        res = {"checks": 0, "fail": []}
        try:
            rc.comm_init_loopback(hub, r)
            b, e = nz * r // P * D, nz * (r + 1) // P * D
            lo, hi = A.rowptr[b], A.rowptr[e]
            M = eigmi.Matrix.from_rows(rc, A.n, b, A.rowptr[b:e + 1] - lo, A.col[lo:hi], A.val[lo:hi])
            M.tune(march_prefetch=16)
            info = M.info
            res["variant"] = (int(info.march_variant), int(info.march_variant_mv))
            own, window, n = int(info.own_offset), int(info.window), int(info.n)
            xw = np.zeros(window)
            xw[own:own + n] = xh[b:e]
            x, y = poison.guarded(rc, xw), poison.guarded_out(rc, window)
            xguard = x.outside(slice(0, window))
            for halo in (0, 1):
                for cache in (8, 16):
                    M.tune(halo_whole=halo, cache=cache)
                    x.reset()  # (ghosts zero again: this launch's exchange must fill them)
                    y.reset()
                    M.mv(x.vec, y.vec)
                    whole = y.whole()
                    xa = x.whole()
                    # (failures are collected, not raised: every rank takes every launch, or the others
                    # would wait in the exchange)
                    bad = poison.leaks(np.ascontiguousarray(y.payload(whole)[own:own + n]), ref[b:e])
                    if bad.size:
                        res["fail"].append((halo, cache, "rows", (b + bad[:8]).tolist()))
                    if not poison.untouched(whole, y.outside(slice(own, own + n))):
                        res["fail"].append((halo, cache, "y written outside the owned rows"))
                    if not np.array_equal(xa.view(np.uint64)[xguard], x.image.view(np.uint64)[xguard]):
                        res["fail"].append((halo, cache, "x guards written"))
                    if not np.array_equal(x.payload(xa)[own:own + n].view(np.uint64), xh[b:e].view(np.uint64)):
                        res["fail"].append((halo, cache, "x owned rows written"))
                    res["checks"] += 1
            res["ghost_poison"] = int((~np.isfinite(np.delete(x.payload(xa), np.s_[own:own + n]))).sum())
            x.free()
            y.free()
            M.close()
        except BaseException as err:  # noqa: BLE001 -- reported below
            res["error"] = repr(err)
        finally:
            rc.close()
        out[r] = res

    th = [threading.Thread(target=rank, args=(r,)) for r in range(P)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    eigmi.loopback_destroy(hub)
    for r, res in enumerate(out):
        assert "error" not in res, (r, res["error"])
        assert res["variant"] == (22, 22) and res["checks"] == 4, (r, res)
        assert not res["fail"], (r, res["fail"])
    assert all(res["ghost_poison"] > 0 for res in out), [res["ghost_poison"] for res in out]
    report("9 slabs, 3 ranks", c, "variant 22 split and whole launches, up and down; poisoned ghost entries per rank "
           f"{[res['ghost_poison'] for res in out]}")
