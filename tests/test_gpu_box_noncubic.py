"""The box-grid kernels (k_box.hip: the row-class kernel k_boxc_mv8 with its epilogues, the box-image
kernels k_box_mv32 / k_box_mv16p) on grids whose three extents differ.  On a cube nx == ny == nz, so
an extent swapped in box_prepare's inference, in a tile bound, in box_cls1's class or in a row
address x + nx y + P z goes unseen; here (tests/box_grids.py) every extent and every offset's value is
its own.

    grid          rows   reaches
    (33,  9, 4)   1188   class tiles 32 + 1 by 8 + 1 (a last x tile of one column, a last y tile of one
                         row); image tiles 16 + 16 + 1
    (40,  8, 3)    960   the minimal ny and nz (one y tile, no interior z run)
    (16, 23, 5)   1840   the minimal nx, ny > nx, three y tiles
    (70, 12, 9)   7560   three class x tiles, five image x tiles

Bars: the SpMM BITWISE the reference row loop restated in oracle.spmm_mv8 (kernels_cpp.hh:626-657),
under every tuning too; the Chebyshev steps equal to the SELL kernel's to rounding (FMA against
separately rounded sums: rtol 1e-13, atol 1e-14 max|ref|, as test_gpu_sym.py::test_boxc_runtime_offsets);
the dot / Gram epilogues within the summation-order bound of test_gpu_blas_mv8.py::test_spmm_dot_gram_pair.
Every case asserts the kernel family it is meant for."""
import numpy as np
import pytest

import box_grids
import eigmi
import oracle

GRIDS = [(33, 9, 4), (40, 8, 3), (16, 23, 5), (70, 12, 9)]
SHAPES = ["p7", "kuhn15", "full27", "nine"]
NOFF = {"p7": 7, "kuhn15": 15, "full27": 27, "nine": 9}
BOX_KERNELS = ("k_box_mv32", "k_box_mv16p", "k_boxc_mv8")


# ---- the helper (CPU) ----

def _brute_pattern(dims, shape):
    nx, ny, nz = dims
    offs = box_grids.offsets(shape)
    rows = []
    for z in range(nz):
        for y in range(ny):
            for x in range(nx):
                rows.append(sorted((x + dx) + nx * ((y + dy) + ny * (z + dz)) for dx, dy, dz in offs
                                   if 0 <= x + dx < nx and 0 <= y + dy < ny and 0 <= z + dz < nz))
    return rows


def _offdiag(A):
    r = np.repeat(np.arange(A.n), np.diff(A.rowptr))
    return A.val[A.col != r]


def test_box_matrix_cube_patterns():
    """On a cube "p7" is the pattern of oracle.poisson3d and "kuhn15" that of the P1 Kuhn matrices."""
    N = 6
    P = oracle.poisson3d(N)
    M = oracle.p1_kuhn(N)[1]
    for values in ("const", "edge"):
        A = box_grids.box_matrix((N, N, N), "p7", values)
        assert np.array_equal(A.rowptr, P.rowptr) and np.array_equal(A.col, P.col)
        A = box_grids.box_matrix((N, N, N), "kuhn15", values)
        assert np.array_equal(A.rowptr, M.indptr) and np.array_equal(A.col, M.indices)


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("values", ["const", "edge"])
def test_box_matrix_properties(shape, values):
    """Every row stores exactly its in-grid neighbours (x fastest); bitwise symmetric; SPD; "const"
    has one value per offset pair, each pair its own, "edge" one per grid edge."""
    dims = (5, 4, 3)
    A = box_grids.box_matrix(dims, shape, values, seed=3)
    assert len(box_grids.offsets(shape)) == NOFF[shape]
    brute = _brute_pattern(dims, shape)
    assert A.n == 60 and A.rowptr.dtype == np.int64 and A.col.dtype == np.int32
    for r in range(A.n):
        assert list(A.col[A.rowptr[r]:A.rowptr[r + 1]]) == brute[r], r
    S = box_grids.to_scipy(A)
    assert (S != S.T).nnz == 0
    assert np.linalg.eigvalsh(S.toarray()).min() > 0
    d = S.diagonal()
    assert np.all(d > np.asarray(abs(S).sum(axis=1)).ravel() - d)  # strictly dominant
    off = _offdiag(A)
    if values == "const":
        assert len(np.unique(off)) == (NOFF[shape] - 1) // 2
    else:
        assert len(np.unique(off)) == off.size // 2  # (each edge's value stored twice)
    B = box_grids.to_scipy(box_grids.box_matrix(GRIDS[0], shape, values))  # and at a size the kernels see
    assert (B != B.T).nnz == 0 and B.shape[0] == 33 * 9 * 4


@pytest.mark.parametrize("shape", SHAPES)
def test_box_matrix_row_classes(shape):
    """The "const" rows equal their geometric class representative (position 0 / 1 / n - 1 per
    direction, what box_classes gathers); of the "edge" rows none but the representatives do."""
    dims = (6, 5, 4)
    rep = box_grids.class_representatives(dims)
    assert len(np.unique(rep)) == 27
    assert np.all(box_grids.rows_equal_class(box_grids.box_matrix(dims, shape, "const", seed=1), dims))
    eq = box_grids.rows_equal_class(box_grids.box_matrix(dims, shape, "edge", seed=1), dims)
    others = rep != np.arange(rep.size)
    assert np.all(eq[~others]) and not np.any(eq[others])


# ---- the kernels ----

def upload(ctx, A, flags=0):
    return eigmi.Matrix.from_bcsr(ctx, A.rowptr, A.col, A.val, flags=flags)


def _spmm(ctx, M, n, m, Q):
    Y = ctx.zeros(n * m)
    eigmi.spmm_mv8(M, m, Q, Y)
    return Y.get()


def _segs(nz):
    """EIG_TUNE_BOX_SEGS values: automatic, 1, 2, nz -- and 4 where the grid has 4 planes (the tile
    counts of these grids times 4 are multiples of 8, which EIG_TUNE_BOX_MAP = 1 needs to apply)."""
    return sorted({0, 1, 2, nz} | ({4} if nz >= 4 else set()))


def _image_tunings(nz):
    return [(cols, segs, xmap) for cols in (32, 16) for segs in _segs(nz) for xmap in (0, 1)]


def _check_image_kernels(ctx, M, A, nz, seed):
    """k_box_mv32 / k_box_mv16p at m = 32, 64: bitwise the reference, and bitwise so under every
    EIG_TUNE_BOX_COLS x EIG_TUNE_BOX_SEGS x EIG_TUNE_BOX_MAP."""
    assert M.kernel("spmm32") == "k_box_mv32"
    for m in (32, 64):
        Qh = oracle.random_mv8(A.n, m, seed + m)
        Q = ctx.array(Qh)
        ref = oracle.spmm_mv8(A, Qh, m)
        assert np.array_equal(_spmm(ctx, M, A.n, m, Q), ref), m
        for cols, segs, xmap in _image_tunings(nz):
            M.tune(box_cols=cols, box_segs=segs, box_map=xmap)
            assert M.kernel("spmm32") == ("k_box_mv16p" if cols == 16 else "k_box_mv32")
            assert np.array_equal(_spmm(ctx, M, A.n, m, Q), ref), (m, cols, segs, xmap)
        M.tune(box_cols=0, box_segs=0, box_map=0)


def _check_no_box(ctx, M, A, seed):
    assert M.kernel("spmm32") not in BOX_KERNELS and M.kernel("spmm8") not in BOX_KERNELS
    for m in (8, 32, 64):
        Qh = oracle.random_mv8(A.n, m, seed + m)
        assert np.array_equal(_spmm(ctx, M, A.n, m, ctx.array(Qh)), oracle.spmm_mv8(A, Qh, m)), m


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("dims", GRIDS, ids=lambda d: "x".join(map(str, d)))
def test_class_spmm_bitwise(ctx, dims, shape):
    """Class-constant rows: k_boxc_mv8 (compile-time 7 / 15 / 27-point stencils and, "nine", the
    runtime offset loop) at m = 8, 24, 32, bitwise the reference for every z-segment count; with
    EIG_MAT_NO_CLASS the same matrix on the box-image kernels (full27: past kBoxMaxNd offsets there
    is no box-image kernel -- no box kernel at all, still bitwise)."""
    A = box_grids.box_matrix(dims, shape, "const", seed=sum(dims))
    nz = dims[2]
    M = upload(ctx, A)
    assert M.info.sym_offsets == NOFF[shape]
    assert M.kernel("spmm8") == "k_boxc_mv8" and M.kernel("spmm32") == "k_boxc_mv8"
    for m in (8, 24, 32):
        Qh = oracle.random_mv8(A.n, m, 7 + m)
        Q = ctx.array(Qh)
        ref = oracle.spmm_mv8(A, Qh, m)
        for segs in _segs(nz):
            M.tune(box_segs=segs)
            assert np.array_equal(_spmm(ctx, M, A.n, m, Q), ref), (m, segs)
        M.tune(box_segs=0)
    M.close()
    Mi = upload(ctx, A, flags=eigmi.MAT_NO_CLASS)
    if shape == "full27":
        _check_no_box(ctx, Mi, A, 11)
    else:
        _check_image_kernels(ctx, Mi, A, nz, 11)
    Mi.close()


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("dims", GRIDS, ids=lambda d: "x".join(map(str, d)))
def test_image_spmm_bitwise(ctx, dims, shape):
    """One value per grid edge (a value read from the wrong row or plane shows anywhere): the
    box-image kernels, bitwise under every tuning; full27 has no box-image kernel."""
    A = box_grids.box_matrix(dims, shape, "edge", seed=sum(dims) + 1)
    M = upload(ctx, A)
    assert M.info.sym_offsets == NOFF[shape]
    if shape == "full27":
        _check_no_box(ctx, M, A, 13)
    else:
        _check_image_kernels(ctx, M, A, dims[2], 13)
    M.close()


@pytest.mark.gpu
@pytest.mark.parametrize("values", ["const", "edge"])
@pytest.mark.parametrize("shape", ["p7", "kuhn15"])
@pytest.mark.parametrize("dims", GRIDS, ids=lambda d: "x".join(map(str, d)))
def test_chebyshev_matches_sell(ctx, dims, shape, values):
    """eig_mass_solve_mv8 of degree 2 / 3 / 7 (the class kernel's first / second / general step
    epilogues; k_box_mv32_cheb and, EIG_TUNE_BOX_COLS = 16, k_box_mv16p_cheb on the image) against
    the same solve on the EIG_MAT_NO_MARCH upload (k_sell_mv8q_cheb), with fixed bounds (the kernels
    run the same recurrence; convergence is not the point)."""
    A = box_grids.box_matrix(dims, shape, values, seed=sum(dims) + 2)
    n, m = A.n, 32
    M, Ms = upload(ctx, A), upload(ctx, A, flags=eigmi.MAT_NO_MARCH)
    assert Ms.kernel("cheb32") == "k_sell_mv8q_cheb"
    Bh = oracle.random_mv8(n, m, 29)
    B = ctx.array(Bh)
    X1, X2 = ctx.zeros(n * m), ctx.zeros(n * m)
    lo, hi = 0.1, 2.0
    for cols in ((0,) if values == "const" else (32, 16)):
        M.tune(box_cols=cols)
        want = "k_boxc_mv8_cheb" if values == "const" else ("k_box_mv16p_cheb" if cols == 16 else "k_box_mv32_cheb")
        assert M.kernel("cheb32") == want
        for degree in (2, 3, 7):
            eigmi.mass_solve_mv8(M, m, degree, B, X1, lo, hi)
            eigmi.mass_solve_mv8(Ms, m, degree, B, X2, lo, hi)
            a, b = X1.get(), X2.get()
            assert np.all(np.isfinite(b)) and np.abs(b).max() > 0
            assert np.allclose(a, b, rtol=1e-13, atol=1e-14 * np.abs(b).max()), (cols, degree, np.abs(a - b).max())
    M.tune(box_cols=0)
    M.close()
    Ms.close()


@pytest.mark.gpu
@pytest.mark.parametrize("shape", ["p7", "kuhn15"])
@pytest.mark.parametrize("dims", GRIDS, ids=lambda d: "x".join(map(str, d)))
def test_dot_gram_epilogues(ctx, dims, shape):
    """eig_spmm_dot_gram_mv8 at m = 8 on the row-class kernel (its dot + Gram epilogue): the product
    bitwise, the diagonal dots and the upper window Gram within the summation-order bound, then
    eig_orthonormalize_gram_mv8 from that Gram within 1e-12 of the restated orthonormalize_blocked."""
    A = box_grids.box_matrix(dims, shape, "const", seed=sum(dims) + 3)
    n, m = A.n, 8
    M = upload(ctx, A)
    assert M.kernel("spmm8") == "k_boxc_mv8"
    Xh = oracle.random_mv8(n, m, 31)
    X, Y, dp, G = ctx.array(Xh), ctx.zeros(n * m), ctx.zeros(8), ctx.zeros(64)
    eigmi.spmm_dot_gram_mv8(M, m, X, Y, dp, G)
    Yh = Y.get()
    assert np.array_equal(Yh, oracle.spmm_mv8(A, Xh, m))
    Xc, Yc = oracle.mv_to_cols(Xh, n, m), oracle.mv_to_cols(Yh, n, m)
    bound_d = 4 * n * 2.3e-16 * np.einsum("ij,ij->j", np.abs(Xc), np.abs(Yc))
    assert np.all(np.abs(dp.get() - oracle.dot_diag_mv8(Xh, Yh, n, m)) <= bound_d)
    Gref = oracle.gram_mv8(Yh, Yh, n, m)
    bound_g = 4 * n * 2.3e-16 * (np.abs(Yc).T @ np.abs(Yc))
    g = G.get().reshape(8, 8)
    up = np.triu(np.ones((8, 8), bool))
    assert np.all(np.abs(g - Gref)[up] <= bound_g[up])
    eigmi.orthonormalize_gram_mv8(ctx, n, m, Y, G)
    ctx.sync()
    ref = oracle.orthonormalize_mv8(Yh, n, m)
    assert np.abs(Y.get() - ref).max() < 1e-12 * max(1.0, np.abs(ref).max())
    M.close()


@pytest.mark.gpu
@pytest.mark.parametrize("dims", [(15, 9, 5), (20, 7, 5), (20, 9, 2)], ids=lambda d: "x".join(map(str, d)))
def test_below_box_minima(ctx, dims):
    """nx < 16, ny < 8 or nz < 3: box_prepare refuses the grid; the product stays bitwise on whatever
    kernel takes it instead."""
    for shape in ("p7", "kuhn15"):
        for values in ("const", "edge"):
            A = box_grids.box_matrix(dims, shape, values, seed=sum(dims))
            M = upload(ctx, A)
            assert M.kernel("spmm32") not in ("k_box_mv32", "k_boxc_mv8"), (shape, values)
            _check_no_box(ctx, M, A, 17)
            M.close()
