"""The blocked tall-skinny product k_spmm_blk_mv8 (k_mv8.hip): Qout = A Qin for a
BCRSMatrix<FieldMatrix<double,b,b>>, b = 2, 3, 4, over the blocked SELL-64 image.

The kernel's arithmetic contract -- per scalar row and column: start from 0.0, the row's stored
blocks in stored order, inside a block c = 0..b-1, s += a[r][c] * x[col*b + c], products and sums
rounded separately -- is exactly what the reference product matmul_sparse_tallskinny_blocked
(kernels_cpp.hh:626-657, oracle.spmm_mv8) does on the matrix's SCALAR EXPANSION: every stored block
becomes b scalar rows with b consecutive scalar entries each, explicit zeros inside blocks kept,
columns ascending.  So every comparison here is BITWISE against the oracle on expand(A), and (one
case) against BCRSMatrix::mv (eig_mv) column by column.

Cases: q1elast(5) (125 block rows: 2 slices, the second with 61 rows; rows of 8..27 blocks; 3x3) at
m = 8, 24, 40 (40 leaves a lone column block in the last group whatever the column blocks per
workgroup); random 2x2 / 4x4 patterns on 130 block rows (3 slices, the last with 2 rows; 0..11 blocks
per row, block row 5 empty); q1elast(52), whose 2,197 slices exceed the launcher's grid cap (2048
workgroups), so the grid-stride loop runs; the error paths.

The product on blocks is eig_spmm_blk_mv8 (eigmi.spmm_blk_mv8).  eig_spmm_mv8, the reference's entry
point, keeps the reference's refusal of blocks (tests/test_gpu_blas_mv8.py pins it)."""
import numpy as np
import pytest

import eigmi
import oracle

pytestmark = pytest.mark.gpu


def expand(rowptr, col, val, b):
    """oracle.CSR of the scalar expansion of a BCSR matrix with b x b row-major blocks: scalar row
    I*b + r holds, for each stored block (I, J) in stored order, the b entries a[r][0..b-1] at columns
    J*b .. J*b + b - 1 (zeros inside blocks kept)."""
    rowptr = np.asarray(rowptr, np.int64)
    col = np.asarray(col, np.int64)
    nb = rowptr.size - 1
    cnt = np.diff(rowptr)                                   # blocks per block row
    srp = np.zeros(nb * b + 1, np.int64)
    np.cumsum(np.repeat(cnt * b, b), out=srp[1:])
    I = np.repeat(np.arange(nb, dtype=np.int64), cnt)       # block row of each stored block
    k = np.arange(col.size, dtype=np.int64) - rowptr[I]     # its position in the block row
    r = np.arange(b, dtype=np.int64)[None, :, None]
    c = np.arange(b, dtype=np.int64)[None, None, :]
    pos = (b * b * rowptr[I] + k * b)[:, None, None] + r * (cnt[I] * b)[:, None, None] + c
    scol = np.empty(col.size * b * b, np.int32)
    sval = np.empty(col.size * b * b, np.float64)
    scol[pos.ravel()] = np.broadcast_to(col[:, None, None] * b + c, pos.shape).ravel()
    sval[pos.ravel()] = np.asarray(val, np.float64).reshape(-1)
    return oracle.CSR(nb * b, srp, scol, sval)


def random_bcsr(b, nb=130, seed=1):
    """0..11 blocks per block row (row 0 has 11, row 5 none), ascending distinct columns,
    unsymmetric normal values."""
    rng = np.random.default_rng(seed)
    cnt = rng.integers(0, 12, nb)
    cnt[0], cnt[5] = 11, 0
    rowptr = np.zeros(nb + 1, np.int64)
    np.cumsum(cnt, out=rowptr[1:])
    col = np.concatenate([np.sort(rng.choice(nb, int(k), replace=False)) for k in cnt]).astype(np.int32)
    val = rng.standard_normal(col.size * b * b)
    return oracle.CSR(nb, rowptr, col, val, b, b)


_cache = {}


def case(name):
    """(blocked oracle.CSR, its scalar expansion), built once per session and left unchanged."""
    if name not in _cache:
        A = {"q1elast5": lambda: oracle.q1elast(5), "q1elast52": lambda: oracle.q1elast(52),
             "rand2": lambda: random_bcsr(2), "rand4": lambda: random_bcsr(4)}[name]()
        _cache[name] = (A, expand(A.rowptr, A.col, A.val, A.br))
    return _cache[name]


def device_spmm(ctx, A, Qh, m):
    M = eigmi.Matrix.from_bcsr(ctx, A.rowptr, A.col, A.val, A.br, A.bc)
    Q, Y = ctx.array(Qh), ctx.zeros(A.n * m)
    eigmi.spmm_blk_mv8(M, m, Q, Y)
    got = Y.get()
    Q.free(), Y.free()
    return M, got


def test_expand_is_the_blocked_matrix():
    """the helper itself: the expansion's product equals BCRSMatrix::mv's restatement bitwise"""
    for name in ("q1elast5", "rand2", "rand4"):
        A, E = case(name)
        assert E.n == A.n and E.nnz == A.nnz * A.br * A.br
        x = np.random.default_rng(3).standard_normal(A.n)
        assert np.array_equal(oracle.csr_mv(E, x), oracle.csr_mv(A, x))


@pytest.mark.parametrize("m", [8, 16, 24, 40])  # 1, 2, 3 and 4 + 1 column blocks
def test_q1elast5_bitwise(ctx, m):
    A, E = case("q1elast5")
    assert A.nrows == 125 and (A.br, A.bc) == (3, 3)
    cnt = np.diff(A.rowptr)
    assert cnt.min() == 8 and cnt.max() == 27
    Qh = oracle.random_mv8(375, m, 7)
    M, got = device_spmm(ctx, A, Qh, m)
    assert M.info.nslices == 2
    assert np.array_equal(got, oracle.spmm_mv8(E, Qh, m))
    M.close()


@pytest.mark.parametrize("m", [8, 16])
@pytest.mark.parametrize("b", [2, 4])
def test_random_pattern_bitwise(ctx, b, m):
    A, E = case(f"rand{b}")
    assert A.rowptr[5] == A.rowptr[6]  # the empty block row: b zero rows in the result
    Qh = oracle.random_mv8(A.n, m, 7)
    M, got = device_spmm(ctx, A, Qh, m)
    assert M.info.nslices == 3
    ref = oracle.spmm_mv8(E, Qh, m)
    assert np.array_equal(got, ref)
    rows = oracle.mv_to_cols(got, A.n, m)[5 * b:6 * b]
    assert np.all(rows == 0.0)
    M.close()


def test_columns_are_eig_mv(ctx):
    """column j of the product is BCRSMatrix::mv (eig_mv, k_spmv_blk) of column j, bitwise: one
    column of the first and one of the last column block (m = 40: the lone block of the last group)"""
    A, _ = case("q1elast5")
    m = 40
    Qh = oracle.random_mv8(A.n, m, 7)
    M, got = device_spmm(ctx, A, Qh, m)
    X, Y = oracle.mv_to_cols(Qh, A.n, m), oracle.mv_to_cols(got, A.n, m)
    for j in (3, 39):
        assert np.array_equal(Y[:, j], M.mv_host(np.ascontiguousarray(X[:, j])))
    M.close()


def test_grid_stride_bitwise(ctx):
    """more slices than the launcher's grid cap (kStreamBlocks = 2048): q1elast(52) has 140,608 block
    rows = 2,197 slices, ~33 M scalar entries"""
    A, E = case("q1elast52")
    m = 8
    Qh = oracle.random_mv8(A.n, m, 7)
    M, got = device_spmm(ctx, A, Qh, m)
    assert M.info.nslices == 2197 > 2048
    assert np.array_equal(got, oracle.spmm_mv8(E, Qh, m))
    M.close()


def test_scalar_matrix_through_the_blocked_entry(ctx):
    """b = 1 through eig_spmm_blk_mv8 is the 1x1 product: bitwise the reference"""
    A = oracle.poisson3d(12)
    Qh = oracle.random_mv8(A.n, 16, 11)
    M, got = device_spmm(ctx, A, Qh, 16)
    assert np.array_equal(got, oracle.spmm_mv8(A, Qh, 16))
    M.close()


def test_error_paths(ctx):
    # rectangular blocks keep the reference's refusal
    nb = 6
    rowptr = np.arange(nb + 1, dtype=np.int64)
    col = np.arange(nb, dtype=np.int32)
    M23 = eigmi.Matrix.from_bcsr(ctx, rowptr, col, np.ones(nb * 6), 2, 3, ncols_blocks=nb)
    Q, Y = ctx.zeros(nb * 3 * 8), ctx.zeros(nb * 3 * 8)
    for product in (eigmi.spmm_blk_mv8, eigmi.spmm_mv8):
        with pytest.raises(eigmi.EigShapeError) as e:
            product(M23, 8, Q, Y)
        assert e.value.code == eigmi.EIG_ERR_BLOCKSIZE
    M23.close()
    A, _ = case("q1elast5")
    M = eigmi.Matrix.from_bcsr(ctx, A.rowptr, A.col, A.val, 3, 3)
    Q3 = ctx.zeros(A.n * 8)
    with pytest.raises(eigmi.EigError):  # in place: the kernel reads rows other workgroups write
        eigmi.spmm_blk_mv8(M, 8, Q3, Q3)
    assert M.kernel("spmm8") == "k_spmm_blk_mv8"
    assert M.kernel("cheb8") == "none"
    M.close()
