"""Geometric multigrid inner solve (csrc/mg.cpp, k_mg.hip; VERDICT r2 'next' #7): the smallest end of
the C5 pencil K x = lambda M x -- what GeneralizedInverse returns (eigensolver.hh:204-351; the
reference factors with UMFPACK, which has no counterpart at 256^3) -- through block Lanczos on
(K - sigma M)^-1 M with the Ks solve by a fixed number of multigrid iterations.

Bars: the device solve equals the numpy restatement (tests/mg_ref.py: same hierarchy, recurrence
and V-cycle; different rounding order) to 1e-12 relative; it converges geometrically (factor < 0.2
per iteration with the default smoother) to 1e-12; the operator is symmetric to rounding (the
Lanczos needs a self-adjoint OP); the 4 smallest eigenvalues at N = 24 within 1e-8 of ARPACK
shift-invert (scipy eigsh sigma = 0, exact factorisation), as test_shift_invert_smallest_p1 holds
the Chebyshev-Jacobi solve."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

import box_grids
import eigmi
import mg_ref
import oracle


def _upload(ctx, A):
    A = A.tocsr()
    A.sort_indices()
    return eigmi.Matrix.from_bcsr(ctx, A.indptr.astype(np.int64), A.indices.astype(np.int32), A.data)


def _mv(ctx, X):
    """(n, m) host array -> device MultiVector<double,8>."""
    return ctx.array(oracle.cols_to_mv(X))


def _cols(d, n, m):
    return oracle.mv_to_cols(d.get(), n, m)


def poisson7(N):
    A = oracle.poisson3d(N)
    return sp.csr_matrix((A.val, A.col, A.rowptr), shape=(A.n, A.n))


def test_mg_ref_hierarchy_is_symmetric_galerkin():
    """CPU: the restatement's coarse operators are P^T A P (to rounding) and bitwise symmetric."""
    K, _ = oracle.p1_kuhn(12)
    mg = mg_ref.Multigrid(K, (12, 12, 12))
    assert [L["A"].shape[0] for L in mg.levels] == [1728, 216, 27]
    for f, c in zip(mg.levels[:-1], mg.levels[1:]):
        G = (f["P"].T @ f["A"] @ f["P"]).toarray()
        assert np.abs(c["A"].toarray() - G).max() <= 1e-14 * np.abs(G).max()
        assert (c["A"] != c["A"].T).nnz == 0


@pytest.mark.gpu
@pytest.mark.parametrize("kind,N,m", [("p1", 12, 8), ("p1", 24, 32), ("poisson7", 20, 16), ("p1", 17, 8),
                                      ("p1var", 24, 32), ("p1var", 18, 24),
                                      ("p1", 32, 16)])  # 32: the 16^3 Galerkin level on the 27-point class kernel
def test_mg_solve_matches_restatement(ctx, kind, N, m):
    """p1var: K + a random positive diagonal -- rows no longer equal their geometric class, so the
    fine level runs the box-image kernels (k_box_mv32) instead of the row-class ones."""
    if kind == "p1var":
        K = oracle.p1_kuhn(N)[0]
        K = (K + sp.diags(np.random.default_rng(N).uniform(0.0, 0.1, K.shape[0]) / (N + 1))).tocsr()
    else:
        K = oracle.p1_kuhn(N)[0] if kind == "p1" else poisson7(N)
    n = K.shape[0]
    dK = _upload(ctx, K)
    mg = eigmi.Multigrid(dK, (N, N, N), max_cols=32, smooth_degree=2, smooth_ratio=5.0)
    ref = mg_ref.Multigrid(K, (N, N, N), 2, 5.0)
    info = mg.info()
    assert info["levels"] == len(ref.levels) and info["coarse_rows"] == ref.levels[-1]["A"].shape[0]
    assert info["coarse_degree"] == ref.levels[-1]["cdeg"]
    B = np.random.default_rng(N).standard_normal((n, m))
    dB, dX = _mv(ctx, B), ctx.zeros(n * m)
    for cycles in (1, 3):
        mg.solve(m, dB, dX, cycles)
        X = _cols(dX, n, m)
        R = ref.solve(B, cycles)
        assert np.abs(X - R).max() <= 1e-12 * np.abs(R).max(), (cycles, np.abs(X - R).max())
    mg.close()
    dK.close()


def test_mg_ref_hierarchy_noncubic():
    """CPU: the restatement on a 66 x 9 x 17 box (three distinct extents, odd and even): each
    direction halves on its own, the coarse operators are P^T A P and bitwise symmetric."""
    dims = (66, 9, 17)
    for shape, values in (("p7", "const"), ("kuhn15", "edge")):
        K = box_grids.to_scipy(box_grids.box_matrix(dims, shape, values, seed=5))
        mg = mg_ref.Multigrid(K, dims)
        assert [L["dims"] for L in mg.levels] == [(66, 9, 17), (33, 4, 8), (16, 2, 4)]
        assert [L["A"].shape[0] for L in mg.levels] == [10098, 1056, 128]
        for f, c in zip(mg.levels[:-1], mg.levels[1:]):
            G = (f["P"].T @ f["A"] @ f["P"]).toarray()
            assert np.abs(c["A"].toarray() - G).max() <= 1e-14 * np.abs(G).max()
            assert (c["A"] != c["A"].T).nnz == 0


BOX_KINDS = {"p7const": ("p7", "const", "k_boxc_mv8"), "full27const": ("full27", "const", "k_boxc_mv8"),
             "p7edge": ("p7", "edge", "k_box_mv32")}


@functools.lru_cache(maxsize=None)
def _box_problem(dims, kind):
    shape, values, _ = BOX_KINDS[kind]
    K = box_grids.to_scipy(box_grids.box_matrix(dims, shape, values, seed=sum(dims)))
    return K, np.random.default_rng(dims[0]).standard_normal((K.shape[0], 32))


@functools.lru_cache(maxsize=None)
def _box_ref(dims, kind, nu):
    return mg_ref.Multigrid(_box_problem(dims, kind)[0], dims, nu, 5.0)


# every grid, kind and smoother degree at least three times, both column counts on each grid
BOX_CASES = [((130, 12, 20), "p7const", 1, 8), ((130, 12, 20), "full27const", 2, 32), ((130, 12, 20), "p7edge", 3, 32),
             ((130, 12, 20), "p7const", 2, 32),
             ((66, 9, 17), "p7const", 3, 32), ((66, 9, 17), "full27const", 1, 8), ((66, 9, 17), "p7edge", 2, 8),
             ((66, 9, 17), "full27const", 3, 32),
             ((40, 24, 10), "p7edge", 1, 32), ((40, 24, 10), "full27const", 2, 8), ((40, 24, 10), "p7const", 3, 8),
             ((17, 40, 12), "full27const", 3, 8), ((17, 40, 12), "p7edge", 1, 8), ((17, 40, 12), "p7const", 2, 32),
             ((17, 40, 12), "p7edge", 2, 32)]


@pytest.mark.gpu
@pytest.mark.parametrize("dims,kind,nu,m", BOX_CASES,
                         ids=["%dx%dx%d-%s-nu%d-m%d" % (*c[0], c[1], c[2], c[3]) for c in BOX_CASES])
def test_mg_solve_matches_restatement_boxes(ctx, dims, kind, nu, m):
    """Grids with three distinct extents (tests/box_grids.py), so galerkin() and the transfers decode
    (x, y, z) from extents that differ, and wide enough in x for more than one workgroup per line:
    130 x 12 x 20 -> 65 x 6 x 10 -> 32 x 3 x 5 -> 16 x 1 x 2 prolongs in three 64-x blocks and restricts
    into cx = 65 (three 32-x blocks) and cx = 32; fx = 66 straddles the 64-x block by two; 17 x 40 x 12
    has y the long direction.  Smoother degrees 1 / 2 / 3 (nu != 2: the post-smoother through
    cheb_solve + axpby).  p7edge: one value per grid edge, the fine level on the box-image kernels.
    Bar: 1e-12 relative to max|R| against tests/mg_ref.py, whose own sensitivity to a 2.2e-16
    perturbation of B is below 1e-15 on these grids; prints the measured deviation."""
    K, B32 = _box_problem(dims, kind)
    n = K.shape[0]
    dK = _upload(ctx, K)
    assert dK.kernel("spmm32") == BOX_KINDS[kind][2]
    mg = eigmi.Multigrid(dK, dims, max_cols=32, smooth_degree=nu, smooth_ratio=5.0)
    ref = _box_ref(dims, kind, nu)
    info = mg.info()
    assert info["levels"] == len(ref.levels) and info["coarse_rows"] == ref.levels[-1]["A"].shape[0]
    assert info["coarse_degree"] == ref.levels[-1]["cdeg"]
    B = np.ascontiguousarray(B32[:, :m])
    dB, dX = _mv(ctx, B), ctx.zeros(n * m)
    for cycles in (1, 3):
        mg.solve(m, dB, dX, cycles)
        X = _cols(dX, n, m)
        R = ref.solve(B, cycles)
        dev = np.abs(X - R).max() / np.abs(R).max()
        print(f"multigrid {dims} {kind} nu={nu} m={m} cycles={cycles}: |X - R|.max() / |R|.max() = {dev:.2e}, "
              f"coarse degree {info['coarse_degree']}")
        assert np.abs(X - R).max() <= 1e-12 * np.abs(R).max(), (cycles, dev)
    mg.close()
    dK.close()


@pytest.mark.gpu
@pytest.mark.parametrize("nu", [2, 3])
def test_mg_is_symmetric_noncubic(ctx, nu):
    """The symmetry check of test_mg_converges_and_is_symmetric on 66 x 9 x 17 at 6 iterations:
    restriction is exactly P^T and the post-smoother the adjoint of the pre-smoother, so B^T S_6 B
    is symmetric to rounding."""
    dims, m = (66, 9, 17), 8
    K, B32 = _box_problem(dims, "p7const")
    n = K.shape[0]
    dK = _upload(ctx, K)
    mg = eigmi.Multigrid(dK, dims, max_cols=8, smooth_degree=nu, smooth_ratio=5.0)
    B = np.ascontiguousarray(B32[:, :m])
    dB, dX = _mv(ctx, B), ctx.zeros(n * m)
    mg.solve(m, dB, dX, 6)
    G = B.T @ _cols(dX, n, m)
    assert np.all(np.isfinite(G))
    assert np.abs(G - G.T).max() <= 1e-13 * np.abs(G).max(), np.abs(G - G.T).max() / np.abs(G).max()
    mg.close()
    dK.close()


@pytest.mark.gpu
def test_mg_converges_and_is_symmetric(ctx):
    N, m = 24, 8
    K, _ = oracle.p1_kuhn(N)
    n = K.shape[0]
    dK = _upload(ctx, K)
    mg = eigmi.Multigrid(dK, (N, N, N), max_cols=8, smooth_degree=2, smooth_ratio=5.0)
    B = np.random.default_rng(3).standard_normal((n, m))
    dB, dX = _mv(ctx, B), ctx.zeros(n * m)
    r = [mg.solve(m, dB, dX, c, resid=True) for c in (2, 6, 14)]
    print("multigrid residual after 2 / 6 / 14 iterations:", r)
    assert np.all(np.isfinite(r)) and r[0] < 0.05, r  # (2 iterations at ~0.1 each)
    rho = (r[1] / r[0]) ** 0.25
    assert rho < 0.2, rho
    assert r[2] <= 1e-12
    # symmetry of the fixed operator S = S_6: y^T S x = x^T S y
    mg.solve(m, dB, dX, 6)
    SB = _cols(dX, n, m)
    G = B.T @ SB
    assert np.abs(G - G.T).max() <= 1e-13 * np.abs(G).max()
    mg.close()
    dK.close()


@pytest.mark.gpu
def test_mg_rejects_bad_grids(ctx):
    K, _ = oracle.p1_kuhn(6)
    dK = _upload(ctx, K)
    with pytest.raises(eigmi.EigShapeError):
        eigmi.Multigrid(dK, (6, 6, 5))
    # a matrix coupling nodes two grid steps apart is not a box stencil on that grid
    A = (sp.identity(216) * 4 + sp.eye(216, k=2) + sp.eye(216, k=-2)).tocsr()
    dA = _upload(ctx, A)
    with pytest.raises(eigmi.EigError):
        eigmi.Multigrid(dA, (6, 6, 6))


@pytest.mark.gpu
@pytest.mark.parametrize("dims", [(128, 128, 1), (64, 64, 4)])
def test_mg_refuses_flat_grids(ctx, dims):
    """A direction below 3 nodes stops the coarsening: a flat grid would leave a coarsest level of
    thousands of rows for the dense host eigensolve -- refused with EIG_ERR_ARG at once."""
    import time
    nx, ny, nz = dims
    L = [sp.diags([-np.ones(k - 1), 2 * np.ones(k), -np.ones(k - 1)], [-1, 0, 1]) for k in (nx, ny, nz)]
    I = [sp.identity(k) for k in (nx, ny, nz)]
    A = (sp.kron(sp.kron(I[2], I[1]), L[0]) + sp.kron(sp.kron(I[2], L[1]), I[0]) +
         sp.kron(sp.kron(L[2], I[1]), I[0]) + 0.1 * sp.identity(nx * ny * nz)).tocsr()
    dA = _upload(ctx, A)
    t0 = time.perf_counter()
    with pytest.raises(eigmi.EigError) as e:
        eigmi.Multigrid(dA, dims)
    assert e.value.code == eigmi.EIG_ERR_ARG and "semi-coarsening" in str(e.value)
    assert time.perf_counter() - t0 < 5.0


@pytest.mark.gpu
def test_shift_invert_smallest_p1_multigrid(ctx):
    """As test_block_lanczos.py::test_shift_invert_smallest_p1, with the K solve by 14 multigrid
    iterations (residual ~1e-13) instead of ~240 Chebyshev-Jacobi steps."""
    import scipy.sparse.linalg as ssl
    N = 24
    K, M = oracle.p1_kuhn(N)
    dK, dM = _upload(ctx, K), _upload(ctx, M)
    mg = eigmi.Multigrid(dK, (N, N, N), max_cols=32, smooth_degree=2, smooth_ratio=5.0)
    bl = eigmi.BlockLanczos(dK, dM, block=32, max_steps=8, Ks=dK, sigma=0.0, mg=mg, cycles=14)
    bl.step(8)
    ev, Y, res = bl.ritz(4, eigmi.WHICH_SA, want_evec=True)
    print("SI block Lanczos N=24 (multigrid solve):", ev)
    ref = np.sort(ssl.eigsh(K, k=4, M=M, sigma=0.0, which="LM", tol=1e-14, v0=np.ones(K.shape[0]),
                            return_eigenvectors=False))
    assert np.all(np.diff(ev) >= 0)
    assert np.max(np.abs(ev - ref) / ref) <= 1e-8, (ev, ref)
    for lam, y in zip(ev, Y):
        r = K @ y - lam * (M @ y)
        assert np.linalg.norm(r) <= 1e-5 * lam * np.linalg.norm(M @ y)
    bl.close()
    mg.close()


@pytest.mark.gpu
def test_solves_reject_aliased_output(ctx):
    """The multigrid and mass solves read B in every iteration / step: X == B is refused."""
    K, M = oracle.p1_kuhn(6)
    dK, dM = _upload(ctx, K), _upload(ctx, M)
    mg = eigmi.Multigrid(dK, (6, 6, 6), max_cols=8)
    B = _mv(ctx, np.ones((K.shape[0], 8)))
    with pytest.raises(eigmi.EigError):
        mg.solve(8, B, B, 2)
    with pytest.raises(eigmi.EigError):
        eigmi.mass_solve_mv8(dM, 8, 4, B, B)
    mg.close()
