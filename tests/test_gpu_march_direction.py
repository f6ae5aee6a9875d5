"""Direction of the 2-line value march (k_march.hip march_rows_geo2_2l<DOWN>, march variants 22 / 23,
MarchPlan::down; DESIGN.md 4e "serpentine"): a launch may march its plane runs from the last plane down
to the first, so that it starts on the planes the launch before it touched last.

Bar: the downward body sums every row as the upward one does -- eig_mv BITWISE the reference row loop
(oracle.csr_mv) in either direction, at plane-run counts whose runs start and end on interior planes and
on the first and last global plane; the fused and classic recurrences within 1e-12 of their restatements
(the suite's bar for the fused step everywhere: only the order in which a launch's three sums add their
rows changes); the direction follows the launch index, so a run in batches or as replayed graphs is
bitwise the one-batch run, repairs in between included.

EIG_TUNE_CACHE: 0 = the default (kMarch2lSerpentine), 8 = every launch up, 16 = every launch of variants
22 / 23 down, 24 = fused launches alternate whatever the default is.

Matrices: the 7-point pattern with another value on every grid edge and every diagonal entry, so a (+D, 0)
pair or an operand carried to the wrong plane changes bits.  Small grids: ny = 2 leaves neither
gathered line, nx = 128 lets the edge lanes cross x runs, 9 planes is an odd count; 15 planes as three
slabs put a rank between two others.  One case runs the benchmark's own 256^3 image and step count."""
import threading

import numpy as np
import pytest

import eigmi
import oracle
from fused_ref import classic, classic_spread, shifted

pytestmark = pytest.mark.gpu

GRIDS = [(64, 4, 6), (128, 2, 5), (64, 6, 9)]
VARIANT = {16: 22, 17: 23}  # EIG_TUNE_MARCH_PREFETCH -> march variant


def box_random(nx, ny, nz, seed):
    """Symmetric 7-point values on an nx x ny x nz box: one random value per grid edge and per diagonal entry."""
    import scipy.sparse as sp
    rng = np.random.default_rng(seed)
    n = nx * ny * nz
    idx = np.arange(n)
    x, y, z = idx % nx, (idx // nx) % ny, idx // (nx * ny)
    rows, cols, vals = [idx], [idx], [6.0 + rng.random(n)]
    for step, ok in ((1, x < nx - 1), (nx, y < ny - 1), (nx * ny, z < nz - 1)):
        i = idx[ok]
        w = -0.5 - rng.random(i.size)
        rows += [i, i + step]
        cols += [i + step, i]
        vals += [w, w]
    S = sp.csr_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(n, n))
    S.sort_indices()
    return oracle.CSR(n, S.indptr.astype(np.int64), S.indices.astype(np.int32), S.data.astype(np.float64))


_CASES = {}


def case(grid):
    """The grid's matrix and its references, computed once and shared (never modified)."""
    if grid not in _CASES:
        A = box_random(*grid, seed=17 + len(_CASES))
        x = np.random.default_rng(31).standard_normal(A.n)
        U0 = oracle.random_vec(A.n, 123)
        _CASES[grid] = dict(A=A, x=x, mv=oracle.csr_mv(A, x), U0=U0, fused=oracle.lanczos_fused(A, U0, 20),
                            classic=oracle.lanczos(A, U0, 20)[1:])
    return _CASES[grid]


def upload(ctx, A):
    return eigmi.Matrix.from_bcsr(ctx, A.rowptr, A.col, A.val)


def fused_run(M, steps, batches=None, graph=False):
    """`steps` fused steps taken in the given batch sizes (one batch by default), eagerly or each batch as
    a captured and replayed graph: (alpha, beta, launches)."""
    batches = batches or (steps,)
    assert sum(batches) == steps
    ws = eigmi.LanczosWorkspace(M, steps, seed=123, fused=True)
    try:
        for k in batches:
            if graph:
                ws.capture(k)
                ws.replay()
            else:
                ws.step(k)
        a, b = ws.tridiag()
        return a, b, ws.info()[1]
    finally:
        ws.close()


# a 16-step run in 4 eager batches and in 3 graph batches; odd batch sizes, so that a direction taken from
# the launch's index within its batch (instead of the workspace's launch index) would change bits
BATCHES = (((3, 5, 3, 5), False), ((5, 6, 5), True))


def close(got, ref, rtol=1e-12):
    return np.allclose(got, ref, rtol=rtol, atol=0)


@pytest.mark.parametrize("grid", GRIDS, ids=lambda g: "x".join(map(str, g)))
def test_downward_body_row_exact(ctx, grid):
    """eig_mv through variants 22 / 23 marching down (cache 16), up (8) and by default (0): bitwise the
    reference row loop at every plane-run count."""
    c = case(grid)
    M = upload(ctx, c["A"])
    try:
        for pf in (16, 17):
            for runs in (0, 1, 2, 3, 5):
                for cache in (16, 8, 0):
                    M.tune(runs, march_prefetch=pf, cache=cache)
                    info = M.info
                    assert info.march_variant == VARIANT[pf] and info.march_variant_mv == VARIANT[pf], (pf, runs)
                    assert np.array_equal(M.mv_host(c["x"]), c["mv"]), (pf, runs, cache)
    finally:
        M.close()


@pytest.mark.parametrize("grid", GRIDS, ids=lambda g: "x".join(map(str, g)))
def test_recurrence_either_direction(ctx, grid):
    """20 fused steps under cache 0 (the default), 8 (up), 16 (down) and 24 (alternating) against
    orc_lanczos_fused, the classic recurrence marching down against orc_lanczos: rtol 1e-12."""
    c = case(grid)
    qa, qb = c["fused"]
    ra, rb = c["classic"]
    M = upload(ctx, c["A"])
    try:
        for pf in (16, 17):
            for runs in (0, 2, 3):
                for cache in (0, 8, 16, 24):
                    M.tune(runs, march_prefetch=pf, cache=cache)
                    assert M.info.march_variant == VARIANT[pf]
                    fa, fb, _ = eigmi.lanczos_run(M, 20, seed=123, fused=True)
                    print(grid, pf, runs, cache, "fused max rel diff alpha %.2e beta %.2e" %
                          (np.max(np.abs(fa - qa) / np.abs(qa)), np.max(np.abs(fb[1:] - qb[1:]) / np.abs(qb[1:]))))
                    assert close(fa, qa) and close(fb, qb), (pf, runs, cache)
                M.tune(runs, march_prefetch=pf, cache=16)
                ca, cb, _ = eigmi.lanczos_run(M, 20, seed=123)
                assert close(ca, ra) and close(cb, rb), (pf, runs)
    finally:
        M.close()


@pytest.mark.parametrize("runs", [0, 2])
@pytest.mark.parametrize("cache", [0, 24])
def test_direction_follows_launch_index(ctx, cache, runs):
    """A 16-step run under the default (cache 0) and under forced alternation (24): in 4 batches (3, 5, 3, 5
    steps) and in 3 batches as replayed graphs (5, 6, 5) bitwise the one-batch run -- the direction is a
    function of the launch index, which continues across batches, and a captured launch replays its own
    direction; odd batches start on either parity.  The
    automatic run count (0) gives this grid one plane per run, where the direction changes no order; at
    2 runs of 3 planes the alternating run (24) differs in its last bits from the all-upward one -- the
    directions do alternate -- while both stay within 1e-12 of each other."""
    c = case(GRIDS[0])
    M = upload(ctx, c["A"])
    try:
        M.tune(runs, march_prefetch=16, cache=cache)
        assert M.info.march_variant == 22 and M.lanczos_kernel_info(True)[0] == "k_lanczos_fused_march"
        a, b, L = fused_run(M, 16)
        for batches, graph in BATCHES:
            a2, b2, L2 = fused_run(M, 16, batches, graph)
            assert np.array_equal(a2, a) and np.array_equal(b2, b), (batches, graph)
        M.tune(runs, march_prefetch=16, cache=8)
        ua, ub, _ = fused_run(M, 16)
        assert close(a, ua) and close(b, ub)
        if cache == 24 and runs == 2:
            assert not (np.array_equal(a, ua) and np.array_equal(b, ub))
    finally:
        M.close()


def test_bench_image_256_either_direction(ctx):
    """What the benchmark runs: the Poisson 256^3 arrays image (EIG_MAT_NO_UNIFORM, variant 22), 10 + 100
    fused steps in two batches, then the coefficients -- under cache 0 (the default), 8 (every launch up)
    and 24 (alternating) against orc_lanczos_fused, rtol 1e-12, no repairs.  The one case here that is not
    small: at 2 runs of 128 planes an upward launch is followed at once by a downward one that re-reads
    the 1 MiB planes just written, which no small grid reproduces; one restatement run (about 12 s) is
    shared by the three settings."""
    N, W, K = 256, 10, 100
    rp, c, v = eigmi.gen_matrix(eigmi.GEN_POISSON3D, N)
    A = oracle.CSR(N ** 3, rp, c, v)
    qa, qb = oracle.lanczos_fused(A, oracle.random_vec(A.n, 123), W + K)
    M = eigmi.Matrix.from_bcsr(ctx, rp, c, v, flags=eigmi.MAT_NO_UNIFORM)
    try:
        assert M.info.march_variant == 22 and M.lanczos_kernel_info(True) == ("k_lanczos_fused_march", 64 * N ** 3)
        for cache in (0, 8, 24):
            M.tune(cache=cache)
            a, b, L = fused_run(M, W + K, (W, K))
            da, db = np.max(np.abs(a - qa) / np.abs(qa)), np.max(np.abs(b[1:] - qb[1:]) / np.abs(qb[1:]))
            print("256^3 cache", cache, "launches", L, "max rel diff alpha %.2e beta %.2e" % (da, db))
            assert L == W + K + 1  # (the steps and the forced repair of tridiag: no repair in between)
            assert a.size == W + K and close(a, qa) and close(b, qb), cache
    finally:
        M.close()


SLAB_GRID, SLAB_RANKS =(64, 4, 15), 3  # 5 planes per rank: the middle rank touches neither end of the grid


def test_downward_on_slabs(ctx):
    """The downward body where MarchPlan::gz0 and MarchPlan::zb are not zero: the 64 x 4 x 15 grid as 3
    z-slabs of 5 planes over the in-process loopback transport (one virtual rank per slab), variant 22.
    Split launches march the interior planes of a slab (zb = 1) and whole launches start on global plane
    gz0 = 5 r; the top rank's runs end on the last global plane, the bottom rank's on plane 0.  eig_mv
    marching down (cache 16), up (8) and by default (0) is bitwise the reference row loop on the global
    matrix; 20 fused steps marching down, up, by default and alternating (24) are within 1e-12 of
    orc_lanczos_fused, and every rank holds the same coefficients."""
    c = case(SLAB_GRID)
    A, P = c["A"], SLAB_RANKS
    D, nz = SLAB_GRID[0] * SLAB_GRID[1], SLAB_GRID[2]
    hub = eigmi.loopback_create(P)
    out = [None] * P

    def rank(r):
        rc = eigmi.Context(0)
        res = {"mv": {}, "fused": {}}
        try:
            rc.comm_init_loopback(hub, r)
            b, e = nz * r // P * D, nz * (r + 1) // P * D
            lo, hi = A.rowptr[b], A.rowptr[e]
            M = eigmi.Matrix.from_rows(rc, A.n, b, A.rowptr[b:e + 1] - lo, A.col[lo:hi], A.val[lo:hi])
            M.tune(march_prefetch=16)
            res["variant"] = (int(M.info.march_variant), int(M.info.march_variant_mv))
            res["rows"] = (b, e)
            for halo in (0, 1):
                for cache in (16, 8, 0, 24):
                    M.tune(halo_whole=halo, cache=cache)
                    if cache != 24:
                        xv, yv = M.window_vector(c["x"][b:e]), M.window_vector()
                        M.mv(xv, yv)
                        res["mv"][halo, cache] = M.owned(yv)
                        xv.free()
                        yv.free()
                    res["fused"][halo, cache] = eigmi.lanczos_run(M, 20, seed=123, fused=True)[:2]
            M.close()
        except Exception as err:  # noqa: BLE001 -- reported below
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
    qa, qb = c["fused"]
    for r, res in enumerate(out):
        assert "error" not in res, res["error"]
        assert res["variant"] == (22, 22), res["variant"]
        b, e = res["rows"]
        for key, y in res["mv"].items():
            assert np.array_equal(y, c["mv"][b:e]), (r, key)
        for key, (fa, fb) in res["fused"].items():
            print("rank", r, "halo_whole, cache", key, "fused max rel diff alpha %.2e beta %.2e" %
                  (np.max(np.abs(fa - qa) / np.abs(qa)), np.max(np.abs(fb[1:] - qb[1:]) / np.abs(qb[1:]))))
            assert close(fa, qa) and close(fb, qb), (r, key)
            assert np.array_equal(fa, out[0]["fused"][key][0]) and np.array_equal(fb, out[0]["fused"][key][1])


@pytest.mark.parametrize("runs", [0, 3])
@pytest.mark.parametrize("cache", [0, 24])
def test_repairs_between_alternating_launches(ctx, cache, runs):
    """+100 on a dozen diagonal entries of the 64 x 6 x 9 grid: some predictions are unsound, those launches
    repair (no march, but a launch index), and the parity of the marching launches continues past them.
    Same launch count as the restatement, alpha / beta within the guard tests' tolerance of it and of the
    classic recurrence; batches and graphs bitwise the one-batch run."""
    A0 = case(GRIDS[2])["A"]
    A = shifted(A0, 0.0, range(0, A0.n, A0.n // 12), 1e2)
    u0 = oracle.random_vec(A.n, 123)
    ca, cb = classic(A, u0, 16)
    oa, ob, oL = oracle.lanczos_fused(A, u0, 16, with_launches=True)
    tol = max(1e-12, 4 * classic_spread(A, u0, 16, cb))
    M = upload(ctx, A)
    try:
        M.tune(runs, march_prefetch=16, cache=cache)
        assert M.info.march_variant == 22
        a, b, L = fused_run(M, 16)
        assert L == oL and L > 17
        print("repairs: launches", L, "tol %.2e" % tol, "max rel diff alpha %.2e beta %.2e" %
              (np.max(np.abs(a - oa) / np.abs(oa)), np.max(np.abs(b[1:] - ob[1:]) / np.abs(ob[1:]))))
        assert np.all(np.abs(a - oa) <= tol * np.abs(oa)) and np.all(np.abs(b - ob) <= tol * np.abs(ob))
        assert np.all(np.abs(a - ca) <= tol * np.abs(ca)) and np.all(np.abs(b - cb) <= tol * np.abs(cb))
        for batches, graph in BATCHES:
            a2, b2, L2 = fused_run(M, 16, batches, graph)
            assert np.array_equal(a2, a) and np.array_equal(b2, b), (batches, graph)
    finally:
        M.close()
