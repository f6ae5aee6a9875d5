"""Pipelined body of the fused 2-line value march (k_march.hip march_rows_geo2_2l<DOWN, PIPE>, MarchPlan::pipe;
DESIGN.md 4e "pipeline"): every loop load of variants 22 / 23 goes through LDS as an LDS-DMA issued one plane
ahead.  The body does the plain body's arithmetic in its order and a lane adds its rows into the launch's
three sums in the same order, so against the plain body of the SAME build (EIG_TUNE_CACHE 32 = never
pipeline) alpha, beta and the final (t, u) pair vector are BITWISE equal; against orc_lanczos_fused the
suite's bar for the fused step, rtol 1e-12.  EIG_TUNE_CACHE 64 pipelines wherever the body can run, so small
grids reach it; + 8 / 16 / 24 fix the direction up / down / alternating (0: the default, serpentine).

Grids: 64 x 2 x 3 (one line pair, no y gathers), 64 x 4 x 1 and 128 x 6 x 5 (the x edge between waves; first,
interior and last line pairs).  march_plan marches a whole matrix only from 4 planes on, so the first two do not
march at all (the row kernels run; asserted, and both arms still agree bitwise); their marching counterparts
64 x 2 x 4 and 64 x 4 x 4 carry what they were chosen for: at 5 plane runs (clipped to 4) every run is ONE
plane -- nothing but the prologue's DMAs and the last-plane wait -- and at 2 runs a run is the prologue plus
one step.  Matrices: 7-point values, constant (Poisson) and one random value per edge and diagonal entry,
uploaded with EIG_MAT_NO_UNIFORM; variant 22 forced with EIG_TUNE_MARCH_PREFETCH 16."""
import threading

import numpy as np
import pytest

import eigmi
import oracle
from fused_ref import shifted

pytestmark = pytest.mark.gpu

GRIDS = [(64, 2, 3), (64, 4, 1), (128, 6, 5), (64, 2, 4), (64, 4, 4)]
RUNS = (1, 2, 5)
DIRS = (0, 8, 16, 24)
STEPS = 20


def box(nx, ny, nz, seed=None):
    """Symmetric 7-point values on an nx x ny x nz box: Poisson (6, -1), or with a seed one random value per
    grid edge and per diagonal entry."""
    import scipy.sparse as sp
    rng = np.random.default_rng(seed)
    n = nx * ny * nz
    idx = np.arange(n)
    x, y, z = idx % nx, (idx // nx) % ny, idx // (nx * ny)
    rows, cols, vals = [idx], [idx], [6.0 + rng.random(n) if seed is not None else np.full(n, 6.0)]
    for step, ok in ((1, x < nx - 1), (nx, y < ny - 1), (nx * ny, z < nz - 1)):
        i = idx[ok]
        w = -0.5 - rng.random(i.size) if seed is not None else np.full(i.size, -1.0)
        rows += [i, i + step]
        cols += [i + step, i]
        vals += [w, w]
    S = sp.csr_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(n, n))
    S.sort_indices()
    return oracle.CSR(n, S.indptr.astype(np.int64), S.indices.astype(np.int32), S.data.astype(np.float64))


_CASES = {}


def case(grid, kind):
    """The grid's matrix and its restatement run, computed once and shared (never modified)."""
    key = (grid, kind)
    if key not in _CASES:
        A = box(*grid, seed=None if kind == "poisson" else 41 + len(_CASES))
        _CASES[key] = dict(A=A, fused=oracle.lanczos_fused(A, oracle.random_vec(A.n, 123), STEPS))
    return _CASES[key]


def upload(ctx, A):
    return eigmi.Matrix.from_bcsr(ctx, A.rowptr, A.col, A.val, flags=eigmi.MAT_NO_UNIFORM)


def fused_run(M, steps, batches=None, graph=False):
    """`steps` fused steps in the given batches (eagerly, or each batch as a captured and replayed graph):
    (alpha, beta, final pair vector, launches)."""
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
        p = ws.pairs()
        a, b = ws.tridiag()
        return a, b, p, ws.info()[1]
    finally:
        ws.close()


def same(r, s):
    return all(np.array_equal(u, v) for u, v in zip(r[:3], s[:3])) and r[3] == s[3]


def close(got, ref, rtol=1e-12):
    return np.allclose(got, ref, rtol=rtol, atol=0)


@pytest.mark.parametrize("kind", ["poisson", "variable"])
@pytest.mark.parametrize("grid", GRIDS, ids=lambda g: "x".join(map(str, g)))
def test_pipelined_body_bitwise(ctx, grid, kind):
    """Runs 1, 2, 5 x directions default / up / down / alternating: the pipelined arm (cache 64 + d) bitwise the
    plain arm (32 + d) in alpha, beta and the final pairs, and within 1e-12 of orc_lanczos_fused."""
    c = case(grid, kind)
    qa, qb = c["fused"]
    marches = grid[2] >= 4
    M = upload(ctx, c["A"])
    try:
        for runs in RUNS:
            for d in DIRS:
                M.tune(runs, march_prefetch=16, cache=32 + d)
                info = M.info
                assert (info.march_variant == 22) == marches and info.march_pipe == 0, (runs, d, info.march_variant)
                plain = fused_run(M, STEPS)
                M.tune(cache=64 + d)
                assert M.info.march_pipe == (1 if marches else 0), (runs, d)
                pipe = fused_run(M, STEPS)
                assert same(pipe, plain), (runs, d)
                assert close(pipe[0], qa) and close(pipe[1], qb), (runs, d)
    finally:
        M.close()


@pytest.mark.parametrize("d", [0, 16])
def test_batches_and_graphs(ctx, d):
    """16 steps in 4 eager batches (3, 5, 3, 5) and in 3 replayed graphs (5, 6, 5), pipelined: bitwise the plain
    body's one-batch run -- `pipe` is a kernel argument, so a captured launch replays its own body and direction."""
    M = upload(ctx, case(GRIDS[2], "variable")["A"])
    try:
        M.tune(2, march_prefetch=16, cache=32 + d)
        plain = fused_run(M, 16)
        M.tune(cache=64 + d)
        assert M.info.march_variant == 22 and M.info.march_pipe == 1
        for batches, graph in (((16,), False), ((3, 5, 3, 5), False), ((5, 6, 5), True)):
            assert same(fused_run(M, 16, batches, graph), plain), (batches, graph)
    finally:
        M.close()


def test_repairs_between_pipelined_launches(ctx):
    """+100 on a dozen diagonal entries: some predictions are unsound and those launches repair (the pipelined
    prologue's DMAs are dropped, the launch marches nothing).  Same launches and bits as the plain body."""
    A0 = case(GRIDS[2], "variable")["A"]
    A = shifted(A0, 0.0, range(0, A0.n, A0.n // 12), 1e2)
    M = upload(ctx, A)
    try:
        for runs in (0, 2):
            M.tune(runs, march_prefetch=16, cache=32)
            plain = fused_run(M, 16)
            assert plain[3] > 17  # (16 steps + the final forced repair + repairs in between)
            M.tune(cache=64)
            assert M.info.march_variant == 22 and M.info.march_pipe == 1
            assert same(fused_run(M, 16), plain), runs
            assert same(fused_run(M, 16, (5, 6, 5), True), plain), runs
    finally:
        M.close()


def test_after_diagonal_shift(ctx):
    """A += sigma I rebuilds the value pack the DMAs read: pipelined bitwise plain, within 1e-12 of the
    restatement on the shifted matrix."""
    A0 = case(GRIDS[2], "variable")["A"]
    sigma = 0.375
    qa, qb = oracle.lanczos_fused(shifted(A0, sigma), oracle.random_vec(A0.n, 123), STEPS)
    M = upload(ctx, A0)
    try:
        M.tune(2, march_prefetch=16, cache=64)
        before = fused_run(M, STEPS)
        M.shift_diag(sigma)
        assert M.info.march_variant == 22 and M.info.march_pipe == 1
        pipe = fused_run(M, STEPS)
        M.tune(cache=32)
        assert same(pipe, fused_run(M, STEPS))
        assert close(pipe[0], qa) and close(pipe[1], qb)
        assert not np.array_equal(pipe[0], before[0])
    finally:
        M.close()


SLAB_GRID, SLAB_RANKS = (64, 4, 15), 3  # 5 planes per rank: the middle rank touches neither end of the grid


def test_pipelined_on_slabs(ctx):
    """MarchPlan::gz0 and MarchPlan::zb not zero: 64 x 4 x 15 as 3 z-slabs over the in-process loopback transport,
    split launches (interior planes, zb = 1) and whole launches (halo first): on every rank the pipelined arm
    bitwise the plain one in every direction, within 1e-12 of orc_lanczos_fused."""
    c = case(SLAB_GRID, "variable")
    A, P = c["A"], SLAB_RANKS
    D, nz = SLAB_GRID[0] * SLAB_GRID[1], SLAB_GRID[2]
    hub = eigmi.loopback_create(P)
    out = [None] * P

    def rank(r):
        rc = eigmi.Context(0)
        res = {"runs": {}}
        try:
            rc.comm_init_loopback(hub, r)
            b, e = nz * r // P * D, nz * (r + 1) // P * D
            lo, hi = A.rowptr[b], A.rowptr[e]
            M = eigmi.Matrix.from_rows(rc, A.n, b, A.rowptr[b:e + 1] - lo, A.col[lo:hi], A.val[lo:hi])
            M.tune(march_prefetch=16)
            for halo in (0, 1):
                for d in DIRS:
                    for arm in (32, 64):
                        M.tune(halo_whole=halo, cache=arm + d)
                        info = M.info
                        res["runs"][halo, d, arm] = (int(info.march_variant), int(info.march_pipe), fused_run(M, STEPS))
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
        for (halo, d, arm), (variant, pipe, run) in res["runs"].items():
            assert variant == 22 and pipe == (1 if arm == 64 else 0), (r, halo, d, arm, variant, pipe)
            if arm == 64:
                assert same(run, res["runs"][halo, d, 32][2]), (r, halo, d)
                assert close(run[0], qa) and close(run[1], qb), (r, halo, d)


def test_default_plan_pipelines_wide_planes(ctx):
    """256 x 256 x 8 with the cache bits at their default: two plane runs on 1,024-column planes are one
    workgroup per CU, so the plan takes the pipelined body by itself; bitwise the never-pipeline arm."""
    A = box(256, 256, 8)
    qa, qb = oracle.lanczos_fused(A, oracle.random_vec(A.n, 123), STEPS)
    M = upload(ctx, A)
    try:
        M.tune(march_prefetch=16, cache=0)
        assert M.info.march_variant == 22 and M.info.march_pipe == 1
        pipe = fused_run(M, STEPS)
        M.tune(cache=32)
        assert M.info.march_pipe == 0
        assert same(pipe, fused_run(M, STEPS))
        assert close(pipe[0], qa) and close(pipe[1], qb)
    finally:
        M.close()
