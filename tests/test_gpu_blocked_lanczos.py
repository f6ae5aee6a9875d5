"""The Lanczos recurrence on blocked matrices (BCRSMatrix<FieldMatrix<double,b,b>>, b = 2, 3, 4, one
rank): the two-kernel step (k_lanczos_spmv_blk + k_lanczos_update) and the guarded one-reduction step
(k_lanczos_fused_blk) through the workspace API (eig_lanczos_create_ex / _step / _capture / _replay /
_tridiag) and eig_lanczos_run.

References: the oracle on the matrix's SCALAR EXPANSION (tests/test_gpu_blocked_spmm.py: the blocked
row product is bitwise the 1x1 product on it) -- oracle.lanczos for the two-kernel step,
oracle.lanczos_fused(with_launches=True) for the fused one.  Start vectors: mt19937(123) normal
numbers on both sides.  Only the order of the grid reductions differs from the oracle, so the bar is
the project's rule of tests/test_gpu_fused_guard.py: relative, on alpha and beta,
tol = max(1e-12, 4 x the classic recurrence's own run-to-run spread), the spread computed by the
oracle (fused_ref.classic_spread).

Matrices are the smallest that reach every branch: the scaled S A S of q1elast(5) (125 block rows, 2
slices, the second with 61 rows; plain q1elast(5) has a degenerate spectrum and a spread of 3e-8 at
40 steps); bitwise-symmetric random 2x2 / 4x4 patterns on 130 block rows (3 slices, the last with 2
rows, block row 5 empty); S A S with outliers (repairs) and shifted by 1e6 (mu from the blocked
diagonal share); q1elast(52), whose 2,197 slices exceed the launcher's 2,048 workgroups."""
import numpy as np
import pytest

import eigmi
import oracle
from fused_ref import classic, classic_spread, shifted
from test_gpu_blocked_drivers import mats
from test_gpu_blocked_spmm import case, expand

pytestmark = pytest.mark.gpu

# EIG_LANCZOS_AUTO on blocked images (fused_step_pays)
AUTO_ON_BLOCKS = "classic"


def up(ctx, A):
    return eigmi.Matrix.from_bcsr(ctx, A.rowptr, A.col, A.val, A.br, A.bc)


def run(M, steps, fused, batches=1, graph=False):
    """(alpha, beta, launches) of `steps` steps in `batches` eager or captured batches."""
    ws = eigmi.LanczosWorkspace(M, steps, seed=123, fused=fused)
    try:
        per = steps // batches
        done = 0
        while done < steps:
            k = min(per, steps - done)
            if graph:
                ws.capture(k)
                ws.replay()
            else:
                ws.step(k)
            done += k
        a, b = ws.tridiag()
        return a, b, ws.info()[1]
    finally:
        ws.close()


def rel(got, ref):
    return float(np.max(np.abs(got - ref) / np.abs(ref)))


def check_both(M, E, steps, tol, tag):
    """both step forms against their oracles on the expansion E; returns the fused launch counts"""
    u0 = oracle.random_vec(E.n, 123)
    _, ra, rb = oracle.lanczos(E, u0, steps)
    a, b, L = run(M, steps, False)
    print(f"{tag} classic: max rel alpha {rel(a, ra):.2e} beta {rel(b, rb):.2e} (tol {tol:.2e})")
    assert L == steps
    assert np.all(np.abs(a - ra) <= tol * np.abs(ra)) and np.all(np.abs(b - rb) <= tol * np.abs(rb))
    oa, ob, oL = oracle.lanczos_fused(E, u0, steps, with_launches=True)
    fa, fb, fL = run(M, steps, True)
    print(f"{tag} fused: max rel alpha {rel(fa, oa):.2e} beta {rel(fb, ob):.2e}, launches {fL} (oracle {oL})")
    assert np.all(np.abs(fa - oa) <= tol * np.abs(oa)) and np.all(np.abs(fb - ob) <= tol * np.abs(ob))
    return fL, oL


def spread_tol(E, steps):
    u0 = oracle.random_vec(E.n, 123)
    _, cb = classic(E, u0, steps)
    return max(1e-12, 4 * classic_spread(E, u0, steps, cb))


def symmetric_bcsr(b, nb=130, seed=2):
    """Bitwise-symmetric blocked matrix: diagonal blocks G + G^T + 4 I, block (I, J) the transpose of
    (J, I), up to 4 random partners among the next 24 block rows (the same pattern for every b:
    0..13 blocks per row); block row / column 5 empty."""
    rng, pat = np.random.default_rng(seed), np.random.default_rng(seed + 100)
    blocks = {}
    for I in range(nb):
        if I == 5:
            continue
        G = rng.standard_normal((b, b))
        blocks[(I, I)] = G + G.T + 4.0 * np.eye(b)
        cand = np.array([J for J in range(I + 1, min(nb, I + 25)) if J != 5])
        k = min(int(pat.integers(0, 5)), cand.size)
        for J in pat.choice(cand, k, replace=False) if k else ():
            G = rng.standard_normal((b, b))
            blocks[(I, int(J))] = G
            blocks[(int(J), I)] = G.T.copy()
    keys = sorted(blocks)
    cnt = np.bincount([I for I, _ in keys], minlength=nb)
    rowptr = np.zeros(nb + 1, np.int64)
    np.cumsum(cnt, out=rowptr[1:])
    col = np.array([J for _, J in keys], np.int32)
    val = np.concatenate([blocks[k].reshape(-1) for k in keys])
    return oracle.CSR(nb, rowptr, col, val, b, b)


def with_outliers(S, rows, add):
    """S (3x3 blocked) with `add` on the diagonal entries of the scalar rows `rows`"""
    v = S.val.copy()
    for i in rows:
        I, r = divmod(i, 3)
        p = S.rowptr[I] + int(np.flatnonzero(S.col[S.rowptr[I]:S.rowptr[I + 1]] == I)[0])
        v[p * 9 + r * 3 + r] += add
    return oracle.CSR(S.nrows, S.rowptr, S.col, v, 3, 3)


# ------------------------------------------------------------------------------- 1. 3x3, both forms
def test_q1elast5_scaled_both_forms(ctx):
    d = mats()
    S, E = d["S"], d["ES"]
    M = up(ctx, S)
    assert M.info.nslices == 2 and (M.info.br, M.info.bc) == (3, 3) and E.n == 375
    tol = spread_tol(E, 40)
    assert tol == 1e-12  # (spread 1.5e-15 at 40 steps)
    fL, oL = check_both(M, E, 40, tol, "SAS q1elast(5) 40 steps")
    assert fL == oL == 41  # 40 steps + the forced final repair
    M.close()


# ---------------------------------------------------------------------------------- 2. 2x2 and 4x4
@pytest.mark.parametrize("b", [2, 4])
def test_random_symmetric_pattern(ctx, b):
    A = symmetric_bcsr(b)
    E = expand(A.rowptr, A.col, A.val, b)
    D = E.to_scipy().toarray()
    assert np.array_equal(D, D.T)
    assert A.rowptr[5] == A.rowptr[6] and np.diff(A.rowptr).max() <= 13
    M = up(ctx, A)
    assert M.info.nslices == 3 and M.info.n == 130 * b
    check_both(M, E, 24, spread_tol(E, 24), f"random {b}x{b} 24 steps")
    M.close()


# ------------------------------------------------------------------------- 3. repairs and batching
def test_repairs_and_batches(ctx):
    """+1e3 on 13 diagonal entries makes some predictions unsound: those launches repair.  The same
    decisions as the oracle, values within tol; 4 eager batches (host top-up launches after each)
    and 3 captured / replayed batches are bitwise the one-batch run."""
    S = mats()["S"]
    n = S.n
    A = with_outliers(S, range(0, n, n // 12), 1e3)
    E = expand(A.rowptr, A.col, A.val, 3)
    assert np.array_equal(E.val, shifted(mats()["ES"], 0.0, range(0, n, n // 12), 1e3).val)
    M = up(ctx, A)
    tol = spread_tol(E, 16)
    fL, oL = check_both(M, E, 16, tol, "SAS + 1e3 outliers 16 steps")
    assert fL == oL and fL > 17
    a, b, L = run(M, 16, True)
    for batches, graph in ((4, False), (3, True)):
        a2, b2, L2 = run(M, 16, True, batches, graph)
        assert np.array_equal(a2, a) and np.array_equal(b2, b)
    ca, cb, _ = run(M, 16, False)
    for batches, graph in ((4, False), (3, True)):
        a2, b2, _ = run(M, 16, False, batches, graph)
        assert np.array_equal(a2, ca) and np.array_equal(b2, cb)
    M.close()


# ----------------------------------------------------------------------------------------- 4. shift
def test_shifted_by_1e6(ctx):
    """Matrix.shift_diag(1e6) on the blocked device matrix: the fused step runs on A - mu I with
    mu = trace / n from the blocked diag_sum / diag_count; against the classic recurrence on the
    expansion + 1e6 I."""
    d = mats()
    M = up(ctx, d["S"])
    M.shift_diag(1e6)
    E = shifted(d["ES"], 1e6)
    u0 = oracle.random_vec(E.n, 123)
    ca, cb = classic(E, u0, 24)
    tol = max(1e-12, 4 * classic_spread(E, u0, 24, cb))
    a, b, L = run(M, 24, True)
    print(f"SAS + 1e6 I fused vs classic: max rel alpha {rel(a, ca):.2e} beta {rel(b, cb):.2e} (tol {tol:.2e}), "
          f"launches {L}")
    assert np.all(np.abs(a - ca) <= 1e-12 * np.abs(ca))
    assert np.all(np.abs(b - cb) <= tol * np.abs(cb))
    assert L == oracle.lanczos_fused(E, u0, 24, with_launches=True)[2]
    M.close()


# ----------------------------------------------------------------------------------- 5. grid-stride
def test_grid_stride(ctx):
    A, E = case("q1elast52")
    M = up(ctx, A)
    assert M.info.nslices == 2197 > 2048
    check_both(M, E, 10, 1e-12, "q1elast(52) 10 steps")
    M.close()


# ------------------------------------------------------------------ 6. kernel info, bytes and auto
def test_kernel_info_bytes_and_auto(ctx):
    S = mats()["S"]
    M = up(ctx, S)
    assert M.kernel("k1") == "k_lanczos_spmv_blk" and M.kernel("fused") == "k_lanczos_fused_blk"
    info = M.info
    b, n = info.br, info.n
    image = (8 * b * b + 4) * info.nnzb_padded + 8 * (info.nslices + 1)
    assert M.lanczos_kernel_info(True) == ("k_lanczos_fused_blk", image + 32 * n)
    assert M.lanczos_kernel_info(False) == ("k_lanczos_spmv_blk", image + 24 * n)
    got = {}
    for fused in (False, True, "auto"):
        ws = eigmi.LanczosWorkspace(M, 12, seed=123, fused=fused)
        ws.step(12)
        got[fused] = (ws.variant, ws.kernel, ws.kernel_bytes) + ws.tridiag()
        ws.close()
    assert got[False][:3] == ("classic", "k_lanczos_spmv_blk", image + 24 * n)
    assert got[True][:3] == ("fused", "k_lanczos_fused_blk", image + 32 * n)
    want = got[AUTO_ON_BLOCKS == "fused"]
    assert got["auto"][:3] == want[:3]
    assert np.array_equal(got["auto"][3], want[3]) and np.array_equal(got["auto"][4], want[4])
    M.close()


# ------------------------------------------------------------------------------------ 7. boundaries
def test_boundaries(ctx):
    nb = 6
    rowptr = np.arange(nb + 1, dtype=np.int64)
    col = np.arange(nb, dtype=np.int32)
    M23 = eigmi.Matrix.from_bcsr(ctx, rowptr, col, np.ones(nb * 6), 2, 3, ncols_blocks=nb)
    M33 = up(ctx, mats()["S"])
    for call in (lambda: eigmi.LanczosWorkspace(M23, 4),
                 lambda: eigmi.LanczosWorkspace(M23, 4, fused=True),
                 lambda: eigmi.lanczos_run(M23, 4),
                 lambda: eigmi.lanczos_run(M23, 4, fused=True),
                 lambda: eigmi.LanczosWorkspace(M33, 4, pipelined=True),
                 lambda: eigmi.lanczos_run(M33, 4, pipelined=True)):
        with pytest.raises(eigmi.EigShapeError) as e:
            call()
        assert e.value.code == eigmi.EIG_ERR_BLOCKSIZE
    # the same calls on the square blocks run (eig_lanczos_run is create + step + tridiag)
    for fused in (False, True):
        a, b, _ = eigmi.lanczos_run(M33, 4, fused=fused)
        wa, wb, _ = run(M33, 4, fused)
        assert np.array_equal(a, wa) and np.array_equal(b, wb) and np.all(b > 0)
    M23.close(), M33.close()
