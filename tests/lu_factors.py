"""General LU factors in the exported (UMFPACK) form -- test infrastructure only (imported like
box_grids.py).  make() returns the dict eigmi.LU.from_factors(ctx, **d) and oracle.LU(**d) take:
unit-lower L by rows with the unit diagonal last, U by columns with the pivot last, random P != Q,
Rs in [0.5, 2], do_recip either way.  Unlike the project's own envelope LU the factors have
unsymmetric patterns, sparse rows with far entries, empty rows and chosen widths / distances, so
they reach the edges of the three device paths of eig_inverse_mv8 (csrc/k_trsv.hip).

The factors are contractive: the off-diagonal |entries| of an L row sum to <= 0.5, those of a U
row to <= 0.5 |pivot|.  Solutions then stay O(1 / pivot) and an error is amplified by at most 2
through the chain.

CASES lists every factor set the GPU tests feed the device, with the kernel eig_lu_solver_info
must report for it; the CPU tests anchor the oracle on each of them (residual_ratio) and check the
expectation against Python restatements of the upload's admission rules (expected_solver)."""
import functools

import numpy as np

import oracle

TB = 64            # rows per block of the device solves (kTB)
RING4 = 4          # blocks the staged kernel keeps in its ring (kRing4)
SLAB = 128         # outside entries per row the staged image holds (kSlab)
BINV_MAX_GD = 8    # coupled blocks the block-inverse image allows (kBinvMaxGD)
BINV_COND = 1e6    # its gate on max|D| max|inv D| 64 per diagonal block (kBinvCond)
U53 = 2.0 ** -53
# The block-inverse solve multiplies by inv(D_b) instead of substituting: agreement with the
# reference arithmetic to rounding.  Bound: 1e-13 of the largest |entry| of the result.
BINV_RTOL = 1e-13


def _values(rng, k, bound):
    """k entries of random sign whose |.| sum to at most bound (and to at least 0.3 bound)."""
    mag = rng.uniform(0.5, 1.0, k)
    return rng.choice([-1.0, 1.0], k) * mag * (bound * rng.uniform(0.6, 1.0) / mag.sum())


def _outside_candidates(lower, b, n, reach, dist):
    """Columns outside block b a row of it may hold: the blocks at the distances in dist (default
    1 .. reach) before (L) / after (U) it."""
    nb = (n + TB - 1) // TB
    cols = []
    for d in sorted(dist if dist is not None else range(1, reach + 1)):
        src = b - d if lower else b + d
        if 0 <= src < nb:
            cols.append(np.arange(src * TB, min(n, src * TB + TB)))
    cols = np.concatenate(cols) if cols else np.zeros(0, np.int64)
    return np.sort(cols)


def _inblock(rng, lower, i, n, mode):
    bs = i // TB * TB
    tri = np.arange(bs, i) if lower else np.arange(i + 1, min(n, bs + TB))
    if mode == "full":
        return tri
    if mode == "none":
        return tri[:0]
    if mode == "col0":   # the tile's column 0 (L rows 1 .. 63 of a block; no U row has it)
        return tri[tri == bs]
    if mode == "col63":  # the tile's column 63 (U rows 0 .. 62 of a full block; no L row has it)
        return tri[tri == bs + TB - 1]
    assert mode == "random", mode
    return tri[rng.random(tri.size) < 0.25]


def _pattern(rng, lower, n, reach, width, inblock, dist, bare_blocks, rows):
    """Per row the stored off-diagonal columns, ascending.  Row 0 of every block is as wide as
    allowed and holds the farthest admissible column (so the coupled-block count is the reach
    exactly); row 9 of every block is empty; the others draw a width in [0, width]."""
    pat = []
    for i in range(n):
        b, r = divmod(i, TB)
        if rows is not None and i in rows:
            pat.append(np.sort(np.asarray(rows[i], np.int64)))
            continue
        if r == 9:
            pat.append(np.zeros(0, np.int64))
            continue
        cand = _outside_candidates(lower, b, n, reach, dist)
        if b in bare_blocks:
            cand = cand[:0]
        wmax = min(width, cand.size)
        if r == 0 and wmax > 0:
            far = cand[0] if lower else cand[-1]
            rest = cand[1:] if lower else cand[:-1]
            out = np.append(rng.choice(rest, wmax - 1, replace=False), far)
        else:
            out = rng.choice(cand, rng.integers(0, wmax + 1), replace=False)
        pat.append(np.sort(np.concatenate([out, _inblock(rng, lower, i, n, inblock)])).astype(np.int64))
    return pat


def make(n, seed=0, reach=(0, 0), width=(0, 0), pivots=(1.0, 2.0), do_recip=0, inblock=("random", "random"),
         dist=(None, None), bare_blocks=(), rows_l=None, rows_u=None, pivot_at=None, shuffle_u=False,
         l_descending=False):
    """The factor dict.  Per factor (L, U): reach = blocks of 64 rows an outside-the-block entry of
    row i may lie away from block i / 64, width = the most outside entries a row draws, dist = the
    admitted block distances (default 1 .. reach), inblock = "random" | "full" | "none" | "col0" |
    "col63".  bare_blocks: blocks whose rows get no outside entry in either factor.  rows_l /
    rows_u: {row: columns} overwrite the whole off-diagonal pattern of chosen rows.  pivots: the
    range the U diagonal is drawn from (log-uniform), pivot_at: {row: value} overrides.  shuffle_u:
    random entry order inside each U column (pivot last); l_descending: L rows stored in
    descending column order (unit diagonal last)."""
    rng = np.random.default_rng(seed)
    lo, hi = pivots
    piv = np.exp(rng.uniform(np.log(lo), np.log(hi), n))
    for i, v in (pivot_at or {}).items():
        piv[i] = v
    lpat = _pattern(rng, True, n, reach[0], width[0], inblock[0], dist[0], bare_blocks, rows_l)
    upat = _pattern(rng, False, n, reach[1], width[1], inblock[1], dist[1], bare_blocks, rows_u)
    Lp, Lj, Lx = [0], [], []
    for i in range(n):
        c = lpat[i]
        assert c.size == np.unique(c).size and (c.size == 0 or (c[0] >= 0 and c[-1] < i)), ("L row", i)
        v = _values(rng, c.size, 0.5) if c.size else np.zeros(0)
        if l_descending:
            c, v = c[::-1], v[::-1]
        Lj += [c, [i]]
        Lx += [v, [1.0]]
        Lp.append(Lp[-1] + c.size + 1)
    cols = [[] for _ in range(n)]  # U by columns: (row, value) above the pivot
    for i in range(n):
        c = upat[i]
        assert c.size == np.unique(c).size and (c.size == 0 or (c[0] > i and c[-1] < n)), ("U row", i)
        v = _values(rng, c.size, 0.5 * abs(piv[i])) if c.size else np.zeros(0)
        for j, x in zip(c, v):
            cols[j].append((i, x))
    Up, Ui, Ux = [0], [], []
    for j in range(n):
        e = cols[j]
        if shuffle_u and len(e) > 1:
            e = [e[k] for k in rng.permutation(len(e))]
        Ui += [[q[0] for q in e], [j]]
        Ux += [[q[1] for q in e], [piv[j]]]
        Up.append(Up[-1] + len(e) + 1)
    cat = lambda parts, t: np.concatenate([np.asarray(p, t) for p in parts]) if parts else np.zeros(0, t)
    P, Q = rng.permutation(n), rng.permutation(n)
    return {"Lp": np.asarray(Lp, np.int64), "Lj": cat(Lj, np.int64), "Lx": cat(Lx, np.float64),
            "Up": np.asarray(Up, np.int64), "Ui": cat(Ui, np.int64), "Ux": cat(Ux, np.float64),
            "P": P.astype(np.int64), "Q": Q.astype(np.int64), "Rs": rng.uniform(0.5, 2.0, n), "do_recip": int(do_recip)}


# ------------------------------------------------------------------ restatements of the factors
def dense_factors(d, dtype=np.float64):
    """(L, U) dense, duplicates summed."""
    n = d["Lp"].size - 1
    L, U = np.zeros((n, n), dtype), np.zeros((n, n), dtype)
    np.add.at(L, (np.repeat(np.arange(n), np.diff(d["Lp"])), d["Lj"]), d["Lx"].astype(dtype))
    np.add.at(U, (d["Ui"], np.repeat(np.arange(n), np.diff(d["Up"]))), d["Ux"].astype(dtype))
    return L, U


def row_widths(d):
    """(w_L, w_U): the largest stored row widths of L and of U by rows, diagonals included."""
    n = d["Lp"].size - 1
    return int(np.diff(d["Lp"]).max()), int(np.bincount(d["Ui"], minlength=n).max())


def outside_stats(d):
    """Per factor (L, U): (coupled blocks, most outside-the-block entries of a row)."""
    n = d["Lp"].size - 1
    out = []
    for rows, colsidx in ((np.repeat(np.arange(n), np.diff(d["Lp"])), d["Lj"]),
                          (d["Ui"], np.repeat(np.arange(n), np.diff(d["Up"])))):
        far = np.abs(rows // TB - colsidx // TB)
        outside = far > 0
        out.append((int(far.max(initial=0)), int(np.bincount(rows[outside], minlength=n).max(initial=0))))
    return out


def gate_estimate(d):
    """The upload's conditioning estimate max |D_b| max |inv D_b| 64 over the diagonal blocks of
    both factors (rows past n: identity padding)."""
    n = d["Lp"].size - 1
    worst = 0.0
    for F in dense_factors(d):
        for bs in range(0, n, TB):
            D = np.eye(TB)
            k = min(TB, n - bs)
            D[:k, :k] = F[bs:bs + k, bs:bs + k]
            worst = max(worst, np.abs(D).max() * np.abs(np.linalg.inv(D)).max() * TB)
    return worst


def expected_solver(d):
    """What eig_lu_solver_info must report, from the admission rules of the upload: the
    block-inverse image for <= 8 coupled blocks and well-conditioned diagonal blocks, else the
    staged image for <= 128 outside entries per row within 4 blocks, else the row-CSR kernel.
    Two rules of the upload are left out, neither reachable at these sizes and pivots: the
    kBinvTiles limit on the image's size and the refusal of the image for a zero U pivot."""
    (gl, wl), (gu, wu) = outside_stats(d)
    if max(gl, gu) <= BINV_MAX_GD and gate_estimate(d) <= BINV_COND:
        return "blockinv", gl, gu
    if max(gl, gu) <= RING4 and max(wl, wu) <= SLAB:
        return "staged", gl, gu
    return "csr", gl, gu


def residual_ratio(d, X, out, m):
    """max over the entries of |L (U y) - b| / ((w_L + w_U + 3) 2^-53 |L| |U| |y| + 2^-53 |b|) in
    numpy.longdouble, with b[k] = scale_k X[P[k]] and y[j] = out[Q[j]]: the backward-error bound
    of two substitutions plus the row scaling.  <= 1 for a solve that is backward stable row by
    row, whatever it was compared with."""
    ld = np.longdouble
    n = d["Lp"].size - 1
    L, U = dense_factors(d, ld)
    Xc, Oc = oracle.mv_to_cols(X, n, m).astype(ld), oracle.mv_to_cols(out, n, m).astype(ld)
    Rs = d["Rs"].astype(ld)[d["P"]]
    b = Xc[d["P"]] * (Rs if d["do_recip"] else 1 / Rs)[:, None]
    y = Oc[d["Q"]]
    res = np.abs(L @ (U @ y) - b)
    wl, wu = row_widths(d)
    bound = (wl + wu + 3) * ld(U53) * (np.abs(L) @ (np.abs(U) @ np.abs(y))) + ld(U53) * np.abs(b)
    assert np.all(bound > 0) or n == 0
    return float((res / bound).max())


# ------------------------------------------------------------------------------- the case table
def _gate(block=0):
    """Pivots 1e-3 and 1e3 in one 64-row block of U: max |D| max |inv D| 64 >= 6.4e7 > kBinvCond
    whatever the other entries are (the inverse of a triangular block has 1 / d on its diagonal),
    so the block-inverse image is refused."""
    return {block * TB + 2: 1e-3, block * TB + 3: 1e3}


def _outside(n, lower, i, count, dists=(1, 2, 3, 4), seed=0):
    """count columns outside block i / 64, spread over the blocks at the given distances."""
    cand = _outside_candidates(lower, i // TB, n, 0, dists)
    assert cand.size >= count, (i, count, cand.size)
    return np.random.default_rng(seed + i).choice(cand, count, replace=False)


def _width_rows(n, lower, block):
    """Rows 0 .. 7 of one block with 0, 1, 7, 8, 9, 120, 127 and 128 outside entries, the odd ones
    with an in-block entry as well."""
    rows = {}
    for r, w in enumerate((0, 1, 7, 8, 9, 120, 127, 128)):
        i = block * TB + r
        inb = [i - 1] if lower and r % 2 else ([i + 1] if not lower and r % 2 else [])
        rows[i] = np.concatenate([_outside(n, lower, i, w), np.asarray(inb, np.int64)])
    return rows


def _mixed_rows(n, lower, rows_widths):
    """Rows with exactly the given numbers of outside entries, half of them in the 3 blocks next to
    the row's own (the LDS ring of k_tsolve), half further away (global reads).  The device reads a
    row in column order (L ascending, U descending), so the far entries all come before the near
    ones: the 32-entry load round at that boundary mixes the two kinds of read, the others hold
    one kind."""
    rows = {}
    for i, w in rows_widths:
        b, nb = i // TB, (n + TB - 1) // TB
        near = w // 2
        far_d = [dd for dd in range(4, 10) if 0 <= (b - dd if lower else b + dd) < nb]
        rows[i] = np.concatenate([_outside(n, lower, i, near, (1, 2, 3)), _outside(n, lower, i, w - near, far_d, 7)])
    return rows


N5 = 5 * TB + 17  # 337: five full blocks and a ragged one
N6 = 6 * TB + 17
STAGED4 = dict(reach=(4, 4), width=(128, 128), pivot_at=_gate())


def _cases():
    C = {}

    def add(name, m, expect, check, **kw):
        C[name] = dict(kw=kw, m=m, expect=expect, check=check)

    # ---- C1: the staged kernel (block-inverse image refused by the pivots of one block)
    for rec in (0, 1):
        for m in (8, 24):
            add(f"staged_random_recip{rec}_m{m}", m, ("staged", 4, 4), "bitwise", n=N5, seed=10 + rec,
                pivots=(1e-3, 1e3), do_recip=rec, **STAGED4)
    add("staged_widths", 24, ("staged", 4, 4), "bitwise", n=N6 + TB, seed=12, reach=(4, 4), width=(9, 9),
        pivot_at=_gate(), rows_l=_width_rows(N6 + TB, True, 4), rows_u=_width_rows(N6 + TB, False, 1))
    add("staged_width0_block", 8, ("staged", 4, 4), "bitwise", n=N6, seed=13, bare_blocks=(3,), **STAGED4)
    add("staged_dist4", 24, ("staged", 4, 4), "bitwise", n=N6 + 2 * TB, seed=14, dist=({4}, {4}), **STAGED4)
    add("staged_dist_mix", 8, ("staged", 4, 4), "bitwise", n=N6, seed=15, reach=(4, 4), width=(12, 12),
        pivot_at=_gate())
    for mode in ("full", "col0", "col63", "none"):
        add(f"staged_tile_{mode}", 8, ("staged", 4, 4), "bitwise", n=N5, seed=16, inblock=(mode, mode), **STAGED4)
    for r in (1, 7, 8, 9, 63):
        add(f"staged_ragged_{r}", 8, ("staged", 4, 4), "bitwise", n=4 * TB + r, seed=20 + r, **STAGED4)
    add("staged_n64", 24, ("staged", 0, 0), "bitwise", n=TB, seed=30, **STAGED4)
    # n = 1: the rows past n pad the diagonal block with the identity, so the gate's estimate is
    # 64 max(1, |d|) max(1, 1 / |d|) = 6.4e6 for the pivot 1e-5
    add("staged_n1", 8, ("staged", 0, 0), "bitwise", n=1, seed=35, pivot_at={0: 1e-5})
    add("staged_unsym_l1_u4", 8, ("staged", 1, 4), "bitwise", n=N5, seed=31, reach=(1, 4), width=(3, 128),
        pivot_at=_gate())
    add("staged_unsym_l4_u1", 24, ("staged", 4, 1), "bitwise", n=N5, seed=32, reach=(4, 1), width=(128, 3),
        pivot_at=_gate())
    add("staged_u_shuffled", 8, ("staged", 4, 4), "bitwise", n=N5, seed=33, shuffle_u=True, **STAGED4)
    add("staged_l_descending", 8, ("staged", 4, 4), "rounding", n=N5, seed=34, l_descending=True, **STAGED4)
    # not admitted to the staged image, still refused by the block-inverse gate: the row-CSR kernel
    i_l, i_u = 5 * TB + 20, TB + 20
    add("refused_l_row129", 8, ("csr", 4, 4), "bitwise", n=N6, seed=40,
        rows_l={i_l: _outside(N6, True, i_l, 129)}, **STAGED4)
    add("refused_u_row129", 8, ("csr", 4, 4), "bitwise", n=N6, seed=41,
        rows_u={i_u: _outside(N6, False, i_u, 129)}, **STAGED4)
    add("refused_l_5back", 8, ("csr", 5, 4), "bitwise", n=N6, seed=42, rows_l={i_l: np.array([7, i_l - 3])}, **STAGED4)
    add("refused_u_5ahead", 8, ("csr", 4, 5), "bitwise", n=N6, seed=43,
        rows_u={20: np.array([21, 5 * TB + 7])}, **STAGED4)
    # ---- C2: the row-CSR kernel on sparse factors that reach past the block-inverse image
    n9 = 9 * TB + 24
    lw = [(8 * TB + 1, 31), (8 * TB + 2, 32), (8 * TB + 3, 33), (8 * TB + 4, 65), (9 * TB + 1, 33), (9 * TB + 20, 65)]
    uw = [(1, 31), (2, 32), (3, 33), (4, 65), (TB + 1, 33), (TB + 20, 65)]
    for m in (8, 24):
        add(f"csr_reach9_m{m}", m, ("csr", 9, 9), "bitwise", n=n9, seed=50, reach=(9, 9), width=(40, 40),
            rows_l=_mixed_rows(n9, True, lw), rows_u=_mixed_rows(n9, False, uw))
    # ---- C3: the block-inverse chain, every template, on benign general factors
    add("binv_n1", 8, ("blockinv", 0, 0), "binv", n=1, seed=60)
    add("binv_0_0_n40", 8, ("blockinv", 0, 0), "binv", n=40, seed=61)
    add("binv_0_0_blockdiag", 24, ("blockinv", 0, 0), "binv", n=3 * TB, seed=62)
    for (gl, gu), n, m in (((1, 6), 7 * TB + 13, 8), ((2, 2), 3 * TB + 5, 24), ((3, 4), 5 * TB + 30, 24),
                           ((5, 8), 9 * TB + 10, 8), ((8, 1), 9 * TB + 10, 24)):
        add(f"binv_{gl}_{gu}", m, ("blockinv", gl, gu), "binv", n=n, seed=63 + gl, reach=(gl, gu), width=(40, 40))
    add("csr_9_1", 8, ("csr", 9, 1), "bitwise", n=10 * TB + 3, seed=70, reach=(9, 1), width=(40, 40))
    return C


CASES = _cases()
# the shapes the generator was first tried at (n, reach, width, pivots): CPU only
EXTRA = {"gen_1": dict(n=1), "gen_63": dict(n=63, width=(20, 20)),
         "gen_450": dict(n=450, reach=(7, 7), width=(200, 200)), "gen_600": dict(n=600, reach=(9, 9), width=(40, 40))}


@functools.lru_cache(maxsize=None)
def case(name):
    """-> (factor dict, X, m, oracle result): built once, shared by the tests, never written to."""
    c = CASES[name] if name in CASES else dict(kw=EXTRA[name], m=8)
    d = make(**c["kw"])
    n = d["Lp"].size - 1
    X = oracle.random_mv8(n, c["m"], 11)
    ref, _ = oracle.inverse_mv8(oracle.LU(**d), X, c["m"])
    for a in list(d.values()) + [X, ref]:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return d, X, c["m"], ref
