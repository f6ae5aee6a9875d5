"""Poisoned inputs and guarded buffers for the sparse products -- test infrastructure only (imported
like box_grids.py).

The invariant under test: y[r] is a function of x[c] for the STORED (r, c) only, and a launch writes
nothing but the owned rows of its output.  Most product kernels load unconditionally from a clamped
address and then gate, select, or multiply by an exact +0; with finite x a wrong gate gives
0 * finite = 0 and every bitwise test still passes.  Here some x[c] are +Inf / NaN, chosen so that

    a row is TAINTED   when it stores a column of the poison set J (its reference sum is non-finite),
    a row is a WITNESS when it is untainted and one of its FALSE ADDRESSES -- what a careless kernel
                       could read for it: the clamped position of an offset the row does not store,
                       column 0, the last column, its own index -- lies in J:

a witness's reference sum is finite, and a kernel that lets the false address into the sum makes it
NaN (0 * Inf, 0 * NaN).  Buffers carry guard bands: NaN around the inputs, one sentinel bit pattern
over the outputs, so that a read past an end poisons and a stray write shows."""
import numpy as np

import oracle

SENTINEL = np.uint64(0x7FF85EED0BADC0DE)  # a quiet NaN with a payload no arithmetic produces
PAGE = 4096
FACES = ("x-", "x+", "y-", "y+", "z-", "z+")


# ---- guarded device buffers ----

def layout(base, n, guard=512):
    """(lead, total) in doubles for a payload of n doubles in a buffer at byte address `base`: at
    least `guard` doubles before and after it and the payload on a 4 KiB boundary.  total does not
    depend on base (the buffer is allocated before its address is known)."""
    assert base % 8 == 0 and guard >= 0
    lead = guard + ((-(base + 8 * guard)) % PAGE) // 8
    return lead, n + 2 * guard + PAGE // 8 - 1


class _Ptr:
    """What the eigmi wrappers take for a device vector: an object with .ptr."""

    def __init__(self, ptr):
        self.ptr = ptr


class Guarded:
    """A device buffer with guard bands around its payload.  .ptr / .vec address the payload, .buf is
    the whole DeviceArray, .image the host copy of what was uploaded (whole buffer)."""

    def __init__(self, ctx, n, guard, fill_bits, host=None):
        total = layout(0, n, guard)[1]
        self.buf = ctx.empty(total)
        self.n, self.guard = int(n), guard
        self.lead = layout(self.buf.ptr.value, n, guard)[0]
        assert self.lead >= guard and self.lead + self.n + guard <= total
        self.image = np.full(total, fill_bits, np.uint64).view(np.float64)
        if host is not None:
            self.image[self.lead:self.lead + self.n] = np.ascontiguousarray(host, np.float64).ravel()
        self.ptr = self.buf.offset(self.lead)
        assert self.ptr.value % PAGE == 0
        self.vec = _Ptr(self.ptr)
        self.reset()

    def reset(self):
        """(Re-)upload the image: an output buffer is all sentinel again."""
        self.buf.upload(self.image)

    def whole(self):
        return self.buf.get()

    def payload(self, whole=None):
        whole = self.whole() if whole is None else whole
        return whole[self.lead:self.lead + self.n]

    def outside(self, *written):
        """Mask over the whole buffer: True everywhere but the payload slices `written` (payload
        indices) -- the entries a launch must leave alone."""
        m = np.ones(self.buf.n, bool)
        for s in written:
            m[self.lead + s.start:self.lead + s.stop] = False
        return m

    def intact(self, whole=None):
        """An input buffer: every bit as uploaded, guards included."""
        whole = self.whole() if whole is None else whole
        return np.array_equal(whole.view(np.uint64), self.image.view(np.uint64))

    def free(self):
        self.buf.free()


def guarded(ctx, host, guard=512):
    """Input buffer: the payload `host`, NaN in the guards."""
    host = np.ascontiguousarray(host, np.float64)
    return Guarded(ctx, host.size, guard, np.array(np.nan).view(np.uint64), host)


def guarded_out(ctx, n, guard=512):
    """Output buffer of n doubles: the sentinel everywhere, guards and payload."""
    return Guarded(ctx, n, guard, SENTINEL)


def untouched(whole, region):
    """Every entry of the host copy `whole` under the mask `region` still holds the sentinel's bits."""
    return bool(np.all(whole.view(np.uint64)[region] == SENTINEL))


# ---- false addresses, poison sets ----

def _row_index(A):
    return np.repeat(np.arange(A.nrows, dtype=np.int64), np.diff(A.rowptr))


def _stores(A, ncols, rows, cols):
    """Per pair: does (block) row rows[i] store (block) column cols[i]?"""
    keys = _row_index(A) * ncols + A.col.astype(np.int64)  # ascending: rows ascending, columns within
    q = np.asarray(rows, np.int64) * ncols + np.asarray(cols, np.int64)
    pos = np.searchsorted(keys, q)
    pos[pos == keys.size] = 0
    return keys[pos] == q if keys.size else np.zeros(q.size, bool)


def band_offsets(A):
    """The union of stored col - row over the matrix, ascending."""
    return np.unique(A.col.astype(np.int64) - _row_index(A))


def box_stencil(A, dims):
    """The (dx, dy, dz) offsets of the box stencil A stores on the grid `dims` (x fastest): the offsets
    whose in-grid neighbour EVERY row stores.  (Found from the pairs, not by decoding col - row: on a
    grid with ny = 2 the linear offset -nx is both (0, -1, 0) and (0, 1, -1).)"""
    nx, ny, nz = dims
    r = np.arange(A.nrows, dtype=np.int64)
    x, y, z = r % nx, (r // nx) % ny, r // (nx * ny)
    out = []
    for dz in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                ok = (x + dx >= 0) & (x + dx < nx) & (y + dy >= 0) & (y + dy < ny) & (z + dz >= 0) & (z + dz < nz)
                if ok.any() and _stores(A, A.nrows, r[ok], r[ok] + dx + nx * (dy + ny * dz)).all():
                    out.append((dx, dy, dz))
    return out


def false_addresses(A, offsets_or_dims=None, sell=False, ncols=None):
    """-> {key: (rows, addresses)}: per row r the (block) columns a careless kernel could read for it
    though r does not store them.

    Band or grid image (offsets_or_dims: None = the union of stored col - row, or an offset list):
    clamp(r + d, 0, n - 1) for every offset d of the image that row r does not store; key = d.
    Box grid (offsets_or_dims = (nx, ny, nz)): the same addresses, keyed by the faces "x-" .. "z+"
    the missing neighbour lies beyond (a corner neighbour counts at each of its faces).
    sell=True adds the keys "first", "last", "own": column 0, column ncols - 1 and the row's own
    index (where r < ncols), each for the rows that do not store it.  sell=True with
    offsets_or_dims="sell" gives those three alone (a general pattern has no offset set)."""
    n = A.nrows
    ncols = n if ncols is None else ncols
    rows_all = np.arange(n, dtype=np.int64)
    out = {}

    def add(key, rows, addr):
        keep = ~_stores(A, ncols, rows, addr)  # (a clamped address the row does store is no false one)
        rows, addr = rows[keep], addr[keep]
        if key in out:
            rows, addr = np.concatenate([out[key][0], rows]), np.concatenate([out[key][1], addr])
        out[key] = (rows, addr)

    if isinstance(offsets_or_dims, str):
        assert offsets_or_dims == "sell" and sell
    elif offsets_or_dims is not None and len(offsets_or_dims) == 3 and int(np.prod(offsets_or_dims)) == n:
        assert ncols == n, "grids are square matrices"
        nx, ny, nz = dims = tuple(int(v) for v in offsets_or_dims)
        pos = (rows_all % nx, (rows_all // nx) % ny, rows_all // (nx * ny))
        for f in FACES:
            out[f] = (np.zeros(0, np.int64), np.zeros(0, np.int64))
        for comp in box_stencil(A, dims):
            a = np.clip(rows_all + comp[0] + nx * (comp[1] + ny * comp[2]), 0, n - 1)
            for axis in range(3):
                if comp[axis]:
                    beyond = (pos[axis] + comp[axis] < 0) | (pos[axis] + comp[axis] >= dims[axis])
                    add(FACES[2 * axis + (comp[axis] > 0)], rows_all[beyond], a[beyond])
    else:
        assert ncols == n, "band images are square matrices"
        for d in (band_offsets(A) if offsets_or_dims is None else offsets_or_dims):
            at = rows_all + int(d)
            add(int(d), rows_all, np.clip(at, 0, n - 1))  # (where at is in range and stored, add() drops the pair)
    if sell:
        add("first", rows_all, np.zeros(n, np.int64))
        add("last", rows_all, np.full(n, ncols - 1, np.int64))
        own = rows_all[rows_all < ncols]
        add("own", own, own.copy())
    return out


def slice_addresses(A, C=64, width=8):
    """-> {"slice": (rows, addresses)} for the SELL image's stencil slices: a slice of C rows whose
    rows draw their columns from at most `width` offsets stores those offsets once and a mask per row,
    so for a row of such a slice the false addresses are clamp(r + d, 0, n - 1) for the slice's offsets
    d that the row does not store."""
    n = A.nrows
    rows, addr = [], []
    d_all = A.col.astype(np.int64) - _row_index(A)
    for s0 in range(0, n, C):
        s1 = min(n, s0 + C)
        offs = np.unique(d_all[A.rowptr[s0]:A.rowptr[s1]])
        if offs.size == 0 or offs.size > width:
            continue
        r = np.repeat(np.arange(s0, s1, dtype=np.int64), offs.size)
        rows.append(r)
        addr.append(np.clip(r + np.tile(offs, s1 - s0), 0, n - 1))
    rows = np.concatenate(rows) if rows else np.zeros(0, np.int64)
    addr = np.concatenate(addr) if addr else np.zeros(0, np.int64)
    keep = ~_stores(A, n, rows, addr)
    return {"slice": (rows[keep], addr[keep])}


def tainted_rows(A, J):
    """Mask over the (block) rows: the row stores a column of J."""
    t = np.zeros(A.nrows, bool)
    t[_row_index(A)[np.isin(A.col, np.asarray(sorted(J), np.int64))]] = True
    return t


def _candidates(fa_k, ncols):
    """A key's (rows, addresses) without the clamp targets 0 and ncols - 1, which are in every J -- unless
    the key has no other address ("first", "last"): a face or an offset is to be witnessed by a pick of
    its own, not by the clamps alone."""
    r, a = fa_k
    inner = (a != 0) & (a != ncols - 1)
    return (r[inner], a[inner]) if inner.any() else (r, a)


def witnesses(A, fa, J, ncols=None):
    """{key: rows}: the untainted rows with a false address of that key in J (the clamp targets count
    only for keys that have no other address)."""
    ncols = A.nrows if ncols is None else ncols
    t = tainted_rows(A, J)
    Ja = np.asarray(sorted(J), np.int64)
    out = {}
    for k in fa:
        r, a = _candidates(fa[k], ncols)
        out[k] = np.unique(r[np.isin(a, Ja) & ~t[r]])
    return out


def poison_set(A, fa, ncols=None, want=4, extra=(), seed=0, cap=0.2):
    """The deterministic poison set J (sorted array of (block) columns): the clamp targets 0 and
    ncols - 1, the columns `extra`, then grown greedily -- `want` rounds over the keys of `fa`, in each
    taking the key's next candidate (row, address) in a seeded order whose row is untainted: a witness
    already if the address is in J, else the address joins J unless a witness counted so far stores it.
    No pick takes the tainted share past `cap`.  (A small grid may leave a key short of `want`: the tests assert what they need, poison.conditions.)"""
    ncols = A.nrows if ncols is None else ncols
    J = {0, ncols - 1} | {int(c) for c in extra}
    tainted = tainted_rows(A, J)
    rowidx = _row_index(A)
    order = np.argsort(A.col, kind="stable")
    cstart = np.searchsorted(A.col[order], np.arange(ncols + 1))

    def storing(c):  # rows that store column c
        return rowidx[order[cstart[c]:cstart[c + 1]]]

    kept = np.zeros(A.nrows, bool)  # witnesses relied on: must stay untainted
    rng = np.random.default_rng(seed)
    cand, have = {}, {key: set() for key in fa}
    for key in fa:
        r, a = _candidates(fa[key], ncols)
        perm = rng.permutation(r.size)
        cand[key] = (r[perm], a[perm])
    # one witness per key and round (not `want` per key in turn: on a small grid the picks of one face
    # taint the candidates of the face opposite)
    for _ in range(want):
        for key in fa:
            r, a = cand[key]
            for i in range(r.size):
                ri, ai = int(r[i]), int(a[i])
                if tainted[ri] or ri in have[key]:
                    continue
                if ai not in J:
                    hit = storing(ai)
                    if kept[hit].any() or tainted.sum() + (~tainted[hit]).sum() > cap * A.nrows:
                        continue
                    J.add(ai)
                    tainted[hit] = True
                have[key].add(ri)
                kept[ri] = True
                break
    return np.asarray(sorted(J), np.int64)


def poison_values(count):
    """+Inf, NaN, +Inf, ... in the order of the sorted set."""
    v = np.full(count, np.inf)
    v[1::2] = np.nan
    return v


def poisoned(x, J, block=1, comp=0):
    """Copy of x with the poison at the entries J * block + comp (one scalar component of a block column)."""
    x = np.array(x, np.float64)
    x[np.asarray(J, np.int64) * block + comp] = poison_values(len(J))
    return x


def conditions(A, fa, J, ncols=None, cap=0.25, want=2):
    """(tainted share, least witness count over the keys that have candidates at all, ok)."""
    share = float(tainted_rows(A, J).mean()) if A.nrows else 0.0
    w = witnesses(A, fa, J, ncols)
    counts = [len(w[k]) for k in fa if fa[k][0].size]
    least = min(counts) if counts else 0
    return share, least, share <= cap and least >= want


def batches(A, cols, base, cap=0.25):
    """Split the columns `cols` into consecutive batches so that each batch together with the set
    `base` taints at most `cap` of the rows: what cannot be poisoned in one launch under the cap is
    poisoned over several."""
    out, cur = [], []
    for c in cols:
        if tainted_rows(A, set(base) | set(cur) | {int(c)}).mean() > cap and cur:
            out.append(cur)
            cur = []
        cur.append(int(c))
    if cur:
        out.append(cur)
    return out


# ---- the comparison ----

def leaks(got, ref):
    """Indices where the finiteness differs, or where ref is finite and got is not bitwise ref."""
    fg, fr = np.isfinite(got), np.isfinite(ref)
    return np.nonzero((fg != fr) | (fr & (got.view(np.uint64) != ref.view(np.uint64))))[0]


def assert_rows_only(got, ref, what=""):
    """isfinite(got) == isfinite(ref) everywhere, and got bitwise ref where ref is finite: a leak makes
    a finite row non-finite, a dropped stored term makes a non-finite row finite."""
    bad = leaks(np.ascontiguousarray(got), np.ascontiguousarray(ref))
    assert bad.size == 0, (what, "first differing entries", bad[:8].tolist(), got[bad[:8]].tolist(),
                           ref[bad[:8]].tolist())


def mv_poison(n, m, Q, entries):
    """Copy of the multivector Q (MultiVector<double,8> layout) with single entries X[j, c] poisoned:
    entries = [(j, c), ...], values alternating +Inf / NaN."""
    Q = np.array(Q, np.float64)
    vals = poison_values(len(entries))
    for (j, c), v in zip(entries, vals):
        Q[oracle.mv_index(n, j, c)] = v
    return Q
