"""Box-stencil matrices on nx x ny x nz grids with three independent extents -- test infrastructure
only (imported like mg_ref.py).  Lexicographic numbering, x fastest (row = x + nx (y + ny z)),
Dirichlet truncation: every row stores exactly its in-grid neighbours.  On a cube a swapped or
mis-tiled extent is invisible; here nx, ny and nz all differ and every offset has its own value."""
import numpy as np
import scipy.sparse as sp

import oracle


def offsets(shape):
    """The stencil's (dx, dy, dz) offsets, the diagonal included."""
    box = [(dx, dy, dz) for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1)]
    if shape == "full27":
        return box
    p7 = [o for o in box if sum(map(abs, o)) <= 1]
    if shape == "p7":
        return p7
    if shape == "nine":  # 7-point plus +-(0, 1, 1) in (dz, dy, dx): the face diagonal x + y
        return p7 + [(1, 1, 0), (-1, -1, 0)]
    if shape == "kuhn15":  # 0, +-e_i, +-(e_i + e_j), +-(1, 1, 1): all components of one sign
        return [o for o in box if min(o) >= 0 or max(o) <= 0]
    raise ValueError(shape)


def coords(dims):
    nx, ny, nz = dims
    idx = np.arange(nx * ny * nz)
    return idx, idx % nx, (idx // nx) % ny, idx // (nx * ny)


def box_matrix(dims, shape, values, seed=0):
    """-> oracle.CSR.  shape: "p7" | "kuhn15" | "full27" | "nine".  values: "const" = one value per
    offset (the same for +o and -o, every pair its own), strictly diagonally dominant -- the rows
    fall into the 27 geometric classes; "edge" = one random value per grid edge, stored bitwise equal
    in both triangles, under a positive dominating diagonal -- no two rows alike."""
    nx, ny, nz = dims
    n = nx * ny * nz
    idx, x, y, z = coords(dims)
    rng = np.random.default_rng(seed)
    ups = [o for o in offsets(shape) if o[0] + nx * (o[1] + ny * o[2]) > 0]
    rows, cols, vals = [], [], []
    rowabs = np.zeros(n)
    for dx, dy, dz in ups:
        ok = (x + dx >= 0) & (x + dx < nx) & (y + dy >= 0) & (y + dy < ny) & (z + dz >= 0) & (z + dz < nz)
        i = idx[ok]
        j = i + dx + nx * (dy + ny * dz)
        if values == "edge":
            w = -0.5 - rng.random(i.size)
            rowabs += np.bincount(i, weights=-w, minlength=n) + np.bincount(j, weights=-w, minlength=n)
        else:
            w = np.full(i.size, -0.5 - rng.random())
            rowabs -= 2.0 * w[0]  # (the full stencil's sum on every row: the diagonal is one constant)
        rows += [i, j]
        cols += [j, i]
        vals += [w, w]
    if values == "edge":
        diag = rowabs + 0.5 + rng.random(n)
    elif values == "const":
        diag = rowabs + 1.0
    else:
        raise ValueError(values)
    rows.append(idx)
    cols.append(idx)
    vals.append(diag)
    S = sp.csr_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(n, n))
    S.sort_indices()
    return oracle.CSR(n, S.indptr.astype(np.int64), S.indices.astype(np.int32), S.data.astype(np.float64))


def to_scipy(A):
    return sp.csr_matrix((A.val, A.col, A.rowptr), shape=(A.n, A.n))


def class_representatives(dims):
    """Per row, the row of its geometric class (first / interior / last in x, y and z) that the
    row-class kernel's table is read from: position 0, 1 or n - 1 in each direction."""
    nx, ny, nz = dims
    _, x, y, z = coords(dims)

    def pos(v, nv):
        return np.where(v == 0, 0, np.where(v == nv - 1, nv - 1, 1))

    return pos(x, nx) + nx * (pos(y, ny) + ny * pos(z, nz))


def rows_equal_class(A, dims):
    """Per row: does it store the same relative offsets and bitwise the same values as its class
    representative?"""
    rep = class_representatives(dims)
    out = np.zeros(A.n, bool)
    for r in range(A.n):
        a, b = slice(A.rowptr[r], A.rowptr[r + 1]), slice(A.rowptr[rep[r]], A.rowptr[rep[r] + 1])
        out[r] = (np.array_equal(A.col[a].astype(np.int64) - r, A.col[b].astype(np.int64) - rep[r]) and
                  np.array_equal(A.val[a], A.val[b]))
    return out
