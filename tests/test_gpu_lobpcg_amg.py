"""The eigensolvers on an algebraic multigrid handle (eig_amg_create): LOBPCG preconditioned by one AMG V-cycle and
the shift-invert block Lanczos with the Ks solve by AMG iterations, on the scrambled + reverse Cuthill-McKee 16^3
7-point Poisson matrix -- no box grid, so the geometric multigrid does not apply and the only other preconditioner
is Chebyshev-Jacobi.

Iteration counts of the restatement (tests/lobpcg_ref.py, block 8, nev 4, tol 1e-8, the seeded start block), from
its CPU run: 15 with one V-cycle of tests/amg_ref.py (theta 0.08, smoother degree 2, ratio 5), 26 with
Chebyshev-Jacobi of degree 4 on [g / 10, g], g the Gershgorin bound."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as ssl

import amg_ref
import eigmi
import lobpcg_ref as lr

pytestmark = pytest.mark.gpu

NEV, BLOCK, TOL = 4, 8, 1e-8


@functools.lru_cache(maxsize=None)
def _problem():
    rp, c, v = eigmi.scrambled_rcm(*eigmi.gen_matrix(eigmi.GEN_POISSON3D, 16))
    K = sp.csr_matrix((v, c, rp), shape=(4096, 4096))
    exact = np.sort(ssl.eigsh(K, k=NEV, sigma=0.0, which="LM", tol=1e-14, v0=np.ones(4096), return_eigenvectors=False))
    return K, exact


@functools.lru_cache(maxsize=None)
def _ref_counts():
    K, _ = _problem()
    out = {}
    g = lr.gershgorin_lmax(K)
    for name, T in (("amg", lr.vcycles(amg_ref.Amg(K, 0.08, 2, 5.0), 1)), ("cheb4", lr.jacobi_cheb(K, 4, g / 10.0, g))):
        s = lr.Lobpcg(K, None, BLOCK, precond=T)
        it, conv = s.step(500, NEV, TOL)
        assert conv
        out[name] = it
    return out


def _upload(ctx, A):
    return eigmi.Matrix.from_bcsr(ctx, A.indptr.astype(np.int64), A.indices.astype(np.int32), A.data)


def test_restatement_counts_are_the_documented_ones():
    assert _ref_counts() == {"amg": 15, "cheb4": 26}


def test_lobpcg_with_one_amg_vcycle(ctx):
    K, exact = _problem()
    counts = _ref_counts()
    dK = _upload(ctx, K)
    mg = eigmi.Multigrid.amg(dK, 0.08, max_cols=BLOCK, smooth_degree=2, smooth_ratio=5.0)
    s = eigmi.Lobpcg(dK, None, block=BLOCK, mg=(mg, 1))
    it, conv, t = s.step(500, NEV, TOL)
    ev, Y, res = s.ritz(NEV, want_evec=True)
    g = lr.gershgorin_lmax(K)
    c = eigmi.Lobpcg(dK, None, block=BLOCK, cheb=(4, g / 10.0, g))
    itc, convc, tc = c.step(500, NEV, TOL)
    evc = c.ritz(NEV, want_resid=False)[0]
    print(f"lobpcg + amg V-cycle: {it} iterations (restatement {counts['amg']}), {t.total_ms:.2f} ms; Chebyshev-Jacobi "
          f"degree 4: {itc} iterations (restatement {counts['cheb4']}), {tc.total_ms:.2f} ms; max rel |ev - eigsh| = "
          f"{np.abs(ev / exact - 1).max():.2e}")
    assert conv and convc
    assert it == counts["amg"]
    assert it < itc and counts["amg"] < counts["cheb4"]
    assert np.abs(ev / exact - 1).max() <= 1e-10 and np.abs(evc / exact - 1).max() <= 1e-10
    host = np.linalg.norm(K @ Y.T - Y.T * ev, axis=0)
    assert np.all(res <= TOL * np.abs(ev) * np.linalg.norm(Y, axis=1)) and np.all(np.abs(res - host) <= 1e-6 * host)
    for h in (s, c, mg, dK):
        h.close()


def test_shift_invert_block_lanczos_with_amg(ctx):
    """eig_blanczos_create_si_mg on an AMG handle: K^-1 M with M = I and the K solve S_24, 24 AMG iterations.  The
    Lanczos needs a fixed symmetric operator, which S_k is for any k; its Ritz values are those of S_k M, off
    1 / lambda by the solve's error, so k is chosen for the 1e-8 bar: 0.3 per cycle gives a residual near 1e-12."""
    K, exact = _problem()
    dK, dM = _upload(ctx, K), _upload(ctx, sp.identity(4096, format="csr"))
    mg = eigmi.Multigrid.amg(dK, 0.08, max_cols=32, smooth_degree=2, smooth_ratio=5.0)
    bl = eigmi.BlockLanczos(dK, dM, block=32, max_steps=8, Ks=dK, sigma=0.0, mg=mg, cycles=24)
    bl.step(8)
    ev = bl.ritz(NEV, eigmi.WHICH_SA)[0]
    print("SI block Lanczos, scrambled Poisson 16^3 (AMG solve):", ev, "rel", np.abs(ev / exact - 1).max())
    assert np.all(np.diff(ev) >= 0)
    assert np.max(np.abs(ev - exact) / exact) <= 1e-8, (ev, exact)
    for h in (bl, mg, dM, dK):
        h.close()
