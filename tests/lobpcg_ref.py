"""numpy restatement of LOBPCG (dune-eigensolver_amd/csrc/lobpcg.cpp, k_lobpcg.hip) -- test
infrastructure only: the same state (S = [X | W | P] M-orthonormal, KS and MS carried by the update),
the same steps in the same order (residual, preconditioner, two classical Gram-Schmidt passes against
[X P] with the carried MX, MP, M-CholQR2 with the reuse-or-recompute choice of mcholqr2_mv, K W,
Rayleigh-Ritz on S^T K S, C_p from C_x by zeroing its X rows, two projections against C_x and a
Householder QR, the update of all three families), the same check of S^T M S = I before the
Rayleigh-Ritz and the same failure handling, in double precision
with another rounding order (the device sums every Gram in another order and uses MFMA), so results
agree to the restatement's own sensitivity (tests/test_lobpcg_ref.py), not bitwise.

Preconditioners are callables R -> W: jacobi_cheb (the device's eig_lobpcg_precond_cheb: `degree`
Chebyshev-Jacobi steps, mg_ref.cheb_solve's recurrence) and vcycles (mg_ref.Multigrid.solve)."""
import numpy as np

import mg_ref
import oracle

REUSE_COND = 1e4  # subspace_host.h kCholQrReuseCond
ORTH_TOL = 1e-10  # lobpcg.cpp kOrthTol: max |S^T M S - I| an iteration may enter its Rayleigh-Ritz with


class Breakdown(Exception):
    pass


def _chol_upper(G):
    G = 0.5 * (G + G.T)
    try:
        return np.linalg.cholesky(G).T
    except np.linalg.LinAlgError:
        raise Breakdown("non-positive pivot")


def mcholqr2(Z, M):
    """Z = Q R with Q M-orthonormal (CholQR twice); returns (Q, M Q)."""
    MZ = M @ Z if M is not None else Z
    R0 = _chol_upper(Z.T @ MZ)
    if not np.all(np.isfinite(R0)) or np.any(np.diag(R0) <= 0):
        raise Breakdown("non-positive pivot")
    S0 = np.linalg.inv(R0)
    d = np.abs(np.diag(R0))
    reuse = d.max() <= REUSE_COND * d.min()
    Z = Z @ S0
    if M is None:
        MZ = Z
    elif reuse:
        MZ = MZ @ S0
    else:
        MZ = M @ Z
    S1 = np.linalg.inv(_chol_upper(Z.T @ MZ))
    Z = Z @ S1
    return Z, (MZ @ S1 if M is not None else Z)


def jacobi_cheb(A, degree, lmin, lmax):
    A = A.tocsr()
    dinv = 1.0 / A.diagonal()
    return lambda R: mg_ref.cheb_solve(A, dinv, R, degree, lmin, lmax)


def vcycles(mg, cycles=1):
    return lambda R: mg.solve(R, cycles)


def gershgorin_lmax(A):
    """max row sum of |D^-1 A|: the upper end the Chebyshev-Jacobi preconditioners are given."""
    A = A.tocsr()
    return float(np.max(np.asarray(abs(A).sum(axis=1)).ravel() / A.diagonal()))


class Lobpcg:
    def __init__(self, K, M=None, block=8, which="SA", X0=None, seed=123, precond=None):
        self.K, self.M, self.m, self.which, self.T = K.tocsr(), (M.tocsr() if M is not None else None), block, which, precond
        n = K.shape[0]
        assert 4 * block <= n and (precond is None or which == "SA")
        if X0 is None:
            X0 = oracle.mv_to_cols(oracle.random_mv8(n, block, seed), n, block)
        X, MX = mcholqr2(np.array(X0, dtype=np.float64), self.M)
        KX = self.K @ X
        self.theta, C = self._ritz_small(X.T @ KX)
        self.X, self.KX, self.MX = X @ C, KX @ C, MX @ C
        self.P = self.KP = self.MP = None
        self.iters = self.p_dropped = self.orth_rejected = 0
        self.orth_dev = 0.0

    def _ritz_small(self, H):
        w, Z = np.linalg.eigh(0.5 * (H + H.T))
        pick = np.arange(self.m) if self.which == "SA" else np.arange(H.shape[0] - 1, H.shape[0] - 1 - self.m, -1)
        return w[pick], Z[:, pick]

    def residual(self, KX=None, MX=None):
        KX = self.KX if KX is None else KX
        MX = self.MX if MX is None else MX
        R = KX - MX * self.theta
        return R, np.sqrt((R * R).sum(axis=0)), np.sqrt((MX * MX).sum(axis=0))

    def _iterate(self, R, use_p):
        m = self.m
        W = self.T(R) if self.T is not None else R.copy()
        B = [self.X, self.P] if use_p else [self.X]
        MB = [self.MX, self.MP] if use_p else [self.MX]
        for _ in range(2):
            C = [mb.T @ W for mb in MB]
            for b, c in zip(B, C):
                W = W - b @ c
        W, MW = mcholqr2(W, self.M)
        KW = self.K @ W
        S = np.hstack([self.X, W] + ([self.P] if use_p else []))
        KS = np.hstack([self.KX, KW] + ([self.KP] if use_p else []))
        MS = np.hstack([self.MX, MW] + ([self.MP] if use_p else []))
        dev = np.abs(S.T @ MS - np.eye(S.shape[1])).max()
        if not dev <= ORTH_TOL:
            self.orth_rejected += 1
            raise Breakdown("S is not M-orthonormal")
        self.orth_dev = max(self.orth_dev, dev)
        theta, Cx = self._ritz_small(S.T @ KS)
        Cp = Cx.copy()
        Cp[:m] = 0.0
        for _ in range(2):
            Cp = Cp - Cx @ (Cx.T @ Cp)
        Cp = np.linalg.qr(Cp)[0]
        self.theta = theta
        self.X, self.KX, self.MX = S @ Cx, KS @ Cx, MS @ Cx
        self.P, self.KP, self.MP = S @ Cp, KS @ Cp, MS @ Cp

    def step(self, max_iters, nev, tol):
        """-> (iterations done, converged); tol = 0 forces max_iters iterations."""
        it = 0
        while True:
            if tol == 0.0 and it == max_iters:
                return it, False
            R, rn, mn = self.residual()
            if tol > 0.0:
                conv = bool(np.all(rn[:nev] <= tol * np.abs(self.theta[:nev]) * mn[:nev]))
                if conv or it == max_iters:
                    return it, conv
            try:
                self._iterate(R, self.P is not None)
            except Breakdown:
                if self.P is None:
                    raise
                self.P = self.KP = self.MP = None
                self.p_dropped += 1
                self._iterate(R, False)
            it += 1
            self.iters += 1

    def ritz(self, nev):
        """theta, vectors (n, nev) and the true residuals from fresh products."""
        X = self.X
        MX = self.M @ X if self.M is not None else X
        _, rn, _ = self.residual(self.K @ X, MX)
        return self.theta[:nev].copy(), X[:, :nev].copy(), rn[:nev]


# ---------------------------------------------------------------------------------------------
# The problems the CPU and GPU tests share: name -> (K, M or None, preconditioner, dense reference
# eigenvalues); built once.
# ---------------------------------------------------------------------------------------------
_problems = {}


def laplace2d(N):
    A = oracle.laplace2d(N)
    return A.to_scipy().tocsr()


def scaled_q1elast(N):
    """The 3x3-blocked pair of tests/test_gpu_blocked_drivers.py (that file's mats(); the GPU test checks
    they are equal): S A S with A = q1elast(N), s_i = 1 + 0.25 sin(1.7 i), and the block-diagonal B with
    block I = (1 + 0.1 (I mod 3)) [[2, .5, 0], [.5, 2, .5], [0, .5, 2]]; both oracle.CSR."""
    A = oracle.q1elast(N)
    s = 1.0 + 0.25 * np.sin(1.7 * np.arange(A.n))
    I = np.repeat(np.arange(A.nrows), np.diff(A.rowptr))
    J = A.col.astype(np.int64)
    r = np.arange(3)
    srow = s[(I[:, None] * 3 + r)][:, :, None]
    scol = s[(J[:, None] * 3 + r)][:, None, :]
    S = oracle.CSR(A.nrows, A.rowptr, A.col, (A.val.reshape(-1, 3, 3) * (srow * scol)).reshape(-1), 3, 3)
    T = np.array([[2.0, 0.5, 0.0], [0.5, 2.0, 0.5], [0.0, 0.5, 2.0]])
    bval = ((1.0 + 0.1 * (np.arange(A.nrows) % 3))[:, None, None] * T).reshape(-1)
    B = oracle.CSR(A.nrows, np.arange(A.nrows + 1, dtype=np.int64), np.arange(A.nrows, dtype=np.int32), bval, 3, 3)
    return S, B


def expand3(A):
    """Scalar expansion of a 3x3-blocked oracle.CSR as scipy CSR."""
    import scipy.sparse as sp
    n = A.nrows * 3
    return sp.bsr_matrix((A.val.reshape(-1, 3, 3), A.col, A.rowptr), shape=(n, n)).tocsr()


def problem(name):
    """p1-N-jacobi / p1-N-mg: the P1 pencil with Chebyshev-Jacobi degree 1 on [0.1 g, g] (g the
    Gershgorin bound: plain Jacobi up to a factor) or one V-cycle of mg_ref (smoother degree 2, ratio 5);
    lap2d-N-cheb8: the 2-D Laplacian, M = None, Chebyshev-Jacobi degree 8 on [g / 10, g];
    q1s-5-cheb4: the scaled q1elast(5) and block-diagonal B of tests/test_gpu_blocked_drivers.py (their
    scalar expansions; "blocked" holds the 3x3 oracle.CSR pair), Chebyshev-Jacobi degree 4 on [g / 10, g];
    p1-N-none: no preconditioner.  -> dict(K, M, T, dims, ...)"""
    if name not in _problems:
        kind, N, prec = name.split("-")
        N = int(N)
        blocked = None
        if kind == "p1":
            K, M = oracle.p1_kuhn(N)
            dims = (N, N, N)
        elif kind == "q1s":
            S, B = scaled_q1elast(N)
            K, M, dims = expand3(S), expand3(B), None
            blocked = (S, B)
        else:
            K, M, dims = laplace2d(N), None, None
        d = dict(K=K, M=M, dims=dims, N=N, blocked=blocked)
        if prec == "mg":
            d["mg"] = mg_ref.Multigrid(K, dims, 2, 5.0)
            d["T"] = vcycles(d["mg"], 1)
        elif prec == "none":
            d["T"] = None
        else:
            g = gershgorin_lmax(K)
            d["degree"] = 1 if prec == "jacobi" else int(prec[4:])
            d["lmin"], d["lmax"] = g / 10.0, g
            d["T"] = jacobi_cheb(K, d["degree"], d["lmin"], d["lmax"])
        _problems[name] = d
    return _problems[name]
