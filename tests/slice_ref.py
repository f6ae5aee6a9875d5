"""numpy restatement of the spectrum-slicing solver (csrc/filter_host.cpp, csrc/slice.cpp) -- test
infrastructure only (imported like lobpcg_ref.py).

Filter: with A^ = (A - c I) / e, c = (lmax + lmin) / 2, e = (lmax - lmin) / 2 and the window mapped to
[a^, b^], p(t) = sum_{k=0..d} gamma_k T_k(t) is the Jackson-damped Chebyshev expansion of the window's
indicator, applied by Clenshaw: b_{d+1} = b_{d+2} = 0, b_k = gamma_k X + 2 A^ b_{k+1} - b_{k+2} for
k = d .. 1, p(A^) X = gamma_0 X + A^ b_1 - b_2.  Every product is one fused step

    out = s1 (A Xk) + s0 Xk + s2 Xold + g B

with the scalars of step_scalars(); b_d = gamma_d X is never formed (folded into the first two steps).

Driver: Y = p(A) X, CholQR2 of Y, H = Q^T A Q, X = Q S, R = A X - X theta; the pairs with theta in
[a, b] are accepted and the run stops when there is at least one and each has
||r_j|| <= tol max(|theta_j|, |a|, |b|) ||x_j||."""
import numpy as np


def filter_window(a, b, lmin, lmax):
    """(c, e, theta_a, theta_b) with the window clamped into [lmin, lmax]; ValueError for a refusal."""
    if not (np.isfinite([a, b, lmin, lmax]).all() and lmin < lmax):
        raise ValueError("filter: finite bounds with lmin < lmax required")
    if not a < b:
        raise ValueError("filter: a < b required")
    if b < lmin or a > lmax:
        raise ValueError("filter: [a, b] does not meet [lmin, lmax]")
    c, e = 0.5 * (lmax + lmin), 0.5 * (lmax - lmin)
    ah = min(1.0, max(-1.0, (max(a, lmin) - c) / e))
    bh = min(1.0, max(-1.0, (min(b, lmax) - c) / e))
    return c, e, float(np.arccos(ah)), float(np.arccos(bh))


def default_degree(a, b, lmin, lmax):
    """degree = 0: the Jackson kernel's resolution pi / (d + 2) at a quarter of the window's angular width,
    d = ceil(4 pi / (theta_a - theta_b)) - 2 clamped to [20, 2000]."""
    _, _, ta, tb = filter_window(a, b, lmin, lmax)
    w = ta - tb
    if not w > 0.0:
        return 2000
    return int(min(2000.0, max(20.0, np.ceil(4.0 * np.pi / w) - 2.0)))


def filter_coefs(a, b, lmin, lmax, degree):
    """gamma_0 .. gamma_d (degree = 0: the default degree)."""
    c, e, ta, tb = filter_window(a, b, lmin, lmax)
    d = default_degree(a, b, lmin, lmax) if degree == 0 else int(degree)
    if d < 2:
        raise ValueError("filter: degree >= 2 required")
    al = np.pi / (d + 2)
    gam = np.zeros(d + 1)
    for k in range(d + 1):
        mu = (ta - tb) / np.pi if k == 0 else 2.0 * (np.sin(k * ta) - np.sin(k * tb)) / (k * np.pi)
        g = ((d + 2 - k) * np.sin(al) * np.cos(k * al) + np.cos(al) * np.sin(k * al)) / ((d + 2) * np.sin(al))
        gam[k] = g * mu
    return gam


def filter_poly(gam, t):
    """p(t) for t in [-1, 1] (the scalar Clenshaw sum)."""
    t = np.asarray(t, float)
    b1, b2 = np.zeros_like(t), np.zeros_like(t)
    for k in range(len(gam) - 1, 0, -1):
        b1, b2 = gam[k] + 2.0 * t * b1 - b2, b1
    return gam[0] + t * b1 - b2


def step_scalars(gam, c, e, k):
    """(s1, s0, s2, g) of the product step that forms b_k (k = d - 1 .. 1) or the result (k = 0)."""
    d = len(gam) - 1
    s1 = (1.0 if k == 0 else 2.0) / e
    s0 = -c * s1
    if k == d - 1:   # b_{k+1} = gamma_d X is the gathered X itself, b_{k+2} = 0
        return gam[d] * s1, gam[d] * s0, 0.0, gam[k]
    if k == d - 2:   # b_{k+2} = gamma_d X goes into the X term
        return s1, s0, 0.0, gam[k] - gam[d]
    return s1, s0, -1.0, gam[k]


def filt_step(A, Xk, Xold, B, s1, s0, s2, g):
    out = s1 * (A @ Xk) + s0 * Xk + g * B
    return out if s2 == 0.0 else out + s2 * Xold


def apply_filter(A, X, a, b, lmin, lmax, degree):
    """Y = p(A) X by the d product steps of the device code."""
    gam = filter_coefs(a, b, lmin, lmax, degree)
    c, e, _, _ = filter_window(a, b, lmin, lmax)
    d = len(gam) - 1
    cur, old = X, None
    for k in range(d - 1, -1, -1):
        nxt = filt_step(A, cur, old, X, *step_scalars(gam, c, e, k))
        cur, old = nxt, cur
    return cur


def spectrum_bounds(alpha, beta):
    """(theta_min - beta_k, theta_max + beta_k) from k Lanczos steps: alpha[0..k-1], beta[0..k] with
    beta[1..k-1] the off-diagonal and beta[k] the last residual norm."""
    k = len(alpha)
    T = np.diag(np.asarray(alpha, float))
    for j in range(1, k):
        T[j, j - 1] = T[j - 1, j] = beta[j]
    th = np.linalg.eigvalsh(T)
    return th[0] - beta[k], th[-1] + beta[k]


def cholqr2(Y):
    """Q of CholQR twice; None at a non-positive pivot."""
    Q = Y
    for _ in range(2):
        G = Q.T @ Q
        G = 0.5 * (G + G.T)
        try:
            L = np.linalg.cholesky(G)
        except np.linalg.LinAlgError:
            return None
        Q = np.linalg.solve(L, Q.T).T
    return Q


def slice_solve(A, X0, a, b, lmin, lmax, degree, tol, max_iters):
    """-> dict(theta, X, resid, accepted, iters, converged, saturated); theta ascending, all `block` pairs."""
    X = cholqr2(np.array(X0, float))
    assert X is not None
    gam = filter_coefs(a, b, lmin, lmax, degree)
    c, e, _, _ = filter_window(a, b, lmin, lmax)
    d = len(gam) - 1
    scale = max(abs(a), abs(b))
    it, conv = 0, False
    theta = np.zeros(X.shape[1])
    res = np.full(X.shape[1], np.inf)
    acc = np.zeros(X.shape[1], bool)
    while it < max_iters:
        cur, old = X, None
        for k in range(d - 1, -1, -1):
            cur, old = filt_step(A, cur, old, X, *step_scalars(gam, c, e, k)), cur
        Q = cholqr2(cur)
        if Q is None:
            raise FloatingPointError("slice: CholQR2 met a non-positive pivot")
        AQ = A @ Q
        H = Q.T @ AQ
        theta, S = np.linalg.eigh(0.5 * (H + H.T))
        X, AX = Q @ S, AQ @ S
        R = AX - X * theta
        res = np.linalg.norm(R, axis=0)
        xn = np.linalg.norm(X, axis=0)
        acc = (theta >= a) & (theta <= b)
        it += 1
        if tol > 0.0 and acc.any() and np.all(res[acc] <= tol * np.maximum(np.abs(theta[acc]), scale) * xn[acc]):
            conv = True
            break
    return dict(theta=theta, X=X, resid=res, accepted=acc, iters=it, converged=conv, saturated=bool(acc.all()))


def count_estimate(A, Z, a, b, lmin, lmax, degree):
    """(1 / nvec) sum_j z_j^T p(A) z_j."""
    Y = apply_filter(A, Z, a, b, lmin, lmax, degree)
    return float(np.sum(Z * Y) / Z.shape[1])
