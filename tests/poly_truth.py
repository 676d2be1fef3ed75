"""Truth for the polynomial-map tests (tests/test_poly_map_host.py, tests/test_gpu_poly_map.py): the exponent list of
PolynomialFeatures, the scaled Legendre features of rom_poly_fit in any dtype and a least squares in 80-bit arithmetic.
A helper, not a test file.  TEST INFRASTRUCTURE."""
import itertools

import numpy as np

LD = np.longdouble
EPS = 2.0 ** -53
C = 64.0


def powers(m, d):
    """The exponent rows of PolynomialFeatures(d).powers_: graded, combinations_with_replacement in each degree."""
    rows = []
    for deg in range(d + 1):
        for comb in itertools.combinations_with_replacement(range(m), deg):
            rows.append(np.bincount(np.array(comb, dtype=np.int64), minlength=m) if deg else np.zeros(m, dtype=np.int64))
    return np.array(rows, dtype=np.int64).reshape(-1, m)


def midrange(X):
    """c, h of the training rows as rom_poly_fit forms them (fp64: 0.5 min + 0.5 max, 0.5 max - 0.5 min)."""
    X = np.asarray(X, dtype=np.float64)
    mn, mx = X.min(axis=0), X.max(axis=0)
    return 0.5 * mn + 0.5 * mx, 0.5 * mx - 0.5 * mn


def features(X, c, h, pw, dtype=np.float64):
    """prod_j L_{alpha_j}((x_j - c_j) / h_j) for the exponent rows pw, in `dtype`; a column with h = 0 has t = 0."""
    X = np.asarray(X, dtype=dtype)
    c, h = np.asarray(c, dtype=dtype), np.asarray(h, dtype=dtype)
    safe = np.where(h > 0, h, dtype(1))
    t = np.where(h > 0, (X - c) / safe, dtype(0))
    d = int(pw.max()) if pw.size else 0
    L = [np.ones_like(t), t]
    for k in range(1, d):
        L.append((dtype(2 * k + 1) * t * L[k] - dtype(k) * L[k - 1]) / dtype(k + 1))
    out = np.ones((X.shape[0], len(pw)), dtype=dtype)
    for p, alpha in enumerate(pw):
        for j, a in enumerate(alpha):
            if a:
                out[:, p] = out[:, p] * L[a][:, j]
    return out


def lstsq_ld(A, B, drop=LD(2) ** -40):
    """argmin ||A W - B|| in 80-bit arithmetic: column-wise classical Gram-Schmidt, twice (CGS2), then back-substitution.
    A column whose remainder is below `drop` times its norm is dependent on the ones before it: its coefficient is zero
    (a least-squares minimiser, as the device's).  Returns W (columns of A x columns of B) and the kept flags."""
    A = np.asarray(A, dtype=LD)
    B = np.asarray(B, dtype=LD).reshape(A.shape[0], -1)
    n = A.shape[1]
    Q = np.zeros_like(A)
    R = np.zeros((n, n), dtype=LD)
    kept = np.zeros(n, dtype=bool)
    for j in range(n):
        v = A[:, j].copy()
        norm0 = np.sqrt(v @ v)
        for _ in range(2):
            coef = Q[:, :j].T @ v
            v = v - Q[:, :j] @ coef
            R[:j, j] += coef
        nv = np.sqrt(v @ v)
        if norm0 > 0 and nv > drop * norm0:
            kept[j] = True
            R[j, j] = nv
            Q[:, j] = v / nv
    Z = Q.T @ B
    W = np.zeros((n, B.shape[1]), dtype=LD)
    for j in range(n - 1, -1, -1):
        if kept[j]:
            W[j] = (Z[j] - R[j, j + 1:] @ W[j + 1:]) / R[j, j]
    return W, kept


def kappa_normalised(Phi, rank=None):
    """kappa_2 of the column-normalised design matrix (columns of zero norm left out); with `rank` the ratio of the largest
    to the rank-th singular value (a matrix of fewer rows than columns)."""
    Phi = np.asarray(Phi, dtype=np.float64)
    nrm = np.linalg.norm(Phi, axis=0)
    s = np.linalg.svd(Phi[:, nrm > 0] / nrm[nrm > 0], compute_uv=False)
    return float(s[0] / s[(rank if rank is not None else len(s)) - 1])


def rms(A, axis=0):
    A = np.asarray(A, dtype=LD)
    return np.sqrt((A * A).mean(axis=axis)).astype(np.float64)
