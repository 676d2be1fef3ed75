"""Truth for the nearest-row search and the library-based parameter estimation (tests/test_nearest_host.py,
tests/test_gpu_nearest.py, tests/test_gpu_param_library.py): an 80-bit checker of a top-t answer, the builder of the search
cases, and a small reduced model built with the oracle for the polish.  A helper, not a test file.  TEST INFRASTRUCTURE."""
import functools
import itertools

import numpy as np

LD = np.longdouble
EPS = 2.0 ** -52


def exact_dist2(p, Q):
    """sum_c (p_c - q_c)^2 against every row of Q, in 80-bit arithmetic (relative error r 2^-64: nothing beside (r + 2) eps)."""
    D = np.asarray(Q, dtype=LD) - np.asarray(p, dtype=LD)[None, :]
    return (D * D).sum(axis=1)


def brute_force(P, Q, t):
    """The t rows of smallest (fp64 difference-form distance in column order, row) per query: what rom_nearest defines."""
    P, Q = np.asarray(P, dtype=np.float64), np.asarray(Q, dtype=np.float64)
    idx = np.zeros((len(P), t), dtype=np.int64)
    d2 = np.zeros((len(P), t))
    for k, p in enumerate(P):
        s = np.zeros(len(Q))
        for c in range(Q.shape[1]):
            d = p[c] - Q[:, c]
            s = d * d + s   # (one rounding more per term than the device's fma: inside the checker's bound)
        order = np.lexsort((np.arange(len(Q)), s))[:t]
        idx[k], d2[k] = order, s[order]
    return idx, d2


def check_neighbours(P, Q, idx, dist2, t):
    """Raises AssertionError unless (idx, dist2) is a valid top-t answer of rom_nearest for the queries P and the library Q:
    every reported distance within (r + 2) eps relative of the exact one, each row sorted by (dist2, index) with distinct
    rows of the library, and no returned row farther than a row that was not returned by more than the factor
    1 + 2 (r + 2) eps (a near tie may resolve either way; nothing is excluded)."""
    P, Q = np.asarray(P, dtype=np.float64), np.asarray(Q, dtype=np.float64)
    idx, dist2 = np.asarray(idx), np.asarray(dist2)
    K, r = P.shape
    M = len(Q)
    assert idx.shape == (K, t) and dist2.shape == (K, t), (idx.shape, dist2.shape, (K, t))
    assert ((idx >= 0) & (idx < M)).all(), "row index out of range"
    tol = LD((r + 2) * EPS)
    for k in range(K):
        D = exact_dist2(P[k], Q)
        got = D[idx[k]]
        assert len(set(idx[k].tolist())) == t, f"query {k}: repeated rows {idx[k]}"
        err = np.abs(dist2[k].astype(LD) - got)
        assert (err <= tol * got).all(), f"query {k}: distances {dist2[k]} off the exact {got.astype(float)} by {err.astype(float)}"
        for s in range(t - 1):
            a, b = (dist2[k, s], idx[k, s]), (dist2[k, s + 1], idx[k, s + 1])
            assert a < b, f"query {k}: entries {s}, {s + 1} not sorted by (dist2, index): {a}, {b}"
        rest = np.ones(M, dtype=bool)
        rest[idx[k]] = False
        if rest.any():
            worst, best_left = got.max(), D[rest].min()
            assert worst <= best_left * (1 + 2 * tol), (
                f"query {k}: returned a row at {float(worst)!r} but left one at {float(best_left)!r} (row {int(np.flatnonzero(rest)[D[rest].argmin()])})")


# ---- the search cases -----------------------------------------------------------------------------------------------
def build_case(kind, M, K, r, seed=0):
    """(Q (M, r), P (K, r)) of one kind: 'uniform' in [0, 1); 'offset' the same at 1e8; 'ulp' rows of a lattice one ulp apart at
    1e8, shuffled, the queries on and between lattice points; 'graded' columns scaled from 1 down to 1e-12; 'self' queries that
    are library rows."""
    rng = np.random.default_rng(seed)
    if kind == "uniform":
        return rng.random((M, r)), rng.random((K, r))
    if kind == "offset":
        return 1e8 + rng.random((M, r)), 1e8 + rng.random((K, r))
    if kind == "ulp":
        u = np.spacing(1e8)
        Q = 1e8 + u * rng.integers(0, 6, size=(M, r)).astype(np.float64)
        P = 1e8 + u * rng.integers(0, 6, size=(K, r)).astype(np.float64)
        return Q, P
    if kind == "graded":
        scale = 10.0 ** (-12.0 * np.arange(r) / max(r - 1, 1))
        return rng.random((M, r)) * scale, rng.random((K, r)) * scale
    if kind == "self":
        Q = rng.standard_normal((M, r))
        return Q, Q[rng.choice(M, size=K, replace=K > M)].copy()
    raise ValueError(kind)


def copies_case(M, K, r, groups, group_size, seed=0):
    """A uniform library in which the row nearest to the (identical) queries is copied into row 5 of each of the `groups` groups
    listed; returns (Q, P, the rows of the copies in ascending order)."""
    rng = np.random.default_rng(seed)
    Q = rng.random((M, r))
    p = rng.random(r)
    best = p + 1e-3 * rng.random(r) / np.sqrt(r)
    rows = np.array(sorted(g * group_size + 5 for g in groups), dtype=np.int64)
    Q[rows] = best
    return Q, np.tile(p, (K, 1)), rows


# ---- a reduced model from the oracle, for the polish ------------------------------------------------------------------
def grid_library(k, per_axis, decades):
    """The per_axis^k grid in log10 a over [0, decades]: (per_axis^k, k)."""
    ax = np.linspace(0.0, decades, per_axis)
    return 10.0 ** np.array(list(itertools.product(ax, repeat=k)))


@functools.lru_cache(maxsize=None)
def oracle_rom(blocks=(2, 2), N=8, n=10, decades=4.0, sensors=16, seed=0):
    """A Galerkin ROM of the (blocks, N) problem on n snapshots at random parameters (Euclidean-orthonormalised): returns a
    dict with the oracle geometry g, the basis W (n, dim), Ahat (k, n, n), bhat (n,), the sensor points and E = l(W) (n, m),
    and the snapshot parameters a_basis (n, *blocks) with their raw snapshots U_basis."""
    from oracle import rom_oracle as ro
    rng = np.random.default_rng(seed)
    g = ro.Geometry(blocks, N)
    k = g.k
    a_basis = 10.0 ** rng.uniform(0.0, decades, size=(n,) + tuple(blocks))
    U = ro.generate_solutions(g, a_basis, "lsqsparse")
    W = np.linalg.qr(U.T)[0].T
    Ahat = ro.reduced_tensor(g, W).reshape(k, n, n)
    bhat = W @ ro.load_vector(g)
    pts = rng.uniform(-0.95, 0.95, size=(sensors, 2)) * np.array([g.ncb / 2.0, g.nrb / 2.0])
    E = ro.evaluate_solutions(g, pts, W)
    return dict(g=g, k=int(k), blocks=tuple(blocks), W=W, Ahat=np.asarray(Ahat), bhat=bhat, points=pts, E=np.asarray(E), a_basis=a_basis,
                U_basis=U, E_basis=np.asarray(ro.evaluate_solutions(g, pts, U)))


def rom_coefficients(Ahat, bhat, a):
    """c(a) = (sum_q a_q Ahat_q)^-1 bhat for the rows of a (K, k)."""
    A = np.einsum("kq,qij->kij", np.asarray(a).reshape(len(a), -1), Ahat)
    return np.linalg.solve(A, np.broadcast_to(bhat, (len(a), len(bhat)))[..., None])[..., 0]
