"""The truth for box-constrained least squares, independent of how it was solved.

min over lo <= c <= hi of ||p - G c||^2 is a convex quadratic programme: a point is its solution exactly when the
Karush-Kuhn-Tucker conditions hold.  ``check_kkt`` forms g = G^T (G c - p) in long double and asserts, per system:

  * lo <= c <= hi;
  * ``bound`` is consistent with c: -1 means c_j == lo_j, +1 means c_j == hi_j, 0 means lo_j < c_j < hi_j strictly (a pinned
    coordinate, lo_j == hi_j, reads -1 and has no condition on g);
  * |g_j| <= tol_j where c_j is interior, g_j >= -tol_j where c_j is at lo, g_j <= tol_j where it is at hi;
  * ``misfit`` equals sqrt(||p - G c||^2 + perp2) recomputed in long double, to MISFIT_C (r + n) eps || |G||c| + |p| ||_2 plus
    4 eps of itself (the rounding of a residual formed in double by any order of summation, and of the square root).

tol_j = KKT_C (r + n) eps sum_i |G_ij| (|G||c| + |p|)_i: the first-order bound on the rounding of g when the residual and the
product with G^T are formed in double, in whatever order.  KKT_C is the worst ratio |violation_j| / ((r + n) eps sum_i ...)
that ``bvls_host`` itself reaches on the shapes of SHAPES, times a margin of 16 because the device sums in another order.
Measured (``python tests/bvls_truth.py``): worst ratio 0.107 at (1, 1, 3) (0.00805 at (4, 6, 5), below 0.002 at the larger
shapes) -> KKT_C = 16 * 0.107 rounded up to 2.  The misfit's worst ratio on the same runs is 0.034, also at (1, 1, 3) (0 elsewhere)
-> MISFIT_C = 16 * 0.034 rounded up to 0.6.  Neither was taken from device output.

``bent`` returns altered copies of a result that the checker must refuse: one c_j moved by 1e-9, one variable put on the
wrong bound, the misfit off by 1e-9 relative."""
import numpy as np

LD = np.longdouble
EPS = float(np.finfo(np.float64).eps)
KKT_C = 2.0
MISFIT_C = 0.6

# (n, r, K)
SHAPES = [(1, 1, 3), (4, 6, 5), (16, 20, 5), (50, 64, 5), (64, 64, 5), (64, 96, 6), (20, 50, 257)]
IDS = ["x".join(map(str, s)) for s in SHAPES]


def case(n, r, K):
    """G = N(0, 1) / sqrt(r), lo = -U(0.2, 1), hi = U(0.2, 1), p = G c* + 0.05 N(0, 1) with c* ~ U(-1.5, 1.5): (G, P, lo, hi)."""
    g = np.random.default_rng(100000 + 1000 * n + 10 * r + K)
    G = g.standard_normal((r, n)) / np.sqrt(r)
    lo, hi = -g.uniform(0.2, 1.0, n), g.uniform(0.2, 1.0, n)
    c_true = g.uniform(-1.5, 1.5, (K, n))
    P = c_true @ G.T + 0.05 * g.standard_normal((K, r))
    return G, P, lo, hi


def gradient(G, P, c):
    """g = G^T (G c - p) (K, n), its rounding unit sum_i |G_ij| (|G||c| + |p|)_i (K, n), the residual norm squared (K,) and
    || |G||c| + |p| ||_2 (K,), all in long double."""
    Gl, Pl, cl = np.asarray(G, dtype=LD), np.asarray(P, dtype=LD), np.asarray(c, dtype=LD)
    res = cl @ Gl.T - Pl
    mag = np.abs(cl) @ np.abs(Gl).T + np.abs(Pl)
    return res @ Gl, mag @ np.abs(Gl), np.einsum("kr,kr->k", res, res), np.sqrt(np.einsum("kr,kr->k", mag, mag))


def kkt_ratios(G, P, lo, hi, res, aux=None):
    """(the worst KKT violation / ((r + n) eps unit_j), the worst |misfit - truth| / ((r + n) eps || |G||c| + |p| ||)) after the
    exact checks (box, bound against c)."""
    G, P = np.asarray(G, dtype=np.float64), np.atleast_2d(np.asarray(P, dtype=np.float64))
    r, n = G.shape
    K = len(P)
    lo, hi = np.broadcast_to(np.asarray(lo, dtype=np.float64), (n,)), np.broadcast_to(np.asarray(hi, dtype=np.float64), (n,))
    c, bound = np.asarray(res.c, dtype=np.float64), np.asarray(res.bound)
    assert c.shape == (K, n) and bound.shape == (K, n) and np.asarray(res.misfit).shape == (K,)
    assert np.isfinite(c).all(), "c is not finite"
    assert ((c >= lo) & (c <= hi)).all(), f"c leaves the box by {max((lo - c).max(), (c - hi).max()):.3g}"
    assert np.isin(bound, (-1, 0, 1)).all()
    pinned = np.broadcast_to(lo == hi, c.shape)
    at_lo, at_hi = (c == lo) & ~pinned, (c == hi) & ~pinned
    assert (bound[pinned] == -1).all(), "a pinned coordinate reads -1"
    assert np.array_equal(bound == -1, at_lo | pinned), "bound = -1 exactly where c == lo"
    assert np.array_equal(bound == 1, at_hi), "bound = +1 exactly where c == hi"
    g, unit, res2, mag = gradient(G, P, c)
    viol = np.where(at_lo, np.maximum(-g, 0), np.where(at_hi, np.maximum(g, 0), np.where(pinned, 0, np.abs(g))))
    tiny = LD(np.finfo(np.float64).tiny)
    kkt = float((viol / ((r + n) * EPS * np.maximum(unit, tiny))).max()) if K else 0.0
    perp2 = np.zeros(K) if aux is None else np.asarray(aux, dtype=np.float64).reshape(K, 2)[:, 0]
    truth = np.sqrt(res2 + perp2.astype(LD))
    err = np.maximum(np.abs(np.asarray(res.misfit, dtype=LD) - truth) - 4 * EPS * truth, 0)
    mis = float((err / ((r + n) * EPS * np.maximum(mag, tiny))).max()) if K else 0.0
    return kkt, mis


def check_kkt(G, P, lo, hi, res, aux=None):
    """Asserts that ``res`` (a BvlsResult) solves every system; returns the two worst ratios to their bounds."""
    kkt, mis = kkt_ratios(G, P, lo, hi, res, aux)
    assert kkt <= KKT_C, f"Karush-Kuhn-Tucker violated: {kkt:.3g} (r + n) eps units, allowed {KKT_C}"
    assert mis <= MISFIT_C, f"misfit off: {mis:.3g} (r + n) eps units, allowed {MISFIT_C}"
    return kkt / KKT_C, mis / MISFIT_C


def kkt_tolerance(G, P, c):
    """tol (K, n) of the gradient conditions at c, as float64."""
    G = np.asarray(G, dtype=np.float64)
    g, unit, _, _ = gradient(G, np.atleast_2d(P), c)
    return g.astype(np.float64), (KKT_C * sum(G.shape) * EPS * unit).astype(np.float64)


def bent(res, lo, hi):
    """[(what, altered result)]: answers a checker has to refuse."""
    n = res.c.shape[1]
    lo, hi = np.broadcast_to(lo, (n,)), np.broadcast_to(hi, (n,))
    out = []
    k, j = np.argwhere(res.bound == 0)[0] if (res.bound == 0).any() else (None, None)
    if k is not None:
        c = res.c.copy()
        c[k, j] += 1e-9
        out.append(("a free c_j moved by 1e-9", res._replace(c=c)))
    idx = np.argwhere((res.bound != 0) & (lo < hi)[None, :])
    if len(idx):
        k, j = idx[0]
        c = res.c.copy()
        c[k, j] += 1e-9 if res.bound[k, j] < 0 else -1e-9
        out.append(("a bound c_j moved by 1e-9", res._replace(c=c)))
        c, b = res.c.copy(), res.bound.copy()
        c[k, j], b[k, j] = (hi[j], 1) if b[k, j] < 0 else (lo[j], -1)
        out.append(("a variable on the wrong bound", res._replace(c=c, bound=b)))
    out.append(("the misfit off by 1e-9 relative", res._replace(misfit=res.misfit * (1 + 1e-9))))
    return out


def permuted_delta(G, P, lo, hi, host, aux=None, max_iter=None):
    """delta (K,): the change of bvls_host's own c when the rows of G (and the entries of p) are permuted."""
    from romhighcontrast_amd.inverse import bvls_host
    perm = np.random.default_rng(9).permutation(G.shape[0])
    again = bvls_host(G[perm], np.atleast_2d(P)[:, perm], lo, hi, aux=aux, max_iter=max_iter)
    return np.abs(again.c - host.c).max(axis=1)


def host_bound(delta, c):
    """The bound of |c_other - c_host| per system: max(1e3 delta, 1e-11 (1 + max|c|))."""
    return np.maximum(1e3 * delta, 1e-11 * (1.0 + np.abs(c).max(axis=1)))


if __name__ == "__main__":   # the measurement behind KKT_C and MISFIT_C
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from romhighcontrast_amd.inverse import bvls_host
    for shape in SHAPES:
        G, P, lo, hi = case(*shape)
        res = bvls_host(G, P, lo, hi)
        print(shape, "ratios (kkt, misfit) %.3g %.3g" % kkt_ratios(G, P, lo, hi, res), "passes up to", res.iterations.max(),
              "bound variables", int((res.bound != 0).sum()), "converged", bool(res.converged.all()))
