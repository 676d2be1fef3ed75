"""The truth for rom_local_select / inverse.local_select_host, independent of how the two solves were made.

A system (measurement vector i, cluster j) is two convex quadratic programmes in a row.  ``check_system`` verifies, in long
double, for a returned (c, a, S, misfit):

  * c solves  min over c_lo <= c <= c_hi of ||p - G c||:  the Karush-Kuhn-Tucker conditions and the misfit, by
    ``bvls_truth.check_kkt`` with its own constants (the bound states are read off c: a coordinate on a bound is bound);
  * a solves  min over a_lo <= a <= a_hi of ||rho - B a||  for B = sum_i c_i R[:, 1 + i k : 1 + (i + 1) k] formed in long double
    from the returned c and rounded once: ``check_kkt`` again, on (B, rho);
  * S = ||R z||_2 with z = (1, -c_i a_q) at index 1 + i k + q, the product formed in long double from R itself, to
    (P + 4) eps || |R||z| ||_2 + 4 eps S, P = 1 + k n: the first-order bound of a sum of P products formed in double in any
    order and any grouping (B first or z first), the rounding of c_i a_q and of the square root.

``cases()`` are the shapes (n, k, rank, r, kc, K) of the tests with their operands; ``spec(name)`` is the specification's
result on a case; ``rule_bounds`` runs it again with the rows of every G_j (with p) and of every R_j permuted -- the
specification's own sensitivity to the order of summation, which is what the device may differ by.  ``spec`` and ``host_bounds``
are computed once per process."""
import functools

import numpy as np

from bvls_truth import EPS, LD, check_kkt

# (n, k, rank, r, kc, K)
SHAPES = {
    "one": (1, 1, 2, 1, 1, 1),
    "small": (3, 2, 7, 5, 3, 5),
    "odd": (17, 3, 52, 17, 3, 70),
    "n32k9": (32, 9, 289, 40, 2, 9),
    "n64k4": (64, 4, 257, 96, 17, 3),
    "k16": (8, 16, 129, 8, 5, 33),
}
GAP = 1e-6   # the relative gap between the two smallest S of a vector that every case keeps in the specification


class Case:
    """RT (kc, rank, 1 + k n), GR (kc, r, n), P (K, kc r), c_lo, c_hi (kc, n), a_lo, a_hi (kc, k)."""

    def __init__(self, n, k, rank, r, kc, K, RT, GR, P, c_lo, c_hi, a_lo, a_hi):
        self.n, self.k, self.rank, self.r, self.kc, self.K = n, k, rank, r, kc, K
        self.RT, self.GR, self.P, self.c_lo, self.c_hi, self.a_lo, self.a_hi = RT, GR, P, c_lo, c_hi, a_lo, a_hi

    def args(self):
        return self.RT, self.GR, self.P, self.c_lo, self.c_hi, self.a_lo, self.a_hi

    def replace(self, **kw):
        d = dict(self.__dict__)
        d.update(kw)
        return Case(**d)


def matrix_ld(R, c, k):
    """B = sum_i c_i R[:, 1 + i k : ...] in long double."""
    R, c = np.asarray(R, dtype=LD), np.asarray(c, dtype=LD)
    return np.einsum("i,riq->rq", c, R[:, 1:].reshape(R.shape[0], len(c), k))


def make_case(n, k, rank, r, kc, K, seed=0):
    """G_j = N(0, 1) / sqrt(r) and c boxes [-U(0.2, 1), U(0.2, 1)]; per cluster a centre c0 ~ U(-1.3, 1.3), and
    p_ij = G_j (c0_j + 0.3 U(-1, 1)) + 0.05 N(0, 1): bounds of c are active (as in bvls_truth.case).  R_j[:, 1:] = N(0, 1) / sqrt(rank)
    and rho_j = B_j(c0_j clipped to the box) a0 + 0.05 N(0, 1) with a0 ~ U(0.5, 3) against a boxes [U(0.8, 1.2), U(1.5, 2.5)]:
    the minimisers over a lie near a0, inside the box and beyond both of its sides."""
    g = np.random.default_rng(770000 + 1000 * n + 100 * k + 10 * kc + K + seed)
    GR = g.standard_normal((kc, r, n)) / np.sqrt(r)
    c_lo, c_hi = -g.uniform(0.2, 1.0, (kc, n)), g.uniform(0.2, 1.0, (kc, n))
    c0 = g.uniform(-1.3, 1.3, (kc, n))
    c_true = c0[None] + 0.3 * g.uniform(-1.0, 1.0, (K, kc, n))
    P = np.einsum("jrn,ijn->ijr", GR, c_true) + 0.05 * g.standard_normal((K, kc, r))
    RT = g.standard_normal((kc, rank, 1 + k * n)) / np.sqrt(rank)
    a_lo, a_hi = g.uniform(0.8, 1.2, (kc, k)), g.uniform(1.5, 2.5, (kc, k))
    for j in range(kc):
        a0 = g.uniform(0.5, 3.0, k)
        RT[j, :, 0] = (matrix_ld(RT[j], np.clip(c0[j], c_lo[j], c_hi[j]), k) @ a0).astype(np.float64) + 0.05 * g.standard_normal(rank)
    return Case(n, k, rank, r, kc, K, RT, GR, np.ascontiguousarray(P.reshape(K, kc * r)), c_lo, c_hi, a_lo, a_hi)


@functools.lru_cache(maxsize=None)
def case(name):
    return make_case(*SHAPES[name])


@functools.lru_cache(maxsize=None)
def spec(name):
    from romhighcontrast_amd.inverse import local_select_host
    return local_select_host(*case(name).args())


def permuted(cs):
    """The same case with the rows of every G_j (and the entries of every p_ij) and the rows of every R_j permuted."""
    g = np.random.default_rng(9)
    pr, pk = g.permutation(cs.r), g.permutation(cs.rank)
    P = cs.P.reshape(cs.K, cs.kc, cs.r)[:, :, pr].reshape(cs.K, cs.kc * cs.r)
    return cs.replace(RT=np.ascontiguousarray(cs.RT[:, pk]), GR=np.ascontiguousarray(cs.GR[:, pr]), P=np.ascontiguousarray(P))


def rule_bounds(cs, host, max_iter=None):
    """Per system the bounds of |c - c_spec|, |a - a_spec|, |S - S_spec|: max(1e3 delta, 1e-11 (1 + max|.|)), delta the
    specification's own change when the rows of every G_j and R_j of the case are permuted (the rule of test_gpu_bvls.py)."""
    from romhighcontrast_amd.inverse import local_select_host
    p = local_select_host(*permuted(cs).args(), max_iter=max_iter)

    def bound(x, y):
        x, y = x.reshape(x.shape[0], x.shape[1], -1), y.reshape(x.shape[0], x.shape[1], -1)
        with np.errstate(invalid="ignore"):
            delta = np.nan_to_num(np.abs(x - y).max(axis=2))
            return np.maximum(1e3 * delta, 1e-11 * (1.0 + np.nan_to_num(np.abs(x)).max(axis=2)))
    return bound(host.c_all, p.c_all), bound(host.a_all, p.a_all), bound(host.surrogate_all, p.surrogate_all)


@functools.lru_cache(maxsize=None)
def host_bounds(name):
    """``rule_bounds`` of a named case against its specification."""
    return rule_bounds(case(name), spec(name))


def within(res, host, bounds):
    """The largest ratios of |c - c_spec|, |a - a_spec|, |S - S_spec| to their bounds, asserted <= 1."""
    worst = []
    for x, y, b in zip((res.c_all, res.a_all, res.surrogate_all), (host.c_all, host.a_all, host.surrogate_all), bounds):
        d = np.abs(x - y).reshape(b.shape[0], b.shape[1], -1).max(axis=2)
        assert (d <= b).all(), f"device - specification up to {(d / b).max():.3g} of the bound"
        worst.append(float((d / b).max()))
    return worst


def label_gap(S, status):
    """Per vector the relative gap (S_2 - S_1) / S_2 between the two smallest S among the systems of status 0 (inf with fewer
    than two)."""
    S = np.where(status == 0, S, np.inf)
    if S.shape[1] < 2:
        return np.full(len(S), np.inf)
    two = np.sort(S, axis=1)[:, :2]
    with np.errstate(invalid="ignore"):
        return np.where(np.isfinite(two[:, 1]), (two[:, 1] - two[:, 0]) / two[:, 1], np.inf)


def _bound_of(c, lo, hi):
    return np.where((lo == hi) | (c == lo), -1, np.where(c == hi, 1, 0))


def surrogate_ld(R, c, a):
    """(||R z||_2, || |R||z| ||_2) in long double, z = (1, -c_i a_q)."""
    R = np.asarray(R, dtype=LD)
    z = np.concatenate([[LD(1)], -(np.asarray(c, dtype=LD)[:, None] * np.asarray(a, dtype=LD)[None, :]).reshape(-1)])
    v, mag = R @ z, np.abs(R) @ np.abs(z)
    return np.sqrt(v @ v), np.sqrt(mag @ mag)


def check_system(R, G, p, c_lo, c_hi, a_lo, a_hi, c, a, S, misfit):
    """Asserts that (c, a, S, misfit) is the answer of one system; returns the worst ratios to the three bounds."""
    from romhighcontrast_amd.inverse import BvlsResult
    k = len(a)
    one = BvlsResult(c[None, :], np.array([misfit]), _bound_of(c, c_lo, c_hi)[None, :], None, None)
    r1 = check_kkt(G, p[None, :], c_lo, c_hi, one)
    B = matrix_ld(R, c, k).astype(np.float64)
    two = BvlsResult(a[None, :], np.array([S]), _bound_of(a, a_lo, a_hi)[None, :], None, None)
    r3 = check_kkt(B, np.asarray(R)[:, 0][None, :], a_lo, a_hi, two)
    truth, mag = surrogate_ld(R, c, a)
    tol = (R.shape[1] + 4) * EPS * mag + 4 * EPS * truth
    assert abs(LD(S) - truth) <= tol, f"S = {S!r} against ||R z|| = {float(truth)!r}: off by {float(abs(LD(S) - truth)):.3g}, allowed {float(tol):.3g}"
    return max(r1), max(r3), float(abs(LD(S) - truth) / tol)


def check_result(cs, res, systems=None):
    """``check_system`` on every system of status 0 of a LocalSelectResult (or on the (i, j) pairs given) and the selection rule
    on its own tables; returns the number of systems checked and the worst ratios."""
    from romhighcontrast_amd.inverse import local_select_labels
    P = cs.P.reshape(cs.K, cs.kc, cs.r)
    worst, count = np.zeros(3), 0
    for i in range(cs.K):
        for j in range(cs.kc):
            if res.status[i, j] != 0 or (systems is not None and (i, j) not in systems):
                continue
            worst = np.maximum(worst, check_system(cs.RT[j], cs.GR[j], P[i, j], cs.c_lo[j], cs.c_hi[j], cs.a_lo[j], cs.a_hi[j],
                                                   res.c_all[i, j], res.a_all[i, j], res.surrogate_all[i, j], res.misfit_all[i, j]))
            count += 1
    assert np.array_equal(res.labels, local_select_labels(res.surrogate_all, res.status)), "labels against the tables"
    pick = res.labels >= 0
    rows = np.arange(cs.K)[pick]
    assert np.array_equal(res.surrogate[pick], res.surrogate_all[rows, res.labels[pick]])
    assert np.array_equal(res.coefficients[pick], res.c_all[rows, res.labels[pick]])
    assert np.array_equal(res.a[pick], res.a_all[rows, res.labels[pick]])
    assert np.array_equal(res.misfit[pick], res.misfit_all[rows, res.labels[pick]])
    return count, worst


def tiny_table(n, k, rank, seed=3):
    """A small residual table (rank, 1 + k n) of N(0, 1) entries with its own c (n,) and a box for a that cuts the
    unconstrained minimiser off on both sides."""
    g = np.random.default_rng(seed + 10 * n + k)
    R = g.standard_normal((rank, 1 + k * n))
    c = g.uniform(-1.0, 1.0, n)
    a0 = g.uniform(0.5, 3.0, k)
    R[:, 0] = (matrix_ld(R, c, k) @ a0).astype(np.float64) + 0.3 * g.standard_normal(rank)
    return R, c, np.full(k, 0.9), np.full(k, 2.1)
