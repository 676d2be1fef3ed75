"""Truth for the small dense layer of the basis stage (csrc/rom_small_dense.hip, csrc/rom_small_dense.h): the eigen-solvers and
whitenings behind ctx.small_eig / ctx.symmetric_orthonormalize, on every device route.  TEST INFRASTRUCTURE: imports no
product code; tests/test_small_dense_host.py proves it on the CPU, tests/test_gpu_small_dense.py uses it on the device.

  * route(), slot(), wave0_slots(), ns_entry(): the dispatch and the mechanisms restated (constants 32, 96, 2048; the
    Newton-Schulz entry at a row-sum bound of 2 -- it was 3 until the cases below showed the wrong root it admits).
  * ExactCase: symmetric matrices of small dyadic rationals with exactly known eigenvalues AND eigenvectors,
        A = P Q (H diag(d) H^T / m  (+)  diag(e)) Q^T P^T,
    H the Sylvester-Hadamard matrix of order m = 2^j <= n, d integer multiples of m (the Hadamard block is an integer
    matrix), e integers, Q = I - v v^T / 2 with four entries +-1 in v (a Householder reflection: entries in quarters) that
    straddle the two blocks (n >= 4), P a seeded permutation.  Eigenpairs: (d_k, P Q [h_k; 0] / sqrt(m)), (e_j, P Q e_{m+j}).
  * CoupledCase: diag(1..n) + a dense 3 x 3 coupling on an index triple; coverage_triples(n): triples whose coupled
    pairs visit every slot of the round-robin order.  Truth: mpmath at 50 digits.
  * InvSqrtCase: G = H diag(4^j) H^T / m, G^(-1/2) = H diag(2^-j) H^T / m exactly; chosen around the Newton-Schulz entry.
  * PivCholCase: X = diag(2^-i) L0 R with an exactly known pivoted-Cholesky whitening transform.
  * GradedCase: A = D B D, D powers of two over sixteen decades; truth mpmath.eigsy of the exact fp64 matrix at 90 digits.
  * jacobi_host(), newton_schulz_host(), pivchol_host(): plain fp64 NumPy restatements (same order, same criterion -- not
    the kernels' bits), with the stop rule of jacobi32_run selectable: "all" slots or the slots wave 0 owns.
  * the bounds: EPS = 2^-53, C = 64 (the project's convention, h10_truth.C).
"""
import json
import os

import numpy as np

import referee as rf

LD = np.longdouble
EPS = 2.0 ** -53
C = 64.0
J32_MAX, LDS_MAX, GRID_MAX = 32, 96, 2048
NS_ENTRY = 2.0    # the fast path is entered when the row-sum bound of |G / mean diag - I| is below this (see ns_entry)
ORDERS = (1, 2, 3, 16, 17, 31, 32, 33, 64, 95, 96, 97, 98, 128, 129, 256)
MODES = {0: "eig", 1: "whiten", 2: "lowdin", 3: "pivchol"}


# ---- the dispatch, restated ------------------------------------------------------------------------------------------
def route(n, mode):
    """Which device code serves rom_small_eig_host(n, mode): "jacobi32" (kb_jacobi32 -> jacobi32_run), "lds" (kb_small_eig in
    LDS, one workgroup), "grid" (jacobi_grid: one launch per round) or "pivchol" (kb_pivchol_whiten / ...32)."""
    assert 1 <= n <= GRID_MAX and mode in MODES
    if mode == 3:
        assert n <= LDS_MAX
        return "pivchol"
    if n > LDS_MAX:
        return "grid"
    return "jacobi32" if (n <= J32_MAX and mode == 0) else "lds"


def reachable_cells():
    """Every (route, mode, gram_like) the entry point can reach: pivchol ignores gram_like (listed once, as 1)."""
    cells = set()
    for rt, modes in (("jacobi32", (0,)), ("lds", (0, 1, 2)), ("grid", (0, 1, 2))):
        cells |= {(rt, m, g) for m in modes for g in (0, 1, 2)}
    cells.add(("pivchol", 3, 1))
    return cells


def slot(p, q, n):
    """The round-robin slot in which the pair (p, q) of an order-n matrix is rotated: with ne = n + (n & 1), index ne - 1 stays
    in slot 0 (for odd n it is the padding: slot 0 holds no real pair), every other pair sits in the slot k of 1 .. ne/2 - 1
    with 2 k = +-(q - p) mod (ne - 1) -- in round r slot k holds ((r + k) mod (ne - 1), (r - k) mod (ne - 1))."""
    ne = n + (n & 1)
    p, q = min(p, q), max(p, q)
    assert 0 <= p < q < n
    if q == ne - 1:
        return 0
    d = q - p
    k = d // 2 if d % 2 == 0 else (ne - 1 - d) // 2
    assert 1 <= k <= ne // 2 - 1 and ((2 * k - d) % (ne - 1) == 0 or (2 * k + d) % (ne - 1) == 0)
    return k


def real_slots(n):
    """Slots that hold a real pair: all of 0 .. ne/2 - 1 for even n, 1 .. ne/2 - 1 for odd n."""
    ne = n + (n & 1)
    return list(range(n & 1, ne // 2))


def wave0_slots(n):
    """jacobi32_run: thread t = k * half + l records the rotation of slot k; the slots whose threads include one of the
    first 64 (wave 0) are k <= 63 // half -- all of them up to n = 16, 4 of 16 at n = 32."""
    half = (n + (n & 1)) // 2
    return [k for k in range(half) if k * half < 64]


COUPLING = np.array([[0.0, 0.25, 0.5], [0.25, 0.0, 0.375], [0.5, 0.375, 0.0]])


def triple_slots(tr, n):
    a, b, c = tr
    return {slot(a, b, n), slot(a, c, n), slot(b, c, n)}


def coverage_triples(n):
    """Index triples (0, a, b) whose coupled pairs between them sit in every real slot: greedy set cover (deterministic;
    among equal gains the triple with the most slots outside wave 0's, then the smallest).  n = 32 starts with (0, 1, 9):
    slots 15, 4, 11, none of which wave 0 of jacobi32_run owns."""
    assert n >= 3
    want = set(real_slots(n))
    w0 = set(wave0_slots(n)) if n <= J32_MAX else set()
    out = [(0, 1, 9)] if n == 32 else []
    have = set().union(*[triple_slots(t, n) for t in out]) if out else set()
    cands = [(0, a, b) for a in range(1, n) for b in range(a + 1, n)]
    cs = {t: triple_slots(t, n) for t in cands}
    while have != want:
        best = max(cands, key=lambda t: (len(cs[t] - have), len(cs[t] - w0), -t[1], -t[2]))
        assert cs[best] - have
        out.append(best)
        have |= cs[best]
    return out


def assert_coverage(n, triples):
    got = set().union(*[triple_slots(t, n) for t in triples])
    assert got == set(real_slots(n)), (n, sorted(set(real_slots(n)) - got))


# ---- Hadamard pieces ---------------------------------------------------------------------------------------------------
def hadamard(m):
    return rf.hadamard_columns(m, np.arange(m))


def _pow2_below(n):
    m = 1
    while 2 * m <= n:
        m *= 2
    return m


# ---- exact spectra -----------------------------------------------------------------------------------------------------
FAMILIES = ("distinct", "triple", "indefinite", "zero", "scalar", "null", "diagonal")


def family_spectrum(n, family):
    """(d / m as integers c, e) of the family; None where the order is too small for it."""
    m = _pow2_below(n)
    r = n - m
    c = np.arange(m, 0, -1, dtype=np.int64)             # d = m c: m^2, ..., 2 m, m
    e = m * np.arange(r, dtype=np.int64) + 1 if m > 1 else np.arange(r, dtype=np.int64) + 2   # = 1 mod m: never a d
    if family == "distinct":
        return c, e
    if family == "triple":
        if n < 3:
            return None
        if r:
            c[1] = c[0]
            e[0] = m * c[0]                              # the eigenspace straddles the two blocks
        else:
            c[1] = c[2] = c[0]
        return c, e
    if family == "indefinite":
        if n < 2:
            return None
        return c * np.where(np.arange(m) % 2, -1, 1), e * np.where(np.arange(r) % 2, 1, -1)
    if family == "zero":
        c = c.copy()
        c[-1] = 0
        return c, e
    return None


class ExactCase:
    def __init__(self, n, family, seed=0):
        self.n, self.family = n, family
        self.id = f"{family}-n{n}"
        m = self.m = _pow2_below(n)
        r = n - m
        rng = np.random.default_rng(1000 * n + seed)
        self.perm = rng.permutation(n)
        self.v = np.zeros(n)
        if family in ("scalar", "null", "diagonal"):
            if family == "scalar":
                self.lam_all = np.full(n, 3.0)
                self.A = 3.0 * np.eye(n)
            elif family == "null":
                self.lam_all = np.zeros(n)
                self.A = np.zeros((n, n))
            else:
                dg = (rng.integers(-3, 4, n)).astype(np.float64)   # unsorted, with ties, both signs and zeros
                self.lam_all = dg
                self.A = np.diag(dg)
            self.Qv = np.eye(n)                          # eigenvector k (column) belongs to lam_all[k]
            self.int_scale = 1
            return
        c, e = family_spectrum(n, family)
        self.c, self.e = c, e
        H = hadamard(m)
        if n >= 4:
            rows = ([0, m - 1, m, n - 1] if r >= 2 else [0, 1, m - 1, m] if r == 1 else [0, 1, m - 2, m - 1])
            self.v[rows] = [1.0, -1.0, 1.0, -1.0]
        B = np.zeros((n, n))
        B[:m, :m] = (H * c.astype(np.float64)) @ H.T     # = H diag(d) H^T / m: integers
        B[m:, m:] = np.diag(e.astype(np.float64))
        Q = np.eye(n) - np.outer(self.v, self.v) / 2
        A = Q @ B @ Q                                    # quarters of integers: every product and sum exact
        self.A = A[np.ix_(self.perm, self.perm)]         # = P A P^T with (P x)_i = x_perm[i]
        self.lam_all = np.concatenate([m * c, e]).astype(np.float64)
        W = np.zeros((n, n))
        W[:m, :m] = H                                    # columns, not normalised
        W[m:, m:] = np.eye(r)
        self.W2 = (2 * (Q @ W))[self.perm]               # 2 P Q W: integers; column k is an eigenvector of lam_all[k]
        nrm = np.concatenate([np.full(m, np.sqrt(float(m))), np.ones(r)])
        self.Qv = (self.W2 / 2) / nrm
        self.int_scale = 4

    @property
    def norm2(self):
        return float(np.abs(self.lam_all).max())

    def sorted_lam(self):
        return np.sort(self.lam_all)[::-1]

    def clusters(self):
        """[(value, [columns of Qv])] in descending order of the eigenvalue."""
        vals = sorted(set(self.lam_all.tolist()), reverse=True)
        return [(v, np.flatnonzero(self.lam_all == v)) for v in vals]

    def gap(self, value):
        other = [abs(value - v) for v in set(self.lam_all.tolist()) if v != value]
        return min(other) if other else np.inf


def exact_cases(orders=ORDERS):
    out = []
    for n in orders:
        for fam in FAMILIES:
            if fam in ("scalar", "null", "diagonal") or family_spectrum(n, fam) is not None:
                out.append((n, fam))
    return out


# ---- pair coverage -----------------------------------------------------------------------------------------------------
class CoupledCase:
    def __init__(self, n, triple):
        import mpmath
        self.n, self.triple = n, tuple(triple)
        self.id = f"coupled-n{n}-{'_'.join(map(str, triple))}"
        A = np.diag(np.arange(1.0, n + 1))
        ix = np.array(triple)
        A[np.ix_(ix, ix)] += COUPLING
        self.A = A
        with mpmath.workdps(50):
            blk = mpmath.matrix([[mpmath.mpf(float(A[i, j])) for j in triple] for i in triple])
            ev = [mpmath.mpf(x) for x in mpmath.eigsy(blk, eigvals_only=True)]
            rest = [mpmath.mpf(i + 1) for i in range(n) if i not in triple]
            self.lam_mp = sorted(ev + rest, reverse=True)
        self.lam = np.array([float(x) for x in self.lam_mp])
        self.norm2 = float(self.lam[0])


# ---- inverse square roots with exact answers ---------------------------------------------------------------------------
def ns_entry(G):
    """The fast-path condition of kb_small_eig restated: (row-sum bound of |G / g - I|, g = mean diagonal) and whether the
    Newton-Schulz iteration is entered (bound < NS_ENTRY = 2: then the spectrum of G / g lies in (0, 3), W = (3 I - Z Y) / 2
    stays positive definite and the iteration can only reach the PRINCIPAL inverse square root)."""
    G = np.asarray(G, dtype=np.float64)
    g = np.trace(G) / len(G)
    if not g > 0:
        return np.inf, False
    esum = float(np.abs(G / g - np.eye(len(G))).sum(axis=1).max())
    return esum, esum < NS_ENTRY


# exponents j of d = 4^j by eighths of the index range (levels[i] for indices k with 8 k // m == i), and the situation
INVSQRT = {
    # G / g in {0.4, 1.6}: inside (0, 2), Newton-Schulz converges
    "ns_converges": (0, 0, 0, 0, 1, 1, 1, 1),
    # row-sum bound 1.91 < 2 with the eigenvalue 2.91 of G / g above 2 (one eighth at 4): still below 3, converges
    "ns_above_two": (0, 0, 0, 0, 0, 0, 0, 1),
    # row-sum bound 2.37 in [2, 3) with the eigenvalue 3.37 of G / g: 3 I - G / g is indefinite, the iteration would reach a
    # NON-principal root (a reflected direction) while its defect ||Z Y - I|| falls -- must go to Jacobi
    "ns_wrong_root": (0, 0, 0, 0, 0, 0, 2, 2),
    # row-sum bound 6.2 >= 3 (one eighth at 64)
    "jacobi": (0, 0, 0, 0, 0, 1, 2, 3),
    # singular: one eighth at d = 0 (level None); Newton-Schulz is entered, stalls and is abandoned
    "singular": (None, 0, 0, 0, 0, 1, 1, 1),
}


class InvSqrtCase:
    def __init__(self, m, kind):
        assert m >= 8 and m & (m - 1) == 0
        self.n = self.m = m
        self.kind = kind
        self.id = f"invsqrt-{kind}-n{m}"
        lev = INVSQRT[kind]
        idx = (8 * np.arange(m)) // m
        d = np.array([0.0 if lev[i] is None else 4.0 ** lev[i] for i in idx])
        root = np.array([0.0 if lev[i] is None else 2.0 ** -lev[i] for i in idx])
        H = hadamard(m)
        self.d = d
        self.G = (H * d) @ H.T / m                       # exact: integers / m
        self.Tinv = (H * root) @ H.T / m                 # G^(-1/2) (pseudo-inverse for the singular family): exact
        pos = d[d > 0]
        self.kappa = float(pos.max() / pos.min())
        self.norm2 = float(d.max())
        self.tnorm2 = float(root.max())
        self.rank = int((d > 0).sum())
        self.H = H
        # between the eigenvalue bound C n eps relative to lam_max (<= 1.9e-12 at n = 256) and lam_min+ / lam_max >= 1 / 64
        self.rel_tol = 2.0 ** -30 if self.rank < m else 0.0

    def spectrum_over_g(self):
        return self.d / self.d.mean()


# ---- pivoted Cholesky with an exact factor -----------------------------------------------------------------------------
class PivCholCase:
    """X = diag(2^-i) L0 R: L0 unit lower bidiagonal with sub-diagonal 1/2, R = b rows (1 ...) of the Hadamard matrix of order
    mh (64; 256 for b > 63 -- an order-64 matrix has no 96 independent rows), R R^T = mh I.  G = X X^T = mh D L0 L0^T D is
    exact (tridiagonal, dyadic), its Cholesky factor is sqrt(mh) D L0 and T = L0^-1 D^-1 / sqrt(mh), entries
    (-1/2)^(i-j) 2^j / sqrt(mh).  The pivots (the residual diagonal 4^-k mh at step k against 1.25 4^-i mh behind it) come in
    the natural order: no swaps.  variant "perm": rows of X permuted (T's columns follow); "rank": the last k rows are copies
    of rows 0 .. k-1 -- their residual is exactly zero after their original's step, ties go to the lower index: rank b - k."""

    def __init__(self, b, variant="plain", seed=0):
        self.n = self.b = b
        self.variant = variant
        self.id = f"pivchol-{variant}-b{b}"
        mh = self.mh = 64 if b <= 63 else 256
        s = np.sqrt(float(mh))
        k = 0 if variant != "rank" else max(1, b // 4)
        r = self.rank = b - k
        D = 2.0 ** -np.arange(r)
        L0 = np.eye(r) + 0.5 * np.eye(r, k=-1)
        R = rf.hadamard_columns(mh, np.arange(1, r + 1)).T
        X = (D[:, None] * L0) @ R
        Tr = np.zeros((r, r))
        for i in range(r):
            for j in range(i + 1):
                Tr[i, j] = (-0.5) ** (i - j) * 2.0 ** j / s
        T = np.zeros((b, b))
        T[:r, :r] = Tr
        if k:
            X = np.vstack([X, X[:k]])
        self.lam = np.concatenate([mh * 4.0 ** -np.arange(r), np.zeros(k)])
        self.rows = np.arange(b)
        if variant == "perm":
            self.rows = np.random.default_rng(b + seed).permutation(b)
            X = X[self.rows]
            T = T[:, self.rows]                          # X'_i = X_rows[i]:  T' X' = T X  <=>  T'[:, i] = T[:, rows[i]]
        self.X, self.T = X, T
        self.G = X @ X.T                                  # exact: dyadic entries, short sums


def pivchol_cases():
    out = []
    for b in (1, 7, 24, 62, 96):
        out.append((b, "plain"))
        if b > 1:
            out += [(b, "perm"), (b, "rank")]
    return out


# ---- graded ------------------------------------------------------------------------------------------------------------
class GradedCase:
    def __init__(self, n):
        import mpmath
        self.n = n
        self.id = f"graded-n{n}"
        rng = np.random.default_rng(n)
        L = np.eye(n) + 0.25 * np.tril(rng.uniform(-1, 1, (n, n)), -1) / np.sqrt(n)
        B = L @ L.T
        B = 0.5 * (B + B.T)
        ex = np.round(53.0 * np.arange(n) / (n - 1)).astype(int)      # 2^-53 = 1.1e-16: sixteen decades
        d = 2.0 ** -ex
        self.A = (d[:, None] * B) * d[None, :]                          # exact scalings of the fp64 entries of B
        sc = 1 / np.sqrt(np.diag(B))
        self.kappa = float(min(np.linalg.cond(B), np.linalg.cond(sc[:, None] * B * sc[None, :])))
        with mpmath.workdps(90):
            M = mpmath.matrix(n, n)
            for i in range(n):
                for j in range(n):
                    M[i, j] = mpmath.mpf(float(self.A[i, j]))
            ev = sorted(mpmath.eigsy(M, eigvals_only=True), reverse=True)
            self.lam = np.array([float(x) for x in ev])
        assert self.lam.min() > 0 and self.lam.max() / self.lam.min() > 1e30


# ---- NumPy restatements ------------------------------------------------------------------------------------------------
def jacobi_host(A, gram_like=1, rule="all", max_sweeps=None):
    """Cyclic Jacobi in the device's round-robin order with its rotation criterion, plain fp64 (the rotation from the
    classical formulas).  rule "all": a sweep without any rotation ends the iteration; "wave0": only the rotations of the
    slots wave 0 of jacobi32_run owns are seen (the stop rule before the fix).  Returns lam (descending, ties by index),
    T (eigenvector rows) and the number of sweeps that rotated."""
    A = 0.5 * (np.array(A, dtype=np.float64) + np.array(A, dtype=np.float64).T)
    n = len(A)
    ne = n + (n & 1)
    half, nm1 = ne // 2, ne - 1
    if max_sweeps is None:
        max_sweeps = 40 if n <= LDS_MAX else 60
    V = np.eye(n)
    dmax = float(np.abs(np.diag(A)).max())
    nu2 = np.abs(np.diag(A)).copy() if gram_like else np.full(n, dmax)
    tol = (16.0 if gram_like == 2 else float(max(n, 8))) * 1.1e-16
    tol2, floor_abs = tol * tol, max(1e-300, 1e-40 * dmax)
    seen = set(wave0_slots(n)) if rule == "wave0" else set(range(half))
    ks = np.arange(half)
    sweeps = 0
    for _ in range(max_sweeps):
        any_seen = False
        for r in range(nm1):
            p = np.where(ks == 0, r, (r + ks) % nm1)
            q = np.where(ks == 0, nm1, (r - ks) % nm1)
            p, q = np.minimum(p, q), np.maximum(p, q)
            real = q < n
            kk, p, q = ks[real], p[real], q[real]
            app, aqq, apq = A[p, p], A[q, q], A[p, q]
            rot = (apq * apq > tol2 * np.abs(app * aqq)) & (np.abs(apq) > floor_abs) & (apq * apq > tol2 * nu2[p] * nu2[q])
            if not rot.any():
                continue
            any_seen = any_seen or bool(set(kk[rot].tolist()) & seen)
            p, q, app, aqq, apq = p[rot], q[rot], app[rot], aqq[rot], apq[rot]
            a, b = aqq - app, 2.0 * apq
            t = np.where(a >= 0, b, -b) / (np.abs(a) + np.hypot(a, b))
            c = 1.0 / np.sqrt(1.0 + t * t)
            s = t * c
            np2, nq2 = nu2[p].copy(), nu2[q].copy()
            nu2[p], nu2[q] = c * c * np2 + s * s * nq2, s * s * np2 + c * c * nq2
            Ap, Aq = A[p].copy(), A[q].copy()
            A[p], A[q] = c[:, None] * Ap - s[:, None] * Aq, s[:, None] * Ap + c[:, None] * Aq
            Ap, Aq = A[:, p].copy(), A[:, q].copy()
            A[:, p], A[:, q] = c * Ap - s * Aq, s * Ap + c * Aq
            Vp, Vq = V[p].copy(), V[q].copy()
            V[p], V[q] = c[:, None] * Vp - s[:, None] * Vq, s[:, None] * Vp + c[:, None] * Vq
        if not any_seen:
            break
        sweeps += 1
    ev = np.diag(A).copy()
    perm = np.argsort(-ev, kind="stable")
    return ev[perm], V[perm], sweeps


def transform_from_eig(lam, T, mode, rel_tol):
    keep = (lam > rel_tol * lam[0]) & (lam > 0)
    sc = np.where(keep, 1.0 / np.sqrt(np.where(keep, lam, 1.0)), 0.0)
    if mode == 1:
        return sc[:, None] * T
    return (T.T * sc) @ T


def newton_schulz_host(G, entry=NS_ENTRY):
    """kb_small_eig's coupled Newton-Schulz iteration restated.  Returns ("skipped" | "abandoned" | "converged", T or None)."""
    G = np.array(G, dtype=np.float64)
    n = len(G)
    g = np.trace(G) / n
    if not g > 0 or not np.abs(G / g - np.eye(n)).sum(axis=1).max() < entry:
        return "skipped", None
    Y, Z, I = G / g, np.eye(n), np.eye(n)
    prev = 1e300
    for it in range(20):
        ZY = Z @ Y
        dev = np.abs(ZY - I).max()
        W = 0.5 * (3 * I - ZY)
        if dev < 4e-16 * n:
            return "converged", (0.5 * (Z + Z.T)) / np.sqrt(g)
        if not dev < prev or it == 19:
            return "abandoned", None
        prev = dev
        Y, Z = Y @ W, W @ Z
    return "abandoned", None


def small_eig_host(A, mode, rel_tol=0.0, gram_like=1, entry=NS_ENTRY):
    """The whole entry point restated for modes 0, 1, 2: (lam, T, path) with path "ns" (lam = the diagonal of A, as the kernel
    reports on its fast path) or "jacobi"."""
    n = len(A)
    if mode != 0 and n <= LDS_MAX:
        st, T = newton_schulz_host(A, entry)
        if st == "converged":
            return np.diag(np.asarray(A, dtype=np.float64)).copy(), T, "ns"
    lam, T, _ = jacobi_host(A, gram_like)
    return lam, (T if mode == 0 else transform_from_eig(lam, T, mode, rel_tol)), "jacobi"


def pivchol_host(G, rel_tol=0.0):
    """Pivoted Cholesky whitening as kb_pivchol_whiten: largest remaining diagonal entry (first on ties), stop at the first
    pivot <= rel_tol x the first or <= 0; T = [L_r^-1 0] P, lam = squared pivots, zeros behind the rank."""
    A = 0.5 * (np.array(G, dtype=np.float64) + np.array(G, dtype=np.float64).T)
    n = len(A)
    perm = np.arange(n)
    rank, first = n, 0.0
    for k in range(n):
        dg = np.diag(A)[k:]
        pv = k + int(np.argmax(dg))
        if k == 0:
            first = dg.max()
        if not (A[pv, pv] > rel_tol * first and A[pv, pv] > 0):
            rank = k
            break
        if pv != k:
            A[[k, pv]] = A[[pv, k]]
            A[:, [k, pv]] = A[:, [pv, k]]
            perm[[k, pv]] = perm[[pv, k]]
        lkk = np.sqrt(A[k, k])
        A[k + 1:, k] /= lkk
        A[k, k] = lkk
        A[k + 1:, k + 1:] -= np.outer(A[k + 1:, k], A[k + 1:, k])
    Li = np.zeros((n, n))
    for j in range(rank):
        for i in range(j, rank):
            s = (1.0 if i == j else 0.0) - A[i, j:i] @ Li[j:i, j]
            Li[i, j] = s / A[i, i]
    T = np.zeros((n, n))
    T[:rank, perm[:rank]] = Li[:rank, :rank]
    lam = np.array([A[i, i] ** 2 if i < rank else 0.0 for i in range(n)])
    return lam, T


# ---- the measures and their bounds ---------------------------------------------------------------------------------------
def norm2_ld(R):
    """Spectral norm of a residual formed in long double."""
    return float(np.linalg.norm(np.asarray(R, dtype=np.float64), 2))


def eig_measures(A, lam, T, norm2):
    """(name, observed, bound) of a mode-0 result that need no truth: orthonormality and the decomposition, in long double."""
    n = len(A)
    Tl, Al = np.asarray(T, dtype=LD), np.asarray(A, dtype=LD)
    out = [("orthonormality ||T T^T - I||_2", norm2_ld(Tl @ Tl.T - np.eye(n)), C * n * EPS)]
    if norm2 > 0:
        out.append(("residual ||T A T^T - diag(lam)||_2 / ||A||_2", norm2_ld(Tl @ Al @ Tl.T - np.diag(np.asarray(lam, dtype=LD))) / norm2,
                    C * n * EPS))
    return out


def exact_measures(case, lam, T):
    """Eigenvalues (C n eps ||A||), eigenvectors / spectral projectors of each cluster (angle <= C n eps ||A|| / gap), order."""
    n, nrm = case.n, case.norm2
    out = [("eigenvalues |lam - truth|", float(np.abs(lam - case.sorted_lam()).max()), C * n * EPS * nrm)]
    out += eig_measures(case.A, lam, T, nrm)
    Tl = np.asarray(T, dtype=LD)
    at = 0
    worst = 0.0
    for value, cols in case.clusters():
        k = len(cols)
        if k < n:
            Qs = np.asarray(case.Qv[:, cols], dtype=LD)
            rows = Tl[at:at + k]
            # sine of the largest angle between span(rows) and the true eigenspace: ||(I - Qs Qs^T) rows^T||_2
            sin = norm2_ld(rows.T - Qs @ (Qs.T @ rows.T))
            worst = max(worst, sin / (C * n * EPS * nrm / case.gap(value)))
        at += k
    out.append(("eigenspaces: sine of the angle / (C n eps ||A|| / gap)", worst, 1.0))
    return out


def whitening_measure(G, T, rank, kappa):
    """||T G T^T - (I_rank (+) 0)||_2 <= C n eps kappa(G), formed in long double."""
    n = len(G)
    Tl, Gl = np.asarray(T, dtype=LD), np.asarray(G, dtype=LD)
    return norm2_ld(Tl @ Gl @ Tl.T - np.diag((np.arange(n) < rank).astype(LD))), C * n * EPS * kappa


# ---- recording -----------------------------------------------------------------------------------------------------------
def record(route_, n, mode, gram_like, case_id, measures):
    """Append one JSON line per case to $ROMHC_SMALL_DENSE_JSON: route, n, mode, observed / bound of every measure."""
    path = os.environ.get("ROMHC_SMALL_DENSE_JSON")
    if not path:
        return
    with open(path, "a") as f:
        f.write(json.dumps({"case": case_id, "route": route_, "n": int(n), "mode": int(mode), "gram_like": int(gram_like),
                            "observed_over_bound": {nm: (float(v / b) if b > 0 else float(v)) for nm, v, b in measures}}) + "\n")
