"""Truth for the point-sensor stage (csrc/rom_riesz.hip, csrc/rom_sensors.hip: rom_riesz_h10, rom_riesz_norms_h10,
rom_sensor_greedy; select_sensors_pbdw / sensor_beta_prefix on top).  TEST INFRASTRUCTURE: nothing in the product path may
import this.  tests/test_sensor_truth_host.py proves it on the CPU, tests/test_gpu_sensor_truth.py uses it on the device.

  * the cases: grids (h10_truth.grid), candidate sets (all interior vertices, random points, the "edges" / "vertices" /
    "interfaces" families of test_gpu_riesz_pbdw._points, east and north boundary points, exact duplicates), bases with a
    known condition number kappa_V of their A_1-normalised Gram matrix (random rows, random combinations of low sine modes)
    and bases with planted dead rows (a zero row, an exact duplicate, an exact integer combination of two earlier rows);
  * the truth, all in 80-bit long double: R (h10_truth.evaluation_rows), Omega = A_1^-1 R through the sine tables, G = R
    Omega^T, nu = diag G, W (referee.a1_orthonormal_span_ld; its `keep` is the dead-row truth), E = R W^T, and TruthState:
    the greedy's state following GIVEN picks (and, in the worst-case mode, the given alpha)
        L[k, :k] = Phi[:k, p],  L_kk^2 = nu_p - sum L^2,  A[k] = Res[:, p] / L_kk,
        Phi[k] = (G[p] - L[k, :k] Phi[:k]) / L_kk,  Res -= A[k]^T Phi[k],
    the criterion of both modes, kappa_k = max_{j<=k} nu_{p_j} / L_jj^2, lambda_min(A_k^T A_k) from an 80-bit Jacobi;
  * riesz_host, norms_host, greedy_host: a plain fp64 NumPy restatement of the device's recurrences (same order of the
    recurrences, not the kernels' bits), with the planted mutations of MUTATIONS selectable;
  * the bounds (EPS = 2^-53, C = 64, the project's convention) and check_points / check_greedy, which hold the restatement
    (on the CPU) and the device (on the GPU) to the same assertions.

The bounds.  Representers per row: h10_truth.riesz_bound.  Gram matrix: |G_ij - T_ij| <= (C eps (nr + nc) + dim eps)
sqrt(T_ii T_jj) (the formation of the spectral rows, and gamma_dim of a dot product in any order).  Norms: |nu - T| <= C eps
(nr + nc) T (every table entry is a sum whose absolute terms are bounded through Cauchy-Schwarz by the all-positive T_00
sums).  Greedy at step k, with u_k = C eps (k + n + nr + nc) kappa_k (1 + kappa_V):  1 - c_k(p_k) / max c_k <= u_k,
|crit_out[k] - c_k(p_k)| <= u_k c_k(p_k),  max|A - A_truth| <= u_m max|A_truth|,  | ||alpha|| - 1 | <= C eps n,
(||A_k alpha||^2 - lambda_min) / ||A_k||^2 <= C eps n.  kappa_V is the condition number of the A_1-normalised Gram matrix of
the live rows (the call returns no W, so the span the device orthonormalised is known only to eps kappa_V).  The form of
u_k is not derived rigorously: test_sensor_truth_host.py justifies it by holding the restatement 8x inside it on every case.
beta_j (where above 1e-6): Weyl, |beta - beta_truth| <= ||A - A_truth||_2 <= sqrt(j n) u_m max|A_truth|, plus C eps n
||A||_2 for the two fp64 SVDs.
"""
import json
import os

import numpy as np

from conftest import observed
import h10_truth as ht
import referee as rf
import small_dense_truth as sd
from test_gpu_riesz_pbdw import _points   # the point families, unchanged

LD = np.longdouble
EPS = 2.0 ** -53
C = 64.0
RZ_MAX_ROWS = 65535 * 64      # rows of riesz_transform_c per launch (csrc/rom_riesz.hip)
SG_TPB, SG_SELECT = 256, 1024  # candidates per workgroup of ks_step; threads of ks_select (csrc/rom_sensors.hip)
A1_DEAD_REL = 1e-26           # the dead-row rule of romb_a1_append, in squared norms (1e-13 of the row's norm)
MODES = {0: "collective", 1: "worst"}
MARGIN = 8.0                  # the restatement sits this far inside every bound (as tests/test_resid_host.py)

# (blocks, N): smaller than a tile; square; 23 x 15; 71 x 47, across a 64-row tile
GRIDS = [((1, 1), 8), ((2, 2), 8), ((3, 2), 8), ((3, 2), 24)]
SIZE_GRID = ((1, 1), 4)       # 3 x 3: the two size cases
MUTATIONS = ("phi_tail", "chol256", "tie_high", "dead_alpha", "split0", "pair_shift", "first_row")


# ---- points ---------------------------------------------------------------------------------------------------------
class Domain:
    """What _points reads of a SolutionsManager, from the oracle geometry of a grid."""

    def __init__(self, gr):
        g = gr.g
        self.x_domain, self.y_domain, self.points_c, self.points_r = g.x_domain, g.y_domain, g.points_c, g.points_r
        self.blocks_geometry = gr.blocks


def vertices(gr):
    """(dim, 2) interior mesh vertices in dof order (SolutionsManager.interior_vertices)."""
    X, Y = np.meshgrid(gr.g.points_c[1:-1], gr.g.points_r[1:-1])
    return np.c_[X.ravel(), Y.ravel()]


def boundary_points(gr, m, seed):
    """m points on the east and north edges of the domain (inside it for the locating convention; nu = 0)."""
    rng = np.random.default_rng(seed)
    (x0, x1), (y0, y1) = gr.g.x_domain, gr.g.y_domain
    h = (m + 1) // 2
    return np.r_[np.c_[np.full(h, x1), rng.uniform(y0, y1, h)], np.c_[rng.uniform(x0, x1, m - h), np.full(m - h, y1)]]


def families(gr, seed):
    """Every point family: random, edges (grid lines and diagonals), vertices, block interfaces, boundary."""
    d = Domain(gr)
    return np.r_[_points(d, "random", 20, seed), _points(d, "edges", 4, seed + 1), _points(d, "vertices", 6, seed + 2),
                 _points(d, "interfaces", 3, seed + 3), boundary_points(gr, 4, seed + 4)]


def point_set(gr, npts, seed):
    """npts points that take in every family (round robin over the families), the last one an exact duplicate of the
    first when npts > 2."""
    d = Domain(gr)
    fam = [_points(d, "random", npts, seed), _points(d, "edges", npts, seed + 1), _points(d, "vertices", npts, seed + 2),
           _points(d, "interfaces", npts, seed + 3), boundary_points(gr, npts, seed + 4)]
    P = np.array([fam[i % 5][i // 5] for i in range(npts)])
    if npts > 2:
        P[-1] = P[0]
    return P


def candidates(gr, n_random, seed, dups=4):
    """All interior vertices, n_random random points, the families, boundary points and `dups` exact duplicates."""
    rng = np.random.default_rng(seed)
    P = np.r_[vertices(gr), _points(Domain(gr), "random", n_random, seed + 10), families(gr, seed)]
    return np.r_[P, P[rng.choice(len(P), dups, replace=False)]]


def locate(gr, pts):
    """(ix, iy, tx, ty) as SolutionsManager._locate / the oracle's evaluate_solutions."""
    P = np.asarray(pts, dtype=np.float64).reshape(-1, 2)
    pc, pr = gr.g.points_c, gr.g.points_r
    ix = np.searchsorted(pc, P[:, 0]) - 1
    iy = np.searchsorted(pr, P[:, 1]) - 1
    tx = (P[:, 0] - pc[ix]) / (pc[ix + 1] - pc[ix])
    ty = (P[:, 1] - pr[iy]) / (pr[iy + 1] - pr[iy])
    return ix.astype(np.int32), iy.astype(np.int32), tx, ty


def first_occurrence(loc):
    """For every point the lowest index of a point with the same (ix, iy, tx, ty): the tie rule's truth."""
    seen, out = {}, np.zeros(len(loc[0]), dtype=np.int64)
    for i, key in enumerate(zip(*[np.asarray(a).tolist() for a in loc])):
        out[i] = seen.setdefault(key, i)
    return out


# ---- bases ----------------------------------------------------------------------------------------------------------
def basis_rows(gr, n, kind, seed):
    """n fp64 rows: "random" (standard normal), or "modes": random combinations of the lowest 2 n sine modes (smooth)."""
    rng = np.random.default_rng(seed)
    if kind == "random":
        return rng.standard_normal((n, gr.dim))
    assert kind == "modes"
    order = np.argsort(np.asarray(gr.lam, dtype=np.float64).ravel(), kind="stable")[:min(2 * n, gr.dim)]
    coef = np.zeros((n, gr.dim))
    coef[:, order] = rng.standard_normal((n, len(order)))
    return np.asarray(gr.transform(coef, 0, 0), dtype=np.float64)


def plant_dead(Cm, where):
    """Cm with three clearly dead rows inserted: a zero row, an exact duplicate of an earlier live row and an exact integer
    combination of two earlier live rows.  "first": the zero row is row 0 and the other two follow the two live rows they
    depend on; "middle" / "last": the three together in the middle / at the end.  (The entries are rounded to multiples of
    2^-20 first, so the combination is exact.)"""
    Cm = np.round(np.asarray(Cm) * 2.0 ** 20) / 2.0 ** 20
    n = len(Cm)
    zero, dup, comb = np.zeros((1, Cm.shape[1])), Cm[1:2], 2.0 * Cm[0:1] - 3.0 * Cm[1:2]
    if where == "first":
        return np.vstack([zero, Cm[:2], dup, comb, Cm[2:]])
    at = {"middle": max(2, n // 2), "last": n}[where]
    return np.vstack([Cm[:at], zero, dup, comb, Cm[at:]])


def kappa_v(gr, Cm, keep):
    """Condition number of the A_1-normalised Gram matrix of the live rows."""
    L = Cm[keep]
    if len(L) <= 1:
        return 1.0
    G = np.asarray(rf._a1_dots_ld(gr.g, L.astype(LD), L.astype(LD)), dtype=np.float64)
    d = np.sqrt(np.diag(G))
    w = np.linalg.eigvalsh(G / d[:, None] / d[None, :])
    return float(w[-1] / w[0])


# ---- the truth ------------------------------------------------------------------------------------------------------
class PointTruth:
    """R (fp64), Z = (0,-2) of R, Omega = A_1^-1 R, G = R Omega^T, nu = diag G of the points, in long double."""

    def __init__(self, gr, pts):
        self.gr, self.pts = gr, np.asarray(pts, dtype=np.float64).reshape(-1, 2)
        self.loc = locate(gr, self.pts)
        self.R = ht.evaluation_rows(gr, self.pts)
        self.Z = gr.transform(self.R, 0, -2)
        self.Om = gr.transform(self.Z, 0, 0)
        Gs = gr.scale(gr.transform(self.R, 0, 0), -1)        # Rhat / sqrt(Lambda): G = Gs Gs^T, symmetric by construction
        self.G = Gs @ Gs.T
        self.nu = np.diag(self.G).copy()
        self.zero = ~np.any(self.R, axis=1)
        self.row_bound = ht.riesz_bound(gr, self.R, self.Z)

    def gram_bound(self):
        d = np.sqrt(np.asarray(self.nu, dtype=np.float64))
        return (C * EPS * (self.gr.nr + self.gr.nc) + self.gr.dim * EPS) * d[:, None] * d[None, :]

    def norm_bound(self):
        return C * EPS * (self.gr.nr + self.gr.nc) * np.asarray(self.nu, dtype=np.float64)


def jacobi_ld(A, sweeps=40):
    """Eigenvalues (ascending, fp64) of a symmetric matrix by cyclic two-sided Jacobi in 80-bit arithmetic, the round-robin
    order vectorised over the disjoint pairs of a round; rotation threshold 2^-62 sqrt(|a_pp a_qq|) or 2^-62 max|diag|."""
    A = np.array(A, dtype=LD)
    A = (A + A.T) / 2
    n = len(A)
    if n == 1:
        return np.asarray(np.diag(A), dtype=np.float64)
    ne = n + (n & 1)
    half, nm1 = ne // 2, ne - 1
    ks = np.arange(half)
    tol = LD(2) ** -62
    for _ in range(sweeps):
        rotated = False
        dmax = np.abs(np.diag(A)).max()
        for r in range(nm1):
            p = np.where(ks == 0, r, (r + ks) % nm1)
            q = np.where(ks == 0, nm1, (r - ks) % nm1)
            p, q = np.minimum(p, q), np.maximum(p, q)
            real = q < n
            p, q = p[real], q[real]
            app, aqq, apq = A[p, p], A[q, q], A[p, q]
            rot = (np.abs(apq) > tol * np.sqrt(np.abs(app * aqq))) & (np.abs(apq) > tol * tol * dmax)
            if not rot.any():
                continue
            rotated = True
            p, q, app, aqq, apq = p[rot], q[rot], app[rot], aqq[rot], apq[rot]
            a, b = aqq - app, 2 * apq
            t = np.where(a >= 0, b, -b) / (np.abs(a) + np.hypot(a, b))
            c = 1 / np.sqrt(1 + t * t)
            s = t * c
            Ap, Aq = A[p].copy(), A[q].copy()
            A[p], A[q] = c[:, None] * Ap - s[:, None] * Aq, s[:, None] * Ap + c[:, None] * Aq
            Ap, Aq = A[:, p].copy(), A[:, q].copy()
            A[:, p], A[:, q] = c * Ap - s * Aq, s * Ap + c * Aq
        if not rotated:
            break
    return np.sort(np.asarray(np.diag(A), dtype=np.float64))


class GreedyTruth:
    """The long-double quantities of one greedy case: the candidates' PointTruth, W / keep of the basis rows Cm, E = R W^T
    as Res0 (n, ncand), kappa_V, the tie rule's first occurrences."""

    def __init__(self, gr, Cm, cand, pt=None):
        self.gr, self.Cm, self.n = gr, np.asarray(Cm, dtype=np.float64), len(Cm)
        self.pt = pt if pt is not None else PointTruth(gr, cand)
        self.W, self.keep = rf.a1_orthonormal_span_ld(gr.g, self.Cm, drop=np.sqrt(A1_DEAD_REL))
        self.Res0 = self.W @ self.pt.R.astype(LD).T
        self.kv = kappa_v(gr, self.Cm, self.keep)
        self.first = first_occurrence(self.pt.loc)
        self.n_live = int(self.keep.sum())


class TruthState:
    """The greedy's state in long double, following given picks (module docstring)."""

    def __init__(self, tr, mode):
        self.tr, self.mode = tr, mode
        self.G, self.nu0 = tr.pt.G, tr.pt.nu
        self.nu = tr.pt.nu.copy()                     # masked as candidates are picked
        self.Res = tr.Res0.copy()
        self.Phi = np.zeros((0, len(self.nu)), dtype=LD)
        self.A = np.zeros((0, tr.n), dtype=LD)
        self.kappa = 1.0

    def criterion(self, alpha=None):
        num = np.sum(self.Res ** 2, axis=0) if self.mode == 0 else (np.asarray(alpha, dtype=LD) @ self.Res) ** 2
        ok = self.nu > 0
        out = np.zeros(len(self.nu), dtype=LD)
        out[ok] = num[ok] / self.nu[ok]
        return out

    def pivot2(self, p):
        return self.nu0[p] - np.sum(self.Phi[:, p] ** 2)

    def push(self, p):
        L = self.Phi[:, p].copy()
        d2 = self.pivot2(p)
        assert d2 > 0 and self.nu[p] > 0, "the pick's representer lies in the span of the earlier picks"
        lkk = np.sqrt(d2)
        a = self.Res[:, p] / lkk
        phi = (self.G[p] - L @ self.Phi) / lkk
        self.Res = self.Res - a[:, None] * phi[None, :]
        self.Phi = np.vstack([self.Phi, phi])
        self.A = np.vstack([self.A, a])
        self.kappa = max(self.kappa, float(self.nu0[p] / d2))
        self.nu[p] = 0

    def lambda_min(self):
        """lambda_min of A_k^T A_k on the live directions: 0 below n_live picks, else by the 80-bit Jacobi."""
        k = len(self.A)
        if k < self.tr.n_live or self.tr.n_live == 0:
            return 0.0
        Al = self.A[:, self.tr.keep]
        return float(jacobi_ld(Al.T @ Al)[0])


def u_bound(tr, k, kappa):
    gr = tr.gr
    return C * EPS * (k + tr.n + gr.nr + gr.nc) * kappa * (1.0 + tr.kv)


# ---- the fp64 restatement -------------------------------------------------------------------------------------------
def point_weights(gr, loc):
    """point_weights of csrc/rom_ops.h, vectorised: y, x (3, npts; -1 / 0 where the vertex is on the boundary), w."""
    ix, iy, tx, ty = [np.asarray(a) for a in loc]
    ix, iy = ix.astype(np.int64), iy.astype(np.int64)
    lower = tx + ty < 1
    w = np.where(lower, [1 - tx - ty, tx, ty], [tx + ty - 1, 1 - tx, 1 - ty])
    y = np.where(lower, [iy, iy, iy + 1], [iy + 1, iy + 1, iy])
    x = np.where(lower, [ix, ix + 1, ix], [ix + 1, ix, ix + 1])
    ok = (y >= 1) & (y <= gr.nr) & (x >= 1) & (x <= gr.nc)
    return np.where(ok, y - 1, -1), np.where(ok, x - 1, 0), np.where(ok, w, 0.0)


def gather(gr, U, pw):
    """k_eval_points: (K, npts) values of the rows U at the points."""
    y, x, w = pw
    U = np.atleast_2d(U)
    out = np.zeros((len(U), y.shape[1]))
    for t in range(3):
        out += w[t] * U[:, np.maximum(y[t], 0) * gr.nc + x[t]]
    return out


def _tables64(gr):
    return gr.Sr.astype(np.float64), gr.Sc.astype(np.float64), gr.lam.astype(np.float64)


def riesz_host(gr, loc, max_rows=RZ_MAX_ROWS, mut=(), gram=True):
    """rom_riesz_h10 restated: (OMEGA (npts, dim), G).  max_rows: the rows of the second transform per launch."""
    Sr, Sc, lam = _tables64(gr)
    y, x, w = point_weights(gr, loc)
    npts, nr, nc = y.shape[1], gr.nr, gr.nc
    Rhat = np.zeros((npts, nr, nc))
    for t in range(3):
        Rhat += w[t][:, None, None] * Sr[:, np.maximum(y[t], 0)].T[:, :, None] * Sc[x[t], :][:, None, :]
    Gs = (Rhat / np.sqrt(lam)).reshape(npts, -1)
    G = Gs @ Gs.T if gram else None
    What = np.ascontiguousarray((Rhat / lam).transpose(1, 0, 2))             # [j][i][k]
    Z = np.einsum("pj,jik->pik", Sr, What).reshape(nr * npts, nc)          # [p][i][k]
    out = What.reshape(nr * npts, nc).copy()                                  # the block the second product overwrites
    for r0 in range(0, nr * npts, max_rows):
        take = min(max_rows, nr * npts - r0)
        at = 0 if ("split0" in mut and r0) else r0
        out[at:at + take] = Z[at:at + take] @ Sc
    return out.reshape(nr, npts, nc).transpose(1, 0, 2).reshape(npts, gr.dim), G


def green_tables_host(gr):
    Sr, Sc, lam = _tables64(gr)
    Linv = 1.0 / lam
    Pr = [Sr.T ** 2, np.vstack([Sr.T[:-1] * Sr.T[1:], np.zeros((1, gr.nr))])]             # P_r^d[y, j]
    Pc = [Sc ** 2, np.hstack([Sc[:, :-1] * Sc[:, 1:], np.zeros((gr.nc, 1))])]             # P_c^d[k, x]
    Q = [Linv @ Pc[0], Linv @ Pc[1]]
    return np.array([[Pr[dy] @ Q[dx] for dx in range(2)] for dy in range(2)])


def norms_host(gr, loc, mut=()):
    """rom_riesz_norms_h10 restated: nu from the four vertex-pair Green tables, green_pair's index shifts included."""
    T = green_tables_host(gr)
    y, x, w = point_weights(gr, loc)

    def pair(ya, xa, yb, xb):
        dy, dx = yb - ya, xb - xa
        if dy < 0 or (dy == 0 and dx < 0):
            dy, dx, ya, xa = -dy, -dx, yb, xb
        if dx < 0 and "pair_shift" not in mut:
            xa -= 1
        return T[dy, int(dx != 0), ya, xa]

    out = np.zeros(y.shape[1])
    for p in range(y.shape[1]):
        s = 0.0
        for t in range(3):
            if y[t, p] < 0:
                continue
            s += w[t, p] * w[t, p] * T[0, 0, y[t, p], x[t, p]]
            for v in range(t + 1, 3):
                if y[v, p] >= 0:
                    s += 2.0 * w[t, p] * w[v, p] * pair(y[t, p], x[t, p], y[v, p], x[v, p])
        out[p] = s
    return out


def cgs2_host(gr, Cm):
    """romb_a1_append restated (dense A_1): W and the dead flags."""
    A1 = gr.a1_dense()
    n = len(Cm)
    W, AW, dead = np.zeros((n, gr.dim)), np.zeros((n, gr.dim)), np.zeros(n, dtype=bool)
    for i in range(n):
        w = np.array(Cm[i], dtype=np.float64)
        n0 = w @ (A1 @ w)
        nrm1 = n0
        if i:
            w = w - (AW[:i] @ w) @ W[:i]
            nrm1 = w @ (A1 @ w)
        dead[i] = not (nrm1 > A1_DEAD_REL * n0) or not (nrm1 > 0)
        w = np.zeros_like(w) if dead[i] else w / np.sqrt(nrm1)
        if i:
            w = w - (AW[:i] @ w) @ W[:i]
            nrm2 = w @ (A1 @ w)
            w = np.zeros_like(w) if (dead[i] or not nrm2 > 0) else w / np.sqrt(nrm2)
        W[i], AW[i] = w, A1 @ w
    return W, dead


def greedy_host(gr, Cm, loc, m, mode, rel_tol, mut=()):
    """rom_sensor_greedy restated in fp64: (picks, crit, A, alpha or None, info) as FE.sensor_greedy returns them."""
    n = len(Cm)
    W, dead = cgs2_host(gr, Cm)
    pw = point_weights(gr, loc)
    ncand = pw[0].shape[1]
    nu = norms_host(gr, loc)
    Res = gather(gr, W, pw)
    Phi = np.zeros((m, ncand))
    picks, crit = np.full(m, -1, dtype=np.int64), np.zeros(m)
    A, alpha = np.zeros((m, n)), (np.zeros((m, n)) if mode else None)
    AtA = np.diag(np.where(dead, 0.0 if "dead_alpha" in mut else 2.0, 0.0))
    lkk = np.zeros(m)

    def eig():
        _, T, _ = sd.jacobi_host(AtA, gram_like=2)
        return T[0 if "first_row" in mut else n - 1].copy()

    def criterion(al):
        s = np.sum(Res ** 2, axis=0) if mode == 0 else (al @ Res) ** 2
        return np.where(nu > 0, s / np.where(nu > 0, nu, 1.0), 0.0)

    al = eig() if mode else None
    c = criterion(al)
    made, reason, c0 = 0, 0, 0.0
    for k in range(m):
        cmax = c.max()
        p = int(np.argmax(c)) if "tie_high" not in mut else int(ncand - 1 - np.argmax(c[::-1]))
        if k == 0:
            c0 = cmax
        if not cmax > 0.0:
            reason = 2
            break
        if k > 0 and cmax <= rel_tol * c0:
            reason = 1
            break
        L = Phi[:k, p].copy()
        if "chol256" in mut:
            L[256:] = 0.0
        d2 = nu[p] - np.sum(L * L)
        if not d2 > 0.0:
            reason = 2
            break
        picks[k], crit[k], made = p, cmax, made + 1
        if mode:
            alpha[k] = al
        lkk[k] = np.sqrt(d2)
        nu[p] = 0.0
        A[k] = Res[:, p] / lkk[k]
        AtA += np.outer(A[k], A[k])
        if k == m - 1:
            break
        g = gather(gr, riesz_host(gr, [a[p:p + 1] for a in loc], gram=False)[0], pw)[0]
        if mode:
            al = eig()
        s = g.copy()
        k4 = k - k % 4
        for j in range(k4):                      # (the device's 4-way unrolled part: the same sequential order)
            s -= L[j] * Phi[j]
        if "phi_tail" not in mut:
            for j in range(k4, k):
                s -= L[j] * Phi[j]
        Phi[k] = s / lkk[k]
        Res -= A[k][:, None] * Phi[k][None, :]
        c = criterion(al)
    info = {"dead_rows": int(dead.sum()), "picks": made, "stop_reason": reason, "host_syncs": 1}
    return picks, crit, A, alpha, info


# ---- the assertions, shared by the restatement and the device ---------------------------------------------------------
def check_points(pt, Om=None, G=None, nu=None):
    """(name, observed, bound) of representers, Gram matrix and squared norms against the truth of `pt`."""
    out = []
    if Om is not None:
        err = np.asarray(np.sqrt(np.sum((np.asarray(Om).astype(LD) - pt.Om) ** 2, axis=1)), dtype=np.float64)
        live = ~pt.zero
        out.append(("representers: row error / riesz_bound", float(np.max(err[live] / pt.row_bound[live], initial=0.0)), 1.0))
        out.append(("representers of vanishing functionals: max |entry|", float(np.abs(np.asarray(Om)[pt.zero]).max(initial=0.0)), 0.0))
    if G is not None:
        b = pt.gram_bound()
        d = np.abs(np.asarray(np.asarray(G).astype(LD) - pt.G, dtype=np.float64))
        live = np.outer(~pt.zero, ~pt.zero)
        out.append(("Gram matrix: |G - T| / ((C eps (nr + nc) + dim eps) sqrt(T_ii T_jj))", float(np.max(d[live] / b[live], initial=0.0)), 1.0))
        out.append(("Gram matrix, rows of vanishing functionals: max |entry|", float(np.abs(np.asarray(G)[~live]).max(initial=0.0)), 0.0))
        out.append(("Gram matrix: asymmetry |G - G^T|", float(np.abs(G - np.asarray(G).T).max(initial=0.0)), 0.0))
    if nu is not None:
        b = pt.norm_bound()
        d = np.abs(np.asarray(np.asarray(nu).astype(LD) - pt.nu, dtype=np.float64))
        live = ~pt.zero
        out.append(("squared norms: |nu - T| / (C eps (nr + nc) T)", float(np.max(d[live] / b[live], initial=0.0)), 1.0))
        out.append(("squared norms of vanishing functionals", float(np.abs(np.asarray(nu)[pt.zero]).max(initial=0.0)), 0.0))
    return out


def check_greedy(tr, mode, m, rel_tol, result, beta=None, expect_picks="generic"):
    """(name, observed, bound) of one greedy result (picks, crit, A, alpha, info) against the truth `tr`, following the
    result's picks and alpha.  Structural violations (a repeated or boundary pick, entries behind a stop) are reported as
    counts with bound 0.  beta: sensor_beta_prefix of the result's A, if it is to be checked.  expect_picks: the number of
    picks the run must make; "generic": min(m, distinct candidates with nu > 0) when rel_tol = 0 and a basis row is live, 0
    when none is (random bases and points: no criterion vanishes while such a candidate is left); None: not checked."""
    picks, crit, A, alpha, info = result
    n, gr = tr.n, tr.gr
    k = info["picks"]
    bad = int(info["dead_rows"] != int((~tr.keep).sum())) + int(not (0 <= k <= m))
    bad += int(np.any(picks[:k] < 0)) + int(np.any(picks[k:] != -1)) + int(np.any(crit[k:] != 0.0)) + int(np.any(A[k:] != 0.0))
    bad += int(len(set(picks[:k].tolist())) != k)
    bad += int(info["stop_reason"] != 0) if k == m else int(info["stop_reason"] not in (1, 2))
    bad += int((alpha is None) != (mode == 0))
    if expect_picks == "generic":
        expect_picks = None if rel_tol > 0 else min(m, len(set(tr.first[~tr.pt.zero].tolist()))) if tr.n_live else 0
    if expect_picks is not None:
        bad += int(k != expect_picks)
    if alpha is not None:
        bad += int(np.any(alpha[k:] != 0.0))
    out = [("structure: violations of the info / stop / padding contract", float(bad), 0.0)]
    pk = picks[:k]
    out.append(("tie rule: picks that are not the first occurrence of their point", float(np.sum(tr.first[pk] != pk)), 0.0))
    out.append(("picks with a vanishing functional", float(np.sum(tr.pt.zero[pk])), 0.0))
    dead = ~tr.keep
    out.append(("dead columns of A: max |entry|", float(np.abs(A[:, dead]).max(initial=0.0)), 0.0))
    if alpha is not None:
        out.append(("dead columns of alpha: max |entry|", float(np.abs(alpha[:, dead]).max(initial=0.0)), 0.0))
    st = TruthState(tr, mode)
    tie = crit_err = unit = eig = 0.0
    for s in range(k):
        p = int(pk[s])
        al = alpha[s] if mode else None
        c = st.criterion(al)
        cmax = c.max()
        if mode:
            unit = max(unit, abs(float(np.sqrt(np.sum(al.astype(LD) ** 2))) - 1.0) / (C * EPS * n))
            if s:
                a2 = float(np.sum(st.A ** 2))
                eig = max(eig, (float(np.sum((st.A @ al.astype(LD)) ** 2)) - st.lambda_min()) / a2 / (C * EPS * n))
        if not (st.nu[p] > 0 and c[p] > 0 and st.pivot2(p) > 0):
            out.append((f"step {s}: the pick has no positive criterion or pivot in the truth", 1.0, 0.0))
            return out
        st.push(p)
        u = u_bound(tr, s + 1, st.kappa)
        tie = max(tie, float(1 - c[p] / cmax) / u)
        crit_err = max(crit_err, abs(float((LD(crit[s]) - c[p]) / c[p])) / u)
    u_m = u_bound(tr, max(k, 1), st.kappa)
    out.append(("tie: (1 - c_k(p_k) / max c_k) / u_k", tie, 1.0))
    out.append(("criterion: |crit_out[k] - c_k(p_k)| / (u_k c_k(p_k))", crit_err, 1.0))
    if k:
        At = np.asarray(st.A, dtype=np.float64)
        amax = float(np.abs(At).max())
        out.append(("A: max|A - A_truth| / (u_m max|A_truth|)", float(np.abs(np.asarray(A[:k].astype(LD) - st.A, dtype=np.float64)).max()) / (u_m * amax), 1.0))
        if beta is not None and tr.n_live and k >= tr.n_live:
            worst = 0.0
            for j in range(tr.n_live, k + 1):
                sv = np.linalg.svd(At[:j], compute_uv=False)
                bt = sv[tr.n_live - 1]
                if bt > 1e-6:
                    worst = max(worst, abs(beta[j - 1] - bt) / (np.sqrt(j * n) * u_m * amax + C * EPS * n * sv[0]))
            out.append(("beta: |beta_j - beta_truth| / (sqrt(j n) u_m max|A_truth| + C eps n ||A||_2), beta_truth > 1e-6", worst, 1.0))
            out.append(("beta below n_live picks", float(np.abs(beta[:tr.n_live - 1]).max(initial=0.0)), 0.0))
    if mode:
        out.append(("| ||alpha|| - 1 | / (C eps n)", unit, 1.0))
        out.append(("(||A_k alpha||^2 - lambda_min) / ||A_k||^2 / (C eps n)", eig, 1.0))
    out.append(("kappa_k (recorded)", st.kappa, np.inf))
    out.append(("kappa_V (recorded)", tr.kv, np.inf))
    return out


def ratio(v, b):
    """observed / bound; a bound of 0 is exact: 0 or inf; recorded-only measures (bound inf) give 0."""
    if b == 0.0:
        return 0.0 if v == 0.0 else np.inf
    return float(v / b)


def worst_ratio(measures):
    return max(ratio(v, b) for _, v, b in measures)


def hold(who, tag, measures, inside=1.0):
    """Record the case, then assert: the exact measures (bound 0) exactly, every other one at most `inside` of its bound
    (through conftest.observed, in units of the bound)."""
    record(who, tag, measures)
    exact = [(nm, v) for nm, v, b in measures if b == 0.0 and v != 0.0]
    assert not exact, (tag, exact)
    for nm, v, b in measures:
        if np.isfinite(b) and b > 0.0:
            observed(f"{tag}: {nm}", ratio(v, b), inside)


def record(who, case_id, measures):
    """Append one JSON line (who: "device" / "restatement") to $ROMHC_SENSOR_TRUTH_JSON."""
    path = os.environ.get("ROMHC_SENSOR_TRUTH_JSON")
    if not path:
        return
    with open(path, "a") as f:
        f.write(json.dumps({"who": who, "case": case_id,
                            "observed_over_bound": {nm: (ratio(v, b) if np.isfinite(b) else float(v)) for nm, v, b in measures}}) + "\n")


# ---- the greedy cases of both test files --------------------------------------------------------------------------------
def _case(cid, grid, n, m, modes, basis="random", cand="full", rel_tol=0.0, dead=None, route=()):
    return dict(id=cid, grid=grid, n=n, m=m, modes=modes, basis=basis, cand=cand, rel_tol=rel_tol, dead=dead, route=route)


G15, G23, G7 = ((2, 2), 8), ((3, 2), 8), ((1, 1), 8)
GREEDY_CASES = [
    _case("n1", G15, 1, 5, (1,), route=("eig_jacobi32",)),
    _case("n2", G15, 2, 5, (1,), basis="modes"),
    _case("n10_m40", G15, 10, 40, (0, 1), basis="modes"),
    _case("n32", G15, 32, 34, (1,), route=("eig_jacobi32",)),
    _case("n33", G15, 33, 35, (1,), route=("eig_lds",)),
    _case("n96", G15, 96, 6, (1,), route=("eig_lds",)),
    _case("n128", G15, 128, 6, (0,), route=("collective_n128",)),
    _case("m1", G15, 10, 1, (0, 1)),
    _case("m2", G15, 10, 2, (0, 1)),
    _case("m5", G15, 10, 5, (0, 1)),
    _case("m260", G23, 20, 260, (0, 1), cand="vertices+40", route=("prep_beyond_256", "two_workgroups")),
    _case("ncand1", G15, 3, 2, (0, 1), cand=1),
    _case("ncand255", G15, 3, 4, (0, 1), cand=255),
    _case("ncand256", G15, 3, 4, (0, 1), cand=256),
    _case("ncand257", G15, 3, 4, (0, 1), cand=257, route=("two_workgroups",)),
    _case("dead_first", G15, 8, 16, (0, 1), dead="first", route=("dead_rows",)),
    _case("dead_middle", G15, 8, 16, (0, 1), basis="modes", dead="middle", route=("dead_rows",)),
    _case("dead_last", G15, 8, 16, (0, 1), dead="last", route=("dead_rows",)),
]
CASES = {c["id"]: c for c in GREEDY_CASES}
_TRUTHS = {}


def case_inputs(case):
    """(gr, Cm (rows, dead rows planted), cand (K, 2)) of a case."""
    gr = ht.grid(*case["grid"])
    seed = sum(map(ord, case["id"]))
    Cm = basis_rows(gr, case["n"], case["basis"], seed)
    if case["dead"]:
        Cm = plant_dead(Cm, case["dead"])
    kind = case["cand"]
    if kind == "full":
        cand = candidates(gr, 40, seed)
    elif kind == "vertices+40":
        cand = np.r_[vertices(gr), _points(Domain(gr), "random", 40, seed)]
    else:   # an exact number of candidates: families first, vertices behind them
        cand = np.r_[families(gr, seed), vertices(gr), _points(Domain(gr), "random", 64, seed + 5)][:kind]
        if kind == 1:
            cand = vertices(gr)[7:8]
    return gr, Cm, cand


def case_truth(case):
    if case["id"] not in _TRUTHS:
        gr, Cm, cand = case_inputs(case)
        _TRUTHS[case["id"]] = GreedyTruth(gr, Cm, cand)
    return _TRUTHS[case["id"]]
