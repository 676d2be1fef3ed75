"""Truth for the D-optimal sensor design (tests/test_dopt_host.py, tests/test_gpu_sensor_dopt.py): from a pick sequence the true
score of every candidate at every step, in numpy.longdouble and WITHOUT the recursion of the implementation, a forward-error bound
for a float64 evaluation after t recursive updates, and the checker of a design.  A helper, not a test file.  TEST INFRASTRUCTURE.

The truth.  In the coordinates whitened by the prior, w_{x,j} = Z0_j^T e_x (Z0_j = X_j T0 / sigma, the state of the empty design,
which is the checker's INPUT: the sensitivities have their own check, ``check_sensitivities``), the posterior precision of the
sensor set S at entry j is Gamma_0^(1/2) F_j(S) Gamma_0^(1/2) = H_j(S) = I + sum_{x in S} w w^T, so that
    log det(Gamma_0^-1 F_j(S)) = log det H_j(S),   score(x | S) = sum_j log1p(w_{x,j}^T H_j(S)^-1 w_{x,j}),
    posterior covariance = T0 H_j(S)^-1 T0^T
-- also where T0 is singular (a known parameter) and Gamma_0 does not exist.  H_j(S) is rebuilt from scratch for every prefix S of
the picks and factored in long double as H = R^T R through the Householder QR of the stacked factor [W_S^T; I] ((|S| + k) x k):
w^T H^-1 w = |R^-T w|^2.  A Cholesky of the assembled H would lose cond(H) eps_LD, which at sigma = 1e-6 (cond(H) ~ 1e12, eps_LD =
5e-20) is 1e-7 and MORE than the float64 recursion loses; the QR works at sqrt(cond(H)) eps_LD ~ 5e-14, a thousand times below
the bound that is checked.

The bound (``Truth.score_bound``).  Notation: eps = 2^-52; z_i the row i of Z_j (a k-vector), r_i(t) = |z_i| after t exact updates
= |R_t^-T z0_i| (the exact rows do not grow: every update multiplies by P = I - beta u u^T, whose eigenvalues are 1 and
1 / sqrt(1 + s)); A_i(t) a bound of the absolute error of the computed row after t updates, A_i(0) = 0.

 * Evaluation: the k dot products v = Z^T e of n terms (in any order, fused or not) are off by at most (n + 2) eps sum_i |e_i| |z_i|
   in norm, and the rows' own errors add sum_i |e_i| A_i:   dv = (n + 2) eps sum_i |e_i| r_i(t) + sum_i |e_i| A_i(t).
   s = |v|^2 in k more operations:  ds = 2 |v| dv + dv^2 + (k + 2) eps s.  log1p is 1-Lipschitz in s / (1 + s):
   d score = sum_j ds_j / (1 + s_j) + 4 eps sum_j log1p(s_j) [the rounding of log1p] + (M + 2) eps sum_j log1p(s_j) [the sum over j].
 * Update t -> t + 1 with the picked row e*: the computed u = Z^T e* is off by d = dv(e*) (above).  P depends on u through
   u u^T / (rho (rho + 1)), rho = sqrt(1 + s): |dP| <= 4 d / rho.  The update z <- z - (beta (z . u)) u of a row costs (k + 8) eps |z|
   in roundoff (beta |u|^2 = (rho - 1) / rho < 1), and errors already there pass through P, of norm 1:
       A_i(t + 1) = A_i(t) (1 + f) + r_i(t) f,   f = (k + 8) eps + 4 d / rho.
   This is where the accumulated sqrt(1 + s) enters: the errors are absolute and relative to the row norms BEFORE the shrinking,
   while the true v of a candidate near an earlier pick has been shrunk by 1 / rho of that pick -- relative to the score the bound
   grows like the product of the rho so far.  (At sigma = 1e-6 the first rho is ~1e6 and the scores afterwards are O(1): relative
   errors of 1e-10 are what the bound allows and what the recursion shows; a constant times eps would fail.)
 * The rows of T_j obey the same recursion from T0's rows, and posterior_sd_a = |row a of T_j|:  d sd = A^T_a + (k + 4) eps sd.
"""
import numpy as np

import lm_truth as lt

LD = np.longdouble
EPS = 2.0 ** -52


def case(n, k, M, ncand, seed):
    """A synthetic design problem: the reduced model of lm_truth.synth(n, k, 1, seed), theta (M, k) ~ U(0.2, log 100 - 0.2),
    candidate rows E (ncand, n) ~ N(0, 1) / sqrt(n)."""
    model = lt.synth(n, k, 1, seed)
    rng = np.random.default_rng(seed + 1000)
    theta = rng.uniform(0.2, np.log(100.0) - 0.2, size=(M, k))
    E = rng.standard_normal((ncand, n)) / np.sqrt(n)
    return dict(n=n, k=k, M=M, ncand=ncand, Ahat=model["Ahat"], bhat=model["bhat"], theta=theta, E=E)


def prior_variances(k):
    """The variance of a uniform law on the box [0, log 100] of lm_truth.synth, per parameter."""
    return np.full(k, np.log(100.0) ** 2 / 12.0)


def check_sensitivities(case_, X, status=None):
    """Every X_j (n, k) of X (M, n, k) is A(theta_j)^-1 [e^theta_q Ahat_q c]_q, c = A^-1 bhat, to 128 n eps cond_2(A) max|X_j|
    (two solves in a row, each a backward-stable factorisation) against the long-double solution, which comes from float64 LU
    with three steps of refinement on long-double residuals; entries of status != 0 must be zero.  Returns the largest ratio."""
    Ahat, bhat, theta = case_["Ahat"].astype(LD), case_["bhat"].astype(LD), case_["theta"]
    n = case_["n"]

    def solve(A, B):
        A64 = A.astype(np.float64)
        Y = np.linalg.solve(A64, B.astype(np.float64)).astype(LD)
        for _ in range(3):
            Y = Y + np.linalg.solve(A64, (B - A @ Y).astype(np.float64)).astype(LD)
        return Y

    worst = 0.0
    for j in range(len(theta)):
        if status is not None and status[j] != 0:
            assert not X[j].any(), f"entry {j}: skipped but X is not zero"
            continue
        ea = np.exp(theta[j].astype(LD))
        A = np.einsum("q,qij->ij", ea, Ahat)
        c = solve(A, bhat[:, None])[:, 0]
        want = solve(A, np.einsum("qij,j->iq", Ahat, c) * ea[None, :])
        err = float(np.abs(X[j].astype(LD) - want).max())
        bound = 128 * n * EPS * np.linalg.cond(A.astype(np.float64)) * float(np.abs(want).max())
        assert err <= bound, f"entry {j}: X off by {err:.3g} > {bound:.3g}"
        worst = max(worst, err / bound)
    return worst


def _householder_R(B):
    """R (M, k, k) upper triangular with B = Q R for the batch B (M, r, k), r >= k, long double."""
    B = B.copy()
    M, r, k = B.shape
    for c in range(k):
        x = B[:, c:, c]
        alpha = -np.where(x[:, 0] >= 0, LD(1), LD(-1)) * np.sqrt((x * x).sum(axis=1))
        v = x.copy()
        v[:, 0] -= alpha
        vv = (v * v).sum(axis=1)
        vv = np.where(vv > 0, vv, LD(1))
        B[:, c:, c:] -= (2 / vv)[:, None, None] * v[:, :, None] * np.einsum("mr,mrc->mc", v, B[:, c:, c:])[:, None, :]
    return np.triu(B[:, :k, :])


def _solve_RT(R, W):
    """Y = R^-T W for W (M, x, k): row-wise y with R^T y = w, by forward substitution."""
    k = R.shape[1]
    Y = np.zeros_like(W)
    for c in range(k):
        acc = W[:, :, c] - np.einsum("mxa,ma->mx", Y[:, :, :c], R[:, :c, c])
        Y[:, :, c] = acc / R[:, c, c, None]
    return Y


class Truth:
    """The true scores, posterior standard deviations and error bounds of the design states after 0 .. len(picks) picks.
    scores[t] (ncand,): the score of every candidate after t picks (NaN for a candidate row with NaN / Inf); score_bound[t]
    (ncand,); sd[t], sd_bound[t] (M, k)."""

    def __init__(self, Z0, T0, E, picks):
        Z0, T0, E = np.asarray(Z0, dtype=np.float64), np.asarray(T0, dtype=np.float64), np.asarray(E, dtype=np.float64)
        M, n, k = Z0.shape
        self.M, self.n, self.k, self.picks = M, n, k, [int(p) for p in picks]
        bad = ~np.isfinite(E).all(axis=1)
        Ec = np.where(bad[:, None], 0.0, E)
        absE = np.abs(Ec)
        W = np.einsum("xn,jnk->jxk", Ec.astype(LD), Z0.astype(LD))          # (M, ncand, k)
        Z0l = Z0.astype(LD)
        T0l = np.array(np.broadcast_to(T0.astype(LD), (M, k, k)))
        A, AT = np.zeros((M, n)), np.zeros((M, k))
        self.scores, self.score_bound, self.sd, self.sd_bound = [], [], [], []
        for t in range(len(self.picks) + 1):
            B = np.concatenate([W[:, self.picks[:t], :], np.array(np.broadcast_to(np.eye(k, dtype=LD), (M, k, k)))], axis=1)
            R = _householder_R(B)
            v = _solve_RT(R, W)
            s = (v * v).sum(axis=2)                                          # (M, ncand)
            r = np.sqrt((_solve_RT(R, Z0l) ** 2).sum(axis=2)).astype(np.float64)   # (M, n): the rows of Z_j
            rT = np.sqrt((_solve_RT(R, T0l) ** 2).sum(axis=2))               # (M, k): the rows of T_j = the posterior sd
            l = np.log1p(s)
            score = l.sum(axis=0)
            s64 = s.astype(np.float64)
            dv = (n + 2) * EPS * np.einsum("xi,ji->jx", absE, r) + np.einsum("xi,ji->jx", absE, A)
            ds = 2.0 * np.sqrt(s64) * dv + dv * dv + (k + 2) * EPS * s64
            bound = (ds / (1.0 + s64)).sum(axis=0) + (M + 6) * EPS * score.astype(np.float64)
            self.scores.append(np.where(bad, np.nan, score))
            self.score_bound.append(np.where(bad, np.nan, bound))
            self.sd.append(rT)
            self.sd_bound.append(AT + (k + 4) * EPS * rT.astype(np.float64))
            if t < len(self.picks):
                x = self.picks[t]
                f = (k + 8) * EPS + 4.0 * dv[:, x] / np.sqrt(1.0 + s64[:, x])
                A = A * (1.0 + f[:, None]) + r * f[:, None]
                AT = AT * (1.0 + f[:, None]) + rT.astype(np.float64) * f[:, None]

    def information(self, live):
        """Phi after every pick (len(picks),) in long double and its bound: the true gains summed over 2 live."""
        g = np.array([self.scores[t][x] for t, x in enumerate(self.picks)], dtype=LD)
        b = np.array([self.score_bound[t][x] for t, x in enumerate(self.picks)])
        info = np.cumsum(g) / (2 * LD(live))
        return info, np.cumsum(b) / (2.0 * live) + (np.arange(len(g)) + 3) * EPS * info.astype(np.float64)


def check_scores(truth, t, scores):
    """The score vector of the state after t picks lies within the bound (NaN or Inf exactly where the candidate's row has NaN / Inf).  Returns the
    largest ratio |score - truth| / bound."""
    want, bound = truth.scores[t], truth.score_bound[t]
    scores = np.asarray(scores, dtype=np.float64)
    nan = np.isnan(want)
    assert np.array_equal(~np.isfinite(scores), nan), f"step {t}: non-finite scores at {np.flatnonzero(~np.isfinite(scores))}, expected at {np.flatnonzero(nan)}"
    err = np.abs(scores.astype(LD) - want)[~nan]
    ratio = (err / bound[~nan]).astype(np.float64)
    bad = np.flatnonzero(ratio > 1.0)
    assert bad.size == 0, (f"step {t}: {bad.size} scores off by more than the bound, the worst {ratio.max():.3g} x "
                           f"(candidate {np.flatnonzero(~nan)[np.argmax(ratio)]})")
    return float(ratio.max()) if ratio.size else 0.0


def pick_gaps(truth):
    """Per step (gap, bound): the true score of the best unpicked candidate minus that of the second best, and the larger of
    their two bounds.  A step is DECIDED where gap > 2 bound: every float64 evaluation within the bound picks the same candidate."""
    out = []
    for t, _ in enumerate(truth.picks):
        sc = np.where(np.isnan(truth.scores[t]), -np.inf, truth.scores[t]).astype(np.float64)
        sc[truth.picks[:t]] = -np.inf
        order = np.argsort(-sc, kind="stable")
        if len(order) < 2 or not np.isfinite(sc[order[1]]):
            out.append((np.inf, 0.0))
            continue
        out.append((float(truth.scores[t][order[0]] - truth.scores[t][order[1]]),
                    float(max(truth.score_bound[t][order[0]], truth.score_bound[t][order[1]]))))
    return out


def check_design(Z0, T0, E, design, live=None, truth=None):
    """Raises AssertionError unless ``design`` (a SensorDesign) is a greedy D-optimal design for the empty state Z0 (M, n, k), T0
    and the candidate rows E to within roundoff: at every step the pick is unpicked, not a NaN candidate, and its TRUE score is not
    more than (its bound + the bound of the true maximum, at most twice the bound) below the true maximum over the unpicked
    candidates; gain and information lie within their bounds; posterior_sd within its bound of sqrt diag(T0 H^-1 T0^T).  Returns
    (the largest ratio observed / bound, the Truth)."""
    picks = [int(p) for p in design.picks]
    truth = Truth(Z0, T0, E, picks) if truth is None else truth
    M = truth.M
    live = M if live is None else live
    assert len(design.gain) == len(picks) and len(design.information) == len(picks)
    worst = 0.0
    for t, x in enumerate(picks):
        assert x not in picks[:t], f"step {t}: candidate {x} picked twice"
        sc, b = truth.scores[t], truth.score_bound[t]
        assert not np.isnan(sc[x]), f"step {t}: picked the NaN candidate {x}"
        rest = np.where(np.isnan(sc), -np.inf, sc).astype(LD)
        rest[picks[:t]] = -np.inf
        best = int(np.argmax(rest))
        gap, tol = float(rest[best] - sc[x]), float(b[x] + b[best])
        assert gap <= tol, f"step {t}: pick {x} has a true score {gap:.3g} below the maximum (candidate {best}), the bound allows {tol:.3g}"
        err = abs(float(LD(design.gain[t]) - sc[x]))
        assert err <= b[x], f"step {t}: gain {design.gain[t]!r} off the true {float(sc[x])!r} by {err:.3g} > {b[x]:.3g}"
        worst = max(worst, err / b[x], gap / tol if tol > 0 else 0.0)
    if picks and live:
        info, ib = truth.information(live)
        err = np.abs(np.asarray(design.information, dtype=np.float64).astype(LD) - info).astype(np.float64)
        assert (err <= ib).all(), f"information off by {err.max():.3g}, bound {ib[np.argmax(err / ib)]:.3g}"
        worst = max(worst, float((err / ib).max()))
    sd, sb = truth.sd[len(picks)], truth.sd_bound[len(picks)]
    err = np.abs(np.asarray(design.posterior_sd, dtype=np.float64).astype(LD) - sd).astype(np.float64)
    ok = err <= sb
    assert ok.all(), f"posterior_sd off by up to {err.max():.3g} (bound {sb[~ok].min():.3g}) at {np.argwhere(~ok)[:4].tolist()}"
    with np.errstate(invalid="ignore", divide="ignore"):
        worst = max(worst, float(np.nanmax(np.where(sb > 0, err / sb, 0.0))))
    return worst, truth


def criterion(Z0, E, picks, live=None):
    """Phi(S) in nats, long double, for the sensor set ``picks`` (any order): 1 / (2 live) sum_j log det(I + W_S W_S^T), by the QR
    factor of [W_S^T; I]."""
    Z0 = np.asarray(Z0, dtype=np.float64)
    M, n, k = Z0.shape
    W = np.einsum("xn,jnk->jxk", np.asarray(E, dtype=np.float64)[list(picks)].astype(LD), Z0.astype(LD))
    R = _householder_R(np.concatenate([W, np.array(np.broadcast_to(np.eye(k, dtype=LD), (M, k, k)))], axis=1))
    return (2 * np.log(np.abs(np.einsum("mcc->mc", R))).sum()) / (2 * LD(M if live is None else live))
