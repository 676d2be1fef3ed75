"""Parameter estimation from sensor data through a library of reduced states.

``EstimatorInv`` / ``EstimatorLinear`` read the parameters off the state-estimation coefficients: defined only for a basis whose
rows are snapshots, they amplify measurement noise by cond(E) and say nothing about how well the data determine the parameters.
Here the parameters are SEARCHED: ``rom_resid_eval`` solves the Galerkin ROM for M library parameters in one call and leaves
their coordinates COEF (M x n) on the device; for K measurement vectors ``rom_nearest`` finds the library states that explain
them best (the K x M misfits never exist), and a Gauss-Newton / Levenberg-Marquardt polish on the host (n x n systems,
batched over the queries; with polish="device" on the GPU, ``rom_lm_polish``) refines the best library entries.  Any basis.

    lib = ParameterLibrary(sm, basis, a_library).observe(points)
    est = lib.estimate(measurements)           # ParameterEstimate
"""
from typing import NamedTuple, Optional

import numpy as np

from .lib.ReducedBasis import ResidualBound, ResidualEstimator
from .lib.SolutionsManagers import DeviceArray


class PolishResult(NamedTuple):
    """``polish_parameters``: theta (K, k) = log a, misfit (K,) = ||w (y - E^T c(theta))||_2, coefficients (K, n), converged
    and iterations (K,), sigma_min (K,) of the final Jacobian d(w E^T c) / d theta, start (K,) the start that won."""
    theta: np.ndarray
    misfit: np.ndarray
    coefficients: np.ndarray
    converged: np.ndarray
    iterations: np.ndarray
    sigma_min: np.ndarray
    start: np.ndarray


class ParameterEstimate(NamedTuple):
    """``ParameterLibrary.estimate``: a (K, *blocks); misfit (K,) of the estimate; start_index / start_misfit (K, t): the library
    rows the search returned and their misfits, nearest first; converged, iterations (K,) of the polish; sigma_min (K,): the
    smallest singular value of the final Jacobian of the weighted predictions with respect to log a -- how well the data
    determine the parameters; coefficients (K, n) of the reduced state in the A_1-orthonormal basis; error_bound: the
    ``ResidualBound`` of the ROM at the estimate; states: DeviceArray (K, dim) of the reduced states, or None."""
    a: np.ndarray
    misfit: np.ndarray
    start_index: np.ndarray
    start_misfit: np.ndarray
    converged: np.ndarray
    iterations: np.ndarray
    sigma_min: np.ndarray
    coefficients: np.ndarray
    error_bound: ResidualBound
    states: Optional[DeviceArray]


def _rom_state(Ahat, bhat, G, y, theta, jacobian=True):
    """c(theta) (B, n), the weighted residual r = y - G c (B, m) and J = dr/dtheta (B, m, k) for B parameter rows; G = w E^T."""
    ea = np.exp(theta)
    A = np.einsum("bq,qij->bij", ea, Ahat)
    c = np.linalg.solve(A, np.broadcast_to(bhat, (len(theta), len(bhat)))[..., None])[..., 0]
    r = y - c @ G.T
    if not jacobian:
        return c, r, None
    V = np.einsum("qij,bj->biq", Ahat, c) * ea[:, None, :]    # A_q c e^theta_q: columns of -A dc/dtheta
    X = np.linalg.solve(A, V)                                   # -dc/dtheta_q = e^theta_q A^-1 A_q c
    return c, r, np.einsum("mi,biq->bmq", G, X)                 # dr/dtheta = -G dc/dtheta


def polish_parameters(Ahat, bhat, E, Y, theta0, lo, hi, weights=None, max_iter=30, misfit_tol=1e-3):
    """Levenberg-Marquardt in theta = log a for  min ||w (y - E^T c(theta))||_2,  c(theta) = (sum_q e^theta_q Ahat_q)^-1 bhat,
    dc/dtheta_q = -e^theta_q A^-1 Ahat_q c; pure NumPy, batched over the queries.  Ahat (k, n, n), bhat (n,): the reduced
    model (``Resid.download("Ahat" / "bhat")``); E (n, m): the basis at the sensors; Y (K, m); theta0 (K, k) or (K, t, k):
    the starts -- the polish runs from each and keeps the smallest misfit; theta stays in the box [lo, hi] (scalars or (k,)).
    ``converged``: the iteration became stationary (or the misfit reached rounding level) AND the final misfit is at most
    misfit_tol max|w y| -- on exact data a run that stalls in a local minimum ends far above that, under noise choose
    misfit_tol above the noise level.  max_iter = 0 only evaluates the starts."""
    Ahat, bhat, E = np.asarray(Ahat, dtype=np.float64), np.asarray(bhat, dtype=np.float64), np.asarray(E, dtype=np.float64)
    Y = np.atleast_2d(np.asarray(Y, dtype=np.float64))
    K, m = Y.shape
    k, n = Ahat.shape[0], Ahat.shape[1]
    theta0 = np.asarray(theta0, dtype=np.float64).reshape(K, -1, k)
    t = theta0.shape[1]
    w = np.ones(m) if weights is None else np.asarray(weights, dtype=np.float64)
    G = w[:, None] * E.T
    lo, hi = np.broadcast_to(np.asarray(lo, dtype=np.float64), (k,)), np.broadcast_to(np.asarray(hi, dtype=np.float64), (k,))
    y = np.repeat(w[None, :] * Y, t, axis=0)                     # (B, m), B = K t
    B = K * t
    theta = np.clip(theta0.reshape(B, k), lo, hi)
    scale = np.maximum(np.abs(y).max(axis=1), np.finfo(float).tiny)
    c, r, _ = _rom_state(Ahat, bhat, G, y, theta, jacobian=False)
    f = np.einsum("bm,bm->b", r, r)
    lam = np.full(B, 1e-3)
    active = np.ones(B, dtype=bool)
    stationary = np.zeros(B, dtype=bool)
    iterations = np.zeros(B, dtype=np.int64)
    for _ in range(int(max_iter)):
        ia = np.flatnonzero(active)
        if ia.size == 0:
            break
        iterations[ia] += 1
        _, ra, Ja = _rom_state(Ahat, bhat, G, y[ia], theta[ia])
        JtJ = np.einsum("bmq,bmp->bqp", Ja, Ja)
        g = np.einsum("bmq,bm->bq", Ja, ra)
        dJ = np.einsum("bqq->bq", JtJ)
        todo = np.ones(ia.size, dtype=bool)
        for _trial in range(8):
            it = np.flatnonzero(todo)
            if it.size == 0:
                break
            damp = lam[ia[it], None] * (dJ[it] + 1e-300) + 1e-30 * dJ[it].max(axis=1, keepdims=True)
            H = JtJ[it] + damp[:, :, None] * np.eye(k)
            step = -np.linalg.solve(H, g[it][..., None])[..., 0]
            new = np.clip(theta[ia[it]] + step, lo, hi)
            moved = np.abs(new - theta[ia[it]]).max(axis=1)
            cn, rn, _ = _rom_state(Ahat, bhat, G, y[ia[it]], new, jacobian=False)
            fn = np.einsum("bm,bm->b", rn, rn)
            ok = fn < f[ia[it]]
            still = moved <= 1e-13 * (1.0 + np.abs(new).max(axis=1))
            acc = ia[it[ok]]
            theta[acc], c[acc], r[acc], f[acc] = new[ok], cn[ok], rn[ok], fn[ok]
            lam[acc] = np.maximum(lam[acc] / 3.0, 1e-12)
            lam[ia[it[~ok]]] *= 4.0
            # a step that no longer moves theta (accepted: below 1e-10 relative), or a misfit at rounding level: stationary
            tiny = ok & (moved <= 1e-10 * (1.0 + np.abs(new).max(axis=1)))
            done = still | tiny | (np.sqrt(f[ia[it]]) <= 1e-14 * scale[ia[it]])
            stationary[ia[it[done]]] = True
            active[ia[it[done]]] = False
            todo[it[ok | done]] = False
        stuck = ia[np.flatnonzero(todo)]     # eight increases of the damping without a decrease: a minimum to working accuracy
        stationary[stuck] = True
        active[stuck] = False
    c, r, J = _rom_state(Ahat, bhat, G, y, theta)
    misfit = np.sqrt(np.einsum("bm,bm->b", r, r))
    sig = np.linalg.svd(J, compute_uv=False)[:, -1] if min(m, k) else np.zeros(B)
    best = np.argmin(misfit.reshape(K, t), axis=1)
    pick = np.arange(K) * t + best
    conv = (stationary | (misfit <= 1e-14 * scale)) & (misfit <= misfit_tol * scale)
    return PolishResult(theta[pick], misfit[pick], c[pick], conv[pick], iterations[pick], sig[pick], best)


LM_LIMITS = dict(n=64, k=16, r=64, t=8)   # rom_lm_polish (csrc/rom_lm.hip)


def _check_lm_limits(n, k, r, t):
    for name, v in (("n", n), ("k", k), ("r", r), ("t", t)):
        if not 1 <= v <= LM_LIMITS[name]:
            raise ValueError(f"the device polish (rom_lm_polish) needs 1 <= {name} <= {LM_LIMITS[name]}, got {name} = {v}: "
                             "use polish=True (the host polish)")


def reduce_sensors(E, weights=None, rel=1e-12):
    """The compact SVD diag(w) E^T = U S V^T truncated at sigma > rel sigma_1: (U (m, r), G_r = S V^T (r, n), V S (n, r))."""
    E = np.asarray(E, dtype=np.float64)
    w = np.ones(E.shape[1]) if weights is None else np.asarray(weights, dtype=np.float64)
    U, S, Vt = np.linalg.svd(w[:, None] * E.T, full_matrices=False)
    r = max(1, int(np.sum(S > rel * S[0])))
    return np.ascontiguousarray(U[:, :r]), np.ascontiguousarray(S[:r, None] * Vt[:r]), np.ascontiguousarray(Vt[:r].T * S[:r])


def reduce_measurements(U, Y, weights):
    """p = U^T (w y) (K, r) and aux (K, 2) = (perp2 = |(I - U U^T)(w y)|^2, scale = max|w y|) of the rows of Y."""
    Yw = Y * weights[None, :]
    Pq = np.ascontiguousarray(Yw @ U)
    perp = Yw - Pq @ U.T
    scale = np.maximum(np.abs(Yw).max(axis=1), np.finfo(float).tiny) if Yw.shape[1] else np.full(len(Yw), np.finfo(float).tiny)
    return Pq, np.ascontiguousarray(np.stack([np.einsum("km,km->k", perp, perp), scale], axis=1))


def polish_parameters_device(ctx, Ahat, bhat, E, Y, theta0, lo, hi, weights=None, max_iter=30, misfit_tol=1e-3) -> PolishResult:
    """``polish_parameters`` on the device of ``ctx`` (``rom_lm_polish``, one workgroup per (query, start)): the same arguments
    and the same result.  The sensors are reduced on the host first -- diag(w) E^T = U S V^T, p = U^T (w y), G_r = S V^T -- so
    the kernel works on r <= min(n, m) rows; the part of w y outside the range of U enters the misfit as a constant."""
    Ahat, bhat, E = np.asarray(Ahat, dtype=np.float64), np.asarray(bhat, dtype=np.float64), np.asarray(E, dtype=np.float64)
    Y = np.atleast_2d(np.asarray(Y, dtype=np.float64))
    K, m = Y.shape
    k, n = Ahat.shape[0], Ahat.shape[1]
    theta0 = np.asarray(theta0, dtype=np.float64).reshape(K, -1, k)
    t = theta0.shape[1]
    w = np.ones(m) if weights is None else np.asarray(weights, dtype=np.float64)
    U, Gr, _ = reduce_sensors(E, w)
    r = U.shape[1]
    _check_lm_limits(n, k, r, t)
    Pq, aux = reduce_measurements(U, Y, w)
    res, _ = ctx.lm_polish(n, k, r, ctx.upload(Ahat), ctx.upload(bhat), ctx.upload(Gr), ctx.upload(Pq) if K else None, 0, r, K, t,
                           ctx.upload(theta0) if K else None, lo, hi, AUX=ctx.upload(aux) if K else None, max_iter=max_iter,
                           misfit_tol=misfit_tol)
    return res


class ParameterLibrary:
    """The Galerkin ROM on ``basis`` solved for the M parameters ``a_library`` (one ``rom_resid_eval`` call over all of them):
    their coordinates COEF (M, n) in the A_1-orthonormal basis stay on the device, ``.a`` (M, k), ``.residual`` and ``.upper``
    (the certified bound ||r|| / a_min of the ROM error of every entry) on the host.  ``observe`` fixes the sensors,
    ``estimate`` answers measurement vectors."""

    def __init__(self, sm, basis, a_library, n=None):
        self.sm = sm
        self.estimator = ResidualEstimator(sm, basis)
        self.n = self.estimator.n if n is None else min(int(n), self.estimator.n)
        ctx = sm._ctx
        self.a = sm._a_batch(a_library)
        self.M = M = self.a.shape[0]
        if M < 1 or self.n < 1:
            raise ValueError("ParameterLibrary needs at least one library parameter and one basis row")
        D = ctx.alloc(M)
        self.COEF = ctx.alloc(M * self.n)
        self.estimator.handle.eval(ctx.upload(self.a), M, self.n, D, COEF=self.COEF)
        self.residual = D.download(M)
        self.upper = self.residual / self.a.min(axis=1)
        self.Ahat = self.estimator.handle.download("Ahat")[:, :self.n, :self.n].copy()
        self.bhat = self.estimator.handle.download("bhat")[:self.n].copy()
        self._W = ctx.alloc(self.estimator.n * sm.vspace_dim)
        self.estimator.handle.basis(self._W)
        self.points = None

    def observe(self, points, weights=None):
        """Fix the sensors: E = l(W) (n, m); compact SVD diag(w) E^T = U S V^T truncated at sigma > 1e-12 sigma_1 (rank r);
        the library coordinates COEF (V S) (M, r) are formed on the device.  The weighted misfit of library entry j is then
        ||U^T (w y) - q_j||^2 + ||(I - U U^T) (w y)||^2."""
        sm, ctx = self.sm, self.sm._ctx
        self.points = np.asarray(points, dtype=np.float64).reshape(-1, 2)
        m = len(self.points)
        self.weights = np.ones(m) if weights is None else np.asarray(weights, dtype=np.float64).reshape(m)
        self.E = sm._fem.evaluate_points(self._W, self.n, *sm._locate(self.points))
        U, S, Vt = np.linalg.svd(self.weights[:, None] * self.E.T, full_matrices=False)
        self.r = r = max(1, int(np.sum(S > 1e-12 * S[0])))
        self.U = np.ascontiguousarray(U[:, :r])
        VS = np.ascontiguousarray(Vt[:r].T * S[:r])
        self.Qc = ctx.alloc(self.M * r)
        ctx.gemm_nn(self.M, r, self.n, self.COEF, 0, self.n, ctx.upload(VS), 0, r, self.Qc, 0, r)
        self.Gr = ctx.upload(np.ascontiguousarray(S[:r, None] * Vt[:r]))    # G_r = S V^T (r, n): the device polish
        return self

    def _search(self, measurements, t, mode):
        """``search`` and what it uploaded: (idx, misfit, info, the device buffer of Pq = U^T (w y) (K, r) or None, Yw, perp2)."""
        if self.points is None:
            raise RuntimeError("ParameterLibrary.observe(points) comes first")
        Y = np.atleast_2d(np.asarray(measurements, dtype=np.float64))
        Yw = Y * self.weights[None, :]
        Pq = np.ascontiguousarray(Yw @ self.U)
        perp = Yw - Pq @ self.U.T
        t = min(int(t), self.M)
        ctx = self.sm._ctx
        Pq_dev = ctx.upload(Pq) if len(Y) else None
        idx, d2, info = ctx.nearest(self.Qc, 0, self.r, self.M, Pq_dev, 0, self.r, len(Y), self.r, t=t, mode=mode)
        perp2 = np.einsum("km,km->k", perp, perp)
        return idx, np.sqrt(d2 + perp2[:, None]), info, Pq_dev, Yw, perp2

    def search(self, measurements, t=4, mode=0):
        """The t library rows of smallest misfit per measurement vector: (idx (K, t), misfit (K, t), info of rom_nearest)."""
        return self._search(measurements, t, mode)[:3]

    def _estimate_device(self, Y, idx, Pq_dev, Yw, perp2, la, states, max_iter, misfit_tol):
        """The device polish from the library rows idx (K, t): (PolishResult, DeviceArray of the lifted states or None).  The
        queries Pq are the buffer the search uploaded; the coefficients are lifted from the result rows on the device."""
        sm, ctx = self.sm, self.sm._ctx
        K, t, k, n = len(Y), idx.shape[1], self.a.shape[1], self.n
        _check_lm_limits(n, k, self.r, t)
        if getattr(self, "_lm_model", None) is None:
            self._lm_model = (ctx.upload(self.Ahat), ctx.upload(self.bhat))
        ldo = k + n + 5
        OUT = ctx.alloc(max(K * ldo, 1))
        scale = np.maximum(np.abs(Yw).max(axis=1), np.finfo(float).tiny) if K else np.zeros(0)
        res, _ = ctx.lm_polish(n, k, self.r, self._lm_model[0], self._lm_model[1], self.Gr, Pq_dev, 0, self.r, K, t,
                               ctx.upload(la[idx]) if K else None, la.min(axis=0), la.max(axis=0),
                               AUX=ctx.upload(np.stack([perp2, scale], axis=1)) if K else None, max_iter=max_iter,
                               misfit_tol=misfit_tol, OUT=OUT, ldo=ldo)
        S = None
        if states:
            dim = sm.vspace_dim
            out = ctx.alloc(max(K * dim, 1))
            if K:
                ctx.gemm_nn(K, dim, n, OUT, k, ldo, self._W, 0, dim, out, 0, dim)
            S = DeviceArray(out, K, dim)
        return res, S

    def estimate(self, measurements, t=4, polish=True, states=False, max_iter=30, misfit_tol=1e-3) -> ParameterEstimate:
        """Parameters for the K measurement vectors (K, m): the search, then (``polish``) Levenberg-Marquardt in log a from
        each of the t library entries found, inside the library's box; without the polish the nearest library entry.
        ``polish="device"`` runs the polish on the GPU (``rom_lm_polish``; ValueError outside its limits n <= 64, k <= 16,
        r <= 64, t <= 8), ``polish=True`` on the host."""
        sm, ctx = self.sm, self.sm._ctx
        Y = np.atleast_2d(np.asarray(measurements, dtype=np.float64))
        K = len(Y)
        if isinstance(polish, str) and polish != "device":
            raise ValueError(f'polish = {polish!r}: True (host), False or "device"')
        if isinstance(polish, str):
            if self.points is None:
                raise RuntimeError("ParameterLibrary.observe(points) comes first")
            _check_lm_limits(self.n, self.a.shape[1], self.r, min(int(t), self.M))
        idx, start_misfit, _, Pq_dev, Yw, perp2 = self._search(Y, t, 0)
        la = np.log(self.a)
        if isinstance(polish, str):
            res, S = self._estimate_device(Y, idx, Pq_dev, Yw, perp2, la, states, max_iter, misfit_tol)
            a = np.exp(res.theta)
            return ParameterEstimate(a.reshape((K,) + tuple(sm.blocks_geometry)), res.misfit, idx, start_misfit, res.converged,
                                     res.iterations, res.sigma_min, res.coefficients, self.estimator.bound(a, n=self.n), S)
        starts = la[idx] if polish else la[idx[:, :1]]
        res = polish_parameters(self.Ahat, self.bhat, self.E, Y, starts, la.min(axis=0), la.max(axis=0), weights=self.weights,
                                max_iter=max_iter if polish else 0, misfit_tol=misfit_tol)
        a = np.exp(res.theta) if polish else self.a[idx[:, 0]]
        bound = self.estimator.bound(a, n=self.n)
        S = None
        if states:
            dim = sm.vspace_dim
            out = ctx.alloc(max(K * dim, 1))
            if K:
                ctx.gemm_nn(K, dim, self.n, ctx.upload(np.ascontiguousarray(res.coefficients)), 0, self.n, self._W, 0, dim, out, 0, dim)
            S = DeviceArray(out, K, dim)
        return ParameterEstimate(a.reshape((K,) + tuple(sm.blocks_geometry)), res.misfit, idx, start_misfit, res.converged,
                                 res.iterations, res.sigma_min, res.coefficients, bound, S)


# ---- box-constrained least squares (Stark-Parker BVLS): the noise-robust linear state estimate ----------------------------------
class BvlsResult(NamedTuple):
    """``bvls_host`` / ``Context.bvls`` / ``bounded_lstsq``: c (K, n) inside the box; misfit (K,) = sqrt(||p - G c||^2 + perp2);
    bound (K, n): -1 at lo, +1 at hi, 0 free (a pinned coordinate, lo_j == hi_j, reads -1); converged (K,): the Karush-Kuhn-Tucker
    conditions were reached; iterations (K,): the passes made."""
    c: np.ndarray
    misfit: np.ndarray
    bound: np.ndarray
    converged: np.ndarray
    iterations: np.ndarray


BVLS_LIMITS = dict(n=64, r=96)   # rom_bvls (csrc/rom_bvls.hip): 1 <= n <= 64, n <= r <= 96


def _check_bvls_limits(n, r):
    if not (1 <= n <= BVLS_LIMITS["n"] and n <= r <= BVLS_LIMITS["r"]):
        raise ValueError(f"the device solve (rom_bvls) needs 1 <= n <= {BVLS_LIMITS['n']} and n <= r <= {BVLS_LIMITS['r']}, got "
                         f"n = {n}, r = {r}: use device=False (bvls_host)")


def _bvls_box(lo, hi, n):
    lo = np.array(np.broadcast_to(np.asarray(lo, dtype=np.float64), (n,)))
    hi = np.array(np.broadcast_to(np.asarray(hi, dtype=np.float64), (n,)))
    if np.isnan(lo).any() or np.isnan(hi).any() or (lo > hi).any() or np.isposinf(lo).any() or np.isneginf(hi).any():
        raise ValueError("bvls: the box needs lo <= hi without NaN (lo may be -inf, hi +inf)")
    return lo, hi


def _bvls_solve(G, gram, free, rhs):
    """z (B, n): the least squares of the rows of rhs (B, r) on the free columns of G (zero elsewhere): a Cholesky of the free
    block of gram = G^T G, then one refinement step with the residual formed on the columns of G themselves."""
    both = free[:, :, None] & free[:, None, :]
    H = np.where(both, gram[None, :, :], 0.0) + (~free)[:, :, None] * np.eye(gram.shape[0])
    L = np.linalg.cholesky(H)
    Lt = np.ascontiguousarray(L.transpose(0, 2, 1))

    def solve(b):
        return np.linalg.solve(Lt, np.linalg.solve(L, b[..., None]))[..., 0]

    z = solve(np.where(free, rhs @ G, 0.0))
    return z + solve(np.where(free, (rhs - z @ G.T) @ G, 0.0))


def bvls_host(G, P, lo, hi, aux=None, max_iter=None) -> BvlsResult:
    """For each row p of P (K, r):  min over lo <= c <= hi of ||p - G c||^2  with G (r, n) of full column rank shared by all rows
    -- Stark-Parker bounded-variable least squares, every decision fixed (``rom_bvls`` is its port); pure NumPy, batched over
    the rows.

    Start: the unconstrained solution clipped to the box; what lands on a bound starts bound, the rest free.  A PASS solves the
    least squares on the free columns with the bound ones moved to the right-hand side (``_bvls_solve``).  Feasible: it is
    taken, g = G^T (G c - p), and the bound variable whose multiplier has the wrong sign (g_j < 0 at lo, g_j > 0 at hi) with the
    largest |g_j| / ||G_j|| is freed, the lowest index among equals; none: the Karush-Kuhn-Tucker conditions hold, ``converged``.
    Infeasible: c moves along the segment to the solution up to the first bound hit, and the variables that hit it are bound.
    A variable freed in one pass that leaves through the same bound in the next is bound again and BARRED from being freed
    until some other variable changes state (a variable that stays free after being freed, or another one bound).  At most
    max_iter passes (default 5 n + 10; 0 returns the clipped start).  lo_j == hi_j PINS c_j bit for bit (never freed, bound -1);
    -inf / +inf bounds are never active.  aux (K, 2) = (perp2, scale) as in ``sense_scores``: misfit = sqrt(||p - G c||^2 + perp2).
    ValueError: lo_j > hi_j or NaN in the box, NaN / Inf in G or P, or G without full column rank."""
    G = np.asarray(G, dtype=np.float64)
    r, n = G.shape
    P = np.asarray(P, dtype=np.float64).reshape(-1, r)
    K = len(P)
    lo, hi = _bvls_box(lo, hi, n)
    max_iter = 5 * n + 10 if max_iter is None else int(max_iter)
    if not (np.isfinite(G).all() and np.isfinite(P).all()):
        raise ValueError("bvls: NaN / Inf in G or P")
    gram = G.T @ G
    gn = np.sqrt(np.diag(gram))
    try:
        if r < n or not (gn > 0).all():
            raise np.linalg.LinAlgError
        np.linalg.cholesky(gram)
    except np.linalg.LinAlgError:
        raise ValueError(f"bvls: G ({r} x {n}) has no full column rank") from None
    perp2 = np.zeros(K) if aux is None else np.asarray(aux, dtype=np.float64).reshape(K, 2)[:, 0]
    pinned = lo == hi
    rows = np.arange
    with np.errstate(invalid="ignore", divide="ignore"):
        start = _bvls_solve(G, gram, np.ones((K, n), dtype=bool), P)
        c = np.minimum(np.maximum(start, lo), hi)
        st = np.where(pinned | (start <= lo), -1, np.where(start >= hi, 1, 0))
        barred = np.zeros((K, n), dtype=bool)
        freed, side = np.full(K, -1), np.zeros(K, dtype=np.int64)
        active, conv, passes = np.full(K, max_iter > 0), np.zeros(K, dtype=bool), np.zeros(K, dtype=np.int64)
        for _ in range(max_iter):
            ia = np.flatnonzero(active)
            if ia.size == 0:
                break
            passes[ia] += 1
            F = st[ia] == 0
            z = np.where(F, _bvls_solve(G, gram, F, P[ia] - np.where(F, 0.0, c[ia]) @ G.T), c[ia])
            below, above = F & (z < lo), F & (z > hi)
            infeasible = (below | above).any(axis=1)
            f = np.flatnonzero(~infeasible)
            if f.size:   # the solution is taken; free the worst multiplier, or stop
                i, zf = ia[f], z[f]
                s = np.where(F[f] & (zf == lo), -1, np.where(F[f] & (zf == hi), 1, st[i]))   # (exactly on a bound: bound)
                c[i] = zf
                g = -((P[i] - zf @ G.T) @ G)
                barred[i[freed[i] >= 0]] = False   # the variable freed in the last pass has stayed free
                viol = np.where(s < 0, -g, g) / gn
                cand = (s != 0) & ~pinned & ~barred[i] & (viol > 0)
                viol = np.where(cand, viol, 0.0)
                j = np.argmax(viol, axis=1)        # (the lowest index among equals)
                go = cand.any(axis=1)
                conv[i[~go]] = True
                active[i[~go]] = False
                freed[i] = np.where(go, j, -1)
                side[i[go]] = s[go, j[go]]
                s[go, j[go]] = 0
                st[i] = s
            f = np.flatnonzero(infeasible)
            if f.size:   # to the first bound on the segment; what hits it is bound
                i, zf, cf, Ff = ia[f], z[f], c[ia[f]], F[f]
                ratio = np.where(below[f], (cf - lo) / (cf - zf), np.where(above[f], (hi - cf) / (zf - cf), np.inf))
                alpha = ratio.min(axis=1, keepdims=True)
                cn = np.minimum(np.maximum(cf + alpha * (zf - cf), lo), hi)
                cn = np.where(ratio == alpha, np.where(below[f], lo, hi), cn)
                cn = np.where(Ff, cn, cf)
                s = np.where(Ff & (cn == lo), -1, np.where(Ff & (cn == hi), 1, st[i]))
                changed = s != st[i]
                fr = np.maximum(freed[i], 0)
                same = (freed[i] >= 0) & changed[rows(len(i)), fr] & (s[rows(len(i)), fr] == side[i])
                others = changed.sum(axis=1) > same
                barred[i[others]] = False
                barred[i[same], fr[same]] = True
                freed[i] = -1
                c[i], st[i] = cn, s
        res = P - c @ G.T
    misfit = np.sqrt(np.einsum("kr,kr->k", res, res) + perp2)
    return BvlsResult(c, misfit, st.astype(np.int64), conv, passes)


def coefficient_box(C, inflate=0.1):
    """(lo, hi) (n each): min / max over the rows of a training coefficient matrix C (M, n), widened on both sides by
    ``inflate`` times the range."""
    C = np.asarray(C, dtype=np.float64)
    C = C.reshape(-1, C.shape[-1])
    lo, hi = C.min(axis=0), C.max(axis=0)
    pad = float(inflate) * (hi - lo)
    return lo - pad, hi + pad


def bounded_lstsq(ctx, E, Y, lo, hi, weights=None, device=True) -> BvlsResult:
    """min over lo <= c <= hi of ||w (y - E^T c)||_2 for the K rows y of Y (K, m): E (n, m) the basis at the sensors, as in
    ``polish_parameters``.  The sensors are reduced first -- diag(w) E^T = U S V^T, p = U^T (w y), G_r = S V^T (``reduce_sensors``
    / ``reduce_measurements``) -- so the solve works on r = n rows and the part of w y outside the range of U enters the misfit
    as a constant; ValueError when the rank is below n.  ``device``: ``rom_bvls`` on ``ctx`` (ValueError outside
    ``BVLS_LIMITS``), else ``bvls_host`` (``ctx`` may be None).  c is in the coordinates of E's rows."""
    E = np.asarray(E, dtype=np.float64)
    n, m = E.shape
    Y = np.asarray(Y, dtype=np.float64).reshape(-1, m)
    K = len(Y)
    lo, hi = _bvls_box(lo, hi, n)
    w = np.ones(m) if weights is None else np.asarray(weights, dtype=np.float64).reshape(m)
    U, Gr, _ = reduce_sensors(E, w)
    r = U.shape[1]
    if r < n:
        raise ValueError(f"bounded_lstsq: the {m} weighted sensors determine {r} of the {n} coefficients (rank of diag(w) E^T below n)")
    Pq, aux = reduce_measurements(U, Y, w)
    if not device:
        return bvls_host(Gr, Pq, lo, hi, aux=aux)
    _check_bvls_limits(n, r)
    res, _ = ctx.bvls(n, r, ctx.upload(Gr), ctx.upload(Pq) if K else None, 0, r, K, lo, hi, AUX=ctx.upload(aux) if K else None)
    return res
