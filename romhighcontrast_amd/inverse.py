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

    def posterior(self, measurements, sigma, t=4, steps=2000, burn=500, thin=0, seed=0, states=False, device=True) -> "ParameterPosterior":
        """Which parameters are compatible with the K measurement vectors (K, m) under independent noise of standard deviation
        ``sigma`` (a scalar or (K,), in the units of the weighted measurements): t chains per vector of adaptive random-walk
        Metropolis in log a inside the library's box (``rom_mcmc``; ``mcmc_host`` is its specification and what ``device=False``
        runs).  The chains start at the t library rows of the search, which are dispersed and so suit R-hat; the proposal factors
        are ``proposal_factors`` at the device-polished estimate.  ``thin`` = 0 keeps no samples, else every thin-th state past
        burn-in; ``states``: the posterior-mean states.  Returns a ``ParameterPosterior``; its a_map is (K, k)."""
        sm, ctx = self.sm, self.sm._ctx
        Y = np.atleast_2d(np.asarray(measurements, dtype=np.float64))
        K, k, n = len(Y), self.a.shape[1], self.n
        if self.points is None:
            raise RuntimeError("ParameterLibrary.observe(points) comes first")
        t = min(int(t), self.M)
        _check_mcmc_limits(n, k, self.r, t)
        steps, burn, thin = int(steps), int(burn), int(thin)
        if thin < 0:
            raise ValueError(f"thin = {thin}: 0 (no samples) or the stride of the kept samples")
        idx, _, _, Pq_dev, Yw, perp2 = self._search(Y, t, 0)
        la = np.log(self.a)
        lo, hi = la.min(axis=0), la.max(axis=0)
        res, _ = self._estimate_device(Y, idx, Pq_dev, Yw, perp2, la, False, 30, 1e-3)
        invvar = 1.0 / np.broadcast_to(np.asarray(sigma, dtype=np.float64), (K,)) ** 2
        Gr = self.Gr.download(self.r * n).reshape(self.r, n)
        L = proposal_factors(self.Ahat, self.bhat, Gr, res.theta, invvar, lo, hi) if K else np.zeros((0, k, k))
        slots = max(0, steps - burn) // thin if thin else 0
        o = mcmc_layout(n, k)
        if not device:
            run = mcmc_host(self.Ahat, self.bhat, Gr, Yw @ self.U, invvar, la[idx], L, lo, hi, seed, steps, burn, max(thin, 1), slots=slots)
            rows, samples = run.state, run.samples
        else:
            rows = np.zeros((K * t, o["row"]))
            rows[:, :k] = la[idx].reshape(K * t, k)
            samples = None
            if K:
                STATE = ctx.upload(rows)
                SAMPLES = ctx.upload(np.full(K * t * slots * k, np.nan)) if slots else None
                ctx.mcmc(n, k, self.r, self._lm_model[0], self._lm_model[1], self.Gr, Pq_dev, 0, self.r, K, t, ctx.upload(invvar),
                         ctx.upload(L), lo, hi, seed, steps, burn, max(thin, 1), STATE, SAMPLES=SAMPLES, slots=slots)
                rows = STATE.download().reshape(K * t, o["row"])
                samples = SAMPLES.download().reshape(K * t, slots, k) if slots else None
        post = posterior_summary(rows, n, k, t, samples=samples if slots else None, perp2=perp2)
        if states:
            dim = sm.vspace_dim
            out = ctx.alloc(max(K * dim, 1))
            if K:
                ctx.gemm_nn(K, dim, n, ctx.upload(np.ascontiguousarray(post.mean_coefficients)), 0, n, self._W, 0, dim, out, 0, dim)
            post = post._replace(states=DeviceArray(out, K, dim))
        return post

    def select_sensors(self, candidates, m, sigma, prior_cov=None, weights=None, subset=None, rel_tol=0.0, device=True) -> "SensorDesign":
        """Up to m of the ``candidates`` (ncand, 2) as sensors for PARAMETER estimation: the greedy Bayesian D-optimal design
        (``sensor_dopt_host``; on the GPU ``rom_sensor_dopt`` unless ``device=False``) averaged over the library's parameters, or
        over its rows ``subset``.  sigma: the noise level of a weighted measurement, as in ``posterior``; ``weights`` (ncand,)
        scales the candidates' rows -- the ``weights`` of ``observe`` -- default 1.  prior_cov None: per parameter the variance of a
        uniform law on the library's box of log a (a parameter with a zero-width box counts as known); else (k,) variances or a
        (k, k) covariance.  The result's ``.points`` is ready for ``.observe(points)``."""
        sm = self.sm
        P = np.asarray(candidates, dtype=np.float64).reshape(-1, 2)
        Ec = np.ascontiguousarray(sm._fem.evaluate_points(self._W, self.n, *sm._locate(P)).T)    # (ncand, n)
        if weights is not None:
            Ec = Ec * np.asarray(weights, dtype=np.float64).reshape(len(P), 1)
        la = np.log(self.a)
        if prior_cov is None:
            prior_cov = (la.max(axis=0) - la.min(axis=0)) ** 2 / 12.0
        theta = la if subset is None else la[np.asarray(subset, dtype=np.int64).ravel()]
        if device:
            des = sensor_dopt_device(sm._ctx, self.Ahat, self.bhat, theta, Ec, m, sigma, prior_cov, rel_tol=rel_tol)
        else:
            des = sensor_dopt_host(self.Ahat, self.bhat, theta, Ec, m, sigma, prior_cov, rel_tol=rel_tol)
        return des._replace(points=P[des.picks])


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


# ---- model selection among local reduced spaces (Cohen, Dahmen, Mula, Nichols 2022) --------------------------------------------
LS_BAD_STATE, LS_BAD_PARAM, LS_OPEN_STATE, LS_OPEN_PARAM = 1, 2, 4, 8   # the bits of a system's status


class LocalSelectResult(NamedTuple):
    """``local_select_host`` / ``Context.local_select``.  labels (K,) int32: the cluster of smallest (S, index) among the systems
    of status 0, -1 when there is none; coefficients (K, n), a (K, k), surrogate (K,), misfit (K,): those of the chosen cluster
    (NaN where the label is -1); c_all (K, kc, n), a_all (K, kc, k), surrogate_all, misfit_all (K, kc): every system;
    passes (K, kc, 2): of the state and of the parameter solve; status (K, kc): 0, or the sum of 1 (the state solve failed on its
    data: NaN / Inf, or G_j without full column rank), 2 (the parameter solve did), 4 (the state solve stopped at max_iter),
    8 (the parameter solve did)."""
    labels: np.ndarray
    coefficients: np.ndarray
    a: np.ndarray
    surrogate: np.ndarray
    misfit: np.ndarray
    c_all: np.ndarray
    a_all: np.ndarray
    surrogate_all: np.ndarray
    misfit_all: np.ndarray
    passes: np.ndarray
    status: np.ndarray


def _local_select_result(rows, labels, n, k) -> LocalSelectResult:
    """From the (K, kc, n + k + 5) rows c | a | S | misfit | passes, passes | status and the labels."""
    K = rows.shape[0]
    labels = np.asarray(labels, dtype=np.int32)
    pick = rows[np.arange(K), np.maximum(labels, 0)] if K else np.zeros((0, n + k + 5))
    pick = np.where((labels >= 0)[:, None], pick, np.nan)
    return LocalSelectResult(labels, pick[:, :n].copy(), pick[:, n:n + k].copy(), pick[:, n + k].copy(), pick[:, n + k + 1].copy(),
                             rows[:, :, :n].copy(), rows[:, :, n:n + k].copy(), rows[:, :, n + k].copy(), rows[:, :, n + k + 1].copy(),
                             rows[:, :, n + k + 2:n + k + 4].astype(np.int64), rows[:, :, n + k + 4].astype(np.int64))


def local_select_labels(surrogate_all, status):
    """Step 4: per row the index of the smallest (S, index) among the entries of status 0 whose S is a number; -1 when there is
    none."""
    S = np.asarray(surrogate_all, dtype=np.float64)
    ok = (np.asarray(status) == 0) & ~np.isnan(S)
    S = np.where(ok, S, np.inf)
    labels = np.argmin(S, axis=1).astype(np.int32) if S.shape[1] else np.zeros(len(S), dtype=np.int32)   # (the first minimum)
    return np.where(ok.any(axis=1), labels, -1).astype(np.int32)


def local_select_matrix(R, c, k):
    """B (rank, k) = sum_i c_i R[:, 1 + i k : 1 + (i + 1) k], the terms in ascending i: ||R z(a, c)|| = ||R[:, 0] - B a||."""
    R, c = np.asarray(R, dtype=np.float64), np.asarray(c, dtype=np.float64)
    B = np.zeros((R.shape[0], k))
    for i in range(len(c)):
        B = c[i] * R[:, 1 + i * k:1 + (i + 1) * k] + B
    return B


def local_select_host(RT, GR, P, c_lo, c_hi, a_lo, a_hi, max_iter=None) -> LocalSelectResult:
    """The NumPy specification of ``rom_local_select``: state estimation from sensors with kc local reduced spaces, the space
    chosen by the PDE residual (Cohen, Dahmen, Mula, Nichols, SIAM/ASA JUQ 10, 2022).  RT (kc, rank, 1 + k n): the residual
    tables R_j of A_1-orthonormal bases W_j (``rom_resid_download`` what = 0; zero rows added to a common rank change nothing);
    GR (kc, r, n): the reduced sensor matrices G_j; P (K, kc r): per measurement vector the kc reduced measurements p_ij; the
    boxes (kc, n) for c and (kc, k) for a, with the rules of ``bvls_host``.  Per system (i, j), two ``bvls_host`` calls:

      1. c_ij = argmin over c_lo[j] <= c <= c_hi[j] of ||p_ij - G_j c||, misfit_ij its residual norm;
      2. B_ij = ``local_select_matrix(R_j, c_ij, k)``: the residual of the state c_ij W_j is rho_j - B_ij a, affine in a;
      3. S_ij = min over a_lo[j] <= a <= a_hi[j] of ||rho_j - B_ij a||, a_ij its minimiser;

    then label_i = the j of smallest (S_ij, j) among the systems of status 0 (``local_select_labels``).  A solve that
    ``bvls_host`` refuses (NaN / Inf, no full column rank) sets the system's status instead of raising: after a refused state
    solve c, a, S and the misfit are NaN, after a refused parameter solve a and S.  max_iter bounds the passes of either solve;
    None: 5 n + 10 and 5 k + 10.  ValueError: a bad box."""
    RT, GR = np.asarray(RT, dtype=np.float64), np.asarray(GR, dtype=np.float64)
    kc, r, n = GR.shape
    rank = RT.shape[1]
    k = (RT.shape[2] - 1) // n
    assert RT.shape == (kc, rank, 1 + k * n), f"local_select_host: RT {RT.shape} against kc = {kc}, n = {n}"
    P = np.asarray(P, dtype=np.float64).reshape(-1, kc, r)
    K = len(P)
    box = [np.array(np.broadcast_to(np.asarray(b, dtype=np.float64), (kc, d))) for b, d in ((c_lo, n), (c_hi, n), (a_lo, k), (a_hi, k))]
    for j in range(kc):
        _bvls_box(box[0][j], box[1][j], n)
        _bvls_box(box[2][j], box[3][j], k)
    rows = np.full((K, kc, n + k + 5), np.nan)
    rows[:, :, n + k + 2:] = 0.0
    for i in range(K):
        for j in range(kc):
            row = rows[i, j]
            try:
                one = bvls_host(GR[j], P[i, j][None, :], box[0][j], box[1][j], max_iter=max_iter)
            except ValueError:
                row[n + k + 4] = LS_BAD_STATE
                continue
            status = 0 if one.converged[0] else LS_OPEN_STATE
            row[:n], row[n + k + 1], row[n + k + 2] = one.c[0], one.misfit[0], one.iterations[0]
            B = local_select_matrix(RT[j], one.c[0], k)
            try:
                two = bvls_host(B, RT[j][:, 0][None, :], box[2][j], box[3][j], max_iter=max_iter)
                status |= 0 if two.converged[0] else LS_OPEN_PARAM
                row[n:n + k], row[n + k], row[n + k + 3] = two.c[0], two.misfit[0], two.iterations[0]
            except ValueError:
                status |= LS_BAD_PARAM
            row[n + k + 4] = status
    labels = local_select_labels(rows[:, :, n + k], rows[:, :, n + k + 4])
    return _local_select_result(rows, labels, n, k)


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


# ---- posterior sampling of the parameters: which log a are compatible with noisy data ---------------------------------------------
_PHILOX_M0, _PHILOX_M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_PHILOX_W0, _PHILOX_W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
_U32, _S32 = np.uint64(0xFFFFFFFF), np.uint64(32)
MCMC_ACCEPT = 0xFFFFFFFF          # the purpose word of the acceptance uniform
MCMC_TARGET = 0.234               # the acceptance rate the scale adapts to


def philox4x32(counter, key):
    """Philox4x32-10: counter (..., 4) and key (..., 2) of 32-bit words (broadcast against each other) -> (..., 4) uint32.
    ``csrc/rom_philox.h`` is the same function for the host and the device."""
    counter, key = np.asarray(counter, dtype=np.uint64), np.asarray(key, dtype=np.uint64)
    c0, c1, c2, c3 = (counter[..., i] for i in range(4))
    k0, k1 = key[..., 0], key[..., 1]
    for _ in range(10):
        p0, p1 = _PHILOX_M0 * c0, _PHILOX_M1 * c2
        c0, c1, c2, c3 = (p1 >> _S32) ^ c1 ^ k0, p1 & _U32, (p0 >> _S32) ^ c3 ^ k1, p0 & _U32
        k0, k1 = (k0 + _PHILOX_W0) & _U32, (k1 + _PHILOX_W1) & _U32
    return np.stack(np.broadcast_arrays(c0, c1, c2, c3), axis=-1).astype(np.uint32)


def mcmc_uniform(hi, lo):
    """u = ((hi >> 6) 2^26 + (lo >> 6) + 0.5) 2^-52 from two 32-bit words: 52 random bits and a half, exact in float64, never 0
    and never 1 (with 53 bits the half would not fit the significand and all-ones words would round to 1)."""
    hi, lo = np.asarray(hi, dtype=np.uint64), np.asarray(lo, dtype=np.uint64)
    bits = ((hi >> np.uint64(6)) << np.uint64(26)) | (lo >> np.uint64(6))
    return (bits.astype(np.float64) + 0.5) * 2.0 ** -52


def mcmc_draws(seed, chain, step, k, dtype=np.float64):
    """The draws of step ``step`` of the chains with the ids ``chain`` (B,): (xi (B, k) standard normals, u (B,) uniform).  Key
    (seed low word, seed high word), counter (step, chain low, chain high, purpose): purpose j < ceil(k / 2) gives the Box-Muller
    pair (2 j, 2 j + 1) -- words 0, 1 -> u1, words 2, 3 -> u2, z0 = sqrt(-2 log u1) cos(2 pi u2), z1 = .. sin(2 pi u2) -- and purpose
    0xFFFFFFFF the uniform (words 0, 1).  The uniforms are exact; ``dtype`` is that of the logarithm and the circular functions."""
    chain = np.atleast_1d(np.asarray(chain, dtype=np.uint64))
    B, kh, T = len(chain), (int(k) + 1) // 2, dtype
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    key = np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=np.uint64)
    step = np.broadcast_to(np.asarray(step, dtype=np.uint64) & _U32, (B,))
    purpose = np.concatenate([np.arange(kh, dtype=np.uint64), np.array([MCMC_ACCEPT], dtype=np.uint64)])
    ctr = np.empty((B, kh + 1, 4), dtype=np.uint64)
    ctr[..., 0], ctr[..., 1], ctr[..., 2], ctr[..., 3] = step[:, None], (chain & _U32)[:, None], (chain >> _S32)[:, None], purpose[None, :]
    w = philox4x32(ctr, key)
    u1, u2 = mcmc_uniform(w[:, :kh, 0], w[:, :kh, 1]).astype(T), mcmc_uniform(w[:, :kh, 2], w[:, :kh, 3]).astype(T)
    rad, ang = np.sqrt(T(-2.0) * np.log(u1)), T(6.283185307179586) * u2
    xi = np.stack([rad * np.cos(ang), rad * np.sin(ang)], axis=-1).reshape(B, 2 * kh)[:, :int(k)]
    return xi, mcmc_uniform(w[:, kh, 0], w[:, kh, 1])


def mcmc_layout(n, k):
    """The state row of a chain (``rom_mcmc_layout``): offsets by name and ``row``, its length:
    theta (k) | phi | ls | mean (k) | M2 (k k) | mean_c (n) | kept | accepted | outside | not_spd | phi_min | theta_min (k)."""
    o = dict(theta=0, phi=k, ls=k + 1, mean=k + 2, M2=2 * k + 2, mean_c=2 * k + 2 + k * k)
    o["kept"] = o["mean_c"] + n
    o.update(accepted=o["kept"] + 1, outside=o["kept"] + 2, not_spd=o["kept"] + 3, phi_min=o["kept"] + 4, theta_min=o["kept"] + 5)
    o["row"] = o["theta_min"] + k
    return o


class McmcRun(NamedTuple):
    """``mcmc_host`` / ``mcmc_device``: state (B, row) the chains' rows (``mcmc_layout``), B = K t, chain = query t + index;
    samples (B, slots, k) with NaN in the slots this call did not write, or None; margin (B,): the smallest |log u - l| over the
    chain's evaluated steps of this call (inf without one) and margin_step (B,) the global step it occurred at (-1) -- host only,
    None from the device; info: the device call's dictionary, or None."""
    state: np.ndarray
    samples: Optional[np.ndarray]
    margin: Optional[np.ndarray]
    margin_step: Optional[np.ndarray]
    info: Optional[dict]


def _mcmc_eval(Ahat, bhat, Gr, p, theta):
    """c(theta) (B, n), Phi = |p - G_r c|^2 (B,) and whether every pivot of A(theta) is positive (B,), in the dtype of theta:
    A = sum_q e^theta_q Ahat_q factored as L D L^T without pivoting (the elimination of ``lm_factor``, csrc/rom_lm_small.h)."""
    A = np.einsum("bq,qij->bij", np.exp(theta), Ahat)
    n = A.shape[1]
    with np.errstate(all="ignore"):
        for j in range(n - 1):
            l = A[:, j + 1:, j] / A[:, j, j, None]
            A[:, j + 1:, j + 1:] -= A[:, j + 1:, j, None] * l[:, None, :]
        d = np.einsum("bjj->bj", A)
        invd = 1.0 / d
        c = np.array(np.broadcast_to(bhat, (len(theta), n)))
        for j in range(n - 1):
            c[:, j + 1:] -= (A[:, j + 1:, j] * invd[:, j, None]) * c[:, j, None]
        c *= invd
        for j in range(n - 1, 0, -1):
            c[:, :j] -= (A[:, j, :j] * invd[:, :j]) * c[:, j, None]
        rho = p - c @ Gr.T
    return c, np.einsum("br,br->b", rho, rho), (d > 0).all(axis=1)


def _mcmc_box(lo, hi, k):
    lo = np.array(np.broadcast_to(np.asarray(lo, dtype=np.float64), (k,)))
    hi = np.array(np.broadcast_to(np.asarray(hi, dtype=np.float64), (k,)))
    if not (np.isfinite(lo).all() and np.isfinite(hi).all() and (lo <= hi).all()):
        raise ValueError("mcmc: the box needs finite lo <= hi")
    return lo, hi


def mcmc_host(Ahat, bhat, Gr, P, invvar, theta0, L, lo, hi, seed, steps, burn, thin, chain0=0, step0=0, state=None, slots=None,
              dtype=np.float64) -> McmcRun:
    """Adaptive random-walk Metropolis for the posterior of theta = log a given noisy data: THE SPECIFICATION of ``rom_mcmc``
    (csrc/rom_mcmc.hip), pure NumPy, vectorised over the chains.

    The model: theta in the box [lo, hi]^k with a uniform prior; in the reduced sensor coordinates of ``polish_parameters_device``
    (p = U^T (w y), G_r) the potential is Phi(theta) = ||p - G_r c(theta)||^2 and the log-posterior inside the box
    -invvar Phi / 2, invvar = 1 / sigma^2 per query.  Ahat (k, n, n), bhat (n,), Gr (r, n), P (K, r), invvar (K,), theta0 (K, k) or
    (K, t, k) the starts (clipped to the box), L (K, k, k) the queries' lower-triangular proposal factors (the strict upper
    triangle is not read).  One chain is a pair (query, index), B = K t of them, with the id chain0 + its position.  Step i, the
    GLOBAL index step0 <= i < step0 + steps:

    1. k standard normals xi and a uniform u: ``mcmc_draws(seed, id, i, k)``.
    2. theta' = theta + e^ls (L xi); a pinned coordinate (lo_q == hi_q) keeps theta_q bit for bit.
    3. A coordinate of theta' outside [lo, hi]: rejected without an evaluation, alpha = 0, ``outside`` goes up.
    4. Else Phi(theta'): a pivot of A(theta') that is not positive rejects with alpha = 0 and ``not_spd`` goes up; otherwise
       l = -invvar (Phi' - Phi) / 2, accepted iff log u < l, alpha = min(1, e^min(l, 0)) (a NaN l rejects with alpha = 0).
    5. i < burn: ls += (i + 1)^-0.6 (alpha - 0.234) (Robbins-Monro; frozen afterwards, so the chain past burn-in is a Metropolis
       chain).
    6. i >= burn: the current state (again after a rejection) enters ``kept``, the Welford mean and M2 (k, k) of theta
       (M2 += (theta - old mean)(theta - new mean)^T), the running mean of c, ``accepted``, and the smallest Phi with its theta
       (both start at the start's); if (i - burn) % thin == thin - 1 and its slot (i - burn) / thin < slots, theta is a sample.

    ``state`` (B, row) with step0 > 0 resumes the chains from their rows (``mcmc_layout``); the model is evaluated at the row's
    theta once more, so a split run returns the bits of the unsplit one.  ``slots`` None: every slot of the steps up to
    step0 + steps; 0: no samples.  A start whose A(theta) is not positive definite raises LinAlgError; a query whose Phi at the
    start is NaN gets a NaN row.  ``dtype=np.longdouble`` runs the same arithmetic in long double from the same Philox words.
    Returns a ``McmcRun``; its margin tells up to which step another arithmetic can be held to this trajectory."""
    T = dtype
    Ahat, bhat, Gr = np.asarray(Ahat, dtype=T), np.asarray(bhat, dtype=T), np.asarray(Gr, dtype=T)
    k, n, r = Ahat.shape[0], Ahat.shape[1], Gr.shape[0]
    P = np.asarray(P, dtype=T).reshape(-1, r)
    K = len(P)
    steps, burn, thin, step0, chain0 = int(steps), int(burn), int(thin), int(step0), int(chain0)
    if steps < 0 or burn < 0 or thin < 1 or step0 < 0 or chain0 < 0:
        raise ValueError(f"mcmc: steps = {steps}, burn = {burn}, thin = {thin}, step0 = {step0}, chain0 = {chain0} (steps, burn, "
                         "step0, chain0 >= 0, thin >= 1)")
    lo, hi = _mcmc_box(lo, hi, k)
    o = mcmc_layout(n, k)
    if state is None:
        if step0:
            raise ValueError("mcmc: step0 > 0 resumes from `state`")
        theta = np.asarray(theta0, dtype=T).reshape(K, -1, k)
        t = theta.shape[1]
        theta = np.clip(theta.reshape(K * t, k), lo.astype(T), hi.astype(T))
    else:
        state = np.array(state, dtype=T).reshape(-1, o["row"])
        t = len(state) // max(K, 1)
        theta = state[:, :k].copy()
    B = K * t
    if len(theta) != B:
        raise ValueError(f"mcmc: {len(theta)} chains for K = {K} queries")
    query = np.repeat(np.arange(K), t)
    p, iv = P[query], np.asarray(invvar, dtype=T).reshape(K)[query]
    Lc = np.tril(np.asarray(L, dtype=T).reshape(K, k, k))[query]
    ids = (chain0 + np.arange(B)).astype(np.uint64)
    pinned = lo == hi
    loT, hiT = lo.astype(T), hi.astype(T)

    c, phi, ok = _mcmc_eval(Ahat, bhat, Gr, p, theta)
    dead = np.isnan(theta[:, 0]) if (state is not None and step0 > 0) else np.zeros(B, dtype=bool)
    if (~ok & ~dead).any():
        raise np.linalg.LinAlgError("mcmc: A(theta) not positive definite at a start")
    dead |= np.isnan(phi)
    if state is None or step0 == 0:
        ls, mean, M2, meanc = np.zeros(B, dtype=T), np.zeros((B, k), dtype=T), np.zeros((B, k, k), dtype=T), np.zeros((B, n), dtype=T)
        cnt = {name: np.zeros(B, dtype=np.int64) for name in ("kept", "accepted", "outside", "not_spd")}
        phimin, thmin = phi.copy(), theta.copy()
    else:
        ls, mean, M2 = state[:, o["ls"]].copy(), state[:, o["mean"]:o["mean"] + k].copy(), state[:, o["M2"]:o["M2"] + k * k].reshape(B, k, k).copy()
        meanc = state[:, o["mean_c"]:o["mean_c"] + n].copy()
        cnt = {name: np.nan_to_num(state[:, o[name]]).astype(np.int64) for name in ("kept", "accepted", "outside", "not_spd")}
        phimin, thmin = state[:, o["phi_min"]].copy(), state[:, o["theta_min"]:o["theta_min"] + k].copy()
    total = max(0, step0 + steps - burn) // thin
    slots = total if slots is None else int(slots)
    samples = np.full((B, slots, k), np.nan, dtype=T) if slots > 0 else None
    margin, margin_step = np.full(B, np.inf), np.full(B, -1, dtype=np.int64)
    s = np.exp(ls)

    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(step0, step0 + steps):
            xi, u = mcmc_draws(seed, ids, i, k, dtype=T)                                         # 1
            prop = np.where(pinned, theta, theta + s[:, None] * np.einsum("bqp,bp->bq", Lc, xi))  # 2
            out = ~((prop >= loT) & (prop <= hiT)).all(axis=1)                                   # 3
            cnt["outside"][out] += 1
            alpha, accept = np.zeros(B, dtype=T), np.zeros(B, dtype=bool)
            ins = np.flatnonzero(~out)
            if ins.size:                                                                         # 4
                cn, phin, okn = _mcmc_eval(Ahat, bhat, Gr, p[ins], prop[ins])
                cnt["not_spd"][ins[~okn]] += 1
                l = T(-0.5) * iv[ins] * (phin - phi[ins])
                good = okn & ~np.isnan(l)
                logu = np.log(u[ins].astype(T))
                acc = good & (logu < l)
                alpha[ins] = np.where(good, np.minimum(T(1.0), np.exp(np.minimum(l, T(0.0)))), T(0.0))
                gap = np.where(good, np.abs(logu - l), np.inf).astype(np.float64)
                closer = gap < margin[ins]
                margin[ins[closer]], margin_step[ins[closer]] = gap[closer], i
                ia = ins[acc]
                theta[ia], c[ia], phi[ia] = prop[ins][acc], cn[acc], phin[acc]
                accept[ia] = True
            if i < burn:                                                                         # 5
                ls = ls + T(i + 1) ** T(-0.6) * (alpha - T(MCMC_TARGET))
                s = np.exp(ls)
                continue
            cnt["kept"] += 1                                                                     # 6
            cnt["accepted"][accept] += 1
            kept = cnt["kept"].astype(T)
            d = theta - mean
            mean = mean + d / kept[:, None]
            M2 = M2 + d[:, :, None] * (theta - mean)[:, None, :]
            meanc = meanc + (c - meanc) / kept[:, None]
            lower = phi < phimin
            phimin[lower], thmin[lower] = phi[lower], theta[lower]
            j = i - burn
            if samples is not None and j % thin == thin - 1 and j // thin < slots:
                samples[:, j // thin] = theta

    out_state = np.zeros((B, o["row"]), dtype=T)
    out_state[:, :k], out_state[:, o["phi"]], out_state[:, o["ls"]] = theta, phi, ls
    out_state[:, o["mean"]:o["mean"] + k], out_state[:, o["M2"]:o["M2"] + k * k] = mean, M2.reshape(B, k * k)
    out_state[:, o["mean_c"]:o["mean_c"] + n] = meanc
    for name in ("kept", "accepted", "outside", "not_spd"):
        out_state[:, o[name]] = cnt[name]
    out_state[:, o["phi_min"]], out_state[:, o["theta_min"]:o["theta_min"] + k] = phimin, thmin
    out_state[dead] = np.nan
    return McmcRun(out_state, samples, margin, margin_step, None)


MCMC_LIMITS = dict(n=64, k=16, r=64, t=8)   # rom_mcmc (csrc/rom_mcmc.hip)


def _check_mcmc_limits(n, k, r, t):
    for name, v in (("n", n), ("k", k), ("r", r), ("t", t)):
        if not 1 <= v <= MCMC_LIMITS[name]:
            raise ValueError(f"the device sampler (rom_mcmc) needs 1 <= {name} <= {MCMC_LIMITS[name]}, got {name} = {v}: "
                             "use device=False (mcmc_host)")


def mcmc_device(ctx, Ahat, bhat, Gr, P, invvar, theta0, L, lo, hi, seed, steps, burn, thin, chain0=0, step0=0, state=None,
                slots=None) -> McmcRun:
    """``mcmc_host`` on the device of ``ctx`` (``rom_mcmc``, one workgroup per chain): the same arguments, in the reduced sensor
    coordinates of ``reduce_sensors`` / ``reduce_measurements`` (Gr = S V^T, P = U^T (w y)), and the same rows.  margin and
    margin_step are None."""
    Ahat, bhat, Gr = np.asarray(Ahat, dtype=np.float64), np.asarray(bhat, dtype=np.float64), np.asarray(Gr, dtype=np.float64)
    k, n, r = Ahat.shape[0], Ahat.shape[1], Gr.shape[0]
    P = np.asarray(P, dtype=np.float64).reshape(-1, r)
    K = len(P)
    o = mcmc_layout(n, k)
    lo, hi = _mcmc_box(lo, hi, k)
    if state is None:
        theta0 = np.asarray(theta0, dtype=np.float64).reshape(K, -1, k)
        t = theta0.shape[1]
        rows = np.zeros((K * t, o["row"]))
        rows[:, :k] = theta0.reshape(K * t, k)
    else:
        rows = np.array(state, dtype=np.float64).reshape(-1, o["row"])
        t = len(rows) // max(K, 1)
    _check_mcmc_limits(n, k, r, t)
    steps, burn, thin = int(steps), int(burn), int(thin)
    total = max(0, int(step0) + steps - burn) // max(thin, 1)
    slots = total if slots is None else int(slots)
    if K == 0:
        return McmcRun(rows, None, None, None, None)
    STATE = ctx.upload(rows)
    SAMPLES = ctx.upload(np.full(K * t * slots * k, np.nan)) if slots > 0 else None
    info = ctx.mcmc(n, k, r, ctx.upload(Ahat), ctx.upload(bhat), ctx.upload(Gr), ctx.upload(P), 0, r, K, t,
                    ctx.upload(np.asarray(invvar, dtype=np.float64).reshape(K)), ctx.upload(np.asarray(L, dtype=np.float64).reshape(K, k, k)),
                    lo, hi, seed, steps, burn, thin, STATE, SAMPLES=SAMPLES, slots=slots, chain0=chain0, step0=step0)
    samples = SAMPLES.download().reshape(K * t, slots, k) if slots > 0 else None
    return McmcRun(STATE.download().reshape(K * t, o["row"]), samples, None, None, info)


def proposal_factors(Ahat, bhat, Gr, theta, invvar, lo, hi):
    """The default proposal factors L (K, k, k), lower triangular, at the points theta (K, k): with J_r = G_r dc/dtheta there,
    H = invvar J_r^T J_r + diag(12 / (hi - lo)^2) -- the Gauss-Newton Hessian of the negative log-posterior plus the inverse
    variance of the uniform prior, which caps the directions the data do not see -- and L = chol(H^-1) 2.38 / sqrt(k).  A pinned
    coordinate (lo_q == hi_q) gets a zero row and column.  NumPy, batched over the queries."""
    Ahat, bhat, Gr = np.asarray(Ahat, dtype=np.float64), np.asarray(bhat, dtype=np.float64), np.asarray(Gr, dtype=np.float64)
    k = Ahat.shape[0]
    theta = np.asarray(theta, dtype=np.float64).reshape(-1, k)
    K = len(theta)
    lo, hi = _mcmc_box(lo, hi, k)
    free = lo < hi
    _, _, J = _rom_state(Ahat, bhat, Gr, np.zeros((K, Gr.shape[0])), theta)
    H = np.asarray(invvar, dtype=np.float64).reshape(K, 1, 1) * np.einsum("bmq,bmp->bqp", J, J)
    H = H + np.diag(12.0 / np.where(free, hi - lo, 1.0) ** 2)
    both = free[:, None] & free[None, :]
    H = np.where(both, H, 0.0) + np.diag((~free).astype(np.float64))
    C = np.linalg.inv(H)
    C = 0.5 * (C + C.transpose(0, 2, 1))
    return np.where(both, np.linalg.cholesky(C), 0.0) * (2.38 / np.sqrt(k))


class ParameterPosterior(NamedTuple):
    """``ParameterLibrary.posterior`` / ``posterior_summary``, everything in theta = log a: mean (K, k), cov (K, k, k) and
    sd (K, k) pooled over the t chains of a query by the law of total variance; rhat (K, k): Gelman-Rubin's potential scale
    reduction from the chains' means and variances (NaN with one chain or a pinned coordinate); acceptance (K, t) of the steps
    past burn-in and scale (K, t) = e^ls, the adapted proposal scales; a_map (K, k) = e^theta at the smallest misfit any chain
    of the query saw, misfit_min (K,) = sqrt(Phi_min + perp2) there; mean_coefficients (K, n): the posterior mean of c;
    outside, not_spd (K, t): proposals rejected for leaving the box / for a pivot that was not positive; samples (K, t, slots, k)
    or None; states: DeviceArray (K, dim) of the posterior-mean states, or None."""
    mean: np.ndarray
    cov: np.ndarray
    sd: np.ndarray
    rhat: np.ndarray
    acceptance: np.ndarray
    scale: np.ndarray
    a_map: np.ndarray
    misfit_min: np.ndarray
    mean_coefficients: np.ndarray
    outside: np.ndarray
    not_spd: np.ndarray
    samples: Optional[np.ndarray]
    states: Optional[DeviceArray]

    def quantiles(self, q):
        """The quantiles q (scalar or (Q,)) of theta per query over the kept samples of all its chains: (K, k) or (Q, K, k)."""
        if self.samples is None:
            raise ValueError("quantiles need kept samples: posterior(..., thin >= 1)")
        K, t, slots, k = self.samples.shape
        return np.quantile(self.samples.reshape(K, t * slots, k), q, axis=1)


def posterior_summary(state, n, k, t, samples=None, perp2=None, states=None) -> ParameterPosterior:
    """The ``ParameterPosterior`` of the state rows (K t, row) of ``mcmc_host`` / ``mcmc_device`` (t chains per query)."""
    o = mcmc_layout(n, k)
    S = np.asarray(state, dtype=np.float64).reshape(-1, t, o["row"])
    K = len(S)
    kept = S[:, :, o["kept"]]
    m = S[:, :, o["mean"]:o["mean"] + k]
    M2 = S[:, :, o["M2"]:o["M2"] + k * k].reshape(K, t, k, k)
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = m.mean(axis=1)
        dm = m - mean[:, None, :]
        cov = (M2 / kept[:, :, None, None]).mean(axis=1) + np.einsum("ktq,ktp->kqp", dm, dm) / t
        sd = np.sqrt(np.einsum("kqq->kq", cov))
        W = (np.einsum("ktqq->ktq", M2) / (kept[:, :, None] - 1.0)).mean(axis=1)
        Bn = (dm * dm).sum(axis=1) / (t - 1) if t > 1 else np.full((K, k), np.nan)
        N = kept.mean(axis=1)[:, None]
        rhat = np.sqrt(((N - 1.0) / N * W + Bn) / W)
        acceptance = S[:, :, o["accepted"]] / kept
        best = np.argmin(np.where(np.isnan(S[:, :, o["phi_min"]]), np.inf, S[:, :, o["phi_min"]]), axis=1)
        pick = S[np.arange(K), best]
        perp2 = np.zeros(K) if perp2 is None else np.asarray(perp2, dtype=np.float64).reshape(K)
        misfit = np.sqrt(pick[:, o["phi_min"]] + perp2)
    cnt = lambda name: np.nan_to_num(S[:, :, o[name]]).astype(np.int64)  # noqa: E731
    return ParameterPosterior(mean, cov, sd, rhat, acceptance, np.exp(S[:, :, o["ls"]]), np.exp(pick[:, o["theta_min"]:o["theta_min"] + k]),
                              misfit, S[:, :, o["mean_c"]:o["mean_c"] + n].mean(axis=1), cnt("outside"), cnt("not_spd"),
                              None if samples is None else np.asarray(samples).reshape(K, t, -1, k), states)


# ---- D-optimal sensor selection for the parameter problem: greedy Bayesian experimental design -----------------------------------
DOPT_LIMITS = dict(n=64, k=16, m=1024)   # rom_sensor_dopt (csrc/rom_oed.hip)
DOPT_STOPS = ("m", "no_gain", "no_candidates")   # stop reasons 0, 1, 2


class SensorDesign(NamedTuple):
    """``sensor_dopt_host`` / ``sensor_dopt_device`` / ``ParameterLibrary.select_sensors``.  picks (made,): indices into the
    candidates, in pick order; gain (made,): the score of every pick, sum_j log1p(s_j) over the library; information (made,): the
    criterion Phi after every pick, in nats -- the expected information gain, the sum of the gains over 2 (M - skipped);
    posterior_sd (M, k): sqrt diag(F_j^-1) of the linearised posterior of log a at every library entry (the prior's for a skipped
    entry); stop_reason: "m", "no_gain" (the gain fell to rel_tol times the first) or "no_candidates"; skipped (M,): 0, 1 (A(theta_j)
    has a pivot that is not positive) or 2 (theta_j is not finite) -- such an entry takes no part; nan_candidates: candidates whose
    first score was not finite (NaN / Inf in their row: never picked); points (made, 2): the picked points, where the candidates were points, else None."""
    picks: np.ndarray
    gain: np.ndarray
    information: np.ndarray
    posterior_sd: np.ndarray
    stop_reason: str
    skipped: np.ndarray
    nan_candidates: int = 0
    points: Optional[np.ndarray] = None


def sensor_prior_factor(prior_cov, k):
    """T0 (k, k) with T0 T0^T = the prior covariance of theta = log a: ``prior_cov`` a scalar or (k,) of variances (T0 diagonal) or
    a (k, k) symmetric positive semi-definite matrix (T0 = V sqrt(lambda) of its eigen-decomposition).  A zero variance is a
    parameter that is known."""
    C = np.asarray(prior_cov, dtype=np.float64)
    if C.ndim < 2:
        v = np.array(np.broadcast_to(C, (k,)))
        if not (np.isfinite(v).all() and (v >= 0).all()):
            raise ValueError("sensor design: the prior variances must be finite and not negative")
        return np.diag(np.sqrt(v))
    if C.shape != (k, k) or not np.isfinite(C).all() or not np.allclose(C, C.T, rtol=1e-12, atol=0.0):
        raise ValueError(f"sensor design: the prior covariance must be a finite symmetric ({k}, {k}) matrix")
    lam, V = np.linalg.eigh(0.5 * (C + C.T))
    if lam.min() < -1e-12 * max(lam.max(), 0.0):
        raise ValueError("sensor design: the prior covariance is not positive semi-definite")
    return V * np.sqrt(np.maximum(lam, 0.0))


def sensor_sensitivities_host(Ahat, bhat, theta, status=False):
    """X (M, n, k) = -dc/dtheta at the rows of theta (M, k): column q = e^theta_q A^-1 Ahat_q c (``_rom_state``, py:59-60), with
    A = sum_q e^theta_q Ahat_q factored as L D L^T without pivoting (the elimination of ``lm_factor``, csrc/rom_lm_small.h).  A row
    whose A has a pivot that is not positive (status 1) or whose theta is not finite (status 2) gets X = 0.  With ``status``:
    (X, status (M,))."""
    Ahat, bhat = np.asarray(Ahat, dtype=np.float64), np.asarray(bhat, dtype=np.float64)
    k, n = Ahat.shape[0], Ahat.shape[1]
    theta = np.asarray(theta, dtype=np.float64).reshape(-1, k)
    M = len(theta)
    with np.errstate(all="ignore"):
        ea = np.exp(theta)
        A = np.einsum("bq,qij->bij", ea, Ahat)
        for j in range(n - 1):
            l = A[:, j + 1:, j] / A[:, j, j, None]
            A[:, j + 1:, j + 1:] -= A[:, j + 1:, j, None] * l[:, None, :]
        d = np.einsum("bjj->bj", A)
        invd = 1.0 / d

        def solve(R):   # R (M, n, cols)
            R = R.copy()
            for j in range(n - 1):
                R[:, j + 1:] -= (A[:, j + 1:, j] * invd[:, j, None])[:, :, None] * R[:, j, None, :]
            R *= invd[:, :, None]
            for j in range(n - 1, 0, -1):
                R[:, :j] -= (A[:, j, :j] * invd[:, :j])[:, :, None] * R[:, j, None, :]
            return R

        c = solve(np.broadcast_to(bhat, (M, n))[:, :, None].copy())[:, :, 0]
        X = solve(np.einsum("qij,bj->biq", Ahat, c) * ea[:, None, :])
    st = np.where(np.isfinite(theta).all(axis=1), np.where((d > 0).all(axis=1), 0, 1), 2).astype(np.int64)
    X[st != 0] = 0.0
    return (X, st) if status else X


def sensor_dopt_scores_host(Z, E, block=4096):
    """score (ncand,) = sum_j log1p(|Z_j^T e_x|^2) for the rows e_x of E (ncand, n) and Z (M, n, k), the entries added in
    ascending j."""
    out = np.empty(len(E))
    with np.errstate(all="ignore"):
        for x0 in range(0, len(E), block):
            U = np.einsum("xn,jnk->xjk", E[x0:x0 + block], Z)
            out[x0:x0 + block] = np.cumsum(np.log1p(np.einsum("xjk,xjk->xj", U, U)), axis=1)[:, -1]
    return out


def sensor_dopt_update_host(Z, T, e):
    """The rank-one update of every entry for the sensor with the row e (n,), in place: u = Z_j^T e, s = |u|^2, rho = sqrt(1 + s),
    beta = 1 / (rho (rho + 1)), Z_j -= beta (Z_j u) u^T, T_j -= beta (T_j u) u^T.  Returns s (M,)."""
    u = np.einsum("n,jnk->jk", e, Z)
    s = np.einsum("jk,jk->j", u, u)
    rho = np.sqrt(1.0 + s)
    beta = 1.0 / (rho * (rho + 1.0))
    Z -= (beta[:, None] * np.einsum("jnk,jk->jn", Z, u))[:, :, None] * u[:, None, :]
    T -= (beta[:, None] * np.einsum("jak,jk->ja", T, u))[:, :, None] * u[:, None, :]
    return s


def sensor_dopt_host(Ahat, bhat, theta, E, m, sigma, prior_cov, rel_tol=0.0) -> SensorDesign:
    """Greedy Bayesian D-optimal sensor selection for the parameters: THE SPECIFICATION of ``rom_sensor_dopt`` (csrc/rom_oed.hip),
    pure NumPy.  Ahat (k, n, n), bhat (n,): the reduced model; theta (M, k) = log a of the library entries the design averages
    over; E (ncand, n): row x the basis at candidate x (times the weight of that sensor); sigma: the standard deviation of the
    independent measurement noise; prior_cov: see ``sensor_prior_factor``.

    With X_j = ``sensor_sensitivities_host`` the Jacobian row of candidate x at entry j is g = X_j^T e_x, the posterior precision
    of a sensor set S is F_j(S) = Gamma_0 + sigma^-2 sum_S g g^T and the criterion Phi(S) = 1 / (2 M) sum_j log det(Gamma_0^-1 F_j(S))
    -- the expected information gain of the linearised Gaussian model, monotone submodular in S, so that the greedy reaches
    (1 - 1/e) of the optimum.  State per entry: T_j (k, k) with T_j T_j^T = F_j^-1 and Z_j = X_j T_j / sigma, from T_j = T0.  A step:

    1. score(x) = sum_j log1p(|Z_j^T e_x|^2), the entries in ascending j (= 2 M times the gain in Phi of adding x);
    2. the pick x* is the first maximum among the candidates not yet picked whose score is finite; none: stop "no_candidates";
       score(x*) <= rel_tol times the first step's: stop "no_gain" (with rel_tol = 0: nothing left to learn);
    3. ``sensor_dopt_update_host``: the symmetric square root of the Sherman-Morrison downdate, (I - beta u u^T)^2 =
       I - u u^T / (1 + s), without a factorisation or a difference of near-equal numbers.

    A skipped entry (see ``SensorDesign``) has Z_j = 0 and adds exactly 0 to every score."""
    Ahat, bhat, E = np.asarray(Ahat, dtype=np.float64), np.asarray(bhat, dtype=np.float64), np.asarray(E, dtype=np.float64)
    k, n = Ahat.shape[0], Ahat.shape[1]
    theta = np.asarray(theta, dtype=np.float64).reshape(-1, k)
    E = E.reshape(-1, n)
    M, ncand, m = len(theta), len(E), int(m)
    if not (sigma > 0 and np.isfinite(sigma)):
        raise ValueError(f"sensor design: sigma = {sigma}, the noise level must be positive and finite")
    if M < 1 or not 1 <= m <= ncand:
        raise ValueError(f"sensor design: M = {M} library entries (at least 1), m = {m} picks of ncand = {ncand} candidates")
    T0 = sensor_prior_factor(prior_cov, k)
    X, st = sensor_sensitivities_host(Ahat, bhat, theta, status=True)
    Z = (X @ T0) / sigma
    T = np.array(np.broadcast_to(T0, (M, k, k)))
    taken = np.zeros(ncand, dtype=bool)
    picks, gain, reason, first, nans = [], [], 0, 0.0, 0
    with np.errstate(all="ignore"):
        for t in range(m):
            score = sensor_dopt_scores_host(Z, E)
            if t == 0:
                nans = int((~np.isfinite(score)).sum())
            ok = np.isfinite(score) & ~taken
            if not ok.any():
                reason = 2
                break
            x = int(np.argmax(np.where(ok, score, -np.inf)))   # (the first maximum)
            if t == 0:
                first = score[x]
            if score[x] <= rel_tol * first:
                reason = 1
                break
            picks.append(x)
            gain.append(score[x])
            taken[x] = True
            sensor_dopt_update_host(Z, T, E[x])
    gain = np.array(gain, dtype=np.float64)
    live = M - int((st != 0).sum())
    info = np.cumsum(gain) / (2.0 * live) if live else np.zeros(len(gain))
    return SensorDesign(np.array(picks, dtype=np.int64), gain, info, np.sqrt(np.einsum("jab,jab->ja", T, T)), DOPT_STOPS[reason], st, nans)


def _check_dopt_limits(n, k, m):
    for name, v in (("n", n), ("k", k), ("m", m)):
        if not 1 <= v <= DOPT_LIMITS[name]:
            raise ValueError(f"the device design (rom_sensor_dopt) needs 1 <= {name} <= {DOPT_LIMITS[name]}, got {name} = {v}: "
                             "use device=False (sensor_dopt_host)")


def sensor_dopt_device(ctx, Ahat, bhat, theta, E, m, sigma, prior_cov, rel_tol=0.0) -> SensorDesign:
    """``sensor_dopt_host`` on the device of ``ctx`` (``rom_sensor_dopt_init``, ``rom_sensor_dopt``): the same arguments and the same
    tuple.  The m steps run without host involvement."""
    Ahat, bhat, E = np.asarray(Ahat, dtype=np.float64), np.asarray(bhat, dtype=np.float64), np.asarray(E, dtype=np.float64)
    k, n = Ahat.shape[0], Ahat.shape[1]
    theta = np.asarray(theta, dtype=np.float64).reshape(-1, k)
    E = E.reshape(-1, n)
    M, ncand = len(theta), len(E)
    _check_dopt_limits(n, k, int(m))
    T0 = sensor_prior_factor(prior_cov, k)
    lay = ctx.sensor_dopt_layout(n, k)
    STATE, _ = ctx.sensor_dopt_init(n, k, ctx.upload(Ahat), ctx.upload(bhat), ctx.upload(theta), 0, k, M, T0, sigma)
    picks, gain, info = ctx.sensor_dopt(n, k, STATE, 0, M, ctx.upload(E), 0, n, ncand, m, rel_tol=rel_tol)
    rows = STATE.download(M * lay["entry"]).reshape(M, lay["entry"])
    T = rows[:, lay["t_offset"]:lay["t_offset"] + lay["kp"] ** 2].reshape(M, lay["kp"], lay["kp"])[:, :k, :k]
    st = rows[:, lay["status_offset"]].astype(np.int64)
    live = M - int((st != 0).sum())
    information = np.cumsum(gain) / (2.0 * live) if live else np.zeros(len(gain))
    return SensorDesign(picks, gain, information, np.sqrt(np.einsum("jab,jab->ja", T, T)), DOPT_STOPS[info["stop_reason"]], st,
                        info["nan_candidates"])


def select_sensors_parameters(sm, basis, a_library, candidates, m, sigma, **kw) -> SensorDesign:
    """``ParameterLibrary(sm, basis, a_library).select_sensors(candidates, m, sigma, **kw)``: D-optimal sensors for estimating the
    parameters, averaged over ``a_library``."""
    return ParameterLibrary(sm, basis, a_library).select_sensors(candidates, m, sigma, **kw)
