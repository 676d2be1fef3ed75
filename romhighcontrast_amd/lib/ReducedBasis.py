"""Host-side mirror of the reference's ``src/lib/ReducedBasis.py`` driving the HIP kernels.

Same public names (constants, helper functions, ``BaseReducedBasis``, ``ReducedBasisGreedy``,
``ReducedBasisRandom``, ``ReducedBasisPCA``) and the same ``build(n, sm, solutions2train, a2train,
solutions2train_h1norm, **kwargs)`` contract; citations are reference file:line.

The arithmetic runs on the GPU: Euclidean orthonormalisation is a re-orthogonalised Gram-Schmidt
(two passes of MFMA GEMMs per vector), the greedy sweep keeps the training set, the approximations
and the residual norms in HBM, and the PCA is a few passes of thin MFMA products over the block (rom_pod).
Orthonormal bases are defined up to the sign of each vector (NumPy's Householder QR at :19 may
return negative diagonals in R); every consumer in the reference is sign-invariant.
"""
from __future__ import annotations

from logging import warning
from typing import List, NamedTuple

import numpy as np

from .. import _ffi
from .Estimators import EstimatorInv, EstimatorLinear
from .SolutionsManagers import DeviceArray, SolutionsManager, _as_device

INFINIT_A = 1e10  # (:11)

GREEDY_FOR_H10 = r"$H^1_0$"  # (:101)
GREEDY_FOR_GALERKIN = "galerkin"  # (:102)
GREEDY_FOR_RESIDUAL = "residual"  # weak greedy on the residual error bound: no training snapshots (rom_weak_greedy)


def get_high_contrast_coefficient(a):
    """(:14-15) largest block coefficient of each parameter."""
    return np.array([np.max(coefs, axis=(-1, -2)) for coefs in a])


def _orthonormalize_device(ctx: _ffi.Context, X: DeviceArray) -> DeviceArray:
    """Rows of X -> Euclidean-orthonormal rows spanning the same nested subspaces (rom_orthonormalize_rows: device
    CGS2, no host round trip per row)."""
    n, dim = X.rows, X.dim
    n = min(n, dim)   # (more rows than dimensions: the thin QR of the reference, np.linalg.qr(rb.T) at :19, returns dim of them)
    Q = ctx.alloc(max(n * dim, 1))
    if n:
        ctx.orthonormalize_rows(X.buf, n, dim, Q)
    return DeviceArray(Q, n, dim)


def orthonormalize_base(rb):
    """(:18-21) Euclidean orthonormalisation of the basis rows (thin QR of ``rb.T``)."""
    if isinstance(rb, DeviceArray):
        return _orthonormalize_device(_ffi.get_context(), rb)
    rb = np.asarray(rb, dtype=np.float64)
    if rb.size == 0:
        return rb.reshape(0, rb.shape[-1] if rb.ndim == 2 else 0)
    ctx = _ffi.get_context()
    return _orthonormalize_device(ctx, _as_device(ctx, rb, rb.shape[-1])).numpy()


def sort_orthogonalize_base(a_selected, rb):
    """(:24-29): order by ``argsort(1/a)``; like the reference the row permutation is applied
    twice before the orthonormalisation."""
    a_selected = np.asarray(a_selected, dtype=np.float64)
    order = np.argsort(1 / a_selected)
    rb = np.asarray(rb)[order, :]
    return a_selected[order], orthonormalize_base(rb[order, :])


def state_estimation_curves(E, measurements, proj, P, T, n_values):
    """State estimation of ``BaseReducedBasis.state_estimation`` (:65-70) for every n in ``n_values`` from the outputs of
    one error-curves call, on the host: ``{n: (c (n, M), absolute H^1_0 errors (M,))}``.

    E (N, points): the N basis rows at the measurement points; measurements (M, points); proj (N+1, M): absolute
    projection errors; P (M, N), T (N, N): the coefficients of the projections in the A_1-orthonormal basis W and
    C = T W.  c is the reference's own least-squares fit on the first n rows (minimum norm when underdetermined); the
    estimate c^T C[:n] = (T[:n, :n]^T c)^T W[:n] lies in span W[:n], so its error is
    sqrt(proj_n^2 + ||T[:n, :n]^T c - p_{:n}||^2) (W is A_1-orthonormal; a dependent row has a zero column in T)."""
    E, measurements = np.asarray(E, dtype=np.float64), np.asarray(measurements, dtype=np.float64)
    proj, P, T = np.asarray(proj), np.asarray(P), np.asarray(T)
    out = {}
    for n in n_values:
        c, *_ = np.linalg.lstsq(E[:n].T, measurements.T, rcond=-1)   # (n, M), as at :67
        d = T[:n, :n].T @ c - P[:, :n].T
        out[n] = (c, np.sqrt(proj[n] ** 2 + np.sum(d * d, axis=0)))
    return out


# ---- PBDW state estimation (parametrized-background data-weak; Maday, Patera, Penn, Yano 2015) --------------------------
# The estimate from measurements y = l(u) at m points is u* = v* + eta*, v* in V_n = span(basis rows), eta* in W_m = span
# of the H^1_0 Riesz representers omega_i of the point evaluations: u* interpolates the data and eta* is H^1_0-orthogonal
# to V_n.  In coefficients, u* = c^T C + d^T Omega with the saddle-point system [[G, L], [L^T, 0]] [d; c] = [y; 0],
# G = Gram matrix of the representers (G[i, j] = l_i(omega_j)), L[i, j] = l_i(C_j).
_PBDW_PIVOT_TOL = 1e-13   # a Cholesky pivot of G below this fraction of its diagonal entry: not numerically SPD
_PBDW_RANK_TOL = 1e-12    # sigma_min(B) / sigma_max(B) below this: the basis is not determined by the measurements


def _pbdw_bad_points(G):
    """Indices of the points that make the Gram matrix G singular: points whose functional vanishes (diagonal ~ 0, a point
    on the boundary) and points that repeat another one (correlation ~ 1)."""
    g = np.diag(G).copy()
    bad = set(np.flatnonzero(g <= _PBDW_PIVOT_TOL * max(float(np.max(g)), np.finfo(float).tiny)).tolist())
    ok = np.flatnonzero(g > 0)
    s = np.sqrt(g[ok])
    corr = G[np.ix_(ok, ok)] / s[:, None] / s[None, :]
    i, j = np.nonzero(np.triu(np.abs(corr) >= 1.0 - 1e-10, 1))
    bad.update(ok[i].tolist())
    bad.update(ok[j].tolist())
    return sorted(bad)


def pbdw_solve(G, L, Y, A_V=None, bounds=None, solver=None):
    """PBDW coefficients on the host.  G (m, m): H^1_0 Gram matrix of the sensors' Riesz representers; L (m, n):
    L[i, j] = l_i(C_j) (``evaluate_solutions(points, basis).T``); Y (K, m): measurements of K states; A_V (n, n), optional:
    H^1_0 Gram matrix of the basis rows.

    G = R^T R (Cholesky), B = R^-T L, y~ = R^-T Y^T; c = argmin ||y~ - B c|| (QR), d = R^-1 (y~ - B c).  With
    A_V = K K^T, beta[n' - 1] = sigma_min((B K^-T)[:, :n']) for n' = 1 .. n: the inf-sup constant of V_n' against the
    sensor space (the Cholesky factors nest, so every prefix is the constant of the first n' rows).

    bounds = (lo, hi) (n each, or scalars): the c-step becomes  argmin over lo <= c <= hi of ||y~ - B c||  (``inverse.bvls_host``,
    or ``solver(B, y~^T, lo, hi)`` returning a ``BvlsResult``); d = R^-1 (y~ - B c) as before, so the estimate still interpolates
    the measurements.  None: the unconstrained c.

    Returns (c (n, K), d (m, K), beta (n,) or None without A_V).  Raises ValueError if n > m, G is not numerically SPD
    (coincident points, or a point on the boundary: named), B is rank-deficient, or A_V is not SPD."""
    import scipy.linalg as sla
    from scipy.linalg.lapack import dpotrf

    G = np.asarray(G, dtype=np.float64)
    L = np.asarray(L, dtype=np.float64)
    m = G.shape[0]
    L = L.reshape(m, -1)
    n = L.shape[1]
    Y = np.asarray(Y, dtype=np.float64).reshape(-1, m)
    if n > m:
        raise ValueError(f"PBDW needs at least as many measurements as basis vectors: n = {n} > m = {m}")
    if m == 0:
        return np.zeros((0, Y.shape[0])), np.zeros((0, Y.shape[0])), (np.zeros(0) if A_V is not None else None)
    Rl, info = dpotrf(G, lower=1, clean=1)
    piv2 = np.diag(Rl) ** 2 / np.where(np.diag(G) > 0, np.diag(G), 1.0) if info == 0 else None
    if info != 0 or np.any(np.diag(G) <= 0) or np.min(piv2) <= _PBDW_PIVOT_TOL:
        bad = _pbdw_bad_points(G)
        if not bad:
            bad = [info - 1] if info > 0 else np.flatnonzero(piv2 <= _PBDW_PIVOT_TOL).tolist()
        raise ValueError(f"the Gram matrix of the measurement functionals is not numerically SPD: points {bad} "
                         "(coincident points, or points whose functional vanishes on the boundary)")
    B = sla.solve_triangular(Rl, L, lower=True)                   # R^-T L   (R = Rl^T)
    yt = sla.solve_triangular(Rl, Y.T, lower=True)                # R^-T Y^T
    if n:
        sv = np.linalg.svd(B, compute_uv=False)
        if not sv[-1] > _PBDW_RANK_TOL * sv[0]:
            raise ValueError(f"the basis is not determined by the measurements: B = R^-T L is rank-deficient "
                             f"(sigma_min / sigma_max = {sv[-1] / sv[0] if sv[0] > 0 else 0.0:.2e})")
        if bounds is None:
            Q, RB = np.linalg.qr(B)
            c = sla.solve_triangular(RB, Q.T @ yt, lower=False)
        else:
            if solver is None:
                from ..inverse import bvls_host as solver
            c = np.ascontiguousarray(solver(B, np.ascontiguousarray(yt.T), bounds[0], bounds[1]).c.T)
        res = yt - B @ c
    else:
        c = np.zeros((0, Y.shape[0]))
        res = yt
    d = sla.solve_triangular(Rl, res, lower=True, trans="T")       # R^-1 (y~ - B c)
    beta = None
    if A_V is not None:
        A_V = np.asarray(A_V, dtype=np.float64).reshape(n, n)
        try:
            KV = np.linalg.cholesky(0.5 * (A_V + A_V.T)) if n else np.zeros((0, 0))
        except np.linalg.LinAlgError as e:
            raise ValueError(f"the H^1_0 Gram matrix of the basis is not SPD (dependent basis rows): {e}") from None
        if n and not np.all(np.diag(KV) > 0):
            raise ValueError("the H^1_0 Gram matrix of the basis is not SPD (dependent basis rows)")
        BK = sla.solve_triangular(KV, B.T, lower=True).T if n else np.zeros((m, 0))   # B K^-T
        beta = np.array([np.linalg.svd(BK[:, :k], compute_uv=False)[-1] for k in range(1, n + 1)])
    return c, d, beta


class PBDWResult(NamedTuple):
    """``pbdw_state_estimation``: coefficients c (n, K) on the basis rows, d (m, K) on the representers, the inf-sup
    constants beta (n,) of the nested sub-bases, and the K estimates c^T C + d^T Omega (K, dim)."""
    c: np.ndarray
    d: np.ndarray
    beta: np.ndarray
    estimates: object


def _pbdw_operators(sm: SolutionsManager, basis, measurement_points, representers=True):
    """On the device: the basis rows C (DeviceArray or None for n = 0), the representers Omega (DeviceArray or None), G,
    L = l(C)^T and A_V = C A_1 C^T (rom_stencil_apply(unit) + rom_gemm_nt)."""
    ctx, dim = sm._ctx, sm.vspace_dim
    n = 0 if basis is None else len(basis)
    C = _as_device(ctx, basis, dim) if n else None
    Om, G = sm.riesz_h10_device(measurement_points, representers=representers)
    m = G.shape[0]
    if n:
        L = sm.evaluate_solutions(measurement_points, C).T
        AC = ctx.alloc(n * dim)
        sm._fem.stencil_apply(C.buf, n, AC)
        AVb = ctx.alloc(n * n)
        ctx.gemm_nt(n, n, dim, AC, 0, dim, C.buf, 0, dim, AVb, 0, n)
        A_V = AVb.download(n * n, shape=(n, n))
    else:
        L, A_V = np.zeros((m, 0)), np.zeros((0, 0))
    return C, Om, G, L, A_V


def pbdw_state_estimation(sm: SolutionsManager, basis, measurement_points, measurements, device=False, bounds=None) -> PBDWResult:
    """PBDW estimates of the K states measured at the m points (measurements (K, m), one row per state) with the
    background space spanned by the n rows of ``basis`` (ndarray or DeviceArray; n = 0 gives the minimum-norm interpolant
    Omega^T G^-1 y).  G, Omega, L and A_V are formed on the device, the (m + n)-sized problem is solved on the host
    (``pbdw_solve``), and the estimates are lifted on the device as c^T C + d^T Omega (two MFMA products into one buffer).
    ``estimates`` is a DeviceArray if ``device``, else an ndarray.  bounds = (lo, hi): the coefficients c stay inside that box
    (``pbdw_solve``; the bounded c-step runs on the device, ``rom_bvls``)."""
    ctx, dim = sm._ctx, sm.vspace_dim
    C, Om, G, L, A_V = _pbdw_operators(sm, basis, measurement_points)
    m, n = G.shape[0], L.shape[1]
    Y = np.asarray(measurements, dtype=np.float64).reshape(-1, m) if m else np.asarray(measurements).reshape(-1, 0)
    solver = None
    if bounds is not None and n:
        from ..inverse import bounded_lstsq
        solver = lambda B, Yt, lo, hi: bounded_lstsq(ctx, B.T, Yt, lo, hi)
    c, d, beta = pbdw_solve(G, L, Y, A_V, bounds=bounds, solver=solver)
    K = Y.shape[0]
    est = ctx.alloc(max(K * dim, 1))
    if K and n:
        ctx.gemm_nn(K, dim, n, ctx.upload(np.ascontiguousarray(c.T)), 0, n, C.buf, 0, dim, est, 0, dim)
    if K and m:
        ctx.gemm_nn(K, dim, m, ctx.upload(np.ascontiguousarray(d.T)), 0, m, Om.buf, 0, dim, est, 0, dim,
                    beta=1.0 if n else 0.0)
    if K and not m:
        est.fill(0.0)
    out = DeviceArray(est, K, dim)
    return PBDWResult(c, d, beta, out if device else out.numpy())


# ---- greedy sensor selection for PBDW (Binev, Cohen, Mula, Nichols 2018; rom_sensor_greedy) ------------------------------
# From a dictionary of candidate points, the greedy adds the point whose representer best captures the part of V_n that
# the chosen sensors do not see yet ("collective": all basis directions at once; "worst": the direction of V_n the sensors
# see worst, the smallest singular direction of A).  The whole loop runs on the device in one call; beta is formed on the
# host from A, A[j, i] = <psi_j, w_i>_{H^1_0} with psi_j / w_i orthonormal bases of W_k / V_n.
_SENSOR_MODES = {"collective": 0, "worst": 1}
_SENSOR_STOPS = {0: "m", 1: "captured", 2: "no_candidates"}


class SensorSelection(NamedTuple):
    """``select_sensors_pbdw``: the k picked points (k, 2) and their indices into the candidates (k,), in pick order;
    beta (k,): beta(V_n, W_j) for j = 1 .. k (0 while j is below the number n' of independent basis rows); the greedy's
    criterion at every pick (k,); and why the selection ended: "m" (m points picked), "captured" (the criterion fell below
    rel_tol times the first one), "no_candidates" (no candidate with a positive criterion left) or "beta_target"."""
    points: np.ndarray
    picks: np.ndarray
    beta: np.ndarray
    criterion: np.ndarray
    stop_reason: str


def sensor_beta_prefix(A, n_live, beta_target=None):
    """beta_j = beta(V_n, W_j) for j = 1 .. k from A (k, n), whose dead basis rows are zero columns: the n_live-th largest
    singular value of A[:j] -- sigma_min(A[:j, live]), the dead columns only add zero singular values -- for j >= n_live,
    0 below.  With ``beta_target``, the prefix up to the first j with beta_j >= beta_target (the greedy is sequential, so
    that prefix is exactly what a run stopped there would pick).  Returns (beta (k',), k', whether the target was met)."""
    A = np.asarray(A, dtype=np.float64)
    k = A.shape[0]
    beta = np.zeros(k)
    if n_live > 0:
        for j in range(n_live, k + 1):
            beta[j - 1] = np.linalg.svd(A[:j], compute_uv=False)[n_live - 1]
    if beta_target is not None:
        hit = np.flatnonzero(beta >= beta_target)
        if hit.size:
            return beta[:hit[0] + 1], int(hit[0]) + 1, True
    return beta, k, False


def select_sensors_pbdw(sm: SolutionsManager, basis, candidates, m, mode="collective", beta_target=None,
                        rel_tol=1e-10) -> SensorSelection:
    """Greedy selection of up to m of the ``candidates`` (K, 2) as PBDW sensors for the span of the rows of ``basis``
    (ndarray or DeviceArray); ``sm.interior_vertices()`` is the natural candidate set.  mode "collective" or "worst" (the
    two OMP variants of Binev, Cohen, Mula and Nichols); the selection stops after m picks, when the criterion falls to
    ``rel_tol`` times the first step's, when no candidate with a positive criterion is left, or -- with ``beta_target`` --
    at the first j with beta(V_n, W_j) >= beta_target.  Raises ValueError for an empty basis or an unknown mode."""
    if mode not in _SENSOR_MODES:
        raise ValueError(f"mode must be one of {sorted(_SENSOR_MODES)}, not {mode!r}")
    n = 0 if basis is None else len(basis)
    if n == 0:
        raise ValueError("sensor selection needs a basis: with n = 0 there is nothing to observe")
    P = np.asarray(candidates, dtype=np.float64).reshape(-1, 2)
    C = _as_device(sm._ctx, basis, sm.vspace_dim)
    picks, crit, A, _, info = sm._fem.sensor_greedy(C.buf, n, *sm._locate(P), int(m), _SENSOR_MODES[mode], rel_tol)
    k = info["picks"]
    beta, k, reached = sensor_beta_prefix(A[:k], n - info["dead_rows"], beta_target)
    stop = "beta_target" if reached else _SENSOR_STOPS[info["stop_reason"]]
    return SensorSelection(P[picks[:k]], picks[:k].copy(), beta, crit[:k].copy(), stop)


# ---- residual error bounds of the Galerkin ROM (rom_resid_*) -----------------------------------------------------------------
class ResidualBound(NamedTuple):
    """``ResidualEstimator.bound`` / ``.curves``: ||r(a)||_{H^-1} and the two sides of
    residual / a_max <= ||u(a) - u_n(a)||_{H^1_0} <= residual / a_min; (M,) arrays, or (N + 1, M) for the curves."""
    residual: np.ndarray
    lower: np.ndarray
    upper: np.ndarray


class ResidualEstimator:
    """A-posteriori error bound of the Galerkin ROM on the rows of ``basis`` for parameters nobody has solved: the H^-1 norm
    of the residual r = f - A(a) u_n from offline quantities of size 1 + k n (k blocks), in the orthonormalised form that
    keeps its accuracy below sqrt(eps) ||f||.  The offline state lives on the device (not picklable; rebuild it from the
    basis).  Effectivity of the upper bound: between 1 and a_max / a_min."""

    def __init__(self, sm: SolutionsManager, basis, n_cap=None):
        self.sm = sm
        n = 0 if basis is None else len(basis)
        self.handle = sm._fem.resid(max(n, n_cap or 0))
        if n:
            self.handle.append(_as_device(sm._ctx, basis, sm.vspace_dim).buf, n)

    @property
    def n(self):
        return self.handle.query()["n"]

    def _eval(self, a, n_values, coefficients=False):
        sm, ctx = self.sm, self.sm._ctx
        a = sm._a_batch(a)
        M = a.shape[0]
        res = np.zeros((len(n_values), M))
        coefs = []
        if M:
            a_dev, D = ctx.upload(a), ctx.alloc(M)
            for i, n in enumerate(n_values):
                Cf = ctx.alloc(max(M * n, 1)) if coefficients else None
                self.handle.eval(a_dev, M, n, D, COEF=Cf)
                res[i] = D.download(M)
                if coefficients:
                    coefs.append(Cf.download(M * n, shape=(M, n)) if n else np.zeros((M, 0)))
        return a, res, coefs

    def bound(self, a, n=None, return_coefs=False):
        """(||r||_{H^-1}, lower = ||r|| / a_max, upper = ||r|| / a_min) for the parameters ``a`` on the first n rows (default:
        all).  ``return_coefs``: also c (M, n), the coordinates of u_n in the A_1-orthonormal basis (||u_n||_{H^1_0} = ||c||_2)."""
        n = self.n if n is None else int(n)
        a, res, coefs = self._eval(a, [n], coefficients=return_coefs)
        out = ResidualBound(res[0], res[0] / a.max(axis=1), res[0] / a.min(axis=1))
        return (out, coefs[0]) if return_coefs else out

    def curves(self, a):
        """The same for every n = 0 .. N through the nested evaluation: (N + 1, M) arrays."""
        a, res, _ = self._eval(a, list(range(self.n + 1)))
        return ResidualBound(res, res / a.max(axis=1)[None, :], res / a.min(axis=1)[None, :])


class BaseReducedBasis:
    """Container of a reduced basis (rows of ``basis``) and the parameters it came from, with the online
    operations of the reference (:32-98).  Pure host object: picklable, no device state."""

    def __init__(self):
        self.basis = None
        self.a = None
        self.inverse_parameter_estimator = None
        self.linear_parameter_estimator = None

    def build(self, **kwargs):
        raise Exception("Not implemented.")  # (:39-40)

    def set(self, basis, a):
        """(:42-46) install a basis and the two parameter estimators built on its parameters."""
        self.basis, self.a = basis, a
        self.inverse_parameter_estimator = EstimatorInv(a)
        self.linear_parameter_estimator = EstimatorLinear(a)

    # -- sizes -----------------------------------------------------------------------------------------
    @property
    def dim(self):
        return np.shape(self.basis)[0]

    @property
    def ambient_space_dim(self):
        return np.shape(self.basis)[1]

    def __str__(self):
        return type(self).__name__

    def __getitem__(self, item):
        """(:88-92) sub-basis with the same slicing applied to vectors and parameters."""
        sub = BaseReducedBasis()
        sub.set(basis=self.basis[item], a=self.a[item])
        return sub

    # -- online stage: thin wrappers over the solutions manager (GPU) ---------------------------------------
    def forward_modeling(self, sm: SolutionsManager, a: np.ndarray):
        """(:59-60) Galerkin reduced-order solutions for the parameters ``a``."""
        return sm.generate_fm_solutions(a=a, coefficients_rom=self.basis)

    def projection(self, sm: SolutionsManager, true_solutions: np.ndarray):
        """(:62-63) H^1_0-orthogonal projections of ``true_solutions``."""
        return sm.project_solutions(true_solutions, self.basis)

    def coefficient_bounds(self, sm: SolutionsManager, training_solutions, inflate=0.1):
        """(lo, hi) (dim each): the box that the coefficients of the H^1_0 projections of ``training_solutions`` on the basis
        rows span, widened by ``inflate`` times its range (``inverse.coefficient_box``) -- the ``bounds`` of ``state_estimation``
        and ``state_estimation_pbdw``.  The Gram matrix C A_1 C^T and the moments U A_1 C^T are formed on the device."""
        from ..inverse import coefficient_box
        ctx, dim, n = sm._ctx, sm.vspace_dim, self.dim
        C, U = _as_device(ctx, self.basis, dim), _as_device(ctx, training_solutions, dim)
        AC, AV, R = ctx.alloc(n * dim), ctx.alloc(n * n), ctx.alloc(U.rows * n)
        sm._fem.stencil_apply(C.buf, n, AC)
        ctx.gemm_nt(n, n, dim, AC, 0, dim, C.buf, 0, dim, AV, 0, n)
        ctx.gemm_nt(U.rows, n, dim, U.buf, 0, dim, AC, 0, dim, R, 0, n)
        A_V = AV.download(n * n, shape=(n, n))
        coef = np.linalg.solve(0.5 * (A_V + A_V.T), R.download(U.rows * n, shape=(U.rows, n)).T).T
        return coefficient_box(coef, inflate)

    def state_estimation(self, sm: SolutionsManager, measurement_points: np.ndarray, measurements: np.ndarray,
                         return_coefs=False, bounds=None, device=True):
        """(:65-70) fit the basis coefficients to point measurements: the basis is evaluated at the
        measurement points on the device, the (points x n) least-squares problem is solved on the host.
        bounds = (lo, hi) (``coefficient_bounds``): the coefficients stay inside that box -- ``inverse.bounded_lstsq``, on the
        device (``rom_bvls``) or with ``device=False`` on the host; on noisy measurements the unconstrained fit amplifies the
        noise by 1 / sigma_min(E)."""
        E = sm.evaluate_solutions(measurement_points, self.basis)          # (n, points)
        if bounds is not None:
            from ..inverse import bounded_lstsq
            c = np.ascontiguousarray(bounded_lstsq(sm._ctx, E, np.asarray(measurements, dtype=np.float64).reshape(-1, E.shape[1]),
                                                   bounds[0], bounds[1], device=device).c.T)
            estimates = c.T @ np.array(self.basis)
            return (c, estimates) if return_coefs else estimates
        c, *_ = np.linalg.lstsq(E.T, measurements.T, rcond=-1)              # (n, n_measured_states)
        estimates = c.T @ np.array(self.basis)
        return (c, estimates) if return_coefs else estimates

    def state_estimation_pbdw(self, sm: SolutionsManager, measurement_points: np.ndarray, measurements: np.ndarray,
                              return_coefs=False, bounds=None):
        """PBDW state estimation (``pbdw_state_estimation``): the estimates interpolate the measurements and differ from
        the basis span by an H^1_0-orthogonal correction in the span of the sensors' Riesz representers.  c (n, K) as in
        ``state_estimation``, so the parameter estimators accept it unchanged.  bounds = (lo, hi): c stays inside that box."""
        r = pbdw_state_estimation(sm, self.basis, measurement_points, measurements, bounds=bounds)
        return (r.c, r.estimates) if return_coefs else r.estimates

    def pbdw_stability(self, sm: SolutionsManager, measurement_points: np.ndarray):
        """beta_n, n = 1 .. dim: the inf-sup constants of the nested sub-bases self[:n] against the sensor space (the
        PBDW error is at most dist(u, V_n) / beta_n)."""
        _, _, G, L, A_V = _pbdw_operators(sm, self.basis, measurement_points, representers=False)
        return pbdw_solve(G, L, np.zeros((0, G.shape[0])), A_V)[2]

    def select_sensors(self, sm: SolutionsManager, candidates: np.ndarray, m: int, **kw) -> SensorSelection:
        """Greedy PBDW sensor selection for this basis (``select_sensors_pbdw``; mode, beta_target, rel_tol as there)."""
        return select_sensors_pbdw(sm, self.basis, candidates, m, **kw)

    def select_sensors_parameters(self, sm: SolutionsManager, candidates: np.ndarray, m: int, a_library, sigma, **kw):
        """Greedy D-optimal sensor selection for estimating the PARAMETERS with this basis, averaged over ``a_library`` under
        measurement noise ``sigma`` (``inverse.select_sensors_parameters``; prior_cov, weights, subset, rel_tol, device as in
        ``ParameterLibrary.select_sensors``).  Returns a ``SensorDesign``."""
        from ..inverse import select_sensors_parameters
        return select_sensors_parameters(sm, self.basis, a_library, candidates, m, sigma, **kw)

    def error_curves(self, sm: SolutionsManager, true_solutions, a=None, n_max=None):
        """Absolute H^1_0 errors of ``projection`` (and, with the snapshots' parameters ``a``, of ``forward_modeling``)
        on the sub-bases ``self[:n]`` for every n = 0 .. n_max (default: all rows) in one device call; see
        ``SolutionsManager.error_curves``."""
        n_max = self.dim if n_max is None else min(int(n_max), self.dim)
        return sm.error_curves(true_solutions, np.asarray(self.basis)[:n_max], a)

    def error_bound(self, sm: SolutionsManager, a, n=None):
        """Residual bounds of ``forward_modeling`` for the parameters ``a`` without their truth (``ResidualEstimator.bound``
        on the first n rows, default all): (||r||_{H^-1}, lower, upper)."""
        n = self.dim if n is None else min(int(n), self.dim)
        return ResidualEstimator(sm, np.asarray(self.basis)[:n]).bound(a)

    def parameter_estimation_inverse(self, c):
        """(:72-78) harmonic-mean style estimate from the state-estimation coefficients."""
        return self.inverse_parameter_estimator.estimate_parameter(c_values=c)

    def parameter_estimation_linear(self, c):
        """(:80-86) linear estimate from the state-estimation coefficients."""
        return self.linear_parameter_estimator.estimate_parameter(c_values=c)

    def parameter_estimation_library(self, sm: SolutionsManager, measurement_points: np.ndarray, measurements: np.ndarray,
                                     a_library, **kw):
        """Parameters from point measurements by a search over the Galerkin ROM's states for the parameters ``a_library``
        (``rom_nearest``) and a Levenberg-Marquardt polish from the best entries: ``inverse.ParameterLibrary`` -- any basis,
        no amplification by cond(E).  ``kw``: weights (of ``observe``), t, polish, states, max_iter, misfit_tol (of
        ``estimate``).  Returns a ``ParameterEstimate``."""
        from ..inverse import ParameterLibrary
        lib = ParameterLibrary(sm, self.basis, a_library).observe(measurement_points, weights=kw.pop("weights", None))
        return lib.estimate(measurements, **kw)

    def parameter_posterior(self, sm: SolutionsManager, measurement_points: np.ndarray, measurements: np.ndarray, a_library, sigma,
                            **kw):
        """The posterior of log a given point measurements with noise of standard deviation ``sigma``: chains of adaptive
        random-walk Metropolis on the Galerkin ROM from the library rows nearest to the data (``inverse.ParameterLibrary.posterior``,
        ``rom_mcmc``) -- credible intervals next to ``parameter_estimation_library``'s point estimate.  ``kw``: weights (of
        ``observe``), t, steps, burn, thin, seed, states, device (of ``posterior``).  Returns a ``ParameterPosterior``."""
        from ..inverse import ParameterLibrary
        lib = ParameterLibrary(sm, self.basis, a_library).observe(measurement_points, weights=kw.pop("weights", None))
        return lib.posterior(measurements, sigma, **kw)

    def orthonormalize(self):
        """(:94-98) replace the basis by its contrast-sorted Euclidean-orthonormal version."""
        vectors = np.reshape(self.basis, (-1, self.ambient_space_dim))
        self.basis = sort_orthogonalize_base(get_high_contrast_coefficient(self.a), vectors)[1]


class ReducedBasisGreedy(BaseReducedBasis):
    """Strong greedy in relative H^1_0 error (:105-139)."""

    def __init__(self, greedy_for=GREEDY_FOR_GALERKIN):
        self.greedy_for = greedy_for
        self.name = "Greedy " + self.greedy_for
        self.linestyle = "solid" if greedy_for == GREEDY_FOR_H10 else "dashed"
        super().__init__()

    def build(self, n: int, sm: SolutionsManager, solutions2train=None, a2train: List[np.ndarray] = (()),
              solutions2train_h1norm=1, **kwargs):
        if self.greedy_for == GREEDY_FOR_RESIDUAL:
            return self._build_weak(n, sm, a2train, kwargs.get("criterion", "bound"), kwargs.get("rel_tol", 0.0))
        if self.greedy_for not in (GREEDY_FOR_H10, GREEDY_FOR_GALERKIN):
            raise Exception(f"Not implemented greedy for {self.greedy_for}, "
                            f"should be one of [{GREEDY_FOR_H10}, {GREEDY_FOR_GALERKIN}]")
        from ..factored import FactoredSnapshots, greedy_factored
        if isinstance(solutions2train, FactoredSnapshots):
            # training block in factored form: the same greedy in coordinates of the interface vectors
            a2train = np.asarray(a2train)
            self.picks, self.max_errors = greedy_factored(solutions2train, a2train, n,
                                                          self.greedy_for == GREEDY_FOR_GALERKIN,
                                                          solutions2train_h1norm)
            basis = solutions2train.take(self.picks).rows().numpy()
            super().set(basis=basis, a=[a2train[i] for i in self.picks])
            return self
        ctx = sm._ctx
        dim = sm.vspace_dim
        a2train = np.asarray(a2train)
        U = _as_device(ctx, solutions2train, dim)  # training set stays in HBM for the whole build
        M = U.rows
        fs = getattr(U, "factored", None)
        if fs is None and isinstance(solutions2train, np.ndarray) and hasattr(sm, "factored_of_host_rows"):
            # the reference's own pattern: solutions = sm.generate_solutions(a) -> a host array -> build(n, sm, solutions, ...).
            # The manager kept the interface vectors of the arrays it returned; if this is one of them and nobody has written
            # into it (checked bit for bit on the device), the build runs on them
            fs = sm.factored_of_host_rows(solutions2train, U)
        if fs is not None and fs.M == M and (self.greedy_for == GREEDY_FOR_H10 or kwargs.get("galerkin_on_interface_vectors", True)):
            # A block that sm.generate_solutions_device has just produced carries its interface vectors: the greedy runs on
            # them (rom_greedy_factored: M x ~300 numbers per pass instead of M x dim; same picks; H^1_0 curves within 1e-12 of
            # the row path's and 3e-13 of the reference arithmetic's on the same rows: tests/test_gpu_parity.py, C4).  In
            # Galerkin mode two exact fp64 routes differ by contrast x eps; against the 80-bit truth of the reduced systems
            # (tests/referee.py, contrast 1e8) the factored form -- its quadratic forms w_i^T S_b w_j in compensated
            # arithmetic since round 5 -- is 4.5e-10 off, the reference's own arithmetic 6.5e-10, the row form 1.9e-10:
            # build(..., galerkin_on_interface_vectors=False) keeps the rows (65 ms instead of 8 at C4, n = 50).
            self.picks, self.max_errors = greedy_factored(fs, a2train, n, self.greedy_for == GREEDY_FOR_GALERKIN,
                                                          solutions2train_h1norm)
            basis = ctx.alloc(max(len(self.picks) * dim, 1)).gather_rows_from(U.buf, np.asarray(self.picks), dim)
            super().set(basis=DeviceArray(basis, len(self.picks), dim).numpy(), a=[a2train[i] for i in self.picks])
            return self
        # One C call (rom_greedy): the reference re-orthonormalises the contrast-sorted picks from scratch in every
        # iteration (:135-136) and recomputes the approximations of all snapshots (:122/:124); both depend on the SPAN of
        # the basis only, which the library carries as an A_1-orthonormal basis with the projection residuals updated in
        # place -- picks and error curve are the reference's (tests: fixture g6, composition with the projectors).
        galerkin = self.greedy_for == GREEDY_FOR_GALERKIN
        a_dev = ctx.upload(np.ascontiguousarray(a2train, dtype=np.float64).reshape(M, -1)) if galerkin else None
        picks, self.max_errors = sm._fem.greedy(U.buf, M, a_dev, solutions2train_h1norm, galerkin, n)
        self.picks = list(picks)
        if isinstance(solutions2train, DeviceArray):
            basis = ctx.alloc(max(len(picks) * dim, 1)).gather_rows_from(U.buf, np.asarray(picks), dim)
            basis = DeviceArray(basis, len(picks), dim).numpy()
        else:
            basis = np.asarray(solutions2train)[picks].reshape(len(picks), -1)
        super().set(basis=basis, a=[a2train[i] for i in picks])  # raw snapshots in pick order (:138)
        return self


    def _build_weak(self, n, sm, a2train, criterion, rel_tol):
        """Weak greedy on the residual bound (rom_weak_greedy): the training set is the (M, k) parameters alone; n truth
        solves.  criterion "bound" (residual / a_min, the upper bound), "residual", or an array of M weights."""
        ctx, dim = sm._ctx, sm.vspace_dim
        a2train = np.asarray(a2train, dtype=np.float64)
        a = sm._a_batch(a2train)
        M = a.shape[0]
        if isinstance(criterion, str):
            if criterion not in ("bound", "residual"):
                raise ValueError(f"criterion must be 'bound', 'residual' or an array of {M} weights, not {criterion!r}")
            w = 1.0 / a.min(axis=1) if criterion == "bound" else None
        else:
            w = np.ascontiguousarray(np.asarray(criterion, dtype=np.float64).reshape(M))
        n = min(int(n), M)
        resid = sm._fem.resid(n)
        basis = ctx.alloc(max(n * dim, 1))
        picks, crit, info = sm._fem.weak_greedy(ctx.upload(a), M, n, resid, basis, weights=ctx.upload(w) if w is not None else None,
                                                rel_tol=rel_tol)
        resid.free()
        self.picks, self.max_errors, self.info = picks, crit, info
        super().set(basis=DeviceArray(basis, len(picks), dim).numpy(), a=[a2train[i] for i in picks])
        return self


def get_inf_solutions_starting_basis(solutions2train, a2train, only_one_block=True):
    """(:142-150) peel off the snapshots that have blocks exactly at INFINIT_A (exactly one such block, or
    any number, per the flag).  Returns (chosen solutions, chosen a, remaining solutions, remaining a)."""
    a2train, solutions2train = np.asarray(a2train), np.asarray(solutions2train)
    n_inf = (a2train == INFINIT_A).reshape(len(a2train), -1).sum(axis=1)
    chosen = (n_inf == 1) if only_one_block else (n_inf > 0)
    return solutions2train[chosen], a2train[chosen], solutions2train[~chosen], a2train[~chosen]


def get_starting_basis(solutions2train, a2train, add_inf_solutions=True):
    """(:153-164) the INFINIT_A snapshots always leave the pool; they lead the basis only on request."""
    lead, lead_a, pool, pool_a = get_inf_solutions_starting_basis(solutions2train, a2train, only_one_block=False)
    if not add_inf_solutions:
        lead, lead_a = np.empty((0, pool.shape[1])), np.empty((0,) + pool_a.shape[1:])
    return lead, lead_a, pool, pool_a


class ReducedBasisRandom(BaseReducedBasis):
    """(:167-180) seeded random snapshots behind the optional INFINIT_A lead -- host indexing only."""

    def __init__(self, add_inf_solutions=True):
        self.add_inf_solutions = add_inf_solutions
        self.name = "Random" + (r" $\infty$" if add_inf_solutions else "")
        super().__init__()

    def build(self, n: int, sm: SolutionsManager, solutions2train, a2train: List[np.ndarray] = (()),
              solutions2train_h1norm=1, seed=42, **kwargs):
        lead, lead_a, pool, pool_a = get_starting_basis(solutions2train, a2train, self.add_inf_solutions)
        np.random.seed(seed)
        picked = np.random.choice(len(pool), size=n, replace=False)
        self.set(basis=np.vstack((lead, pool[picked]))[:n], a=np.vstack((lead_a, pool_a[picked]))[:n])
        return self


_pod_warned = set()


def warn_completed_modes(info, n, rel_floor):
    """One warning per process and message when a POD call completed modes the data do not determine (pod_modes and
    pod_modes_factored alike), with the reason the C call reported."""
    floor = max(rel_floor, 1e-13)
    if info["stop_reason"] == "budget":
        msg = (f"POD: {info['completed_modes']} of the {n} requested modes were NOT found although the spectrum had not "
               f"reached the floor ({floor:g} sigma_1): a sketch pass accepted nothing; completed with orthonormal "
               "directions of zero singular value")
    else:
        msg = (f"POD: {info['completed_modes']} of the {n} requested modes lie below the floor of the snapshot block (sigma < "
               f"{floor:g} sigma_1" + ("" if rel_floor > 1e-13 else ": fp64 noise of the data") + "); completed with "
               "orthonormal directions of zero singular value")
    if msg not in _pod_warned:  # (once per process and message: a bench calls this a dozen times on the same block)
        _pod_warned.add(msg)
        warning(msg)


def pod_modes(ctx: _ffi.Context, X: DeviceArray, n: int, center=True, rel_floor=0.0, download=True):
    """Leading ``n`` right singular vectors / singular values of the (M, dim) snapshot block: one C call (rom_pod).

    Randomised range-finder passes over the implicitly deflated block (four thin GEMMs each, one power step, the rows
    orthonormalised on both sides of it: a pass resolves modes over seven orders of magnitude to LAPACK's own bound
    eps sigma_1 / sigma) with a convergence rule per pass; a spectrum that decays too slowly for that -- the first pass
    says so -- gets its leading modes from the MFMA Gram matrix ``G = Xc Xc^T`` instead (eigenpairs iterated in M space,
    modes with lambda_k > 1e-10 lambda_1) and the passes go on below; until the request is filled or the spectrum has
    reached the fp64 noise of the snapshots (1e-13 sigma_1); a Rayleigh-Ritz step over the collected modes orders them.  What is still missing
    then does not exist in the data; like LAPACK / scikit-learn, which return SOME orthonormal directions there, the
    basis is completed with orthonormalised pseudo-random directions (singular value 0, seeded by the number of
    resolved modes: deterministic), so the rows returned are always orthonormal.  Rows follow scikit-learn's
    ``svd_flip(u_based_decision=False)`` sign convention (the PCA call at src/lib/ReducedBasis.py:196).  X is
    overwritten.  ``pod_modes.last_info``: flop accounting and pass counts of the call.  ``rel_floor``: do not look for
    modes below that fraction of sigma_1 (rom_pod_ex; default: the fp64 noise floor of the block, 1e-13).
    ``download=False`` returns the modes as a DeviceArray."""
    M, dim = X.rows, X.dim
    n = min(n, M, dim)
    V = ctx.alloc(max(n * dim, 1))
    X.factored = None  # (the rows are about to be centred in place: they stop being the image of their interface vectors)
    try:
        sig, info = ctx.pod(X.buf, M, dim, n, V, center=center, rel_floor=rel_floor)
    except _ffi.RomLibraryError as e:
        if "NaN / Inf" in str(e) or "rescale the block" in str(e):   # (scikit-learn's PCA raises ValueError on such input)
            raise ValueError(str(e)) from None
        raise
    pod_modes.last_info = info
    pod_modes.resolved = info["resolved_modes"]
    if info["completed_modes"]:
        warn_completed_modes(info, n, rel_floor)
    elif info["stop_reason"] == "budget":
        warning("POD: the eigenpairs of the Gram matrix did not converge (a spectrum so flat that the subspace iteration "
                f"stalls, with more than 1024 snapshots: M = {M}); the trailing modes of the request are approximate")
    if n == 0:
        return (np.zeros((0, dim)) if download else DeviceArray(V, 0, dim)), sig
    return (V.download(n * dim, shape=(n, dim)) if download else DeviceArray(V, n, dim)), sig


def pod_modes_h10(sm: SolutionsManager, X: DeviceArray, n: int, center=True, rel_floor=0.0, download=True):
    """Leading ``n`` modes / singular values of the (M, dim) snapshot block in the H^1_0 inner product: one C call
    (rom_pod_h10).  The n-dimensional space that minimises sum_m ||u_m - P_n u_m||^2_{H^1_0} -- the lower envelope of the
    mean-square curves of ``error_curves`` -- where ``pod_modes`` minimises the Euclidean sum (the reference's notebook:
    "PCA (optimal with respect to L2)").  The block goes to the coordinates in which the H^1_0 inner product is Euclidean
    (the 2-D sine transform that diagonalises A_1, on MFMA), ``rom_pod_ex`` runs there with its full range, and the modes
    come back A_1-orthonormal; singular values are those of the block in the H^1_0 geometry.  The contract of ``pod_modes``
    (completion below the floor with its warning, sign rule on the returned rows, ``pod_modes_h10.last_info``), except that
    ``X`` -- and ``X.factored`` -- are left untouched: the centring happens in the transformed copy."""
    M, dim = X.rows, X.dim
    assert dim == sm.vspace_dim, "pod_modes_h10: rows of the manager's FE space"
    n = min(n, M, dim)
    ctx = sm._ctx
    V = ctx.alloc(max(n * dim, 1))
    try:
        sig, info = sm._fem.pod_h10(X.buf, M, n, V, center=center, rel_floor=rel_floor)
    except _ffi.RomLibraryError as e:
        if "NaN / Inf" in str(e) or "rescale the block" in str(e):   # (as pod_modes)
            raise ValueError(str(e)) from None
        raise
    pod_modes_h10.last_info = info
    pod_modes_h10.resolved = info["resolved_modes"]
    if info["completed_modes"]:
        warn_completed_modes(info, n, rel_floor)
    elif info["stop_reason"] == "budget":
        warning("POD: the eigenpairs of the Gram matrix did not converge (a spectrum so flat that the subspace iteration "
                f"stalls, with more than 1024 snapshots: M = {M}); the trailing modes of the request are approximate")
    if n == 0:
        return (np.zeros((0, dim)) if download else DeviceArray(V, 0, dim)), sig
    return (V.download(n * dim, shape=(n, dim)) if download else DeviceArray(V, n, dim)), sig


PCA_INNER_L2 = "l2"
PCA_INNER_H10 = "h10"


class ReducedBasisPCA(BaseReducedBasis):
    """(:183-200) mean-centred PCA of the training snapshots (INFINIT_A ones peeled off first).  ``inner_product="h10"``:
    the POD in the H^1_0 inner product (``pod_modes_h10`` / ``pod_modes_factored(inner="h10")``), the basis that is optimal
    in the norm the errors are reported in; the default is the reference's Euclidean PCA."""

    def __init__(self, add_inf_solutions=True, inner_product=PCA_INNER_L2):
        self.add_inf_solutions = add_inf_solutions
        self.inner_product = inner_product
        self.name = ("PCA $H^1_0$" if inner_product == PCA_INNER_H10 else "PCA") + (r" $\infty$" if add_inf_solutions else "")
        super().__init__()

    def build(self, n: int, sm: SolutionsManager, solutions2train, a2train: List[np.ndarray] = (()),
              solutions2train_h1norm=1, add_inf_solutions=True, seed=42, **kwargs):
        from ..factored import FactoredSnapshots, pod_modes_factored
        if self.inner_product not in (PCA_INNER_L2, PCA_INNER_H10):
            raise Exception(f"Not implemented PCA for the inner product {self.inner_product}, "
                            f"should be one of [{PCA_INNER_L2}, {PCA_INNER_H10}]")
        h10 = self.inner_product == PCA_INNER_H10
        if isinstance(solutions2train, FactoredSnapshots):
            # the training block in factored form (e.g. gathered from several GPUs): the same peel-off of the
            # INFINIT_A snapshots by index, POD on the interface vectors, only the basis rows are materialised
            fs, a2train = solutions2train, np.asarray(a2train)
            has_inf = (a2train == INFINIT_A).reshape(len(a2train), -1).any(axis=1)
            lead_idx = np.flatnonzero(has_inf) if self.add_inf_solutions else np.zeros(0, dtype=np.int64)
            pool = fs.take(np.flatnonzero(~has_inf))
            comps, sigma = pod_modes_factored(pool, n, inner="h10") if h10 else pod_modes_factored(pool, n)
            self.singular_values_ = sigma
            self.resolved_modes_ = pod_modes_factored.last_info.get("resolved_modes", n)
            lead = fs.take(lead_idx).rows().numpy() if lead_idx.size else np.empty((0, sm.vspace_dim))
            super().set(basis=np.vstack((lead, comps))[:n], a=np.vstack((a2train[lead_idx], a2train[~has_inf]))[:n])
            return self
        if isinstance(solutions2train, DeviceArray):
            # the training block is resident in HBM: the INFINIT_A snapshots are peeled off BY INDEX on the device
            # (get_starting_basis, :153-164, does it on host rows), the pool is gathered into the private copy that rom_pod
            # overwrites, and only the basis rows ever cross PCIe
            Ud, a2 = solutions2train, np.asarray(a2train)
            if getattr(Ud, "factored", None) is not None and Ud.factored.M == Ud.rows:
                # fresh from sm.generate_solutions_device: the block's interface vectors are at hand -- the PCA of the rows IS
                # the PCA of their energy coordinates (rom_pod_factored: same modes, a matrix dim / ~300 times narrower)
                return self.build(n, sm, Ud.factored, a2, solutions2train_h1norm, **kwargs)
            ctx, dim = sm._ctx, Ud.dim
            has_inf = (a2 == INFINIT_A).reshape(len(a2), -1).sum(axis=1) > 0
            pool_idx = np.flatnonzero(~has_inf)
            lead_idx = np.flatnonzero(has_inf) if self.add_inf_solutions else np.zeros(0, dtype=np.int64)
            X = ctx.alloc(max(len(pool_idx) * dim, 1)).gather_rows_from(Ud.buf, pool_idx, dim)
            if h10:
                comps, sigma = pod_modes_h10(sm, DeviceArray(X, len(pool_idx), dim), n, center=True)
            else:
                comps, sigma = pod_modes(ctx, DeviceArray(X, len(pool_idx), dim), n, center=True)
            self.singular_values_ = sigma
            self.resolved_modes_ = pod_modes_h10.resolved if h10 else pod_modes.resolved
            if lead_idx.size:
                lead = DeviceArray(ctx.alloc(lead_idx.size * dim).gather_rows_from(Ud.buf, lead_idx, dim), lead_idx.size, dim).numpy()
            else:
                lead = np.empty((0, dim))
            super().set(basis=np.vstack((lead, comps))[:n], a=np.vstack((a2[lead_idx].reshape((-1,) + a2.shape[1:]), a2[pool_idx]))[:n])
            warning("PCA method has not been adapted for inverse parameter estimation, the a coefficients are not correct.")
            return self
        basis, a, solutions2train, a2train = get_starting_basis(solutions2train, a2train, self.add_inf_solutions)
        ctx = sm._ctx
        X = _as_device(ctx, np.array(solutions2train, dtype=np.float64), sm.vspace_dim)  # private copy
        comps, sigma = pod_modes_h10(sm, X, n, center=True) if h10 else pod_modes(ctx, X, n, center=True)
        self.singular_values_ = sigma
        self.resolved_modes_ = pod_modes_h10.resolved if h10 else pod_modes.resolved  # modes above the fp64 noise floor of the block (the rest: see pod_modes)
        super().set(basis=np.vstack((basis, comps))[:n], a=np.vstack((a, a2train))[:n])
        warning("PCA method has not been adapted for inverse parameter estimation, the a coefficients are not correct.")
        return self


# ---- full PCA of a tall block (M >> dim): rom_pca_tall ---------------------------------------------------------------------
class TallPCA:
    """Result of ``pca_tall``, with scikit-learn's attribute names: ``components_`` (n, dim), ``singular_values_`` (n,),
    ``explained_variance_`` = sigma^2 / (M - 1), ``explained_variance_ratio_``, ``mean_`` (dim,), ``n_samples_``,
    ``n_components_``; and ``resolved_modes_`` (modes above 1e-13 sigma_1: what the fp64 data determine), ``scores`` (M, n)
    = ``pca.transform`` of the training block (a DeviceArray with ``download=False``, None when not asked for), ``info``
    (pass and flop counts of the call).  ``explained_variance_ratio_`` is taken over the modes returned: scikit-learn's
    ratio for n = dim (what ``do_pca`` asks for); for n < dim the variance of the modes left out is not in it."""

    def __init__(self, components, singular_values, mean, n_samples, resolved_modes, scores=None, info=None, ctx=None):
        self.components_ = components
        self.singular_values_ = np.asarray(singular_values, dtype=np.float64)
        self.mean_ = mean
        self.n_samples_ = int(n_samples)
        self.n_components_ = len(self.singular_values_)
        self.resolved_modes_ = int(resolved_modes)
        self.scores = scores
        self.info = dict(info or {})
        self._ctx = ctx

    @property
    def explained_variance_(self):
        return self.singular_values_ ** 2 / max(self.n_samples_ - 1, 1)

    @property
    def explained_variance_ratio_(self):
        ev = self.explained_variance_
        total = float(ev.sum())
        return ev / total if total > 0.0 else np.zeros_like(ev)

    def transform(self, Y, download=True):
        """Scores of new rows: (Y - mean_) components_^T, centred and multiplied (rom_gemm_nt) on the device."""
        ctx = self._ctx if self._ctx is not None else _ffi.get_context()
        n = self.n_components_
        comps = self.components_
        dim = comps.dim if isinstance(comps, DeviceArray) else np.shape(comps)[1]
        if isinstance(Y, DeviceArray):   # a private copy: the caller's rows stay as they are
            Yd = DeviceArray(ctx.alloc(max(Y.rows * dim, 1)).copy_from(Y.buf, Y.rows * dim), Y.rows, dim)
        else:
            Yd = _as_device(ctx, np.array(Y, dtype=np.float64), dim)
        K = Yd.rows
        if K == 0 or n == 0:
            return np.zeros((K, n)) if download else DeviceArray(ctx.alloc(1), K, n)
        Vd = comps if isinstance(comps, DeviceArray) else _as_device(ctx, comps, dim)
        mean = self.mean_.numpy().ravel() if isinstance(self.mean_, DeviceArray) else np.asarray(self.mean_, dtype=np.float64)
        if mean.any():
            ctx.gemm_nn(K, dim, 1, ctx.upload(np.ones(K)), 0, 1, ctx.upload(mean), 0, dim, Yd.buf, 0, dim, alpha=-1.0, beta=1.0)
        S = ctx.alloc(K * n)
        ctx.gemm_nt(K, n, dim, Yd.buf, 0, dim, Vd.buf, 0, dim, S, 0, n)
        return S.download(K * n, shape=(K, n)) if download else DeviceArray(S, K, n)


_pca_tall_warned = set()


def pca_tall(ctx: _ffi.Context, X, n=None, center=True, scores=True, download=True) -> TallPCA:
    """Full PCA of a TALL block, M >> dim <= 1024 (``PCA(n).fit`` + ``.transform``, the reference's
    src/experiments/NonLinearROM.py:34-41): one C call (rom_pca_tall).

    Block one-sided Jacobi on Gram matrices of the ROTATED DATA (Y = Xc V^T, G = Y^T Y on MFMA, Jacobi of G with the
    relative stopping rule, V <- Q^T V; three passes over the block are typical): singular values and scores are accurate
    relative to each mode over the whole fp64 range, where a one-pass covariance eigendecomposition (what scikit-learn
    picks for this shape) stops at sqrt(eps) sigma_1.  All ``n`` rows returned belong to one complete orthonormal basis;
    nothing is completed with random directions.  ``n`` defaults to ``dim``.  A DeviceArray ``X`` is overwritten when
    ``center`` (the column means are subtracted in place); a host array is uploaded into a private copy."""
    if isinstance(X, DeviceArray):
        Xd = X
        if center:
            Xd.factored = None   # (centred in place: the rows stop being the image of their interface vectors)
    else:
        arr = np.array(X, dtype=np.float64)
        assert arr.ndim == 2, "pca_tall: a (M, dim) block"
        Xd = _as_device(ctx, arr, arr.shape[1])
    M, dim = Xd.rows, Xd.dim
    n = dim if n is None else int(n)
    V = ctx.alloc(max(n * dim, 1))
    S = ctx.alloc(max(M * n, 1)) if scores else None
    mean = ctx.alloc(dim)
    try:
        sig, info = ctx.pca_tall(Xd.buf, M, dim, n, V, S=S, mean=mean, center=center)
    except _ffi.RomLibraryError as e:
        if "NaN / Inf" in str(e) or "rescale the block" in str(e):   # (scikit-learn's PCA raises ValueError on such input)
            raise ValueError(str(e)) from None
        raise
    if n > info["resolved_modes"]:
        msg = (f"PCA: {n - info['resolved_modes']} of the {n} requested modes lie below the floor of the snapshot block "
               f"(sigma < 1e-13 sigma_1: fp64 noise of the data): resolved_modes_ = {info['resolved_modes']}; the rows past "
               "them are orthonormal directions measured at noise level, not determined by the data")
        if msg not in _pca_tall_warned:
            _pca_tall_warned.add(msg)
            warning(msg)
    if info["stop_reason"] != "converged":
        warning(f"PCA: the rotations had not converged after {info['passes']} passes over the block (largest off-diagonal "
                f"{info['worst_ratio']:.3g} x its tolerance)")
    if download:
        comps = V.download(n * dim, shape=(n, dim)) if n else np.zeros((0, dim))
        sc = (S.download(M * n, shape=(M, n)) if n else np.zeros((M, 0))) if scores else None
        mu = mean.download(dim)
    else:
        comps, mu = DeviceArray(V, n, dim), DeviceArray(mean, 1, dim)
        sc = DeviceArray(S, M, n) if scores else None
    return TallPCA(comps, sig, mu, M, info["resolved_modes"], scores=sc, info=info, ctx=ctx)


# ---- clustered local bases (romhighcontrast_amd/local.py), exported beside the global ones ---------------------------------
from ..local import KMeans, LocalReducedBasis  # noqa: E402,F401
