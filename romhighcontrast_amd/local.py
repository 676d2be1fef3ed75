"""Local reduced bases: the parameter domain is split by k-means and every part gets its own small POD basis (hp-RB: Eftang,
Patera, Ronquist; Amsallem, Zahr, Farhat).  The other standard answer -- beside the curved charts of ``nonlinear.py`` -- to a
slowly decaying Kolmogorov width: a local basis of dimension n reaches the error of a global one of 2 - 4 times the dimension
in the pre-asymptotic range, and the online reduced solve costs n^3 per parameter.  The gain shrinks once n reaches the
effective dimension of the manifold.

``kmeans_host`` / ``maximin_rows_host`` are the NumPy specification of ``rom_kmeans_fit`` / ``rom_kmeans_init_maximin`` (the same
rules: the total order (dist2, centroid index), empty clusters kept where they are, the stop rules, the final assignment);
``KMeans`` is the estimator on the device and ``LocalReducedBasis`` the clustered POD bases with the online operations of
``BaseReducedBasis``.

When the parameter is the unknown -- state estimation from point sensors -- the cluster cannot be looked up:
``LocalReducedBasis.observe`` fixes the sensors and returns a ``LocalSensing``, whose ``estimate`` computes the linear estimate in
every local space and keeps the one whose PDE residual, minimised over the cluster's parameter box, is smallest (Cohen, Dahmen,
Mula, Nichols, SIAM/ASA JUQ 10, 2022; ``rom_local_select``, specification ``inverse.local_select_host``)."""
from __future__ import annotations

from logging import warning
from typing import NamedTuple

import numpy as np

__all__ = ["kmeans_host", "maximin_rows_host", "dist2_host", "KMeansHostResult", "KMeans", "LocalReducedBasis", "LocalSensing",
           "LocalEstimate"]


# ---- the NumPy specification ------------------------------------------------------------------------------------------------
def dist2_host(X, C):
    """(M, kc) squared distances sum_c (x_c - c_c)^2 from the original operands, differences first, columns in order (one rounding
    more per term than the device's fma chain)."""
    X, C = np.asarray(X, dtype=np.float64), np.asarray(C, dtype=np.float64)
    D = np.zeros((len(X), len(C)))
    for c in range(X.shape[1]):
        d = X[:, c][:, None] - C[:, c][None, :]
        D = d * d + D
    return D


def _assign_host(X, C):
    D = dist2_host(X, C)
    labels = np.argmin(D, axis=1).astype(np.int32)   # (the first minimum: the smallest (dist2, index))
    return labels, D[np.arange(len(X)), labels]


class KMeansHostResult(NamedTuple):
    centers: np.ndarray          # (kc, r)
    labels: np.ndarray           # (M,) int32, against `centers`
    dist2: np.ndarray            # (M,)
    counts: np.ndarray           # (kc,) int64, of `labels`
    inertia: float               # of `labels`
    inertia_history: np.ndarray  # inertia of the assignment of every iteration
    n_iter: int
    converged: bool
    mu: np.ndarray               # (r,) the shift
    trace: list                  # per iteration (C_t, labels_t, C_t+1): what check_update and the margin condition look at


def kmeans_host(X, init, max_iter=50, tol=0.0) -> KMeansHostResult:
    """Lloyd's algorithm as ``rom_kmeans_fit`` defines it.  Iteration t assigns every row to the centroid of C_t that is smallest
    under (dist2, index) and updates c_j = mu + sum_members (x - mu) / n_j (mu: the column means of X; an empty cluster keeps its
    centroid); it stops when no label changed (converged), when max_j |C_t+1,j - C_t,j|^2 <= tol x (mean column variance), or
    at max_iter.  The result's labels, dist2, counts and inertia come from a final assignment against the returned centroids."""
    X = np.asarray(X, dtype=np.float64)
    C = np.array(init, dtype=np.float64)
    M, r = X.shape
    kc = len(C)
    if C.shape != (kc, r) or M < kc:
        raise ValueError(f"kmeans_host: {M} rows of {r} against initial centroids of shape {C.shape}")
    if not (np.isfinite(X).all() and np.isfinite(C).all()):
        raise ValueError("kmeans_host: NaN / Inf in the block or the initial centroids")
    mu = X.mean(axis=0)
    Xs = X - mu
    meanvar = float((Xs * Xs).sum() / (M * r))
    labels = np.full(M, -1, dtype=np.int32)
    hist, trace, it, converged = [], [], 0, False
    while it < max_iter:
        new, d2 = _assign_host(X, C)
        changed = int((new != labels).sum())
        labels = new
        hist.append(float(d2.sum()))
        Cn = C.copy()
        for j in range(kc):
            members = labels == j
            n = int(members.sum())
            if n:
                Cn[j] = mu + Xs[members].sum(axis=0) / n
        shift = float(((Cn - C) ** 2).sum(axis=1).max())
        trace.append((C, labels.copy(), Cn))
        C = Cn
        it += 1
        if changed == 0:
            converged = True
            break
        if shift <= tol * meanvar:
            break
    labels, d2 = _assign_host(X, C)
    return KMeansHostResult(C, labels, d2, np.bincount(labels, minlength=kc).astype(np.int64), float(d2.sum()), np.array(hist), it,
                            converged, mu, trace)


def maximin_rows_host(X, kc) -> np.ndarray:
    """The deterministic farthest-point start of ``rom_kmeans_init_maximin``: the row nearest to the column means, then always the
    row whose smallest dist2 to the rows chosen so far is largest; the lowest row index among equals."""
    X = np.asarray(X, dtype=np.float64)
    rows = np.zeros(int(kc), dtype=np.int64)
    rows[0] = int(np.argmin(dist2_host(X, X.mean(axis=0)[None, :])[:, 0]))
    D = np.full(len(X), np.inf)
    for s in range(1, int(kc)):
        D = np.minimum(D, dist2_host(X, X[rows[s - 1]][None, :])[:, 0])
        rows[s] = int(np.argmax(D))
    return rows


# ---- the estimator ----------------------------------------------------------------------------------------------------------------
class KMeans:
    """k-means on the device (rom_kmeans_*) with scikit-learn's attribute names: ``labels_``, ``cluster_centers_``, ``counts_``,
    ``inertia_``, ``inertia_history_``, ``n_iter_``, ``converged_``.  ``init``: "maximin" (the deterministic farthest-point
    start), row indices (kc,) or a (kc, r) array.  ``fit`` / ``predict`` take host arrays or DeviceArrays; ``fit_columns`` a
    column range of a DeviceArray, as ``PolynomialMap``.  An empty cluster stays where it is and is reported with a warning.
    Pickles without its device handle, which is rebuilt from the centroids on first use."""

    def __init__(self, n_clusters, init="maximin", max_iter=50, tol=0.0, ctx=None):
        self.n_clusters, self.init, self.max_iter, self.tol = int(n_clusters), init, int(max_iter), float(tol)
        self._ctx = ctx
        self.handle_ = None
        self.cluster_centers_ = None

    def _context(self):
        from . import _ffi
        if self._ctx is None:
            self._ctx = _ffi.get_context()
        return self._ctx

    def _device(self, X):
        from .lib.SolutionsManagers import DeviceArray
        if isinstance(X, DeviceArray):
            return X
        arr = np.ascontiguousarray(np.asarray(X, dtype=np.float64))
        arr = arr.reshape(len(arr), -1)
        return DeviceArray(self._context().upload(arr), arr.shape[0], arr.shape[1])

    def __getstate__(self):
        d = dict(self.__dict__)
        d["_ctx"] = None
        d["handle_"] = None
        return d

    # -- fitting ----------------------------------------------------------------------------------------------------------------
    def fit(self, X):
        Xd = self._device(X)
        return self.fit_columns(Xd, (0, Xd.dim), 0, Xd.rows)

    def fit_columns(self, Xd, cols, row0, rows):
        """Fit on rows [row0, row0 + rows) of the column range cols = (lo, hi) of the DeviceArray Xd: nothing is copied."""
        from . import _ffi
        ctx, kc, r = self._context(), self.n_clusters, cols[1] - cols[0]
        _ffi.kmeans_layout(r, kc)
        off = row0 * Xd.dim + cols[0]
        if isinstance(self.init, str):
            if self.init != "maximin":
                raise ValueError(f"KMeans: init = {self.init!r}, 'maximin', row indices or a (kc, r) array")
            init = ctx.kmeans_init_maximin(Xd.buf, off, Xd.dim, r, rows, kc)
        else:
            init = np.asarray(self.init)
        if init.ndim == 1:
            idx = init.astype(np.int64)
            if idx.shape != (kc,) or (idx < 0).any() or (idx >= rows).any():
                raise ValueError(f"KMeans: {kc} initial rows inside [0, {rows}) expected")
            G = ctx.alloc(kc * Xd.dim).gather_rows_from(Xd.buf, row0 + idx, Xd.dim)
            init = G.download(kc * Xd.dim, shape=(kc, Xd.dim))[:, cols[0]:cols[1]]
        self.handle_ = ctx.kmeans_fit(Xd.buf, off, Xd.dim, r, rows, kc, init, self.max_iter, self.tol)
        return self._collect()

    def fit_host(self, X):
        """The same estimator from the NumPy specification (no device): ``kmeans_host`` / ``maximin_rows_host``."""
        X = np.asarray(X, dtype=np.float64)
        X = X.reshape(len(X), -1)
        init = maximin_rows_host(X, self.n_clusters) if isinstance(self.init, str) else np.asarray(self.init)
        if init.ndim == 1:
            init = X[init.astype(np.int64)]
        res = kmeans_host(X, init, self.max_iter, self.tol)
        self.handle_ = None
        self.cluster_centers_, self.labels_, self.counts_, self.mu_ = res.centers, res.labels, res.counts, res.mu
        self.inertia_, self.inertia_history_, self.n_iter_, self.converged_ = res.inertia, res.inertia_history, res.n_iter, res.converged
        self.info_ = {}
        return self._warn_empty()

    def _collect(self):
        h = self.handle_
        self.info_ = h.info
        self.cluster_centers_, self.counts_, self.labels_ = h.download("centroids"), h.download("counts"), h.download("labels")
        hist = h.download("inertia")
        self.mu_ = h.download("shift")
        self.inertia_, self.inertia_history_ = float(hist[-1]), hist[:-1]
        self.n_iter_, self.converged_ = h.info["iterations"], h.info["converged"]
        return self._warn_empty()

    def _warn_empty(self):
        empty = np.flatnonzero(self.counts_ == 0)
        if empty.size:
            warning(f"KMeans: {empty.size} of the {self.n_clusters} clusters are empty ({empty[:8].tolist()}); their centroids stay "
                    "where they were")
        return self

    # -- prediction -------------------------------------------------------------------------------------------------------------
    def _handle(self):
        """The device handle.  After unpickling (or ``fit_host``) it is rebuilt with max_iter = 0, which keeps the centroids bit
        for bit, on the centroids themselves as the block: the shift then is their mean, not the training block's -- it only
        steers the screen, never the labels or distances."""
        if self.handle_ is None:
            assert self.cluster_centers_ is not None, "KMeans.predict before fit"
            ctx, C = self._context(), np.ascontiguousarray(self.cluster_centers_)
            self.handle_ = ctx.kmeans_fit(ctx.upload(C), 0, C.shape[1], C.shape[1], C.shape[0], C.shape[0], C, max_iter=0)
        return self.handle_

    def predict(self, X, return_dist2=False):
        Xd = self._device(X)
        labels, d2, _ = self._handle().assign(Xd.buf, 0, Xd.dim, Xd.rows, dist2=return_dist2)
        return (labels, d2) if return_dist2 else labels


# ---- clustered local POD bases --------------------------------------------------------------------------------------------------
class LocalReducedBasis:
    """One POD basis per cluster of the parameter domain.  ``build`` clusters the features of the training parameters (log a
    flattened, or caller-supplied rows), gathers each cluster's snapshots on the device and runs ``pod_modes_h10`` /
    ``pod_modes`` on them; ``classify`` sends new parameters to their clusters (rom_kmeans_assign), ``forward_modeling`` and
    ``projection`` run the existing operators per cluster on the member rows and return the rows in input order.  ``bases``:
    one ``BaseReducedBasis`` per cluster, ``kmeans``: the fitted ``KMeans``, ``labels_``: the clusters of the training rows."""

    def __init__(self, n_clusters, inner_product="h10", center=False, features="log_a", max_iter=50):
        if inner_product not in ("h10", "l2"):
            raise ValueError(f"LocalReducedBasis: inner_product = {inner_product!r}, 'h10' or 'l2'")
        if features != "log_a":
            raise ValueError(f"LocalReducedBasis: features = {features!r}; 'log_a', or pass the rows to build / classify")
        self.n_clusters, self.inner_product, self.center, self.features, self.max_iter = int(n_clusters), inner_product, bool(center), \
            features, int(max_iter)
        self.kmeans, self.bases, self.labels_ = None, [], None
        self.name = f"Local PCA ({n_clusters})" + (" $H^1_0$" if inner_product == "h10" else "")

    def __str__(self):
        return type(self).__name__

    @staticmethod
    def _features(a, features):
        from .lib.SolutionsManagers import DeviceArray
        if features is not None:
            return features if isinstance(features, DeviceArray) else np.asarray(features, dtype=np.float64).reshape(len(features), -1)
        a = np.asarray(a, dtype=np.float64)
        return np.log(a.reshape(len(a), -1))

    def build(self, n: int, sm, solutions2train, a2train, features=None, **kwargs):
        """Cluster, then one POD per cluster.  For ``observe`` it also stores, per cluster, the parameter ranges (``a_ranges_``,
        ``a_range_``) and the box its training snapshots span in the A_1-orthonormal basis of its modes
        (``coefficient_boxes_``): one ``ResidualEstimator``, one stencil application and one GEMM per cluster, paid by every
        ``build`` (None for a centred basis, which ``observe`` refuses)."""
        from .factored import FactoredSnapshots
        from .lib.ReducedBasis import BaseReducedBasis, pod_modes, pod_modes_h10
        from .lib.SolutionsManagers import DeviceArray, _as_device
        if isinstance(solutions2train, FactoredSnapshots):
            raise TypeError("LocalReducedBasis.build takes the snapshot rows (a host array or a DeviceArray); a FactoredSnapshots "
                            "block is not supported: pass its rows()")
        ctx, dim = sm._ctx, sm.vspace_dim
        Ud = _as_device(ctx, solutions2train, dim)
        a2 = np.asarray(a2train, dtype=np.float64)
        F = self._features(a2, features)
        assert len(F) == Ud.rows, "LocalReducedBasis.build: one feature row per snapshot"
        self.kmeans = KMeans(self.n_clusters, max_iter=self.max_iter, ctx=ctx).fit(F)
        self.labels_ = self.kmeans.labels_
        self.bases, self.singular_values_, self.coefficient_boxes_ = [], [], []
        a_flat = a2.reshape(len(a2), -1)
        self.a_range_ = (a_flat.min(axis=0), a_flat.max(axis=0))          # the box of all training parameters, per block
        self.a_ranges_ = []                                              # and of every cluster's
        for j in range(self.n_clusters):
            idx = np.flatnonzero(self.labels_ == j)
            if idx.size < n + 1:
                raise ValueError(f"LocalReducedBasis.build: cluster {j} has {idx.size} rows, a basis of dimension {n} needs at least "
                                 f"{n + 1}; use fewer clusters or more training rows")
            X = DeviceArray(ctx.alloc(idx.size * dim).gather_rows_from(Ud.buf, idx, dim), idx.size, dim)   # (private copy)
            if self.inner_product == "h10":
                comps, sigma = pod_modes_h10(sm, X, n, center=self.center)
            else:
                comps, sigma = pod_modes(ctx, X, n, center=self.center)
            rb = BaseReducedBasis()
            rb.set(basis=comps, a=a2[idx][:n])   # (as ReducedBasisPCA: the parameters are not those of the modes)
            self.bases.append(rb)
            self.singular_values_.append(sigma)
            self.a_ranges_.append((a_flat[idx].min(axis=0), a_flat[idx].max(axis=0)))
            self.coefficient_boxes_.append(None if self.center else self._training_box(sm, comps, X))
        return self

    @staticmethod
    def _training_box(sm, comps, X):
        """``coefficient_box`` of the coordinates X A_1 W^T of the cluster's snapshots X in the A_1-orthonormal basis W that a
        residual estimator builds on ``comps`` (the coordinates ``LocalSensing`` works in); None when ``comps`` has dead rows."""
        from .inverse import coefficient_box
        from .lib.ReducedBasis import ResidualEstimator
        ctx, dim, n = sm._ctx, sm.vspace_dim, len(comps)
        est = ResidualEstimator(sm, comps)
        try:
            if est.handle.download("dead").any():
                return None
            Wd, AW, Cf = ctx.alloc(n * dim), ctx.alloc(n * dim), ctx.alloc(X.rows * n)
            est.handle.basis(Wd)
            sm._fem.stencil_apply(Wd, n, AW)
            ctx.gemm_nt(X.rows, n, dim, X.buf, 0, dim, AW, 0, dim, Cf, 0, n)
            return coefficient_box(Cf.download(X.rows * n, shape=(X.rows, n)))
        finally:
            est.handle.free()

    def classify(self, a=None, features=None) -> np.ndarray:
        """The cluster of every parameter (or feature row): (M,) int32."""
        assert self.kmeans is not None, "LocalReducedBasis.classify before build"
        return self.kmeans.predict(self._features(a, features))

    def _per_cluster(self, sm, labels, run):
        """run(j, idx) -> DeviceArray of the member rows idx of cluster j; the results concatenated in cluster order and brought
        back to input order by one gather with the inverse permutation."""
        from .lib.SolutionsManagers import DeviceArray
        ctx, dim, M = sm._ctx, sm.vspace_dim, len(labels)
        cat = ctx.alloc(max(M * dim, 1))
        order, at = [], 0
        for j in range(self.n_clusters):
            idx = np.flatnonzero(labels == j)
            if idx.size == 0:
                continue
            part = run(j, idx)
            cat.copy_from(part.buf, idx.size * dim, dst_off=at * dim)
            order.append(idx)
            at += idx.size
        out = ctx.alloc(max(M * dim, 1))
        if M:
            inverse = np.empty(M, dtype=np.int64)
            inverse[np.concatenate(order)] = np.arange(M)
            out.gather_rows_from(cat, inverse, dim)
        return DeviceArray(out, M, dim)

    def forward_modeling(self, sm, a, features=None):
        """Galerkin reduced-order solutions for the parameters ``a``, each on the basis of its cluster; rows in input order."""
        a2 = sm._a_batch(a)
        labels = self.classify(a2, features)
        res = self._per_cluster(sm, labels, lambda j, idx: sm.generate_fm_solutions_device(a2[idx], self.bases[j].basis))
        return res.numpy()

    def projection(self, sm, true_solutions, a, features=None):
        """H^1_0-orthogonal projections of ``true_solutions`` onto the basis of each row's cluster; host rows in give host rows
        out, a DeviceArray gives a DeviceArray."""
        from .lib.SolutionsManagers import DeviceArray, _as_device
        ctx, dim = sm._ctx, sm.vspace_dim
        Ud = _as_device(ctx, true_solutions, dim)
        labels = self.classify(sm._a_batch(a) if features is None else None, features)
        assert len(labels) == Ud.rows, "LocalReducedBasis.projection: one parameter per solution"

        def run(j, idx):
            rows = DeviceArray(ctx.alloc(idx.size * dim).gather_rows_from(Ud.buf, idx, dim), idx.size, dim)
            return sm.project_solutions_device(rows, self.bases[j].basis)
        res = self._per_cluster(sm, labels, run)
        return res if isinstance(true_solutions, DeviceArray) else res.numpy()

    def errors(self, sm, true_solutions, a):
        """(projection, Galerkin) relative H^1_0 errors per row."""
        from .lib.SolutionsManagers import _as_device
        Ud = _as_device(sm._ctx, true_solutions, sm.vspace_dim)
        norms = sm.H10norm(Ud)
        proj = sm.H10norm_diff(self.projection(sm, Ud, a), Ud) / norms
        gal = sm.H10norm_diff(self.forward_modeling(sm, a), Ud) / norms
        return proj, gal

    # -- the inverse problem: the parameter, and with it the cluster, is unknown ----------------------------------------------
    def observe(self, sm, points, weights=None, bounds=None, a_box="cluster", inflate=0.1) -> "LocalSensing":
        """Fix the sensors: ``points`` (m, 2) with optional weights (m,).  Per cluster a ``ResidualEstimator`` on its basis gives
        the A_1-orthonormal basis W_j and the residual table R_j; W_j is evaluated at the points and the sensors are reduced
        (``inverse.reduce_sensors``); the packed tables are uploaded once.  ValueError when a basis has dead directions, when the
        sensors do not determine the n coefficients of a cluster, for a basis built with center=True, or outside the limits of
        ``rom_local_select_layout``.
        bounds: None (the plain least squares of the reference in every cluster), "training" (each cluster's
        ``coefficient_boxes_``: the box its training snapshots span in W_j, computed by ``build``) or (lo, hi), kc x n arrays.
        a_box: "cluster" -- per block [min, max] of the cluster's training parameters, widened on both sides by ``inflate`` times
        the range in log a -- or "global": the box of all training parameters, for every cluster."""
        assert self.kmeans is not None, "LocalReducedBasis.observe before build"
        if self.center:
            raise ValueError("LocalReducedBasis.observe: center=True is not supported (the local spaces are linear: the estimate "
                             "c W_j has no mean added); build with center=False")
        return LocalSensing(self, sm, points, weights, bounds, a_box, inflate)

    def state_estimation(self, sm, measurement_points, measurements, return_coefs=False, **observe_kwargs):
        """``BaseReducedBasis.state_estimation`` with the local space chosen per measurement vector by the residual surrogate:
        the estimates (K, dim), with ``return_coefs`` also c (n, K) -- in the coordinates of the A_1-orthonormal basis of the
        chosen cluster (``LocalSensing.W``).  ``observe_kwargs``: weights, bounds, a_box, inflate of ``observe``."""
        est = self.observe(sm, measurement_points, **observe_kwargs).estimate(measurements, states=True)
        return (np.ascontiguousarray(est.coefficients.T), est.states) if return_coefs else est.states


class LocalEstimate(NamedTuple):
    """``LocalSensing.estimate``.  labels (K,) int32 (-1: no cluster's two solves converged on finite data); coefficients (K, n)
    in the chosen cluster's W; a (K, k): the minimiser of the surrogate, the blocks flattened as in ``a.reshape(K, -1)``;
    surrogate (K,) = min over the box of ||r(a; c W)||_{H^-1}; misfit (K,): the weighted measurement residual including the part
    outside the range of the reduced sensors; surrogate_all, misfit_all (K, kc), coefficients_all (K, kc, n), a_all (K, kc, k),
    status (K, kc): every cluster's; converged (K,): label >= 0; states (K, dim) = c W_label, or None."""
    labels: np.ndarray
    coefficients: np.ndarray
    a: np.ndarray
    surrogate: np.ndarray
    misfit: np.ndarray
    surrogate_all: np.ndarray
    misfit_all: np.ndarray
    converged: np.ndarray
    states: "np.ndarray | None"
    coefficients_all: np.ndarray
    a_all: np.ndarray
    status: np.ndarray


class LocalSensing:
    """Sensors fixed on a ``LocalReducedBasis`` (``LocalReducedBasis.observe``).  Host: ``W`` (kc of (n, dim)), ``RT``
    (kc, rank, 1 + k n), ``GR`` (kc, r, n), ``U`` (kc of (m, r)), the boxes ``c_lo``, ``c_hi`` (kc, n), ``a_lo``, ``a_hi`` (kc, k);
    the same tables stay on the device.  It holds device state and is not picklable: pickle the ``LocalReducedBasis`` and call
    ``observe`` again."""

    def __init__(self, lrb, sm, points, weights, bounds, a_box, inflate):
        from . import _ffi
        from .inverse import reduce_sensors
        from .lib.ReducedBasis import ResidualEstimator
        ctx, kc = sm._ctx, lrb.n_clusters
        points = np.asarray(points, dtype=np.float64)
        m = len(points)
        self.lrb, self.sm, self.ctx, self.kc, self.m = lrb, sm, ctx, kc, m
        self.weights = np.ones(m) if weights is None else np.asarray(weights, dtype=np.float64).reshape(m)
        self.W, self.U, tables, G = [], [], [], []
        for j in range(kc):
            est = ResidualEstimator(sm, lrb.bases[j].basis)
            try:
                dead = est.handle.download("dead")
                if dead.any():
                    raise ValueError(f"LocalReducedBasis.observe: the basis of cluster {j} has dead directions (rows "
                                     f"{np.flatnonzero(dead)[:8].tolist()}): no A_1-orthonormal basis of its dimension")
                tables.append(est.handle.download("R"))
                self.W.append(est.handle.download("W"))
            finally:
                est.handle.free()
            n = len(self.W[j])
            E = sm.evaluate_solutions(points, self.W[j])
            Uj, Gj, _ = reduce_sensors(E, self.weights)
            if Uj.shape[1] < n:
                raise ValueError(f"LocalReducedBasis.observe: the {m} weighted sensors determine {Uj.shape[1]} of the {n} coefficients "
                                 f"of cluster {j} (E_j lacks full column rank)")
            self.U.append(Uj)
            G.append(Gj)
        n = len(self.W[0])
        assert all(len(W) == n for W in self.W), "LocalReducedBasis.observe: one dimension for all clusters"
        self.n, self.r = n, n
        self.k = (tables[0].shape[1] - 1) // n
        self.rank = max(len(R) for R in tables)
        self.layout = _ffi.local_select_layout(self.n, self.k, self.rank, self.r)   # (ValueError outside the limits)
        if kc > self.layout["kc_max"]:
            raise ValueError(f"LocalReducedBasis.observe: kc = {kc} clusters, at most {self.layout['kc_max']} (rom_local_select)")
        self.RT = np.zeros((kc, self.rank, 1 + self.k * n))
        for j, R in enumerate(tables):
            self.RT[j, :len(R)] = R                  # (zero rows: exact)
        self.GR = np.ascontiguousarray(np.stack(G))
        self.Ucat = np.ascontiguousarray(np.concatenate(self.U, axis=1))   # (m, kc r): Y [U_1 .. U_kc] is one product
        self.c_lo, self.c_hi = self._c_box(bounds)
        self.a_lo, self.a_hi = self._a_box(a_box, inflate)
        self.RT_dev, self.GR_dev, self.U_dev = ctx.upload(self.RT), ctx.upload(self.GR), ctx.upload(self.Ucat)
        self.W_dev = [ctx.upload(W) for W in self.W]

    def __getstate__(self):
        raise TypeError("LocalSensing holds device state and is not picklable: pickle the LocalReducedBasis and call observe again")

    def _c_box(self, bounds):
        kc, n = self.kc, self.n
        if bounds is None:
            return np.full((kc, n), -np.inf), np.full((kc, n), np.inf)
        if isinstance(bounds, str):
            if bounds != "training":
                raise ValueError(f"LocalReducedBasis.observe: bounds = {bounds!r}; None, 'training' or (lo, hi)")
            boxes = getattr(self.lrb, "coefficient_boxes_", None)
            if not boxes or any(b is None for b in boxes):
                raise ValueError("LocalReducedBasis.observe: bounds = 'training' needs the boxes that build stores (coefficient_boxes_)")
            return np.stack([b[0] for b in boxes]), np.stack([b[1] for b in boxes])
        lo, hi = (np.array(np.broadcast_to(np.asarray(b, dtype=np.float64), (kc, n))) for b in bounds)
        return lo, hi

    def _a_box(self, a_box, inflate):
        lrb, kc = self.lrb, self.kc
        if a_box == "global":
            return np.tile(lrb.a_range_[0], (kc, 1)), np.tile(lrb.a_range_[1], (kc, 1))
        if a_box != "cluster":
            raise ValueError(f"LocalReducedBasis.observe: a_box = {a_box!r}; 'cluster' or 'global'")
        lo, hi = np.log(np.stack([b[0] for b in lrb.a_ranges_])), np.log(np.stack([b[1] for b in lrb.a_ranges_]))
        pad = float(inflate) * (hi - lo)
        return np.exp(lo - pad), np.exp(hi + pad)

    def _perp2(self, Yw, P):
        """(K, kc): |(w y) - U_j p_ij|^2, the part of the weighted measurements outside the range of U_j, from the product P."""
        out = np.zeros((len(Yw), self.kc))
        for j, Uj in enumerate(self.U):
            perp = Yw - P[:, j * self.r:(j + 1) * self.r] @ Uj.T
            out[:, j] = np.einsum("km,km->k", perp, perp)
        return out

    def reduce(self, measurements):
        """On the host: (Y w (K, m), P = Y w [U_1 .. U_kc] (K, kc r) with p_ij = U_j^T (w y_i) in block j, perp2 (K, kc)) -- per
        cluster what ``inverse.reduce_measurements`` returns, from one product."""
        Yw = np.asarray(measurements, dtype=np.float64).reshape(-1, self.m) * self.weights[None, :]
        P = np.ascontiguousarray(Yw @ self.Ucat)
        return Yw, P, self._perp2(Yw, P)

    def estimate(self, measurements, states=False, device=True) -> LocalEstimate:
        """For the K rows of ``measurements`` (K, m): the linear estimate in every local space, the cluster of smallest residual
        surrogate, its coefficients and parameter.  ``device``: one device product Y w [U_1 .. U_kc] for the reduced measurements
        of all clusters (downloaded once, for the part of w y outside the range of each U_j that the misfit includes), then
        ``rom_local_select``; False: ``reduce`` and the NumPy specification ``inverse.local_select_host``.  ``states``: also
        c W_label (K, dim), one ``rom_gemm_nn`` per non-empty cluster (rows of label -1: NaN)."""
        from .inverse import local_select_host
        ctx, kc, n, k, r = self.ctx, self.kc, self.n, self.k, self.r
        if device and len(np.atleast_2d(measurements)):
            Yw = np.asarray(measurements, dtype=np.float64).reshape(-1, self.m) * self.weights[None, :]
            K = len(Yw)
            Pd = ctx.alloc(K * kc * r)
            ctx.gemm_nn(K, kc * r, self.m, ctx.upload(Yw), 0, self.m, self.U_dev, 0, kc * r, Pd, 0, kc * r)
            res, _ = ctx.local_select(kc, n, k, self.rank, r, self.RT_dev, self.GR_dev, Pd, 0, kc * r, K, self.c_lo, self.c_hi, self.a_lo,
                                      self.a_hi)
            perp2 = self._perp2(Yw, Pd.download(K * kc * r, shape=(K, kc * r)))
        else:
            Yw, P, perp2 = self.reduce(measurements)
            K = len(Yw)
            res = local_select_host(self.RT, self.GR, P, self.c_lo, self.c_hi, self.a_lo, self.a_hi)
        misfit_all = np.sqrt(res.misfit_all ** 2 + perp2)
        labels = res.labels
        ok = labels >= 0
        misfit = np.where(ok, misfit_all[np.arange(K), np.maximum(labels, 0)], np.nan)
        lifted = self._lift(res.coefficients, labels) if states else None
        return LocalEstimate(labels, res.coefficients, res.a, res.surrogate, misfit, res.surrogate_all, misfit_all, ok, lifted,
                             res.c_all, res.a_all, res.status)

    def _lift(self, coefficients, labels):
        """c W_label per row (K, dim) on the host; rows of label -1 are NaN."""
        from .lib.SolutionsManagers import DeviceArray
        ctx, dim, n = self.ctx, self.sm.vspace_dim, self.n
        ok = np.flatnonzero(labels >= 0)
        out = np.full((len(labels), dim), np.nan)
        if ok.size:
            C = np.ascontiguousarray(coefficients[ok])

            def run(j, idx):
                part = ctx.alloc(idx.size * dim)
                ctx.gemm_nn(idx.size, dim, n, ctx.upload(C[idx]), 0, n, self.W_dev[j], 0, dim, part, 0, dim)
                return DeviceArray(part, idx.size, dim)
            out[ok] = self.lrb._per_cluster(self.sm, labels[ok], run).numpy()
        return out
