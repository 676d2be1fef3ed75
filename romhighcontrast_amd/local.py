"""Local reduced bases: the parameter domain is split by k-means and every part gets its own small POD basis (hp-RB: Eftang,
Patera, Ronquist; Amsallem, Zahr, Farhat).  The other standard answer -- beside the curved charts of ``nonlinear.py`` -- to a
slowly decaying Kolmogorov width: a local basis of dimension n reaches the error of a global one of 2 - 4 times the dimension
in the pre-asymptotic range, and the online reduced solve costs n^3 per parameter.  The gain shrinks once n reaches the
effective dimension of the manifold.

``kmeans_host`` / ``maximin_rows_host`` are the NumPy specification of ``rom_kmeans_fit`` / ``rom_kmeans_init_maximin`` (the same
rules: the total order (dist2, centroid index), empty clusters kept where they are, the stop rules, the final assignment);
``KMeans`` is the estimator on the device and ``LocalReducedBasis`` the clustered POD bases with the online operations of
``BaseReducedBasis``."""
from __future__ import annotations

from logging import warning
from typing import NamedTuple

import numpy as np

__all__ = ["kmeans_host", "maximin_rows_host", "dist2_host", "KMeansHostResult", "KMeans", "LocalReducedBasis"]


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
        self.bases, self.singular_values_ = [], []
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
        return self

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
