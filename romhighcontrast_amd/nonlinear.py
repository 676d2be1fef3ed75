"""The device-independent parts of the reference's second experiment, src/experiments/NonLinearROM.py ("learn the higher
PCA coordinates of a solution from its leading ones"): the parameter sweep, the full PCA of the tall snapshot block and
the index bookkeeping of the regression experiments.  The sweep runs on the device (SolutionsManagerFEM) and the PCA is
``pca_tall`` (rom_pca_tall: 25,000 x 81 is M >> dim, the shape rom_pod was not designed for).  The polynomial regressions
of the third stage have a device path as well (``PolynomialMap``, ``learn_eigenvalues_device``, ``nonlinear_reconstruction``:
rom_poly_fit / rom_poly_predict), and so have the regression tree and the random forest of the model list (``TreeMap``,
``ForestMap``: rom_tree_fit / rom_tree_predict, CART trees built level by level over all trees of a forest at once); MLPs
stay scikit-learn's.  The plots and the PerplexityLab LabPipeline driver of the reference are out of scope.
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np

from .lib.ReducedBasis import pca_tall
from .lib.SolutionsManagers import DeviceArray, SolutionsManagerFEM

__all__ = ["ZERO", "Bounds", "MWhere", "draw_parameters", "vn_family_sampler", "do_pca", "get_known_unknown_indexes",
           "learn_eigenvalues", "PolynomialMap", "TreeMap", "ForestMap", "learn_eigenvalues_device", "nonlinear_reconstruction"]

ZERO = 1e-15
Bounds = namedtuple("Bounds", "lower upper")
MWhere = namedtuple("MWhere", "m start")   # the m known PCA coordinates start at index `start`


def draw_parameters(n_max, geometry, lower_bounds, upper_bounds):
    """The reference's draw (:25-28): seed 42, then one ``uniform(lo, hi, n_max)`` call per block in row-major block
    order; sample i takes entry i of every call.  Returns the list of n_max arrays of shape ``geometry``."""
    np.random.seed(42)
    per_block = [np.random.uniform(lower_bounds, upper_bounds, n_max) for _ in range(int(np.prod(geometry)))]
    return [np.reshape(coefs, geometry) for coefs in zip(*per_block)]


def vn_family_sampler(n_max, geometry, lower_bounds, upper_bounds, mesh):
    """(:24-31) n_max snapshots of the (geometry, N = mesh) problem for the parameters of ``draw_parameters``."""
    a = draw_parameters(n_max, geometry, lower_bounds, upper_bounds)
    sm = SolutionsManagerFEM(blocks_geometry=tuple(geometry), N=mesh, num_cores=1, method="lsq")
    solutions = sm.generate_solutions(a)
    return {"solution_manager": sm, "a": a, "solutions": solutions}


def do_pca(solutions, ctx=None):
    """(:34-41) the full PCA of the snapshot block, all min(M, dim) modes: the scores of the block, the variances and
    the singular values.  ``do_pca.last`` keeps the TallPCA of the call (components, mean, resolved_modes_)."""
    from . import _ffi
    ctx = _ffi.get_context() if ctx is None else ctx
    M, dim = np.shape(solutions)
    n = min(M, dim)
    pca = pca_tall(ctx, solutions, n=n, center=True, scores=True, download=True)
    do_pca.last = pca
    return {"pca_projections": pca.scores, "explained_variance": pca.explained_variance_,
            "singular_values": pca.singular_values_}


def get_known_unknown_indexes(mwhere, pca_projections, learn_higher_modes_only, only_j=None):
    """(:44-51) columns of the scores that are given (``mwhere.m`` of them from ``mwhere.start``) and columns to learn:
    those after the known ones -- the first ``only_j`` of them when given -- and, unless ``learn_higher_modes_only``, the
    ones before the known block as well (listed first)."""
    n_modes = np.shape(pca_projections)[1]
    idx = np.arange(n_modes, dtype=int)
    first_after = mwhere.start + mwhere.m
    known = idx[mwhere.start:first_after]
    stop = n_modes if only_j is None else first_after + only_j
    unknown = idx[first_after:stop]
    if not learn_higher_modes_only:
        unknown = np.append(idx[:mwhere.start], unknown)
    return known, unknown


def learn_eigenvalues(model):
    """(:54-70) an experiment function around a scikit-learn pipeline: fit unknown <- known coordinates on the rows
    [n_test, n_test + n_train), predict the first n_test rows (always the same test rows), return the errors.  Host
    scikit-learn on the (M, n) scores: not a hot path."""

    def experiment(n_train, n_test, pca_projections, mwhere: MWhere, only_j, learn_higher_modes_only=True):
        known, unknown = get_known_unknown_indexes(mwhere, pca_projections, learn_higher_modes_only, only_j)
        train = slice(n_test, n_test + n_train)
        model.fit(pca_projections[train, known], pca_projections[train, unknown])
        predictions = np.asarray(model.predict(pca_projections[:n_test, known]))
        return {"error": pca_projections[:n_test, unknown] - predictions.reshape((-1, len(unknown)))}

    experiment.__name__ = " ".join(step[0] for step in model.steps)
    return experiment


# ---- the regression stage on the device: rom_poly_fit / rom_poly_predict --------------------------------------------------


def _contiguous_ranges(idx):
    """[a, a+1, .., b-1, c, c+1, ...] -> [(a, b), (c, ...)]: the runs of consecutive column indices, in order."""
    idx = [int(i) for i in idx]
    runs = []
    for i in idx:
        if runs and runs[-1][1] == i:
            runs[-1][1] = i + 1
        else:
            runs.append([i, i + 1])
    return [tuple(r) for r in runs]


class PolynomialMap:
    """(:131-139) ``Pipeline([PolynomialFeatures(degree), LinearRegression()])`` as one device fit (rom_poly_fit): the
    least-squares polynomial of total degree <= ``degree`` in a basis of scaled Legendre products, by a CholeskyQR whose
    Gram matrices come from the data.  Same function space as the scikit-learn pipeline -- the same predictions whenever
    the problem has full rank -- independent of the scales of the input columns.  ``fit`` / ``predict`` follow
    scikit-learn's protocol on host arrays or DeviceArrays (``predict`` returns what it was given: a host array for a host
    array); ``steps`` lets ``learn_eigenvalues(model)`` take it unchanged.  ``info_`` is the PolyMap's info dict."""

    def __init__(self, degree, rcond=0.0, ctx=None):
        self.degree, self.rcond, self._ctx = int(degree), float(rcond), ctx
        # (the reference's names, :131-139: "LR", "Quadratic LR", "Degree 4 LR")
        first = [] if self.degree == 1 else [("Quadratic" if self.degree == 2 else f"Degree {self.degree}", None)]
        self.steps = first + [("LR device", self)]
        self.map_ = None

    def _context(self):
        from . import _ffi
        if self._ctx is None:
            self._ctx = _ffi.get_context()
        return self._ctx

    def _device(self, A):
        if isinstance(A, DeviceArray):
            return A
        arr = np.asarray(A, dtype=np.float64)
        arr = arr.reshape(-1, 1) if arr.ndim == 1 else arr
        arr = np.ascontiguousarray(arr)
        return DeviceArray(self._context().upload(arr), arr.shape[0], arr.shape[1])

    def fit(self, X, y):
        Xd, Yd = self._device(X), self._device(y)
        assert Xd.rows == Yd.rows, "PolynomialMap.fit: X and y have different numbers of rows"
        return self.fit_columns(Xd, (0, Xd.dim), Yd, (0, Yd.dim), 0, Xd.rows)

    def fit_columns(self, Xd, xcols, Yd, ycols, row0, rows):
        """Fit on rows [row0, row0 + rows) of the column ranges xcols = (lo, hi) of Xd and ycols of Yd (DeviceArrays; they
        may be the same block): nothing is copied."""
        from . import _ffi
        try:
            self.map_ = self._context().poly_fit(Xd.buf, row0 * Xd.dim + xcols[0], Xd.dim, xcols[1] - xcols[0], Yd.buf,
                                                 row0 * Yd.dim + ycols[0], Yd.dim, ycols[1] - ycols[0], rows, self.degree, self.rcond)
        except _ffi.RomLibraryError as e:
            if "NaN / Inf" in str(e):   # (scikit-learn's estimators raise ValueError on such input)
                raise ValueError(str(e)) from None
            raise
        self.info_ = self.map_.info
        return self

    def predict(self, X):
        assert self.map_ is not None, "PolynomialMap.predict before fit"
        Xd = self._device(X)
        out = self._context().alloc(max(Xd.rows * self.map_.q, 1))
        self.map_.predict(Xd.buf, 0, Xd.dim, Xd.rows, OUT=out)
        res = DeviceArray(out, Xd.rows, self.map_.q)
        return res if isinstance(X, DeviceArray) else res.numpy()


class TreeMap(PolynomialMap):
    """(:136) ``DecisionTreeRegressor()`` as one device fit (rom_tree_fit): a multi-output CART tree with the weighted-MSE
    criterion summed over the targets, thresholds halfway between consecutive distinct values of fp64 inputs, ties to the
    lowest input and position (scikit-learn draws them at random).  The protocol of PolynomialMap: ``fit`` / ``fit_columns`` /
    ``predict`` on host arrays or DeviceArrays, ``map_`` (the TreeMapHandle), ``info_``, ``steps``."""

    _name = "Tree device"

    def __init__(self, max_depth=None, min_samples_split=2, min_samples_leaf=1, ctx=None):
        self.max_depth, self.min_samples_split, self.min_samples_leaf = max_depth, int(min_samples_split), int(min_samples_leaf)
        self._ctx = ctx
        self.steps = [(self._name, self)]
        self.map_ = None
        self.counts_ = None

    def _counts(self, M):
        """(T, M) multiplicities of the rows per tree, or None: every row once."""
        return None

    n_trees = 1

    def fit_columns(self, Xd, xcols, Yd, ycols, row0, rows):
        from . import _ffi
        self.counts_ = self._counts(int(rows))
        try:
            self.map_ = self._context().tree_fit(Xd.buf, row0 * Xd.dim + xcols[0], Xd.dim, xcols[1] - xcols[0], Yd.buf,
                                                 row0 * Yd.dim + ycols[0], Yd.dim, ycols[1] - ycols[0], rows, self.n_trees,
                                                 self.counts_, self.max_depth, self.min_samples_split, self.min_samples_leaf)
        except _ffi.RomLibraryError as e:
            if "NaN / Inf" in str(e):   # (scikit-learn's estimators raise ValueError on such input)
                raise ValueError(str(e)) from None
            raise
        self.info_ = self.map_.info
        return self


class ForestMap(TreeMap):
    """(:137) ``RandomForestRegressor(n_estimators)`` as one device fit: ``n_estimators`` trees on bootstrap samples of the
    rows, all built together level by level; the prediction is the mean over the trees.  Every input is a split candidate at
    every node, as in scikit-learn's regressor (max_features = 1.0).  The draw is
    ``np.random.default_rng(random_state).integers(0, M, (T, M))``, kept per tree as the counts ``counts_`` (T, M)."""

    _name = "RF device"

    def __init__(self, n_estimators=10, bootstrap=True, random_state=0, max_depth=None, min_samples_split=2, min_samples_leaf=1,
                 ctx=None):
        super().__init__(max_depth, min_samples_split, min_samples_leaf, ctx)
        self.n_estimators, self.bootstrap, self.random_state = int(n_estimators), bool(bootstrap), random_state
        self.n_trees = self.n_estimators

    def _counts(self, M):
        return self.bootstrap_counts(self.n_estimators, M, self.random_state) if self.bootstrap else None

    @staticmethod
    def bootstrap_counts(T, M, random_state=0):
        draw = np.random.default_rng(random_state).integers(0, M, (T, M))
        return np.stack([np.bincount(row, minlength=M) for row in draw]).astype(np.int32)


def learn_eigenvalues_device(degree=None, rcond=0.0, ctx=None, model=None):
    """(:54-70) ``learn_eigenvalues`` with the device fit (``model``: a TreeMap / ForestMap / PolynomialMap instance used
    instead of the polynomial of ``degree``; it is fitted again for every range of unknowns): the same experiment function, but ``pca_projections`` is the
    DeviceArray of scores (``pca_tall(..., download=False).scores``) and nothing of size (rows, modes) comes to the host
    except the (n_test, unknown) errors.  Fit on rows [n_test, n_test + n_train), predict rows [0, n_test).  A
    non-contiguous unknown list (``learn_higher_modes_only=False``) is fitted as its contiguous ranges.  Returns
    ``{"error": ..., "rmse": ...}``: ``rmse`` per unknown mode from the device's column sums of squares."""

    def experiment(n_train, n_test, pca_projections, mwhere: MWhere, only_j, learn_higher_modes_only=True):
        from . import _ffi
        S = pca_projections
        assert isinstance(S, DeviceArray), "learn_eigenvalues_device: the scores as a DeviceArray"
        c = _ffi.get_context() if ctx is None else ctx
        known, unknown = get_known_unknown_indexes(mwhere, np.empty((0, S.dim)), learn_higher_modes_only, only_j)
        errors, rmse = [], []
        for lo, hi in _contiguous_ranges(unknown):
            fitted = PolynomialMap(degree, rcond, c) if model is None else model
            if fitted._ctx is None:
                fitted._ctx = c
            fitted.fit_columns(S, (int(known[0]), int(known[-1]) + 1), S, (lo, hi), n_test, n_train)
            E = c.alloc(max(n_test * (hi - lo), 1))
            ss = fitted.map_.predict(S.buf, int(known[0]), S.dim, n_test, OUT=E, Yref=S.buf, r_off=lo, ldr=S.dim, sumsq=True)
            errors.append(E.download(n_test * (hi - lo), shape=(n_test, hi - lo)))
            rmse.append(np.sqrt(ss / n_test))
        if not errors:
            return {"error": np.zeros((n_test, 0)), "rmse": np.zeros(0)}
        return {"error": np.hstack(errors), "rmse": np.concatenate(rmse)}

    experiment.__name__ = " ".join(step[0] for step in (PolynomialMap(degree) if model is None else model).steps)
    return experiment


def nonlinear_reconstruction(pca, poly, known_scores, known_start=0, unknown_start=None, download=True):
    """The reduced model the fitted map defines: u = mean + known scores . their components + predicted scores . theirs.
    ``pca``: a TallPCA; ``poly``: a fitted PolynomialMap, TreeMap or ForestMap (or its handle) from m known to q unknown score columns;
    ``known_scores``: (K, m) host array or DeviceArray; the known columns are the components [known_start, known_start + m)
    and the predicted ones [unknown_start, unknown_start + q) (default: right after the known ones).  Two rom_gemm_nn
    products on the device."""
    from . import _ffi
    pm = poly.map_ if isinstance(poly, PolynomialMap) else poly
    ctx = pm.ctx
    m, q = pm.m, pm.q
    unknown_start = known_start + m if unknown_start is None else int(unknown_start)
    if isinstance(known_scores, DeviceArray):
        Kd = known_scores
    else:
        arr = np.ascontiguousarray(np.asarray(known_scores, dtype=np.float64)).reshape(-1, m)
        Kd = DeviceArray(ctx.upload(arr), arr.shape[0], m)
    assert Kd.dim == m, "nonlinear_reconstruction: known_scores must have the map's m columns"
    K = Kd.rows
    comps = pca.components_
    Vd = comps if isinstance(comps, DeviceArray) else DeviceArray(ctx.upload(np.asarray(comps, dtype=np.float64)), *np.shape(comps))
    dim = Vd.dim
    assert known_start + m <= Vd.rows and unknown_start + q <= Vd.rows, "nonlinear_reconstruction: components out of range"
    mean = pca.mean_.numpy().ravel() if isinstance(pca.mean_, DeviceArray) else np.asarray(pca.mean_, dtype=np.float64).ravel()
    pred = ctx.alloc(max(K * q, 1))
    pm.predict(Kd.buf, 0, m, K, OUT=pred)
    U = ctx.upload(np.tile(mean, (K, 1)))
    ctx.gemm_nn(K, dim, m, Kd.buf, 0, m, Vd.buf, known_start * dim, dim, U, 0, dim, alpha=1.0, beta=1.0)
    ctx.gemm_nn(K, dim, q, pred, 0, q, Vd.buf, unknown_start * dim, dim, U, 0, dim, alpha=1.0, beta=1.0)
    out = DeviceArray(U, K, dim)
    return out.numpy() if download else out
