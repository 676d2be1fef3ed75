"""The device-independent parts of the reference's second experiment, src/experiments/NonLinearROM.py ("learn the higher
PCA coordinates of a solution from its leading ones"): the parameter sweep, the full PCA of the tall snapshot block and
the index bookkeeping of the regression experiments.  The sweep runs on the device (SolutionsManagerFEM) and the PCA is
``pca_tall`` (rom_pca_tall: 25,000 x 81 is M >> dim, the shape rom_pod was not designed for).  The polynomial regressions
of the third stage have a device path as well (``PolynomialMap``, ``learn_eigenvalues_device``, ``nonlinear_reconstruction``:
rom_poly_fit / rom_poly_predict), and so have the regression tree and the random forest of the model list (``TreeMap``,
``ForestMap``: rom_tree_fit / rom_tree_predict, CART trees built level by level over all trees of a forest at once) and the
"NN" entry of that list (``MLPMap``: rom_mlp_fit / rom_mlp_predict, loss and gradient in one fused MFMA kernel and a device
L-BFGS whose specification is ``mlp_fit_host``).  The plots and the PerplexityLab LabPipeline driver of the reference are out of scope.
"""
from __future__ import annotations

from collections import namedtuple
from typing import NamedTuple, Optional

import numpy as np

from .lib.ReducedBasis import pca_tall
from .lib.SolutionsManagers import DeviceArray, SolutionsManagerFEM

__all__ = ["ZERO", "Bounds", "MWhere", "draw_parameters", "vn_family_sampler", "do_pca", "get_known_unknown_indexes",
           "learn_eigenvalues", "PolynomialMap", "TreeMap", "ForestMap", "MLPMap", "mlp_loss_grad_host", "mlp_fit_host", "learn_eigenvalues_device", "nonlinear_reconstruction", "SenseResult", "SensingEstimate", "legendre_table",
           "legendre_features", "sensing_matrix", "sense_scores", "PolynomialSensing"]

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


# ---- MLP maps: rom_mlp_fit / rom_mlp_predict and their specification ------------------------------------------------------


def _mlp_split(w, sizes):
    """The flat parameter vector as [(W_l (outputs, inputs), b_l)]: all W in layer order (row-major), then all b."""
    nl = len(sizes) - 1
    Ws, at = [], 0
    for l in range(nl):
        Ws.append(w[at:at + sizes[l + 1] * sizes[l]].reshape(sizes[l + 1], sizes[l]))
        at += sizes[l + 1] * sizes[l]
    bs = []
    for l in range(nl):
        bs.append(w[at:at + sizes[l + 1]])
        at += sizes[l + 1]
    assert at == len(w), f"mlp: {len(w)} parameters for the sizes {list(sizes)}, which have {at}"
    return list(zip(Ws, bs))


def mlp_loss_grad_host(w, sizes, activation, T, Ys, alpha, dtype=np.float64):
    """The loss of rom_mlp_* and its gradient in plain NumPy, all arithmetic in ``dtype``: L = 1/(2M) sum |net(T) - Ys|^2 +
    alpha/(2M) sum_l |W_l|_F^2 for the scaled inputs T (M, m) and scaled targets Ys (M, q), ``sizes`` = [m, hidden .., q],
    ``activation`` "tanh", "logistic" or "relu" (linear output), w flat as in ``_ffi.mlp_layout``.  The specification of
    k_mlp_eval / k_mlp_reduce.  Returns (L, gradient (P,))."""
    w, T, Ys = np.asarray(w, dtype=dtype), np.asarray(T, dtype=dtype), np.asarray(Ys, dtype=dtype)
    one, half, M = w.dtype.type(1), w.dtype.type(0.5), w.dtype.type(len(T))
    alpha = w.dtype.type(alpha)
    layers = _mlp_split(w, sizes)
    A = [T]
    for l, (W, b) in enumerate(layers):
        z = A[-1] @ W.T + b
        if l + 1 < len(layers):
            z = np.tanh(z) if activation == "tanh" else one / (one + np.exp(-z)) if activation == "logistic" else np.where(z > 0, z, 0 * z)
        A.append(z)
    delta = A[-1] - Ys
    loss = (half * (delta * delta).sum() + half * alpha * sum((W * W).sum() for W, _ in layers)) / M
    gW, gb = [None] * len(layers), [None] * len(layers)
    for l in range(len(layers) - 1, -1, -1):
        W = layers[l][0]
        gW[l] = ((delta.T @ A[l] + alpha * W) / M).ravel()
        gb[l] = delta.sum(axis=0) / M
        if l > 0:
            a = A[l]
            d = one - a * a if activation == "tanh" else a * (one - a) if activation == "logistic" else (a > 0).astype(w.dtype)
            delta = (delta @ W) * d
    return loss, np.concatenate(gW + gb)


def mlp_fit_host(w0, sizes, activation, T, Ys, alpha, max_iter, tol, memory, dtype=np.float64):
    """The optimiser of rom_mlp_fit (k_mlp_director), step for step, in plain NumPy with all arithmetic in ``dtype``: full-batch
    L-BFGS (two-loop recursion over at most ``memory`` pairs, gamma = s.y / y.y), first step min(1, 1/|g|_2) then 1, Armijo
    backtracking (c1 = 1e-4, halving, at most 30 trials), a pair kept when s.y > 1e-10 |s| |y|, steepest descent with cleared
    memory when g.d >= 0.  Stops: 0 |g|_inf <= tol, 1 relative loss decrease <= tol 1e-2 on two consecutive accepted
    iterations, 2 max_iter, 3 line search exhausted.  Returns a dict: w, loss, grad_inf, iterations, evaluations, stop,
    loss_curve (iterations + 1), trials (evaluations of every line search)."""
    dt = np.dtype(dtype).type
    w = np.array(w0, dtype=dtype)
    f, g = mlp_loss_grad_host(w, sizes, activation, T, Ys, alpha, dtype)
    evals, k, stag, hist, trials = 1, 0, 0, [f], []
    S, Yp, rho, gamma = [], [], [], dt(1)
    tol = dt(tol)
    while True:
        ginf = np.abs(g).max()
        if ginf <= tol:
            stop = 0
            break
        if stag >= 2:
            stop = 1
            break
        if k >= max_iter:
            stop = 2
            break
        q, al = g.copy(), []
        for c in range(len(S) - 1, -1, -1):          # newest pair first
            a = rho[c] * (S[c] @ q)
            al.append(a)
            q = q - a * Yp[c]
        if S:
            q = q * gamma
        for c in range(len(S)):
            b = rho[c] * (Yp[c] @ q)
            q = q + (al[len(S) - 1 - c] - b) * S[c]
        d = -q
        gd, gg = g @ d, g @ g
        if not gd < 0:                               # not a descent direction: steepest descent, the memory cleared
            d, gd, S, Yp, rho = -g, -gg, [], [], []
        t = min(dt(1), dt(1) / np.sqrt(gg)) if k == 0 else dt(1)
        accepted = False
        for trial in range(30):
            wt = w + t * d
            ft, gt = mlp_loss_grad_host(wt, sizes, activation, T, Ys, alpha, dtype)
            evals += 1
            if ft <= f + dt(1e-4) * t * gd:
                accepted = True
                break
            t = t * dt(0.5)
        trials.append(trial + 1)
        if not accepted:
            stop = 3
            break
        s, y = wt - w, gt - g
        sy, ss, yy = s @ y, s @ s, y @ y
        if sy > dt(1e-10) * np.sqrt(ss) * np.sqrt(yy):
            if len(S) == memory:
                S, Yp, rho = S[1:], Yp[1:], rho[1:]
            S, Yp, rho, gamma = S + [s], Yp + [y], rho + [dt(1) / sy], sy / yy
        fold, w, f, g, k = f, wt, ft, gt, k + 1
        hist.append(f)
        stag = stag + 1 if fold - f <= tol * dt(1e-2) * max(abs(fold), abs(f)) else 0
    return dict(w=w, loss=f, grad_inf=ginf, iterations=k, evaluations=evals, stop=stop, loss_curve=np.array(hist, dtype=dtype),
                trials=trials)


class MLPMap(PolynomialMap):
    """(:138, src/lib/Estimators.py:75-97) the reference's ``FNNModel`` / ``MLPRegressor`` as one device fit (rom_mlp_fit): m inputs
    -> ``hidden_layer_sizes`` (1 .. 3 layers of 1 .. 64 units; "tanh", "logistic" -- alias "sigmoid", the reference's word -- or
    "relu") -> q linear outputs, scikit-learn's loss with L2 penalty ``alpha``, full-batch L-BFGS on the device (``mlp_fit_host``
    is its specification), inputs scaled to [-1, 1] and, with ``scale_targets``, targets standardised.  Initial weights:
    scikit-learn's Glorot uniform draw from ``np.random.RandomState(random_state)`` (``initial_weights``).  The protocol of
    PolynomialMap: ``fit`` / ``fit_columns`` / ``predict`` on host arrays or DeviceArrays, ``map_`` (the MLPHandle), ``info_``,
    ``steps``; after a fit ``coefs_`` / ``intercepts_`` (scikit-learn's shapes, in scaled coordinates), ``loss_``,
    ``loss_curve_``, ``n_iter_``.  ValueError outside the limits of ``_ffi.mlp_layout``."""

    def __init__(self, hidden_layer_sizes=(20, 20), activation="tanh", alpha=1e-4, max_iter=200, tol=1e-6, random_state=0,
                 scale_targets=True, memory=10, ctx=None):
        from . import _ffi
        hidden = (hidden_layer_sizes,) if np.isscalar(hidden_layer_sizes) else tuple(hidden_layer_sizes)
        self.hidden_layer_sizes = tuple(int(v) for v in hidden)
        if activation not in _ffi.MLP_ACTIVATIONS:
            raise ValueError(f"MLPMap: activation {activation!r}, one of {sorted(_ffi.MLP_ACTIVATIONS)}")
        self.activation = "logistic" if activation == "sigmoid" else activation
        self.alpha, self.max_iter, self.tol, self.random_state = float(alpha), int(max_iter), float(tol), random_state
        self.scale_targets, self.memory, self._ctx = bool(scale_targets), int(memory), ctx
        self.steps = [("NN device", self)]
        self.map_ = None

    @staticmethod
    def initial_weights(sizes, activation="tanh", random_state=0):
        """scikit-learn's initialisation (MLPRegressor._init_coef): per layer W (fan_in, fan_out) then b (fan_out,), uniform in
        +- sqrt(6 / (fan_in + fan_out)) (2 instead of 6 for "logistic"), from ``np.random.RandomState(random_state)``.  Returns
        the flat parameter vector of ``_ffi.mlp_layout``: all W_l^T (outputs x inputs, row-major), then all b_l."""
        rng = np.random.RandomState(random_state)
        factor = 2.0 if activation in ("logistic", "sigmoid") else 6.0
        Ws, bs = [], []
        for fan_in, fan_out in zip(sizes[:-1], sizes[1:]):
            bound = np.sqrt(factor / (fan_in + fan_out))
            Ws.append(rng.uniform(-bound, bound, (fan_in, fan_out)).T.ravel())
            bs.append(rng.uniform(-bound, bound, fan_out))
        return np.concatenate(Ws + bs)

    def _check(self, m, q):
        from . import _ffi
        return _ffi.mlp_layout(int(m), self.hidden_layer_sizes, int(q))   # ValueError outside the limits: no device call yet

    def fit(self, X, y):
        shape = lambda A: (A.rows, A.dim) if isinstance(A, DeviceArray) else (np.shape(A) + (1,))[:2]
        self._check(shape(X)[1], shape(y)[1])
        return super().fit(X, y)

    def fit_columns(self, Xd, xcols, Yd, ycols, row0, rows):
        m, q = xcols[1] - xcols[0], ycols[1] - ycols[0]
        lay = self._check(m, q)
        w0 = self.initial_weights(lay["sizes"], self.activation, self.random_state)
        self.map_ = self._context().mlp_fit(Xd.buf, row0 * Xd.dim + xcols[0], Xd.dim, m, Yd.buf, row0 * Yd.dim + ycols[0], Yd.dim, q,
                                            rows, self.hidden_layer_sizes, w0, self.activation, self.alpha, self.scale_targets,
                                            self.max_iter, self.tol, self.memory)
        self.info_ = self.map_.info
        self.coefs_, self.intercepts_ = self.map_.weights()
        self.loss_curve_ = self.map_.download("loss_curve")
        self.loss_, self.n_iter_ = self.info_["loss"], self.info_["iterations"]
        return self


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


# ---- sensor state estimation on the polynomial manifold: rom_poly_sense ---------------------------------------------------


class SenseResult(NamedTuple):
    """``sense_scores`` / ``Context.poly_sense``: t (K, m) the scaled known coordinates, misfit (K,) = sqrt(|p - G_r phi(t)|^2 +
    perp2), converged and iterations (K,), sigma_min (K,) of the final Jacobian's free columns, start (K,) the start that won."""
    t: np.ndarray
    misfit: np.ndarray
    converged: np.ndarray
    iterations: np.ndarray
    sigma_min: np.ndarray
    start: np.ndarray


class SensingEstimate(NamedTuple):
    """``PolynomialSensing.estimate``: known_scores (K, m) = c + h t and predicted_scores (K, q) = the map at them; misfit,
    converged, iterations, sigma_min, start (K,) of the nonlinear least squares (``SenseResult``); linear_scores (K, m): the
    least-squares estimate on the m known modes alone; states: DeviceArray (K, dim) of the decoded states, or None."""
    known_scores: np.ndarray
    predicted_scores: np.ndarray
    misfit: np.ndarray
    converged: np.ndarray
    iterations: np.ndarray
    sigma_min: np.ndarray
    start: np.ndarray
    linear_scores: np.ndarray
    states: Optional[DeviceArray]


def legendre_table(t, d):
    """L_k(t) and L'_k(t), k = 0 .. d, of every entry of t: two arrays t.shape + (d + 1,), in t's dtype.  The recurrences of
    rom_poly.hip and rom_sense.hip: (k + 1) L_{k+1} = (2k + 1) t L_k - k L_{k-1};  L'_{k+1} = L'_{k-1} + (2k + 1) L_k."""
    t = np.asarray(t)
    L, D = [np.ones_like(t), t], [np.zeros_like(t), np.ones_like(t)]
    for k in range(1, int(d)):
        L.append(((2 * k + 1) * t * L[k] - k * L[k - 1]) / (k + 1))
        D.append(D[k - 1] + (2 * k + 1) * L[k])
    return np.stack(L[:d + 1], axis=-1), np.stack(D[:d + 1], axis=-1)


def legendre_features(t, powers, jacobian=True):
    """phi (B, P) and d phi / d t (B, P, m) (None unless ``jacobian``) at the rows of t (B, m) for the exponent rows ``powers``
    (P, m) (``_ffi.poly_terms``): phi_p = prod_j L_{powers[p, j]}(t_j), the factors taken in the order of j."""
    t = np.asarray(t)
    powers = np.asarray(powers, dtype=np.int64)
    m = powers.shape[1]
    d = max(int(powers.max()) if powers.size else 0, 1)
    L, D = legendre_table(t, d)                        # (B, m, d + 1)
    cols = np.arange(m)[None, :]
    sel = L[:, cols, powers]                           # (B, P, m)
    F = sel.prod(axis=-1)
    if not jacobian:
        return F, None
    dsel = D[:, cols, powers]
    dF = np.empty(sel.shape, dtype=sel.dtype)
    for j in range(m):
        s = sel.copy()
        s[:, :, j] = dsel[:, :, j]
        dF[:, :, j] = s.prod(axis=-1)
    return F, dF


def sensing_matrix(e0, Ek, Eu, c, h, W, powers):
    """S (ms, P) with  l(mean + z V_known + g(z) V_unknown) = S phi(t),  z = c + h t,  g = W phi:  S = E_u W, plus e0 + E_k c on
    the column of the constant term and h_j E_k[:, j] on the column of the term t_j.  e0 (ms,) = l(mean), Ek (ms, m) and Eu
    (ms, q) = l(known / predicted components), c, h (m,) and W (q, P) of the fitted map, powers (P, m)."""
    e0, Ek, Eu = np.asarray(e0, dtype=np.float64), np.asarray(Ek, dtype=np.float64), np.asarray(Eu, dtype=np.float64)
    c, h, W = np.asarray(c, dtype=np.float64), np.asarray(h, dtype=np.float64), np.asarray(W, dtype=np.float64)
    powers = np.asarray(powers, dtype=np.int64)
    S = Eu @ W
    degree = powers.sum(axis=1)
    S[:, int(np.flatnonzero(degree == 0)[0])] += e0 + Ek @ c
    for j in range(len(c)):
        p = int(np.flatnonzero((degree == 1) & (powers[:, j] == 1))[0])
        S[:, p] += h[j] * Ek[:, j]
    return S


SENSE_LIMITS = dict(m=16, d=8, P=96, r=96, t=8)   # rom_poly_sense (csrc/rom_sense.hip)
from .inverse import BVLS_LIMITS  # noqa: E402,F401  rom_bvls (csrc/rom_bvls.hip), the linear estimators' limits: defined in inverse.py
_SENSE_CHUNK = 4096                                # systems of one batch of the host iteration


def _check_sense_limits(m, d, P, r, t):
    for name, v in (("m", m), ("d", d), ("P", P), ("r", r), ("t", t)):
        if not 1 <= v <= SENSE_LIMITS[name]:
            raise ValueError(f"the device estimate (rom_poly_sense) needs 1 <= {name} <= {SENSE_LIMITS[name]}, got {name} = {v}: "
                             "use device=False (the host iteration)")


def _residual(Gr, y, F):
    """rho = y - F G_r^T (B, r) and f = |rho|^2 (B,), both formed in long double and rounded to fp64.  Off the manifold |rho| is a
    few percent of |G_r phi|: in plain fp64 the rounding of G_r phi and of the sum of squares puts noise of eps |rho| |G_r phi|
    on f, the acceptance f_new < f is decided by rounding once a step gains less than that, and the final t is reproducible to
    1e-9 only -- correctly rounded, to a few 1e-11 (rom_sense.hip does the same in double-double arithmetic).  Where long double
    is fp64 this is the plain fp64 residual."""
    LD = np.longdouble
    rho = (y.astype(LD) - F.astype(LD) @ Gr.T.astype(LD)).astype(np.float64)
    r2 = rho.astype(LD)
    return rho, (r2 * r2).sum(axis=1).astype(np.float64)


def _sense_batch(Gr, features, y, perp2, scale, T0, lo, hi, free, max_iter, misfit_tol):
    """``sense_scores`` / ``mlp_sense_scores`` for one batch of queries: y (K, r), perp2, scale (K,), T0 (K, t, m);
    ``features(t, jacobian)`` -> (psi (B, P), d psi / d t (B, P, m) or None), the model."""
    K, t, m = T0.shape
    B = K * t
    kf = int(free.sum())
    y, perp2, scale = np.repeat(y, t, axis=0), np.repeat(perp2, t), np.repeat(scale, t)
    th = np.clip(T0.reshape(B, m), lo, hi)
    F, _ = features(th, False)
    rho, f = _residual(Gr, y, F)
    lam = np.full(B, 1e-3)
    active = np.ones(B, dtype=bool)
    stationary = np.zeros(B, dtype=bool)
    iterations = np.zeros(B, dtype=np.int64)
    for _ in range(int(max_iter)):
        ia = np.flatnonzero(active)
        if ia.size == 0:
            break
        iterations[ia] += 1
        _, dF = features(th[ia], True)
        Ja = -np.einsum("rp,bpj->brj", Gr, dF[:, :, free])     # the free columns only: a pinned coordinate has none
        JtJ = np.einsum("bmq,bmp->bqp", Ja, Ja)
        g = np.einsum("bmq,bm->bq", Ja, rho[ia])
        dJ = np.einsum("bqq->bq", JtJ)
        todo = np.ones(ia.size, dtype=bool)
        for _trial in range(8):
            it = np.flatnonzero(todo)
            if it.size == 0:
                break
            damp = lam[ia[it], None] * (dJ[it] + 1e-300) + 1e-30 * dJ[it].max(axis=1, keepdims=True, initial=0.0)
            H = JtJ[it] + damp[:, :, None] * np.eye(kf)
            step = np.zeros((it.size, m))
            step[:, free] = -np.linalg.solve(H, g[it][..., None])[..., 0]
            new = np.clip(th[ia[it]] + step, lo, hi)
            moved = np.abs(new - th[ia[it]]).max(axis=1)
            Fn, _ = features(new, False)
            rn, fn = _residual(Gr, y[ia[it]], Fn)
            ok = fn < f[ia[it]]
            still = moved <= 1e-13 * (1.0 + np.abs(new).max(axis=1))
            acc = ia[it[ok]]
            th[acc], rho[acc], f[acc] = new[ok], rn[ok], fn[ok]
            lam[acc] = np.maximum(lam[acc] / 3.0, 1e-12)
            lam[ia[it[~ok]]] *= 4.0
            # a step that no longer moves t (accepted: below 1e-10 relative), or a misfit at rounding level: stationary
            tiny = ok & (moved <= 1e-10 * (1.0 + np.abs(new).max(axis=1)))
            done = still | tiny | (np.sqrt(f[ia[it]] + perp2[ia[it]]) <= 1e-14 * scale[ia[it]])
            stationary[ia[it[done]]] = True
            active[ia[it[done]]] = False
            todo[it[ok | done]] = False
        stuck = ia[np.flatnonzero(todo)]     # eight increases of the damping without a decrease: a minimum to working accuracy
        stationary[stuck] = True
        active[stuck] = False
    misfit = np.sqrt(f + perp2)
    sig = np.zeros(B)
    if kf and Gr.shape[0] >= kf:             # (fewer sensor coordinates than free columns: the kf-th singular value is 0)
        _, dF = features(th, True)
        J = -np.einsum("rp,bpj->brj", Gr, dF[:, :, free])
        sig = np.linalg.svd(J, compute_uv=False)[:, -1]
    best = np.argmin(misfit.reshape(K, t), axis=1)
    pick = np.arange(K) * t + best
    conv = (stationary | (misfit <= 1e-14 * scale)) & (misfit <= misfit_tol * scale)
    return th[pick], misfit[pick], conv[pick], iterations[pick], sig[pick], best


def sense_scores(Gr, powers, P, T0, lo, hi, aux=None, max_iter=30, misfit_tol=1e-3) -> SenseResult:
    """Levenberg-Marquardt in t for  min over lo <= t <= hi of ||p - G_r phi(t)||^2 + perp2,  phi the Legendre products of the
    exponent rows ``powers`` (P, m) (``legendre_features``), J = -G_r d phi / d t: ``inverse.polish_parameters`` with this model,
    pure NumPy, batched over the queries (in batches of 4,096 systems); the specification of ``rom_poly_sense``.  Gr (r, P) and
    the queries P (K, r) in reduced sensor coordinates (``inverse.reduce_sensors`` / ``reduce_measurements`` of the sensing
    matrix), aux (K, 2) = (perp2, scale) or None: 0 and max|p|.  T0 (K, m) or (K, t, m): the starts -- the iteration runs from
    each and keeps the smallest misfit, the lowest index among equals; t stays in the box [lo, hi] (scalars or (m,)).  A
    coordinate with lo_j == hi_j is PINNED: it stays at its clipped start bit for bit, has no row or column in J^T J and no
    column in the J whose ``sigma_min`` is reported (0 when nothing is free).  ``converged``: the iteration became stationary
    (or the misfit reached rounding level) AND the final misfit is at most misfit_tol scale.  max_iter = 0 only evaluates the
    clipped starts.  The residual and its squared norm are formed in long double and rounded once (``_residual``)."""
    Gr = np.asarray(Gr, dtype=np.float64)
    powers = np.asarray(powers, dtype=np.int64)
    m = powers.shape[1]
    return _sense_queries(Gr, lambda th, jacobian: legendre_features(th, powers, jacobian), m, P, T0, lo, hi, aux, max_iter, misfit_tol)


def _sense_queries(Gr, features, m, P, T0, lo, hi, aux, max_iter, misfit_tol) -> SenseResult:
    """The part of ``sense_scores`` / ``mlp_sense_scores`` that does not know the model (``features``, as in ``_sense_batch``):
    the shapes, the box, perp2 and scale, the batches."""
    P = np.asarray(P, dtype=np.float64).reshape(-1, Gr.shape[0])
    K = len(P)
    T0 = np.asarray(T0, dtype=np.float64).reshape(K, -1, m)
    t = T0.shape[1]
    lo, hi = np.broadcast_to(np.asarray(lo, dtype=np.float64), (m,)), np.broadcast_to(np.asarray(hi, dtype=np.float64), (m,))
    free = lo < hi
    tiny = np.finfo(float).tiny
    if aux is None:
        perp2 = np.zeros(K)
        scale = np.maximum(np.abs(P).max(axis=1), tiny) if P.shape[1] else np.full(K, tiny)
    else:
        aux = np.asarray(aux, dtype=np.float64).reshape(K, 2)
        perp2, scale = aux[:, 0], np.maximum(aux[:, 1], tiny)
    step = max(1, _SENSE_CHUNK // max(t, 1))
    parts = [_sense_batch(Gr, features, P[k0:k0 + step], perp2[k0:k0 + step], scale[k0:k0 + step], T0[k0:k0 + step], lo, hi, free,
                          max_iter, misfit_tol) for k0 in range(0, K, step)]
    if not parts:
        return SenseResult(np.zeros((0, m)), np.zeros(0), np.zeros(0, dtype=bool), np.zeros(0, dtype=np.int64), np.zeros(0),
                           np.zeros(0, dtype=np.int64))
    return SenseResult(*(np.concatenate([p[i] for p in parts]) for i in range(6)))


class PolynomialSensing:
    """State estimation from point measurements on the manifold of a fitted polynomial map: the decoder u(z) = mean + z V_known +
    g(z) V_unknown of ``nonlinear_reconstruction`` is fitted to y = l(u) -- m unknowns where a linear space of that accuracy
    needs m + q.  ``pca``: a TallPCA; ``poly``: a fitted PolynomialMap from the m known to the q predicted score columns (a
    TreeMap / ForestMap is not differentiable: TypeError); the known columns are the components [known_start, known_start + m)
    and the predicted ones [unknown_start, unknown_start + q) (default: right after the known ones).

        est = PolynomialSensing(sm, pca, poly).observe(points).estimate(measurements, states=True)   # SensingEstimate
    """

    def __init__(self, sm, pca, poly, known_start=0, unknown_start=None):
        if isinstance(poly, (TreeMap, MLPMap)) or not isinstance(poly, PolynomialMap):
            raise TypeError(f"PolynomialSensing needs a PolynomialMap: {type(poly).__name__} is not differentiable")
        if poly.map_ is None:
            raise ValueError("PolynomialSensing needs a fitted PolynomialMap (fit / fit_columns comes first)")
        from . import _ffi
        self.sm, self.pca, self.poly = sm, pca, poly
        pm = poly.map_
        self.m, self.q, self.degree = pm.m, pm.q, pm.degree
        self.known_start = int(known_start)
        self.unknown_start = self.known_start + self.m if unknown_start is None else int(unknown_start)
        rows = pca.components_.rows if isinstance(pca.components_, DeviceArray) else np.shape(pca.components_)[0]
        if self.known_start < 0 or self.unknown_start < 0 or max(self.known_start + self.m, self.unknown_start + self.q) > rows:
            raise ValueError(f"PolynomialSensing: the components [{self.known_start}, {self.known_start + self.m}) and "
                             f"[{self.unknown_start}, {self.unknown_start + self.q}) are not all among the {rows} of the PCA")
        self.c, self.h, self.W = pm.download("c"), pm.download("h"), pm.download("W")
        self.powers = _ffi.poly_terms(self.m, self.degree)
        self.points = None

    def observe(self, points, weights=None, extrapolate=0.5):
        """Fix the sensors: mean and components at the points, the sensing matrix S (``sensing_matrix``), the compact SVD
        diag(w) S = U Sigma V^T truncated at sigma > 1e-12 sigma_1 (rank r), G_r = Sigma V^T on the device, and the box
        [-1 - extrapolate, 1 + extrapolate] of t (t in [-1, 1] over the training rows); a constant training column (h_j = 0)
        is pinned at t_j = 0."""
        from .inverse import reduce_sensors
        sm, ctx, m, q = self.sm, self.sm._ctx, self.m, self.q
        self.points = np.asarray(points, dtype=np.float64).reshape(-1, 2)
        ms = len(self.points)
        self.weights = np.ones(ms) if weights is None else np.asarray(weights, dtype=np.float64).reshape(ms)
        comps, mean = self.pca.components_, self.pca.mean_
        comps = comps.numpy() if isinstance(comps, DeviceArray) else np.asarray(comps, dtype=np.float64)
        mean = mean.numpy().ravel() if isinstance(mean, DeviceArray) else np.asarray(mean, dtype=np.float64).ravel()
        rows = np.vstack([mean[None, :], comps[self.known_start:self.known_start + m], comps[self.unknown_start:self.unknown_start + q]])
        E = np.asarray(sm.evaluate_solutions(self.points, rows))            # (1 + m + q, ms)
        self.e0, self.Ek, self.Eu = E[0].copy(), E[1:1 + m].T.copy(), E[1 + m:].T.copy()
        self.S = sensing_matrix(self.e0, self.Ek, self.Eu, self.c, self.h, self.W, self.powers)
        self.U, Gr, _ = reduce_sensors(self.S.T, self.weights)
        self.Gr_host, self.r = Gr, self.U.shape[1]
        self.Gr = ctx.upload(Gr)
        bound = 1.0 + float(extrapolate)
        self.lo = np.where(self.h > 0.0, -bound, 0.0)
        self.hi = np.where(self.h > 0.0, bound, 0.0)
        return self

    def _scaled(self, z):
        """t = (z - c) / h, 0 for a constant column."""
        safe = np.where(self.h > 0.0, self.h, 1.0)
        return np.where(self.h > 0.0, (z - self.c) / safe, 0.0)

    def linear_scores(self, measurements):
        """The least-squares estimate on the m known modes alone: min ||w (y - e0 - E_k z)||_2."""
        Y = np.atleast_2d(np.asarray(measurements, dtype=np.float64))
        w = self.weights
        return np.linalg.lstsq(w[:, None] * self.Ek, (w[None, :] * (Y - self.e0[None, :])).T, rcond=None)[0].T

    def estimate(self, measurements, starts=None, device=True, states=False, max_iter=30, misfit_tol=1e-3) -> SensingEstimate:
        """The known scores of the K measurement vectors (K, ms) by nonlinear least squares on the manifold, from t starts per
        vector: by default the linear least-squares estimate and the centre of the training box (t = 0); ``starts``: (K, t, m)
        scores instead.  ``device=True`` runs ``rom_poly_sense`` (ValueError outside its limits m <= 16, d <= 8, P <= 96,
        r <= 96, t <= 8), ``device=False`` the host iteration ``sense_scores``.  ``states``: decode the estimates
        (``nonlinear_reconstruction``) into a DeviceArray (None when K = 0)."""
        from .inverse import reduce_measurements
        if self.points is None:
            raise RuntimeError("PolynomialSensing.observe(points) comes first")
        ctx, m = self.sm._ctx, self.m
        Y = np.atleast_2d(np.asarray(measurements, dtype=np.float64))
        K = len(Y)
        zl = self.linear_scores(Y) if K else np.zeros((0, m))
        if starts is None:
            T0 = np.stack([self._scaled(zl), np.zeros((K, m))], axis=1)
        else:
            T0 = self._scaled(np.asarray(starts, dtype=np.float64).reshape(K, -1, m))
        t = T0.shape[1]
        Pq, aux = reduce_measurements(self.U, Y, self.weights)
        if device:
            _check_sense_limits(m, self.degree, len(self.powers), self.r, t)
            res, _ = ctx.poly_sense(m, self.degree, self.r, self.Gr, ctx.upload(Pq) if K else None, 0, self.r, K, t,
                                    ctx.upload(np.ascontiguousarray(T0)) if K else None, self.lo, self.hi,
                                    AUX=ctx.upload(aux) if K else None, max_iter=max_iter, misfit_tol=misfit_tol)
        else:
            res = sense_scores(self.Gr_host, self.powers, Pq, T0, self.lo, self.hi, aux=aux, max_iter=max_iter, misfit_tol=misfit_tol)
        z = self.c + self.h * res.t
        predicted = legendre_features(res.t, self.powers, False)[0] @ self.W.T
        S = None
        if states and K:
            S = nonlinear_reconstruction(self.pca, self.poly, z, self.known_start, self.unknown_start, download=False)
        return SensingEstimate(z, predicted, res.misfit, res.converged, res.iterations, res.sigma_min, res.start, zl, S)


# ---- sensor state estimation on the MLP manifold: rom_mlp_sense -----------------------------------------------------------

MLP_SENSE_LIMITS = dict(m=16, layers=3, width=64, r=96, t=8)   # rom_mlp_sense (csrc/rom_mlp_sense.hip)


def _check_mlp_sense_limits(m, hidden, r, t):
    hidden = tuple(int(v) for v in hidden)
    checks = [("m", m, "m"), ("layers", len(hidden), "layers")] + [("width", v, "width") for v in hidden] + [("r", r, "r"), ("t", t, "t")]
    for name, v, key in checks:
        if not 1 <= v <= MLP_SENSE_LIMITS[key]:
            raise ValueError(f"the device estimate (rom_mlp_sense) needs 1 <= {name} <= {MLP_SENSE_LIMITS[key]}, got {name} = {v} "
                             f"(hidden layers {hidden}): use device=False (the host iteration)")


def mlp_hidden_features(t, layers, activation, jacobian=True):
    """psi (B, P) = [1, t, a_L(t)] and d psi / d t (B, P, m) = [0; I; D_L] (None unless ``jacobian``) at the rows of t (B, m), in
    t's dtype, P = 1 + m + H_L: the hidden layers ``layers`` = [(W_l (outputs, inputs), b_l)] with ``activation`` "tanh",
    "logistic" or "relu", a_0 = t, a_{l+1} = sigma(W_l a_l + b_l), and in forward mode D_0 = I, D_{l+1} = diag(sigma'(a_{l+1})) W_l
    D_l with sigma' = 1 - a^2, a (1 - a), [a > 0] (as in ``mlp_loss_grad_host``)."""
    t = np.asarray(t)
    B, m = t.shape
    one = t.dtype.type(1)
    a = t
    D = np.broadcast_to(np.eye(m, dtype=t.dtype), (B, m, m)) if jacobian else None
    for W, b in layers:
        W, b = np.asarray(W, dtype=t.dtype), np.asarray(b, dtype=t.dtype)
        z = a @ W.T + b
        a = np.tanh(z) if activation == "tanh" else one / (one + np.exp(-z)) if activation == "logistic" else np.where(z > 0, z, 0 * z)
        if jacobian:
            d = one - a * a if activation == "tanh" else a * (one - a) if activation == "logistic" else (a > 0).astype(t.dtype)
            D = d[:, :, None] * np.matmul(W, D)
    psi = np.concatenate([np.ones((B, 1), dtype=t.dtype), t, a], axis=1)
    if not jacobian:
        return psi, None
    eye = np.broadcast_to(np.eye(m, dtype=t.dtype), (B, m, m))
    return psi, np.concatenate([np.zeros((B, 1, m), dtype=t.dtype), eye, D], axis=1)


def mlp_sensing_matrix(e0, Ek, Eu, c, h, y_mean, y_scale, W_out, b_out):
    """S (ms, 1 + m + H_L) with  l(mean + z V_known + g(z) V_unknown) = S psi(t),  z = c + h t,  g = y_mean + y_scale (W_out a_L(t) +
    b_out),  psi = [1; t; a_L(t)] (``mlp_hidden_features``):  S = [e0 + E_k c + E_u (y_mean + y_scale b_out) | E_k diag(h) | E_u
    diag(y_scale) W_out].  e0 (ms,) = l(mean), Ek (ms, m) and Eu (ms, q) = l(known / predicted components); c, h (m,), y_mean,
    y_scale (q,), W_out (q, H_L) and b_out (q,) of the fitted map."""
    f = lambda A: np.asarray(A, dtype=np.float64)   # noqa: E731
    e0, Ek, Eu, c, h, y_mean, y_scale, W_out, b_out = map(f, (e0, Ek, Eu, c, h, y_mean, y_scale, W_out, b_out))
    s0 = e0 + Ek @ c + Eu @ (y_mean + y_scale * b_out)
    return np.concatenate([s0[:, None], Ek * h[None, :], Eu @ (y_scale[:, None] * W_out)], axis=1)


def mlp_sense_scores(Gr, sizes, activation, WH, P, T0, lo, hi, aux=None, max_iter=30, misfit_tol=1e-3) -> SenseResult:
    """``sense_scores`` with the features psi = [1; t; last hidden layer] of the network ``sizes`` = [m, hidden ..] with
    ``activation``, WH its hidden layers' flat parameters (``_mlp_split(WH, sizes)``: all W_l, outputs x inputs row-major, then
    all b_l):  min over lo <= t <= hi of ||p - G_r psi(t)||^2 + perp2,  Gr (r, 1 + m + sizes[-1]) the reduced
    ``mlp_sensing_matrix``.  The same iteration (``_sense_batch``), arguments and result; the specification of ``rom_mlp_sense``."""
    Gr = np.asarray(Gr, dtype=np.float64)
    sizes = [int(v) for v in sizes]
    activation = "logistic" if activation == "sigmoid" else activation
    if activation not in ("tanh", "logistic", "relu"):
        raise ValueError(f"mlp_sense_scores: activation {activation!r}, one of 'tanh', 'logistic' ('sigmoid'), 'relu'")
    layers = _mlp_split(np.asarray(WH, dtype=np.float64).ravel(), sizes)
    assert Gr.shape[1] == 1 + sizes[0] + sizes[-1], f"mlp_sense_scores: Gr has {Gr.shape[1]} columns, 1 + m + H_L = {1 + sizes[0] + sizes[-1]}"
    return _sense_queries(Gr, lambda th, jacobian: mlp_hidden_features(th, layers, activation, jacobian), sizes[0], P, T0, lo, hi, aux,
                          max_iter, misfit_tol)


class MLPSensing(PolynomialSensing):
    """``PolynomialSensing`` for the decoder of a fitted ``MLPMap`` (the reference's "NN" model): the same protocol --

        est = MLPSensing(sm, pca, mlp).observe(points).estimate(measurements, states=True)   # SensingEstimate

    -- with the features psi(t) = [1; t; last hidden layer] in place of the Legendre products: the output layer and the target
    scaling are part of the sensing matrix (``mlp_sensing_matrix``), the device estimate is ``rom_mlp_sense``, the host one
    ``mlp_sense_scores``.  TypeError for anything that is not an MLPMap, ValueError for an unfitted map or components out of range."""

    def __init__(self, sm, pca, mlp, known_start=0, unknown_start=None):
        if not isinstance(mlp, MLPMap):
            raise TypeError(f"MLPSensing needs an MLPMap, not {type(mlp).__name__} (PolynomialSensing takes a PolynomialMap)")
        if mlp.map_ is None:
            raise ValueError("MLPSensing needs a fitted MLPMap (fit / fit_columns comes first)")
        self.sm, self.pca, self.poly = sm, pca, mlp
        pm = mlp.map_
        self.m, self.q, self.activation = pm.m, pm.q, pm.activation
        self.hidden = tuple(pm.layout["sizes"][1:-1])
        self.known_start = int(known_start)
        self.unknown_start = self.known_start + self.m if unknown_start is None else int(unknown_start)
        rows = pca.components_.rows if isinstance(pca.components_, DeviceArray) else np.shape(pca.components_)[0]
        if self.known_start < 0 or self.unknown_start < 0 or max(self.known_start + self.m, self.unknown_start + self.q) > rows:
            raise ValueError(f"MLPSensing: the components [{self.known_start}, {self.known_start + self.m}) and "
                             f"[{self.unknown_start}, {self.unknown_start + self.q}) are not all among the {rows} of the PCA")
        self.c, self.h, self.y_mean, self.y_scale = (pm.download(part) for part in ("c", "h", "y_mean", "y_scale"))
        w, lay = pm.download("w"), pm.layout
        nl, sizes = lay["layers"], lay["sizes"]
        self.W_out = w[lay["w_offsets"][-1]:lay["w_offsets"][-1] + sizes[-1] * sizes[-2]].reshape(sizes[-1], sizes[-2]).copy()
        self.b_out = w[lay["b_offsets"][-1]:lay["b_offsets"][-1] + sizes[-1]].copy()
        # the hidden layers alone, in the flat order of _mlp_split(., [m, *hidden])
        self.WH = np.concatenate([w[lay["w_offsets"][l]:lay["w_offsets"][l] + sizes[l + 1] * sizes[l]] for l in range(nl - 1)] +
                                 [w[lay["b_offsets"][l]:lay["b_offsets"][l] + sizes[l + 1]] for l in range(nl - 1)])
        self.sizes = [self.m, *self.hidden]
        self.layers = _mlp_split(self.WH, self.sizes)
        self.points = None

    def _sensing_matrix(self):
        return mlp_sensing_matrix(self.e0, self.Ek, self.Eu, self.c, self.h, self.y_mean, self.y_scale, self.W_out, self.b_out)

    def observe(self, points, weights=None, extrapolate=0.5):
        """As ``PolynomialSensing.observe``, with the sensing matrix ``mlp_sensing_matrix``; the hidden weights go to the device."""
        from .inverse import reduce_sensors
        sm, ctx, m, q = self.sm, self.sm._ctx, self.m, self.q
        self.points = np.asarray(points, dtype=np.float64).reshape(-1, 2)
        ms = len(self.points)
        self.weights = np.ones(ms) if weights is None else np.asarray(weights, dtype=np.float64).reshape(ms)
        comps, mean = self.pca.components_, self.pca.mean_
        comps = comps.numpy() if isinstance(comps, DeviceArray) else np.asarray(comps, dtype=np.float64)
        mean = mean.numpy().ravel() if isinstance(mean, DeviceArray) else np.asarray(mean, dtype=np.float64).ravel()
        rows = np.vstack([mean[None, :], comps[self.known_start:self.known_start + m], comps[self.unknown_start:self.unknown_start + q]])
        E = np.asarray(sm.evaluate_solutions(self.points, rows))            # (1 + m + q, ms)
        self.e0, self.Ek, self.Eu = E[0].copy(), E[1:1 + m].T.copy(), E[1 + m:].T.copy()
        self.S = self._sensing_matrix()
        self.U, Gr, _ = reduce_sensors(self.S.T, self.weights)
        self.Gr_host, self.r = Gr, self.U.shape[1]
        self.Gr, self.WH_dev = ctx.upload(Gr), ctx.upload(self.WH)
        bound = 1.0 + float(extrapolate)
        self.lo = np.where(self.h > 0.0, -bound, 0.0)
        self.hi = np.where(self.h > 0.0, bound, 0.0)
        return self

    def predict_scores(self, t):
        """y_mean + y_scale net(t): the predicted scores at the scaled coordinates t (K, m)."""
        a = mlp_hidden_features(np.asarray(t, dtype=np.float64).reshape(-1, self.m), self.layers, self.activation, False)[0][:, 1 + self.m:]
        return self.y_mean + self.y_scale * (a @ self.W_out.T + self.b_out)

    def estimate(self, measurements, starts=None, device=True, states=False, max_iter=30, misfit_tol=1e-3) -> SensingEstimate:
        """As ``PolynomialSensing.estimate``: ``device=True`` runs ``rom_mlp_sense`` (ValueError outside ``MLP_SENSE_LIMITS``),
        ``device=False`` the host iteration ``mlp_sense_scores``; predicted_scores = y_mean + y_scale net(t)."""
        from .inverse import reduce_measurements
        if self.points is None:
            raise RuntimeError("MLPSensing.observe(points) comes first")
        ctx, m = self.sm._ctx, self.m
        Y = np.atleast_2d(np.asarray(measurements, dtype=np.float64))
        K = len(Y)
        zl = self.linear_scores(Y) if K else np.zeros((0, m))
        if starts is None:
            T0 = np.stack([self._scaled(zl), np.zeros((K, m))], axis=1)
        else:
            T0 = self._scaled(np.asarray(starts, dtype=np.float64).reshape(K, -1, m))
        t = T0.shape[1]
        Pq, aux = reduce_measurements(self.U, Y, self.weights)
        if device:
            _check_mlp_sense_limits(m, self.hidden, self.r, t)
            res, _ = ctx.mlp_sense(m, self.hidden, self.activation, self.WH_dev, self.r, self.Gr, ctx.upload(Pq) if K else None, 0,
                                   self.r, K, t, ctx.upload(np.ascontiguousarray(T0)) if K else None, self.lo, self.hi,
                                   AUX=ctx.upload(aux) if K else None, max_iter=max_iter, misfit_tol=misfit_tol)
        else:
            res = mlp_sense_scores(self.Gr_host, self.sizes, self.activation, self.WH, Pq, T0, self.lo, self.hi, aux=aux,
                                   max_iter=max_iter, misfit_tol=misfit_tol)
        z = self.c + self.h * res.t
        S = None
        if states and K:
            S = nonlinear_reconstruction(self.pca, self.poly, z, self.known_start, self.unknown_start, download=False)
        return SensingEstimate(z, self.predict_scores(res.t), res.misfit, res.converged, res.iterations, res.sigma_min, res.start, zl, S)
