"""Parameter estimators used by ``BaseReducedBasis.set`` (reference: src/lib/Estimators.py:24-37).

O(n*k) host arithmetic on the tiny (n_basis, M) coefficient matrices -- out of scope of the GPU hot
path: the two estimators the basis objects instantiate, and ``EstimatorNN`` (:75-97), whose
regressors are device MLP maps (``nonlinear.MLPMap``: rom_mlp_fit / rom_mlp_predict).
"""
import numpy as np


class Estimator:
    def __init__(self, a_values_base):
        self.a_values_base = a_values_base

    def fit(self, c_values, a_values):
        return self

    def estimate_parameter(self, c_values):
        raise Exception("Not implemented.")


class EstimatorLinear(Estimator):
    """a_est = sum_b c[b, i] * a_base[b]  (:24-27)."""

    def estimate_parameter(self, c_values):
        return np.tensordot(np.asarray(c_values).T, np.asarray(self.a_values_base), axes=(1, 0))


class EstimatorInv(Estimator):
    """1 / a_est = sum_b c[b, i] / a_base[b]  (:30-37)."""

    def __init__(self, a_values_base):
        super().__init__(a_values_base)
        self.inv_a_values_base = 1.0 / np.array(self.a_values_base)

    def estimate_parameter(self, c_values):
        return 1.0 / np.tensordot(np.asarray(c_values).T, self.inv_a_values_base, axes=(1, 0))


class EstimatorNN(Estimator):
    """One MLP per parameter on X = c_values * a_base[:, i]  (:75-97: ``MLPRegressor(hidden_layer_sizes)`` per column of
    ``a_values_base``; here ``nonlinear.MLPMap`` with q = 1, ``mlp_kwargs`` passed on).  c_values: (samples, n_basis);
    a_values_base: (n_basis, n_parameters).  ValueError beyond the limits of the device map."""

    def __init__(self, a_values_base, hidden_layer_sizes, **mlp_kwargs):
        super().__init__(a_values_base)
        from .. import _ffi
        from ..nonlinear import MLPMap
        n_basis, n_par = np.shape(a_values_base)
        hidden = (hidden_layer_sizes,) if np.isscalar(hidden_layer_sizes) else tuple(hidden_layer_sizes)
        _ffi.mlp_layout(n_basis, hidden, 1)
        self.tree = [MLPMap(hidden_layer_sizes=hidden, **mlp_kwargs) for _ in range(n_par)]

    def tree_iterator(self, c_values):
        c_values = np.asarray(c_values, dtype=np.float64)
        for tree, a_base in zip(self.tree, np.asarray(self.a_values_base, dtype=np.float64).T):
            yield tree, c_values * a_base[None, :]

    def fit(self, c_values, a_values):
        a_values = np.asarray(a_values, dtype=np.float64)
        for i, (tree, X) in enumerate(self.tree_iterator(c_values)):
            tree.fit(X, a_values[:, i])
        return self

    def estimate_parameter(self, c_values):
        return np.array([np.asarray(tree.predict(X)).ravel() for tree, X in self.tree_iterator(c_values)]).T
