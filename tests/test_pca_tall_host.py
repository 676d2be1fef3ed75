"""Host-side checks of the tall-block PCA feature (no GPU): the C entry is exported and bound, its argument checks answer
without a device, and the device-independent parts of romhighcontrast_amd/nonlinear.py (the reference's
src/experiments/NonLinearROM.py) do what the reference's do."""
import ctypes as C

import numpy as np

from romhighcontrast_amd import _ffi


def test_entry_point_is_exported_and_bound():
    assert "rom_pca_tall" in _ffi.PROTOTYPES
    lib = C.CDLL(_ffi.LIB_PATH)
    assert hasattr(lib, "rom_pca_tall")
    res, args = _ffi.PROTOTYPES["rom_pca_tall"]
    assert res is C.c_int and len(args) == 14


def test_null_context_is_an_invalid_argument():
    lib = _ffi.load_library()
    sigma, info = np.zeros(4), np.zeros(8)
    st = lib.rom_pca_tall(None, None, 0, 10, 4, 4, 1, None, 0, None, 0, None, sigma.ctypes.data, info.ctypes.data)
    assert st == 1                                          # ROM_ERR_INVALID
    assert "rom_pca_tall" in _ffi.last_error() and "null" in _ffi.last_error()


def test_known_unknown_indexes_against_hand_written_lists():
    from romhighcontrast_amd.nonlinear import MWhere, get_known_unknown_indexes
    P = np.zeros((5, 10))
    w = MWhere(0, 4)                                        # m = 0 known coordinates, starting at 4
    assert (w.m, w.start) == (0, 4)
    k, u = get_known_unknown_indexes(w, P, True)
    assert k.tolist() == [] and u.tolist() == [4, 5, 6, 7, 8, 9]
    k, u = get_known_unknown_indexes(w, P, False)
    assert k.tolist() == [] and u.tolist() == [0, 1, 2, 3, 4, 5, 6, 7, 8, 9]
    k, u = get_known_unknown_indexes(w, P, True, only_j=2)
    assert k.tolist() == [] and u.tolist() == [4, 5]
    k, u = get_known_unknown_indexes(w, P, False, only_j=2)
    assert k.tolist() == [] and u.tolist() == [0, 1, 2, 3, 4, 5]
    w = MWhere(2, 3)                                        # coordinates 3 and 4 are known
    k, u = get_known_unknown_indexes(w, P, True)
    assert k.tolist() == [3, 4] and u.tolist() == [5, 6, 7, 8, 9]
    k, u = get_known_unknown_indexes(w, P, False)
    assert k.tolist() == [3, 4] and u.tolist() == [0, 1, 2, 5, 6, 7, 8, 9]
    k, u = get_known_unknown_indexes(w, P, True, only_j=1)
    assert k.tolist() == [3, 4] and u.tolist() == [5]
    k, u = get_known_unknown_indexes(w, P, False, only_j=3)
    assert k.tolist() == [3, 4] and u.tolist() == [0, 1, 2, 5, 6, 7]
    k, u = get_known_unknown_indexes(w, P, True, only_j=0)
    assert k.tolist() == [3, 4] and u.tolist() == []


def test_parameter_draw_is_the_reference_draw():
    from romhighcontrast_amd.nonlinear import draw_parameters
    n_max, geometry, lo, hi = 37, (2, 3), 1, 100
    a = draw_parameters(n_max, geometry, lo, hi)
    np.random.seed(42)
    cols = [np.random.uniform(lo, hi, n_max) for _ in range(int(np.prod(geometry)))]
    want = [np.reshape(c, geometry) for c in zip(*cols)]
    assert len(a) == n_max and all(x.shape == geometry and np.array_equal(x, y) for x, y in zip(a, want))
    assert a[5][1, 2] == cols[5][5] and a[5][0, 1] == cols[1][5]


def test_tall_pca_arithmetic():
    from romhighcontrast_amd.lib.ReducedBasis import TallPCA
    sig = np.array([4.0, 2.0, 1.0, 0.0])
    p = TallPCA(np.eye(4), sig, np.zeros(4), n_samples=17, resolved_modes=3)
    assert np.array_equal(p.explained_variance_, sig ** 2 / 16.0)
    assert np.array_equal(p.explained_variance_ratio_, (sig ** 2 / 16.0) / (21.0 / 16.0))
    assert p.n_components_ == 4 and p.n_samples_ == 17 and p.resolved_modes_ == 3
    z = TallPCA(np.eye(2), np.zeros(2), np.zeros(2), n_samples=5, resolved_modes=0)
    assert not z.explained_variance_ratio_.any()


def test_learn_eigenvalues_fits_train_rows_and_scores_test_rows():
    from romhighcontrast_amd.nonlinear import MWhere, learn_eigenvalues

    class Linear:                                           # least squares with an intercept, scikit-learn's protocol
        steps = [("Quadratic", None), ("LR", None)]

        def fit(self, X, y):
            A = np.hstack((X, np.ones((len(X), 1))))
            self.coef = np.linalg.lstsq(A, y, rcond=None)[0]
            self.seen = (X.copy(), y.copy())
            return self

        def predict(self, X):
            return np.hstack((X, np.ones((len(X), 1)))) @ self.coef

    rng = np.random.default_rng(0)
    P = rng.standard_normal((60, 6))
    P[:, 4] = 2 * P[:, 0] - P[:, 1] + 3                      # column 4 is an affine function of the known ones
    model = Linear()
    f = learn_eigenvalues(model)
    assert f.__name__ == "Quadratic LR"
    out = f(n_train=40, n_test=10, pca_projections=P, mwhere=MWhere(m=2, start=0), only_j=3)
    assert np.array_equal(model.seen[0], P[10:50, :2]) and np.array_equal(model.seen[1], P[10:50, 2:5])
    assert out["error"].shape == (10, 3) and np.abs(out["error"][:, 2]).max() < 1e-12


def test_names_import_from_the_reference_path():
    from src.experiments.NonLinearROM import (MWhere, ZERO, Bounds, do_pca, get_known_unknown_indexes,  # noqa: F401
                                              learn_eigenvalues, vn_family_sampler)
    from src.lib.ReducedBasis import TallPCA, pca_tall  # noqa: F401
    assert MWhere._fields == ("m", "start") and Bounds._fields == ("lower", "upper") and ZERO == 1e-15
