"""Host-side checks of the polynomial maps (no GPU): the C entries are exported and bound, the argument checks that need no
device answer, rom_poly_terms is scikit-learn's exponent list, and the 80-bit least squares of tests/poly_truth.py -- the
truth of tests/test_gpu_poly_map.py -- reproduces an exactly representable polynomial."""
import ctypes as C
from math import comb

import numpy as np
import pytest

import poly_truth as pt
from romhighcontrast_amd import _ffi

ENTRIES = {"rom_poly_terms": 4, "rom_poly_fit": 14, "rom_poly_predict": 12, "rom_poly_query": 2, "rom_poly_download": 4,
           "rom_poly_destroy": 1}
SHAPES = [(4, 4), (3, 2), (12, 2), (1, 8), (6, 3)]


def test_entry_points_are_exported_and_bound():
    lib = C.CDLL(_ffi.LIB_PATH)
    for name, nargs in ENTRIES.items():
        assert name in _ffi.PROTOTYPES and hasattr(lib, name), name
        res, args = _ffi.PROTOTYPES[name]
        assert res is C.c_int and len(args) == nargs, name
    assert hasattr(_ffi.Context, "poly_fit") and hasattr(_ffi.PolyMap, "predict")


def test_null_context_is_an_invalid_argument():
    lib = _ffi.load_library()
    h, info = C.c_void_p(), np.zeros(8)
    st = lib.rom_poly_fit(None, None, 0, 4, 4, None, 0, 4, 4, 10, 2, 0.0, C.byref(h), info.ctypes.data)
    assert st == 1                                          # ROM_ERR_INVALID
    assert "rom_poly_fit" in _ffi.last_error() and "null" in _ffi.last_error()
    st = lib.rom_poly_predict(None, None, 0, 4, 10, None, 0, 4, None, 0, 4, None)
    assert st == 1 and "rom_poly_predict" in _ffi.last_error() and "null" in _ffi.last_error()


@pytest.mark.parametrize("m,d", SHAPES)
def test_terms_are_scikit_learns_powers(m, d):
    from sklearn.preprocessing import PolynomialFeatures
    want = PolynomialFeatures(degree=d).fit(np.zeros((1, m))).powers_
    got = _ffi.poly_terms(m, d)
    assert got.shape == (comb(m + d, d), m) and np.array_equal(got, want)
    assert np.array_equal(pt.powers(m, d), want)            # (the helper of the GPU tests lists the same rows)


def test_too_many_terms_are_refused():
    lib = _ffi.load_library()
    P = C.c_int(0)
    assert lib.rom_poly_terms(4, 5, C.byref(P), None) == 1  # C(9, 5) = 126 terms
    assert "rom_poly_terms" in _ffi.last_error() and "96" in _ffi.last_error() and "126" in _ffi.last_error()
    assert lib.rom_poly_terms(17, 1, C.byref(P), None) == 1 and "m = 17" in _ffi.last_error()
    assert lib.rom_poly_terms(2, 9, C.byref(P), None) == 1 and "d = 9" in _ffi.last_error()
    assert lib.rom_poly_terms(12, 2, C.byref(P), None) == 0 and P.value == 91


def test_long_double_least_squares_is_exact_on_a_dyadic_grid():
    # a polynomial with small dyadic coefficients on the grid {-1, -1/2, 0, 1/2, 1}^2: features, targets and the solution are
    # exactly representable, so the 80-bit solve may only differ from it by its own rounding (eps_80 = 2^-64 = 5e-20)
    g = np.array([-1.0, -0.5, 0.0, 0.5, 1.0])
    X = np.array([[a, b] for a in g for b in g])
    pw = pt.powers(2, 3)
    c, h = pt.midrange(X)
    assert np.array_equal(c, [0.0, 0.0]) and np.array_equal(h, [1.0, 1.0])
    Phi = pt.features(X, c, h, pw, dtype=pt.LD)
    assert Phi.dtype == pt.LD and Phi.shape == (25, 10)
    # L_2(1/2) = -1/8, L_3(1/2) = -7/16: the recurrence is exact on this grid
    j2, j3 = pw.tolist().index([2, 0]), pw.tolist().index([3, 0])
    row = X.tolist().index([0.5, 0.0])
    assert Phi[row, j2] == pt.LD(-0.125) and Phi[row, j3] == pt.LD(-0.4375)
    W = np.array([[1.0, -0.5, 0.25, 2.0, -1.0, 0.5, 0.125, -0.25, 1.5, -2.0],
                  [0.0, 1.0, 0.0, 0.0, 0.5, 0.0, 0.0, 0.0, 0.0, 0.25]]).T
    Y = (Phi @ W.astype(pt.LD))
    got, kept = pt.lstsq_ld(Phi, Y)
    assert kept.all()
    assert float(np.abs(got - W).max()) <= 1e-17
    # a dependent column gets a zero coefficient and the fit stays exact
    Phi2 = np.hstack((Phi, Phi[:, 1:2] + Phi[:, 2:3]))
    got2, kept2 = pt.lstsq_ld(Phi2, Y)
    assert kept2.tolist() == [True] * 10 + [False] and not got2[10].any() and float(np.abs(got2[:10] - W).max()) <= 1e-17


def test_names_import_from_the_reference_path():
    from src.experiments.NonLinearROM import PolynomialMap, learn_eigenvalues_device, nonlinear_reconstruction  # noqa: F401
    from romhighcontrast_amd.nonlinear import learn_eigenvalues
    assert learn_eigenvalues_device(1).__name__ == "LR device"
    assert learn_eigenvalues_device(2).__name__ == "Quadratic LR device"
    assert learn_eigenvalues(PolynomialMap(4)).__name__ == "Degree 4 LR device"
