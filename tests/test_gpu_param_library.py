"""ParameterLibrary on the GPU: geometry (2, 2), N = 8, a basis of n = 10 snapshots, a 12^4 grid library over two decades, 16
random sensors.  The search goes through the checker of tests/nearest_truth.py against the downloaded library coordinates
(which are COEF (V S) to rounding); ROM-exact queries at library parameters find themselves; the polish, the error bound and
the lifted states run on truth snapshots; a sensor set smaller than the basis (m < n) gives r = m and still answers."""
import numpy as np
import pytest

import nearest_truth as nt

pytestmark = pytest.mark.gpu
DECADES, N_BASIS = 2.0, 10


@pytest.fixture(scope="module")
def setup():
    from romhighcontrast_amd.inverse import ParameterLibrary
    from src.lib.SolutionsManagers import SolutionsManagerFEM
    sm = SolutionsManagerFEM((2, 2), 8)
    rng = np.random.default_rng(0)
    a_basis = 10.0 ** rng.uniform(0.0, DECADES, size=(N_BASIS, 2, 2))
    basis = sm.generate_solutions(a_basis)
    grid = nt.grid_library(4, 12, DECADES)
    points = rng.uniform(-0.95, 0.95, size=(16, 2))
    lib = ParameterLibrary(sm, basis, grid).observe(points)
    a_true = 10.0 ** rng.uniform(0.0, DECADES, size=(8, 2, 2))
    Y = sm.evaluate_solutions(points, sm.generate_solutions(a_true))
    return dict(sm=sm, basis=basis, a_basis=a_basis, grid=grid, points=points, lib=lib, a_true=a_true, Y=Y)


def _raw_search(lib, Y, t, mode=0):
    ctx = lib.sm._ctx
    Pq = np.ascontiguousarray((Y * lib.weights[None, :]) @ lib.U)
    idx, d2, info = ctx.nearest(lib.Qc, 0, lib.r, lib.M, ctx.upload(Pq), 0, lib.r, len(Y), lib.r, t=t, mode=mode)
    return Pq, idx, d2, info


def test_library_state(setup):
    lib = setup["lib"]
    M = 12 ** 4
    assert lib.M == M and lib.n == N_BASIS and lib.r == N_BASIS
    assert lib.a.shape == (M, 4) and lib.residual.shape == (M,) and lib.upper.shape == (M,)
    assert (lib.residual >= 0).all() and (lib.upper >= lib.residual / lib.a.max(axis=1)).all()
    coef = lib.COEF.download(shape=(M, lib.n))
    np.testing.assert_allclose(coef, nt.rom_coefficients(lib.Ahat, lib.bhat, lib.a), rtol=0, atol=1e-9 * np.abs(coef).max())
    # the library coordinates on the device are COEF (V S)
    _, S, Vt = np.linalg.svd(lib.weights[:, None] * lib.E.T, full_matrices=False)
    Qc = lib.Qc.download(shape=(M, lib.r))
    want = coef @ (Vt[:lib.r].T * S[:lib.r])
    assert np.abs(Qc - want).max() <= 1e-12 * np.abs(want).max()


def test_search_passes_the_checker(setup):
    lib = setup["lib"]
    Qc = lib.Qc.download(shape=(lib.M, lib.r))
    out = []
    for mode in (0, 1):
        Pq, idx, d2, info = _raw_search(lib, setup["Y"], 4, mode)
        nt.check_neighbours(Pq, Qc, idx, d2, 4)
        out.append((idx, d2))
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1].view(np.uint64), out[1][1].view(np.uint64))
    idx, misfit, _ = lib.search(setup["Y"], t=4)
    assert np.array_equal(idx, out[0][0]) and (np.diff(misfit, axis=1) >= 0).all()
    # the misfit reported IS the weighted misfit of that library state
    coef = lib.COEF.download(shape=(lib.M, lib.n))
    direct = np.linalg.norm(setup["Y"][:, None, :] - coef[idx] @ lib.E, axis=2)
    np.testing.assert_allclose(misfit, direct, rtol=1e-9)


def test_rom_exact_queries_at_library_parameters_find_themselves(setup):
    lib = setup["lib"]
    rows = np.random.default_rng(4).choice(lib.M, size=24, replace=False)
    Y = lib.COEF.download(shape=(lib.M, lib.n))[rows] @ lib.E
    idx, misfit, _ = lib.search(Y, t=2)
    assert np.array_equal(idx[:, 0], rows)
    assert (misfit[:, 0] <= 1e-12 * np.linalg.norm(Y, axis=1)).all(), misfit[:, 0] / np.linalg.norm(Y, axis=1)
    est = lib.estimate(Y, t=2, polish=False)
    assert np.array_equal(est.a.reshape(24, 4), lib.a[rows]) and (est.iterations == 0).all()


def test_estimate_on_truth_snapshots(setup):
    sm, lib, Y, a_true = setup["sm"], setup["lib"], setup["Y"], setup["a_true"]
    K = len(Y)
    est = lib.estimate(Y, t=4, states=True)
    assert est._fields == ("a", "misfit", "start_index", "start_misfit", "converged", "iterations", "sigma_min", "coefficients",
                           "error_bound", "states")
    assert est.a.shape == (K, 2, 2) and est.misfit.shape == (K,) and est.start_index.shape == (K, 4) and est.start_misfit.shape == (K, 4)
    assert est.converged.shape == (K,) and est.converged.dtype == bool and est.iterations.shape == (K,) and est.sigma_min.shape == (K,)
    assert est.coefficients.shape == (K, N_BASIS) and est.states.shape == (K, sm.vspace_dim)
    for part in est.error_bound:
        assert part.shape == (K,) and np.isfinite(part).all() and (part >= 0).all()
    assert (est.a >= lib.a.min() * (1 - 1e-12)).all() and (est.a <= lib.a.max() * (1 + 1e-12)).all()
    assert (est.sigma_min > 0).all()
    # the polish only ever lowers the misfit of its best start
    assert (est.misfit <= est.start_misfit[:, 0] * (1 + 1e-12)).all()
    # the lifted states are the coefficients' states: at the sensors they give E^T c
    at_sensors = sm.evaluate_solutions(setup["points"], est.states)
    np.testing.assert_allclose(at_sensors, est.coefficients @ lib.E, rtol=0, atol=1e-11 * np.abs(at_sensors).max())
    np.testing.assert_allclose(np.linalg.norm(Y - at_sensors, axis=1), est.misfit, rtol=1e-6, atol=1e-13 * np.abs(Y).max())
    err_lib = np.abs(np.log10(lib.a[est.start_index[:, 0]]) - np.log10(a_true.reshape(K, 4))).max(axis=1)
    err = np.abs(np.log10(est.a) - np.log10(a_true)).reshape(K, 4).max(axis=1)
    print(f"max |log10 a_est - log10 a|: library alone {np.sort(err_lib)}, with polish {np.sort(err)}; converged {est.converged}")
    # the method on the basis object is the same computation
    from src.lib.ReducedBasis import BaseReducedBasis
    rb = BaseReducedBasis()
    rb.set(setup["basis"], setup["a_basis"])
    again = rb.parameter_estimation_library(sm, setup["points"], Y, setup["grid"], t=4)
    assert np.array_equal(again.a, est.a) and np.array_equal(again.start_index, est.start_index) and again.states is None


def test_fewer_sensors_than_basis_rows(setup):
    from romhighcontrast_amd.inverse import ParameterLibrary
    sm = setup["sm"]
    grid = nt.grid_library(4, 5, DECADES)
    lib = ParameterLibrary(sm, setup["basis"], grid).observe(setup["points"][:6])
    assert lib.r == 6 and lib.E.shape == (N_BASIS, 6)
    Y = setup["Y"][:, :6]
    Pq, idx, d2, _ = _raw_search(lib, Y, 3)
    nt.check_neighbours(Pq, lib.Qc.download(shape=(lib.M, 6)), idx, d2, 3)
    est = lib.estimate(Y, t=3)
    assert est.a.shape == (len(Y), 2, 2) and np.isfinite(est.a).all() and np.isfinite(est.misfit).all()
    assert (est.misfit <= est.start_misfit[:, 0] * (1 + 1e-12)).all()
