"""ParameterLibrary.estimate(polish="device") on the GPU: geometry (2, 2), N = 8, a basis of n = 10 snapshots, a 12^4 grid library
over two decades, 16 random sensors (the shapes of tests/test_gpu_param_library.py).  The device route returns the fields and
shapes of the host route, its misfit within 1e-10 max|y| of polish=True, lifted states that give E^T c at the sensors, and the
method on the basis object agrees with the direct call; polish=True and polish=False return the same bits on a repeated call;
outside the kernel's limits the device route raises ValueError."""
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


def test_device_polish_matches_the_host_route(setup):
    sm, lib, Y = setup["sm"], setup["lib"], setup["Y"]
    K = len(Y)
    host = lib.estimate(Y, t=4, polish=True, states=True)
    dev = lib.estimate(Y, t=4, polish="device", states=True)
    assert dev._fields == host._fields
    for name in host._fields:
        if name == "error_bound":
            for ph, pd in zip(host.error_bound, dev.error_bound):
                assert pd.shape == ph.shape and np.isfinite(pd).all() and (pd >= 0).all()
        else:
            hv, dv = getattr(host, name), getattr(dev, name)
            assert dv.shape == hv.shape, (name, dv.shape, hv.shape)
            if name != "states":
                assert dv.dtype == hv.dtype, (name, dv.dtype, hv.dtype)
    assert np.array_equal(dev.start_index, host.start_index) and np.array_equal(dev.start_misfit, host.start_misfit)
    diff = np.abs(dev.misfit - host.misfit)
    print(f"|misfit_dev - misfit_host| / max|y| up to {(diff / np.abs(Y).max()).max():.3g}; |log10 a_dev - log10 a_host| up to "
          f"{np.abs(np.log10(dev.a) - np.log10(host.a)).max():.3g}; converged device {dev.converged}, host {host.converged}")
    assert (diff <= 1e-10 * np.abs(Y).max()).all()
    assert (dev.misfit <= dev.start_misfit[:, 0] * (1 + 1e-12)).all() and (dev.sigma_min > 0).all()
    assert (dev.a >= lib.a.min() * (1 - 1e-12)).all() and (dev.a <= lib.a.max() * (1 + 1e-12)).all()
    at_sensors = sm.evaluate_solutions(setup["points"], dev.states)
    np.testing.assert_allclose(at_sensors, dev.coefficients @ lib.E, rtol=0, atol=1e-11 * np.abs(at_sensors).max())
    np.testing.assert_allclose(np.linalg.norm(Y - at_sensors, axis=1), dev.misfit, rtol=1e-6, atol=1e-13 * np.abs(Y).max())
    # the same bits on a repeated call
    again = lib.estimate(Y, t=4, polish="device")
    assert np.array_equal(again.a, dev.a) and np.array_equal(again.misfit, dev.misfit) and again.states is None


def test_host_routes_are_unchanged_and_repeatable(setup):
    lib, Y = setup["lib"], setup["Y"]
    from romhighcontrast_amd.inverse import polish_parameters
    for polish in (True, False):
        one, two = lib.estimate(Y, t=4, polish=polish), lib.estimate(Y, t=4, polish=polish)
        assert np.array_equal(one.a.view(np.uint64), two.a.view(np.uint64))
        # what the route computed before the device polish existed: the search, then polish_parameters from its rows
        idx, _, _ = lib.search(Y, t=4)
        la = np.log(lib.a)
        ref = polish_parameters(lib.Ahat, lib.bhat, lib.E, Y, la[idx] if polish else la[idx[:, :1]], la.min(axis=0), la.max(axis=0),
                                weights=lib.weights, max_iter=30 if polish else 0)
        want = np.exp(ref.theta) if polish else lib.a[idx[:, 0]]
        assert np.array_equal(one.a.reshape(len(Y), 4).view(np.uint64), want.view(np.uint64))
    assert np.array_equal(lib.estimate(Y, t=4).a, lib.estimate(Y, t=4, polish=True).a)


def test_method_on_the_basis_object(setup):
    from src.lib.ReducedBasis import BaseReducedBasis
    sm, lib, Y = setup["sm"], setup["lib"], setup["Y"]
    rb = BaseReducedBasis()
    rb.set(setup["basis"], setup["a_basis"])
    via = rb.parameter_estimation_library(sm, setup["points"], Y, setup["grid"], t=4, polish="device")
    direct = lib.estimate(Y, t=4, polish="device")
    assert np.array_equal(via.a, direct.a) and np.array_equal(via.start_index, direct.start_index) and via.states is None
    assert np.array_equal(via.misfit, direct.misfit)


def test_outside_the_limits_is_an_error(setup):
    lib, Y = setup["lib"], setup["Y"]
    with pytest.raises(ValueError, match="t <= 8"):
        lib.estimate(Y, t=9, polish="device")
    with pytest.raises(ValueError, match="polish"):
        lib.estimate(Y, t=4, polish="gpu")
