"""Host side of the sensor state estimation on the MLP manifold: the checker of tests/mlp_sense_truth.py accepts what
mlp_sense_scores returns and rejects bent answers -- t shifted by 1e-9, a misfit off by 1e-9 relative, a wrong start, t outside
the box; the derivative features agree with long-double central differences; mlp_sensing_matrix reproduces the sensor image of
the decoder; a permutation of the hidden units leaves S psi unchanged to rounding; mlp_sense_scores recovers t* on every shape of
the device tests, also with the weights scaled by 3; Context.mlp_sense has the host's signature; MLPSensing refuses what it
cannot run and the limit check names the limit."""
import inspect

import numpy as np
import pytest

import mlp_sense_truth as mt
from mlp_sense_truth import IDS, SHAPES

REF = (4, (20, 20), "logistic", 12, 5, 3)


def test_checker_accepts_the_host_iteration():
    for max_iter in (0, 1, 2, 30):
        model, t_true, P, T0 = mt.case(*REF)
        res = mt.host_sense(model, P, T0, max_iter=max_iter)
        worst = mt.check_state(model, P, None, res, T0=T0, max_iter=max_iter)
        print(f"max_iter {max_iter}: largest observed / bound {worst:.3g}; iterations {res.iterations}")
    assert res.converged.all() and np.abs(res.t - t_true).max() <= 1e-8


def test_checker_rejects_bent_answers():
    model, _, P, T0 = mt.case(*REF)
    res = mt.host_sense(model, P, T0, max_iter=0)   # (the starts: misfits far from zero)
    mt.check_state(model, P, None, res, T0=T0, max_iter=0)
    t = res.t.copy()
    t[2, 1] += 1e-9
    with pytest.raises(AssertionError, match="misfit"):
        mt.check_state(model, P, None, res._replace(t=t))
    t = res.t.copy()
    t[2, 1] = model["hi"][1] + 1e-12
    with pytest.raises(AssertionError, match="outside the box"):
        mt.check_state(model, P, None, res._replace(t=t))
    misfit = res.misfit.copy()
    misfit[1] *= 1 + 1e-9
    with pytest.raises(AssertionError, match="misfit"):
        mt.check_state(model, P, None, res._replace(misfit=misfit))
    start = res.start.copy()
    start[3] = (start[3] + 1) % 3
    with pytest.raises(AssertionError, match="start"):
        mt.check_state(model, P, None, res._replace(start=start), T0=T0, max_iter=0)


@pytest.mark.parametrize("shape", SHAPES[:8], ids=IDS[:8])
def test_derivative_features_against_long_double_central_differences(shape):
    """Step 1e-6 in long double, the weights scaled by 3: |d psi - central difference| <= 1e-8 (1 + max|d psi|) (truncation
    h^2 |psi'''| / 6 ~ 1e-12 times the third derivative's scale, rounding 2^-63 / h ~ 1e-13).  Observed: at most 2.4e-11.  relu is
    piecewise linear: the bound holds where no unit changes sign within the step, and none does at these draws."""
    from romhighcontrast_amd.nonlinear import _mlp_split, mlp_hidden_features
    m, hidden, activation = shape[:3]
    model = mt.case(m, hidden, activation, 1, 1, 1, weight_scale=3.0)[0]
    t = np.random.default_rng(5).uniform(-1.4, 1.4, size=(3, m))
    F, dF = mlp_hidden_features(t, _mlp_split(model["WH"], model["sizes"]), activation)
    Ft, dFt = mt.features(t, model, mt.LD)
    assert F.shape == (3, 1 + m + hidden[-1]) and dF.shape == (3, 1 + m + hidden[-1], m)
    assert np.abs(F - Ft.astype(float)).max() <= 1e-13 * (1 + np.abs(F).max())
    h = mt.LD(1e-6)
    worst = 0.0
    for j in range(m):
        e = np.zeros(m, dtype=mt.LD)
        e[j] = h
        cd = (mt.features(t.astype(mt.LD) + e, model, mt.LD, jacobian=False)[0] - mt.features(t.astype(mt.LD) - e, model, mt.LD, jacobian=False)[0]) / (2 * h)
        worst = max(worst, float(np.abs(dF[:, :, j] - cd.astype(float)).max()), float(np.abs(dFt[:, :, j] - cd).max()))
    print(f"largest |d psi - central difference| {worst:.3g}, max |d psi| {np.abs(dF).max():.3g}")
    assert worst <= 1e-8 * (1 + np.abs(dF).max())


def test_sensing_matrix_is_the_sensor_image_of_the_decoder():
    from romhighcontrast_amd.nonlinear import MLPMap, _mlp_split, mlp_hidden_features, mlp_sensing_matrix
    rng = np.random.default_rng(4)
    m, hidden, q, ms, dim = 4, (20, 20), 7, 9, 30
    mean, Vk, Vu = rng.standard_normal(dim), rng.standard_normal((m, dim)), rng.standard_normal((q, dim))
    ell = rng.standard_normal((dim, ms))          # l: a state -> its ms measurements
    c, h = rng.standard_normal(m), rng.uniform(0.5, 2.0, m)
    y_mean, y_scale = rng.standard_normal(q), rng.uniform(0.5, 2.0, q)
    layers = _mlp_split(MLPMap.initial_weights([m, *hidden, q], "tanh", 3), [m, *hidden, q])
    (W_out, b_out), hidden_layers = layers[-1], layers[:-1]
    S = mlp_sensing_matrix(mean @ ell, (Vk @ ell).T, (Vu @ ell).T, c, h, y_mean, y_scale, W_out, b_out)
    assert S.shape == (ms, 1 + m + hidden[-1])
    t = rng.uniform(-1.2, 1.2, size=(6, m))
    psi = mlp_hidden_features(t, hidden_layers, "tanh", False)[0]
    z = c + h * t
    g = y_mean + y_scale * (psi[:, 1 + m:] @ W_out.T + b_out)
    direct = (mean + z @ Vk + g @ Vu) @ ell
    err = np.abs(psi @ S.T - direct).max() / np.abs(direct).max()
    print(f"|S psi - l(u(z))| / max {err:.3g}")
    assert err <= 1e-12


@pytest.mark.parametrize("shape", SHAPES[:8], ids=IDS[:8])
def test_hidden_unit_permutation_leaves_the_sensor_image_unchanged(shape):
    from romhighcontrast_amd.nonlinear import _mlp_split, mlp_hidden_features
    model, t_true, P, _ = mt.case(*shape)
    other, _ = mt.permuted(model, rows=False)
    F2 = mlp_hidden_features(t_true, _mlp_split(other["WH"], other["sizes"]), other["activation"], False)[0]
    P2 = F2 @ other["Gr"].T
    width = 1 + model["m"] + sum(model["hidden"])
    assert np.abs(P2 - P).max() <= 16 * width * mt.EPS * (np.abs(F2) @ np.abs(other["Gr"]).T).max()


@pytest.mark.parametrize("scale", [1.0, 3.0], ids=["w1", "w3"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_host_iteration_recovers_exact_coordinates(shape, scale):
    model, t_true, P, T0 = mt.case(*shape, weight_scale=scale)
    res = mt.host_sense(model, P, T0)
    if scale == 1.0:
        mt.check_state(model, P, None, res, T0=T0)
    err = np.abs(res.t - t_true).max()
    print(f"max |t - t*| {err:.3g}; iterations up to {res.iterations.max()}")
    assert res.converged.all() and err <= 1e-8


def test_pinned_coordinates_on_the_host():
    model, t_true, _, _ = mt.case(*REF)
    model["lo"][1] = model["hi"][1] = 0.25
    t_true = t_true.copy()
    t_true[:, 1] = 0.25
    P = mt.exact_queries(model, t_true)
    T0 = t_true[:, None, :] + 0.1 * np.random.default_rng(8).standard_normal((5, 3, 4))
    res = mt.host_sense(model, P, T0)
    mt.check_state(model, P, None, res, T0=T0)
    assert (res.t[:, 1] == 0.25).all() and res.converged.all() and np.abs(res.t - t_true).max() <= 1e-8
    model["lo"][:], model["hi"][:] = 0.25, 0.25    # nothing free
    res = mt.host_sense(model, P, T0)
    mt.check_state(model, P, None, res, T0=T0)
    assert (res.t == 0.25).all() and (res.sigma_min == 0.0).all()


def test_device_call_has_the_host_signature():
    from romhighcontrast_amd._ffi import Context
    from romhighcontrast_amd.nonlinear import mlp_sense_scores
    host, dev = inspect.signature(mlp_sense_scores).parameters, inspect.signature(Context.mlp_sense).parameters
    for name in ("activation", "WH", "lo", "hi", "max_iter", "misfit_tol"):
        assert dev[name].default == host[name].default and dev[name].kind == host[name].kind, name
    assert dev["AUX"].default is None and host["aux"].default is None
    names = ("Gr", "P", "T0", "lo", "hi", "AUX", "max_iter", "misfit_tol")
    assert [n for n in dev if n in names] == list(names)
    assert [n for n in dev if n in ("activation", "WH", "P")] == [n for n in host if n in ("activation", "WH", "P")]
    assert list(host) == ["Gr", "sizes", "activation", "WH", "P", "T0", "lo", "hi", "aux", "max_iter", "misfit_tol"]
    assert list(dev)[1:] == ["m", "hidden", "activation", "WH", "r", "Gr", "P", "p_off", "ldp", "K", "t", "T0", "lo", "hi", "AUX", "max_iter",
                             "misfit_tol", "OUT", "out_off", "ldo"]


def test_mlp_sensing_refuses_what_it_cannot_run():
    from romhighcontrast_amd import nonlinear as nl
    for other in (nl.TreeMap(), nl.ForestMap(), nl.PolynomialMap(2), None):
        with pytest.raises(TypeError, match="MLPMap"):
            nl.MLPSensing(None, None, other)
    with pytest.raises(ValueError, match="fitted"):
        nl.MLPSensing(None, None, nl.MLPMap((20, 20)))
    with pytest.raises(TypeError, match="not differentiable"):     # (PolynomialSensing is what it was)
        nl.PolynomialSensing(None, None, nl.MLPMap((20, 20)))
    assert nl.MLP_SENSE_LIMITS == dict(m=16, layers=3, width=64, r=96, t=8)
    nl._check_mlp_sense_limits(16, (64, 64, 64), 96, 8)
    for args, word in (((17, (20,), 4, 2), "m <= 16"), ((4, (), 4, 2), "layers <= 3"), ((4, (5, 5, 5, 5), 4, 2), "layers <= 3"),
                       ((4, (20, 65), 4, 2), "width <= 64"), ((4, (0,), 4, 2), "width <= 64"), ((4, (20,), 97, 2), "r <= 96"),
                       ((4, (20,), 6, 9), "t <= 8")):
        with pytest.raises(ValueError, match=word) as e:
            nl._check_mlp_sense_limits(*args)
        assert "device=False" in str(e.value)
