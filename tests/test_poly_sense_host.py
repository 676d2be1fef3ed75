"""Host side of the sensor state estimation on the polynomial manifold: the checker of tests/sense_truth.py accepts what
sense_scores returns and rejects bent answers -- t shifted by 1e-9, a misfit off by 1e-9 relative, a wrong start, and on the
nearly rank-deficient twin case a sigma_min taken from the eigenvalues of J^T J; the derivative features agree with long-double
central differences; sensing_matrix reproduces the sensor image of the decoder; sense_scores recovers t* on every shape of the
device tests; Context.poly_sense has the host's signature; PolynomialSensing refuses what it cannot differentiate or run."""
import inspect

import numpy as np
import pytest

import sense_truth as st

#          m   d  r   K    t
SHAPES = [(1,  1, 1,  3,   3),
          (4,  2, 6,  5,   3),
          (4,  4, 12, 5,   3),
          (16, 1, 20, 5,   3),
          (12, 2, 40, 5,   3),
          (2,  8, 5,  5,   3),
          (3,  6, 96, 6,   3),
          (4,  2, 6,  257, 1),
          (4,  2, 6,  1,   8)]
IDS = ["x".join(map(str, s)) for s in SHAPES]


def case(m, d, r, K, t):
    """The model (seed 7), t*, exact P, the starts t* + 0.1 N(0, 1) (seed 8)."""
    model = st.synth(m, d, r, 7)
    t_true, P = st.exact_queries(model, K, 7)
    T0 = t_true[:, None, :] + 0.1 * np.random.default_rng(8).standard_normal((K, t, m))
    return model, t_true, P, T0


def test_truth_powers_are_the_library_terms():
    from romhighcontrast_amd import _ffi
    for m, d in ((1, 1), (4, 2), (4, 4), (16, 1), (12, 2), (2, 8), (3, 6)):
        assert np.array_equal(st.powers(m, d), _ffi.poly_terms(m, d)), (m, d)


def test_checker_accepts_the_host_iteration():
    for max_iter in (0, 1, 2, 30):
        model, t_true, P, T0 = case(4, 2, 6, 5, 3)
        res = st.host_sense(model, P, T0, max_iter=max_iter)
        worst = st.check_state(model, P, None, res, T0=T0, max_iter=max_iter)
        print(f"max_iter {max_iter}: largest observed / bound {worst:.3g}; iterations {res.iterations}")
    assert res.converged.all() and np.abs(res.t - t_true).max() <= 1e-8


def test_checker_rejects_bent_answers():
    model, _, P, T0 = case(4, 2, 6, 5, 3)
    res = st.host_sense(model, P, T0, max_iter=0)   # (the starts: misfits far from zero)
    st.check_state(model, P, None, res, T0=T0, max_iter=0)
    t = res.t.copy()
    t[2, 1] += 1e-9
    with pytest.raises(AssertionError, match="misfit"):
        st.check_state(model, P, None, res._replace(t=t))
    t = res.t.copy()
    t[2, 1] = model["hi"][1] + 1e-12
    with pytest.raises(AssertionError, match="outside the box"):
        st.check_state(model, P, None, res._replace(t=t))
    misfit = res.misfit.copy()
    misfit[1] *= 1 + 1e-9
    with pytest.raises(AssertionError, match="misfit"):
        st.check_state(model, P, None, res._replace(misfit=misfit))
    start = res.start.copy()
    start[3] = (start[3] + 1) % 3
    with pytest.raises(AssertionError, match="start"):
        st.check_state(model, P, None, res._replace(start=start), T0=T0, max_iter=0)


def test_checker_rejects_sigma_min_from_the_normal_equations():
    model, t = st.twin_case()
    P = st.features(t + 0.05, model["powers"], jacobian=False)[0] @ model["Gr"].T
    res = st.host_sense(model, P, t, max_iter=0)
    st.check_state(model, P, None, res, T0=t, max_iter=0)
    _, dF = st.features(t, model["powers"])
    J = -model["Gr"] @ dF[0]
    sv = np.linalg.svd(J, compute_uv=False)
    gram_route = np.sqrt(np.abs(np.linalg.eigvalsh(J.T @ J)[0]))
    print(f"twin case: sigma_min {sv[-1]:.3g}, sigma_max {sv[0]:.3g}, the J^T J route is off by {abs(gram_route - sv[-1]):.3g}")
    assert sv[-1] < 1e-6 * sv[0]
    with pytest.raises(AssertionError, match="sigma_min"):
        st.check_state(model, P, None, res._replace(sigma_min=np.array([gram_route])))


@pytest.mark.parametrize("m,d", [(1, 1), (4, 2), (4, 4), (2, 8), (3, 6), (12, 2)])
def test_derivative_features_against_long_double_central_differences(m, d):
    """h = 2^-24 in long double (eps 2^-63): truncation h^2 |phi'''| / 6 and rounding 2^-63 |phi| / h are both ~ 1e-12 of the
    feature's scale; the product's derivative is accepted at 1e-10 (1 + |d phi|)."""
    from romhighcontrast_amd.nonlinear import legendre_features
    pw = st.powers(m, d)
    t = np.random.default_rng(5).uniform(-1.4, 1.4, size=(3, m))
    F, dF = legendre_features(t, pw)
    Ft, dFt = st.features(t, pw, st.LD)
    assert np.abs(F - Ft.astype(float)).max() <= 1e-13 * (1 + np.abs(F).max())
    h = st.LD(2.0) ** -24
    for j in range(m):
        e = np.zeros(m, dtype=st.LD)
        e[j] = h
        cd = (st.features(t.astype(st.LD) + e, pw, st.LD, jacobian=False)[0] - st.features(t.astype(st.LD) - e, pw, st.LD, jacobian=False)[0]) / (2 * h)
        err = np.abs(dF[:, :, j] - cd.astype(float))
        assert (err <= 1e-10 * (1 + np.abs(dF[:, :, j]))).all(), (j, err.max())
        assert (np.abs(dFt[:, :, j] - cd) <= 1e-10 * (1 + np.abs(cd))).all()


def test_sensing_matrix_is_the_sensor_image_of_the_decoder():
    from romhighcontrast_amd.nonlinear import legendre_features, sensing_matrix
    rng = np.random.default_rng(4)
    m, d, q, ms, dim = 4, 3, 7, 9, 30
    pw = st.powers(m, d)
    mean, Vk, Vu = rng.standard_normal(dim), rng.standard_normal((m, dim)), rng.standard_normal((q, dim))
    ell = rng.standard_normal((dim, ms))          # l: a state -> its ms measurements
    c, h, W = rng.standard_normal(m), rng.uniform(0.5, 2.0, m), rng.standard_normal((q, len(pw)))
    S = sensing_matrix(mean @ ell, (Vk @ ell).T, (Vu @ ell).T, c, h, W, pw)
    t = rng.uniform(-1.2, 1.2, size=(6, m))
    phi = legendre_features(t, pw, False)[0]
    z = c + h * t
    direct = (mean + z @ Vk + (phi @ W.T) @ Vu) @ ell
    assert np.abs(phi @ S.T - direct).max() <= 1e-13 * np.abs(direct).max()


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_host_iteration_recovers_exact_coordinates(shape):
    model, t_true, P, T0 = case(*shape)
    res = st.host_sense(model, P, T0)
    st.check_state(model, P, None, res, T0=T0)
    err = np.abs(res.t - t_true).max()
    print(f"max |t - t*| {err:.3g}; iterations up to {res.iterations.max()}")
    assert res.converged.all() and err <= 1e-8


def test_pinned_coordinates_on_the_host():
    model, t_true, _, _ = case(4, 2, 6, 5, 3)
    model["lo"][1] = model["hi"][1] = 0.25
    t_true = t_true.copy()
    t_true[:, 1] = 0.25
    P = st.features(t_true, model["powers"], jacobian=False)[0] @ model["Gr"].T
    T0 = t_true[:, None, :] + 0.1 * np.random.default_rng(8).standard_normal((5, 3, 4))
    res = st.host_sense(model, P, T0)
    st.check_state(model, P, None, res, T0=T0)
    assert (res.t[:, 1] == 0.25).all() and res.converged.all() and np.abs(res.t - t_true).max() <= 1e-8
    model["lo"][:], model["hi"][:] = 0.25, 0.25    # nothing free
    res = st.host_sense(model, P, T0)
    st.check_state(model, P, None, res, T0=T0)
    assert (res.t == 0.25).all() and (res.sigma_min == 0.0).all()


def test_device_call_has_the_host_signature():
    from romhighcontrast_amd._ffi import Context
    from romhighcontrast_amd.nonlinear import sense_scores
    host, dev = inspect.signature(sense_scores).parameters, inspect.signature(Context.poly_sense).parameters
    for name in ("lo", "hi", "max_iter", "misfit_tol"):
        assert dev[name].default == host[name].default and dev[name].kind == host[name].kind, name
    assert dev["AUX"].default is None and host["aux"].default is None
    order = [n for n in dev if n in ("Gr", "P", "T0", "lo", "hi", "AUX", "max_iter", "misfit_tol")]
    assert order == ["Gr", "P", "T0", "lo", "hi", "AUX", "max_iter", "misfit_tol"]
    assert [n for n in host if n != "powers"] == ["Gr", "P", "T0", "lo", "hi", "aux", "max_iter", "misfit_tol"]


def test_polynomial_sensing_refuses_what_it_cannot_run():
    from romhighcontrast_amd import nonlinear as nl
    with pytest.raises(TypeError, match="not differentiable"):
        nl.PolynomialSensing(None, None, nl.TreeMap())
    with pytest.raises(TypeError, match="not differentiable"):
        nl.PolynomialSensing(None, None, nl.ForestMap())
    with pytest.raises(ValueError, match="fitted"):
        nl.PolynomialSensing(None, None, nl.PolynomialMap(2))
    nl._check_sense_limits(16, 8, 96, 96, 8)
    for args, word in (((17, 1, 18, 4, 2), "m <= 16"), ((2, 9, 55, 4, 2), "d <= 8"), ((4, 5, 126, 4, 2), "P <= 96"),
                       ((4, 2, 15, 97, 2), "r <= 96"), ((4, 2, 15, 6, 9), "t <= 8")):
        with pytest.raises(ValueError, match=word):
            nl._check_sense_limits(*args)
