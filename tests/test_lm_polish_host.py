"""Host side of the device polish: the checker of tests/lm_truth.py accepts what polish_parameters returns on a synthetic
reduced model and rejects bent answers -- a theta past the box, a coefficient off by 1e-9 relative, a misfit off by 1e-9
relative, and on the nearly rank-deficient twin case a sigma_min taken from the eigenvalues of J^T J -- and
polish_parameters_device has the host function's signature behind `ctx`."""
import inspect

import numpy as np
import pytest

import lm_truth as lt


def _case(max_iter):
    model = lt.synth(10, 4, 6, 7)
    theta_true, P = lt.exact_queries(model, 5, 7)
    theta0 = theta_true[:, None, :] + 0.1 * np.random.default_rng(8).standard_normal((5, 3, 4))
    return model, theta_true, P, theta0, lt.host_polish(model, P, theta0, max_iter=max_iter)


def test_checker_accepts_the_host_polish():
    for max_iter in (0, 1, 2, 30):
        model, theta_true, P, theta0, res = _case(max_iter)
        worst = lt.check_state(model, P, None, res, theta0=theta0, max_iter=max_iter)
        print(f"max_iter {max_iter}: largest observed / bound {worst:.3g}; iterations {res.iterations}")
    assert res.converged.all() and np.abs(res.theta - theta_true).max() <= 1e-8


def test_checker_rejects_bent_answers():
    model, _, P, theta0, res = _case(0)   # (the starts: misfits far from zero)
    lt.check_state(model, P, None, res, theta0=theta0, max_iter=0)
    theta = res.theta.copy()
    theta[2, 1] = model["hi"][1] + 1e-12
    with pytest.raises(AssertionError, match="outside the box"):
        lt.check_state(model, P, None, res._replace(theta=theta))
    c = res.coefficients.copy()
    i = np.abs(c[3]).argmax()
    c[3, i] *= 1 + 1e-9
    with pytest.raises(AssertionError, match="does not solve"):
        lt.check_state(model, P, None, res._replace(coefficients=c))
    misfit = res.misfit.copy()
    misfit[1] *= 1 + 1e-9
    with pytest.raises(AssertionError, match="misfit"):
        lt.check_state(model, P, None, res._replace(misfit=misfit))


def test_checker_rejects_sigma_min_from_the_normal_equations():
    model, theta = lt.twin_case()
    P = lt.coefficients(model, theta + 0.05) @ model["Gr"].T
    res = lt.host_polish(model, P, theta, max_iter=0)
    lt.check_state(model, P, None, res, theta0=theta, max_iter=0)
    J, A = lt.jacobian(model, res.theta[0])
    sv = np.linalg.svd(J, compute_uv=False)
    gram_route = np.sqrt(np.abs(np.linalg.eigvalsh(J.T @ J)[0]))
    bound = 64 * lt.EPS * np.linalg.cond(A) * sv[0]
    print(f"twin case: sigma_min {sv[-1]:.3g}, sigma_max {sv[0]:.3g}, checker's bound {bound:.3g}, the J^T J route is off by "
          f"{abs(gram_route - sv[-1]):.3g}")
    assert sv[-1] < 1e-6 * sv[0]
    with pytest.raises(AssertionError, match="sigma_min"):
        lt.check_state(model, P, None, res._replace(sigma_min=np.array([gram_route])))


def test_device_polish_has_the_host_signature():
    from romhighcontrast_amd.inverse import polish_parameters, polish_parameters_device
    host, dev = inspect.signature(polish_parameters), inspect.signature(polish_parameters_device)
    assert list(dev.parameters) == ["ctx"] + list(host.parameters)
    for name, p in host.parameters.items():
        assert dev.parameters[name].default == p.default and dev.parameters[name].kind == p.kind, name
