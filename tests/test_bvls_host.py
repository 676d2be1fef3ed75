"""bvls_host, the specification of rom_bvls, on the CPU: the Karush-Kuhn-Tucker checker of tests/bvls_truth.py on every shape,
scipy's BVLS to the permuted-host bound, a wide box against numpy.linalg.lstsq, pinned and infinite bounds, the refusals; the
checker refuses bent answers; the estimators' new keywords at None change no bit; Context.bvls has the host's signature."""
import inspect

import numpy as np
import pytest

import bvls_truth as bt
from bvls_truth import IDS, SHAPES

from romhighcontrast_amd.inverse import (BVLS_LIMITS, BvlsResult, _check_bvls_limits, bounded_lstsq, bvls_host, coefficient_box)


@pytest.fixture(scope="module")
def solved():
    out = {}
    for shape in SHAPES:
        G, P, lo, hi = bt.case(*shape)
        out[shape] = (G, P, lo, hi, bvls_host(G, P, lo, hi))
    return out


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_host_reaches_kkt(solved, shape):
    G, P, lo, hi, res = solved[shape]
    n = shape[0]
    worst = bt.check_kkt(G, P, lo, hi, res)
    print(f"kkt / bound {worst[0]:.3g}, misfit / bound {worst[1]:.3g}; passes up to {res.iterations.max()}; "
          f"{int((res.bound != 0).sum())} bound variables")
    assert res.converged.all() and (res.iterations <= 5 * n + 10).all() and (res.iterations >= 1).all()
    assert res.c.dtype == np.float64 and res.bound.dtype == np.int64 and res.iterations.dtype == np.int64
    assert (res.bound != 0).any(), "the case has no active bound"


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_host_agrees_with_scipy(solved, shape):
    from scipy.optimize import lsq_linear
    G, P, lo, hi, res = solved[shape]
    ref = np.array([lsq_linear(G, p, bounds=(lo, hi), method="bvls", tol=1e-14).x for p in P])
    bound = bt.host_bound(bt.permuted_delta(G, P, lo, hi, res), res.c)
    diff = np.abs(res.c - ref).max(axis=1)
    print(f"|c - scipy| up to {diff.max():.3g}, largest ratio to the bound {(diff / bound).max():.3g}")
    assert (diff <= bound).all(), (diff / bound).max()


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_checker_refuses_bent_answers(solved, shape):
    G, P, lo, hi, res = solved[shape]
    cases = bt.bent(res, lo, hi)
    assert len(cases) >= 3 or shape[0] == 1
    for what, wrong in cases:
        with pytest.raises(AssertionError):
            bt.check_kkt(G, P, lo, hi, wrong)
            print("accepted:", what)


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_wide_box_is_lstsq(solved, shape):
    G, P = solved[shape][:2]
    res = bvls_host(G, P, -1e3, 1e3)
    ref = np.linalg.lstsq(G, P.T, rcond=None)[0].T
    assert res.converged.all() and (res.iterations == 1).all() and (res.bound == 0).all()
    err = np.abs(res.c - ref).max() / np.abs(ref).max()
    print(f"|c - lstsq| / max|c| {err:.3g}")
    assert err <= 1e-12 * np.linalg.cond(G)
    bt.check_kkt(G, P, -1e3, 1e3, res)


def test_max_iter_zero_is_the_clipped_start(solved):
    G, P, lo, hi, _ = solved[(16, 20, 5)]
    res = bvls_host(G, P, lo, hi, max_iter=0)
    free = bvls_host(G, P, -np.inf, np.inf)
    assert np.array_equal(res.c, np.clip(free.c, lo, hi)) and (res.iterations == 0).all() and not res.converged.any()
    assert np.array_equal(res.bound, np.where(free.c <= lo, -1, np.where(free.c >= hi, 1, 0)))
    one = bvls_host(G, P, lo, hi, max_iter=1)
    assert (one.iterations == 1).all() and not one.converged.all()


def test_pinned_and_infinite_bounds(solved):
    G, P, lo, hi, _ = solved[(16, 20, 5)]
    lo, hi = lo.copy(), hi.copy()
    lo[3] = hi[3] = 0.1234567890123
    lo[5], hi[5] = -np.inf, np.inf
    lo[7] = -np.inf
    hi[9] = np.inf
    res = bvls_host(G, P, lo, hi)
    bt.check_kkt(G, P, lo, hi, res)
    assert res.converged.all()
    assert np.array_equal(res.c[:, 3].view(np.uint64), np.full(len(P), 0.1234567890123).view(np.uint64)) and (res.bound[:, 3] == -1).all()
    assert (res.bound[:, 5] == 0).all() and (res.bound[:, 7] >= 0).all() and (res.bound[:, 9] <= 0).all()
    everything = bvls_host(G, P, lo[3], lo[3])    # nothing free
    assert (everything.c == lo[3]).all() and everything.converged.all() and (everything.bound == -1).all()
    aux = np.stack([np.arange(1.0, 6.0), np.ones(5)], axis=1)
    with_aux = bvls_host(G, P, lo, hi, aux=aux)
    np.testing.assert_allclose(with_aux.misfit ** 2, res.misfit ** 2 + aux[:, 0], rtol=1e-14)
    bt.check_kkt(G, P, lo, hi, with_aux, aux=aux)


def test_refusals(solved):
    G, P, lo, hi, _ = solved[(4, 6, 5)]
    bad = hi.copy()
    bad[2] = lo[2] - 1.0
    with pytest.raises(ValueError, match="lo <= hi"):
        bvls_host(G, P, lo, bad)
    bad[2] = np.nan
    with pytest.raises(ValueError, match="NaN"):
        bvls_host(G, P, lo, bad)
    Pn = P.copy()
    Pn[1, 1] = np.inf
    with pytest.raises(ValueError, match="NaN / Inf"):
        bvls_host(G, Pn, lo, hi)
    with pytest.raises(ValueError, match="rank"):
        bvls_host(np.c_[G[:, :3], G[:, 0]], P, lo, hi)
    with pytest.raises(ValueError, match="rank"):
        bvls_host(G[:3], P[:, :3], lo, hi)
    assert BVLS_LIMITS == dict(n=64, r=96)
    _check_bvls_limits(64, 96)
    _check_bvls_limits(1, 1)
    for n, r in ((65, 70), (4, 97), (6, 4)):
        with pytest.raises(ValueError, match="device=False"):
            _check_bvls_limits(n, r)
    with pytest.raises(ValueError, match="device=False"):
        bounded_lstsq(None, np.random.default_rng(0).standard_normal((65, 80)), np.zeros((1, 80)), -1.0, 1.0)
    with pytest.raises(ValueError, match="rank"):
        bounded_lstsq(None, np.ones((2, 5)), np.zeros((1, 5)), -1.0, 1.0, device=False)


def test_bounded_lstsq_on_the_host_and_the_box():
    g = np.random.default_rng(21)
    n, m, K = 6, 9, 7
    E, w = g.standard_normal((n, m)), g.uniform(0.5, 2.0, m)
    C = g.uniform(-1.0, 1.0, (40, n))
    lo, hi = coefficient_box(C, inflate=0.25)
    np.testing.assert_allclose(lo, C.min(axis=0) - 0.25 * np.ptp(C, axis=0), rtol=1e-15)
    np.testing.assert_allclose(hi, C.max(axis=0) + 0.25 * np.ptp(C, axis=0), rtol=1e-15)
    Y = g.uniform(-2.0, 2.0, (K, n)) @ E + 0.1 * g.standard_normal((K, m))
    res = bounded_lstsq(None, E, Y, lo, hi, weights=w, device=False)
    assert isinstance(res, BvlsResult) and res.converged.all()
    # in the original coordinates: the weighted problem itself
    bt.check_kkt(w[:, None] * E.T, Y * w[None, :], lo, hi, res)
    assert (res.bound != 0).any()


def test_new_keywords_at_none_change_no_bit():
    import scipy.linalg as sla
    from romhighcontrast_amd.lib.ReducedBasis import BaseReducedBasis, pbdw_solve
    g = np.random.default_rng(5)
    m, n, K, dim = 9, 4, 6, 30
    A = g.standard_normal((m, m + 3))
    G, L, Y = A @ A.T, g.standard_normal((m, n)), g.standard_normal((K, m))
    c, d, beta = pbdw_solve(G, L, Y)
    c2, d2, _ = pbdw_solve(G, L, Y, None, bounds=None, solver=None)
    Rl = np.linalg.cholesky(G)
    B, yt = sla.solve_triangular(Rl, L, lower=True), sla.solve_triangular(Rl, Y.T, lower=True)
    Q, RB = np.linalg.qr(B)
    ref = sla.solve_triangular(RB, Q.T @ yt, lower=False)
    assert beta is None and np.array_equal(c, c2) and np.array_equal(d, d2)
    np.testing.assert_allclose(c, ref, rtol=1e-12, atol=1e-13)
    # the bounded c-step: inside the box, and the estimate still interpolates (G d + L c = y)
    lo, hi = -0.05 * np.ones(n), 0.05 * np.ones(n)
    cb, db, _ = pbdw_solve(G, L, Y, bounds=(lo, hi))
    assert ((cb >= lo[:, None]) & (cb <= hi[:, None])).all() and (np.abs(cb) == 0.05).any()
    np.testing.assert_allclose(G @ db + L @ cb, Y.T, rtol=0, atol=1e-11 * np.abs(Y).max() * np.linalg.cond(G))
    bt.check_kkt(B, yt.T, lo, hi, bvls_host(B, yt.T, lo, hi))
    cw, dw, _ = pbdw_solve(G, L, Y, bounds=(-1e6, 1e6))
    np.testing.assert_allclose(cw, c, rtol=1e-9, atol=1e-11)

    class Manager:   # state_estimation needs evaluate_solutions only
        def evaluate_solutions(self, points, basis):
            return E

    E = g.standard_normal((n, m))
    rb = BaseReducedBasis()
    rb.set(g.standard_normal((n, dim)), np.ones((n, 2, 2)))
    est = rb.state_estimation(Manager(), None, Y)
    c_ref = np.linalg.lstsq(E.T, Y.T, rcond=-1)[0]
    assert np.array_equal(est, c_ref.T @ np.array(rb.basis))
    c3, est3 = rb.state_estimation(Manager(), None, Y, return_coefs=True, bounds=None, device=True)
    assert np.array_equal(c3, c_ref) and np.array_equal(est3, est)
    Manager._ctx = None
    cb, estb = rb.state_estimation(Manager(), None, Y, return_coefs=True, bounds=(-0.2, 0.2), device=False)
    assert cb.shape == c_ref.shape and (np.abs(cb) <= 0.2).all() and np.array_equal(estb, cb.T @ np.array(rb.basis))
    from romhighcontrast_amd.lib.ReducedBasis import pbdw_state_estimation
    for fn, defaults in ((BaseReducedBasis.state_estimation, dict(bounds=None, device=True)),
                         (BaseReducedBasis.state_estimation_pbdw, dict(bounds=None)), (pbdw_state_estimation, dict(bounds=None)),
                         (pbdw_solve, dict(bounds=None, solver=None))):
        par = inspect.signature(fn).parameters
        assert {k: par[k].default for k in defaults} == defaults, fn


def test_device_call_has_the_host_signature():
    from romhighcontrast_amd._ffi import PROTOTYPES, Context
    host, dev = inspect.signature(bvls_host).parameters, inspect.signature(Context.bvls).parameters
    assert list(host) == ["G", "P", "lo", "hi", "aux", "max_iter"]
    order = [k for k in dev if k in ("Gr", "P", "lo", "hi", "AUX", "max_iter")]
    assert order == ["Gr", "P", "lo", "hi", "AUX", "max_iter"]
    assert dev["AUX"].default is None and host["aux"].default is None
    assert dev["max_iter"].default is None and host["max_iter"].default is None
    assert len(PROTOTYPES["rom_bvls"][1]) == 17
