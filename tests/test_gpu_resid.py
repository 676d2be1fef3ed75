"""GPU tests of the residual estimator (rom_resid_*) and the weak greedy (rom_weak_greedy) against the long-double truth of
tests/resid_truth.py.

Estimator tests take the coefficients c that the device returned, so what is measured is the estimator and not the
conditioning of the reduced system; the truth is r = f - A(a) W^T c in 80 bits with the device's own W.
Bound: |Delta - Delta_truth| <= C eps (P + nr + nc) S(a, c), C = 64 (absolute; tests/test_resid_host.py shows the plain
fp64 NumPy restatement at least 8x inside it on the same inputs).
"""
import pickle

import numpy as np
import pytest

from conftest import observed
import resid_truth as rt

pytestmark = pytest.mark.gpu

NAN = np.nan


@pytest.fixture(scope="module")
def ctx():
    from romhighcontrast_amd import _ffi
    return _ffi.get_context()


_SMS = {}


def _sm(blocks, N):
    from romhighcontrast_amd.lib.SolutionsManagers import SolutionsManagerFEM
    key = (tuple(blocks), N)
    if key not in _SMS:
        _SMS[key] = SolutionsManagerFEM(blocks, N)
    return _SMS[key]


def _handle(ctx, sm, basis, n_cap=None, c_row0=0):
    """An estimator of the rows of `basis`, appended from inside a larger buffer (NaN rows around them) that must come back
    unmodified."""
    basis = np.asarray(basis, dtype=np.float64).reshape(-1, sm.vspace_dim)
    n = len(basis)
    h = sm._fem.resid(n if n_cap is None else n_cap)
    if n:
        host = np.vstack([np.full((c_row0, sm.vspace_dim), NAN), basis, np.full((2, sm.vspace_dim), NAN)])
        Cb = ctx.upload(host)
        h.append(Cb, n, c_row0=c_row0)
        assert np.array_equal(Cb.download(host.size), host.ravel(), equal_nan=True), "the basis rows were modified"
    return h


def _eval(ctx, h, a, n, off=0, weights=None):
    """rom_resid_eval with every array inside a larger buffer at offset `off`, NaN sentinels around.  Returns (delta, c,
    DELTA buffer, COEF buffer)."""
    a2 = np.ascontiguousarray(np.asarray(a, dtype=np.float64).reshape(len(a), -1))
    M, k = a2.shape
    ahost = np.vstack([np.full((off, k), NAN), a2, np.full((2, k), NAN)])
    ab = ctx.upload(ahost)
    D = ctx.upload(np.full(off + M + 3, NAN))
    Cf = ctx.upload(np.full((off + M + 2) * max(n, 1), NAN))
    wb = ctx.upload(weights) if weights is not None else None
    h.eval(ab, M, n, D, weights=wb, COEF=Cf, a_row0=off, d_off=off, coef_row0=off)
    d = D.download(off + M + 3)
    c = Cf.download((off + M + 2) * max(n, 1))
    assert np.isnan(d[:off]).all() and np.isnan(d[off + M:]).all(), "DELTA sentinels"
    assert np.isnan(c[:off * n]).all() and np.isnan(c[(off + M) * n:]).all(), "COEF sentinels"
    assert np.array_equal(ab.download(ahost.size), ahost.ravel(), equal_nan=True), "the parameters were modified"
    return d[off:off + M], c[off * n:(off + M) * n].reshape(M, n), D, Cf


@pytest.mark.parametrize("case", rt.CASES, ids=[c[0] for c in rt.CASES])
def test_estimator_and_certification(ctx, case, monkeypatch):
    cid, blocks, N, n, M, e, off = case
    tr, sm = rt.truth(blocks, N), _sm(blocks, N)
    a, ab = rt.case_inputs(case)
    basis = sm.generate_solutions(ab) if n else np.zeros((0, tr.dim))
    h = _handle(ctx, sm, basis, c_row0=off)
    q = h.query()
    assert (q["n"], q["P"], q["k"], q["dim"]) == (n, 1 + tr.k * n, tr.k, tr.dim) and q["n_live"] == n and 1 <= q["rank"] <= q["P"]
    d, c, D, Cf = _eval(ctx, h, a, n, off)
    W = h.download("W")
    t = tr.residuals(W, a, c)
    bound = tr.bound(W, a, c)
    observed(f"resid {cid}: |Delta - 80-bit truth| in units of C eps (P + nr + nc) S", np.abs(d - t) / bound, 1.0)
    # same bits on a second call, and from a fresh handle whose workspace was poisoned
    d2, c2, D2, Cf2 = _eval(ctx, h, a, n, off)
    assert D.same_bits_as(D2, M, off, off) and (n == 0 or Cf.same_bits_as(Cf2, M * n, off * n, off * n))
    monkeypatch.setenv("ROMHC_POISON_WS", "1")
    h3 = _handle(ctx, sm, basis, c_row0=off)
    d3, c3, D3, Cf3 = _eval(ctx, h3, a, n, off)
    monkeypatch.delenv("ROMHC_POISON_WS")
    assert D.same_bits_as(D3, M, off, off) and (n == 0 or Cf.same_bits_as(Cf3, M * n, off * n, off * n))
    # certification: lower - slack <= ||u - u_n|| <= upper + slack against truth snapshots
    a2 = a.reshape(M, -1)
    U = sm.generate_solutions(a)
    err = tr.h10(U.astype(rt.LD) - c.astype(rt.LD) @ W.astype(rt.LD))
    slack = bound / a2.min(axis=1) + 1e-11 * tr.h10(U)
    lower, upper = d / a2.max(axis=1), d / a2.min(axis=1)
    observed(f"resid {cid}: (lower bound - error) / slack", (lower - err) / slack, 1.0)
    observed(f"resid {cid}: (error - upper bound) / slack", (err - upper) / slack, 1.0)
    # weights scale the output
    w = np.linspace(0.5, 2.0, M)
    dw, _, _, _ = _eval(ctx, h, a, n, off, weights=w)
    np.testing.assert_allclose(dw, w * d, rtol=4 * rt.EPS, atol=0)


def _abs_form_bound(tr, W, q):
    """Rounding bound of fl(w_l . fl(A_q w_i)): C eps |w_l|^T |A_q| |w_i| (the standard bound of a dot product of dim terms,
    its summation constant inside C)."""
    return rt.C * rt.EPS * (np.abs(W) @ (abs(tr.Aq[q]) @ np.abs(W).T))


@pytest.mark.parametrize("case", [rt.CASES[7], rt.CASES[8]], ids=["rect_n17", "tall_n5"])
def test_handle_invariants(ctx, case):
    import referee as rf
    cid, blocks, N, n, M, e, off = case
    tr, sm = rt.truth(blocks, N), _sm(blocks, N)
    _, ab = rt.case_inputs(case)
    h = _handle(ctx, sm, sm.generate_solutions(ab))
    q = h.query()
    R, Q, W = h.download("R"), h.download("Q"), h.download("W")
    ranks = h.download("ranks")
    assert R.shape == (q["rank"], q["P"]) and ranks[-1] == q["rank"] and np.all(np.diff(ranks) >= 0) and ranks[0] == 1
    observed(f"resid {cid}: |Q Q^T - I|", np.abs(Q @ Q.T - np.eye(len(Q))), 1e-13)
    # rows of R beyond the rank at the time of a column are zero (the nested evaluation relies on it)
    for i in range(n + 1):
        assert np.all(R[int(ranks[i]):, :1 + tr.k * i] == 0.0)
    Gh = tr.ghat(tr.functionals(W))
    rec = Gh - (R.T.astype(rt.LD) @ Q.astype(rt.LD))
    gn = np.asarray(np.sqrt((Gh * Gh).sum(axis=1)), dtype=np.float64)
    rn = np.asarray(np.sqrt((rec * rec).sum(axis=1)), dtype=np.float64)
    observed(f"resid {cid}: ||g^_j - sum_i R_ij q_i|| / (C eps (nr + nc) ||g^_j||)", rn / (rt.C * rt.EPS * (tr.gr.nr + tr.gr.nc) * gn), 1.0)
    forms = rf._energy_forms_ld(tr.g, W.astype(rt.LD))
    Ahat, bhat = h.download("Ahat"), h.download("bhat")
    for b in range(tr.k):
        observed(f"resid {cid}: |Ahat_{b} - W A_{b} W^T (80 bit)| / (C eps |W| |A_{b}| |W|^T)",
                 np.abs(Ahat[b] - np.asarray(forms[b], dtype=np.float64)) / _abs_form_bound(tr, W, b), 1.0)
    bt = np.asarray(W.astype(rt.LD) @ tr.f, dtype=np.float64)
    observed(f"resid {cid}: |bhat - W f (80 bit)| / (C eps |W| |f|)", np.abs(bhat - bt) / (rt.C * rt.EPS * (np.abs(W) @ np.abs(tr.f64))), 1.0)
    assert h.download("dead").sum() == 0


def test_duplicated_row_changes_nothing(ctx):
    case = rt.CASES[2]
    cid, blocks, N, n, M, e, off = case
    tr, sm = rt.truth(blocks, N), _sm(blocks, N)
    a, ab = rt.case_inputs(case)
    basis = sm.generate_solutions(ab)
    dup = np.vstack([basis[:3], basis[1:2], basis[3:]])   # row 3 repeats row 1
    h, hd = _handle(ctx, sm, basis), _handle(ctx, sm, dup)
    q, qd = h.query(), hd.query()
    assert qd["n"] == n + 1 and qd["n_live"] == n and q["n_live"] == n and qd["rank"] == q["rank"]
    assert list(hd.download("dead")) == [0, 0, 0, 1, 0, 0]
    d, c, _, _ = _eval(ctx, h, a, n)
    dd, cd, _, _ = _eval(ctx, hd, a, n + 1)
    assert np.all(cd[:, 3] == 0.0)
    bound = tr.bound(h.download("W"), a, c) + tr.bound(hd.download("W"), a, cd)
    observed("resid duplicate row: |Delta - Delta without it| / (sum of the two bounds)", np.abs(d - dd) / bound, 1.0)


def test_nested_evaluation(ctx):
    case = rt.CASES[3]
    cid, blocks, N, n, M, e, off = case
    tr, sm = rt.truth(blocks, N), _sm(blocks, N)
    a, ab = rt.case_inputs(case)
    basis = sm.generate_solutions(ab)
    full = _handle(ctx, sm, basis)
    for n1 in (0, 3, 17):
        part = _handle(ctx, sm, basis[:n1])
        d, c, _, _ = _eval(ctx, full, a, n1, off)
        dp, cp, _, _ = _eval(ctx, part, a, n1, off)
        bound = tr.bound(part.download("W"), a, cp)
        observed(f"resid nested n' = {n1}: |eval(n') of n = 17 - eval of n = n'| / (2 bound)", np.abs(d - dp) / (2 * bound), 1.0)


def _weak(ctx, sm, a, n_max, weights=None, rel_tol=0.0, row0=0):
    a2 = np.ascontiguousarray(a.reshape(len(a), -1))
    dim = sm.vspace_dim
    ahost = a2.copy()
    ab = ctx.upload(ahost)
    B = ctx.upload(np.full((row0 + n_max + 2, dim), NAN))
    h = sm._fem.resid(n_max)
    picks, crit, info = sm._fem.weak_greedy(ab, len(a2), n_max, h, B, weights=ctx.upload(weights) if weights is not None else None,
                                            rel_tol=rel_tol, basis_row0=row0)
    rows = B.download((row0 + n_max + 2) * dim, shape=(row0 + n_max + 2, dim))
    made = len(picks)
    assert np.isnan(rows[:row0]).all() and np.isnan(rows[row0 + made:]).all(), "BASIS sentinels"
    assert np.array_equal(ab.download(ahost.size), ahost.ravel()), "the parameters were modified"
    return picks, np.array(crit), info, rows[row0:row0 + made], h


def test_deep_case_bound_at_every_step(ctx):
    p = rt.DEEP
    tr, sm = rt.truth(p["blocks"], p["N"]), _sm(p["blocks"], p["N"])
    a = rt.params(p["blocks"], p["M"], p["e"], p["seed"])
    w = 1.0 / a.reshape(len(a), -1).min(axis=1)
    picks, crit, info, rows, h = _weak(ctx, sm, a, p["n"], weights=w)
    assert len(picks) == p["n"] and len(set(picks)) == p["n"] and info["stop_reason"] == "n_max"
    W = h.download("W")
    norms = tr.ghat_norms(W)
    fnorm = norms[0]
    worst, deepest = 0.0, np.inf
    for n1 in range(p["n"] + 1):
        d, c, _, _ = _eval(ctx, h, a, n1)
        keep = np.setdiff1d(np.arange(len(a)), picks[:n1])
        t = tr.residuals(W[:n1], a[keep], c[keep])
        bound = tr.bound(W[:n1], a[keep], c[keep], norms[:1 + tr.k * n1])
        worst = max(worst, float(np.max(np.abs(d[keep] - t) / bound)))
        deepest = min(deepest, float(t.min() / fnorm))
    print(f"deep case: true residuals down to {deepest:.2e} ||f||, worst |Delta - truth| / bound = {worst:.3e}")
    assert deepest < 1e-9
    observed("resid deep case: |Delta - 80-bit truth| / bound over all steps and unpicked parameters", worst, 1.0)


@pytest.fixture(scope="module")
def greedy_truth():
    p = rt.GREEDY
    tr = rt.truth(p["blocks"], p["N"])
    a = rt.params(p["blocks"], p["M"], p["e"], p["seed"])
    w = 1.0 / a.reshape(len(a), -1).min(axis=1)
    return (tr, a, w) + tuple(tr.weak_greedy_ld(a, p["n"], weights=w))


def test_weak_greedy_against_80bit_greedy(ctx, greedy_truth):
    tr, a, w, tpicks, tcrit, gaps, trows, _, pbound = greedy_truth
    p = rt.GREEDY
    sm = _sm(p["blocks"], p["N"])
    picks, crit, info, rows, h = _weak(ctx, sm, a, p["n"], weights=w, row0=2)
    assert np.all(gaps > 1e-6), "no step of the ten may be excluded"
    assert picks == tpicks, (picks, tpicks)
    assert len(set(picks)) == len(picks)
    assert info["picks"] == p["n"] and info["stop_reason"] == "n_max" and info["dead_rows"] == 0 and info["rank"] == h.query()["rank"]
    U = sm.generate_solutions(a[picks])
    observed("weak greedy: BASIS rows vs generate_solutions of the picks (relative H^1_0)", tr.h10(rows - U) / tr.h10(U), 1e-11)
    observed("weak greedy: |criterion - 80-bit criterion| / (bound x weight)", np.abs(crit - tcrit) / pbound, 1.0)


def test_weak_greedy_stops(ctx):
    p = rt.DEEP
    sm = _sm(p["blocks"], p["N"])
    a = rt.params(p["blocks"], p["M"], p["e"], p["seed"])
    # the 80-bit greedy says where the unweighted criterion first falls to 0.4 of the first step's (the criterion is not
    # monotone; on this input the steps around the crossing are 0.52 and 0.27 of it, far from the threshold)
    tr = rt.truth(p["blocks"], p["N"])
    tcrit = tr.weak_greedy_ld(a, 12)[1]
    expect = int(np.flatnonzero(tcrit <= 0.4 * tcrit[0])[0])
    assert 0 < expect < 12 and np.min(np.abs(tcrit / tcrit[0] - 0.4)) > 0.05
    picks, crit, info, rows, h = _weak(ctx, sm, a, 12, rel_tol=0.4)
    assert info["stop_reason"] == "rel_tol" and len(picks) == expect and info["picks"] == len(picks)
    assert info["last_criterion"] <= 0.4 * crit[0] and np.all(crit > 0.4 * crit[0])
    picks2, crit2, info2, _, _ = _weak(ctx, sm, a, len(picks))
    assert info2["stop_reason"] == "n_max" and picks2 == picks and np.array_equal(crit2, crit)
    picks3, _, info3, _, _ = _weak(ctx, sm, a[:3], 5)
    assert info3["stop_reason"] == "exhausted" and sorted(picks3) == [0, 1, 2]
    assert info["host_syncs"] > 0


def test_builder_surface(ctx, greedy_truth):
    from romhighcontrast_amd.lib.ReducedBasis import (GREEDY_FOR_GALERKIN, GREEDY_FOR_H10, GREEDY_FOR_RESIDUAL, ReducedBasisGreedy,
                                                      ResidualEstimator)
    tr, a, w, tpicks, tcrit, gaps, trows, _, pbound = greedy_truth
    p = rt.GREEDY
    sm = _sm(p["blocks"], p["N"])
    assert GREEDY_FOR_RESIDUAL == "residual"
    rb = ReducedBasisGreedy(GREEDY_FOR_RESIDUAL).build(p["n"], sm, solutions2train=None, a2train=a, criterion="bound")
    assert rb.picks == tpicks and np.asarray(rb.basis).shape == (p["n"], tr.dim) and len(rb.max_errors) == p["n"]
    assert np.array_equal(np.asarray(rb.a), a[tpicks])
    rb2 = pickle.loads(pickle.dumps(rb))
    assert rb2.picks == rb.picks and np.array_equal(rb2.basis, rb.basis)
    # "residual" and an array of ones are the same criterion
    ra = ReducedBasisGreedy(GREEDY_FOR_RESIDUAL).build(4, sm, None, a[:48], criterion="residual")
    rb3 = ReducedBasisGreedy(GREEDY_FOR_RESIDUAL).build(4, sm, np.zeros(3), a[:48], criterion=np.ones(48))
    assert ra.picks == rb3.picks and np.array_equal(ra.basis, rb3.basis)
    # the estimator object and BaseReducedBasis.error_bound agree with the raw calls
    est = ResidualEstimator(sm, rb.basis)
    b = est.bound(a[:20])
    cur = est.curves(a[:20])
    assert cur.residual.shape == (p["n"] + 1, 20) and np.array_equal(cur.residual[-1], b.residual)
    a2 = a[:20].reshape(20, -1)
    assert np.array_equal(b.lower, b.residual / a2.max(axis=1)) and np.array_equal(b.upper, b.residual / a2.min(axis=1))
    eb = rb.error_bound(sm, a[:20])
    assert np.array_equal(eb.residual, b.residual)
    eb5 = rb.error_bound(sm, a[:20], n=5)
    assert np.array_equal(eb5.residual, cur.residual[5])
    with pytest.raises(Exception, match="Not implemented greedy for"):
        ReducedBasisGreedy("foo").build(2, sm, np.zeros((2, tr.dim)), a[:2])
    with pytest.raises(ValueError):
        ReducedBasisGreedy(GREEDY_FOR_RESIDUAL).build(2, sm, None, a[:8], criterion="nope")


def test_strong_greedy_modes_unchanged_on_the_smoke_geometry(ctx):
    """The H^1_0 and Galerkin modes of the same class: the picks of the reference arithmetic and the rows of the block, bit
    for bit, and the same bits on a second build."""
    from oracle import rom_oracle as ro
    from romhighcontrast_amd.lib.ReducedBasis import GREEDY_FOR_GALERKIN, GREEDY_FOR_H10, ReducedBasisGreedy
    blocks, N, M = (2, 2), 16, 16
    sm = _sm(blocks, N)
    a = 10.0 ** np.random.default_rng(0).uniform(0, 3, size=(M,) + blocks)
    U = sm.generate_solutions(a)
    g = ro.Geometry(blocks, N)
    h1 = sm.H10norm(U)
    for mode, omode in ((GREEDY_FOR_H10, ro.GREEDY_FOR_H10), (GREEDY_FOR_GALERKIN, ro.GREEDY_FOR_GALERKIN)):
        rb = ReducedBasisGreedy(mode).build(4, sm, U, a, h1)
        if mode == GREEDY_FOR_H10:   # (the comparison of the smoke run)
            _, _, picks = ro.greedy_build(g, 4, U, a, ro.H10norm(g, U), greedy_for=omode)
            assert rb.picks == picks
        assert len(set(rb.picks)) == 4 and np.array_equal(np.asarray(rb.basis), U[rb.picks])
        rb2 = ReducedBasisGreedy(mode).build(4, sm, U, a, h1)
        assert rb2.picks == rb.picks and rb2.max_errors == rb.max_errors and np.array_equal(rb2.basis, rb.basis)
