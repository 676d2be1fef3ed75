"""CPU checks behind tests/test_gpu_resid.py: on every input the GPU tests use, the plain fp64 NumPy restatement of the
residual estimator (resid_truth.NumpyEstimator: Householder QR of the functionals in H^-1 coordinates) stays at least 8x
inside the bound C eps (P + nr + nc) S that the device code is held to; and on the deep case the textbook form z^T G z
violates that bound by more than 1e3, which is why it was not built."""
import numpy as np
import pytest

import resid_truth as rt


@pytest.mark.parametrize("case", rt.CASES, ids=[c[0] for c in rt.CASES])
def test_numpy_restatement_is_8x_inside_the_bound(case):
    cid, blocks, N, n, M, e, _ = case
    tr = rt.truth(blocks, N)
    a, ab = rt.case_inputs(case)
    est = rt.NumpyEstimator(tr, rt.oracle_snapshots(tr, ab))
    c = est.coefficients(a)
    d = est.delta(a, c)
    t = tr.residuals(est.W, a, c)
    bound = tr.bound(est.W, a, c)
    worst = float(np.max(np.abs(d - t) / bound))
    print(f"{cid}: P = {1 + tr.k * n}, max |delta - truth| / bound = {worst:.3e}")
    assert worst <= 1.0 / 8.0, (cid, worst)


@pytest.fixture(scope="module")
def deep():
    p = rt.DEEP
    tr = rt.truth(p["blocks"], p["N"])
    a = rt.params(p["blocks"], p["M"], p["e"], p["seed"])
    picks, crits, gaps, rows, allc, _ = tr.weak_greedy_ld(a, p["n"], weights=1.0 / a.reshape(len(a), -1).min(axis=1))
    return tr, a, picks, rows


def test_deep_case_restatement_holds_and_gram_form_fails(deep):
    tr, a, picks, rows = deep
    est = rt.NumpyEstimator(tr, rows)
    c = est.coefficients(a)
    keep = np.setdiff1d(np.arange(len(a)), picks)
    t = tr.residuals(est.W, a, c)
    bound = tr.bound(est.W, a, c)
    fnorm = tr.residuals(np.zeros((0, tr.dim)), a[:1], np.zeros((1, 0)))[0]
    print(f"deep: true residuals / ||f|| from {t[keep].min() / fnorm:.2e} to {t[keep].max() / fnorm:.2e}")
    assert t[keep].min() < 1e-9 * fnorm          # the case is deep: far below sqrt(eps) ||f||
    worst = float(np.max(np.abs(est.delta(a, c) - t)[keep] / bound[keep]))
    assert worst <= 1.0 / 8.0, worst
    gram = float(np.max(np.abs(est.gram_form(a, c) - t)[keep] / bound[keep]))
    print(f"deep: orthonormalised form {worst:.3e} of the bound, z^T G z form {gram:.3e}")
    assert gram > 1e3, gram


def test_greedy_case_has_no_close_calls():
    """The pick test of the GPU suite excludes steps whose top-two gap is below 1e-6; none of the ten may be."""
    p = rt.GREEDY
    tr = rt.truth(p["blocks"], p["N"])
    a = rt.params(p["blocks"], p["M"], p["e"], p["seed"])
    picks, crits, gaps, rows, _, _ = tr.weak_greedy_ld(a, p["n"], weights=1.0 / a.reshape(len(a), -1).min(axis=1))
    print("picks", picks, "smallest gap", gaps.min())
    assert gaps.min() > 1e-6 and len(set(picks)) == p["n"]
