"""state_estimation_curves (romhighcontrast_amd/lib/ReducedBasis.py) on the CPU: the state-estimation errors of every
dimension from the outputs of one error-curves call (projection curve, P, T -- here computed by the oracle in long
double) against the reference's per-n formulation (ReducedBasis.py:65-70: lstsq on the first n rows, the estimate
c^T C[:n], its oracle H^1_0 error), and the two parameter estimators on the coefficients it returns."""
import numpy as np
import pytest

from oracle import rom_oracle as ro

import referee


def _device_outputs_ld(g, C, U):
    """What rom_error_curves returns, from the exact span in long double: proj (N+1, M), P (M, N), T (N, N)."""
    Q, keep = referee.a1_orthonormal_span_ld(g, C)
    CL, UL = C.astype(referee.LD), U.astype(referee.LD)
    T = np.asarray(referee._a1_dots_ld(g, CL, Q))              # C_i = sum_j <C_i, q_j>_A q_j
    P = np.asarray(referee._a1_dots_ld(g, UL, Q))
    u2 = np.array([referee.h10_ld(g, u) ** 2 for u in UL])
    proj = np.array([np.sqrt(np.maximum(u2 - np.sum(P[:, :n] ** 2, axis=1), 0)) for n in range(len(C) + 1)])
    return (np.asarray(proj, dtype=np.float64), np.asarray(P, dtype=np.float64), np.tril(np.asarray(T, dtype=np.float64)),
            keep)


CASES = [
    # id, blocks, mesh N, snapshots, basis rows, measurement points, dependent row (index copied from row 1) or None
    ("square", (2, 2), 6, 9, 8, 12, None),
    ("rect_underdetermined", (1, 3), 5, 7, 10, 6, None),      # n > points: the minimum-norm fit
    ("square_dependent_row", (2, 2), 6, 9, 7, 12, 4),
]


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_state_estimation_curves_match_per_n_reference(case):
    from romhighcontrast_amd.lib.Estimators import EstimatorInv, EstimatorLinear
    from romhighcontrast_amd.lib.ReducedBasis import state_estimation_curves
    cid, blocks, Nm, M, n, npts, dep = case
    rng = np.random.default_rng(len(cid))
    g = ro.Geometry(blocks, Nm)
    a = 10.0 ** rng.uniform(0, 2, size=(M,) + blocks)
    U = ro.generate_solutions(g, a, "lsq")
    C = rng.standard_normal((n, g.dim))
    a_basis = 10.0 ** rng.uniform(0, 2, size=(n,) + blocks)
    if dep is not None:
        C[dep] = 2.5 * C[1]
    proj, P, T, keep = _device_outputs_ld(g, C, U)
    assert keep.sum() == n - (dep is not None)
    if dep is not None:
        assert np.all(T[:, dep] == 0) and np.all(P[:, dep] == 0)
    xr, yr = (-blocks[1] / 2, blocks[1] / 2), (-blocks[0] / 2, blocks[0] / 2)
    pts = np.column_stack([rng.uniform(*xr, npts), rng.uniform(*yr, npts)])
    meas = ro.evaluate_solutions(g, pts, U)                      # (M, points)
    E = ro.evaluate_solutions(g, pts, C)                          # (n, points)
    got = state_estimation_curves(E, meas, proj, P, T, range(1, n + 1))
    h1 = ro.H10norm(g, U)
    for k in range(1, n + 1):
        c, _ = np.linalg.lstsq(E[:k].T, meas.T, rcond=-1)[:2]    # the reference's fit (:67)
        est = c.T @ C[:k]
        ref = ro.H10norm(g, est - U)
        gc, ge = got[k]
        np.testing.assert_array_equal(gc, c)
        rel = np.abs(ge - ref) / np.maximum(ref, 1e-300)
        assert rel.max() <= 1e-12, (cid, k, rel.max())
        # the estimators see exactly the reference's coefficients
        ab = a_basis[:k]
        np.testing.assert_array_equal(EstimatorInv(ab).estimate_parameter(gc), EstimatorInv(ab).estimate_parameter(c))
        np.testing.assert_array_equal(EstimatorLinear(ab).estimate_parameter(gc), EstimatorLinear(ab).estimate_parameter(c))
        assert np.all(ge / h1 >= proj[k] / h1 * (1 - 1e-14))


def test_state_estimation_curves_empty_request():
    from romhighcontrast_amd.lib.ReducedBasis import state_estimation_curves
    assert state_estimation_curves(np.zeros((3, 4)), np.zeros((2, 4)), np.zeros((4, 2)), np.zeros((2, 3)), np.zeros((3, 3)), []) == {}
