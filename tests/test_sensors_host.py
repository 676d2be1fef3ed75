"""The host side of the PBDW sensor selection: ``sensor_beta_prefix`` turns the greedy's A (A[j, i] = <psi_j, w_i>, dead
basis rows as zero columns) into beta(V_n, W_j) for every j and applies ``beta_target``.  Checked against direct SVDs
and against the principal angles between the two subspaces (no GPU)."""
import numpy as np
import pytest
import scipy.linalg as sla

from romhighcontrast_amd.lib.ReducedBasis import SensorSelection, sensor_beta_prefix


def _orthonormal_pair(rng, d, n, k):
    """An orthonormal basis w (n, d) of V and psi (k, d) of W in R^d, and A = psi w^T."""
    w = np.linalg.qr(rng.standard_normal((d, n)))[0].T
    psi = np.linalg.qr(rng.standard_normal((d, k)))[0].T
    return w, psi, psi @ w.T


@pytest.mark.parametrize("d,n,k", [(40, 1, 5), (60, 6, 20), (80, 12, 12), (50, 3, 30)])
def test_beta_prefix_against_svd_and_principal_angles(d, n, k):
    rng = np.random.default_rng(d + n + k)
    w, psi, A = _orthonormal_pair(rng, d, n, k)
    beta, kk, reached = sensor_beta_prefix(A, n)
    assert kk == k and not reached and beta.shape == (k,)
    assert np.all(beta[:n - 1] == 0.0)
    for j in range(n, k + 1):
        ref = np.linalg.svd(A[:j], compute_uv=False)[-1]
        assert abs(beta[j - 1] - ref) <= 1e-14
        # beta(V, W_j) = cos of the largest principal angle between V and W_j (dim W_j >= dim V)
        ang = sla.subspace_angles(w.T, psi[:j].T)
        assert abs(beta[j - 1] - np.cos(np.max(ang))) <= 1e-12
    # nested sensor spaces: beta never decreases
    assert np.all(np.diff(beta[n - 1:]) >= -1e-14)


def test_beta_prefix_dead_columns():
    rng = np.random.default_rng(3)
    _, _, A = _orthonormal_pair(rng, 50, 5, 15)
    Ad = np.zeros((15, 8))
    live = [0, 2, 3, 6, 7]
    Ad[:, live] = A
    beta, kk, _ = sensor_beta_prefix(Ad, 5)
    ref, _, _ = sensor_beta_prefix(A, 5)
    assert kk == 15
    np.testing.assert_allclose(beta, ref, rtol=0, atol=1e-14)
    for j in range(5, 16):
        assert abs(beta[j - 1] - np.linalg.svd(Ad[:j][:, live], compute_uv=False)[-1]) <= 1e-14
    # no live direction at all: beta is 0 throughout
    b0, k0, r0 = sensor_beta_prefix(np.zeros((4, 3)), 0)
    assert k0 == 4 and not r0 and np.all(b0 == 0.0)


def test_beta_target_truncation():
    rng = np.random.default_rng(7)
    _, _, A = _orthonormal_pair(rng, 30, 4, 25)
    full, k, _ = sensor_beta_prefix(A, 4)
    for j in (4, 9, 25):
        target = full[j - 1]
        first = int(np.flatnonzero(full >= target)[0]) + 1
        beta, kk, reached = sensor_beta_prefix(A, 4, beta_target=target)
        assert reached and kk == first and first <= j
        assert np.array_equal(beta, full[:kk])
    # a target above every beta keeps the whole selection and is not reached
    beta, kk, reached = sensor_beta_prefix(A, 4, beta_target=1.0 + 1e-9)
    assert kk == 25 and not reached and np.array_equal(beta, full)
    # an empty selection
    beta, kk, reached = sensor_beta_prefix(np.zeros((0, 4)), 4, beta_target=0.5)
    assert kk == 0 and not reached and beta.shape == (0,)


def test_selection_record_fields():
    assert SensorSelection._fields == ("points", "picks", "beta", "criterion", "stop_reason")
