"""The one A_1 Gram-Schmidt step (romb_a1_append, csrc/rom_basis.hip) behind rom_error_curves, rom_resid_append and
rom_sensor_greedy on an MI355X: the three callers orthonormalise the same rows with the same dead-row rule (a1_dead).

Six rows built from snapshots at (2,2) blocks, N = 8 (dim 225): row 3 equals row 1 exactly, row 4 is zero.  All three calls
must flag exactly those two rows; the handle's W is exactly zero there, A_1-orthonormal on the live rows, and T W (T from
the curves) gives the live input rows back.  A_1 comes from the oracle on the host.  The bounds are those
test_gpu_error_curves applies to the same basis: C n eps (1 + kappa), C = 64, kappa the condition number of the
row-normalised live rows in the A_1 norm (CGS2 loses orthogonality, and reproduces its input, to a multiple of eps kappa).
"""
import numpy as np
import pytest

from conftest import observed
from oracle import rom_oracle as ro
from test_gpu_error_curves import C_BOUND, EPS, _snapshots

pytestmark = pytest.mark.gpu

DEAD = np.array([0, 0, 0, 1, 1, 0], dtype=bool)


@pytest.fixture(scope="module")
def setup():
    blocks, N = (2, 2), 8
    sm, a, U = _snapshots(blocks, N, 40, 1e2, seed=3)
    U = np.asarray(U)
    assert U.shape[1] == 225
    C = np.vstack([U[5], U[9], U[17], U[9], np.zeros(U.shape[1]), U[23]])
    g = ro.Geometry(blocks, N)
    A1 = lambda X: ro.stencil_apply(g, np.ones(blocks), X)  # noqa: E731
    live = C[~DEAD]
    G = live @ A1(live).T
    d = np.sqrt(np.diag(G))
    w = np.linalg.eigvalsh(G / d[:, None] / d[None, :])
    kappa = float(np.sqrt(w[-1] / w[0]))
    ctx = sm._ctx
    Ub, Cb = ctx.upload(U), ctx.upload(C)
    curves = sm._fem.error_curves(Ub, len(U), Cb, len(C), ctx.upload(np.ascontiguousarray(a.reshape(len(U), -1))))
    r = sm._fem.resid(len(C))
    r.append(Cb, len(C))
    W, dead_r = r.download("W"), r.download("dead")
    r.free()
    loc = sm._locate(sm.interior_vertices())
    sensors = [sm._fem.sensor_greedy(Cb, len(C), *loc, 5, mode, 1e-10) for mode in (0, 1)]
    return dict(C=C, A1=A1, kappa=kappa, curves=curves, W=W, dead_r=dead_r, sensors=sensors)


def test_dead_flags_agree(setup):
    proj, galc, P, T, info = setup["curves"]
    assert np.array_equal(np.diag(T) == 0.0, DEAD)
    assert np.array_equal(setup["dead_r"] != 0.0, DEAD)
    assert info["dependent_rows"] == 2
    for picks, crit, A, alpha, sinfo in setup["sensors"]:
        assert sinfo["dead_rows"] == 2


def test_w_is_zero_where_dead_and_a1_orthonormal_where_live(setup):
    W, n = setup["W"], len(DEAD)
    assert np.all(W[DEAD] == 0.0)
    Wl = W[~DEAD]
    defect = np.abs(Wl @ setup["A1"](Wl).T - np.eye(len(Wl)))
    observed("a1 basis: |W A_1 W^T - I| on the live rows (bound C n eps (1 + kappa))", defect, C_BOUND * n * EPS * (1 + setup["kappa"]))


def test_t_times_w_reproduces_the_live_rows(setup):
    proj, galc, P, T, info = setup["curves"]
    C, W, A1, n = setup["C"], setup["W"], setup["A1"], len(DEAD)
    assert np.all(T[:, DEAD] == 0.0)
    D = (T @ W - C)[~DEAD]
    err = np.sqrt(np.einsum("ki,ki->k", D, A1(D)))
    norm = np.sqrt(np.einsum("ki,ki->k", C[~DEAD], A1(C[~DEAD])))
    observed("a1 basis: ||T W - C||_A / ||C||_A on the live rows (bound C n eps (1 + kappa))", err / norm,
             C_BOUND * n * EPS * (1 + setup["kappa"]))
