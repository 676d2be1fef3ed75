"""CPU checks of the 80-bit greedy referee (tests/referee.py: greedy_ld) that tests/test_gpu_greedy_routes.py holds both
device greedy routes to: against galerkin_truth_nested (Galerkin mode), against projections formed from _a1_dots_ld
(H^1_0 mode), against an fp64 rerun of the reference's definition (the oracle's greedy_build), and on dependent picks."""
import numpy as np
import pytest

from oracle import rom_oracle as ro
import referee as rf

LD = np.longdouble


@pytest.fixture(scope="module")
def case():
    g = ro.Geometry((2, 2), 6)
    M = 14
    rng = np.random.default_rng(31)
    a = 10.0 ** rng.uniform(0, 3, size=(M, 2, 2))
    U = rng.standard_normal((M, g.nr * g.nc))
    return g, a, U


def _projection_errors_ld(g, U, C):
    """||u - P u||_A1 / ||u||_A1 for the span of the rows of C, through the A_1 Gram matrix of C and _a1_dots_ld."""
    G = rf._a1_dots_ld(g, C.astype(LD), C.astype(LD))
    b = rf._a1_dots_ld(g, C.astype(LD), U.astype(LD))               # (n, M)
    x = np.linalg.solve(np.asarray(G, dtype=np.float64), np.asarray(b, dtype=np.float64)).astype(LD)
    for _ in range(3):                                                # refinement: the residual in long double
        x += np.linalg.solve(np.asarray(G, dtype=np.float64), np.asarray(b - G @ x, dtype=np.float64)).astype(LD)
    D = U.astype(LD) - x.T @ C.astype(LD)
    return np.sqrt(np.einsum("mm->m", rf._a1_dots_ld(g, D, D))) / np.sqrt(np.einsum("mm->m", rf._a1_dots_ld(g, U.astype(LD), U.astype(LD))))


def test_greedy_ld_h10_matches_projections(case):
    g, a, U = case
    h1 = np.array([float(rf.h10_ld(g, u.astype(LD))) for u in U])
    picks = [3, 0, 11, 7, 5, 9]
    E, live = rf.greedy_ld(g, U, a, h1, picks, galerkin=False)
    assert live.all() and E.shape == (len(picks), len(U))
    np.testing.assert_allclose(np.asarray(E[0], dtype=np.float64), 1.0, rtol=2.3e-16, atol=0)
    for i in range(1, len(picks)):
        ref = _projection_errors_ld(g, U, U[picks[:i]])
        d = np.abs(np.asarray(E[i] - ref, dtype=np.float64))
        assert d.max() <= 1e-15, (i, d.max())
        assert np.asarray(E[i], dtype=np.float64)[picks[:i]].max() <= 1e-15     # a member of the span has no error


def test_greedy_ld_galerkin_matches_galerkin_truth_nested(case):
    g, a, U = case
    h1 = np.array([float(rf.h10_ld(g, u.astype(LD))) for u in U])
    picks = [3, 0, 11, 7, 5, 9, 2]
    E, live = rf.greedy_ld(g, U, a, h1, picks, galerkin=True)
    assert live.all()
    truth = rf.galerkin_truth_nested(g, a, U[picks], U, range(1, len(picks)))
    for i in range(1, len(picks)):
        d = np.abs(np.asarray(E[i], dtype=np.float64) - truth[i])
        assert d.max() <= 1e-14 * max(1.0, truth[i].max()), (i, d.max())


@pytest.mark.parametrize("mode", [ro.GREEDY_FOR_H10, ro.GREEDY_FOR_GALERKIN])
def test_greedy_ld_follows_the_fp64_definition(case, mode):
    """The oracle's greedy (the reference's definition in fp64) picks the maximum of greedy_ld's error vector at every
    iteration (to fp64 resolution) and reports its value.  Galerkin mode on snapshots: on random rows the Galerkin error
    of a picked row does not drop (its approximation solves the PDE, not the row), so the greedy picks it again."""
    g, a, U = case
    if mode == ro.GREEDY_FOR_GALERKIN:
        U = ro.generate_solutions(g, a)
    h1 = ro.H10norm(g, U)
    n = 8
    _, _, picks, errs = ro.greedy_build(g, n, U, a, h1, greedy_for=mode, return_errors=True)
    E, live = rf.greedy_ld(g, U, a, h1, picks, galerkin=mode == ro.GREEDY_FOR_GALERKIN)
    assert live.all()
    contrast = ro.get_high_contrast_coefficient(a).max() / a.min()
    tol = 1e-12 * (contrast if mode == ro.GREEDY_FOR_GALERKIN else 1.0)
    for i in range(n):
        e = np.asarray(E[i], dtype=np.float64)
        assert abs(e.max() - errs[i]) <= tol, (i, e.max(), errs[i])
        assert e[picks[i]] >= e.max() - tol


@pytest.mark.parametrize("galerkin", [False, True])
def test_greedy_ld_dependent_picks_are_zero_directions(case, galerkin):
    """A duplicate row picked again, and an exactly scaled copy of an earlier pick, enter as zero directions: the curve then
    equals the curve of the live picks alone."""
    g, a, U = case
    U2 = np.vstack((U, U[4:5], -2.0 * U[6:7]))
    a2 = np.concatenate((a, a[4:5], a[6:7]))
    M = len(U2)
    h1 = np.ones(M)
    picks = [4, M - 2, 1, 6, M - 1, 8]
    E, live = rf.greedy_ld(g, U2, a2, h1, picks, galerkin=galerkin)
    assert list(live[:-1]) == [True, False, True, True, False]
    live_picks = [4, 1, 6, 8]
    E0, live0 = rf.greedy_ld(g, U2, a2, h1, live_picks, galerkin=galerkin)
    assert live0.all()
    # iteration i of the full sequence has the span of the live picks among picks[:i]
    for i, j in ((1, 1), (2, 1), (3, 2), (4, 3), (5, 3)):
        np.testing.assert_allclose(np.asarray(E[i], dtype=np.float64), np.asarray(E0[j], dtype=np.float64), rtol=1e-15, atol=1e-17)
