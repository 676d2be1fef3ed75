"""CPU checks of the exact-SVD blocks of tests/referee.py (ExactSVD) that tests/test_gpu_pod_routes.py holds rom_pod_ex to:
sampled entries against Python-integer arithmetic, the column mean against its construction, and numpy.linalg.svd against
the known singular values and vectors to LAPACK's own bound."""
import numpy as np
import pytest

import referee as rf

EPS = 2.0 ** -53


def _spread(r, decades, bits=41):
    return np.round(2.0 ** bits * 10.0 ** -np.linspace(0, decades, r)).astype(np.int64)


@pytest.mark.parametrize("M,D,dim,r,mean", [(64, 1024, 1000 + 24, 40, False), (64, 1024, 1500, 40, True), (16, 16, 16, 15, True),
                                            (128, 512, 700, 100, False)])
def test_entries_are_exact(M, D, dim, r, mean):
    rng = np.random.default_rng(M + r)
    mean_int = rng.integers(-2 ** 20, 2 ** 20, size=dim) if mean else None
    t = rf.ExactSVD(M, D, dim, _spread(r, 11), 40, seed=r, mean_int=mean_int)
    for i, j in zip(rng.integers(0, M, 200), rng.integers(0, dim, 200)):
        assert t.X[i, j] == t.entry_int(i, j) * t.q, (i, j)
    # the column mean is exactly the mean row (every column sum is exact, 1 / M a power of two)
    assert np.array_equal(t.X.sum(axis=0) / M, t.mean)
    assert np.array_equal(t.X - t.X.mean(axis=0), t.centred())
    # support: only the scattered columns carry the modes
    off = np.setdiff1d(np.arange(dim), t.cols)
    assert np.array_equal(t.centred()[:, off], np.zeros((M, off.size)))


def test_padded_rows_and_hadamard_columns():
    H = rf.hadamard_columns(8, np.arange(8))
    assert np.array_equal(H @ H.T, 8 * np.eye(8))
    t = rf.ExactSVD(16, 64, 64, [5, 3, 3, 1], 2, seed=1, pad=5)
    assert t.X.shape == (21, 64) and not t.X[16:].any()
    assert np.array_equal(t.s, [1.25, 0.75, 0.75, 0.25])


@pytest.mark.parametrize("M,D,dim,r,decades", [(64, 1024, 1024, 40, 11), (32, 32, 50, 20, 4), (256, 64, 64, 60, 6)])
def test_lapack_agrees_to_its_own_bound(M, D, dim, r, decades):
    t = rf.ExactSVD(M, D, dim, _spread(r, decades), 41, seed=7)
    U, s, Vt = np.linalg.svd(t.X, full_matrices=False)
    tol = 8 * EPS * max(M, dim) ** 0.5 * t.s[0]
    assert np.abs(s[:r] - t.s).max() <= tol
    assert s[r:].max(initial=0.0) <= tol
    # each isolated mode: sin(angle) <= tol / gap
    gaps = np.array([np.min(np.abs(np.delete(np.append(t.s, 0.0), k) - t.s[k])) for k in range(r)])
    c = np.sum(Vt[:r] * t.V, axis=1)
    ang = np.linalg.norm(Vt[:r] - c[:, None] * t.V, axis=1)
    assert np.all(ang <= tol / gaps + 4 * EPS * np.sqrt(dim))


def test_clusters_have_exact_projectors():
    mant = [8, 8, 8, 4, 4, 1]
    t = rf.ExactSVD(32, 32, 40, mant, 3, seed=2)
    U, s, Vt = np.linalg.svd(t.X, full_matrices=False)
    assert np.allclose(s[:6], [1, 1, 1, .5, .5, .125], rtol=0, atol=1e-15)
    for lo, hi in ((0, 3), (3, 5), (5, 6)):
        P = Vt[lo:hi].T @ Vt[lo:hi]
        Pt = t.V[lo:hi].T @ t.V[lo:hi]
        assert np.abs(P - Pt).max() <= 64 * EPS


def test_coherent_blocks():
    """u_k = unit vectors: one term per entry, a diagonal Gram matrix, and LAPACK's values / vectors to its bound."""
    mant = _spread(40, 8, bits=30)
    t = rf.ExactSVD(100, 256, 300, mant, 30, seed=4, coherent=True)
    rng = np.random.default_rng(5)
    for i, j in zip(rng.integers(0, 100, 300), rng.integers(0, 300, 300)):
        assert t.X[i, j] == t.entry_int(i, j) * t.q, (i, j)
    rows = np.sort(t.L)
    G = t.X[rows] @ t.X[rows].T
    assert np.abs(G - np.diag(np.diag(G))).max() <= 4 * EPS * t.s[0] ** 2
    assert not np.delete(t.X, t.L, axis=0).any()
    _, s, Vt = np.linalg.svd(t.X, full_matrices=False)
    tol = 8 * EPS * 300 ** 0.5 * t.s[0]
    assert np.abs(s[:40] - t.s).max() <= tol and s[40:].max() <= tol
    c = np.sum(Vt[:40] * t.V, axis=1)
    gaps = np.array([np.min(np.abs(np.delete(np.append(t.s, 0.0), k) - t.s[k])) for k in range(40)])
    assert np.all(np.linalg.norm(Vt[:40] - c[:, None] * t.V, axis=1) <= tol / gaps + 4 * EPS * np.sqrt(300))
