"""Truth for k-means (tests/test_kmeans_host.py, tests/test_gpu_kmeans.py): the builder of the cases and a long-double checker
of assignments, updates and fixed points.  eps = 2^-52 throughout.  A helper, not a test file.  TEST INFRASTRUCTURE."""
from types import SimpleNamespace

import numpy as np

LD = np.longdouble
EPS = 2.0 ** -52


# ---- the checker --------------------------------------------------------------------------------------------------------------
def exact_dist2(X, C):
    """(M, kc) squared distances in 80-bit arithmetic (relative error r 2^-64: nothing beside (r + 2) eps)."""
    X, C = np.asarray(X, dtype=LD), np.asarray(C, dtype=LD)
    D = np.zeros((len(X), len(C)), dtype=LD)
    for c in range(X.shape[1]):
        d = X[:, c][:, None] - C[:, c][None, :]
        D += d * d
    return D


def check_assignment(X, C, labels, dist2, D=None):
    """dist2 within (r + 2) eps relative of the exact distance to the chosen centroid (exactly 0.0 for a coincident row), and
    that distance <= (1 + 2 (r + 2) eps) x the exact minimum (a near tie may resolve either way)."""
    X, C = np.asarray(X, dtype=np.float64), np.asarray(C, dtype=np.float64)
    M, r = X.shape
    labels, dist2 = np.asarray(labels), np.asarray(dist2)
    assert labels.shape == (M,) and dist2.shape == (M,), (labels.shape, dist2.shape)
    assert ((labels >= 0) & (labels < len(C))).all(), "label out of range"
    D = exact_dist2(X, C) if D is None else D
    got = D[np.arange(M), labels]
    tol = LD((r + 2) * EPS)
    err = np.abs(dist2.astype(LD) - got)
    worst = int(np.argmax(err - tol * got))
    assert (err <= tol * got).all(), f"row {worst}: dist2 {dist2[worst]!r} against the exact {float(got[worst])!r}"
    assert (dist2[got == 0] == 0.0).all() and not np.signbit(dist2[got == 0]).any(), "a coincident row without dist2 = +0.0"
    best = D.min(axis=1)
    far = got > best * (1 + 2 * tol)
    assert not far.any(), f"row {int(np.flatnonzero(far)[0])}: centroid {labels[far][0]} chosen, {int(D[far][0].argmin())} is nearer"


def check_update(X, labels, C_old, C_new, mu, counts=None):
    """counts exact; every entry of a non-empty cluster's centroid within (n_j + 2) eps sum_members |x - mu| / n_j + 2 eps |c*|
    of the exact mean c* (any summation order of the shifted rows); an empty cluster bit-equal to its old centroid."""
    X, labels = np.asarray(X, dtype=np.float64), np.asarray(labels)
    C_old, C_new = np.asarray(C_old, dtype=np.float64), np.asarray(C_new, dtype=np.float64)
    kc = len(C_old)
    n = np.bincount(labels, minlength=kc)
    if counts is not None:
        assert np.array_equal(np.asarray(counts).astype(np.int64), n), (counts, n)
    for j in range(kc):
        if n[j] == 0:
            assert np.array_equal(C_new[j].view(np.uint64), C_old[j].view(np.uint64)), f"empty cluster {j} moved"
            continue
        Xm = X[labels == j].astype(LD)
        exact = Xm.sum(axis=0) / n[j]
        bound = (n[j] + 2) * LD(EPS) * np.abs(Xm - np.asarray(mu, dtype=LD)).sum(axis=0) / n[j] + 2 * LD(EPS) * np.abs(exact)
        err = np.abs(C_new[j].astype(LD) - exact)
        assert (err <= bound).all(), f"cluster {j}: centroid off by {float((err - bound).max())!r} beyond the bound"


def check_fixed_point(X, res):
    """res: centers, labels, dist2, counts, inertia, inertia_history, converged, mu.  The inertia within (M + r + 2) eps relative
    of the exact sum of the exact distances to the chosen centroids, the history non-increasing up to twice that; when
    converged, every row with a nearest centroid and every centroid the mean of its members."""
    X = np.asarray(X, dtype=np.float64)
    M, r = X.shape
    D = exact_dist2(X, res.centers)
    check_assignment(X, res.centers, res.labels, res.dist2, D)
    assert np.array_equal(np.asarray(res.counts).astype(np.int64), np.bincount(res.labels, minlength=len(res.centers)))
    exact = D[np.arange(M), res.labels].sum()
    tol = LD((M + r + 2) * EPS)
    assert abs(LD(res.inertia) - exact) <= tol * exact, (res.inertia, float(exact))
    h = np.asarray(res.inertia_history, dtype=np.float64)
    assert (h[1:] <= h[:-1] * (1 + 2 * float(tol))).all(), f"inertia history increases: {h}"
    if res.converged:
        check_update(X, res.labels, res.centers, res.centers, res.mu)


def margin(X, C):
    """The smallest relative gap (second - best) / second between the best and the second-best exact distance over the rows
    (inf with a single centroid)."""
    if len(C) < 2:
        return float("inf")
    D = np.sort(exact_dist2(X, C), axis=1)
    gap = np.where(D[:, 1] > 0, (D[:, 1] - D[:, 0]) / np.where(D[:, 1] > 0, D[:, 1], 1), 0)
    return float(gap.min())


def margin_bound(r):
    return 64 * (r + 2) * EPS


# ---- the cases ----------------------------------------------------------------------------------------------------------------
#          id                 M      r    kc
SHAPES = {"one_cluster":     (5,     3,   1),
          "short_slab_r1":   (31,    1,   2),
          "slab_plus_one":   (33,    3,   17),
          "pad_r_chunks":    (20001, 5,   5),
          "widest_r":        (257,   128, 64),
          "most_clusters":   (600,   32,  256),
          "ulp_ties":        (700,   3,   4),
          "duplicate_init":  (200,   4,   6),
          "offset":          (3000,  8,   8)}
SEPARATED = ("one_cluster", "short_slab_r1", "slab_plus_one", "pad_r_chunks", "widest_r", "most_clusters", "offset")
CASES = tuple(SHAPES)


def _blobs(rng, M, r, kc, spread=3.0):
    centres = spread * rng.standard_normal((kc, r))
    return centres[rng.integers(0, kc, size=M)] + rng.standard_normal((M, r))


def build_case(name):
    """(X (M, r), init (kc, r)) of the case.  The separated cases: Gaussian blobs started from kc of their rows ('offset': the
    same at 1e6).  'ulp_ties': rows within ulps of the plane equidistant from two of the four initial centroids.
    'duplicate_init': dyadic data, mirror-symmetric about 0 (the column means are exactly 0, every sum is exact) with a blob that
    is symmetric about 0 itself; centroids 4 and 5 both start AT 0: 4 takes the blob by the index rule and stays at 0 bit for
    bit, 5 stays empty."""
    M, r, kc = SHAPES[name]
    rng = np.random.default_rng(len(name) + 11 * M)
    if name == "ulp_ties":
        init = np.array([[1.0, 0, 0], [0, 1.0, 0], [-1.0, 0, 0], [0, -1.0, 0]])
        t = rng.uniform(0.1, 2.0, size=M)
        X = np.stack([t, t.copy(), rng.uniform(-1, 1, size=M)], axis=1)     # x = y: equidistant from centroids 0 and 1
        X[:, 0] += np.spacing(X[:, 0]) * rng.integers(-2, 3, size=M)        # ... to within two ulps
        X[::7] *= -1.0                                                      # (and from 2 and 3)
        return X, init
    if name == "duplicate_init":
        q = np.zeros((2, r))
        q[0, 0], q[1, 1] = 4.0, 4.0
        off = lambda n: rng.integers(-512, 512, size=(n, r)) / 1024.0
        half = np.vstack([q[0] + off(34), q[1] + off(34), off(32)])
        X = np.vstack([half, -half])
        X = X[rng.permutation(M)]
        init = np.vstack([q[0], -q[0], q[1], -q[1], np.zeros(r), np.zeros(r)])
        return X, init
    X = _blobs(rng, M, r, kc)
    if name == "offset":
        X = X / 3.0 + 1e6
    init = X[rng.choice(M, size=kc, replace=False)].copy()
    return X, init


def second_block(name, rows=77):
    """Other rows of the case's kind for rom_kmeans_assign."""
    M, r, kc = SHAPES[name]
    X, _ = build_case(name)
    rng = np.random.default_rng(5)
    return X[rng.integers(0, M, size=rows)] + 0.25 * rng.standard_normal((rows, r)) * X.std()


def as_result(centers, labels, dist2, counts, inertia, inertia_history, converged, mu):
    return SimpleNamespace(centers=centers, labels=labels, dist2=dist2, counts=counts, inertia=inertia,
                           inertia_history=inertia_history, converged=converged, mu=mu)
