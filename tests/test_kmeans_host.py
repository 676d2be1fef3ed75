"""Host side of k-means and the local reduced bases (no GPU): the NumPy specification ``kmeans_host`` / ``maximin_rows_host``
through the long-double checker of tests/kmeans_truth.py on every case of the GPU test, the margin condition of the separated
cases (on which two implementations must agree label for label), pickling of a ``KMeans`` fitted by the host path,
rom_kmeans_layout and its limits, and the gain of local over global H^1_0-POD bases that tests/test_gpu_local_basis.py caps,
recomputed with the oracle."""
import pickle

import numpy as np
import pytest

import kmeans_truth as kt


@pytest.fixture(scope="module")
def runs():
    from romhighcontrast_amd.local import kmeans_host
    out = {}
    for name in kt.CASES:
        X, init = kt.build_case(name)
        out[name] = (X, init, kmeans_host(X, init, max_iter=50))
    return out


@pytest.mark.parametrize("name", kt.CASES)
def test_specification_through_the_checker(runs, name):
    X, init, res = runs[name]
    M, r, kc = kt.SHAPES[name]
    assert X.shape == (M, r) and init.shape == (kc, r) and res.n_iter >= 1 and len(res.inertia_history) == res.n_iter
    kt.check_fixed_point(X, res)
    for C_old, labels, C_new in res.trace[:3] + res.trace[-1:]:
        kt.check_assignment(X, C_old, labels, np.asarray(kt.exact_dist2(X, C_old)[np.arange(M), labels], dtype=np.float64))
        kt.check_update(X, labels, C_old, C_new, res.mu)
    assert res.converged, (name, res.n_iter)


@pytest.mark.parametrize("name", kt.SEPARATED)
def test_separated_cases_keep_their_margin_at_every_iteration(runs, name):
    X, init, res = runs[name]
    r = X.shape[1]
    m = min([kt.margin(X, C_old) for C_old, _, _ in res.trace] + [kt.margin(X, res.centers)])
    print(f"{name}: margin {m:.3e} against {kt.margin_bound(r):.3e}")
    assert m > kt.margin_bound(r)


def test_duplicate_initial_centroid_stays_empty_and_bit_equal(runs):
    X, init, res = runs["duplicate_init"]
    assert res.counts[5] == 0 and res.counts[4] == 64 and np.array_equal(res.centers[5].view(np.uint64), init[5].view(np.uint64))
    assert np.array_equal(res.centers[4].view(np.uint64), init[4].view(np.uint64)) and (res.mu == 0.0).all()


def test_max_iter_zero_and_tolerance_stop():
    from romhighcontrast_amd.local import kmeans_host
    X, init = kt.build_case("offset")
    r0 = kmeans_host(X, init, max_iter=0)
    assert r0.n_iter == 0 and not r0.converged and np.array_equal(r0.centers, init) and len(r0.inertia_history) == 0
    kt.check_assignment(X, init, r0.labels, r0.dist2)
    full = kmeans_host(X, init, max_iter=50)
    loose = kmeans_host(X, init, max_iter=50, tol=1e-2)
    assert 1 <= loose.n_iter <= full.n_iter and (loose.n_iter < full.n_iter) == (not loose.converged)
    with pytest.raises(ValueError):
        kmeans_host(X[:4], init)
    Xn = X.copy()
    Xn[3, 2] = np.nan
    with pytest.raises(ValueError):
        kmeans_host(Xn, init)


@pytest.mark.parametrize("name", kt.SEPARATED + ("duplicate_init",))
def test_maximin_rows(name):
    from romhighcontrast_amd.local import maximin_rows_host
    X, _ = kt.build_case(name)
    kc = kt.SHAPES[name][2]
    rows = maximin_rows_host(X, kc)
    assert rows.shape == (kc,) and len(set(rows.tolist())) == kc
    D = kt.exact_dist2(X, X.mean(axis=0)[None, :])[:, 0]
    assert D[rows[0]] <= D.min() * (1 + 2 * (X.shape[1] + 2) * kt.EPS) + 1e-300
    for s in range(1, min(kc, 6)):
        Dm = kt.exact_dist2(X, X[rows[:s]]).min(axis=1)
        assert Dm[rows[s]] >= Dm.max() * (1 - 2 * (X.shape[1] + 2) * kt.EPS)
    if name == "duplicate_init":   # mirrored rows are equally near the mean 0: the lower index wins
        twin = int(np.flatnonzero((X == -X[rows[0]]).all(axis=1))[0])
        assert rows[0] < twin


def test_host_fitted_kmeans_pickles():
    from romhighcontrast_amd.local import KMeans
    X, init = kt.build_case("slab_plus_one")
    km = KMeans(17, init=init).fit_host(X)
    assert km.converged_ and km.labels_.shape == (33,) and km.cluster_centers_.shape == (17, 3)
    km2 = pickle.loads(pickle.dumps(km))
    assert km2.handle_ is None and np.array_equal(km2.cluster_centers_, km.cluster_centers_) and np.array_equal(km2.labels_, km.labels_)
    assert km2.inertia_ == km.inertia_ and km2.n_iter_ == km.n_iter_
    rows = KMeans(17, init=np.arange(17)).fit_host(X)
    assert np.array_equal(rows.cluster_centers_.shape, (17, 3))
    mm = KMeans(3).fit_host(X)
    assert mm.counts_.sum() == 33


LAYOUT_OK = [(1, 1), (3, 17), (5, 5), (128, 64), (64, 128), (32, 256), (4, 16), (16, 64), (64, 64)]
LAYOUT_BAD = [(0, 4), (129, 4), (4, 0), (4, 257), (128, 128), (64, 129), (36, 256)]


@pytest.mark.parametrize("r,kc", LAYOUT_OK)
def test_layout_accepts(r, kc):
    from romhighcontrast_amd import _ffi
    lay = _ffi.kmeans_layout(r, kc)
    rp, kp, r1 = (r + 3) // 4 * 4, (kc + 15) // 16 * 16, (r + 1 + 15) // 16 * 16
    assert (lay["r_padded"], lay["kc_padded"], lay["r1_padded"], lay["slab_rows"]) == (rp, kp, r1, 32)
    assert kp * rp <= 8192 and lay["lds_bytes"] <= 160 * 1024 and lay["partial_doubles"] == kp * r1
    assert 1 <= lay["tiles_per_wave"] <= 6 and lay["tile_stride"] >= kp + r1 and lay["tile_stride"] % 32 == 16
    base = 8 * (kp * (rp + 2) + kp + 32 * (rp + 2) + 32 * lay["tile_stride"] + 16 + 128)
    assert lay["lds_bytes"] == (base + 8 * kc * r if base + 8 * kc * r <= 160 * 1024 else base)


@pytest.mark.parametrize("r,kc", LAYOUT_BAD)
def test_layout_rejects(r, kc):
    from romhighcontrast_amd import _ffi
    from romhighcontrast_amd.local import KMeans
    lib = _ffi.load_library()
    out = np.zeros(8, dtype=np.int64)
    assert lib.rom_kmeans_layout(r, kc, out.ctypes.data) == _ffi.ROM_ERR_INVALID
    assert "rom_kmeans_layout" in _ffi.last_error()
    with pytest.raises(ValueError):
        _ffi.kmeans_layout(r, kc)
    if r >= 1 and kc >= 1:   # the estimator refuses the shape before any device call (there may be no device here)
        from romhighcontrast_amd.lib.SolutionsManagers import DeviceArray
        with pytest.raises(ValueError):
            KMeans(kc, init=np.zeros((kc, r)), ctx=object()).fit_columns(DeviceArray(None, kc, r), (0, r), 0, kc)


def test_prototypes_and_exports():
    from romhighcontrast_amd import _ffi
    from romhighcontrast_amd.lib import ReducedBasis
    lib = _ffi.load_library()
    for name in ("rom_kmeans_layout", "rom_kmeans_init_maximin", "rom_kmeans_fit", "rom_kmeans_assign", "rom_kmeans_query",
                 "rom_kmeans_download", "rom_kmeans_destroy"):
        assert name in _ffi.PROTOTYPES and hasattr(lib, name), name
    assert len(_ffi.PROTOTYPES["rom_kmeans_fit"][1]) == 13 and len(_ffi.PROTOTYPES["rom_kmeans_assign"][1]) == 9
    assert ReducedBasis.LocalReducedBasis.__module__ == "romhighcontrast_amd.local" and ReducedBasis.KMeans is not None


def test_local_bases_beat_the_global_basis_on_the_probe_problem():
    """The figures that tests/test_gpu_local_basis.py caps (local <= 0.5 x global at n = 8), recomputed with the oracle, the NumPy
    Lloyd and an uncentred H^1_0-POD: (2,2) / N = 8, 1500 training rows, 300 held out, 8 clusters of log a."""
    from oracle import rom_oracle as ro
    from romhighcontrast_amd.local import kmeans_host, maximin_rows_host
    rng = np.random.default_rng(7)
    a = 10.0 ** rng.uniform(0, 2, size=(1800, 2, 2))
    g = ro.Geometry((2, 2), 8)
    U = np.asarray(ro.generate_solutions(g, a, "lsqsparse"))
    A1 = np.asarray(ro.assemble_dense(g, np.ones((2, 2))))   # the matrix of the H^1_0 inner product
    L = np.linalg.cholesky(A1)
    Y = U @ L                      # Euclidean coordinates of the H^1_0 inner product
    F = np.log(a.reshape(len(a), -1))
    tr, te, n = slice(0, 1500), slice(1500, 1800), 8

    def rel_err(Ytr, Yte):
        V = np.linalg.svd(Ytr, full_matrices=False)[2][:n]
        return ((Yte - Yte @ V.T @ V) ** 2).sum(axis=1) / (Yte ** 2).sum(axis=1)

    glob = np.sqrt(rel_err(Y[tr], Y[te]).mean())
    res = kmeans_host(F[tr], F[tr][maximin_rows_host(F[tr], 8)], max_iter=50)
    assert res.counts.min() >= 9
    from romhighcontrast_amd.local import dist2_host
    lab = np.argmin(dist2_host(F[te], res.centers), axis=1)
    e2 = np.zeros(300)
    for j in range(8):
        if (lab == j).any():
            e2[lab == j] = rel_err(Y[tr][res.labels == j], Y[te][lab == j])
    loc = np.sqrt(e2.mean())
    print(f"rms relative H10 projection error, n = 8: global {glob:.4f}, local (8 clusters) {loc:.4f}, ratio {loc / glob:.3f}; "
          f"smallest cluster {res.counts.min()}")
    assert loc <= 0.5 * glob
