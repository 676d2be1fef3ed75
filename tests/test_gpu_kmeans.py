"""rom_kmeans on the GPU against the long-double checker of tests/kmeans_truth.py.

Every case runs the fused kernel (mode 0) and the exhaustive scan (mode 1) on column ranges of NaN-filled blocks with wider
strides: identical bits between the modes for labels, dist2, centroids, counts and the inertia history, operands back bit for
bit, the same bits on a second call, and every checker passes.  Shapes (tests/kmeans_truth.py): a single centroid; fewer rows
than one 32-row slab with one column; one row past a slab with one centroid past a 16-tile; r = 5 padded to 8 over several
workgroup chunks; the widest rows; the most centroids; rows within ulps of equidistant from two centroids; two equal initial
centroids; data at 1e6 with unit spread."""
import numpy as np
import pytest

import kmeans_truth as kt

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from romhighcontrast_amd import _ffi
    return _ffi.get_context()


def _same_bits(a, b):
    return np.array_equal(np.asarray(a, dtype=np.float64).view(np.uint64), np.asarray(b, dtype=np.float64).view(np.uint64))


class Block:
    """rows x r values from column `col` of rows [1, 1 + rows) of a NaN block with `extra` more columns."""

    def __init__(self, ctx, X, col, extra):
        rows, r = X.shape
        self.ld = r + extra
        self.off = self.ld + col
        self.host = np.full((rows + 2, self.ld), np.nan)
        self.host[1:1 + rows, col:col + r] = X
        self.buf = ctx.upload(self.host)

    def unchanged(self):
        return _same_bits(self.buf.download(shape=self.host.shape), self.host)


def _fit(ctx, blk, X, init, max_iter, mode, tol=0.0):
    M, r = X.shape
    h = ctx.kmeans_fit(blk.buf, blk.off, blk.ld, r, M, len(init), init, max_iter=max_iter, tol=tol, mode=mode)
    labels, d2, inertia = h.assign(blk.buf, blk.off, blk.ld, M, mode=mode)
    hist = h.download("inertia")
    out = kt.as_result(h.download("centroids"), h.download("labels"), d2, h.download("counts"), float(hist[-1]), hist[:-1],
                       h.info["converged"], h.download("shift"))
    out.info, out.handle = h.info, h
    assert np.array_equal(labels, out.labels), "rom_kmeans_assign on the training block disagrees with the labels of the fit"
    assert inertia == out.inertia, (inertia, out.inertia)
    assert h.info["host_syncs"] <= 2 + -(-h.info["iterations"] // 8), h.info
    return out


def _both_modes(ctx, X, init, max_iter):
    """Modes 0 and 1 (mode 0 twice) on a NaN-framed copy; the shared assertions; returns mode 0's result."""
    blk = Block(ctx, X, 2, 5)
    runs = [_fit(ctx, blk, X, init, max_iter, mode) for mode in (0, 1, 0)]
    assert blk.unchanged()
    a = runs[0]
    for b in runs[1:]:
        assert np.array_equal(a.labels, b.labels), np.flatnonzero(a.labels != b.labels)[:6]
        assert _same_bits(a.dist2, b.dist2) and _same_bits(a.centers, b.centers) and np.array_equal(a.counts, b.counts)
        assert _same_bits(a.inertia_history, b.inertia_history) and a.inertia == b.inertia
        assert a.info["iterations"] == b.info["iterations"] and a.converged == b.converged
    kt.check_fixed_point(X, a)
    return a


@pytest.fixture(scope="module")
def host_runs():
    from romhighcontrast_amd.local import kmeans_host
    out = {}
    for name in kt.CASES:
        X, init = kt.build_case(name)
        out[name] = (X, init, kmeans_host(X, init, max_iter=50))
    return out


@pytest.mark.parametrize("name", kt.CASES)
def test_cases(ctx, host_runs, name):
    X, init, ref = host_runs[name]
    M, r, kc = kt.SHAPES[name]
    res = _both_modes(ctx, X, init, 50)
    print(name, res.info)
    assert _same_bits(res.mu, res.handle.download("shift")) and abs(res.mu - X.mean(axis=0)).max() <= M * kt.EPS * abs(X).max()
    # one iteration from the initial centroids: its labels are the assignment of max_iter = 0, its update goes through the checker
    first = _both_modes(ctx, X, init, 0)
    assert first.info["iterations"] == 0 and not first.converged and _same_bits(first.centers, init) and len(first.inertia_history) == 0
    kt.check_assignment(X, init, first.labels, first.dist2)
    one = _both_modes(ctx, X, init, 1)
    assert one.info["iterations"] == 1
    kt.check_update(X, first.labels, init, one.centers, one.mu)
    assert one.inertia_history[0] == first.inertia
    if name == "pad_r_chunks":
        assert res.info["chunks"] >= 2, res.info
    if name in kt.SEPARATED:
        assert np.array_equal(res.labels, ref.labels) and res.info["iterations"] == ref.n_iter and res.converged == ref.converged
    if name == "duplicate_init":
        assert res.counts[5] == 0 and res.counts[4] == 64 and _same_bits(res.centers[5], init[5]) and _same_bits(res.centers[4], init[4])
    if name == "ulp_ties":
        D = np.asarray(kt.exact_dist2(X, init), dtype=np.float64)
        near = np.sort(D, axis=1)
        assert ((near[:, 1] - near[:, 0]) <= 64 * kt.EPS * near[:, 1]).mean() > 0.5, "the case lost its ties"
    # other rows against the fitted centroids
    P = kt.second_block(name)
    pb = Block(ctx, P, 1, 3)
    answers = [res.handle.assign(pb.buf, pb.off, pb.ld, len(P), mode=mode) for mode in (0, 1)]
    assert pb.unchanged()
    assert np.array_equal(answers[0][0], answers[1][0]) and _same_bits(answers[0][1], answers[1][1]) and answers[0][2] == answers[1][2]
    kt.check_assignment(P, res.centers, answers[0][0], answers[0][1])


@pytest.mark.parametrize("name", kt.SEPARATED + ("duplicate_init",))
def test_maximin_start(ctx, name):
    from romhighcontrast_amd.local import maximin_rows_host
    X, _ = kt.build_case(name)
    kc = kt.SHAPES[name][2]
    blk = Block(ctx, X, 2, 5)
    rows = ctx.kmeans_init_maximin(blk.buf, blk.off, blk.ld, X.shape[1], len(X), kc)
    assert blk.unchanged()
    assert np.array_equal(rows, maximin_rows_host(X, kc)), (rows, maximin_rows_host(X, kc))
    assert np.array_equal(rows, ctx.kmeans_init_maximin(blk.buf, blk.off, blk.ld, X.shape[1], len(X), kc))


def test_tolerance_stop_and_estimator(ctx):
    from romhighcontrast_amd.local import KMeans, kmeans_host
    X, init = kt.build_case("offset")
    blk = Block(ctx, X, 0, 0)
    ref = kmeans_host(X, init, max_iter=50, tol=1e-2)
    res = _fit(ctx, blk, X, init, 50, 0, tol=1e-2)
    assert res.info["iterations"] == ref.n_iter and res.converged == ref.converged and np.array_equal(res.labels, ref.labels)
    km = KMeans(8, init=init, ctx=ctx).fit(X)
    full = kmeans_host(X, init, max_iter=50)
    assert km.converged_ and km.n_iter_ == full.n_iter and np.array_equal(km.labels_, full.labels) and km.inertia_history_.shape == (km.n_iter_,)
    assert np.array_equal(km.predict(X), km.labels_) and np.array_equal(km.counts_, full.counts)
    mm = KMeans(8, ctx=ctx).fit(X)
    assert mm.converged_ and mm.counts_.sum() == len(X)
    by_rows = KMeans(8, init=np.arange(8), ctx=ctx).fit(X)
    assert _same_bits(by_rows.cluster_centers_, KMeans(8, init=X[:8], ctx=ctx).fit(X).cluster_centers_)


def test_refused_shapes_and_values(ctx):
    X = np.random.default_rng(0).random((300, 129))
    buf = ctx.upload(X)
    with pytest.raises(ValueError):
        ctx.kmeans_fit(buf, 0, 129, 129, 300, 4, np.zeros((4, 129)))
    with pytest.raises(ValueError):
        ctx.kmeans_fit(buf, 0, 129, 4, 300, 257, np.zeros((257, 4)))
    with pytest.raises(ValueError):
        ctx.kmeans_fit(buf, 0, 129, 128, 300, 128, np.zeros((128, 128)))
    with pytest.raises(ValueError):
        ctx.kmeans_fit(buf, 0, 129, 4, 7, 8, X[:8, :4])               # M < kc
    with pytest.raises(ValueError):
        ctx.kmeans_init_maximin(buf, 0, 129, 4, 7, 8)
    Xn = X[:, :4].copy()
    Xn[250, 3] = np.nan
    bn = ctx.upload(Xn)
    for mode in (0, 1):
        with pytest.raises(ValueError, match="NaN / Inf"):
            ctx.kmeans_fit(bn, 0, 4, 4, 300, 8, X[:8, :4], mode=mode)
    with pytest.raises(ValueError, match="NaN / Inf"):
        ctx.kmeans_init_maximin(bn, 0, 4, 4, 300, 8)
    init = X[:8, :4].copy()
    init[2, 1] = np.inf
    with pytest.raises(ValueError, match="NaN / Inf"):
        ctx.kmeans_fit(buf, 0, 129, 4, 300, 8, init)
    h = ctx.kmeans_fit(buf, 0, 129, 4, 300, 8, X[:8, :4])
    with pytest.raises(ValueError, match="NaN / Inf"):
        h.assign(bn, 0, 4, 300)
    # the context still works after the refusals
    assert h.assign(buf, 0, 129, 300)[0].shape == (300,)
