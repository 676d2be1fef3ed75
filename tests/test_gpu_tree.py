"""rom_tree_fit / rom_tree_predict on the GPU against the certificate checker of tests/tree_truth.py.

Near-ties make a tree non-unique under rounding, so the device's trees are not compared node by node with a truth tree: every
node of the downloaded forest is VERIFIED (tree_truth.check_tree: partition and counts exact; the chosen candidate valid and its
80-bit gain within 64 n eps SS_node of the best; a stop condition at every leaf; leaf values within 64 n eps max|y - mean| +
eps |mean|, bit for bit for constant targets).  The shapes are the smallest that reach each path: one row, an exact cross-input
tie, one position past a wave, zero-count rows and weights > 1, segments across several workgroups of four 64-position tiles,
max_depth / min_samples_leaf, a constant input and a constant target, the widest q, and a target of mean 1e8 and spread 1 (the
case the node-mean shift exists for).  X and Y are column ranges of ONE NaN-filled block with NaN sentinel rows, which must
come back bit for bit; predictions go into a NaN block of wider ldo whose surroundings stay NaN."""
import numpy as np
import pytest

from conftest import observed
import tree_truth as tt

pytestmark = pytest.mark.gpu
LD, EPS = tt.LD, tt.EPS
N_TEST = 100


@pytest.fixture(scope="module")
def ctx():
    from romhighcontrast_amd import _ffi
    return _ffi.get_context()


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


class Block:
    """X (m columns from column 3) and Y (q columns from column 3 + m + 2) inside one block of ld = m + q + 6 columns, rows
    [2, 2 + rows) of it; every other entry is NaN."""

    def __init__(self, ctx, X, Y):
        self.rows, self.m = X.shape
        self.q = Y.shape[1]
        self.ld = self.m + self.q + 6
        self.xc, self.yc = 3, 3 + self.m + 2
        host = np.full((self.rows + 4, self.ld), np.nan)
        host[2:2 + self.rows, self.xc:self.xc + self.m] = X
        host[2:2 + self.rows, self.yc:self.yc + self.q] = Y
        self.host = host
        self.buf = ctx.upload(host)

    def x_off(self, row):
        return (2 + row) * self.ld + self.xc

    def y_off(self, row):
        return (2 + row) * self.ld + self.yc

    def unchanged(self):
        return _same_bits(self.buf.download(shape=self.host.shape), self.host)


def _fit(ctx, blk, M, T=1, counts=None, **kw):
    return ctx.tree_fit(blk.buf, blk.x_off(0), blk.ld, blk.m, blk.buf, blk.y_off(0), blk.ld, blk.q, M, T, counts, **kw)


def _predict(ctx, tm, blk, row0, rows, **kw):
    """Predictions for rows [row0, row0 + rows) of the block, into a NaN block of ld = q + 3 from column 2, rows [1, 1 + rows)."""
    ldo = blk.q + 3
    out = ctx.alloc((rows + 2) * ldo).fill(np.nan)
    ss = tm.predict(blk.buf, blk.x_off(row0), blk.ld, rows, OUT=out, o_off=ldo + 2, ldo=ldo, **kw)
    full = out.download(shape=(rows + 2, ldo))
    assert np.isnan(full[0]).all() and np.isnan(full[-1]).all() and np.isnan(full[:, :2]).all() and np.isnan(full[:, 2 + blk.q:]).all()
    return full[1:1 + rows, 2:2 + blk.q], ss


def _data(M, m, q, seed, rows=None):
    rng = np.random.default_rng(seed)
    rows = M if rows is None else rows
    X = rng.uniform(-1, 1, (rows, m)) * 10.0 ** -np.arange(m) + 0.3
    k = np.arange(q)
    Y = np.sin(3 * (k % 5 + 1) * X[:, :1]) + (k % 3) * (X[:, m - 1:m] * 10.0 ** (m - 1)) ** 2 + 0.1 * rng.standard_normal((rows, q))
    return X, Y


def _bootstrap(T, M, seed):
    from romhighcontrast_amd.nonlinear import ForestMap
    return ForestMap.bootstrap_counts(T, M, seed)


def _case(cid):
    """(X, Y, T, counts, keywords of the fit)"""
    if cid == "one_row":
        return (*_data(1, 1, 1, 1), 1, None, {})
    if cid == "two_rows_tie":
        X, Y = _data(2, 3, 2, 2)
        return X, Y, 1, None, {}
    if cid == "three_rows":
        return (*_data(3, 2, 1, 3), 1, None, {})
    if cid == "m65_past_a_wave":
        return (*_data(65, 1, 1, 4), 1, None, {})
    if cid == "m257_q17":
        return (*_data(257, 4, 17, 5), 1, None, {})
    if cid == "m1025_bootstrap_T3":
        return (*_data(1025, 4, 20, 6), 3, _bootstrap(3, 1025, 6), {})
    if cid == "m4101_m16_T2":
        return (*_data(4101, 16, 5, 7), 2, None, {})
    if cid == "m8193_depth3":
        return (*_data(8193, 2, 1, 8), 1, None, dict(max_depth=3))
    if cid == "m8193_leaf50":
        return (*_data(8193, 2, 1, 8), 1, None, dict(min_samples_leaf=50))
    if cid == "m300_levels_constants":
        rng = np.random.default_rng(9)
        X = np.column_stack((rng.integers(0, 5, 300).astype(np.float64), np.full(300, 2.5), rng.uniform(-1, 1, 300)))
        Y = np.column_stack((X[:, 0] + np.sin(3 * X[:, 2]) + 0.1 * rng.standard_normal(300), np.full(300, -7.25)))
        return X, Y, 1, None, {}
    if cid == "m64_q128":
        return (*_data(64, 1, 128, 10), 1, None, {})
    if cid == "mean_1e8":
        rng = np.random.default_rng(11)
        X = rng.uniform(-1, 1, (500, 2))
        Y = 1e8 + np.column_stack((np.sin(3 * X[:, 0]), X[:, 1] ** 2)) + 0.1 * rng.standard_normal((500, 2))
        return X, Y, 1, None, {}
    raise KeyError(cid)


CASES = ["one_row", "two_rows_tie", "three_rows", "m65_past_a_wave", "m257_q17", "m1025_bootstrap_T3", "m4101_m16_T2", "m8193_depth3",
         "m8193_leaf50", "m300_levels_constants", "m64_q128", "mean_1e8"]


@pytest.mark.parametrize("cid", CASES)
def test_certificate(ctx, cid):
    X, Y, T, counts, kw = _case(cid)
    M = X.shape[0]
    blk = Block(ctx, X, Y)
    tm = _fit(ctx, blk, M, T, counts, **kw)
    nodes = tm.nodes()
    print(f"{cid}: {tm.info}")
    assert blk.unchanged(), (cid, "inputs and the NaNs around them")
    trees = tt.split_forest(nodes, T)
    stats = tt.check_forest(trees, X, Y, counts, max_depth=kw.get("max_depth", 0), min_samples_leaf=kw.get("min_samples_leaf", 1))
    print(f"{cid}: {stats}")
    observed(f"tree {cid}: (best 80-bit gain - gain of the device's candidate) / (64 n eps SS), worst node",
             max(s["worst_gain"] for s in stats), 1.0)
    observed(f"tree {cid}: |leaf value - 80-bit mean| / (64 n eps max|y - mean| + eps |mean|), worst leaf",
             max(s["worst_value"] for s in stats), 1.0)
    # the figures of the handle: nodes = 2 leaves - 1 per tree
    assert tm.info["nodes"] == sum(s["nodes"] for s in stats) == 2 * tm.info["leaves"] - T
    assert tm.info["deepest_level"] == max(s["deepest"] for s in stats) == tm.info["levels"] - 1
    qy = tm.query()
    assert (qy["m"], qy["q"], qy["T"], qy["M_train"], qy["nodes"], qy["deepest_level"]) == (blk.m, blk.q, T, M, tm.info["nodes"],
                                                                                           tm.info["deepest_level"])
    assert tm.info["host_syncs"] == tm.info["levels"] + 2 and qy["launches"] == tm.info["launches"]
    if cid == "two_rows_tie":   # every input separates the two rows with the same gain: the lowest input wins
        assert nodes["feature"].tolist() == [0, -1, -1]
    if cid == "m8193_depth3":
        assert tm.info["nodes"] == 15
    # the same bits on a second fit
    nodes2 = _fit(ctx, blk, M, T, counts, **kw).nodes()
    assert all(_same_bits(nodes[k], nodes2[k]) for k in nodes), (cid, "repeat")


def test_interpolation_and_predict_against_a_host_walk(ctx):
    M, m, q = 700, 3, 4
    X, Y = _data(M, m, q, 21, rows=M + N_TEST)
    blk = Block(ctx, X, Y)
    tm = _fit(ctx, blk, M)
    tree = tt.split_forest(tm.nodes(), 1)[0]
    pred, _ = _predict(ctx, tm, blk, 0, M)
    assert _same_bits(pred, Y[:M]), "distinct inputs, default parameters: the tree interpolates its training rows bit for bit"
    # held-out rows, some of them exactly ON a threshold: they go left
    Xt = X[M:].copy()
    inner = np.flatnonzero(tree["feature"] >= 0)
    for i, nd in enumerate(inner[:20]):
        Xt[i, tree["feature"][nd]] = tree["threshold"][nd]
    blk_t = Block(ctx, Xt, Y[M:])
    got, _ = _predict(ctx, tm, blk_t, 0, N_TEST)
    assert _same_bits(got, tt.predict_tree(tree, Xt)), "T = 1: the device's walk = the host's walk of the downloaded nodes"
    root_f, root_t = tree["feature"][0], tree["threshold"][0]
    on = Xt[0].copy()
    on[root_f] = root_t
    assert tt.leaves_of(tree, on[None])[0] == tt.leaves_of(tree, np.where(np.arange(m) == root_f, root_t - 1e-9, on)[None])[0]
    # Yref and the sums of squares
    diff, ss = _predict(ctx, tm, blk_t, 0, N_TEST, Yref=blk_t.buf, r_off=blk_t.y_off(0), ldr=blk_t.ld, sumsq=True)
    assert _same_bits(diff, Y[M:] - got)
    want = (diff.astype(LD) ** 2).sum(0)
    observed("tree sumsq_host of Yref - prediction: |device - long double| / (M eps sum)",
             np.abs(ss.astype(LD) - want).astype(np.float64) / (N_TEST * EPS * want.astype(np.float64)), 1.0)
    _, ss_p = _predict(ctx, tm, blk_t, 0, N_TEST, sumsq=True)
    want = (got.astype(LD) ** 2).sum(0)
    observed("tree sumsq_host of the prediction: |device - long double| / (M eps sum)",
             np.abs(ss_p.astype(LD) - want).astype(np.float64) / (N_TEST * EPS * want.astype(np.float64)), 1.0)
    only = tm.predict(blk_t.buf, blk_t.x_off(0), blk_t.ld, N_TEST, OUT=None, Yref=blk_t.buf, r_off=blk_t.y_off(0), ldr=blk_t.ld, sumsq=True)
    assert _same_bits(only, ss), "OUT = NULL: the same sums"
    assert blk.unchanged() and blk_t.unchanged()
    # a forest of three: the mean over the trees in tree order
    counts = _bootstrap(3, M, 22)
    fm = _fit(ctx, blk, M, 3, counts)
    trees = tt.split_forest(fm.nodes(), 3)
    got3, _ = _predict(ctx, fm, blk_t, 0, N_TEST)
    want3 = tt.predict_forest(trees, Xt)
    vmax = max(np.abs(t["value"]).max() for t in trees)
    observed("forest T = 3: |device prediction - host walk| / (4 eps max|value|)", np.abs(got3 - want3) / (4 * EPS * vmax), 1.0)


def test_parity_with_scikit_learn_one_input(ctx):
    from sklearn.tree import DecisionTreeRegressor
    rng = np.random.default_rng(1)
    M = 257
    x = (rng.permutation(M + N_TEST) / (M + N_TEST) + rng.uniform(0.1, 0.4, M + N_TEST) / (M + N_TEST)).astype(np.float32).astype(np.float64)
    y = np.sin(7 * x) + 0.1 * rng.standard_normal(M + N_TEST)
    blk = Block(ctx, x[:, None], y[:, None])
    tm = _fit(ctx, blk, M)
    got, _ = _predict(ctx, tm, blk, M, N_TEST)
    sk = DecisionTreeRegressor().fit(x[:M, None], y[:M]).predict(x[M:, None])
    observed("tree m = 1 on float32-exact inputs: |device - DecisionTreeRegressor| on 100 held-out rows", np.abs(got[:, 0] - sk), 1e-12)


# ---- real scores: the reference's experiment at 3000 samples -------------------------------------------------------------
@pytest.fixture(scope="module")
def scores(ctx):
    from src.experiments import NonLinearROM as NL
    out = NL.vn_family_sampler(3000, (2, 2), 1, 100, 5)
    pca = NL.pca_tall(ctx, out["solutions"], center=True, scores=True, download=False)
    return dict(pca=pca, Sd=pca.scores, S=pca.scores.numpy())


def test_real_scores_experiment_functions_and_decoder(ctx, scores):
    from sklearn.ensemble import RandomForestRegressor
    from src.experiments import NonLinearROM as NL
    S, Sd, pca = scores["S"], scores["Sd"], scores["pca"]
    m, q, n_train = 4, 16, 3000 - N_TEST
    w = NL.MWhere(m=m, start=0)
    rms = np.sqrt(np.mean(S[N_TEST:, m:m + q] ** 2, axis=0))
    for make in (lambda: NL.TreeMap(ctx=ctx), lambda: NL.ForestMap(10, ctx=ctx)):
        exp_dev = NL.learn_eigenvalues_device(model=make(), ctx=ctx)
        dev = exp_dev(n_train, N_TEST, Sd, w, q)
        host = NL.learn_eigenvalues(make())(n_train, N_TEST, S, w, q)
        name = exp_dev.__name__
        assert name in ("Tree device", "RF device") and dev["error"].shape == host["error"].shape == (N_TEST, q)
        observed(f"learn_eigenvalues_device(model = {name}) vs learn_eigenvalues on downloaded scores / (1e-12 column RMS)",
                 np.abs(dev["error"] - host["error"]).max(0) / (1e-12 * rms), 1.0)
        want = np.sqrt(np.mean(dev["error"] ** 2, axis=0))
        observed(f"{name}: rmse of the device's sums of squares vs the column RMS of its error / ((n_test + 2) eps)",
                 np.abs(dev["rmse"] - want) / want / ((N_TEST + 2) * EPS), 1.0)
    # The forest against scikit-learn's, RMSE per mode over the 100 held-out rows against the median over 20 seeds.  The band
    # asked for first was 10 %.  Measured: device / median = 0.958 .. 1.467 over the 16 modes; the 80-bit host greedy of
    # tests/tree_truth.py on the same problem 0.940 .. 1.525 (bootstrap seed 0; seeds 1, 2, 3: 0.894 .. 1.384, 0.761 .. 1.517,
    # 0.939 .. 1.323), so the deviation belongs to the statistic, not to the device: scikit-learn's OWN 20 seeds spread over
    # 0.63 .. 2.53 of their median per mode (0.84 .. 1.28 for all modes together), because a per-mode RMSE over 100 rows of a
    # noise-free target hangs on which of two training rows a held-out row is given to in the last splits.  The band is
    # therefore a factor of 2 either way -- the extremes of the reference's own seeds -- and the spread is printed.
    Xtr, Ytr, Xte, Yte = S[N_TEST:, :m], S[N_TEST:, m:m + q], S[:N_TEST, :m], S[:N_TEST, m:m + q]
    sk = np.array([np.sqrt(np.mean((RandomForestRegressor(n_estimators=10, random_state=s).fit(Xtr, Ytr).predict(Xte) - Yte) ** 2, axis=0))
                   for s in range(20)])
    med = np.median(sk, axis=0)
    ratio = dev["rmse"] / med
    print("forest RMSE per mode / median of scikit-learn's RF over 20 seeds:", np.round(ratio, 4))
    print("scikit-learn's own seeds, min / median and max / median per mode:", np.round(sk.min(0) / med, 3), np.round(sk.max(0) / med, 3))
    observed("RF device: |log2(RMSE per mode / median of RandomForestRegressor(10) over 20 seeds)|", np.abs(np.log2(ratio)), 1.0)
    # the decoder with a tree
    model = NL.TreeMap(ctx=ctx).fit_columns(Sd, (0, m), Sd, (m, m + q), N_TEST, n_train)
    known = S[:N_TEST, :m]
    rec = NL.nonlinear_reconstruction(pca, model, known)
    V, mean = pca.components_.numpy(), pca.mean_.numpy().ravel()
    pred = np.asarray(model.predict(known))
    want = mean + known @ V[:m] + pred @ V[m:m + q]
    observed("nonlinear_reconstruction with a TreeMap vs NumPy on the downloaded pieces / (1e-12 ||row||)",
             np.linalg.norm(rec - want, axis=1) / (1e-12 * np.linalg.norm(want, axis=1)), 1.0)


def test_error_cases(ctx):
    from romhighcontrast_amd import _ffi
    from src.experiments import NonLinearROM as NL
    rng = np.random.default_rng(0)
    Z = ctx.upload(rng.standard_normal((50, 8)))

    def fails(words, fn, *args, **kw):
        with pytest.raises(_ffi.RomLibraryError) as ei:
            fn(*args, **kw)
        assert all(w in str(ei.value) for w in words), str(ei.value)

    fit = ctx.tree_fit
    fails(["rom_tree_fit", "null"], fit, None, 0, 8, 2, Z, 2, 8, 2, 50)
    fails(["rom_tree_fit", "m = 17"], fit, ctx.alloc(50 * 20), 0, 20, 17, Z, 2, 8, 2, 50)
    fails(["rom_tree_fit", "q = 129"], fit, Z, 0, 8, 2, ctx.alloc(2 * 129), 0, 129, 129, 2)
    fails(["rom_tree_fit", "T = 0"], fit, Z, 0, 8, 2, Z, 2, 8, 2, 50, 0)
    fails(["rom_tree_fit", "T = 257"], fit, Z, 0, 8, 2, Z, 2, 8, 2, 50, 257)
    fails(["rom_tree_fit", "M = 0"], fit, Z, 0, 8, 2, Z, 2, 8, 2, 0)
    fails(["rom_tree_fit", "X holds 400"], fit, Z, 7, 8, 2, Z, 2, 8, 2, 50)
    fails(["rom_tree_fit", "min_samples_split = 1"], fit, Z, 0, 8, 2, Z, 2, 8, 2, 50, min_samples_split=1)
    counts = np.ones((2, 50), dtype=np.int32)
    counts[1] = 0
    fails(["rom_tree_fit", "tree 1", "without rows"], fit, Z, 0, 8, 2, Z, 2, 8, 2, 50, 2, counts)
    counts[1, 3] = -1
    fails(["rom_tree_fit", "negative"], fit, Z, 0, 8, 2, Z, 2, 8, 2, 50, 2, counts)
    bad = rng.standard_normal((50, 8))
    bad[7, 1] = np.nan
    fails(["rom_tree_fit", "NaN / Inf"], fit, ctx.upload(bad), 0, 8, 2, Z, 2, 8, 2, 50)
    bad[7, 1] = np.inf
    fails(["rom_tree_fit", "NaN / Inf"], fit, Z, 0, 8, 2, ctx.upload(bad), 0, 8, 2, 50)
    with pytest.raises(ValueError):
        NL.TreeMap(ctx=ctx).fit(bad[:, :2], bad[:, 2:4])
    with pytest.raises(ValueError):
        NL.ForestMap(3, ctx=ctx).fit(bad[:, :2], bad[:, 2:4])
    tm = fit(Z, 0, 8, 2, Z, 2, 8, 3, 50)
    out = ctx.alloc(50 * 3)
    fails(["rom_tree_predict", "OUT == NULL"], tm.predict, Z, 0, 8, 50)
    fails(["rom_tree_predict", "ldx = 1 < m = 2"], tm.predict, Z, 0, 1, 50, OUT=out)   # a block of another m
    fails(["rom_tree_predict", "ldo = 2 < q = 3"], tm.predict, Z, 0, 8, 50, OUT=out, ldo=2)
    fails(["rom_tree_predict", "X holds 400"], tm.predict, Z, 0, 8, 51, OUT=out)
    fails(["rom_tree_predict", "OUT holds 150"], tm.predict, Z, 0, 8, 50, OUT=out, o_off=1)
    fails(["rom_tree_predict", "Yref holds 400"], tm.predict, Z, 0, 8, 50, OUT=out, Yref=Z, r_off=6, ldr=8)
    fails(["rom_tree_predict", "OUT overlaps X"], tm.predict, Z, 0, 8, 40, OUT=Z, o_off=4, ldo=8)
    fails(["rom_tree_download", "count"], lambda: _ffi.check(ctx.lib.rom_tree_download(tm.h, 1, np.zeros(4).ctypes.data, 4)))


def test_blocks_that_end_on_the_last_double_of_their_buffers(ctx):
    import tight_blocks
    counts = np.random.default_rng(6).integers(0, 3, (2, tight_blocks.M)).astype(np.int32)
    tight_blocks.check(ctx, "rom_tree", lambda *blocks: ctx.tree_fit(*blocks, 2, counts))
