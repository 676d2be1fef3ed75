"""rom_mlp_fit / rom_mlp_loss_grad / rom_mlp_predict on the GPU against the 80-bit truth of tests/mlp_truth.py.

THE BOUND (mlp_truth.py): per gradient entry and for the loss |device - truth| <= (M + sum_l K_l + 32) eps G_abs, eps = 2^-53,
G_abs the absolute-value propagation; per predicted entry (sum_l K_l + 32) eps (|y_mean| + y_scale abs-propagated output).
NumPy's fp64 evaluation of the same quantity is printed beside every device figure.  The truth takes the scaled inputs and
targets formed in fp64 from the handle's own scalings (each operation correctly rounded: the device's bits); the scalings
themselves are checked against NumPy separately.

X and Y are column ranges of ONE wider block whose other entries, and the sentinel rows around it, are NaN: the NaNs and both
inputs must come back bit for bit.  The optimiser is held against its NumPy specification (nonlinear.mlp_fit_host) in long
double after 1, 2 and 3 iterations: tolerance 64 x the distance between that specification in fp64 and in long double
(64 = sqrt(M) growth of a chained sum against NumPy's pairwise one at M <= 4101), floored at 64 eps max|w|."""
import numpy as np
import pytest

from conftest import observed
import mlp_truth as mt

pytestmark = pytest.mark.gpu
LD, EPS = mt.LD, mt.EPS


@pytest.fixture(scope="module")
def ctx():
    from romhighcontrast_amd import _ffi
    return _ffi.get_context()


def _same_bits(a, b):
    return np.array_equal(np.asarray(a).view(np.uint64), np.asarray(b).view(np.uint64))


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


def _fit(ctx, blk, M, hidden, w0, activation, alpha, max_iter=0, tol=1e-6, memory=10, scale_targets=True):
    return ctx.mlp_fit(blk.buf, blk.x_off(0), blk.ld, blk.m, blk.buf, blk.y_off(0), blk.ld, blk.q, M, hidden, w0, activation, alpha,
                       scale_targets, max_iter, tol, memory)


def _predict(ctx, h, blk, row0, rows, **kw):
    """Predictions for rows [row0, row0 + rows) of the block, into a NaN block of ld = q + 3 from column 2, rows [1, 1 + rows)."""
    ldo = blk.q + 3
    out = ctx.alloc((rows + 2) * ldo).fill(np.nan)
    ss = h.predict(blk.buf, blk.x_off(row0), blk.ld, rows, OUT=out, o_off=ldo + 2, ldo=ldo, **kw)
    full = out.download(shape=(rows + 2, ldo))
    assert np.isnan(full[0]).all() and np.isnan(full[-1]).all() and np.isnan(full[:, :2]).all() and np.isnan(full[:, 2 + blk.q:]).all()
    return full[1:1 + rows, 2:2 + blk.q], ss


def _device_scaled(h, X, Y):
    """(T, Ys, c, h, y_mean, y_scale): the scaled inputs and targets in fp64 from the handle's own scalings"""
    c, hh, mean, scale = (h.download(k) for k in ("c", "h", "y_mean", "y_scale"))
    return mt.scale_inputs(X, c, hh), mt.scale_targets(Y, mean, scale), c, hh, mean, scale


def _check_loss_grad(name, L, g, w, sizes, activation, T, Ys, alpha):
    from romhighcontrast_amd.nonlinear import mlp_loss_grad_host
    Ln, gn = mlp_loss_grad_host(w, sizes, activation, T, Ys, alpha)
    nl, ng = mt.ratios(Ln, gn, w, sizes, activation, T, Ys, alpha)
    rl, rg = mt.ratios(L, g, w, sizes, activation, T, Ys, alpha)
    observed(f"mlp {name}: |device loss - 80-bit| / ((M + sum K + 32) eps L_abs)  [NumPy fp64 {nl:.1e}]", rl, 1.0)
    observed(f"mlp {name}: max |device grad - 80-bit| / ((M + sum K + 32) eps G_abs)  [NumPy fp64 {ng:.1e}]", rg, 1.0)
    return rl, rg


@pytest.mark.parametrize("case", mt.CASES, ids=[c[0] for c in mt.CASES])
def test_loss_and_gradient(ctx, case):
    cid, m, hidden, q, M, activation, gain, alpha, seed = case
    X, Y, w, sizes = mt.case_data(case)
    blk = Block(ctx, X, Y)
    h = _fit(ctx, blk, M, hidden, w, activation, alpha)
    assert h.info["iterations"] == 0 and h.info["evaluations"] == 1 and h.info["stop_reason"] == "budget", h.info
    assert h.query()["M_train"] == M and h.query()["P"] == len(w) and (h.m, h.q) == (m, q)
    assert _same_bits(h.download("w"), w), "max_iter = 0: the handle holds w0"
    T, Ys, c, hh, mean, scale = _device_scaled(h, X[:M], Y[:M])
    c0, h0, mean0, scale0 = mt.scalings(X[:M], Y[:M])
    assert _same_bits(c, c0) and _same_bits(hh, h0), "mid-range and half-range: the bits of 0.5 min + 0.5 max, 0.5 max - 0.5 min"
    observed(f"mlp {cid}: |y_mean - NumPy| / (2 (M + 2) eps mean|y|)",
             np.abs(mean - mean0) / (2 * (M + 2) * EPS * np.abs(Y[:M]).mean(axis=0)), 1.0)
    observed(f"mlp {cid}: |y_scale - NumPy| / (4 (M + 8) eps y_scale)", np.abs(scale - scale0) / (4 * (M + 8) * EPS * scale0), 1.0)
    if cid == mt.CONSTANT_COLUMNS_CASE:
        assert hh[2] == 0.0 and c[2] == 1.75 and mean[3] == -0.5 and scale[3] == 1.0 and not T[:, 2].any() and not Ys[:, 3].any()
    L, g = h.loss_grad(blk.buf, blk.x_off(0), blk.ld, blk.buf, blk.y_off(0), blk.ld, M)
    _check_loss_grad(cid, L, g, w, sizes, activation, T, Ys, alpha)
    observed(f"mlp {cid}: |loss of rom_mlp_fit's info - rom_mlp_loss_grad's|", abs(h.info["loss"] - L), 0.0)
    observed(f"mlp {cid}: | |g|_inf of rom_mlp_fit's info - rom_mlp_loss_grad's|", abs(h.info["grad_inf"] - np.abs(g).max()), 0.0)
    L2, g2 = h.loss_grad(blk.buf, blk.x_off(0), blk.ld, blk.buf, blk.y_off(0), blk.ld, M)
    assert L2 == L and _same_bits(g2, g), "a repeated call gives the same bits"
    # a held-out block of another M through the same handle (its scalings), another alpha
    Th, Yh = mt.scale_inputs(X[M:], c, hh), mt.scale_targets(Y[M:], mean, scale)
    Lh, gh = h.loss_grad(blk.buf, blk.x_off(M), blk.ld, blk.buf, blk.y_off(M), blk.ld, mt.HELD_OUT, alpha=0.5)
    _check_loss_grad(cid + " held-out", Lh, gh, w, sizes, activation, Th, Yh, 0.5)
    assert blk.unchanged(), (cid, "inputs and the NaNs around them")


@pytest.mark.parametrize("case", mt.CASES, ids=[c[0] for c in mt.CASES])
def test_prediction(ctx, case):
    cid, m, hidden, q, M, activation, gain, alpha, seed = case
    X, Y, w, sizes = mt.case_data(case)
    blk = Block(ctx, X, Y)
    h = _fit(ctx, blk, M, hidden, w, activation, alpha)
    rows = M + mt.HELD_OUT
    T, _, c, hh, mean, scale = _device_scaled(h, X, Y)
    pred, ss = _predict(ctx, h, blk, 0, rows, sumsq=True)
    out, _ = mt.forward(w, sizes, activation, T)
    truth = mean.astype(LD) + scale.astype(LD) * out
    _, _, out_abs = mt.abs_propagation(w, sizes, activation, T, np.zeros((rows, q)), 0.0)
    bound = (sum(sizes[:-1]) + 32) * EPS * (np.abs(mean).astype(LD) + scale.astype(LD) * out_abs)
    out64, _ = mt.forward(w, sizes, activation, T, dtype=np.float64)
    r64 = float((np.abs((mean + scale * out64).astype(LD) - truth) / bound).max())
    observed(f"mlp {cid}: max |device prediction - 80-bit| / ((sum K + 32) eps abs-propagated output)  [NumPy fp64 {r64:.1e}]",
             (np.abs(pred.astype(LD) - truth) / bound).astype(np.float64), 1.0)
    diff, ss_d = _predict(ctx, h, blk, 0, rows, Yref=blk.buf, r_off=blk.y_off(0), ldr=blk.ld, sumsq=True)
    assert _same_bits(diff, Y - pred), "Yref mode = Yref - prediction of the plain mode, bit for bit"
    for name, vals, got in (("prediction", pred, ss), ("Yref - prediction", diff, ss_d)):
        want = (vals.astype(LD) ** 2).sum(axis=0)
        observed(f"mlp {cid} sumsq_host of the {name}: |device - long double| / ((rows + 2) eps sum)",
                 np.abs(got.astype(LD) - want).astype(np.float64) / ((rows + 2) * EPS * want.astype(np.float64)), 1.0)
    only = h.predict(blk.buf, blk.x_off(0), blk.ld, rows, OUT=None, Yref=blk.buf, r_off=blk.y_off(0), ldr=blk.ld, sumsq=True)
    assert _same_bits(only, ss_d), "OUT = NULL: the same sums"
    pred2, _ = _predict(ctx, h, blk, 0, rows)
    assert _same_bits(pred2, pred) and blk.unchanged()


def test_raw_targets(ctx):
    """scale_targets = 0: mean 0 and scale 1, scikit-learn's loss on the raw targets"""
    case = mt.CASES[0]
    cid, m, hidden, q, M, activation, gain, alpha, seed = case
    X, Y, w, sizes = mt.case_data(case)
    blk = Block(ctx, X, Y)
    h = _fit(ctx, blk, M, hidden, w, activation, alpha, scale_targets=False)
    T, Ys, c, hh, mean, scale = _device_scaled(h, X[:M], Y[:M])
    assert not mean.any() and (scale == 1.0).all() and _same_bits(Ys, Y[:M])
    L, g = h.loss_grad(blk.buf, blk.x_off(0), blk.ld, blk.buf, blk.y_off(0), blk.ld, M)
    _check_loss_grad(cid + " raw targets", L, g, w, sizes, activation, T, Ys, alpha)


@pytest.mark.parametrize("case", mt.OPT_CASES, ids=[c[0] for c in mt.OPT_CASES])
def test_optimiser_against_its_specification(ctx, case):
    from romhighcontrast_amd.nonlinear import MLPMap, mlp_fit_host
    cid, m, hidden, q, M, activation, seed = case
    X, Y, sizes = mt.opt_data(case)
    blk = Block(ctx, X, Y)
    w0 = MLPMap.initial_weights(sizes, activation, seed)
    T = Ys = None
    for it in (1, 2, 3):
        h = _fit(ctx, blk, M, hidden, w0, activation, mt.OPT_ALPHA, max_iter=it, tol=mt.OPT_TOL, memory=mt.OPT_MEMORY)
        if T is None:
            T, Ys = _device_scaled(h, X, Y)[:2]
        args = (w0, sizes, activation, T, Ys, mt.OPT_ALPHA, it, mt.OPT_TOL, mt.OPT_MEMORY)
        spec64, spec = mlp_fit_host(*args), mlp_fit_host(*args, dtype=LD)
        assert spec64["trials"] == spec["trials"], "the condition on the fixed cases (tests/test_mlp_host.py)"
        assert h.info["iterations"] == spec["iterations"] == it and h.info["evaluations"] == spec["evaluations"], (h.info, spec["trials"])
        assert h.info["stop_reason"] == "budget"
        w = h.download("w")
        tol = 64 * max(float(np.abs(spec64["w"] - spec["w"]).max()), EPS * float(np.abs(w).max()))
        observed(f"mlp {cid}: max |device w - specification in long double| after {it} iterations / (64 x |fp64 - long double|, floor 64 eps max|w|)",
                 float(np.abs(w.astype(LD) - spec["w"]).max()) / tol, 1.0)
        curve = h.download("loss_curve")
        assert curve.shape == (it + 1,) and np.all(np.diff(curve) <= 0) and curve[-1] == h.info["loss"]
        np.testing.assert_allclose(curve, spec["loss_curve"].astype(np.float64), rtol=1e-12)
    assert blk.unchanged()


def test_full_fit(ctx):
    from romhighcontrast_amd.nonlinear import MLPMap, PolynomialMap
    m, hidden, q, M, n_out, activation, alpha, tol = 4, [20, 20], 5, 1000, 200, "tanh", 1e-4, 1e-6
    rng = np.random.default_rng(11)
    X = rng.uniform(-1, 1, (M + n_out, m))
    Y = mt.smooth_map(X, q)
    sizes = [m] + hidden + [q]
    blk = Block(ctx, X, Y)
    w0 = MLPMap.initial_weights(sizes, activation, 0)
    h = _fit(ctx, blk, M, hidden, w0, activation, alpha, max_iter=200, tol=tol)
    print(f"full fit: {h.info}")
    curve = h.download("loss_curve")
    assert curve.shape == (h.info["iterations"] + 1,) and np.all(np.diff(curve) <= 0), "the loss history is non-increasing"
    assert curve[-1] == h.info["loss"] < 0.05 * curve[0]
    w = h.download("w")
    T, Ys, c, hh, mean, scale = _device_scaled(h, X[:M], Y[:M])
    Lt, Gt = mt.loss_grad(w, sizes, activation, T, Ys, alpha)
    La, Ga, _ = mt.abs_propagation(w, sizes, activation, T, Ys, alpha)
    f = LD(mt.bound_factor(sizes, M))
    observed("mlp full fit: |reported final loss - 80-bit at the downloaded weights| / bound", float(abs(LD(h.info["loss"]) - Lt) / (f * La)), 1.0)
    gbound = float((f * Ga).max())
    observed("mlp full fit: | reported |g|_inf - 80-bit | / bound", abs(h.info["grad_inf"] - float(np.abs(Gt).max())) / gbound, 1.0)
    if h.info["stop_reason"] == "gradient":
        assert float(np.abs(Gt).max()) <= tol + gbound
    pred, _ = _predict(ctx, h, blk, M, n_out)
    lin = PolynomialMap(1, ctx=ctx).fit(X[:M], Y[:M]).predict(X[M:])
    rmse = np.sqrt(((pred - Y[M:]) ** 2).mean(axis=0))
    rmse_lin = np.sqrt(((lin - Y[M:]) ** 2).mean(axis=0))
    print(f"full fit: held-out RMSE {rmse}, of the linear fit {rmse_lin}")
    assert (rmse < rmse_lin).all(), (rmse, rmse_lin)
    h2 = _fit(ctx, blk, M, hidden, w0, activation, alpha, max_iter=200, tol=tol)
    assert _same_bits(h2.download("w"), w) and h2.info == h.info, "a second fit from the same w0 gives the same bits"
    assert blk.unchanged()


# ---- the protocol of PolynomialMap ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scores(ctx):
    from src.experiments import NonLinearROM as NL
    out = NL.vn_family_sampler(1000, (2, 2), 1, 100, 5)
    pca = NL.pca_tall(ctx, out["solutions"], center=True, scores=True, download=False)
    return dict(pca=pca, Sd=pca.scores, S=pca.scores.numpy())


def test_fit_predict_return_what_they_were_given(ctx):
    from romhighcontrast_amd.lib.SolutionsManagers import DeviceArray
    from romhighcontrast_amd.nonlinear import MLPMap
    rng = np.random.default_rng(3)
    X = rng.uniform(-1, 1, (200, 3))
    Y = mt.smooth_map(X, 2)
    model = MLPMap((8,), max_iter=15, ctx=ctx)
    assert model.fit(X, Y) is model
    pred = model.predict(X)
    assert isinstance(pred, np.ndarray) and pred.shape == (200, 2)
    Xd = DeviceArray(ctx.upload(X), 200, 3)
    pd = MLPMap((8,), max_iter=15, ctx=ctx).fit(Xd, DeviceArray(ctx.upload(Y), 200, 2)).predict(Xd)
    assert isinstance(pd, DeviceArray) and _same_bits(pd.numpy(), pred)
    assert [cf.shape for cf in model.coefs_] == [(3, 8), (8, 2)] and [b.shape for b in model.intercepts_] == [(8,), (2,)]
    assert model.n_iter_ == model.info_["iterations"] == len(model.loss_curve_) - 1 and model.loss_ == model.loss_curve_[-1]
    # y as a vector: one target column
    one = MLPMap((8,), max_iter=5, ctx=ctx).fit(X, Y[:, 0]).predict(X)
    assert one.shape == (200, 1)
    # the attributes are the map: a NumPy forward pass with coefs_ / intercepts_ and the scalings reproduces predict
    hm = model.map_
    a = mt.scale_inputs(X, hm.download("c"), hm.download("h"))
    a = np.tanh(a @ model.coefs_[0] + model.intercepts_[0]) @ model.coefs_[1] + model.intercepts_[1]
    np.testing.assert_allclose(hm.download("y_mean") + hm.download("y_scale") * a, pred, rtol=0, atol=1e-12)


@pytest.mark.parametrize("only_j", [1, 20])
def test_experiment_functions(ctx, scores, only_j):
    from src.experiments import NonLinearROM as NL
    S, Sd = scores["S"], scores["Sd"]
    n_test, n_train, w = 100, 900, NL.MWhere(m=4, start=0)
    mh, md = NL.MLPMap(max_iter=20, ctx=ctx), NL.MLPMap(max_iter=20, ctx=ctx)
    host = NL.learn_eigenvalues(mh)(n_train, n_test, S, w, only_j)
    dev = NL.learn_eigenvalues_device(model=md, ctx=ctx)(n_train, n_test, Sd, w, only_j)
    assert NL.learn_eigenvalues(mh).__name__ == NL.learn_eigenvalues_device(model=md).__name__ == "NN device"
    assert host["error"].shape == dev["error"].shape == (n_test, only_j) and dev["rmse"].shape == (only_j,)
    assert _same_bits(mh.map_.download("w"), md.map_.download("w")), "the same weights by both routes"
    observed(f"learn_eigenvalues(MLPMap) vs learn_eigenvalues_device(model=MLPMap), only_j = {only_j}: max |error difference| / 1e-12",
             np.abs(host["error"] - dev["error"]).max() / 1e-12, 1.0)
    want = np.sqrt((dev["error"] ** 2).mean(axis=0))
    np.testing.assert_allclose(dev["rmse"], want, rtol=(n_test + 2) * 2 * EPS)


def test_decoder(ctx, scores):
    from src.experiments import NonLinearROM as NL
    S, Sd, pca = scores["S"], scores["Sd"], scores["pca"]
    m, q, n_test = 4, 16, 100
    model = NL.MLPMap(max_iter=20, ctx=ctx).fit_columns(Sd, (0, m), Sd, (m, m + q), n_test, 900)
    known = S[:n_test, :m]
    rec = NL.nonlinear_reconstruction(pca, model, known)
    V, mean = pca.components_.numpy(), pca.mean_.numpy().ravel()
    pred = np.asarray(model.predict(known))
    want = mean + known @ V[:m] + pred @ V[m:m + q]
    observed("nonlinear_reconstruction with an MLPMap vs NumPy on the map's own predictions / (1e-13 ||row||)",
             np.linalg.norm(rec - want, axis=1) / (1e-13 * np.linalg.norm(want, axis=1)), 1.0)


def test_error_cases(ctx):
    from romhighcontrast_amd import _ffi
    from romhighcontrast_amd.nonlinear import MLPMap
    rng = np.random.default_rng(0)
    X, Y = rng.uniform(-1, 1, (50, 3)), rng.standard_normal((50, 2))
    for bad_x, bad_y in ((np.nan, None), (np.inf, None), (None, np.nan), (None, -np.inf)):
        Xb, Yb = X.copy(), Y.copy()
        if bad_x is not None:
            Xb[7, 1] = bad_x
        if bad_y is not None:
            Yb[11, 0] = bad_y
        with pytest.raises(ValueError, match="NaN / Inf"):
            MLPMap((5,), ctx=ctx).fit(Xb, Yb)
    Z = ctx.upload(np.hstack((X, Y)))
    w0 = MLPMap.initial_weights([3, 5, 2], "tanh", 0)
    w0[4] = np.nan
    with pytest.raises(ValueError, match="NaN / Inf"):
        ctx.mlp_fit(Z, 0, 5, 3, Z, 3, 5, 2, 50, [5], w0)
    w0[4] = 0.1
    with pytest.raises(ValueError):
        ctx.mlp_fit(Z, 0, 5, 3, Z, 3, 5, 2, 50, [65], w0)
    with pytest.raises(ValueError):
        ctx.mlp_fit(Z, 0, 5, 3, Z, 3, 5, 2, 50, [5], w0[:-1])

    def fails(words, fn, *args, **kw):
        with pytest.raises(_ffi.RomLibraryError) as ei:
            fn(*args, **kw)
        assert all(w in str(ei.value) for w in words), str(ei.value)

    fails(["rom_mlp_fit", "M = 0"], ctx.mlp_fit, Z, 0, 5, 3, Z, 3, 5, 2, 0, [5], w0)
    fails(["rom_mlp_fit", "X holds 250"], ctx.mlp_fit, Z, 3, 5, 3, Z, 3, 5, 2, 50, [5], w0)
    fails(["rom_mlp_fit", "memory"], ctx.mlp_fit, Z, 0, 5, 3, Z, 3, 5, 2, 50, [5], w0, memory=0)
    h = ctx.mlp_fit(Z, 0, 5, 3, Z, 3, 5, 2, 50, [5], w0, max_iter=2)
    out = ctx.alloc(100)
    fails(["rom_mlp_predict", "OUT == NULL"], h.predict, Z, 0, 5, 50)
    fails(["rom_mlp_predict", "X holds 250"], h.predict, Z, 0, 5, 51, OUT=out)
    fails(["rom_mlp_predict", "OUT holds 100"], h.predict, Z, 0, 5, 50, OUT=out, o_off=1)
    fails(["rom_mlp_predict", "OUT overlaps X"], h.predict, Z, 0, 5, 40, OUT=Z, o_off=3, ldo=5)
    fails(["rom_mlp_loss_grad", "Y holds 250"], h.loss_grad, Z, 0, 5, Z, 4, 5, 50)
    fails(["rom_mlp_download", "count"], lambda: _ffi.check(ctx.lib.rom_mlp_download(h.h, 0, np.zeros(4).ctypes.data, 4)))


def test_blocks_that_end_on_the_last_double_of_their_buffers(ctx):
    import tight_blocks as tb
    from romhighcontrast_amd import _ffi
    from romhighcontrast_amd.nonlinear import MLPMap
    w0 = MLPMap.initial_weights([tb.m, 5, tb.q], "tanh", 0)
    h, bufs = tb.check(ctx, "rom_mlp", lambda *blocks: ctx.mlp_fit(*blocks, [5], w0, max_iter=3))
    # rom_mlp_loss_grad reads X and Y the same way
    (loss, grad), (loss64, grad64) = (h.loss_grad(bufs[s][0], tb.X_OFF, tb.LD, bufs[s][1], tb.Y_OFF, tb.LD, tb.M) for s in (0, 64))
    assert _same_bits([loss], [loss64]) and _same_bits(grad, grad64)
    for words, s_x, s_y in ((f"X holds {bufs[-1][0].n}", -1, 0), (f"Y holds {bufs[-1][1].n}", 0, -1)):
        with pytest.raises(_ffi.RomLibraryError, match=words):
            h.loss_grad(bufs[s_x][0], tb.X_OFF, tb.LD, bufs[s_y][1], tb.Y_OFF, tb.LD, tb.M)


def test_estimator_nn(ctx):
    from src.lib.Estimators import EstimatorNN
    from romhighcontrast_amd.nonlinear import MLPMap
    rng = np.random.default_rng(4)
    n, n_par, K = 5, 2, 64
    a_base = rng.uniform(1, 10, (n, n_par))
    c_values = rng.dirichlet(np.ones(n), K)
    a_values = c_values @ a_base + 0.1 * np.sin(c_values @ a_base)
    est = EstimatorNN(a_base, (8, 8), max_iter=30, ctx=ctx).fit(c_values, a_values)
    got = est.estimate_parameter(c_values)
    assert got.shape == (K, n_par)
    for i in range(n_par):
        Xi = c_values * a_base[:, i]
        by_hand = MLPMap((8, 8), max_iter=30, ctx=ctx).fit(Xi, a_values[:, i]).predict(Xi).ravel()
        assert _same_bits(got[:, i], by_hand)
    assert np.sqrt(((got - a_values) ** 2).mean()) < a_values.std()
