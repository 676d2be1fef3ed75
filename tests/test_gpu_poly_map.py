"""rom_poly_fit / rom_poly_predict on the GPU against an 80-bit least squares (tests/poly_truth.py).

THE BOUND.  Per target column: RMS over the held-out rows of |device prediction - prediction of the 80-bit fit|, divided by
the RMS of the training target column, must be <= C eps kappa_2(Phi^) + M eps with C = 64, eps = 2^-53 (as
test_gpu_pca_tall.py), Phi^ the column-normalised Legendre design matrix formed here on the host, and M eps the gamma_M of a
dot product of length M in any summation order.  numpy.linalg.lstsq on the same Phi is printed next to every device figure.

Cases: the smallest shapes that reach each path of the kernels -- P padded to 16 with M no multiple of 32; P = 70 over several
workgroup chunks with a 5-row tail; P = 91 with two target groups and q no multiple of 16; one input at degree 8; P = 15, 16
and 17 around one 16-column tile with one-row last slabs; fewer rows
than terms (rank < P); two inputs that agree to 2^-25 (kappa = 7e7: the re-whitening and a third pass).  X and Y are column ranges of ONE wider block whose other entries, and the sentinel rows around it, are
NaN: the NaNs and both inputs must come back bit for bit.  Real scores: the (2, 2) / N = 5 problem of the reference's
experiment, 3000 samples."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import observed
import poly_truth as pt

pytestmark = pytest.mark.gpu
LD, EPS, C = pt.LD, pt.EPS, pt.C
N_TEST = 100

#            id             m  d   M    q
CASES = [("p10_m300",       3, 2, 300, 5),
         ("p70_m4101",      4, 4, 4101, 5),
         ("p91_q100",       12, 2, 2048, 100),
         ("p9_deg8",        1, 8, 257, 1),
         # tile and slab edges of the slab engine (csrc/rom_slab.h): P = 16 is one tile, with a full target group and two slabs
         # per chunk of which the last holds one row; P = 17 pads to 32, with a second target group of one column and a one-row
         # second slab; P = 15 with q = 17: q_pad = 32 with 15 padded columns
         ("p16_q96_m8193",  15, 1, 8193, 96),
         ("p17_q97_m33",    16, 1, 33, 97),
         ("p15_q17_m1025",  2, 4, 1025, 17),
         ("p84_m31_rank",   6, 3, 31, 3)]
FULL_RANK = CASES[:-1]


@pytest.fixture(scope="module")
def ctx():
    from romhighcontrast_amd import _ffi
    return _ffi.get_context()


def _same_bits(a, b):
    return np.array_equal(np.asarray(a).view(np.uint64), np.asarray(b).view(np.uint64))


class Block:
    """X (m columns from column 3) and Y (q columns from column 3 + m + 2) inside one block of ld = m + q + 6 columns,
    rows [2, 2 + M + N_TEST) of it; every other entry is NaN."""

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


def _fit(ctx, blk, M, d, rcond=0.0):
    return ctx.poly_fit(blk.buf, blk.x_off(0), blk.ld, blk.m, blk.buf, blk.y_off(0), blk.ld, blk.q, M, d, rcond)


def _predict(ctx, pm, blk, row0, rows, **kw):
    """Predictions for rows [row0, row0 + rows) of the block, into a NaN block of ld = q + 3 from column 2, rows [1, 1 + rows)."""
    ldo = blk.q + 3
    out = ctx.alloc((rows + 2) * ldo).fill(np.nan)
    ss = pm.predict(blk.buf, blk.x_off(row0), blk.ld, rows, OUT=out, o_off=ldo + 2, ldo=ldo, **kw)
    full = out.download(shape=(rows + 2, ldo))
    assert np.isnan(full[0]).all() and np.isnan(full[-1]).all() and np.isnan(full[:, :2]).all() and np.isnan(full[:, 2 + blk.q:]).all()
    return full[1:1 + rows, 2:2 + blk.q], ss


def _synthetic(m, d, M, q, seed):
    rng = np.random.default_rng(seed)
    scale = 10.0 ** -np.arange(m)
    X = rng.uniform(-1, 1, (M + N_TEST, m)) * scale + 0.3 * scale
    pw = pt.powers(m, d)
    c, h = pt.midrange(X[:M])
    Phi = pt.features(X, c, h, pw)
    Y0 = Phi @ rng.standard_normal((len(pw), q))
    return X, Y0, Y0 + 0.1 * rng.standard_normal(Y0.shape), pw, c, h


def _truth(X, Y, M, pw, c, h):
    """(80-bit predictions of all rows, kappa of the normalised design matrix, fp64 lstsq predictions)"""
    PhiL = pt.features(X, c, h, pw, dtype=LD)
    W, kept = pt.lstsq_ld(PhiL[:M], Y[:M])
    Phi = PhiL.astype(np.float64)
    lap = Phi @ np.linalg.lstsq(Phi[:M], Y[:M], rcond=None)[0]
    return (PhiL @ W), pt.kappa_normalised(Phi[:M]), lap, bool(kept.all())


def _ratio(pred, truth, Ytrain, kappa, M):
    """per column: RMS |pred - truth| / RMS(train target) / (C eps kappa + M eps)"""
    err = pt.rms(np.asarray(pred, dtype=LD) - truth)
    return err / np.maximum(pt.rms(Ytrain), 1e-300) / (C * EPS * kappa + M * EPS)


@pytest.mark.parametrize("cid,m,d,M,q", FULL_RANK, ids=[c[0] for c in FULL_RANK])
def test_synthetic_full_rank(ctx, cid, m, d, M, q, monkeypatch):
    X, Y0, Y1, pw, c, h = _synthetic(m, d, M, q, seed=m * 100 + d)
    for tag, Y in (("exact", Y0), ("noisy", Y1)):
        blk = Block(ctx, X, Y)
        pm = _fit(ctx, blk, M, d)
        info = pm.info
        print(f"{cid} {tag}: {info}")
        assert info["P"] == len(pw) and info["rank"] == len(pw) and info["stop_reason"] == "full_rank" and 2 <= info["passes"] <= 3, info
        assert pm.query() == dict(m=m, d=d, P=len(pw), q=q, rank=len(pw), M_train=M, passes=info["passes"], host_syncs=info["host_syncs"])
        assert _same_bits(pm.download("c"), c) and _same_bits(pm.download("h"), h) and not pm.download("dropped").any()
        pred, _ = _predict(ctx, pm, blk, M, N_TEST)
        assert blk.unchanged(), (cid, "inputs and the NaNs around them")
        truth, kappa, lap, full = _truth(X, Y, M, pw, c, h)
        assert full
        r_lap = _ratio(lap[M:], truth[M:], Y[:M], kappa, M).max()
        print(f"{cid} {tag}: kappa = {kappa:.3g}, delta = {info['delta_max']:.2e}, numpy.linalg.lstsq ratio = {r_lap:.3e}")
        observed(f"poly {cid} {tag}: held-out RMS |device - 80-bit| / RMS(y) / (C eps kappa + M eps)  [lstsq {r_lap:.1e}]",
                 _ratio(pred, truth[M:], Y[:M], kappa, M), 1.0)
        if tag == "noisy":
            # the same bits on a second fit + predict, and with poisoned workspaces
            W = pm.download("W")
            for poison in (False, True):
                if poison:
                    monkeypatch.setenv("ROMHC_POISON_WS", "1")
                pm2 = _fit(ctx, blk, M, d)
                pred2, _ = _predict(ctx, pm2, blk, M, N_TEST)
                if poison:
                    monkeypatch.delenv("ROMHC_POISON_WS")
                assert _same_bits(pm2.download("W"), W) and _same_bits(pred2, pred) and pm2.info == info, (cid, "poisoned" if poison else "repeat")


def test_fewer_rows_than_terms(ctx):
    cid, m, d, M, q = CASES[-1]
    X, Y0, Y1, pw, c, h = _synthetic(m, d, M, q, seed=63)
    Phi = pt.features(X[:M], c, h, pw)
    kappa = pt.kappa_normalised(Phi, rank=M)     # (31 rows: the ratio of the largest to the 31st singular value)
    for tag, Y in (("exact", Y0), ("noisy", Y1)):
        blk = Block(ctx, X, Y)
        pm = _fit(ctx, blk, M, d)
        print(f"{cid} {tag}: {pm.info}, kappa_31 = {kappa:.3g}")
        assert pm.info["stop_reason"] == "terms_dropped" and pm.info["rank"] <= 31 and pm.info["P"] == 84, pm.info
        dropped = pm.download("dropped")
        assert dropped.sum() == 84 - pm.info["rank"] and not pm.download("W")[:, dropped > 0].any()
        pred, _ = _predict(ctx, pm, blk, 0, M)
        W, _ = pt.lstsq_ld(pt.features(X[:M], c, h, pw, dtype=LD), Y[:M])
        res_truth = pt.rms(Y[:M].astype(LD) - pt.features(X[:M], c, h, pw, dtype=LD) @ W)
        res_dev = pt.rms(Y[:M].astype(LD) - pred.astype(LD))
        observed(f"poly {cid} {tag}: |RMS training residual - 80-bit's| / RMS(y) / (C eps kappa_31 + M eps)",
                 np.abs(res_dev - res_truth) / pt.rms(Y[:M]) / (C * EPS * kappa + M * EPS), 1.0)
        assert blk.unchanged()


def test_prediction_modes(ctx):
    m, d, M, q = 3, 3, 777, 21
    X, Y0, Y1, pw, c, h = _synthetic(m, d, M, q, seed=5)
    blk = Block(ctx, X, Y1)
    pm = _fit(ctx, blk, M, d)
    rows = M + N_TEST
    pred, ss = _predict(ctx, pm, blk, 0, rows, sumsq=True)
    diff, ss_d = _predict(ctx, pm, blk, 0, rows, Yref=blk.buf, r_off=blk.y_off(0), ldr=blk.ld, sumsq=True)
    assert _same_bits(diff, Y1 - pred), "Yref mode = Yref - prediction of the plain mode, bit for bit"
    for name, vals, got in (("prediction", pred, ss), ("Yref - prediction", diff, ss_d)):
        want = (vals.astype(LD) ** 2).sum(axis=0)
        observed(f"poly sumsq_host of the {name}: |device - long double| / ((M + 2) eps sum)",
                 np.abs(got.astype(LD) - want).astype(np.float64) / ((rows + 2) * EPS * want.astype(np.float64)), 1.0)
    only = pm.predict(blk.buf, blk.x_off(0), blk.ld, rows, OUT=None, Yref=blk.buf, r_off=blk.y_off(0), ldr=blk.ld, sumsq=True)
    assert _same_bits(only, ss_d), "OUT = NULL: the same sums"
    assert blk.unchanged()


def test_scale_invariance(ctx):
    """The property that motivates the feature: input column j times 2^(10 j) gives the same map."""
    m, d, M, q = 4, 4, 1500, 5
    X, Y0, Y1, pw, c, h = _synthetic(m, d, M, q, seed=11)
    blk = Block(ctx, X, Y1)
    pred, _ = _predict(ctx, _fit(ctx, blk, M, d), blk, M, N_TEST)
    Xs = X * 2.0 ** (10 * np.arange(m))
    blk_s = Block(ctx, Xs, Y1)
    pm_s = _fit(ctx, blk_s, M, d)
    pred_s, _ = _predict(ctx, pm_s, blk_s, M, N_TEST)
    kappa = pt.kappa_normalised(pt.features(X[:M], c, h, pw))
    observed("poly scale invariance: held-out RMS |scaled fit - unscaled fit| / RMS(y) / (C eps kappa + M eps)",
             _ratio(pred_s, pred.astype(LD), Y1[:M], kappa, M), 1.0)
    assert pm_s.info["rank"] == len(pw)


def test_third_pass_near_the_limit_of_the_method(ctx):
    """Two inputs that agree to 2^-25: kappa(Phi^) = 7e7, at the eps^-1/2 limit of a Cholesky factorisation of the Gram matrix
    (with an explicit rcond: the squared pivot of the third term, 9e-16 of the largest, sits at the default's P eps = 3e-16).  kappa^2 eps is of order one, so the Gram
    matrix of pass 2 is far from I: the re-whitening and a third pass must run, and the bound must hold after it."""
    M, q = 2000, 2
    rng = np.random.default_rng(7)
    x1 = rng.uniform(-1, 1, M + N_TEST)
    X = np.column_stack((x1, x1 + 2.0 ** -25 * rng.uniform(-1, 1, M + N_TEST)))
    pw = pt.powers(2, 1)
    c, h = pt.midrange(X[:M])
    Y = pt.features(X, c, h, pw) @ rng.standard_normal((3, q)) + 0.1 * rng.standard_normal((M + N_TEST, q))
    blk = Block(ctx, X, Y)
    pm = _fit(ctx, blk, M, 1, rcond=1e-10)
    truth, kappa, lap, full = _truth(X, Y, M, pw, c, h)
    print(f"third pass: {pm.info}, kappa = {kappa:.3g}")
    assert full and pm.info["rank"] == 3 and pm.info["stop_reason"] == "full_rank" and 3 <= pm.info["passes"] <= 4, pm.info
    assert pm.info["delta_max"] * 3 <= 1.0 / 3.0
    pred, _ = _predict(ctx, pm, blk, M, N_TEST)
    r_lap = _ratio(lap[M:], truth[M:], Y[:M], kappa, M).max()
    observed(f"poly three passes, kappa = {kappa:.1e}: held-out RMS |device - 80-bit| / RMS(y) / (C eps kappa + M eps)  [lstsq {r_lap:.1e}]",
             _ratio(pred, truth[M:], Y[:M], kappa, M), 1.0)
    # the squared pivot of that term is 9e-16 of the largest: rcond = 1e-6 (1e-12) drops it, and the map says so
    pm0 = _fit(ctx, blk, M, 1, rcond=1e-6)
    assert pm0.info["rank"] == 2 and pm0.info["stop_reason"] == "terms_dropped" and pm0.download("dropped").sum() == 1, pm0.info


# ---- real scores: the reference's experiment at 3000 samples -------------------------------------------------------------
@pytest.fixture(scope="module")
def scores(ctx):
    from src.experiments import NonLinearROM as NL
    out = NL.vn_family_sampler(3000, (2, 2), 1, 100, 5)
    pca = NL.pca_tall(ctx, out["solutions"], center=True, scores=True, download=False)
    S = pca.scores.numpy()
    return dict(pca=pca, Sd=pca.scores, S=S, U=np.asarray(out["solutions"]))


@pytest.mark.parametrize("d", [1, 2, 4])
def test_real_scores(ctx, scores, d):
    from src.experiments import NonLinearROM as NL
    S, Sd = scores["S"], scores["Sd"]
    m, q, M = 4, 16, 3000 - N_TEST
    Xtr, Ytr, Xte = S[N_TEST:, :m], S[N_TEST:, m:m + q], S[:N_TEST, :m]
    model = NL.PolynomialMap(d, ctx=ctx).fit_columns(Sd, (0, m), Sd, (m, m + q), N_TEST, M)
    assert model.info_["rank"] == model.info_["P"] and model.info_["passes"] <= 3, model.info_
    out = ctx.alloc(N_TEST * q)
    model.map_.predict(Sd.buf, 0, Sd.dim, N_TEST, OUT=out)
    pred = out.download(shape=(N_TEST, q))
    pw = pt.powers(m, d)
    c, h = pt.midrange(Xtr)
    PhiL = pt.features(np.vstack((Xtr, Xte)), c, h, pw, dtype=LD)
    W, kept = pt.lstsq_ld(PhiL[:M], Ytr)
    assert kept.all()
    truth = PhiL[M:] @ W
    Phi = PhiL.astype(np.float64)
    kappa = pt.kappa_normalised(Phi[:M])
    lap = Phi[M:] @ np.linalg.lstsq(Phi[:M], Ytr, rcond=None)[0]
    r_lap = _ratio(lap, truth, Ytr, kappa, M).max()
    print(f"real scores d = {d}: {model.info_}, kappa = {kappa:.3g}, numpy.linalg.lstsq on Phi ratio = {r_lap:.3e}")
    observed(f"poly real scores d = {d}: held-out RMS |device - 80-bit| / RMS(y) / (C eps kappa + M eps)  [lstsq {r_lap:.1e}]",
             _ratio(pred, truth, Ytr, kappa, M), 1.0)
    from sklearn.linear_model import LinearRegression
    from sklearn.pipeline import Pipeline
    from sklearn.preprocessing import PolynomialFeatures
    sk = Pipeline([("poly", PolynomialFeatures(d)), ("LR", LinearRegression())]).fit(Xtr, Ytr).predict(Xte)
    r_sk = _ratio(sk, truth, Ytr, kappa, M)
    if d <= 2:
        observed(f"poly real scores d = {d}: held-out RMS |device - scikit-learn pipeline| / RMS(y) / (2 bound)",
                 _ratio(pred, sk.astype(LD), Ytr, kappa, M) / 2.0, 1.0)
    else:
        print(f"real scores d = {d}: distance from the 80-bit fit in units of the bound: scikit-learn's monomial pipeline "
              f"{r_sk.max():.3e}, device {_ratio(pred, truth, Ytr, kappa, M).max():.3e}")


def test_experiment_functions_and_decoder(ctx, scores):
    from src.experiments import NonLinearROM as NL
    S, Sd, pca = scores["S"], scores["Sd"], scores["pca"]
    m, q, n_train = 4, 16, 3000 - N_TEST
    w = NL.MWhere(m=m, start=0)
    host = NL.learn_eigenvalues(NL.PolynomialMap(2, ctx=ctx))(n_train, N_TEST, S, w, q)
    dev = NL.learn_eigenvalues_device(2, ctx=ctx)(n_train, N_TEST, Sd, w, q)
    assert host["error"].shape == dev["error"].shape == (N_TEST, q) and dev["rmse"].shape == (q,)
    Phi = pt.features(S[N_TEST:, :m], *pt.midrange(S[N_TEST:, :m]), pt.powers(m, 2))
    kappa = pt.kappa_normalised(Phi)
    observed("learn_eigenvalues(PolynomialMap(2)) vs learn_eigenvalues_device(2): RMS error difference / RMS(y) / bound",
             _ratio(dev["error"], host["error"].astype(LD), S[N_TEST:, m:m + q], kappa, n_train), 1.0)
    want = pt.rms(dev["error"])
    observed("learn_eigenvalues_device rmse vs the column RMS of its error / ((n_test + 2) eps)",
             np.abs(dev["rmse"] - want) / want / ((N_TEST + 2) * EPS), 1.0)
    # a list of unknowns in two ranges: the columns before the known block and those after it
    w2 = NL.MWhere(m=2, start=2)
    dev2 = NL.learn_eigenvalues_device(1, ctx=ctx)(n_train, N_TEST, Sd, w2, 3, learn_higher_modes_only=False)
    host2 = NL.learn_eigenvalues(NL.PolynomialMap(1, ctx=ctx))(n_train, N_TEST, S, w2, 3, learn_higher_modes_only=False)
    assert dev2["error"].shape == (N_TEST, 5) and dev2["rmse"].shape == (5,)
    kappa2 = pt.kappa_normalised(pt.features(S[N_TEST:, 2:4], *pt.midrange(S[N_TEST:, 2:4]), pt.powers(2, 1)))
    observed("learn_eigenvalues_device with two unknown ranges vs the host-array route / bound",
             _ratio(dev2["error"], host2["error"].astype(LD), S[N_TEST:, [0, 1, 4, 5, 6]], kappa2, n_train), 1.0)
    # the decoder: mean + known scores . components + predicted scores . components
    model = NL.PolynomialMap(2, ctx=ctx).fit_columns(Sd, (0, m), Sd, (m, m + q), N_TEST, n_train)
    known = S[:N_TEST, :m]
    rec = NL.nonlinear_reconstruction(pca, model, known)
    V, mean = pca.components_.numpy(), pca.mean_.numpy().ravel()
    pred = np.asarray(model.predict(known))
    want = mean + known @ V[:m] + pred @ V[m:m + q]
    observed("nonlinear_reconstruction vs NumPy on the downloaded pieces / (1e-13 ||row||)",
             np.linalg.norm(rec - want, axis=1) / (1e-13 * np.linalg.norm(want, axis=1)), 1.0)
    # ... and it is a reduced model: closer to the snapshots than the linear reconstruction from the same m coordinates
    U = scores["U"][:N_TEST]
    assert np.linalg.norm(rec - U) < np.linalg.norm(mean + known @ V[:m] - U)


# ---- the error cases of the contract -----------------------------------------------------------------------------------
def test_error_cases(ctx):
    from romhighcontrast_amd import _ffi
    from src.experiments import NonLinearROM as NL
    rng = np.random.default_rng(0)
    Z = ctx.upload(rng.standard_normal((50, 8)))

    def fails(words, fn, *args, **kw):
        with pytest.raises(_ffi.RomLibraryError) as ei:
            fn(*args, **kw)
        assert all(w in str(ei.value) for w in words), str(ei.value)

    fit = ctx.poly_fit
    fails(["rom_poly_fit", "null"], fit, None, 0, 8, 2, Z, 2, 8, 2, 50, 2)
    fails(["rom_poly_fit", "m = 0"], fit, Z, 0, 8, 0, Z, 2, 8, 2, 50, 2)
    fails(["rom_poly_fit", "m = 17"], fit, ctx.alloc(50 * 20), 0, 20, 17, Z, 2, 8, 2, 50, 1)
    fails(["rom_poly_fit", "d = 9"], fit, Z, 0, 8, 2, Z, 2, 8, 2, 50, 9)
    fails(["rom_poly_fit", "126", "96"], fit, Z, 0, 8, 4, Z, 4, 8, 2, 50, 5)
    fails(["rom_poly_fit", "q = 0"], fit, Z, 0, 8, 2, Z, 2, 8, 0, 50, 2)
    fails(["rom_poly_fit", "q = 1025"], fit, Z, 0, 8, 2, ctx.alloc(2050), 0, 1025, 1025, 2, 2)
    fails(["rom_poly_fit", "M = 0"], fit, Z, 0, 8, 2, Z, 2, 8, 2, 0, 2)
    fails(["rom_poly_fit", "ldx = 1 < m = 2"], fit, Z, 0, 1, 2, Z, 2, 8, 2, 50, 2)
    fails(["rom_poly_fit", "ldy = 2 < q = 3"], fit, Z, 0, 8, 2, Z, 2, 2, 3, 50, 2)
    fails(["rom_poly_fit", "X holds 400"], fit, Z, 7, 8, 2, Z, 2, 8, 2, 50, 2)
    fails(["rom_poly_fit", "Y holds 400"], fit, Z, 0, 8, 2, Z, 7, 8, 2, 50, 2)
    bad = rng.standard_normal((50, 8))
    bad[7, 1] = np.nan
    fails(["rom_poly_fit", "NaN / Inf"], fit, ctx.upload(bad), 0, 8, 2, Z, 2, 8, 2, 50, 2)
    bad[7, 1] = np.inf
    fails(["rom_poly_fit", "NaN / Inf"], fit, Z, 0, 8, 2, ctx.upload(bad), 0, 8, 2, 50, 2)
    with pytest.raises(ValueError):
        NL.PolynomialMap(2, ctx=ctx).fit(bad[:, :2], bad[:, 2:4])
    pm = fit(Z, 0, 8, 2, Z, 2, 8, 3, 50, 2)
    out = ctx.alloc(50 * 3)
    fails(["rom_poly_predict", "OUT == NULL"], pm.predict, Z, 0, 8, 50)
    fails(["rom_poly_predict", "ldx = 1 < m = 2"], pm.predict, Z, 0, 1, 50, OUT=out)
    fails(["rom_poly_predict", "ldo = 2 < q = 3"], pm.predict, Z, 0, 8, 50, OUT=out, ldo=2)
    fails(["rom_poly_predict", "X holds 400"], pm.predict, Z, 0, 8, 51, OUT=out)
    fails(["rom_poly_predict", "OUT holds 150"], pm.predict, Z, 0, 8, 50, OUT=out, o_off=1)
    fails(["rom_poly_predict", "Yref holds 400"], pm.predict, Z, 0, 8, 50, OUT=out, Yref=Z, r_off=6, ldr=8)
    fails(["rom_poly_predict", "OUT overlaps X"], pm.predict, Z, 0, 8, 40, OUT=Z, o_off=4, ldo=8)
    fails(["rom_poly_download", "count"], lambda: _ffi.check(ctx.lib.rom_poly_download(pm.h, 2, np.zeros(4).ctypes.data, 4)))
    # a constant input column: t = 0 for it, its higher terms drop out by the rank rule
    Zc = rng.standard_normal((50, 8))
    Zc[:, 1] = 2.5
    pmc = fit(ctx.upload(Zc), 0, 8, 2, Z, 2, 8, 2, 50, 2)
    assert pmc.info["stop_reason"] == "terms_dropped" and pmc.info["rank"] == 3 and pmc.download("h")[1] == 0.0, pmc.info


def test_blocks_that_end_on_the_last_double_of_their_buffers(ctx):
    import tight_blocks
    tight_blocks.check(ctx, "rom_poly", lambda *blocks: ctx.poly_fit(*blocks, 2))


# ---- which kernels ran: a child process (ROMHC_PROF_DETAIL is read once per process) -----------------------------------
def test_kernels_confirmed_by_profile_names():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, ROMHC_PROF_DETAIL="1")
    r = subprocess.run([sys.executable, os.path.join(root, "tests", "poly_map_child.py")], env=env, cwd=root,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    out = r.stdout.decode(errors="replace")
    print(out)
    assert r.returncode == 0 and out.rstrip().endswith("OK"), out[-4000:]
    got = json.loads([ln for ln in out.splitlines() if ln.startswith("KERNELS ")][-1][8:])
    for key, groups in (("q5", 1), ("q100", 2)):
        g = got[key]
        assert g["pass_kernel"] == g["passes"] * groups and g["per_group"] == [g["passes"]] * groups, got
        assert g["gemm"] == 0 and g["syrk_tn"] == 0 and g["predict"] == 1, got
