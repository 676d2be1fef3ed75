"""rom_mlp_sense on the GPU against mlp_sense_scores and the checker of tests/mlp_sense_truth.py.

Every call runs on NaN-framed operands -- P and OUT as column ranges of wider NaN blocks from an offset, the others with a NaN
tail -- which must come back bit for bit (OUT: everything outside its rows); every call is made twice and must return the same
bits; every result goes through check_state.  The shapes (m, hidden, activation, r, K, t) are those of mlp_sense_truth.SHAPES.

max_iter 0: t is the clipped start bit for bit, start and iterations are the host's.  max_iter 1, 2:
|t_dev - t_host| <= max(1e3 delta, 1e-11 (1 + max|t|)), delta the host's own difference when the rows of G_r and the hidden units
of every layer are permuted."""
import numpy as np
import pytest

import mlp_sense_truth as mt
from mlp_sense_truth import IDS, SHAPES

pytestmark = pytest.mark.gpu

REF = (4, (20, 20), "logistic", 12, 5, 3)


@pytest.fixture(scope="module")
def ctx():
    from romhighcontrast_amd import _ffi
    return _ffi.get_context()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


class Tail:
    """The operand followed by seven NaN."""

    def __init__(self, ctx, X):
        self.host = np.concatenate([np.asarray(X, dtype=np.float64).ravel(), np.full(7, np.nan)])
        self.buf = ctx.upload(self.host)

    def unchanged(self):
        return np.array_equal(_bits(self.buf.download()), _bits(self.host))


def run(ctx, model, P, T0, aux=None, max_iter=30, misfit_tol=1e-3, check=True):
    """rom_mlp_sense twice on NaN-framed operands; returns (SenseResult, info)."""
    m, r = model["m"], model["r"]
    P = np.atleast_2d(P)
    K = len(P)
    T0 = np.asarray(T0, dtype=np.float64).reshape(K, -1, m)
    t = T0.shape[1]
    ldp, p_off, ldo, o_off = r + 3, r + 3 + 1, m + 5 + 2, 3
    ph = np.full((K + 2, ldp), np.nan)
    ph[1:1 + K, 1:1 + r] = P
    ops = [Tail(ctx, model["WH"]), Tail(ctx, model["Gr"]), Tail(ctx, ph), Tail(ctx, T0)]
    auxb = Tail(ctx, aux) if aux is not None else None
    outs = []
    for _ in range(2):
        OUT = ctx.upload(np.full(o_off + K * ldo + 4, np.nan))
        res, info = ctx.mlp_sense(m, model["hidden"], model["activation"], ops[0].buf, r, ops[1].buf, ops[2].buf, p_off, ldp, K, t,
                                  ops[3].buf, model["lo"], model["hi"], AUX=auxb.buf if auxb else None, max_iter=max_iter,
                                  misfit_tol=misfit_tol, OUT=OUT, out_off=o_off, ldo=ldo)
        raw = OUT.download()
        body = raw[o_off:o_off + K * ldo].reshape(K, ldo)
        assert np.isnan(raw[:o_off]).all() and np.isnan(raw[o_off + K * ldo:]).all() and np.isnan(body[:, m + 5:]).all(), "OUT's frame"
        assert not np.isnan(body[:, :m + 5]).any()
        outs.append((raw, res, info))
    for op in ops + ([auxb] if auxb else []):
        assert op.unchanged(), "an input buffer was modified"
    assert np.array_equal(_bits(outs[0][0]), _bits(outs[1][0])), "two calls, different bits"
    res, info = outs[0][1], outs[0][2]
    assert info["launches"] == 2 and info["host_syncs"] == 1 and info["systems"] == K * t, info
    assert info["iterations"] <= max_iter * K * t and info["evaluations"] >= 2 * K * t, info
    if max_iter == 0:
        assert info["iterations"] == 0 and info["evaluations"] == 2 * K * t, info
    if check:
        worst = mt.check_state(model, P, aux, res, T0=T0, misfit_tol=misfit_tol, max_iter=max_iter)
        print(f"check_state: largest observed / bound {worst:.3g}; {info}")
    return res, info


@pytest.fixture(scope="module")
def cases():
    return {shape: mt.case(*shape) for shape in SHAPES}


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_recovers_exact_coordinates(ctx, cases, shape):
    model, t_true, P, T0 = cases[shape]
    res, info = run(ctx, model, P, T0)
    err = np.abs(res.t - t_true).max(axis=1)
    print(f"max |t - t*| {err.max():.3g}; iterations up to {res.iterations.max()}; unflagged {int((~res.converged).sum())}")
    assert res.converged.all(), np.flatnonzero(~res.converged)
    assert (err <= 1e-8).all(), err.max()


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_first_iterations_follow_the_host(ctx, cases, shape):
    model, _, P, T0 = cases[shape]
    K = len(P)
    other, perm = mt.permuted(model)
    for max_iter in (0, 1, 2):
        res, _ = run(ctx, model, P, T0, max_iter=max_iter)
        host = mt.host_sense(model, P, T0, max_iter=max_iter)
        if max_iter == 0:
            clipped = np.clip(T0, model["lo"], model["hi"])
            assert np.array_equal(res.start, host.start) and np.array_equal(res.iterations, host.iterations)
            assert np.array_equal(_bits(res.t), _bits(clipped[np.arange(K), res.start]))
            continue
        again = mt.host_sense(other, P[:, perm], T0, max_iter=max_iter)
        delta = np.abs(again.t - host.t).max(axis=1)
        bound = np.maximum(1e3 * delta, 1e-11 * (1.0 + np.abs(host.t).max(axis=1)))
        diff = np.abs(res.t - host.t).max(axis=1)
        print(f"max_iter {max_iter}: device - host up to {diff.max():.3g}, host - permuted host up to {delta.max():.3g}, largest ratio "
              f"to the bound {(diff / bound).max():.3g}")
        assert np.array_equal(res.iterations, host.iterations)
        assert (diff <= bound).all(), (diff / bound).max()


def test_pinned_coordinate(ctx, cases):
    model, t_true, _, _ = cases[REF]
    model = dict(model, lo=model["lo"].copy(), hi=model["hi"].copy())
    model["lo"][1] = model["hi"][1] = 0.25
    pinned = t_true.copy()
    pinned[:, 1] = 0.25
    P = mt.exact_queries(model, pinned)
    T0 = pinned[:, None, :] + 0.1 * np.random.default_rng(8).standard_normal((5, 3, 4))   # (the starts of t_1 lie elsewhere)
    assert (T0[:, :, 1] != 0.25).all()
    for max_iter in (0, 30):
        res, _ = run(ctx, model, P, T0, max_iter=max_iter)   # (check_state: sigma_min of the three free columns)
        assert np.array_equal(_bits(res.t[:, 1]), _bits(np.full(5, 0.25)))
    host = mt.host_sense(model, P, T0)
    print(f"max |t - t*| {np.abs(res.t - pinned).max():.3g}; sigma_min device {res.sigma_min}, host {host.sigma_min}")
    assert res.converged.all() and np.abs(res.t - pinned).max() <= 1e-8
    model["lo"][:], model["hi"][:] = 0.25, 0.25    # nothing free: one iteration that moves nothing
    res, _ = run(ctx, model, P, T0)
    assert np.array_equal(_bits(res.t), _bits(np.full((5, 4), 0.25))) and (res.sigma_min == 0.0).all()
    assert np.array_equal(res.iterations, mt.host_sense(model, P, T0).iterations)


def test_a_start_outside_the_box_is_clipped(ctx, cases):
    model, t_true, P, T0 = cases[REF]
    wild = T0 + np.array([-9.0, 9.0, 0.0, 0.0])
    res, _ = run(ctx, model, P, wild, max_iter=0)
    clipped = np.clip(wild, model["lo"], model["hi"])
    assert np.array_equal(_bits(res.t), _bits(clipped[np.arange(len(P)), res.start]))
    assert (res.t[:, 0] == model["lo"][0]).all() and (res.t[:, 1] == model["hi"][1]).all()
    res, _ = run(ctx, model, P, wild)
    print(f"from the clipped corner: max |t - t*| {np.abs(res.t - t_true).max():.3g}; converged {res.converged}")


@pytest.mark.parametrize("shape", [REF, (12, (64, 64, 64), "tanh", 40, 5, 3)], ids=["4x20-20", "12x64-64-64"])
def test_noisy_data_pass_the_checker(ctx, cases, shape):
    model, _, P, T0 = cases[shape]
    noisy = P + 1e-3 * np.random.default_rng(12).standard_normal(P.shape)
    aux = np.stack([np.full(len(P), 1e-6), np.abs(noisy).max(axis=1)], axis=1)
    res, _ = run(ctx, model, noisy, T0, aux=aux)
    host = mt.host_sense(model, noisy, T0, aux=aux)
    print(f"misfit device {res.misfit}, host {host.misfit}; iterations device {res.iterations}, host {host.iterations}")


def test_limits_raise_before_any_launch():
    from romhighcontrast_amd import nonlinear as nl
    for args, word in (((17, (20,), 4, 2), "m <= 16"), ((4, (5, 5, 5, 5), 4, 2), "layers <= 3"), ((4, (20, 65), 4, 2), "width <= 64"),
                       ((4, (20,), 97, 2), "r <= 96"), ((4, (20,), 6, 9), "t <= 8")):
        with pytest.raises(ValueError, match=word):
            nl._check_mlp_sense_limits(*args)


def test_errors(ctx):
    from romhighcontrast_amd._ffi import RomLibraryError
    model, _, P, _ = mt.case(4, (20, 20), "tanh", 12, 2, 1)
    up = ctx.upload
    big, wh = up(np.zeros(97 * 81)), up(np.zeros(3 * 64 * 64 + 3 * 64))
    T0, p = up(np.zeros(2 * 9 * 17)), up(np.zeros((2, 97)))
    lo, hi = -np.ones(17), np.ones(17)
    for (m, hidden, act, r, t, ldo), word in (((17, (20,), "tanh", 6, 1, 40), "m = 17"), ((4, (), "tanh", 6, 1, 40), "0 hidden layers"),
                                              ((4, (5, 5, 5, 5), "tanh", 6, 1, 40), "4 hidden layers"),
                                              ((4, (20, 65), "tanh", 6, 1, 40), "width = 65"), ((4, (0,), "tanh", 6, 1, 40), "width = 0"),
                                              ((4, (20,), "tanh", 97, 1, 40), "r = 97"), ((4, (20,), "tanh", 6, 9, 40), "t = 9"),
                                              ((4, (20,), "tanh", 6, 1, 8), "ldo")):
        OUT = up(np.full(400, np.nan))
        with pytest.raises(RomLibraryError, match=word) as e:
            ctx.mlp_sense(m, hidden, act, wh, r, big, p, 0, 97, 2, t, T0, lo[:m], hi[:m], OUT=OUT, ldo=ldo)
        assert "error 1" in str(e.value)   # ROM_ERR_INVALID
        assert np.isnan(OUT.download()).all(), "OUT was written"
    with pytest.raises(ValueError, match="activation"):
        ctx.mlp_sense(4, (20,), "gelu", wh, 6, big, p, 0, 97, 2, 1, T0, lo[:4], hi[:4])
    args = lambda: (4, model["hidden"], "tanh", up(model["WH"]), 12, up(model["Gr"]))  # noqa: E731
    # K = 0 is a no-op
    res, info = ctx.mlp_sense(*args(), None, 0, 12, 0, 1, None, model["lo"], model["hi"])
    assert res.t.shape == (0, 4) and info["launches"] == 0 and info["host_syncs"] == 0
    # NaN in each of WH, Gr, P, T0: an error, and the next call works
    start = np.zeros((2, 1, 4))
    for name in ("WH", "Gr", "P", "T0"):
        ops = dict(WH=model["WH"].copy(), Gr=model["Gr"].copy(), P=P.copy(), T0=start.copy())
        ops[name].reshape(-1)[ops[name].size // 2] = np.nan if name in ("WH", "P") else np.inf
        with pytest.raises(RomLibraryError, match="NaN / Inf") as e:
            ctx.mlp_sense(4, model["hidden"], "tanh", up(ops["WH"]), 12, up(ops["Gr"]), up(ops["P"]), 0, 12, 2, 1, up(ops["T0"]),
                          model["lo"], model["hi"])
        assert "error 1" in str(e.value), name
        res, _ = ctx.mlp_sense(*args(), up(P), 0, 12, 2, 1, up(start), model["lo"], model["hi"])
        assert np.isfinite(res.t).all(), name   # (the failure was reported once)


def _permuted_sensing(sense):
    """The same MLPSensing with the hidden units of every layer permuted (host side only)."""
    import copy
    from romhighcontrast_amd.nonlinear import _mlp_split
    other = copy.copy(sense)
    rng = np.random.default_rng(9)
    prev, layers = np.arange(sense.m), []
    for W, b in sense.layers:
        perm = rng.permutation(len(W))
        layers.append((W[perm][:, prev].copy(), b[perm].copy()))
        prev = perm
    other.WH = np.concatenate([W.ravel() for W, _ in layers] + [b for _, b in layers])
    other.layers = _mlp_split(other.WH, other.sizes)
    other.W_out = sense.W_out[:, prev].copy()
    from romhighcontrast_amd.inverse import reduce_sensors
    other.S = other._sensing_matrix()
    other.U, other.Gr_host, _ = reduce_sensors(other.S.T, other.weights)
    return other


@pytest.fixture(scope="module")
def experiment(ctx):
    """(2, 2) blocks, N = 5: 2,000 parameters a ~ U(1, 100), the first 64 held out; PCA, the (20, 20) tanh network from 4 to 8
    score columns, 8 sensors at interior vertices; the estimate from the exact measurements of the held-out states, on the device
    and on the host, and on the host with the hidden units permuted."""
    from romhighcontrast_amd.lib.ReducedBasis import pca_tall
    from romhighcontrast_amd.lib.SolutionsManagers import SolutionsManagerFEM
    from romhighcontrast_amd.nonlinear import MLPMap, MLPSensing
    n_test, m, q = 64, 4, 8
    sm = SolutionsManagerFEM(blocks_geometry=(2, 2), N=5)
    a = np.random.default_rng(42).uniform(1.0, 100.0, size=(2000, 2, 2))
    U = np.asarray(sm.generate_solutions(a))
    pca = pca_tall(ctx, U[n_test:], n=m + q, center=True, scores=True, download=True)
    Z = pca.scores
    mlp = MLPMap((20, 20), ctx=ctx).fit(Z[:, :m], Z[:, m:m + q])
    X, Yg = np.meshgrid(sm.points_c[1:-1], sm.points_r[1:-1])   # the interior vertices
    verts = np.c_[X.ravel(), Yg.ravel()]
    points = verts[np.random.default_rng(3).choice(len(verts), 8, replace=False)]
    Y = np.asarray(sm.evaluate_solutions(points, U[:n_test]))
    sense = MLPSensing(sm, pca, mlp).observe(points)
    dev = sense.estimate(Y, states=True, device=True)
    host = sense.estimate(Y, states=False, device=False)
    again = _permuted_sensing(sense).estimate(Y, states=False, device=False)
    return dict(sm=sm, U=U[:n_test], pca=pca, mlp=mlp, sense=sense, Y=Y, dev=dev, host=host, again=again, m=m, points=points)


def test_end_to_end_device_scores_equal_the_host_paths(experiment):
    """The device's known_scores equal the host path's within max(1e3 delta_host, 1e-9) max|z|, delta_host the host path's own
    change (relative to max|z|) when the hidden units of every layer are permuted; both paths pass check_state and
    predicted_scores = y_mean + y_scale net(t).

    Measured on an MI355X: device - host 1.22e-10 of max|z|, delta_host 6.63e-10, so the bound is 6.63e-7.  The two starts reach the
    same minimum and the last bits decide which is reported: another start on 29 of 64 queries, another iteration count on 27."""
    from romhighcontrast_amd.inverse import reduce_measurements
    from romhighcontrast_amd.nonlinear import SenseResult
    e = experiment
    sense, dev, host, again, m = e["sense"], e["dev"], e["host"], e["again"], e["m"]
    model = dict(m=m, hidden=sense.hidden, sizes=sense.sizes, activation=sense.activation, r=sense.r, WH=sense.WH, Gr=sense.Gr_host,
                 lo=sense.lo, hi=sense.hi)
    Pq, aux = reduce_measurements(sense.U, e["Y"], sense.weights)
    T0 = np.stack([sense._scaled(dev.linear_scores), np.zeros((len(e["U"]), m))], axis=1)
    for est in (dev, host):   # (t from the scores: (c + h t - c) / h is t to a rounding, so a t on the box's face is put back on it)
        t = np.clip(sense._scaled(est.known_scores), sense.lo, sense.hi)
        mt.check_state(model, Pq, aux, SenseResult(t, est.misfit, est.converged, est.iterations, est.sigma_min, est.start), T0=T0)
        assert np.abs(est.predicted_scores - sense.predict_scores(t)).max() <= 1e-12 * np.abs(est.predicted_scores).max()
    scale = np.abs(host.known_scores).max()
    delta = np.abs(again.known_scores - host.known_scores).max() / scale
    diff = np.abs(dev.known_scores - host.known_scores).max() / scale
    bound = max(1e3 * delta, 1e-9)
    print(f"known scores device - host {diff:.3g} of max|z|, host - permuted host {delta:.3g}, bound {bound:.3g}; starts differ on "
          f"{int((dev.start != host.start).sum())} queries, iteration counts on {int((dev.iterations != host.iterations).sum())}")
    assert diff <= bound, (diff, bound)


def test_end_to_end_states_are_the_reconstruction_at_the_scores(experiment):
    """states=True is nonlinear_reconstruction at the returned scores; the three rms H^1_0 errors (manifold estimate, linear least
    squares on 4 and on 8 modes) are printed, their order depends on the trained network and is not asserted.

    Measured on an MI355X: manifold estimate 0.003493, linear on 4 modes 0.00628, linear on 8 modes 0.01536; no query is flagged
    converged (held-out states are off the manifold, the misfit stays above misfit_tol)."""
    from romhighcontrast_amd.nonlinear import nonlinear_reconstruction
    e = experiment
    sm, pca, dev, m, U = e["sm"], e["pca"], e["dev"], e["m"], e["U"]
    direct = nonlinear_reconstruction(pca, e["mlp"], dev.known_scores)
    states = dev.states.numpy()
    assert np.array_equal(_bits(states), _bits(direct))
    with pytest.raises(ValueError, match="t <= 8"):   # (a limit exceeded: ValueError before any launch)
        e["sense"].estimate(e["Y"], starts=np.zeros((len(U), 9, m)))
    mean, V = np.asarray(pca.mean_).ravel(), np.asarray(pca.components_)
    E = np.asarray(sm.evaluate_solutions(e["points"], np.vstack([mean[None, :], V[:8]])))
    z8 = np.linalg.lstsq(E[1:].T, (e["Y"] - E[0][None, :]).T, rcond=None)[0].T
    rms = lambda W: float(np.sqrt(np.mean(np.asarray(sm.H10norm(np.ascontiguousarray(W - U))) ** 2)))  # noqa: E731
    print(f"rms H10 error: manifold estimate {rms(states):.4g}, linear on 4 modes {rms(mean + dev.linear_scores @ V[:m]):.4g}, linear on 8 "
          f"modes {rms(mean + z8 @ V[:8]):.4g}; iterations up to {dev.iterations.max()}; converged {int(dev.converged.sum())} of {len(U)}")
