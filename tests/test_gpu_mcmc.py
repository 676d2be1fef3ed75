"""rom_mcmc on the GPU against its specification inverse.mcmc_host and the truth of tests/mcmc_truth.py.

Every call runs on NaN-framed operands -- P, STATE and SAMPLES as column ranges of wider NaN blocks from an offset, the others
with a NaN tail -- which must come back bit for bit (STATE and SAMPLES: everything outside their rows); a fresh call finds NaN in
its rows behind the starts; every call is made twice and must return the same bits; every finite state row goes through
mcmc_truth.check_rows.  Shapes (n, k, r, K, t): the smallest; r < n; odd sizes; the limits (64, 16, 64); one chain past 256 with
t = 1; one query with t = 8.

The device follows the specification: 48 steps, burn 16, thin 1; per chain up to the first step whose decision margin on the host
is below 1e-9 the samples, and for a chain without such a step the counters (equal) and theta, mean, ls, Phi_min, lie within
mcmc_truth.trajectory_bound, the bound the float64 specification is held to against long double in tests/test_mcmc_host.py."""
import numpy as np
import pytest

import lm_truth as lt
import mcmc_truth as mt
from test_gpu_lm_polish import Tail, _bits
from test_mcmc_host import SHAPES, IDS, calibration_case, coverage, truth_case

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from romhighcontrast_amd import _ffi
    return _ffi.get_context()


def run(ctx, model, P, invvar, theta0, L, seed, steps, burn, thin, chain0=0, step0=0, state=None, slots=None, samples=True, box=None,
        check=True):
    """rom_mcmc twice on NaN-framed operands; returns (state rows (B, row), samples (B, slots, k) or None, info)."""
    from romhighcontrast_amd.inverse import mcmc_layout
    n, k, r = model["n"], model["k"], model["r"]
    lo, hi = box if box is not None else (model["lo"], model["hi"])
    P = np.atleast_2d(P)
    K = len(P)
    o = ctx.mcmc_layout(n, k)
    assert o == mcmc_layout(n, k)
    row = o["row"]
    if state is None:
        theta0 = np.asarray(theta0, dtype=np.float64).reshape(K, -1, k)
        t = theta0.shape[1]
        rows = np.full((K * t, row), np.nan)
        rows[:, :k] = theta0.reshape(K * t, k)
    else:
        rows = np.asarray(state, dtype=np.float64).reshape(-1, row)
        t = len(rows) // K
    B = K * t
    total = max(0, step0 + steps - burn) // thin
    slots = total if slots is None else slots
    ldp, p_off, lds, s_off, smp_off = r + 3, r + 3 + 1, row + 2, 3, 5
    ph = np.full((K + 2, ldp), np.nan)
    ph[1:1 + K, 1:1 + r] = P
    ops = [Tail(ctx, model["Ahat"]), Tail(ctx, model["bhat"]), Tail(ctx, model["Gr"]), Tail(ctx, ph), Tail(ctx, invvar), Tail(ctx, L)]
    sh = np.full(s_off + B * lds + 4, np.nan)
    sh[s_off:s_off + B * lds].reshape(B, lds)[:, :row] = rows
    outs = []
    for _ in range(2):
        STATE = ctx.upload(sh)
        SAMPLES = ctx.upload(np.full(smp_off + B * slots * k + 4, np.nan)) if samples else None
        info = ctx.mcmc(n, k, r, ops[0].buf, ops[1].buf, ops[2].buf, ops[3].buf, p_off, ldp, K, t, ops[4].buf, ops[5].buf, lo, hi, seed,
                        steps, burn, thin, STATE, s_off=s_off, lds=lds, SAMPLES=SAMPLES, smp_off=smp_off, slots=slots, chain0=chain0,
                        step0=step0)
        raw = STATE.download()
        body = raw[s_off:s_off + B * lds].reshape(B, lds)
        assert np.isnan(raw[:s_off]).all() and np.isnan(raw[s_off + B * lds:]).all() and np.isnan(body[:, row:]).all(), "STATE's frame"
        sraw = SAMPLES.download() if samples else np.zeros(0)
        if samples:
            assert np.isnan(sraw[:smp_off]).all() and np.isnan(sraw[smp_off + B * slots * k:]).all(), "SAMPLES' frame"
        outs.append((raw, sraw, info))
    for op in ops:
        assert op.unchanged(), "an input buffer was modified"
    assert np.array_equal(_bits(outs[0][0]), _bits(outs[1][0])) and np.array_equal(_bits(outs[0][1]), _bits(outs[1][1])), "two calls, different bits"
    raw, sraw, info = outs[0]
    st = raw[s_off:s_off + B * lds].reshape(B, lds)[:, :row].copy()
    smp = sraw[smp_off:smp_off + B * slots * k].reshape(B, slots, k).copy() if samples else None
    assert info["launches"] == max(1, -(-steps // 1024)) and info["host_syncs"] == 1 and info["chains"] == B, info
    if check:
        assert info["steps"] == B * steps and B <= info["evaluations"] <= B * (steps + info["launches"]), info
        mt.check_rows(model, P, t, st, step0 + steps, burn, thin, smp)
    return st, smp, info


# ---- the device follows the specification -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_device_follows_the_specification(ctx, shape):
    from romhighcontrast_amd.inverse import mcmc_host
    n, k, r, K, t = shape
    model, P, invvar, theta0, L = mt.trajectory_case(*shape)
    ref = mcmc_host(model["Ahat"], model["bhat"], model["Gr"], P, invvar, theta0, L, model["lo"], model["hi"], 2024, 48, 16, 1)
    st, smp, info = run(ctx, model, P, invvar, theta0, L, 2024, 48, 16, 1)
    assert not np.isnan(smp).any()
    cut = mt.first_close_steps(model, P, invvar, theta0, L, 2024, 48, 16, run=ref)
    bound = mt.trajectory_bound(48, k, n, np.abs(ref.state[:, :k]).max(), model["lo"], model["hi"])
    worst, ncut = mt.compare_runs(ref, st, smp, cut, 48, 16, n, k, bound)
    print(f"device against the float64 specification: largest observed / bound {worst:.3g}; chains cut {ncut} of {K * t}; smallest host "
          f"margin {ref.margin.min():.3g}; {info}")
    assert ncut * 16 <= K * t


# ---- posterior truth and calibration ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(3, 1, 2), (6, 2, 4)], ids=["A", "B"])
def test_posterior_moments_against_quadrature(ctx, shape):
    from romhighcontrast_amd.inverse import mcmc_layout
    model, theta_true, p, invvar = truth_case(*shape)
    n, k = model["n"], model["k"]
    truth = mt.quadrature_moments(model, p[0], invvar)
    # 256 chains of one query: 32 identical queries of 8 chains, the ids 0 .. 255
    P, chains = np.repeat(p, 32, axis=0), 256
    st, _, _ = run(ctx, model, P, np.full(32, invvar), np.broadcast_to(theta_true, (32, 8, k)), np.broadcast_to(0.3 * np.eye(k), (32, k, k)),
                   12345, 600, 200, 1, slots=0)
    o = mcmc_layout(n, k)
    worst, ok = mt.moments_within(st, n, k, truth)
    print(f"largest |average - truth| / standard error {worst:.3g} over {chains} chains; acceptance {(st[:, o['accepted']] / st[:, o['kept']]).mean():.3g}")
    assert ok, worst


@pytest.fixture(scope="module")
def calibration_host():
    from romhighcontrast_amd.inverse import mcmc_host
    model, theta_true, P = calibration_case()
    args = (np.full(128, 1.0 / 0.02 ** 2), np.repeat(theta_true[:, None, :], 2, axis=1), np.broadcast_to(0.3 * np.eye(4), (128, 4, 4)).copy())
    run_ = mcmc_host(model["Ahat"], model["bhat"], model["Gr"], P, *args, model["lo"], model["hi"], 99, 1500, 500, 5)
    return model, theta_true, P, args, run_


def test_credible_intervals_are_calibrated(ctx, calibration_host):
    model, theta_true, P, args, host = calibration_host
    st, smp, _ = run(ctx, model, P, *args, 99, 1500, 500, 5)
    assert smp.shape == (256, 200, 4) and not np.isnan(smp).any()
    dev, hst = coverage(smp, theta_true, 2), coverage(host.samples, theta_true, 2)
    ncut = int((host.margin < mt.MARGIN).sum())
    print(f"coverage of theta* by the 90 % intervals: device {dev} of 512 = {dev / 512:.4f}, host {hst} of 512 = {hst / 512:.4f}; chains "
          f"cut {ncut}; smallest host margin {host.margin.min():.3g}")
    assert 0.82 <= dev / 512 <= 0.97, dev / 512
    assert abs(dev - hst) <= ncut, (dev, hst, ncut)


# ---- splits ---------------------------------------------------------------------------------------------------------------------------
def test_a_split_call_returns_the_same_bits(ctx):
    model, P, invvar, theta0, L = mt.trajectory_case(6, 2, 4, 5, 3)
    whole, wsmp, _ = run(ctx, model, P, invvar, theta0, L, 3, 64, 16, 2)
    first, fsmp, _ = run(ctx, model, P, invvar, theta0, L, 3, 32, 16, 2, slots=24)
    second, ssmp, _ = run(ctx, model, P, invvar, None, L, 3, 32, 16, 2, step0=32, state=first)
    assert np.array_equal(_bits(second), _bits(whole))
    assert not np.isnan(fsmp[:, :8]).any() and np.isnan(fsmp[:, 8:]).all() and np.isnan(ssmp[:, :8]).all()
    assert np.array_equal(_bits(np.where(np.isnan(ssmp), fsmp, ssmp)), _bits(wsmp))


def test_the_internal_launch_split(ctx):
    """1025 steps, one past the steps of a launch: two launches inside the call, the bits of 1024 + 1 steps in two calls."""
    model, P, invvar, theta0, L = mt.trajectory_case(1, 1, 1, 3, 3)
    whole, wsmp, info = run(ctx, model, P, invvar, theta0, L, 3, 1025, 100, 25)
    assert info["launches"] == 2
    first, fsmp, _ = run(ctx, model, P, invvar, theta0, L, 3, 1024, 100, 25, slots=37)
    second, ssmp, _ = run(ctx, model, P, invvar, None, L, 3, 1, 100, 25, step0=1024, state=first)
    assert np.array_equal(_bits(second), _bits(whole))
    assert np.array_equal(_bits(np.where(np.isnan(ssmp), fsmp, ssmp)), _bits(wsmp)) and not np.isnan(wsmp).any()


def test_chain_ids_do_not_depend_on_the_call(ctx):
    model, P, invvar, theta0, L = mt.trajectory_case(6, 2, 4, 1, 8)
    whole, wsmp, _ = run(ctx, model, P, invvar, theta0, L, 3, 40, 10, 1)
    lo4, lsmp, _ = run(ctx, model, P, invvar, theta0[:, :4], L, 3, 40, 10, 1)
    hi4, hsmp, _ = run(ctx, model, P, invvar, theta0[:, 4:], L, 3, 40, 10, 1, chain0=4)
    assert np.array_equal(_bits(whole), _bits(np.concatenate([lo4, hi4])))
    assert np.array_equal(_bits(wsmp), _bits(np.concatenate([lsmp, hsmp])))


# ---- edges ----------------------------------------------------------------------------------------------------------------------------
def test_no_steps_no_samples_few_slots(ctx):
    from romhighcontrast_amd.inverse import mcmc_layout
    model, P, invvar, theta0, L = mt.trajectory_case(6, 2, 4, 5, 3)
    o = mcmc_layout(6, 2)
    wild = theta0 + np.array([-9.0, 9.0])
    st, _, info = run(ctx, model, P, invvar, wild, L, 3, 0, 5, 1)
    assert np.array_equal(_bits(st[:, :2]), _bits(np.clip(wild, model["lo"], model["hi"]).reshape(-1, 2)))
    assert (st[:, o["ls"]] == 0).all() and (st[:, o["kept"]:o["kept"] + 4] == 0).all() and info["steps"] == 0 and info["evaluations"] == 15
    assert np.array_equal(_bits(st[:, o["phi"]]), _bits(st[:, o["phi_min"]])) and np.array_equal(_bits(st[:, :2]), _bits(st[:, o["theta_min"]:]))
    full, fsmp, _ = run(ctx, model, P, invvar, theta0, L, 3, 40, 10, 1)
    none, nsmp, _ = run(ctx, model, P, invvar, theta0, L, 3, 40, 10, 1, samples=False)
    assert nsmp is None and np.array_equal(_bits(none), _bits(full))
    few, wsmp, _ = run(ctx, model, P, invvar, theta0, L, 3, 40, 10, 1, slots=7)   # (run checks that nothing lies behind the last slot)
    assert np.array_equal(_bits(few), _bits(full)) and np.array_equal(_bits(wsmp), _bits(fsmp[:, :7]))
    burnt, _, _ = run(ctx, model, P, invvar, theta0, L, 3, 10, 10, 1)
    assert (burnt[:, o["kept"]] == 0).all() and (burnt[:, o["ls"]] != 0).all()


def test_a_pinned_coordinate_stays_bit_for_bit(ctx):
    model, P, invvar, theta0, L = mt.trajectory_case(6, 2, 4, 5, 3)
    lo, hi = model["lo"].copy(), model["hi"].copy()
    lo[1] = hi[1] = 1.2345678901234567
    pinned = dict(model, lo=lo, hi=hi)
    full = np.broadcast_to(np.array([[0.3, 0.0], [0.2, 0.3]]), L.shape).copy()
    st, smp, _ = run(ctx, pinned, P, invvar, theta0, full, 3, 80, 20, 1)
    assert np.array_equal(_bits(smp[:, :, 1]), _bits(np.full(smp.shape[:2], lo[1]))) and len(np.unique(smp[0, :, 0])) > 3
    assert ((smp >= lo) & (smp <= hi)).all()


def test_a_start_that_is_not_positive_definite_is_reported_once(ctx):
    from scipy.linalg import LinAlgError
    from romhighcontrast_amd._ffi import ROM_OK
    model, P, invvar, theta0, L = mt.trajectory_case(6, 2, 4, 2, 1)
    before, _, _ = run(ctx, model, P, invvar, theta0, L, 3, 20, 5, 1)
    broken = dict(model, Ahat=model["Ahat"].copy())
    broken["Ahat"][0] = -broken["Ahat"][0]
    with pytest.raises(LinAlgError, match="not positive definite"):
        run(ctx, broken, P, invvar, theta0, L, 3, 20, 5, 1, check=False)
    assert ctx.lib.rom_solve_status(ctx.h) == ROM_OK, "the failure of rom_mcmc is reported a second time"
    after, _, _ = run(ctx, model, P, invvar, theta0, L, 3, 20, 5, 1)
    assert np.array_equal(_bits(after), _bits(before))


def test_nan_in_a_query_gives_a_nan_row(ctx):
    model, P, invvar, theta0, L = mt.trajectory_case(6, 2, 4, 3, 2)
    Pn = P.copy()
    Pn[1, 2] = np.nan
    st, smp, _ = run(ctx, model, Pn, invvar, theta0, L, 3, 1030, 5, 1, check=False)
    assert np.isnan(st[2:4]).all() and np.isnan(smp[2:4]).all()
    sound, ssmp, _ = run(ctx, model, P, invvar, theta0, L, 3, 1030, 5, 1)
    keep = [0, 1, 4, 5]
    assert np.array_equal(_bits(st[keep]), _bits(sound[keep])) and np.array_equal(_bits(smp[keep]), _bits(ssmp[keep]))


def test_errors(ctx):
    from romhighcontrast_amd._ffi import RomLibraryError
    up = ctx.upload
    big = up(np.zeros(17 * 65 * 65))
    lo, hi = np.zeros(17), np.ones(17)
    good = dict(n=4, k=2, r=3, t=1, steps=4, burn=1, thin=1, lds=None)
    for change, word in ((dict(n=65), "n = 65"), (dict(k=17), "k = 17"), (dict(r=65), "r = 65"), (dict(t=9), "t = 9"), (dict(steps=-1), "steps = -1"),
                         (dict(burn=-1), "burn = -1"), (dict(thin=0), "thin = 0"), (dict(lds=5), "lds")):
        a = dict(good, **change)
        with pytest.raises(RomLibraryError, match=word) as e:
            ctx.mcmc(a["n"], a["k"], a["r"], big, big, big, big, 0, 65, 2, a["t"], big, big, lo[:a["k"]], hi[:a["k"]], 1, a["steps"], a["burn"],
                     a["thin"], big, lds=400 if a["lds"] is None else a["lds"])
        assert "error 1" in str(e.value)   # ROM_ERR_INVALID
    with pytest.raises(RomLibraryError, match="STATE holds"):
        ctx.mcmc(4, 2, 3, big, big, big, big, 0, 3, 2, 1, big, big, lo[:2], hi[:2], 1, 4, 1, 1, up(np.zeros(40)))
    with pytest.raises(RomLibraryError, match="SAMPLES holds"):
        ctx.mcmc(4, 2, 3, big, big, big, big, 0, 3, 2, 1, big, big, lo[:2], hi[:2], 1, 4, 1, 1, big, SAMPLES=up(np.zeros(8)), slots=3)
    info = ctx.mcmc(4, 2, 3, big, big, big, None, 0, 3, 0, 1, None, None, lo[:2], hi[:2], 1, 4, 1, 1, None)
    assert info["launches"] == 0 and info["host_syncs"] == 0


# ---- end to end -----------------------------------------------------------------------------------------------------------------------
def test_posterior_of_a_parameter_library(ctx):
    from romhighcontrast_amd.inverse import ParameterLibrary
    from src.lib.ReducedBasis import GREEDY_FOR_H10, ReducedBasisGreedy
    from src.lib.SolutionsManagers import SolutionsManagerFEM
    sm = SolutionsManagerFEM((2, 2), 5)
    rng = np.random.default_rng(0)
    a_train = 10.0 ** rng.uniform(0.0, 2.0, size=(32, 2, 2))
    U = sm.generate_solutions(a_train)
    rb = ReducedBasisGreedy(GREEDY_FOR_H10).build(8, sm, U, a_train, sm.H10norm(U))
    a_lib = 10.0 ** rng.uniform(0.0, 2.0, size=(256, 2, 2))
    points = rng.uniform(-0.95, 0.95, size=(12, 2))
    a_true = 10.0 ** rng.uniform(0.2, 1.8, size=(8, 2, 2))
    Y = sm.evaluate_solutions(points, sm.generate_solutions(a_true))
    sigma = 1e-2 * np.abs(Y).max()
    Y = Y + sigma * rng.standard_normal(Y.shape)
    lib = ParameterLibrary(sm, rb.basis, a_lib).observe(points)
    K, k, n, t = 8, 4, lib.n, 4
    post = lib.posterior(Y, sigma, t=t, steps=400, burn=100, thin=4, seed=1, states=True)
    for name, shape in (("mean", (K, k)), ("cov", (K, k, k)), ("sd", (K, k)), ("rhat", (K, k)), ("acceptance", (K, t)), ("scale", (K, t)),
                        ("a_map", (K, k)), ("misfit_min", (K,)), ("mean_coefficients", (K, n)), ("outside", (K, t)), ("not_spd", (K, t)),
                        ("samples", (K, t, 75, k))):
        v = getattr(post, name)
        assert v.shape == shape and np.isfinite(v).all(), (name, v.shape)
    assert (post.a_map >= lib.a.min(axis=0)).all() and (post.a_map <= lib.a.max(axis=0)).all()
    la = np.log(lib.a)
    assert ((post.samples >= la.min(axis=0)) & (post.samples <= la.max(axis=0))).all() and (post.not_spd == 0).all()
    q = post.quantiles([0.05, 0.95])
    assert q.shape == (2, K, k) and (q[0] <= q[1]).all()
    W = lib._W.download(n * sm.vspace_dim, shape=(n, sm.vspace_dim))
    S = post.states.numpy()
    assert S.shape == (K, sm.vspace_dim)
    assert np.abs(S - post.mean_coefficients @ W).max() <= 1e-12 * max(1.0, np.abs(S).max())
    host = lib.posterior(Y, sigma, t=t, steps=400, burn=100, thin=4, seed=1, device=False)
    cover = int(((q[0] <= np.log(a_true.reshape(K, k))) & (np.log(a_true.reshape(K, k)) <= q[1])).sum())
    print(f"median R-hat {np.nanmedian(post.rhat):.3g}; acceptance {post.acceptance.mean():.3g}; true log a inside the 90 % interval: {cover} of "
          f"{K * k}; |mean_dev - mean_host| up to {np.abs(post.mean - host.mean).max():.3g}")
    assert np.array_equal(post.outside, host.outside) and np.array_equal(post.not_spd, host.not_spd)
    assert np.array_equal(np.round(post.acceptance * 300), np.round(host.acceptance * 300))
    same = rb.parameter_posterior(sm, points, Y, a_lib, sigma, t=t, steps=400, burn=100, thin=4, seed=1)
    assert np.array_equal(_bits(same.mean), _bits(post.mean)) and np.array_equal(_bits(same.samples), _bits(post.samples))
