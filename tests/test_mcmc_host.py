"""The posterior sampler on the host: Philox4x32-10 and the draws (inverse.philox4x32, mcmc_uniform, mcmc_draws) against known
answers and against csrc/rom_philox.h (a stand-alone program under AddressSanitizer and UBSan), and inverse.mcmc_host -- the
specification of rom_mcmc -- against posterior moments by quadrature, for calibration of its credible intervals, for its
structure (splits, chain ids, pinned coordinates, the box), and in float64 against itself in long double.

Measured (float64 specification against long double, 48 steps, burn 16, the six shapes of tests/test_gpu_mcmc.py): no chain cut,
smallest decision margin 6.4e-5, largest observed / bound 0.0011."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import lm_truth as lt
import mcmc_truth as mt
from romhighcontrast_amd import inverse as iv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KNOWN = [((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
         ((0xffffffff,) * 4, (0xffffffff,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
         ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), "d16cfe09 94fdcceb 5001e420 24126ea1")]
SHAPES = [(1, 1, 1, 3, 3), (6, 2, 4, 5, 3), (33, 9, 20, 5, 3), (64, 16, 64, 6, 3), (6, 2, 4, 257, 1), (6, 2, 4, 1, 8)]
IDS = ["x".join(map(str, s)) for s in SHAPES]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


# ---- Philox ---------------------------------------------------------------------------------------------------------------------
def test_philox_known_answers():
    for counter, key, want in KNOWN:
        assert " ".join(f"{w:08x}" for w in iv.philox4x32(counter, key)) == want


def test_uniform_is_never_0_or_1():
    u0, u1 = float(iv.mcmc_uniform(0, 0)), float(iv.mcmc_uniform(0xffffffff, 0xffffffff))
    assert 0.0 < u0 < u1 < 1.0 and u0 == 2.0 ** -53 and u1 == 1.0 - 2.0 ** -53


def test_header_agrees_with_numpy_bit_for_bit(tmp_path):
    gxx = shutil.which("g++")
    assert gxx, "g++ is part of the image"
    exe = str(tmp_path / "philox_host_check")
    csrc = os.path.join(ROOT, "romhighcontrast_amd", "csrc")
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-I", csrc, os.path.join(ROOT, "tests", "c_abi", "philox_host_check.cpp"), "-o", exe]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0, r.stdout.decode()
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert r.returncode == 0 and not r.stderr, (r.returncode, r.stderr.decode())
    lines = r.stdout.decode().splitlines()
    rows = [[int(x, 16) for x in ln.split()] for ln in lines if not ln.startswith("extremes")]
    assert len(rows) == 64
    for (counter, key, want), row in zip(KNOWN, rows):
        assert tuple(row[:4]) == tuple(counter) and " ".join(f"{w:08x}" for w in row[6:10]) == want
    rows = np.array(rows, dtype=np.uint64)
    w = iv.philox4x32(rows[:, :4], rows[:, 4:6])
    assert np.array_equal(w.astype(np.uint64), rows[:, 6:10])
    assert np.array_equal(_bits(iv.mcmc_uniform(w[:, 0], w[:, 1])), rows[:, 10])
    assert np.array_equal(_bits(iv.mcmc_uniform(w[:, 2], w[:, 3])), rows[:, 11])


def test_draws():
    xi, u = iv.mcmc_draws(5, np.arange(4000), 3, 5)
    assert xi.shape == (4000, 5) and u.shape == (4000,) and (0 < u).all() and (u < 1).all()
    assert abs(xi.mean()) < 5 / np.sqrt(20000) and abs(xi.std() - 1) < 0.02 and abs(u.mean() - 0.5) < 5 / np.sqrt(12 * 4000)
    # a chain's stream depends on its id, the step and the seed alone
    xi2, u2 = iv.mcmc_draws(5, np.arange(100, 110), 3, 5)
    assert np.array_equal(_bits(xi2), _bits(xi[100:110])) and np.array_equal(_bits(u2), _bits(u[100:110]))
    xi3, _ = iv.mcmc_draws(5, np.arange(4000), 3, 4)
    assert np.array_equal(_bits(xi3), _bits(xi[:, :4]))
    assert not np.array_equal(iv.mcmc_draws(6, np.arange(10), 3, 5)[0], xi[:10])
    assert not np.array_equal(iv.mcmc_draws(5, np.arange(10), 4, 5)[0], xi[:10])
    big = iv.mcmc_draws(2 ** 40 + 3, np.array([2 ** 33 + 1]), 2 ** 31 - 1, 3)
    assert np.isfinite(big[0]).all()


# ---- posterior truth --------------------------------------------------------------------------------------------------------------
def truth_case(n, k, r):
    """(model, theta*, p, invvar): one query p = G_r c(theta*) + 0.02 N(0, 1) from default_rng(3), sigma = 0.02."""
    model = lt.synth(n, k, r, 7)
    rng = np.random.default_rng(3)
    theta_true, _ = lt.exact_queries(model, 1, 7)
    p = mt.noisy_query(model, theta_true, 0.02, rng)
    return model, theta_true, p, 1.0 / 0.02 ** 2


@pytest.mark.parametrize("shape", [(3, 1, 2), (6, 2, 4)], ids=["A", "B"])
def test_posterior_moments_against_quadrature(shape):
    model, theta_true, p, invvar = truth_case(*shape)
    n, k = model["n"], model["k"]
    truth = mt.quadrature_moments(model, p[0], invvar)
    chains = 256
    run = iv.mcmc_host(model["Ahat"], model["bhat"], model["Gr"], p, [invvar], np.repeat(theta_true[:, None, :], chains, axis=1),
                       0.3 * np.eye(k)[None], model["lo"], model["hi"], 12345, 600, 200, 1, slots=0)
    mt.check_rows(model, p, chains, run.state, 600, 200)
    o = iv.mcmc_layout(n, k)
    worst, ok = mt.moments_within(run.state, n, k, truth)
    print(f"largest |average - truth| / standard error {worst:.3g}; acceptance {(run.state[:, o['accepted']] / run.state[:, o['kept']]).mean():.3g}; "
          f"truth mean {truth[0]}")
    assert ok, worst


# ---- calibration --------------------------------------------------------------------------------------------------------------------
def calibration_case():
    model = lt.synth(8, 4, 6, 7)
    rng = np.random.default_rng(5)
    theta_true = rng.uniform(model["lo"], model["hi"], size=(128, 4))
    P = mt.noisy_query(model, theta_true, 0.02, rng)
    return model, theta_true, P


def coverage(samples, theta_true, t):
    """The number of (query, parameter) pairs whose pooled 5 % - 95 % sample quantiles contain theta*."""
    K, k = theta_true.shape
    pooled = np.asarray(samples, dtype=np.float64).reshape(K, -1, k)
    q = np.quantile(pooled, [0.05, 0.95], axis=1)
    return int(((q[0] <= theta_true) & (theta_true <= q[1])).sum())


def test_credible_intervals_are_calibrated():
    model, theta_true, P = calibration_case()
    run = iv.mcmc_host(model["Ahat"], model["bhat"], model["Gr"], P, np.full(128, 1.0 / 0.02 ** 2), np.repeat(theta_true[:, None, :], 2, axis=1),
                       np.broadcast_to(0.3 * np.eye(4), (128, 4, 4)), model["lo"], model["hi"], 99, 1500, 500, 5)
    assert run.samples.shape == (256, 200, 4) and not np.isnan(run.samples).any()
    mt.check_rows(model, P, 2, run.state, 1500, 500, 5, run.samples)
    share = coverage(run.samples, theta_true, 2) / 512
    print(f"coverage of theta* by the 90 % intervals: {share:.4f}")
    assert 0.82 <= share <= 0.97, share


# ---- structure ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small():
    model, P, invvar, theta0, L = mt.trajectory_case(6, 2, 4, 4, 2)
    return model, (model["Ahat"], model["bhat"], model["Gr"], P, invvar), theta0, L


def test_a_split_call_returns_the_same_bits(small):
    model, args, theta0, L = small
    box = (model["lo"], model["hi"])
    whole = iv.mcmc_host(*args, theta0, L, *box, 3, 64, 16, 2)
    first = iv.mcmc_host(*args, theta0, L, *box, 3, 32, 16, 2)
    second = iv.mcmc_host(*args, None, L, *box, 3, 32, 16, 2, step0=32, state=first.state)
    assert np.array_equal(_bits(second.state), _bits(whole.state))
    assert first.samples.shape[1] == 8 and second.samples.shape[1] == 24 and np.isnan(second.samples[:, :8]).all()
    merged = np.where(np.isnan(second.samples), np.pad(first.samples, ((0, 0), (0, 16), (0, 0)), constant_values=np.nan), second.samples)
    assert np.array_equal(_bits(merged), _bits(whole.samples))
    mt.check_rows(model, args[3], 2, whole.state, 64, 16, 2, whole.samples)


def test_chain_ids_do_not_depend_on_the_call(small):
    model, args, theta0, L = small
    box = (model["lo"], model["hi"])
    A, b, G, P, invvar = args
    th8 = np.repeat(theta0[:1, :1], 8, axis=1)
    whole = iv.mcmc_host(A, b, G, P[:1], invvar[:1], th8, L[:1], *box, 3, 40, 10, 1)
    lo4 = iv.mcmc_host(A, b, G, P[:1], invvar[:1], th8[:, :4], L[:1], *box, 3, 40, 10, 1)
    hi4 = iv.mcmc_host(A, b, G, P[:1], invvar[:1], th8[:, 4:], L[:1], *box, 3, 40, 10, 1, chain0=4)
    assert np.array_equal(_bits(whole.state), _bits(np.concatenate([lo4.state, hi4.state])))
    assert np.array_equal(_bits(whole.samples), _bits(np.concatenate([lo4.samples, hi4.samples])))
    assert len({r.tobytes() for r in whole.state}) == 8


def test_a_pinned_coordinate_never_moves_and_samples_stay_in_the_box(small):
    model, args, theta0, L = small
    lo, hi = model["lo"].copy(), model["hi"].copy()
    lo[1] = hi[1] = 1.2345678901234567
    full = np.broadcast_to(np.array([[0.3, 0.0], [0.2, 0.3]]), L.shape)
    run = iv.mcmc_host(*args, theta0, full, lo, hi, 3, 80, 20, 1)
    assert np.array_equal(_bits(run.samples[:, :, 1]), _bits(np.full(run.samples.shape[:2], lo[1])))
    assert ((run.samples >= lo) & (run.samples <= hi)).all()
    assert len(np.unique(run.samples[0, :, 0])) > 3
    o = iv.mcmc_layout(6, 2)
    assert (run.state[:, o["M2"] + 3] == 0).all() and (run.state[:, o["mean"] + 1] == lo[1]).all()
    wide = iv.mcmc_host(*args, theta0, 3.0 * L, model["lo"], model["hi"], 3, 80, 0, 1)
    assert ((wide.samples >= model["lo"]) & (wide.samples <= model["hi"])).all() and wide.state[:, o["outside"]].sum() > 0


def test_burn_beyond_the_steps_keeps_nothing(small):
    model, args, theta0, L = small
    run = iv.mcmc_host(*args, theta0, L, model["lo"], model["hi"], 3, 20, 20, 1)
    o = iv.mcmc_layout(6, 2)
    assert run.samples is None and (run.state[:, o["kept"]] == 0).all() and (run.state[:, o["accepted"]] == 0).all()
    assert (run.state[:, o["ls"]] != 0).all()
    mt.check_rows(model, args[3], 2, run.state, 20, 20)
    zero = iv.mcmc_host(*args, theta0, L, model["lo"], model["hi"], 3, 0, 5, 1)
    assert np.array_equal(_bits(zero.state[:, :2]), _bits(np.clip(theta0, model["lo"], model["hi"]).reshape(-1, 2)))
    assert (zero.state[:, o["ls"]] == 0).all() and (zero.state[:, o["kept"]:o["kept"] + 4] == 0).all()
    assert np.array_equal(_bits(zero.state[:, o["phi"]]), _bits(zero.state[:, o["phi_min"]]))


def test_failures_of_the_start(small):
    model, args, theta0, L = small
    A, b, G, P, invvar = args
    broken = A.copy()
    broken[0] = -broken[0]
    with pytest.raises(np.linalg.LinAlgError, match="not positive definite"):
        iv.mcmc_host(broken, b, G, P, invvar, theta0, L, model["lo"], model["hi"], 3, 4, 1, 1)
    Pn = P.copy()
    Pn[1, 0] = np.nan
    run = iv.mcmc_host(A, b, G, Pn, invvar, theta0, L, model["lo"], model["hi"], 3, 4, 1, 1)
    assert np.isnan(run.state[2:4]).all() and np.isfinite(run.state[:2]).all() and np.isfinite(run.state[4:]).all()


def test_proposal_factors(small):
    model, args, theta0, L = small
    A, b, G, P, invvar = args
    lo, hi = model["lo"].copy(), model["hi"].copy()
    F = iv.proposal_factors(A, b, G, theta0[:, 0], invvar, lo, hi)
    assert F.shape == (4, 2, 2) and (F[:, 0, 1] == 0).all() and (F[:, [0, 1], [0, 1]] > 0).all()
    J = np.stack([lt.jacobian(model, th)[0] for th in theta0[:, 0]])
    H = invvar[:, None, None] * np.einsum("bmq,bmp->bqp", J, J) + np.diag(12.0 / (hi - lo) ** 2)
    assert np.allclose(np.einsum("bqp,bsp->bqs", F, F) @ H, np.eye(2) * 2.38 ** 2 / 2, atol=1e-8)
    lo[0] = hi[0] = 1.0
    F = iv.proposal_factors(A, b, G, theta0[:, 0], invvar, lo, hi)
    assert (F[:, 0, :] == 0).all() and (F[:, :, 0] == 0).all() and (F[:, 1, 1] > 0).all()


def test_limits():
    assert iv.MCMC_LIMITS == dict(n=64, k=16, r=64, t=8)
    iv._check_mcmc_limits(64, 16, 64, 8)
    for bad, word in (((65, 1, 1, 1), "n = 65"), ((1, 17, 1, 1), "k = 17"), ((1, 1, 65, 1), "r = 65"), ((1, 1, 1, 9), "t = 9"),
                      ((0, 1, 1, 1), "n = 0")):
        with pytest.raises(ValueError, match=word):
            iv._check_mcmc_limits(*bad)
    model, P, invvar, theta0, L = mt.trajectory_case(1, 1, 1, 1, 1)
    for kw in (dict(steps=-1), dict(burn=-1), dict(thin=0)):
        a = dict(steps=4, burn=1, thin=1)
        a.update(kw)
        with pytest.raises(ValueError):
            iv.mcmc_host(model["Ahat"], model["bhat"], model["Gr"], P, invvar, theta0, L, model["lo"], model["hi"], 3, a["steps"], a["burn"], a["thin"])


# ---- float64 against long double ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_float64_follows_long_double(shape):
    """The float64 specification held to the trajectory bound of tests/mcmc_truth.py against itself in long double."""
    n, k, r, K, t = shape
    model, P, invvar, theta0, L = mt.trajectory_case(*shape)
    args = (model["Ahat"], model["bhat"], model["Gr"], P, invvar, theta0, L, model["lo"], model["hi"], 2024, 48, 16, 1)
    ref = iv.mcmc_host(*args, dtype=np.longdouble)
    run = iv.mcmc_host(*args)
    cut = np.minimum(mt.first_close_steps(model, P, invvar, theta0, L, 2024, 48, 16, run=ref, dtype=np.longdouble),
                     mt.first_close_steps(model, P, invvar, theta0, L, 2024, 48, 16, run=run))
    bound = mt.trajectory_bound(48, k, n, np.abs(run.state[:, :k]).max(), model["lo"], model["hi"])
    worst, ncut = mt.compare_runs(ref, run.state, run.samples, cut, 48, 16, n, k, bound)
    print(f"float64 against long double: largest observed / bound {worst:.3g}; chains cut {ncut} of {K * t}; smallest margin "
          f"{min(run.margin.min(), ref.margin.min()):.3g}")
    assert ncut * 16 <= K * t
    mt.check_rows(model, P, t, run.state, 48, 16, 1, run.samples)
