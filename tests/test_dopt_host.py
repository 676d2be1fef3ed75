"""The NumPy specification of the D-optimal sensor design (inverse.sensor_dopt_host) against the long-double truth of
tests/dopt_truth.py, the checker's teeth, the statuses, the stop rules, a pinned parameter, the submodular guarantee and the
host-only layout entry point.  No GPU.

The guarantee is tested against random sensor sets only: the tests' NumPy counterpart of select_sensors_pbdw (sensor_truth.py)
works on a finite-element space, which the synthetic reduced models here do not have; tests/test_gpu_sensor_dopt.py compares with
select_sensors_pbdw's points on a real space."""
import numpy as np
import pytest

import dopt_truth as dt
from conftest import observed

SHAPES = [(1, 1, 1, 1, 1), (5, 3, 7, 37, 5), (8, 4, 33, 130, 8), (64, 16, 3, 20, 6)]   # (n, k, M, ncand, m)
IDS = ["x".join(str(v) for v in s) for s in SHAPES]
SIGMAS = [1e-1, 1e-3, 1e-6]
SEED = 7


def empty_state(c, sigma, prior=None):
    """(Z0 (M, n, k), T0, status) of the specification for the case c."""
    from romhighcontrast_amd.inverse import sensor_prior_factor, sensor_sensitivities_host
    X, st = sensor_sensitivities_host(c["Ahat"], c["bhat"], c["theta"], status=True)
    T0 = sensor_prior_factor(dt.prior_variances(c["k"]) if prior is None else prior, c["k"])
    return X @ T0 / sigma, T0, st


def spec(c, m, sigma, prior=None, **kw):
    from romhighcontrast_amd.inverse import sensor_dopt_host
    return sensor_dopt_host(c["Ahat"], c["bhat"], c["theta"], c["E"], m, sigma, dt.prior_variances(c["k"]) if prior is None else prior, **kw)


@pytest.mark.parametrize("sigma", SIGMAS)
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_specification_passes_the_checker(shape, sigma):
    n, k, M, ncand, m = shape
    c = dt.case(n, k, M, ncand, SEED)
    des = spec(c, m, sigma)
    assert des.stop_reason == "m" and len(des.picks) == m and not des.skipped.any() and des.posterior_sd.shape == (M, k)
    Z0, T0, st = empty_state(c, sigma)
    from romhighcontrast_amd.inverse import sensor_sensitivities_host
    observed(f"dopt host sensitivities {shape}", dt.check_sensitivities(c, sensor_sensitivities_host(c["Ahat"], c["bhat"], c["theta"]), st), 1.0)
    worst, truth = dt.check_design(Z0, T0, c["E"], des)
    observed(f"dopt host design / bound {shape} sigma {sigma:g}", worst, 1.0)
    # the information is the criterion of the picked set, computed from scratch
    phi = dt.criterion(Z0, c["E"], des.picks)
    assert abs(float(phi - des.information[-1])) <= truth.information(M)[1][-1]


# ---- the checker has teeth ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sigma", SIGMAS)
def test_checker_rejects_a_moved_score(sigma):
    from romhighcontrast_amd.inverse import sensor_dopt_scores_host
    c = dt.case(8, 4, 33, 130, SEED)
    Z0, T0, _ = empty_state(c, sigma)
    truth = dt.Truth(Z0, T0, c["E"], [])
    scores = sensor_dopt_scores_host(Z0, c["E"])
    assert dt.check_scores(truth, 0, scores) <= 1.0
    scores[17] += 10.0 * truth.score_bound[0][17]
    with pytest.raises(AssertionError, match="off by more than the bound"):
        dt.check_scores(truth, 0, scores)


@pytest.mark.parametrize("sigma", SIGMAS)
@pytest.mark.parametrize("shape", SHAPES[1:], ids=IDS[1:])
def test_checker_rejects_the_second_best_pick(shape, sigma):
    """At every step the truth's gap between the best and the second-best candidate exceeds 4 x the bound (asserted: the seeds are
    chosen so), and a sequence that takes the second best at a step is rejected at that step."""
    from romhighcontrast_amd.inverse import SensorDesign
    n, k, M, ncand, m = shape
    c = dt.case(n, k, M, ncand, SEED)
    des = spec(c, m, sigma)
    Z0, T0, _ = empty_state(c, sigma)
    truth = dt.Truth(Z0, T0, c["E"], des.picks)
    for t, (gap, bound) in enumerate(dt.pick_gaps(truth)):
        assert gap > 4.0 * bound, (t, gap, bound)
    for t in (0, m // 2, m - 1):
        sc = np.where(np.isnan(truth.scores[t]), -np.inf, truth.scores[t]).astype(np.float64)
        sc[des.picks[:t]] = -np.inf
        second = int(np.argsort(-sc, kind="stable")[1])
        picks = np.concatenate([des.picks[:t], [second]])
        tr = dt.Truth(Z0, T0, c["E"], picks)
        gain = np.array([float(tr.scores[i][x]) for i, x in enumerate(picks)])
        fake = SensorDesign(picks, gain, np.cumsum(gain) / (2.0 * M), tr.sd[len(picks)].astype(np.float64), "m", np.zeros(M, dtype=np.int64))
        with pytest.raises(AssertionError, match=f"step {t}: pick {second} has a true score"):
            dt.check_design(Z0, T0, c["E"], fake, truth=tr)


# ---- statuses -------------------------------------------------------------------------------------------------------------------
def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def indefinite_case(n, k, M, ncand, seed, where):
    """dt.case with Ahat_{k-1} = -1e-6 I -- harmless for theta in the box -- and, inserted at row ``where``, an entry whose
    theta_{k-1} = 40 makes A indefinite.  Returns (the case with the entry, the case without it)."""
    c = dt.case(n, k, M, ncand, seed)
    c["Ahat"] = c["Ahat"].copy()
    c["Ahat"][k - 1] = -1e-6 * np.eye(n)
    bad = c["theta"][0].copy()
    bad[k - 1] = 40.0
    with_bad = dict(c, theta=np.insert(c["theta"], where, bad, axis=0), M=M + 1)
    return with_bad, c


@pytest.mark.parametrize("kind", ["indefinite", "nan_theta"])
def test_a_skipped_entry_changes_no_other_number(kind):
    n, k, M, ncand, m, where = 8, 4, 33, 130, 8, 5
    wb, c = indefinite_case(n, k, M, ncand, SEED, where)
    if kind == "nan_theta":
        wb["theta"][where, 1] = np.nan
    a, b = spec(wb, m, 1e-3), spec(c, m, 1e-3)
    assert a.skipped[where] == (1 if kind == "indefinite" else 2) and a.skipped.sum() == a.skipped[where] and not b.skipped.any()
    assert np.array_equal(a.picks, b.picks)
    assert np.array_equal(_bits(a.gain), _bits(b.gain)) and np.array_equal(_bits(a.information), _bits(b.information))
    assert np.array_equal(_bits(np.delete(a.posterior_sd, where, axis=0)), _bits(b.posterior_sd))
    from romhighcontrast_amd.inverse import sensor_prior_factor
    assert np.array_equal(a.posterior_sd[where], np.sqrt(np.diag(sensor_prior_factor(dt.prior_variances(k), k)) ** 2))   # the prior's
    Z0, T0, st = empty_state(wb, 1e-3)
    assert not Z0[where].any()
    observed(f"dopt host design with a skipped entry ({kind})", dt.check_design(Z0, T0, wb["E"], a, live=M)[0], 1.0)


def test_a_nan_candidate_is_never_picked():
    c = dt.case(5, 3, 7, 6, SEED)
    c["E"] = c["E"].copy()
    c["E"][2, 1] = np.nan
    c["E"][4, 0] = np.inf
    des = spec(c, 6, 1e-3)
    assert sorted(des.picks) == [0, 1, 3, 5] and des.stop_reason == "no_candidates" and des.nan_candidates == 2   # stop rule 2
    Z0, T0, _ = empty_state(c, 1e-3)
    observed("dopt host design with NaN candidates", dt.check_design(Z0, T0, c["E"], des)[0], 1.0)


# ---- stop rules -----------------------------------------------------------------------------------------------------------------
def test_stop_rule_gain():
    c = dt.case(8, 4, 33, 130, SEED)
    full = spec(c, 8, 1e-1)
    rel = 0.5 * (full.gain[3] + full.gain[4]) / full.gain[0]   # between the gains of the steps 3 and 4
    assert full.gain[4] < rel * full.gain[0] < full.gain[3]
    des = spec(c, 8, 1e-1, rel_tol=rel)
    assert des.stop_reason == "no_gain" and np.array_equal(des.picks, full.picks[:4])
    assert np.array_equal(_bits(des.gain), _bits(full.gain[:4])) and np.array_equal(_bits(des.information), _bits(full.information[:4]))


def test_everything_known_means_no_gain():
    c = dt.case(5, 3, 7, 37, SEED)
    des = spec(c, 5, 1e-3, prior=np.zeros(3))
    assert des.stop_reason == "no_gain" and len(des.picks) == 0 and len(des.information) == 0 and not des.posterior_sd.any()


# ---- a pinned parameter ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["variances", "covariance"])
def test_pinned_parameter_carries_no_information(form):
    """Zero prior variance: the parameter is known, its posterior sd stays 0, its column of Z is zero, and the design is the one
    the truth confirms for the singular prior."""
    n, k, M, ncand, m = 8, 4, 33, 130, 6
    c = dt.case(n, k, M, ncand, SEED)
    var = dt.prior_variances(k)
    var[2] = 0.0
    prior = var if form == "variances" else np.diag(var)
    des = spec(c, m, 1e-3, prior=prior)
    assert not des.posterior_sd[:, 2].any() and (des.posterior_sd[:, [0, 1, 3]] > 0).all()
    Z0, T0, _ = empty_state(c, 1e-3, prior=prior)
    assert not Z0[:, :, 2].any() if form == "variances" else np.abs(T0 @ T0.T - np.diag(var)).max() < 1e-15
    observed(f"dopt host design with a pinned parameter ({form})", dt.check_design(Z0, T0, c["E"], des)[0], 1.0)
    # the information is that of the three free parameters: the same design with a prior variance of 1e-300 agrees to roundoff
    var[2] = 1e-300
    near = spec(c, m, 1e-3, prior=var)
    assert np.array_equal(near.picks, des.picks) and np.allclose(near.information, des.information, rtol=1e-12, atol=0.0)


# ---- the submodular guarantee ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sigma", [1e-1, 1e-3])
def test_greedy_guarantee_against_random_sets(sigma):
    n, k, M, ncand, m = 8, 4, 33, 130, 8
    c = dt.case(n, k, M, ncand, SEED)
    des = spec(c, m, sigma)
    Z0, T0, _ = empty_state(c, sigma)
    truth = dt.Truth(Z0, T0, c["E"], des.picks)
    phi_greedy, bound = dt.criterion(Z0, c["E"], des.picks), truth.information(M)[1][-1]
    rng = np.random.default_rng(99)
    best = 0.0
    for _ in range(50):
        S = rng.choice(ncand, size=m, replace=False)
        phi = dt.criterion(Z0, c["E"], S)
        best = max(best, float(phi))
        assert phi_greedy >= (1.0 - 1.0 / np.e) * phi - bound, (phi_greedy, phi, S)
    print(f"sigma {sigma:g}: Phi(greedy) = {float(phi_greedy):.4f} nats, the best of 50 random sets {best:.4f}")


# ---- the host-only entry point and the wrappers -----------------------------------------------------------------------------------
def test_layout_and_prototypes():
    from romhighcontrast_amd import _ffi
    lib = _ffi.load_library()
    for name in ("rom_sensor_dopt_layout", "rom_sensor_dopt_init", "rom_sensor_dopt_scores", "rom_sensor_dopt"):
        assert name in _ffi.PROTOTYPES and hasattr(lib, name), name
    for n, k, kp in [(1, 1, 1), (5, 3, 4), (8, 4, 4), (50, 5, 8), (64, 9, 16), (64, 16, 16), (2, 2, 2)]:
        lay = _ffi.sensor_dopt_layout(n, k)
        npad = (n + 3) // 4 * 4
        assert lay["kp"] == kp and lay["n_padded"] == npad and lay["entry"] == kp * npad + kp * kp + 2, lay
        assert lay["chunk"] * kp == 2048 and lay["t_offset"] == kp * npad and lay["status_offset"] == kp * (npad + kp) and lay["table"] == 128
        assert lay["lds_bytes"] == (128 + 64) * (npad + 2) * 8 <= 160 * 1024
    for n, k, word in [(0, 1, "n = 0"), (65, 1, "n = 65"), (4, 0, "k = 0"), (4, 17, "k = 17")]:
        with pytest.raises(ValueError, match=word):
            _ffi.sensor_dopt_layout(n, k)
    for name in ("sensor_dopt_layout", "sensor_dopt_init", "sensor_dopt_scores", "sensor_dopt"):
        assert callable(getattr(_ffi.Context, name))


def test_argument_errors_of_the_specification():
    from romhighcontrast_amd.inverse import sensor_prior_factor
    c = dt.case(5, 3, 7, 37, SEED)
    for bad in (0.0, -1.0, np.inf, np.nan):
        with pytest.raises(ValueError, match="sigma"):
            spec(c, 3, bad)
    with pytest.raises(ValueError, match="m = 38"):
        spec(c, 38, 1e-3)
    with pytest.raises(ValueError, match="variances"):
        sensor_prior_factor([1.0, -1.0, 1.0], 3)
    with pytest.raises(ValueError, match="positive semi-definite"):
        sensor_prior_factor(np.array([[1.0, 2.0], [2.0, 1.0]]), 2)
    with pytest.raises(ValueError, match="symmetric"):
        sensor_prior_factor(np.array([[1.0, 0.5], [0.0, 1.0]]), 2)
    C = np.array([[2.0, 0.5], [0.5, 1.0]])
    T0 = sensor_prior_factor(C, 2)
    assert np.abs(T0 @ T0.T - C).max() < 1e-15
