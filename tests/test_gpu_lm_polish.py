"""rom_lm_polish on the GPU against polish_parameters and the checker of tests/lm_truth.py.

Every call runs on NaN-framed operands -- P and OUT as column ranges of wider NaN blocks from an offset, the others with a NaN
tail -- which must come back bit for bit (OUT: everything outside its rows); every call is made twice and must return the same
bits; every result goes through check_state.  Shapes (n, k, r, K, t): the smallest; r < n; odd sizes; the limits (64, 16, 64);
one system past 256 with t = 1; one query with t = 8.

max_iter 0: theta is the clipped start bit for bit, start and iterations are the host's.  max_iter 1, 2:
|theta_dev - theta_host| <= max(1e3 d, 1e-11 (1 + max|theta|)), d the host's own difference when its sensor rows are permuted
(the device's elimination differs from LAPACK's by more than a reordering)."""
import numpy as np
import pytest

import lm_truth as lt
import nearest_truth as nt

pytestmark = pytest.mark.gpu

#          n   k   r   K    t
SHAPES = [(1,  1,  1,  3,   3),
          (10, 4,  6,  5,   3),
          (33, 9,  20, 5,   3),
          (64, 16, 64, 6,   3),
          (10, 4,  6,  257, 1),
          (10, 4,  6,  1,   8)]
IDS = ["x".join(map(str, s)) for s in SHAPES]


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


def run(ctx, model, P, theta0, aux=None, max_iter=30, misfit_tol=1e-3, check=True):
    """rom_lm_polish twice on NaN-framed operands; returns (PolishResult, info)."""
    n, k, r = model["n"], model["k"], model["r"]
    P = np.atleast_2d(P)
    K = len(P)
    theta0 = np.asarray(theta0, dtype=np.float64).reshape(K, -1, k)
    t = theta0.shape[1]
    ldp, p_off, ldo, o_off = r + 3, r + 3 + 1, k + n + 5 + 2, 3
    ph = np.full((K + 2, ldp), np.nan)
    ph[1:1 + K, 1:1 + r] = P
    ops = [Tail(ctx, model["Ahat"]), Tail(ctx, model["bhat"]), Tail(ctx, model["Gr"]), Tail(ctx, ph), Tail(ctx, theta0)]
    auxb = Tail(ctx, aux) if aux is not None else None
    outs = []
    for _ in range(2):
        OUT = ctx.upload(np.full(o_off + K * ldo + 4, np.nan))
        res, info = ctx.lm_polish(n, k, r, ops[0].buf, ops[1].buf, ops[2].buf, ops[3].buf, p_off, ldp, K, t, ops[4].buf, model["lo"],
                                  model["hi"], AUX=auxb.buf if auxb else None, max_iter=max_iter, misfit_tol=misfit_tol, OUT=OUT,
                                  out_off=o_off, ldo=ldo)
        raw = OUT.download()
        body = raw[o_off:o_off + K * ldo].reshape(K, ldo)
        assert np.isnan(raw[:o_off]).all() and np.isnan(raw[o_off + K * ldo:]).all() and np.isnan(body[:, k + n + 5:]).all(), "OUT's frame"
        assert not np.isnan(body[:, :k + n + 5]).any()
        outs.append((raw, res, info))
    for op in ops + ([auxb] if auxb else []):
        assert op.unchanged(), "an input buffer was modified"
    assert np.array_equal(_bits(outs[0][0]), _bits(outs[1][0])), "two calls, different bits"
    res, info = outs[0][1], outs[0][2]
    assert info["launches"] == 2 and info["host_syncs"] == 1 and info["systems"] == K * t, info
    assert info["iterations"] <= max_iter * K * t and info["factorisations"] >= K * t, info
    if max_iter == 0:
        assert info["iterations"] == 0 and info["factorisations"] == K * t, info
    if check:
        worst = lt.check_state(model, P, aux, res, theta0=theta0, misfit_tol=misfit_tol, max_iter=max_iter)
        print(f"check_state: largest observed / bound {worst:.3g}; {info}")
    return res, info


@pytest.fixture(scope="module")
def cases():
    """Per shape: the model (seed 7), theta*, ROM-exact P, the starts theta* + 0.1 N(0, 1)."""
    out = {}
    for n, k, r, K, t in SHAPES:
        model = lt.synth(n, k, r, 7)
        theta_true, P = lt.exact_queries(model, K, 7)
        theta0 = theta_true[:, None, :] + 0.1 * np.random.default_rng(8).standard_normal((K, t, k))
        out[(n, k, r, K, t)] = (model, theta_true, P, theta0)
    return out


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_recovers_rom_exact_parameters(ctx, cases, shape):
    model, theta_true, P, theta0 = cases[shape]
    res, info = run(ctx, model, P, theta0)
    err = np.abs(res.theta - theta_true).max(axis=1)
    print(f"max |theta - theta*| {err.max():.3g}; iterations up to {res.iterations.max()}; unflagged {int((~res.converged).sum())}")
    assert res.converged.all(), np.flatnonzero(~res.converged)
    assert (err <= 1e-8).all(), err.max()


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_first_iterations_follow_the_host(ctx, cases, shape):
    model, _, P, theta0 = cases[shape]
    K, r = len(P), model["r"]
    perm = np.random.default_rng(9).permutation(r)
    permuted = dict(model, Gr=model["Gr"][perm])
    for max_iter in (0, 1, 2):
        res, _ = run(ctx, model, P, theta0, max_iter=max_iter)
        host = lt.host_polish(model, P, theta0, max_iter=max_iter)
        if max_iter == 0:
            clipped = np.clip(theta0, model["lo"], model["hi"])
            assert np.array_equal(res.start, host.start) and np.array_equal(res.iterations, host.iterations)
            assert np.array_equal(_bits(res.theta), _bits(clipped[np.arange(K), res.start]))
            continue
        again = lt.host_polish(permuted, P[:, perm], theta0, max_iter=max_iter)
        d = np.abs(again.theta - host.theta).max(axis=1)
        bound = np.maximum(1e3 * d, 1e-11 * (1.0 + np.abs(host.theta).max(axis=1)))
        diff = np.abs(res.theta - host.theta).max(axis=1)
        print(f"max_iter {max_iter}: device - host up to {diff.max():.3g}, host - permuted host up to {d.max():.3g}, largest ratio to "
              f"the bound {(diff / bound).max():.3g}, to 1e-11 (1 + max|theta|) {(diff / (1e-11 * (1.0 + np.abs(host.theta).max(axis=1)))).max():.3g}")
        assert np.array_equal(res.iterations, host.iterations)
        assert (diff <= bound).all(), (diff / bound).max()


def test_box(ctx, cases):
    model, theta_true, P, theta0 = cases[(10, 4, 6, 5, 3)]
    # starts outside the box are clipped
    wild = theta0 + np.array([-9.0, 9.0, 0.0, 0.0])
    res, _ = run(ctx, model, P, wild, max_iter=0)
    clipped = np.clip(wild, model["lo"], model["hi"])
    assert np.array_equal(_bits(res.theta), _bits(clipped[np.arange(len(P)), res.start]))
    res, _ = run(ctx, model, P, wild)
    # theta*_0 = lo exactly, starts below it
    edge = theta_true.copy()
    edge[:, 0] = model["lo"][0]
    Pe = lt.coefficients(model, edge) @ model["Gr"].T
    below = edge[:, None, :] + 0.1 * np.random.default_rng(10).standard_normal((len(Pe), 3, 4))
    below[:, :, 0] = model["lo"][0] - 0.3
    res, _ = run(ctx, model, Pe, below)
    assert (res.theta[:, 0] >= model["lo"][0]).all()
    print(f"theta_0 - lo {res.theta[:, 0] - model['lo'][0]}; max |theta - theta*| {np.abs(res.theta - edge).max():.3g}; converged {res.converged}")


def test_sigma_min_of_a_nearly_rank_deficient_jacobian(ctx):
    model, theta = lt.twin_case()
    P = lt.coefficients(model, theta + 0.05) @ model["Gr"].T
    res, _ = run(ctx, model, P, theta, max_iter=0)
    J, A = lt.jacobian(model, res.theta[0])
    sv = np.linalg.svd(J, compute_uv=False)
    print(f"sigma_min device {res.sigma_min[0]!r}, NumPy {sv[-1]!r}, difference {abs(res.sigma_min[0] - sv[-1]):.3g}; bound "
          f"{64 * lt.EPS * np.linalg.cond(A) * sv[0]:.3g}")
    assert sv[-1] < 1e-6 * sv[0]


def _library_starts(rom, lib, Y, t):
    pred = nt.rom_coefficients(rom["Ahat"], rom["bhat"], lib) @ rom["E"]
    idx, _ = nt.brute_force(Y, pred, t)
    return np.log(lib[idx])


def _reduced(rom, Y):
    """The oracle ROM in reduced sensor coordinates: (model, P, aux)."""
    from romhighcontrast_amd.inverse import reduce_measurements, reduce_sensors
    U, Gr, _ = reduce_sensors(rom["E"])
    k, n = rom["Ahat"].shape[0], rom["Ahat"].shape[1]
    P, aux = reduce_measurements(U, Y, np.ones(Y.shape[1]))
    return dict(n=n, k=k, r=U.shape[1], Ahat=rom["Ahat"], bhat=rom["bhat"], Gr=Gr), P, aux


def test_oracle_rom_exact_queries(ctx):
    rom = nt.oracle_rom(decades=4.0)
    lib = nt.grid_library(rom["k"], 12, 4.0)
    a_true = 10.0 ** np.random.default_rng(1).uniform(0.0, 4.0, size=(64, rom["k"]))
    Y = nt.rom_coefficients(rom["Ahat"], rom["bhat"], a_true) @ rom["E"]
    starts = _library_starts(rom, lib, Y, 1)
    model, P, aux = _reduced(rom, Y)
    model.update(lo=np.zeros(rom["k"]), hi=np.full(rom["k"], np.log(1e4)))
    res, info = run(ctx, model, P, starts, aux=aux)
    err = np.abs(res.theta - np.log(a_true)).max(axis=1) / np.log(10.0)
    print(f"flagged {int(res.converged.sum())} of 64; max error of the flagged {err[res.converged].max():.3g}; errors of the unflagged "
          f"{np.sort(err[~res.converged])}; iterations up to {res.iterations.max()}")
    assert (err[res.converged] <= 1e-8).all()
    assert (~res.converged).sum() <= 6


def test_noise_agrees_with_the_host(ctx):
    from oracle import rom_oracle as ro
    rom = nt.oracle_rom(decades=2.0)
    g, k = rom["g"], rom["k"]
    lib = nt.grid_library(k, 12, 2.0)
    rng = np.random.default_rng(2)
    a_true = 10.0 ** rng.uniform(0.0, 2.0, size=(40,) + rom["blocks"])
    Y = ro.evaluate_solutions(g, rom["points"], ro.generate_solutions(g, a_true, "lsqsparse"))
    Y = Y + 1e-3 * np.abs(Y).max(axis=1, keepdims=True) * rng.standard_normal(Y.shape)
    starts = _library_starts(rom, lib, Y, 4)
    tol = 2e-3 * np.sqrt(Y.shape[1])
    from romhighcontrast_amd.inverse import polish_parameters
    host = polish_parameters(rom["Ahat"], rom["bhat"], rom["E"], Y, starts, 0.0, np.log(100.0), misfit_tol=tol)
    model, P, aux = _reduced(rom, Y)
    model.update(lo=np.zeros(k), hi=np.full(k, np.log(100.0)))
    res, _ = run(ctx, model, P, starts, aux=aux, misfit_tol=tol)
    diff = np.abs(res.misfit - host.misfit) / aux[:, 1]
    print(f"|misfit_dev - misfit_host| / scale sorted, largest five {np.sort(diff)[-5:]}; converged device {int(res.converged.sum())}, host "
          f"{int(host.converged.sum())} of 40")
    assert (diff <= 1e-10).sum() >= 38, np.sort(diff)[-5:]


def test_a_start_that_is_not_positive_definite_is_reported_once(ctx):
    """Ahat_0 negated: A(theta) is indefinite at the start, the call fails with ROM_ERR_NOT_SPD (which the binding, and only that
    status, raises as LinAlgError) -- and leaves the context's status word clear: rom_solve_status right after it reports nothing,
    and the same call on the sound model returns the bits it returned before."""
    from scipy.linalg import LinAlgError
    from romhighcontrast_amd._ffi import ROM_OK
    model = lt.synth(4, 2, 3, 7)
    theta_true, P = lt.exact_queries(model, 2, 7)
    theta0 = theta_true[:, None, :] + 0.1 * np.random.default_rng(8).standard_normal((2, 1, 2))
    up = ctx.upload

    def call(Ahat):
        OUT = up(np.full(2 * 11, np.nan))
        ctx.lm_polish(4, 2, 3, up(Ahat), up(model["bhat"]), up(model["Gr"]), up(P), 0, 3, 2, 1, up(theta0), model["lo"], model["hi"], OUT=OUT)
        return OUT.download()

    before = call(model["Ahat"])
    assert np.isfinite(before).all()
    broken = model["Ahat"].copy()
    broken[0] = -broken[0]
    with pytest.raises(LinAlgError, match="not positive definite"):
        call(broken)
    assert ctx.lib.rom_solve_status(ctx.h) == ROM_OK, "the failure of rom_lm_polish is reported a second time"
    after = call(model["Ahat"])
    assert np.isfinite(after).all() and np.array_equal(_bits(after), _bits(before))


def test_errors(ctx):
    from romhighcontrast_amd._ffi import RomLibraryError
    model = lt.synth(4, 2, 3, 7)
    _, P = lt.exact_queries(model, 2, 7)
    up = ctx.upload
    big = up(np.zeros(17 * 65 * 65))
    th, p = up(np.zeros(2 * 9 * 17)), up(np.zeros((2, 65)))
    lo, hi = np.zeros(17), np.ones(17)
    for (n, k, r, t, ldo), word in (((65, 2, 3, 1, 80), "n = 65"), ((4, 17, 3, 1, 80), "k = 17"), ((4, 2, 65, 1, 80), "r = 65"),
                                   ((4, 2, 3, 9, 80), "t = 9"), ((4, 2, 3, 1, 10), "ldo")):
        with pytest.raises(RomLibraryError, match=word) as e:
            ctx.lm_polish(n, k, r, big, big, big, p, 0, 65, 2, t, th, lo[:k], hi[:k], OUT=up(np.zeros(400)), ldo=ldo)
        assert "error 1" in str(e.value)   # ROM_ERR_INVALID
    res, info = ctx.lm_polish(4, 2, 3, up(model["Ahat"]), up(model["bhat"]), up(model["Gr"]), None, 0, 3, 0, 1, None, model["lo"], model["hi"])
    assert res.theta.shape == (0, 2) and res.coefficients.shape == (0, 4) and info["launches"] == 0 and info["host_syncs"] == 0
