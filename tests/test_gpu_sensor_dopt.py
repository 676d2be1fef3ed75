"""rom_sensor_dopt on the GPU against the long-double truth of tests/dopt_truth.py and the specification inverse.sensor_dopt_host.

Every call runs on NaN-framed operands -- THETA, E, STATE and SCORE from an offset inside wider NaN blocks, THETA and E with padded
leading dimensions, Ahat and bhat with a NaN tail -- which must come back bit for bit (STATE and SCORE: everything outside their
blocks), and is made twice with equal bits.  Against the truth: the empty state's sensitivities, the scores after init and after
each of three updates, the picks, gain, information and posterior_sd of a whole design; where the truth's gap between the two best
candidates exceeds 4 x the bound -- asserted for every seeded case -- the picks equal the specification's.  Shapes (n, k, M, ncand,
m): the four of tests/test_dopt_host.py; k = 3, 5, 9 (kp = 4, 8, 16); ncand = 129, one past a candidate table; M kp = 33, one row
past a slab; M one past the chunk length of rom_sensor_dopt_layout (the partial sums and their reduction)."""
import numpy as np
import pytest

import dopt_truth as dt
from conftest import observed
from test_dopt_host import IDS, SEED, SHAPES, SIGMAS, spec
from test_gpu_lm_polish import Tail, _bits

pytestmark = pytest.mark.gpu

EXTRA = [(6, 3, 9, 40, 4), (6, 5, 9, 40, 4), (12, 9, 5, 40, 4), (5, 3, 7, 129, 5), (4, 1, 33, 20, 3), (2, 1, 2049, 17, 3)]
CASES = [(s, sg) for s in SHAPES for sg in SIGMAS] + [(s, 1e-3) for s in EXTRA]
CASE_IDS = [f"{'x'.join(str(v) for v in s)}-{sg:g}" for s, sg in CASES]


@pytest.fixture(scope="module")
def ctx():
    from romhighcontrast_amd import _ffi
    return _ffi.get_context()


class Problem:
    """A case on the device: the framed operands, and the calls made twice."""

    def __init__(self, ctx, c, sigma, prior=None):
        from romhighcontrast_amd.inverse import sensor_prior_factor
        self.ctx, self.c, self.sigma = ctx, c, sigma
        self.n, self.k, self.M, self.ncand = c["n"], c["k"], len(c["theta"]), len(c["E"])
        n, k, M, ncand = self.n, self.k, self.M, self.ncand
        self.lay = ctx.sensor_dopt_layout(n, k)
        self.T0 = sensor_prior_factor(dt.prior_variances(k) if prior is None else prior, k)
        self.ldt, self.lde, self.s_off = k + 3, n + 3, 3
        self.t_off, self.e_off = self.ldt + 1, self.lde + 1
        th = np.full((M + 2, self.ldt), np.nan)
        th[1:1 + M, 1:1 + k] = c["theta"]
        eh = np.full((ncand + 2, self.lde), np.nan)
        eh[1:1 + ncand, 1:1 + n] = c["E"]
        self.ops = [Tail(ctx, c["Ahat"]), Tail(ctx, c["bhat"]), Tail(ctx, th), Tail(ctx, eh)]
        self.size = M * self.lay["entry"]

    def unchanged(self):
        for op in self.ops:
            assert op.unchanged(), "an input buffer was modified"

    def framed_state(self, body=None):
        sh = np.full(self.s_off + self.size + 4, np.nan)
        if body is not None:
            sh[self.s_off:self.s_off + self.size] = body
        return self.ctx.upload(sh)

    def body(self, STATE):
        raw = STATE.download()
        assert np.isnan(raw[:self.s_off]).all() and np.isnan(raw[self.s_off + self.size:]).all(), "STATE's frame"
        return raw[self.s_off:self.s_off + self.size].copy()

    def init(self):
        """The empty state, twice: (the body of STATE, info)."""
        out = []
        for _ in range(2):
            STATE = self.framed_state()
            _, info = self.ctx.sensor_dopt_init(self.n, self.k, self.ops[0].buf, self.ops[1].buf, self.ops[2].buf, self.t_off, self.ldt,
                                                self.M, self.T0, self.sigma, STATE=STATE, s_off=self.s_off)
            out.append((self.body(STATE), info))
        self.unchanged()
        assert np.array_equal(_bits(out[0][0]), _bits(out[1][0])), "two init calls, different bits"
        assert not np.isnan(out[0][0]).any() and out[0][1]["launches"] == 1 and out[0][1]["host_syncs"] == 1, out[0][1]
        return out[0]

    def unpack(self, body):
        """(Z (M, n, k), T (M, k, k), status (M,)) of a STATE body; the padding must be zero."""
        lay, n, k = self.lay, self.n, self.k
        rows = body.reshape(self.M, lay["entry"])
        Zt = rows[:, :lay["t_offset"]].reshape(self.M, lay["kp"], lay["n_padded"])
        T = rows[:, lay["t_offset"]:lay["status_offset"]].reshape(self.M, lay["kp"], lay["kp"])
        assert not Zt[:, k:, :].any() and not Zt[:, :, n:].any() and not T[:, k:, :].any() and not T[:, :, k:].any(), "padding not zero"
        return np.ascontiguousarray(Zt[:, :k, :n].transpose(0, 2, 1)), T[:, :k, :k].copy(), rows[:, lay["status_offset"]].astype(np.int64)

    def scores(self, body, x0=0, count=None):
        """rom_sensor_dopt_scores of the candidates [x0, x0 + count) on the state, twice."""
        count = self.ncand - x0 if count is None else count
        STATE = self.framed_state(body)
        out = []
        for _ in range(2):
            SCORE = self.ctx.upload(np.full(5 + count + 3, np.nan))
            self.ctx.sensor_dopt_scores(self.n, self.k, STATE, self.s_off, self.M, self.ops[3].buf, self.e_off + x0 * self.lde, self.lde,
                                        count, SCORE=SCORE, sc_off=5)
            raw = SCORE.download()
            assert np.isnan(raw[:5]).all() and np.isnan(raw[5 + count:]).all(), "SCORE's frame"
            out.append(raw[5:5 + count].copy())
        self.unchanged()
        assert np.array_equal(_bits(self.body(STATE)), _bits(body)), "the scoring pass modified STATE"
        assert np.array_equal(_bits(out[0]), _bits(out[1])), "two scoring calls, different bits"
        return out[0]

    def design(self, body, m, rel_tol=0.0, taken=None):
        """rom_sensor_dopt on a copy of the state, twice: (picks, gain, info, the body afterwards)."""
        out = []
        for _ in range(2):
            STATE = self.framed_state(body)
            picks, gain, info = self.ctx.sensor_dopt(self.n, self.k, STATE, self.s_off, self.M, self.ops[3].buf, self.e_off, self.lde,
                                                     self.ncand, m, rel_tol=rel_tol, taken=taken)
            out.append((picks, gain, info, self.body(STATE)))
        self.unchanged()
        assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(_bits(out[0][1]), _bits(out[1][1])), "two designs, different picks"
        assert np.array_equal(_bits(out[0][3]), _bits(out[1][3])) and out[0][2] == out[1][2], "two designs, different bits"
        chunks = -(-self.M // self.lay["chunk"])
        assert out[0][2]["host_syncs"] == 1 and out[0][2]["launches"] == (3 + (chunks > 1)) * m, out[0][2]
        return out[0]


def design_tuple(p, picks, gain, body, info):
    from romhighcontrast_amd.inverse import DOPT_STOPS, SensorDesign
    _, T, st = p.unpack(body)
    live = p.M - int((st != 0).sum())
    return SensorDesign(picks, gain, np.cumsum(gain) / (2.0 * live), np.sqrt(np.einsum("jab,jab->ja", T, T)), DOPT_STOPS[info["stop_reason"]], st,
                        info["nan_candidates"])


@pytest.mark.parametrize("shape,sigma", CASES, ids=CASE_IDS)
def test_device_against_the_truth(ctx, shape, sigma):
    n, k, M, ncand, m = shape
    c = dt.case(n, k, M, ncand, SEED)
    p = Problem(ctx, c, sigma)
    if shape == EXTRA[-1]:
        assert M == p.lay["chunk"] + 1
    body0, info = p.init()
    Z0, T, st = p.unpack(body0)
    assert info["skipped"] == 0 and not st.any() and np.array_equal(T, np.broadcast_to(p.T0, (M, k, k)))
    X = Z0 * sigma / np.diag(p.T0)[None, None, :]
    observed(f"dopt device sensitivities {shape}", dt.check_sensitivities(c, X), 1.0 + 8 * dt.EPS)   # (X recovered with two roundings)
    # the whole design
    picks, gain, info, body = p.design(body0, m)
    des = design_tuple(p, picks, gain, body, info)
    assert des.stop_reason == "m" and len(picks) == m and info["skipped"] == 0 and info["nan_candidates"] == 0
    worst, truth = dt.check_design(Z0, p.T0, c["E"], des)
    observed(f"dopt device design / bound {shape} sigma {sigma:g}", worst, 1.0)
    for t, (gap, bound) in enumerate(dt.pick_gaps(truth)):
        assert gap > 4.0 * bound, (t, gap, bound)
    assert np.array_equal(picks, spec(c, m, sigma).picks)
    # the scores after init and after each of three updates, one step per call
    steps = min(3, m)
    worst, b, taken = dt.check_scores(truth, 0, p.scores(body0)), body0, []
    for t in range(steps):
        pk, g, _, b = p.design(b, 1, taken=taken)
        assert pk[0] == picks[t] and _bits(g)[0] == _bits(gain)[t]
        taken.append(int(pk[0]))
        worst = max(worst, dt.check_scores(truth, t + 1, p.scores(b)))
    observed(f"dopt device scores / bound {shape} sigma {sigma:g}", worst, 1.0)


def test_candidate_ranges_have_the_bits_of_the_whole(ctx):
    for shape in [(8, 4, 33, 70, 3), (2, 1, 2049, 70, 3)]:
        n, k, M, ncand, m = shape
        p = Problem(ctx, dt.case(n, k, M, ncand, SEED), 1e-3)
        body = p.design(p.init()[0], 2)[3]
        whole = p.scores(body)
        parts = np.concatenate([p.scores(body, 0, 33), p.scores(body, 33, 37)])
        assert np.array_equal(_bits(whole), _bits(parts)), shape


def test_a_split_design_has_the_bits_of_the_whole(ctx):
    for shape in [(8, 4, 33, 130, 6), (2, 1, 2049, 17, 6)]:
        n, k, M, ncand, m = shape
        p = Problem(ctx, dt.case(n, k, M, ncand, SEED), 1e-1)
        body0 = p.init()[0]
        picks, gain, info, body = p.design(body0, 6)
        p1, g1, _, b1 = p.design(body0, 3)
        p2, g2, _, b2 = p.design(b1, 3, taken=p1)
        assert np.array_equal(picks, np.r_[p1, p2]) and np.array_equal(_bits(gain), _bits(np.r_[g1, g2])), shape
        assert np.array_equal(_bits(body), _bits(b2)), shape


def test_statuses(ctx):
    from test_dopt_host import indefinite_case
    n, k, M, ncand, m, where = 8, 4, 33, 130, 6, 5
    wb, c = indefinite_case(n, k, M, ncand, SEED, where)
    wb["theta"][9, 2] = np.nan   # a second skipped entry, status 2
    wb["E"] = wb["E"].copy()
    wb["E"][11, 3] = np.nan
    p = Problem(ctx, wb, 1e-3)
    body0, info = p.init()
    Z0, T, st = p.unpack(body0)
    assert info["skipped"] == 2 and st[where] == 1 and st[9] == 2 and st.sum() == 3 and not Z0[[where, 9]].any()
    picks, gain, info, body = p.design(body0, m)
    assert info["skipped"] == 2 and info["nan_candidates"] == 1 and 11 not in picks and info["stop_reason"] == 0
    des = design_tuple(p, picks, gain, body, info)
    observed("dopt device design with skipped entries and a NaN candidate", dt.check_design(Z0, p.T0, wb["E"], des, live=M - 1)[0], 1.0)
    # against the call without the two entries: the same picks and, the sums being exact with the zeros, the same bits in the gains
    c2 = dict(c, theta=np.delete(wb["theta"], [where, 9], axis=0), E=wb["E"])
    q = Problem(ctx, c2, 1e-3)
    picks2, gain2, _, _ = q.design(q.init()[0], m)
    assert np.array_equal(picks, picks2) and np.array_equal(_bits(gain), _bits(gain2))


def test_stop_rules(ctx):
    c = dt.case(8, 4, 33, 130, SEED)
    p = Problem(ctx, c, 1e-1)
    body0 = p.init()[0]
    full = p.design(body0, 8)
    rel = 0.5 * (full[1][3] + full[1][4]) / full[1][0]
    picks, gain, info, _ = p.design(body0, 8, rel_tol=rel)
    assert info["stop_reason"] == 1 and info["picks"] == 4 and np.array_equal(picks, full[0][:4]) and np.array_equal(_bits(gain), _bits(full[1][:4]))
    c = dt.case(5, 3, 7, 6, SEED)
    c["E"] = c["E"].copy()
    c["E"][2, 1] = np.nan
    c["E"][4, 0] = np.inf
    p = Problem(ctx, c, 1e-3)
    picks, gain, info, _ = p.design(p.init()[0], 6)
    assert info["stop_reason"] == 2 and sorted(picks) == [0, 1, 3, 5] and info["nan_candidates"] == 2
    assert np.array_equal(picks, spec(c, 6, 1e-3).picks)
    # everything known: nothing to gain, no pick
    p = Problem(ctx, dt.case(5, 3, 7, 37, SEED), 1e-3, prior=np.zeros(3))
    picks, gain, info, _ = p.design(p.init()[0], 5)
    assert info["stop_reason"] == 1 and len(picks) == 0


def test_limits_raise_value_error(ctx):
    c = dt.case(5, 3, 7, 37, SEED)
    p = Problem(ctx, c, 1e-3)
    body0 = p.init()[0]
    STATE, E = p.framed_state(body0), p.ops[3].buf
    A, b, TH = (op.buf for op in p.ops[:3])
    n, k, M, nc = 5, 3, 7, 37

    def dopt(n=n, k=k, M=M, ncand=nc, m=3, lde=p.lde, e_off=p.e_off, s_off=p.s_off, **kw):
        return ctx.sensor_dopt(n, k, STATE, s_off, M, E, e_off, lde, ncand, m, **kw)

    for kw, word in [(dict(n=0), "n = 0"), (dict(n=65), "n = 65"), (dict(k=0), "k = 0"), (dict(k=17), "k = 17"), (dict(M=0), "M = 0"),
                     (dict(M=2 ** 24 + 1), "M = 16777217"), (dict(ncand=0), "ncand = 0"), (dict(ncand=2 ** 22 + 1), "ncand = 4194305"),
                     (dict(m=0), "m = 0"), (dict(m=38), "m = 38"), (dict(ncand=2000, m=1025), "m = 1025"), (dict(M=8), "STATE holds"),
                     (dict(lde=4), "lde = 4"), (dict(ncand=45), "E holds"), (dict(e_off=2 ** 62), "E holds"), (dict(s_off=2 ** 62), "STATE holds"),
                     (dict(rel_tol=-0.1), "rel_tol"), (dict(rel_tol=1.0), "rel_tol"), (dict(taken=[37]), "taken"), (dict(taken=[-1]), "taken")]:
        with pytest.raises(ValueError, match=word):
            dopt(**kw)
    for kw, word in [(dict(n=65), "n = 65"), (dict(k=17), "k = 17"), (dict(M=0), "M = 0"), (dict(ncand=0), "ncand = 0"), (dict(ncand=45), "E holds")]:
        a = dict(n=n, k=k, M=M, ncand=nc)
        a.update(kw)
        with pytest.raises(ValueError, match=word):
            ctx.sensor_dopt_scores(a["n"], a["k"], STATE, p.s_off, a["M"], E, p.e_off, p.lde, a["ncand"])
    with pytest.raises(ValueError, match="SCORE holds"):
        ctx.sensor_dopt_scores(n, k, STATE, p.s_off, M, E, p.e_off, p.lde, nc, SCORE=ctx.alloc(36))
    for kw, word in [(dict(n=65), "n = 65"), (dict(k=17), "k = 17"), (dict(M=0), "M = 0"), (dict(sigma=0.0), "sigma"), (dict(sigma=np.nan), "sigma"),
                     (dict(ldt=2), "ldt = 2"), (dict(M=8), "STATE holds"), (dict(T0=np.full((3, 3), np.nan)), "T0")]:
        a = dict(n=n, k=k, M=M, sigma=1e-3, ldt=p.ldt, T0=p.T0)
        a.update(kw)
        with pytest.raises(ValueError, match=word):
            ctx.sensor_dopt_init(a["n"], a["k"], A, b, TH, p.t_off, a["ldt"], a["M"], np.resize(a["T0"], (a["k"], a["k"])), a["sigma"],
                                 STATE=STATE, s_off=p.s_off)
    assert np.array_equal(_bits(p.body(STATE)), _bits(body0)), "a refused call wrote to STATE"
    from romhighcontrast_amd.inverse import sensor_dopt_device
    with pytest.raises(ValueError, match="m = 1025"):
        sensor_dopt_device(ctx, c["Ahat"], c["bhat"], c["theta"], np.zeros((2000, 5)), 1025, 1e-3, dt.prior_variances(3))


# ---- end to end -----------------------------------------------------------------------------------------------------------------
def test_end_to_end_on_a_real_space(ctx):
    """(2, 2) / N = 8, a POD basis of n = 6, 64 library parameters, all interior vertices as candidates, m = 8: the design's points go
    into observe; Phi of the design, in long double, is at least (1 - 1/e) of that of select_sensors_pbdw's eight points, minus the
    bound; the device design is the specification's."""
    from romhighcontrast_amd.inverse import ParameterLibrary, select_sensors_parameters, sensor_prior_factor, sensor_sensitivities_host
    from romhighcontrast_amd.lib.ReducedBasis import _as_device, pod_modes, select_sensors_pbdw
    from src.lib.ReducedBasis import BaseReducedBasis
    from src.lib.SolutionsManagers import SolutionsManagerFEM
    sm = SolutionsManagerFEM((2, 2), 8)
    rng = np.random.default_rng(5)
    U = sm.generate_solutions(10.0 ** rng.uniform(0.0, 2.0, size=(32, 2, 2)))
    basis, _ = pod_modes(sm._ctx, _as_device(sm._ctx, np.array(U), sm.vspace_dim), 6, center=False)
    a_lib = 10.0 ** rng.uniform(0.0, 2.0, size=(64, 2, 2))
    cand, m, sigma = sm.interior_vertices(), 8, 1e-3
    lib = ParameterLibrary(sm, basis, a_lib)
    des = lib.select_sensors(cand, m, sigma)
    host = lib.select_sensors(cand, m, sigma, device=False)
    assert des.points.shape == (m, 2) and des.stop_reason == "m" and not des.skipped.any() and des.posterior_sd.shape == (64, 4)
    assert np.array_equal(des.points, cand[des.picks])
    lib.observe(des.points)
    assert lib.E.shape == (6, m)
    # the truth of this design
    la = np.log(lib.a)
    Ec = np.ascontiguousarray(sm._fem.evaluate_points(lib._W, lib.n, *sm._locate(cand)).T)
    T0 = sensor_prior_factor((la.max(axis=0) - la.min(axis=0)) ** 2 / 12.0, 4)
    Z0 = sensor_sensitivities_host(lib.Ahat, lib.bhat, la) @ T0 / sigma
    worst, truth = dt.check_design(Z0, T0, Ec, des)
    observed("dopt device design / bound, end to end", worst, 1.0)
    if all(gap > 4.0 * bound for gap, bound in dt.pick_gaps(truth)):
        assert np.array_equal(des.picks, host.picks)
    bound = truth.information(64)[1][-1]
    phi = dt.criterion(Z0, Ec, des.picks)
    assert abs(float(phi - des.information[-1])) <= bound
    pbdw = select_sensors_pbdw(sm, basis, cand, m)
    phi_pbdw = dt.criterion(Z0, Ec, pbdw.picks)
    rnd = max(float(dt.criterion(Z0, Ec, rng.choice(len(cand), size=m, replace=False))) for _ in range(20))
    print(f"Phi in nats: D-optimal {float(phi):.4f}, PBDW greedy ({len(pbdw.picks)} points) {float(phi_pbdw):.4f}, best of 20 random sets {rnd:.4f}")
    assert phi >= (1.0 - 1.0 / np.e) * phi_pbdw - bound
    # the other two ways in
    again = select_sensors_parameters(sm, basis, a_lib, cand, m, sigma)
    rb = BaseReducedBasis()
    rb.set(basis, a_lib[:6])
    third = rb.select_sensors_parameters(sm, cand, m, a_lib, sigma, subset=np.arange(64))
    assert np.array_equal(again.picks, des.picks) and np.array_equal(third.picks, des.picks)
    assert np.array_equal(_bits(again.gain), _bits(des.gain)) and np.array_equal(_bits(third.gain), _bits(des.gain))
