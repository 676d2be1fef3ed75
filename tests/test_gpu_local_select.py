"""rom_local_select on the GPU against inverse.local_select_host and the long-double checker of tests/local_select_truth.py.

Every call runs on NaN-framed operands -- the tables RT and GR with a NaN tail, P and OUT as column ranges of wider NaN blocks
from an offset -- which must come back bit for bit (OUT: everything outside its rows); every call is made twice and must return
the same bits.  Device against the specification: equal pass counts and status; c, a and S within
max(1e3 delta, 1e-11 (1 + max|.|)) with delta the specification's own change when the rows of every G_j and R_j are permuted
(the rule of test_gpu_bvls.py); every system of status 0 through ``check_system``; equal labels except where the two smallest S
of the specification lie within 1e-9 relative (at most 5 % of a case -- and the cases are generated with a gap of 1e-6, which is
asserted here, so that there are none)."""
import numpy as np
import pytest

import local_select_truth as lt

pytestmark = pytest.mark.gpu
LAUNCHES = 3


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


def run(ctx, cs, max_iter=None, rows=None):
    """rom_local_select twice on NaN-framed operands, on the measurement vectors ``rows`` (a slice; all when None); returns
    (LocalSelectResult, info, the raw OUT rows (K kc, n + k + 5))."""
    n, k, kc, r = cs.n, cs.k, cs.kc, cs.r
    P = cs.P if rows is None else cs.P[rows]
    K, w = len(P), n + k + 5
    ldp, p_off, ldo, o_off = kc * r + 3, kc * r + 3 + 1, w + 2, 3
    ph = np.full((K + 2, ldp), np.nan)
    ph[1:1 + K, 1:1 + kc * r] = P
    ops = [Tail(ctx, cs.RT), Tail(ctx, cs.GR), Tail(ctx, ph)]
    outs = []
    for _ in range(2):
        OUT = ctx.upload(np.full(o_off + K * kc * ldo + 4, np.nan))
        res, info = ctx.local_select(kc, n, k, cs.rank, r, ops[0].buf, ops[1].buf, ops[2].buf, p_off, ldp, K, cs.c_lo, cs.c_hi, cs.a_lo,
                                     cs.a_hi, max_iter=max_iter, OUT=OUT, out_off=o_off, ldo=ldo)
        raw = OUT.download()
        body = raw[o_off:o_off + K * kc * ldo].reshape(K * kc, ldo)
        assert np.isnan(raw[:o_off]).all() and np.isnan(raw[o_off + K * kc * ldo:]).all() and np.isnan(body[:, w:]).all(), "OUT's frame"
        assert not np.isnan(body[:, n + k + 2:w]).any()
        outs.append((raw, res, info, body[:, :w].copy()))
    for op in ops:
        assert op.unchanged(), "an input buffer was modified"
    assert np.array_equal(_bits(outs[0][0]), _bits(outs[1][0])), "two calls, different bits"
    assert np.array_equal(outs[0][1].labels, outs[1][1].labels)
    res, info = outs[0][1], outs[0][2]
    assert info["launches"] == LAUNCHES and info["host_syncs"] == 1 and info["systems"] == K * kc, info
    assert info["passes"] == res.passes.sum() and info["unconverged"] == (res.status != 0).sum(), info
    # a solve factors once for its start and once per pass; a system refused for NaN / Inf in its measurements factors nothing
    assert info["factorisations"] == res.passes.sum() + 2 * ((res.status & 3) == 0).sum(), info
    return res, info, outs[0][3]


def follows(name, cs, res, host):
    """Equal status and passes; c, a, S within the permuted-specification bounds; the long-double checker; the labels."""
    assert np.array_equal(res.status, host.status), np.argwhere(res.status != host.status)
    assert np.array_equal(res.passes, host.passes), np.argwhere(res.passes != host.passes)
    bc, ba, bs = lt.host_bounds(name)
    dc = np.abs(res.c_all - host.c_all).max(axis=2)
    da = np.abs(res.a_all - host.a_all).max(axis=2)
    ds = np.abs(res.surrogate_all - host.surrogate_all)
    print(f"{name}: device - specification / bound: c {(dc / bc).max():.3g}, a {(da / ba).max():.3g}, S {(ds / bs).max():.3g} "
          f"(differences up to {dc.max():.3g}, {da.max():.3g}, {ds.max():.3g})")
    assert (dc <= bc).all() and (da <= ba).all() and (ds <= bs).all()
    pmax = np.abs(cs.P.reshape(cs.K, cs.kc, cs.r)).max(axis=2)   # (r = n can fit p exactly: the misfit is then rounding of |p|)
    assert (np.abs(res.misfit_all - host.misfit_all) <= 1e-12 * (host.misfit_all + pmax)).all()
    count, worst = lt.check_result(cs, res)
    print(f"{name}: {count} systems through the long-double checker, worst ratios to its bounds {worst}")
    assert count == (host.status == 0).sum()
    gap = lt.label_gap(host.surrogate_all, host.status)
    assert (gap >= lt.GAP).all(), f"the case has a near-tie in the specification itself: {gap.min():.3g}"
    clear = gap >= 1e-9
    assert clear.mean() >= 0.95
    assert np.array_equal(res.labels[clear], host.labels[clear])


@pytest.mark.parametrize("name", list(lt.SHAPES))
def test_follows_the_specification(ctx, name):
    cs, host = lt.case(name), lt.spec(name)
    assert (host.status == 0).all()
    res, info, _ = run(ctx, cs)
    follows(name, cs, res, host)
    print(f"{name}: labels {np.bincount(res.labels, minlength=cs.kc).tolist()}, passes up to {res.passes.max(axis=(0, 1)).tolist()}, {info}")


def test_tie_between_identical_clusters(ctx):
    """Cluster 2 of the (3, 2, 7, 5, 3, 5) case made a copy of cluster 1, which wins four of the five vectors: S is bit-equal
    between the two and the lower index is the label."""
    from romhighcontrast_amd.inverse import local_select_host
    cs = lt.case("small")
    RT, GR, P = cs.RT.copy(), cs.GR.copy(), cs.P.reshape(cs.K, cs.kc, cs.r).copy()
    RT[2], GR[2], P[:, 2] = RT[1], GR[1], P[:, 1]
    box = [b.copy() for b in (cs.c_lo, cs.c_hi, cs.a_lo, cs.a_hi)]
    for b in box:
        b[2] = b[1]
    tie = cs.replace(RT=RT, GR=GR, P=P.reshape(cs.K, -1), c_lo=box[0], c_hi=box[1], a_lo=box[2], a_hi=box[3])
    res, _, rows = run(ctx, tie)
    rows = rows.reshape(cs.K, cs.kc, -1)
    assert np.array_equal(_bits(rows[:, 1]), _bits(rows[:, 2]))
    assert (res.labels != 2).all() and (res.labels == 1).sum() >= 4
    assert np.array_equal(res.labels, local_select_host(*tie.args()).labels)


def test_boxes_of_a_and_c(ctx):
    """A box of a active at both ends (rho chosen so that the unconstrained minimiser lies outside on both sides), a pinned
    block of a, an infinite box of c and a pinned coordinate of c: against the specification and the checker."""
    from romhighcontrast_amd.inverse import local_select_host, local_select_matrix
    cs = lt.case("small")
    RT, a_lo, a_hi, c_lo, c_hi = cs.RT.copy(), cs.a_lo.copy(), cs.a_hi.copy(), cs.c_lo.copy(), cs.c_hi.copy()
    # cluster 0: rho = B(c) (0.2, 5) for the c of the first vector: the free minimiser is (0.2, 5), outside [1, 2]^2 on both sides
    c00 = lt.spec("small").c_all[0, 0]
    RT[0, :, 0] = local_select_matrix(RT[0], c00, cs.k) @ np.array([0.2, 5.0])
    a_lo[0], a_hi[0] = 1.0, 2.0
    a_lo[1, 1] = a_hi[1, 1] = 1.2345678901234      # pinned block of a
    c_lo[2], c_hi[2] = -np.inf, np.inf             # the reference's lstsq
    c_lo[1, 0] = c_hi[1, 0] = -0.0123456789        # pinned coordinate of c
    alt = cs.replace(RT=RT, a_lo=a_lo, a_hi=a_hi, c_lo=c_lo, c_hi=c_hi)
    host = local_select_host(*alt.args())
    res, _, _ = run(ctx, alt)
    assert np.array_equal(res.status, host.status) and (res.status == 0).all() and np.array_equal(res.passes, host.passes)
    print("device - specification / bound (c, a, S):", lt.within(res, host, lt.rule_bounds(alt, host)))
    lt.check_result(alt, res)
    assert np.array_equal(res.a_all[0, 0], [1.0, 2.0]), res.a_all[0, 0]
    assert np.array_equal(_bits(res.a_all[:, 1, 1]), _bits(np.full(cs.K, 1.2345678901234)))
    assert np.array_equal(_bits(res.c_all[:, 1, 0]), _bits(np.full(cs.K, -0.0123456789)))
    P = cs.P.reshape(cs.K, cs.kc, cs.r)
    ref = np.linalg.lstsq(cs.GR[2], P[:, 2].T, rcond=None)[0].T
    np.testing.assert_allclose(res.c_all[:, 2], ref, rtol=0, atol=1e-12 * np.abs(ref).max() * np.linalg.cond(cs.GR[2]))
    assert np.array_equal(res.labels, host.labels)


def test_nan_in_one_measurement_vector(ctx):
    """Vector 4 of the K = 70 case has a NaN in the measurements of cluster 1: that system gets status 1 and NaN results; a NaN
    in every cluster's block gives label -1.  The other vectors are bit-equal to a call without that row."""
    cs = lt.case("odd")
    P = cs.P.copy()
    P[4, cs.r + 2] = np.nan
    P[9] = np.nan
    res, info, rows = run(ctx, cs.replace(P=P))
    assert res.status[4, 1] == 1 and (res.status[4, [0, 2]] == 0).all() and res.labels[4] in (0, 2)
    assert np.isnan(res.c_all[4, 1]).all() and np.isnan(res.surrogate_all[4, 1]) and (res.passes[4, 1] == 0).all()
    assert (res.status[9] == 1).all() and res.labels[9] == -1 and np.isnan(res.coefficients[9]).all()
    assert info["unconverged"] == 4
    keep = np.r_[0:4, 5:9, 10:cs.K]
    _, _, rows_without = run(ctx, cs.replace(P=cs.P[keep], K=len(keep)))
    w = rows.shape[1]
    assert np.array_equal(_bits(rows.reshape(cs.K, cs.kc, w)[keep]), _bits(rows_without.reshape(len(keep), cs.kc, w)))
    # vector 4's clean systems equal those of the clean call
    res0, _, rows0 = run(ctx, cs)
    assert np.array_equal(_bits(rows.reshape(cs.K, cs.kc, w)[4, [0, 2]]), _bits(rows0.reshape(cs.K, cs.kc, w)[4, [0, 2]]))
    assert np.array_equal(res.labels[keep], res0.labels[keep])


def test_split_rows_same_bits(ctx):
    cs = lt.case("odd")
    whole, _, rows = run(ctx, cs)
    a, _, ra = run(ctx, cs, rows=slice(0, 33))
    b, _, rb = run(ctx, cs, rows=slice(33, 70))
    assert np.array_equal(_bits(rows), _bits(np.concatenate([ra, rb])))
    assert np.array_equal(whole.labels, np.concatenate([a.labels, b.labels]))


def test_max_iter_reports_open_solves(ctx):
    from romhighcontrast_amd.inverse import local_select_host
    cs = lt.case("small")
    for max_iter in (0, 1):
        host = local_select_host(*cs.args(), max_iter=max_iter)
        res, _, _ = run(ctx, cs, max_iter=max_iter)
        assert np.array_equal(res.status, host.status) and np.array_equal(res.passes, host.passes) and (res.passes <= max_iter).all()
        assert np.array_equal(res.labels, host.labels)
        lt.within(res, host, lt.rule_bounds(cs, host, max_iter=max_iter))
    assert (local_select_host(*cs.args(), max_iter=0).status == 12).all()


def test_limits(ctx):
    """ValueError just outside each limit of rom_local_select_layout (naming it), and the largest admissible shapes run."""
    from romhighcontrast_amd._ffi import local_select_layout
    for (n, k, rank, r), word in (((0, 1, 2, 1), "n = 0"), ((65, 4, 300, 70), "n = 65"), ((4, 0, 8, 4), "k = 0"), ((4, 17, 40, 4), "k = 17"),
                                  ((4, 2, 8, 3), "r = 3"), ((4, 2, 8, 97), "r = 97"), ((4, 3, 2, 4), "rank = 2")):
        with pytest.raises(ValueError, match=word):
            local_select_layout(n, k, rank, r)
    for n, k, r in ((1, 1, 1), (64, 16, 96), (32, 9, 96), (64, 4, 96)):
        top = local_select_layout(n, k, k, r)["rank_max"]
        lay = local_select_layout(n, k, top, r)
        assert lay["lds_bytes"] <= 64 * 1024 < local_select_layout(n, k, top, r)["lds_bytes"] + 8 * (k + 2)
        with pytest.raises(ValueError, match=f"rank = {top + 1}"):
            local_select_layout(n, k, top + 1, r)
    assert local_select_layout(64, 4, 257, 96)["rank_max"] >= 257 and local_select_layout(32, 9, 289, 96)["rank_max"] >= 289
    up = ctx.upload
    small = lt.case("small")
    with pytest.raises(ValueError, match="kc = 257"):
        ctx.local_select(257, 1, 1, 2, 1, up(np.zeros(257 * 4)), up(np.zeros(257)), up(np.zeros(257)), 0, 257, 1, -1.0, 1.0, 1.0, 2.0)
    bad = small.a_hi.copy()
    bad[1, 0] = np.nan
    OUT = up(np.full(400, np.nan))
    with pytest.raises(ValueError, match="cluster 1 coordinate 0 of a"):
        ctx.local_select(3, 3, 2, 7, 5, up(small.RT), up(small.GR), up(small.P), 0, 15, 5, small.c_lo, small.c_hi, small.a_lo, bad, OUT=OUT)
    assert np.isnan(OUT.download()).all(), "OUT was written"
    with pytest.raises(ValueError, match=r"at most 2\^23"):   # (the x extent of the fit kernel's grid)
        ctx.local_select(3, 3, 2, 7, 5, up(small.RT), up(small.GR), up(small.P), 0, 15, 2 ** 23 + 1, small.c_lo, small.c_hi, small.a_lo,
                         small.a_hi, OUT=OUT)
    assert np.isnan(OUT.download()).all(), "OUT was written"
    res, info = ctx.local_select(3, 3, 2, 7, 5, up(small.RT), up(small.GR), None, 0, 15, 0, small.c_lo, small.c_hi, small.a_lo, small.a_hi)
    assert res.labels.shape == (0,) and info["launches"] == 0 and info["host_syncs"] == 0
    # the largest shapes of each kind, each with the largest rank beside it: kc; n and r; k
    for n, k, r, kc, K in ((2, 1, 2, 256, 1), (64, 2, 96, 1, 2), (2, 16, 96, 2, 2)):
        rank = local_select_layout(n, k, k, r)["rank_max"]
        big = lt.make_case(n, k, rank, r, kc, K, seed=1)
        res, _, _ = run(ctx, big)
        assert (res.status == 0).all()
        systems = {(0, 0), (K - 1, kc - 1)}
        lt.check_result(big, res, systems=systems)


# ---- end to end on (2, 2) / N = 8 -------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def experiment(ctx):
    """The sizes of tests/test_gpu_local_basis.py: 600 parameters a ~ U(1, 100) (seed 42), rows 100.. training, rows 0..99 held
    out; kc = 4 clusters, n = 6; 24 sensors at interior vertices chosen with default_rng(3)."""
    from romhighcontrast_amd.lib.SolutionsManagers import SolutionsManagerFEM
    from romhighcontrast_amd.local import LocalReducedBasis
    sm = SolutionsManagerFEM(blocks_geometry=(2, 2), N=8)
    a = np.random.default_rng(42).uniform(1.0, 100.0, size=(600, 2, 2))
    U = np.asarray(sm.generate_solutions(a))
    lrb = LocalReducedBasis(4).build(6, sm, U[100:], a[100:])
    X, Yg = np.meshgrid(sm.points_c[1:-1], sm.points_r[1:-1])
    verts = np.c_[X.ravel(), Yg.ravel()]
    points = verts[np.random.default_rng(3).choice(len(verts), 24, replace=False)]
    Y = np.asarray(sm.evaluate_solutions(points, U[:100]))
    return sm, a, U, lrb, points, Y


def test_end_to_end_selection(ctx, experiment):
    """Noise-free measurements of the 100 held-out states, a_box = "global".  With j* = classify(a_true), the two provable
    inequalities: S_{i,j*} <= max(a_true) ||u_i - c_{ij*} W_{j*}||_{H^1_0} (the true parameter is admissible, and
    ||r(a; v)||_{H^-1} = ||u(a) - v||_a <= sqrt(max a) ... <= max(a) ||u - v||_{H^1_0}), and surrogate_i <= S_{i,j*} (j* is among
    the candidates).  Printed, not asserted: the share of rows with label = j*, and the rms H^1_0 errors of the selected, the
    oracle-best and the global-basis estimates.
    Measured on an MI355X: S_ij* / (max a ||u - c W||) up to 0.925, surrogate / S_ij* up to 1; label = j* on 0.78 of the rows (the
    cluster of smallest true error on 0.92); rms H^1_0 error selected 0.003355, j* 0.002332, oracle-best 0.002057, global basis
    of n = 6 0.009135."""
    import pickle
    from romhighcontrast_amd.lib.ReducedBasis import ReducedBasisPCA
    from romhighcontrast_amd.local import LocalSensing
    sm, a, U, lrb, points, Y = experiment
    held, a_true = U[:100], a[:100]
    sensing = lrb.observe(sm, points, a_box="global")
    assert isinstance(sensing, LocalSensing)
    a_flat = a[100:].reshape(500, -1)
    assert np.array_equal(sensing.a_lo, np.tile(a_flat.min(axis=0), (4, 1))) and np.array_equal(sensing.a_hi, np.tile(a_flat.max(axis=0), (4, 1)))
    assert ((a_true.reshape(100, -1) >= sensing.a_lo[0]) & (a_true.reshape(100, -1) <= sensing.a_hi[0])).all(), "held-out parameters in the box"
    est = sensing.estimate(Y, states=True)
    assert est.converged.all() and (est.labels >= 0).all()
    jstar = lrb.classify(a_true)
    rows = np.arange(100)
    # the state c_{ij*} W_{j*} of every row, lifted on the host from the downloaded bases
    lifted = np.stack([est.coefficients_all[i, jstar[i]] @ sensing.W[jstar[i]] for i in rows])
    err_star = np.asarray(sm.H10norm_diff(np.ascontiguousarray(lifted), np.ascontiguousarray(held)))
    S_star = est.surrogate_all[rows, jstar]
    amax = a_true.reshape(100, -1).max(axis=1)
    print(f"S_ij* / (max a ||u - c W||) up to {(S_star / (amax * err_star)).max():.3g}; surrogate / S_ij* up to {(est.surrogate / S_star).max():.3g}")
    assert (S_star <= amax * err_star * (1 + 1e-9)).all()
    assert (est.surrogate <= S_star).all()
    # states = c W_label
    want = np.stack([est.coefficients[i] @ sensing.W[est.labels[i]] for i in rows])
    scale = np.abs(want).max()
    assert np.abs(np.asarray(est.states) - want).max() <= 1e-12 * scale
    c2, st2 = lrb.state_estimation(sm, points, Y, return_coefs=True, a_box="global")
    assert np.abs(np.asarray(st2) - want).max() <= 1e-12 * scale and np.array_equal(c2, est.coefficients.T)
    # device=False: the specification on the same tables; the device within the rule of the permuted specification
    from romhighcontrast_amd.inverse import local_select_host
    host = sensing.estimate(Y, device=False)
    _, P, _ = sensing.reduce(Y)
    cs = lt.Case(sensing.n, sensing.k, sensing.rank, sensing.r, 4, 100, sensing.RT, sensing.GR, P, sensing.c_lo, sensing.c_hi, sensing.a_lo,
                 sensing.a_hi)
    perm = local_select_host(*lt.permuted(cs).args())
    assert np.array_equal(host.labels, est.labels) and np.array_equal(host.status, est.status)
    for x, y, yp in ((est.coefficients_all, host.coefficients_all, perm.c_all), (est.a_all, host.a_all, perm.a_all),
                     (est.surrogate_all[:, :, None], host.surrogate_all[:, :, None], perm.surrogate_all[:, :, None])):
        bound = np.maximum(1e3 * np.abs(yp - y).max(axis=2), 1e-11 * (1.0 + np.abs(y).max(axis=2)))
        assert (np.abs(x - y).max(axis=2) <= bound).all(), (np.abs(x - y).max(axis=2) / bound).max()
    pickle.loads(pickle.dumps(lrb))
    with pytest.raises(TypeError):
        pickle.dumps(sensing)
    # the figures of the README row
    rms = lambda V: float(np.sqrt(np.mean(np.asarray(sm.H10norm_diff(np.ascontiguousarray(V), np.ascontiguousarray(held))) ** 2)))
    every = np.stack([np.stack([est.coefficients_all[i, j] @ sensing.W[j] for j in range(4)]) for i in rows])
    errs = np.stack([np.asarray(sm.H10norm_diff(np.ascontiguousarray(every[:, j]), np.ascontiguousarray(held))) for j in range(4)], axis=1)
    oracle = float(np.sqrt(np.mean(errs.min(axis=1) ** 2)))
    glob = ReducedBasisPCA()
    glob.build(6, sm, U[100:], a[100:])
    e_glob = rms(np.asarray(glob.state_estimation(sm, points, Y)))
    print(f"label = j* on {np.mean(est.labels == jstar):.2f} of the rows, label = argmin of the true error on "
          f"{np.mean(est.labels == errs.argmin(axis=1)):.2f}; rms H10 error selected {rms(np.asarray(est.states)):.4g}, "
          f"j* {float(np.sqrt(np.mean(err_star ** 2))):.4g}, oracle-best {oracle:.4g}, global basis n = 6 {e_glob:.4g}")
