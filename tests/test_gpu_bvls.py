"""rom_bvls on the GPU against bvls_host and the Karush-Kuhn-Tucker checker of tests/bvls_truth.py.

Every call runs on NaN-framed operands -- P and OUT as column ranges of wider NaN blocks from an offset, G_r and AUX with a NaN
tail -- which must come back bit for bit (OUT: everything outside its rows); every call is made twice and must return the same
bits; every converged result goes through check_kkt.  Device against host: |c_dev - c_host| <= max(1e3 delta, 1e-11 (1 + max|c|))
with delta the host's own change when the rows of G are permuted, equal pass counts, and equal ``bound`` wherever
|g_j| > 1e3 tol_j."""
import numpy as np
import pytest

import bvls_truth as bt
from bvls_truth import IDS, SHAPES

pytestmark = pytest.mark.gpu


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


def run(ctx, G, P, lo, hi, aux=None, max_iter=None, check=True):
    """rom_bvls twice on NaN-framed operands; returns (BvlsResult, info)."""
    r, n = G.shape
    P = np.atleast_2d(P)
    K = len(P)
    ldp, p_off, ldo, o_off = r + 3, r + 3 + 1, n + 4 + 2, 3
    ph = np.full((K + 2, ldp), np.nan)
    ph[1:1 + K, 1:1 + r] = P
    ops = [Tail(ctx, G), Tail(ctx, ph)]
    auxb = Tail(ctx, aux) if aux is not None else None
    outs = []
    for _ in range(2):
        OUT = ctx.upload(np.full(o_off + K * ldo + 4, np.nan))
        res, info = ctx.bvls(n, r, ops[0].buf, ops[1].buf, p_off, ldp, K, lo, hi, AUX=auxb.buf if auxb else None, max_iter=max_iter,
                             OUT=OUT, out_off=o_off, ldo=ldo)
        raw = OUT.download()
        body = raw[o_off:o_off + K * ldo].reshape(K, ldo)
        assert np.isnan(raw[:o_off]).all() and np.isnan(raw[o_off + K * ldo:]).all() and np.isnan(body[:, n + 4:]).all(), "OUT's frame"
        assert not np.isnan(body[:, :n + 4]).any()
        outs.append((raw, res, info))
    for op in ops + ([auxb] if auxb else []):
        assert op.unchanged(), "an input buffer was modified"
    assert np.array_equal(_bits(outs[0][0]), _bits(outs[1][0])), "two calls, different bits"
    assert np.array_equal(outs[0][1].bound, outs[1][1].bound)
    res, info = outs[0][1], outs[0][2]
    limit = 5 * n + 10 if max_iter is None else max_iter
    assert info["launches"] == 2 and info["host_syncs"] == 1 and info["systems"] == K, info
    assert info["workspace_bytes"] == 8 * (n * n + 2), info
    assert info["passes"] == res.iterations.sum() <= limit * K and info["factorisations"] == info["passes"] + K, info
    assert np.array_equal(info["bound_variables"], (res.bound != 0).sum(axis=1))
    if check:
        worst = bt.check_kkt(G, P, lo, hi, res, aux=aux)
        print(f"check_kkt: kkt / bound {worst[0]:.3g}, misfit / bound {worst[1]:.3g}; passes {info['passes']}, up to {res.iterations.max()}")
    return res, info


@pytest.fixture(scope="module")
def cases():
    from romhighcontrast_amd.inverse import bvls_host
    out = {}
    for shape in SHAPES:
        G, P, lo, hi = bt.case(*shape)
        host = bvls_host(G, P, lo, hi)
        out[shape] = (G, P, lo, hi, host, bt.permuted_delta(G, P, lo, hi, host))
    return out


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_solves_and_follows_the_host(ctx, cases, shape):
    G, P, lo, hi, host, delta = cases[shape]
    res, _ = run(ctx, G, P, lo, hi)
    assert res.converged.all(), np.flatnonzero(~res.converged)
    bound = bt.host_bound(delta, host.c)
    diff = np.abs(res.c - host.c).max(axis=1)
    print(f"device - host up to {diff.max():.3g}, host - permuted host up to {delta.max():.3g}, largest ratio to the bound "
          f"{(diff / bound).max():.3g}; {int((res.bound != 0).sum())} bound variables")
    assert (diff <= bound).all(), (diff / bound).max()
    assert np.array_equal(res.iterations, host.iterations), np.flatnonzero(res.iterations != host.iterations)
    g, tol = bt.kkt_tolerance(G, P, host.c)
    clear = np.abs(g) > 1e3 * tol
    assert np.array_equal(res.bound[clear], host.bound[clear])
    rel = np.abs(res.misfit - host.misfit) / host.misfit
    assert (rel <= 1e-12).all(), rel.max()


@pytest.mark.parametrize("shape", [(4, 6, 5), (64, 96, 6)], ids=["4x6x5", "64x96x6"])
def test_max_iter_zero_and_a_few_passes(ctx, cases, shape):
    from romhighcontrast_amd.inverse import bvls_host
    G, P, lo, hi, _, _ = cases[shape]
    free = bvls_host(G, P, -np.inf, np.inf).c
    res, info = run(ctx, G, P, lo, hi, max_iter=0, check=False)
    # the clipped start: the device's own unconstrained solution differs from the host's by rounding, the clipped entries do not
    host0 = bvls_host(G, P, lo, hi, max_iter=0)
    away = np.minimum(np.abs(free - lo), np.abs(free - hi)) > 1e-9
    assert np.array_equal(res.bound[away], host0.bound[away])
    assert np.array_equal(_bits(res.c[host0.bound != 0]), _bits(host0.c[host0.bound != 0]))
    np.testing.assert_allclose(res.c, host0.c, rtol=0, atol=1e-11)
    assert (res.iterations == 0).all() and not res.converged.any() and info["passes"] == 0
    for max_iter in (1, 3):
        res, _ = run(ctx, G, P, lo, hi, max_iter=max_iter, check=False)
        host = bvls_host(G, P, lo, hi, max_iter=max_iter)
        bound = bt.host_bound(bt.permuted_delta(G, P, lo, hi, host, max_iter=max_iter), host.c)
        assert np.array_equal(res.iterations, host.iterations) and np.array_equal(res.converged, host.converged)
        assert (np.abs(res.c - host.c).max(axis=1) <= bound).all()
        assert ((res.c >= lo) & (res.c <= hi)).all()


def test_pinned_infinite_and_aux(ctx, cases):
    from romhighcontrast_amd.inverse import bvls_host
    G, P, lo, hi, _, _ = cases[(16, 20, 5)]
    lo, hi = lo.copy(), hi.copy()
    lo[3] = hi[3] = 0.1234567890123
    lo[5], hi[5] = -np.inf, np.inf
    lo[7] = -np.inf
    hi[9] = np.inf
    aux = np.stack([np.arange(1.0, 6.0), np.ones(5)], axis=1)
    res, _ = run(ctx, G, P, lo, hi, aux=aux)
    host = bvls_host(G, P, lo, hi, aux=aux)
    assert res.converged.all() and np.array_equal(res.iterations, host.iterations) and np.array_equal(res.bound, host.bound)
    assert np.array_equal(_bits(res.c[:, 3]), _bits(np.full(5, 0.1234567890123))) and (res.bound[:, 3] == -1).all()
    assert (res.bound[:, 5] == 0).all()
    np.testing.assert_allclose(res.misfit, host.misfit, rtol=1e-13)
    res, _ = run(ctx, G, P, lo[3], lo[3])   # nothing free
    assert np.array_equal(_bits(res.c), _bits(np.full((5, 16), lo[3]))) and res.converged.all() and (res.iterations == 1).all()
    res, _ = run(ctx, G, P, -1e3, 1e3)      # nothing bound: the least squares
    ref = np.linalg.lstsq(G, P.T, rcond=None)[0].T
    assert (res.bound == 0).all() and (res.iterations == 1).all()
    np.testing.assert_allclose(res.c, ref, rtol=0, atol=1e-12 * np.abs(ref).max() * np.linalg.cond(G))


def test_errors(ctx):
    from romhighcontrast_amd._ffi import RomLibraryError
    G, P, lo, hi = bt.case(4, 6, 5)
    up = ctx.upload
    big, p = up(np.zeros(97 * 65)), up(np.zeros((2, 97)))
    one = np.ones(65)
    for (n, r, ldo, l, h), word in (((65, 70, 80, -one, one), "n = 65"), ((4, 97, 80, -one, one), "r = 97"), ((6, 4, 80, -one, one), "r = 4"),
                                    ((4, 6, 7, -one, one), "ldo"), ((4, 6, 80, one, -one), "lo <= hi"),
                                    ((4, 6, 80, -one, one * np.nan), "lo <= hi")):
        OUT = up(np.full(400, np.nan))
        with pytest.raises(RomLibraryError, match=word) as e:
            ctx.bvls(n, r, big, p, 0, 97, 2, l[:n], h[:n], OUT=OUT, ldo=ldo)
        assert "error 1" in str(e.value)   # ROM_ERR_INVALID
        assert np.isnan(OUT.download()).all(), "OUT was written"
    # K = 0 is a no-op
    res, info = ctx.bvls(4, 6, up(G), None, 0, 6, 0, lo, hi)
    assert res.c.shape == (0, 4) and res.bound.shape == (0, 4) and info["launches"] == 0 and info["host_syncs"] == 0
    # NaN in P: reported once
    bad = P.copy()
    bad[1, 2] = np.nan
    with pytest.raises(RomLibraryError, match="NaN / Inf") as e:
        ctx.bvls(4, 6, up(G), up(bad), 0, 6, 5, lo, hi)
    assert "error 1" in str(e.value)
    res, _ = ctx.bvls(4, 6, up(G), up(P), 0, 6, 5, lo, hi)
    bt.check_kkt(G, P, lo, hi, res)
    # NaN in Gr, and a Gr without full column rank
    Gn = G.copy()
    Gn[5, 3] = np.inf
    with pytest.raises(RomLibraryError, match="NaN / Inf"):
        ctx.bvls(4, 6, up(Gn), up(P), 0, 6, 5, lo, hi)
    with pytest.raises(RomLibraryError, match="rank"):
        ctx.bvls(4, 6, up(np.c_[G[:, :3], np.zeros(6)]), up(P), 0, 6, 5, lo, hi)
    res, _ = ctx.bvls(4, 6, up(G), up(P), 0, 6, 5, lo, hi, bound=False)
    assert res.bound is None and np.isfinite(res.c).all()


@pytest.fixture(scope="module")
def experiment(ctx):
    """(2, 2) blocks, N = 5: 600 parameters a ~ U(1, 100) (seed 42), rows 100.. training, rows 0..99 held out, snapshots from the
    device; the basis: the leading right singular vectors of the uncentred training block (NumPy SVD); sensors at interior
    vertices chosen with default_rng(3); Gaussian noise from default_rng(5)."""
    from romhighcontrast_amd.lib.ReducedBasis import BaseReducedBasis
    from romhighcontrast_amd.lib.SolutionsManagers import SolutionsManagerFEM
    sm = SolutionsManagerFEM(blocks_geometry=(2, 2), N=5)
    a = np.random.default_rng(42).uniform(1.0, 100.0, size=(600, 2, 2))
    U = np.asarray(sm.generate_solutions(a))
    Vt = np.linalg.svd(U[100:], full_matrices=False)[2]
    X, Yg = np.meshgrid(sm.points_c[1:-1], sm.points_r[1:-1])
    verts = np.c_[X.ravel(), Yg.ravel()]

    def setup(n, m, sigma):
        rb = BaseReducedBasis()
        rb.set(np.ascontiguousarray(Vt[:n]), a[100:100 + n])
        points = verts[np.random.default_rng(3).choice(len(verts), m, replace=False)]
        Y = np.asarray(sm.evaluate_solutions(points, U[:100]))
        Y = Y + sigma * np.random.default_rng(5).standard_normal(Y.shape)
        return rb, points, Y, rb.coefficient_bounds(sm, U[100:], inflate=0.0)

    return sm, U, setup


@pytest.mark.parametrize("n,m", [(16, 20), (12, 14)], ids=["16x20", "12x14"])
def test_end_to_end_the_box_survives_noise(ctx, experiment, n, m):
    """Noise 1e-3 on the measurements of the 100 held-out states: the rms H^1_0 error of the box-constrained estimates is at
    most half that of the plain least squares, for state_estimation and for state_estimation_pbdw; the device and device=False
    paths agree to the permuted-host bound.  (Oracle + scipy: 0.0107 against 0.132 at (16, 20), 0.0637 against 553 at (12, 14).)
    Measured on an MI355X: (16, 20) plain 0.1321, box 0.01068 on both paths, PBDW 0.1333 -> 0.01241, device - host 2.1e-17;
    (12, 14) plain 553.1, box 0.06494 on both paths, PBDW 549.3 -> 0.06666, device - host 7.6e-16 at cond(G_r) = 4.9e5."""
    from romhighcontrast_amd.inverse import bvls_host, reduce_measurements, reduce_sensors
    sm, U, setup = experiment
    rb, points, Y, box = setup(n, m, 1e-3)
    rms = lambda V: float(np.sqrt(np.mean(np.asarray(sm.H10norm(np.ascontiguousarray(V - U[:100]))) ** 2)))
    plain = rb.state_estimation(sm, points, Y)
    c_dev, boxed = rb.state_estimation(sm, points, Y, return_coefs=True, bounds=box)
    c_host, boxed_host = rb.state_estimation(sm, points, Y, return_coefs=True, bounds=box, device=False)
    e_plain, e_box, e_host = rms(plain), rms(boxed), rms(boxed_host)
    e_proj = rms(np.asarray(rb.projection(sm, U[:100])))
    pb_plain = rb.state_estimation_pbdw(sm, points, Y)
    pb_box = rb.state_estimation_pbdw(sm, points, Y, bounds=box)
    e_pb_plain, e_pb_box = rms(pb_plain), rms(pb_box)
    print(f"n = {n}, m = {m}: rms H10 error plain {e_plain:.4g}, box {e_box:.4g} (host path {e_host:.4g}), projection {e_proj:.3g}; "
          f"PBDW plain {e_pb_plain:.4g}, box {e_pb_box:.4g}")
    assert ((c_dev >= box[0][:, None]) & (c_dev <= box[1][:, None])).all()
    assert e_box <= 0.5 * e_plain and e_host <= 0.5 * e_plain, (e_box, e_host, e_plain)
    assert e_pb_box <= 0.5 * e_pb_plain, (e_pb_box, e_pb_plain)
    # the PBDW estimate still interpolates the (noisy) measurements
    at = np.asarray(sm.evaluate_solutions(points, pb_box))
    assert np.abs(at - Y).max() <= 1e-8 * max(1.0, np.abs(pb_box).max())
    # device against host, in the reduced coordinates both work in
    E = sm.evaluate_solutions(points, rb.basis)
    Ur, Gr, _ = reduce_sensors(E)
    Pq, aux = reduce_measurements(Ur, Y, np.ones(m))
    host = bvls_host(Gr, Pq, box[0], box[1], aux=aux)
    assert np.array_equal(host.c.T, c_host)
    bound = bt.host_bound(bt.permuted_delta(Gr, Pq, box[0], box[1], host, aux=aux), host.c)
    diff = np.abs(c_dev.T - host.c).max(axis=1)
    print(f"device - host up to {diff.max():.3g}, largest ratio to the bound {(diff / bound).max():.3g}; cond(G_r) {np.linalg.cond(Gr):.3g}")
    assert (diff <= bound).all(), (diff / bound).max()
