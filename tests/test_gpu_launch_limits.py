"""Truth tests at every launch split and grid-dimension limit (needs an MI355X).

grid.y and grid.z hold at most 65535 workgroups.  Where a caller's count goes into one of them the host code splits the launch
(the second launch at a base pointer moved on by 65535 items), clamps the grid and strides, or refuses the count.  A mistake
there is a wrong pointer or stride for everything after the first 65535 items: invisible at the shapes of the other files.
Each case below is large in the count only -- the smallest geometry, (1,1)/4: 3 x 3 inner vertices -- and built from 67 base
rows (tests/launch_limits_truth.py, whose generators and checkers tests/test_launch_limits_host.py proves on the CPU, planted
lost offsets included), so the long-double truths cost 67 rows.  NaN rows frame inputs and outputs; every row is checked, rows
0, 65534, 65535, 65536 and the last are named in the messages; every case runs twice and must give the same bits.

The audit: every <<<...>>> site of csrc whose grid takes a caller's count in y or z, or a clamped x with a stride loop over one,
by launcher and kernel.

  rom_spectral.hip launch_left: k_sine_left, snapshots in z, loop at 65535 ........ case 1 here (K = 65537); 22 launches in case 2
  rom_spectral.hip launch_right: loop at 65535 * 64 rows of the product ........... case 2 here
  rom_spectral.hip rom_launch_sine_transform: k_lambda_scale, x clamped, strided .. case 2 here with (pre, post) = (-1, 2)
  rom_ops.hip rom_launch_rows_scale: rows in y, loop at 65535; x clamped at 64 .... case 3 here (dim = 16389 for the x loop)
  rom_ops.hip rom_launch_rows_sign_flip: rows in y, loop at 65535 ................. case 3 here
  rom_nearest.hip k_nn_exhaust: blocks of 16 queries in y, loop at 65535 .......... case 4 here (mode 1)
  rom_nearest.hip k_nn_screen: tables of 128 / 64 queries in y .................... bounded by the cap of 65535 tables per pass
      (`kc` of rom_nearest).  The pass loop is case 4 here; the cap itself takes effect above 65535 * 128 queries and is NOT
      exercised by any case.
  rom_curves.hip kc_galerkin_nested<true>: x = min(M, 65535), stride loop ......... case 5 here (M = 65537)
  rom_curves.hip kc_galerkin_nested<false>: x clamped at 4 per CU, stride loop .... case 5 here (N = 70, M = 2051)
  rom_curves.hip launch_curve: edge tiles in y .................................... bounded by 2 per CU (`ntiles` of rom_error_curves)
  rom_fem_solve.hip enqueue_solve: the systems of a chunk in y, by 64 (k_expand, k_back_pre, k_edge_transform, k_extend,
      k_extend128) and one by one (k_scatter_interface) ........................... bounded by the cap of 65535 systems per
      chunk (`Mc_max` of solve_batch_impl).  Case 5b here runs M = 65537 and asserts the two chunks.  ((1,1)/4 has no
      interface: k_scatter_interface is not launched there; the cap is what bounds it.)
  rom_fem_solve.hip rom_assemble_batch: parameters in y, loop at 65535 ............ already tested in test_gpu_fe_ops.py::
      test_assemble_more_parameters_than_one_grid_dimension
  rom_ops.hip rom_evaluate_points: solutions in y, loop at 65535 .................. already tested in test_gpu_fe_ops.py::
      test_evaluate_points_more_solutions_than_one_grid_dimension
  rom_riesz.hip rom_riesz_h10: kr_spectral (points in y, clamped, strided), the rows of the product (loop at 65535 * 64),
      kr_permute (x clamped, strided) ............................................. already tested in test_gpu_sensor_truth.py::
      test_split_launch_of_the_representer_transform
  rom_ops.hip rom_launch_h10norm: vectors in z .................................... bounded by its K <= 65535 check; already
      tested in test_gpu_fe_ops.py::test_h10norm_refuses_more_rows_than_one_grid_dimension
  rom_ops.hip rom_launch_l2norm, rom_launch_rowdot: vectors in y .................. bounded by their K <= 65535 checks; case 6 here
  rom_ops.hip rom_launch_stencil_apply(_band): vectors in z ....................... bounded by their K <= 65535 checks; case 6 here
  rom_ops.hip rom_launch_stencil_apply_blocks: blocks of the geometry in z ........ at most 64 blocks: not a caller's count
  rom_basis.hip rom_greedy: snapshots in z by GU_SYS .............................. bounded by its M <= 65535 check; case 6 here
  rom_factored.hip rom_greedy_factored ............................................ bounded by its M <= 65535 check; case 6 here
  rom_factored.hip kf_gather_rect: compact coordinates Kc in y .................... bounded by the K <= 65535 check of
      rom_launch_stencil_apply_band, called with Kc just before it
  rom_factored.hip pod_factored: kf_scatter_pivots, modes in y .................... bounded by its n <= 65535 check; case 6 here
  rom_ops.hip rom_launch_gemm_nn, rom_launch_gemm_nt_ex: 64-row tiles of m in y ... row blocks of 65535 * 64; case 7 here.
      (rom_gram and the thin routes put their tiles in x.)
  rom_tree.hip: inputs m in y, trees T in z ....................................... bounded by the m <= 16, T <= 256 checks of rom_tree_fit
  rom_poly.hip k_poly_predict: target-column groups of 96 in y .................... bounded by the q <= 1024 check of rom_poly_fit
  rom_pca_tall.hip k_syrk_tn: chunks of the slab plan in y ........................ at most one per CU (rom_slab_plan); the rotation
      product is bounded by the M <= 65535 * 64 check of rom_pca_tall
  rom_sensors.hip k_eval_points: basis rows n in y ................................ bounded by the n <= 128 check of rom_sensor_greedy
  rom_pod.hip kp_scale_eigvec_rows, kb_rows_axpy, kb_next_block: the width of an eigenvector / sketch block in y: chosen by the
      driver, not a caller's count

The MI355X runtime launches grids with y > 65535; other HIP runtimes this project has run on refuse them (the regressions that
test_assemble_more_parameters_... and test_evaluate_points_more_solutions_... pin).  The loops and caps above make the entry
points independent of that.  (Where a runtime does refuse the first launch of rom_launch_rows_sign_flip, the unsplit code went
on to k_rows_sign_pivots, a 1-D grid, which read candidate positions from a scratch block nobody had written.)
"""
import numpy as np
import pytest

from conftest import observed
from oracle import rom_oracle as ro
import fe_truth as ft
import h10_truth as ht
import launch_limits_truth as lt

pytestmark = pytest.mark.gpu

LIMIT = lt.LIMIT
WS_DEFAULT = 24 << 30
_SM = {}


@pytest.fixture(scope="module")
def ctx():
    from romhighcontrast_amd import _ffi
    return _ffi.get_context()


def _sm(blocks, N):
    from src.lib import SolutionsManagers as SM
    if (blocks, N) not in _SM:
        _SM[(blocks, N)] = SM.SolutionsManagerFEM(blocks, N)
    return _SM[(blocks, N)]


def _framed(X, before, after=2):
    X = np.asarray(X, dtype=np.float64).reshape(len(X), -1)
    return np.vstack((np.full((before, X.shape[1]), np.nan), X, np.full((after, X.shape[1]), np.nan)))


def _same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


def _still_usable(ctx):
    """After a refused or failed call the context takes the next small call and computes it right."""
    X = np.arange(12.0).reshape(4, 3) - 5.0
    Xd = ctx.upload(X)
    ctx.rows_scale(Xd, 2, 3, [2.0, -0.5], row0=1)
    want = X.copy()
    want[1:3] *= np.array([2.0, -0.5])[:, None]
    assert _same_bits(Xd.download(shape=X.shape), want), "the context is not usable after a failed call"


def _call(ctx, what, fn, *args, **kw):
    """fn(*args): a library error on a legal count fails the test -- after showing that the context survived it."""
    from romhighcontrast_amd import _ffi
    try:
        return fn(*args, **kw)
    except _ffi.RomLibraryError as e:
        _still_usable(ctx)
        pytest.fail(f"{what}: a legal call fails (the context is usable afterwards): {e}")


# ---- 1, 2. rom_sine_transform past the split of the left factor (snapshots in grid.z) and of the right one -----------------------
def _transform_case(K, pre, post, what):
    sm, gr = _sm(*lt.GEOM), ht.grid(*lt.GEOM)
    ctx, dim = sm._ctx, sm.vspace_dim
    assert (sm.nr_inner_vertices, sm.nc_inner_vertices, dim) == (gr.nr, gr.nc, gr.dim)
    tt = lt.TransformTruth(gr, lt.base_rows(gr.dim, lt.TRANSFORM_SEED), pre, post)
    x0, o0 = 2, 3
    Xs = _framed(lt.rows(tt.base, K), x0)
    Xb = ctx.upload(Xs)

    def run():
        Ob = ctx.alloc((o0 + K + 2) * dim).fill(np.nan)
        _call(ctx, what, sm._fem.sine_transform, Xb, K, Ob, pre=pre, post=post, x_row0=x0, out_row0=o0)
        return Ob

    Ob = run()
    O = Ob.download(shape=(o0 + K + 2, dim))
    assert np.isnan(O[:o0]).all() and np.isnan(O[o0 + K:]).all(), (what, "OUT sentinels")
    lt.check_transform(what, tt, O[o0:o0 + K], observed)
    del O
    assert run().same_bits_as(Ob, Ob.n), (what, "repeat")
    assert Xb.same_bits_as(ctx.upload(Xs), Xb.n), (what, "X modified")


@pytest.mark.parametrize("pre,post", [(0, 1), (-1, 0), (-1, 2)])
def test_sine_transform_more_snapshots_than_one_grid_dimension(pre, post):
    """K = 65537: k_sine_left's second launch (snapshots 65535, 65536) at X + 65535 dim, in both orders of the two factors and
    with the elementwise pass of pre != 0, post != 0."""
    _transform_case(lt.K_BATCH, pre, post, "sine transform, 65537 snapshots")


@pytest.mark.parametrize("pre,post", [(0, 1), (-1, 0), (-1, 2)])
def test_sine_transform_more_rows_than_one_launch_of_the_right_factor(pre, post):
    """K nr just above 65535 * 64 in ONE workspace chunk (the default limit): the right factor's second launch at
    X + 65535 * 64 * nc -- on the input with pre = 0, on the intermediate otherwise -- and 22 launches of the left one.
    (-1, 2): the elementwise pass over more entries than its clamped grid has threads (the stride loop of k_lambda_scale)."""
    gr = ht.grid(*lt.GEOM)
    K = lt.right_count(gr.nr)
    assert K * gr.nr > lt.RIGHT_ROWS and K * gr.dim * 8 < WS_DEFAULT
    _transform_case(K, pre, post, f"sine transform, {K} snapshots = {K * gr.nr} rows of the right factor")


# ---- 3. rom_rows_scale, rom_rows_sign_flip: rows in grid.y ---------------------------------------------------------------------
@pytest.mark.parametrize("rows,dim", [(r, d) for r in (LIMIT, LIMIT + 1, LIMIT + 2) for d in (3, 17)] + [(3, 64 * 256 + 5)])
def test_rows_scale_around_one_grid_dimension(ctx, rows, dim):
    """One rounding per entry: the fp64 product, bit for bit, on every row.  (3 rows of 16389 columns: the stride loop over
    the columns, whose grid is clamped at 64 workgroups.)"""
    X, fac, want = lt.scale_case(rows, dim)
    host = _framed(X, 2)
    got = []
    for _ in range(2):
        Xd = ctx.upload(host)
        _call(ctx, f"rom_rows_scale, {rows} rows", ctx.rows_scale, Xd, rows, dim, fac, row0=2)
        got.append(Xd.download(shape=host.shape))
    assert np.isnan(got[0][:2]).all() and np.isnan(got[0][2 + rows:]).all(), "sentinels"
    lt.check_exact(f"rows_scale rows={rows} dim={dim}", got[0][2:2 + rows], want)
    assert _same_bits(got[0], got[1]), "repeat"


@pytest.mark.parametrize("dim", [3, 17])
@pytest.mark.parametrize("rows", [LIMIT, LIMIT + 1, LIMIT + 2])
def test_rows_sign_flip_around_one_grid_dimension(ctx, rows, dim):
    """NumPy's svd_flip rule (first maximum on ties), bit for bit, on every row; ties, zero rows and negative last maxima
    recur through the block."""
    X, want = lt.sign_case(rows, dim)
    host = _framed(X, 2)
    got = []
    for _ in range(2):
        Xd = ctx.upload(host)
        _call(ctx, f"rom_rows_sign_flip, {rows} rows", ctx.rows_sign_flip, Xd, rows, dim, row0=2)
        got.append(Xd.download(shape=host.shape))
    assert np.isnan(got[0][:2]).all() and np.isnan(got[0][2 + rows:]).all(), "sentinels"
    lt.check_exact(f"rows_sign_flip rows={rows} dim={dim}", got[0][2:2 + rows], want)
    assert _same_bits(got[0], got[1]), "repeat"


# ---- 4. rom_nearest: query blocks of the exhaustive scan in grid.y ------------------------------------------------------------------
class Block:
    """rows x r values from column `col` of rows [1, 1 + rows) of a NaN block with `extra` more columns
    (tests/test_gpu_nearest.py)."""

    def __init__(self, ctx, X, col, extra):
        rows, r = X.shape
        self.ld = r + extra
        self.off = self.ld + col
        self.host = np.full((rows + 2, self.ld), np.nan)
        self.host[1:1 + rows, col:col + r] = X
        self.buf = ctx.upload(self.host)

    def unchanged(self):
        return _same_bits(self.buf.download(shape=self.host.shape), self.host)


@pytest.mark.parametrize("r,t", [(1, 1), (1, 3), (5, 1), (5, 3)])
def test_nearest_more_query_blocks_than_one_grid_dimension(ctx, r, t):
    """K = 65535 * 16 + 17 queries against 40 library rows: the exhaustive scan (mode 1) needs 65537 blocks of 16 queries; the
    screened search (mode 0) in one pass and, under a workspace limit, in five.  All with the bits of mode 1.
    "Every row is checked" here means: nearest_truth.check_neighbours on three windows of 871 queries (the first cycle, the one
    across query 65535 * 16, the last), and every other query bit for bit against its twin in the first cycle -- which rests
    on rom_nearest's documented reproducibility: the same query against the same library gives the same bits in whichever
    workgroup, launch or pass it lands."""
    Q, base = lt.nearest_case(r)
    K, M = lt.NN_K, len(Q)
    qb, pb = Block(ctx, Q, 2, 5), Block(ctx, lt.rows(base, K), 1, 3)

    def search(mode, what):
        idx, d2, info = _call(ctx, f"rom_nearest mode {mode}, {K} queries{what}", ctx.nearest, qb.buf, qb.off, qb.ld, M, pb.buf,
                              pb.off, pb.ld, K, r, t=t, mode=mode)
        assert info["certified"] + info["fallbacks"] == K, info
        lt.check_nearest(f"nearest r={r} t={t} mode {mode}{what}", base, Q, idx, d2, t)
        return idx, d2, info

    idx1, d1, info1 = search(1, "")
    assert info1["certified"] == 0 and info1["fallbacks"] == K and info1["groups_rescored"] == 0, info1
    again = ctx.nearest(qb.buf, qb.off, qb.ld, M, pb.buf, pb.off, pb.ld, K, r, t=t, mode=1)
    assert np.array_equal(again[0], idx1) and _same_bits(again[1], d1), "repeat"
    idx0, d0, info0 = search(0, "")
    assert np.array_equal(idx0, idx1) and _same_bits(d0, d1), np.argwhere(idx0 != idx1)[:4]
    ctx.set_workspace_limit(32 << 20)          # tables of 16 slots per query: 262144 queries per pass
    try:
        idxp, dp, infop = search(0, ", five passes")
    finally:
        ctx.set_workspace_limit(WS_DEFAULT)
    assert infop["launches"] - info0["launches"] == 2 * 4, (info0, infop)
    assert np.array_equal(idxp, idx1) and _same_bits(dp, d1), np.argwhere(idxp != idx1)[:4]
    assert qb.unchanged() and pb.unchanged()


# ---- 5. rom_error_curves: the strided second trip of the Galerkin LDS route --------------------------------------------------------
CURVES = [(lt.GEOM, 2, lt.CURVES_M, True), (lt.GEOM, 2, lt.CURVES_M, False), (lt.GEOM, 9, lt.CURVES_M, True),
          (lt.GEOM, 9, lt.CURVES_M, False), (((1, 3), 8), 70, 2051, True)]


@pytest.mark.parametrize("geom,N,M,with_a", CURVES, ids=[f"N{c[1]}_M{c[2]}_{'galerkin' if c[3] else 'projection'}" for c in CURVES])
def test_error_curves_more_snapshots_than_the_clamped_grid(ctx, geom, N, M, with_a):
    """M = 65537 snapshots (67 distinct ones, each with its own parameter): kc_galerkin_nested<true> runs on 65535 workgroups and
    two of them take a second snapshot; the curve passes, the products and the transposes see M as well.  N = 70 on (1,3)/8:
    the global-memory route, whose grid is clamped at four workgroups per CU, with M = 2051 snapshots."""
    blocks, Nm = geom
    sm, g = _sm(blocks, Nm), ro.Geometry(blocks, Nm)
    dim = sm.vspace_dim
    a, Cr = lt.curves_inputs(blocks, dim, N)
    U = sm.generate_solutions(a)
    b = np.arange(M) % lt.PERIOD
    Ub, Cb = ctx.upload(_framed(U[b], 1)), ctx.upload(_framed(Cr, 2))
    ab = ctx.upload(np.ascontiguousarray(a.reshape(lt.PERIOD, -1)[b])) if with_a else None
    what = f"error curves M={M} N={N} {'with' if with_a else 'without'} parameters"
    proj, galc, P, T, info = _call(ctx, what, sm._fem.error_curves, Ub, M, Cb, N, ab, u_row0=1, c_row0=2)
    assert info["galerkin_route"] == (("lds" if N <= 64 else "global") if with_a else None), info
    dead = np.diag(T) == 0.0
    assert info["dependent_rows"] == dead.sum() == 0, info
    tr = lt.CurvesTruth(g, U, Cr, a if with_a else None, 10.0 ** lt.CURVES_DECADES, dead)
    lt.check_curves(what, tr, proj, galc, P, observed)
    r2 = sm._fem.error_curves(Ub, M, Cb, N, ab, u_row0=1, c_row0=2)
    for x, y in zip((proj, galc, P, T), r2[:4]):
        assert (x is None and y is None) or _same_bits(x, y), (what, "repeat")


# ---- 5b. the snapshot sweep: the systems of one chunk in grid.y -------------------------------------------------------------------------
def test_sweep_more_systems_than_one_grid_dimension(ctx):
    """M = 65537 parameters (67 distinct ones): the sweep takes at most 65535 systems per chunk (their count is a grid dimension
    of its expansion and scatter kernels), so this one runs as 65535 + 2 -- asserted from the profile: k_coef once per chunk.
    Every snapshot within the project's snapshot bound (sweep_truth.SNAP_TOL, relative H^1_0) of the oracle's solution of
    its parameter."""
    import sweep_truth as swt
    blocks, Nm = lt.GEOM
    sm, g = _sm(blocks, Nm), ro.Geometry(blocks, Nm)
    a = lt.curves_inputs(blocks, sm.vspace_dim, 1)[0]
    ref = ro.generate_solutions(g, a, "lsqsparse")
    for M, chunks in ((LIMIT, 1), (LIMIT + 2, 2)):
        b = np.arange(M) % lt.PERIOD
        ctx.profile_reset()
        ctx.profile(True)
        try:
            U = sm.generate_solutions(a[b])
            prof = ctx.profile_report()
        finally:
            ctx.profile(False)
        assert prof.get("coef", {}).get("launches") == chunks, (M, {k: v["launches"] for k, v in prof.items()})
        assert U.shape == (M, sm.vspace_dim)
        err = ro.H10norm(g, U - ref[b]) / ro.H10norm(g, ref)[b]
        lt.check_ratios(f"sweep M={M} on (1,1)/4: relative H10 error vs the oracle / {swt.SNAP_TOL:g}", err / swt.SNAP_TOL, observed)
        assert _same_bits(sm.generate_solutions(a[b]), U), "repeat"


# ---- 6. refusals, and the largest count that is taken -----------------------------------------------------------------------------------
def _refused(ctx, st):
    from romhighcontrast_amd import _ffi
    msg = ctx.lib.rom_last_error()
    assert st == _ffi.ROM_ERR_INVALID and b"65535" in msg, (st, msg)
    _still_usable(ctx)


def test_l2norm_refuses_more_rows_than_one_grid_dimension(ctx):
    """K = 65536: ROM_ERR_INVALID with the limit in the message.  K = 65535 integer rows times powers of two: every sum of
    squares is exact, every norm its square root to one ulp."""
    dim = 3
    base = np.random.default_rng(3).integers(-1000, 1001, size=(lt.PERIOD, dim)).astype(np.float64)
    Ub = ctx.upload(lt.rows(base, LIMIT + 1))
    out = np.zeros(LIMIT + 1)
    _refused(ctx, ctx.lib.rom_l2norm(ctx.h, Ub.h, 0, LIMIT + 1, dim, out.ctypes.data))
    got = ctx.l2norm(Ub, 0, LIMIT, dim)
    S = [int(v) for v in (base.astype(np.int64) ** 2).sum(axis=1)]
    unscaled = got / lt.pow2(np.arange(LIMIT))
    ok = np.array([ft.sqrt_ulps_ok(unscaled[i], S[i % lt.PERIOD]) for i in range(lt.CYCLE)])
    assert ok.all(), np.flatnonzero(~ok)[:5]
    lt.check_exact("l2norm K=65535 against the first cycle", unscaled[:, None], unscaled[:lt.CYCLE][np.arange(LIMIT) % lt.CYCLE][:, None])
    assert _same_bits(ctx.l2norm(Ub, 0, LIMIT, dim), got), "repeat"


@pytest.mark.parametrize("unit", [True, False], ids=["unit", "blocks"])
def test_stencil_apply_refuses_more_rows_than_one_grid_dimension(ctx, unit):
    """K = 65536 is refused; K = 65535 (vectors in grid.z) equals the integer product on every row (fe_truth: exact)."""
    from romhighcontrast_amd import _ffi
    blocks, Nm = lt.GEOM
    fem = _ffi.Fem(ctx, blocks[0], blocks[1], Nm)
    a, Xi, Yi = ft.exact_stencil_case(blocks, Nm, lt.PERIOD, seed=11 + unit, unit=unit)
    assert not np.array_equal(Yi[9], Yi[0]) and not np.array_equal(Yi[10], Yi[0])
    X = lt.rows(Xi, LIMIT + 1)
    Xb = ctx.upload(_framed(X, 1))
    Yb = ctx.alloc((2 + LIMIT + 1 + 2) * fem.dim).fill(np.nan)
    a_host = None if unit else np.ascontiguousarray(a.ravel())
    _refused(ctx, ctx.lib.rom_stencil_apply(fem.h, None if unit else a_host.ctypes.data, 1 if unit else 0, Xb.h, 1, LIMIT + 1, Yb.h, 2))
    assert np.isnan(Yb.download()).all(), "a refused call wrote"
    want = lt.rows(Yi, LIMIT)
    for rep in range(2):
        Yb.fill(np.nan)
        fem.stencil_apply(Xb, LIMIT, Yb, a_one=None if unit else a.ravel(), x_row0=1, y_row0=2)
        Y = Yb.download(shape=(2 + LIMIT + 3, fem.dim))
        assert np.isnan(Y[:2]).all() and np.isnan(Y[2 + LIMIT:]).all(), "sentinels"
        lt.check_exact(f"stencil_apply K=65535 unit={unit} run {rep}", Y[2:2 + LIMIT], want)


def test_greedy_refuses_more_rows_than_one_grid_dimension(ctx):
    """M = 65536 is refused.  M = 65535, n = 3 on 67 distinct rows: the picks are those of the 80-bit greedy, each the lowest
    index among its equal rows; the curve within the bound model of tests/test_gpu_greedy_routes.py."""
    blocks, Nm = lt.GEOM
    sm, g = _sm(blocks, Nm), ro.Geometry(blocks, Nm)
    fem, n = sm._fem, lt.GREEDY_N
    U, h1 = lt.greedy_inputs(sm.vspace_dim, 1)
    b = np.arange(LIMIT + 1) % lt.PERIOD
    Ub = ctx.upload(_framed(U[b], 1))
    h1M = np.ascontiguousarray(h1[b])
    picks, errs = np.zeros(n, dtype=np.int64), np.zeros(n)
    _refused(ctx, ctx.lib.rom_greedy(fem.h, Ub.h, 1, LIMIT + 1, None, h1M.ctypes.data, 0, n, picks.ctypes.data, errs.ctypes.data))
    truth = lt.greedy_truth(g, U, h1, n)
    got = fem.greedy(Ub, LIMIT, None, h1M[:LIMIT], False, n, u_row0=1)
    lt.check_greedy("greedy rows M=65535", truth, got[0], got[1], observed)
    again = fem.greedy(Ub, LIMIT, None, h1M[:LIMIT], False, n, u_row0=1)
    assert again[0] == got[0] and _same_bits(again[1], got[1]), "repeat"


def test_greedy_factored_refuses_more_rows_than_one_grid_dimension(ctx):
    """The same on the compact interface vectors of (2,2)/16, the smallest geometry the greedy tests use for the factored route:
    67 random interface vectors, the bound with the energy map's own term (tests/test_gpu_greedy_routes.py)."""
    from romhighcontrast_amd import factored
    blocks, Nm = (2, 2), 16
    sm, g = _sm(blocks, Nm), ro.Geometry(blocks, Nm)
    fem, n = sm._fem, lt.GREEDY_N
    assert fem.expansion_is_linear
    Y = ctx.upload(np.random.default_rng(2).standard_normal((lt.PERIOD, fem.reduced_stride)))
    fs = factored.FactoredSnapshots(sm, Y, lt.PERIOD)
    Kc = fs.map.Kc
    U, Ych = fs.rows().numpy(), fs.Yc.download(lt.PERIOD * Kc, shape=(lt.PERIOD, Kc))
    h1 = lt.greedy_inputs(4, 2)[1]
    k1, _ = fs.map.build()
    em = factored.expansion_map(sm)
    Bt = ctx.alloc(Kc * em.dim)
    em.expand_compact(ctx.upload(np.eye(Kc)), Kc, Bt)
    scale2 = float(np.max((Ych ** 2 @ fem.h10norm(Bt, Kc) ** 2) / h1 ** 2))
    map_delta = (lt.C_GREEDY * Kc * lt.EPS + max(Kc - k1, 0) * 1e-14) * scale2
    b = np.arange(LIMIT + 1) % lt.PERIOD
    Yb = ctx.upload(_framed(Ych[b], 1))
    h1M = np.ascontiguousarray(h1[b])
    picks, errs = np.zeros(n, dtype=np.int64), np.zeros(n)
    _refused(ctx, ctx.lib.rom_greedy_factored(fem.h, Yb.h, 1, LIMIT + 1, None, h1M.ctypes.data, 0, n, picks.ctypes.data,
                                             errs.ctypes.data))
    truth = lt.greedy_truth(g, U, h1, n, map_delta)
    got = fem.greedy_factored(Yb, LIMIT, None, h1M[:LIMIT], False, n, c_row0=1)
    lt.check_greedy("greedy factored M=65535", truth, got[0], got[1], observed)
    again = fem.greedy_factored(Yb, LIMIT, None, h1M[:LIMIT], False, n, c_row0=1)
    assert again[0] == got[0] and _same_bits(again[1], got[1]), "repeat"


def test_pod_factored_refuses_more_modes_than_one_grid_dimension(ctx):
    """n = 65536 modes (kf_scatter_pivots takes them in grid.y) are refused by both factored PODs, with the limit in the message."""
    sm = _sm((2, 2), 16)
    fem = sm._fem
    Yb, Vb, sig, info = ctx.alloc(16), ctx.alloc(16), np.zeros(LIMIT + 1), np.zeros(8)
    _refused(ctx, ctx.lib.rom_pod_factored(fem.h, Yb.h, 0, 4, LIMIT + 1, 1, Vb.h, 0, sig.ctypes.data, info.ctypes.data))
    _refused(ctx, ctx.lib.rom_pod_h10_factored(fem.h, Yb.h, 0, 4, LIMIT + 1, 1, Vb.h, 0, sig.ctypes.data, info.ctypes.data))


# ---- 7. the dense products: 64-row tiles of m in grid.y ---------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["nn", "nt"])
@pytest.mark.parametrize("m", [lt.RIGHT_ROWS, lt.RIGHT_ROWS + 1])
def test_gemm_more_row_tiles_than_one_grid_dimension(ctx, which, m):
    """m = 65535 * 64 and one more row, n = k = 1: C = A b is ONE rounding per entry, so every row equals the fp64 product bit for
    bit; the row past the limit belongs to a second row block at A + 65535 * 64 lda.  NaN frames, beta = 0 over NaN in C."""
    A = lt.rows(lt.base_rows(1, seed=31), m)
    bval = 1.0 / 3.0
    host = _framed(A, 2)
    Ab, Bb = ctx.upload(host), ctx.upload(np.array([np.nan, bval, np.nan]))
    gemm = ctx.gemm_nn if which == "nn" else ctx.gemm_nt
    got = []
    for _ in range(2):
        Cb = ctx.alloc(m + 4).fill(np.nan)
        _call(ctx, f"rom_gemm_{which}, m = {m}", gemm, m, 1, 1, Ab, 2, 1, Bb, 1, 1, Cb, 2, 1)
        got.append(Cb.download())
    assert np.isnan(got[0][:2]).all() and np.isnan(got[0][2 + m:]).all(), "sentinels"
    lt.check_exact(f"gemm_{which} m={m}", got[0][2:2 + m, None], A * bval)
    assert _same_bits(got[0], got[1]), "repeat"
    assert Ab.same_bits_as(ctx.upload(host), Ab.n), "A modified"
