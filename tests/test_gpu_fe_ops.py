"""The FE-operator layer under the greedy, the error curves and the projectors -- rom_assemble_batch, rom_stencil_apply,
rom_h10norm, rom_evaluate_points, rom_reduced_solve_batch, rom_project_h10, rom_galerkin_rom, rom_orthonormalize_rows --
against truths that do not share its rounding (tests/fe_truth.py, proved on the CPU by tests/test_fe_truth_host.py).  Needs
an MI355X.

  * EXACT cases (integer vectors, coefficients m 2^e): every product and partial sum is representable, so the result must
    EQUAL the integer one, on the smallest geometries at which each mechanism of the kernels can go wrong (fe_truth.GEOMETRIES:
    one mesh row, exactly 64 / 65 / 256 / 257 columns, 8 slabs / 8 slabs + 1 row, block rows that change just past a slab
    boundary, strips, 64 blocks), with M > 1 parameters per call and more than 65 535 of them.
  * ROUNDING cases against the long-double edge-form product with the rigorous bound gamma_7 |A||x|; norms of rows from
    1e-150 to 1e150 against the long-double edge form.
  * Outputs sit inside larger allocations filled with a NaN-payload sentinel; the bands must keep their bits.  Row offsets
    on inputs and outputs.  ROMHC_POISON_WS repeats must give the same bits.
  * Reduced solves: fe_truth.reduced_route restates the launcher's decision and a pure-Python test asserts that the sizes
    take every storage route, sit on both sides of 89 | 90 and 141 | 142, and that one case needs two launches.  Bounds:
    Higham's normwise backward error n gamma_(3n+1) (independent of the conditioning) and a forward error within
    8 x max(LAPACK's own, n u) of the 80-bit solution.
  * Projectors: relative H^1_0 distance from the 80-bit truth within 8 x max(the oracle's own, dim u).

Every bound goes through conftest.observed: the terminal summary shows the GPU's value next to its bound and, for the
reference-relative bounds, the reference's own error (the lines ending in "[reference]").

The two-launch reduced solve (n = 512, kb = 2, M = 513: 511 + 2 systems, 1 GiB of scratch) takes 0.2 s on an MI355X
(host references included), against a median of 0.05 s for the other cases of the reduced-solve test: it stays.
"""
import math

import numpy as np
import pytest
import scipy.linalg

from conftest import observed
from oracle import rom_oracle as ro
import fe_truth as ft
import referee as rf

pytestmark = pytest.mark.gpu

LD = np.longdouble
U = 2.0 ** -53
SENTINEL = np.array([0x7FF8DEADBEEF0001], dtype=np.uint64).view(np.float64)[0]   # a NaN with a payload: the guard bands
SENT_BITS = np.uint64(0x7FF8DEADBEEF0001)


@pytest.fixture(scope="module")
def ctx():
    from romhighcontrast_amd import _ffi
    return _ffi.get_context()


@pytest.fixture(scope="module")
def fems(ctx):
    """_ffi.Fem handles, one per (blocks, N), created on first use and shared by the whole module."""
    from romhighcontrast_amd import _ffi
    cache = {}

    def get(gm):
        if gm not in cache:
            (p, q), N = gm
            cache[gm] = _ffi.Fem(ctx, p, q, N)
        return cache[gm]
    return get


class Guarded:
    """An output window of n doubles at offset `lead` of a larger device buffer filled with the sentinel."""

    def __init__(self, ctx, n, lead=0, tail=37):
        self.n, self.lead = n, lead
        self.buf = ctx.upload(np.full(lead + n + tail, SENTINEL))

    def read(self, shape=None):
        """The window; asserts that both bands kept their bits."""
        got = self.buf.download()
        bits = got.view(np.uint64)
        assert (bits[:self.lead] == SENT_BITS).all() and (bits[self.lead + self.n:] == SENT_BITS).all(), \
            "an entry outside the output window changed"
        w = got[self.lead:self.lead + self.n]
        return w.reshape(shape) if shape is not None else w


def _rows_in_nan(ctx, X, row0, tail_rows=1):
    """Rows X (K, dim) at row offset row0 of a device buffer whose other rows are NaN."""
    K, dim = X.shape
    host = np.full((row0 + K + tail_rows, dim), np.nan)
    host[row0:row0 + K] = X
    return ctx.upload(host)


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


# =====================================================================================================================
# a. rom_assemble_batch
# =====================================================================================================================
def _assemble(ctx, fem, g, a):
    M = len(a)
    ne, nn = g.nr * (g.nc - 1), (g.nr - 1) * g.nc
    D, E, Nn = Guarded(ctx, M * g.dim), Guarded(ctx, M * ne), Guarded(ctx, M * nn)
    fem.assemble_batch(ctx.upload(a), M, D.buf, E.buf, Nn.buf)
    return D.read((M, g.nr, g.nc)), E.read((M, g.nr, g.nc - 1)), Nn.read((M, g.nr - 1, g.nc))


@pytest.mark.parametrize("M", [1, 2, 65, 300])
@pytest.mark.parametrize("gm", ft.GEOMETRIES, ids=ft.geom_id)
def test_assemble_exact(ctx, fems, gm, M):
    """M parameters per call with exact coefficients: diag / east / north EQUAL the integer truth (the m-strided writes, the
    LDS staging of a[m]); nothing past the arrays changes."""
    blocks, N = gm
    a, diag, east, north = ft.exact_assemble_case(blocks, N, M, seed=1000 * M + N)
    got = _assemble(ctx, fems(gm), ro.Geometry(blocks, N), a)
    for name, x, ref in zip(("diag", "east", "north"), got, (diag, east, north)):
        assert np.array_equal(x, ref), f"{name}: {int((x != ref).sum())} entries differ, first at {tuple(np.argwhere(x != ref)[0])}"


@pytest.mark.parametrize("gm", ft.GEOMETRIES, ids=ft.geom_id)
def test_assemble_random_equals_the_oracle_bit_for_bit(ctx, fems, gm):
    """Coefficients 10^U(0, 8), M > 1: the kernel adds in the reference's order, so every row equals ro.stencil_arrays."""
    blocks, N = gm
    g = ro.Geometry(blocks, N)
    for M in (3, 65) if g.dim < 20000 else (3,):
        a = 10.0 ** np.random.default_rng(N + M).uniform(0, 8, size=(M,) + blocks)
        got = _assemble(ctx, fems(gm), g, a)
        for m in range(M):
            for x, ref in zip(got, ro.stencil_arrays(g, a[m])):
                assert same_bits(x[m], ref), (M, m)


def test_assemble_more_parameters_than_one_grid_dimension(ctx, fems):
    """M = 65537 > 65535 (the limit of grid.y): the call succeeds and every row -- 0, 65534, 65535, 65536 among them -- is
    right.  (Regression: the launch put M into grid.y and failed with a HIP launch error.)"""
    gm = ((1, 1), 3)
    M = 65537
    a, diag, east, north = ft.exact_assemble_case((1, 1), 3, M, seed=7)
    got = _assemble(ctx, fems(gm), ro.Geometry(*gm), a)
    for x, ref in zip(got, (diag, east, north)):
        for m in (0, 65534, 65535, 65536):
            assert np.array_equal(x[m], ref[m]), m
        assert np.array_equal(x, ref)


# =====================================================================================================================
# b. rom_stencil_apply
# =====================================================================================================================
def _apply(ctx, fem, g, a, X, x_row0, y_row0):
    K = len(X)
    Xb = _rows_in_nan(ctx, X, x_row0)
    Y = Guarded(ctx, K * g.dim, lead=y_row0 * g.dim, tail=g.dim + 5)
    fem.stencil_apply(Xb, K, Y.buf, a_one=a, x_row0=x_row0, y_row0=y_row0)
    return Y.read((K, g.dim))


@pytest.mark.parametrize("K", [1, 3])
@pytest.mark.parametrize("unit", [True, False], ids=["unit", "blocks"])
@pytest.mark.parametrize("gm", ft.GEOMETRIES, ids=ft.geom_id)
def test_stencil_apply_exact(ctx, fems, gm, unit, K):
    """Integer X, unit or exact block coefficients: Y EQUALS A(a) X (lane shuffles and edge lanes, slab hand-over, the block
    row of every mesh row); K = 3 with X at row 1 and Y at row 2 of larger buffers, guard bands intact."""
    blocks, N = gm
    a, X, Yref = ft.exact_stencil_case(blocks, N, K, seed=N + 10 * K + unit, unit=unit)
    off = (1, 2) if K == 3 else (0, 0)
    got = _apply(ctx, fems(gm), ro.Geometry(blocks, N), None if unit else a, X, *off)
    assert np.array_equal(got, Yref), f"{int((got != Yref).sum())} entries differ, first at {tuple(np.argwhere(got != Yref)[0])}"


@pytest.mark.parametrize("gm", ft.GEOMETRIES, ids=ft.geom_id)
def test_stencil_apply_rounding_bound(ctx, fems, gm, monkeypatch):
    """Normal entries scaled over 10^+-8, coefficients 10^U(0, 8): |Y - ref| <= gamma_7 |A||x| entrywise against the long-double
    edge-form product of the same fp64 inputs (five products and four additions per entry; the oracle's stencil arrays,
    which the kernel reproduces to the bit, are the exact data of both).  The same bits over a poisoned scratch area."""
    blocks, N = gm
    g = ro.Geometry(blocks, N)
    rng = np.random.default_rng(N)
    a = 10.0 ** rng.uniform(0, 8, size=blocks)
    X = rng.standard_normal((2, g.dim)) * 10.0 ** rng.uniform(-8, 8, size=(2, g.dim))
    ref, absprod = ft.apply_ld(g, a, X)
    got = _apply(ctx, fems(gm), g, a, X, 1, 1)
    assert np.isfinite(got).all()
    err = np.abs(got.astype(LD) - ref)
    observed(f"fe {ft.geom_id(gm)} stencil_apply: |Y - ref| / (gamma_7 |A||x|)", np.asarray(err / (ft.gamma(7) * absprod), dtype=np.float64), 1.0)
    monkeypatch.setenv("ROMHC_POISON_WS", "1")
    again = _apply(ctx, fems(gm), g, a, X, 1, 1)
    monkeypatch.delenv("ROMHC_POISON_WS")
    assert same_bits(got, again), "poisoned scratch area: different bits"


# =====================================================================================================================
# c. rom_h10norm
# =====================================================================================================================
@pytest.mark.parametrize("diff", [False, True], ids=["plain", "difference"])
@pytest.mark.parametrize("gm", ft.GEOMETRIES, ids=ft.geom_id)
def test_h10norm_exact(ctx, fems, gm, diff):
    """Integer rows: x^T A_1 x is an exact integer in any summation order, the norm is its square root to one ulp; U == V
    gives exactly 0.  Rows at offsets 1 (U) and 2 (V)."""
    blocks, N = gm
    Uh, Vh, S = ft.exact_norm_case(blocks, N, 3, seed=3 * N + diff, diff=diff)
    fem = fems(gm)
    Ub = _rows_in_nan(ctx, Uh, 1)
    Vb = _rows_in_nan(ctx, Vh, 2) if diff else None
    got = fem.h10norm(Ub, 3, u_row0=1, V=Vb, v_row0=2)
    for k in range(3):
        assert ft.sqrt_ulps_ok(got[k], S[k]), f"row {k}: {got[k]!r} vs sqrt({S[k]}) = {math.sqrt(S[k])!r}"
    zero = fem.h10norm(Ub, 3, u_row0=1, V=_rows_in_nan(ctx, Uh, 2), v_row0=2)
    assert same_bits(zero, np.zeros(3))


def test_h10norm_rows_of_very_different_scale(ctx, fems):
    """300 rows on 65 x 65 scaled from 1e-150 to 1e150 (no overflow in the squares) against the long-double edge form: relative
    error <= (dim + 4) u -- the first-order bound of a sum of dim-odd non-negative terms, each a rounded difference squared;
    the square root halves it and the bound keeps that slack."""
    gm = ((1, 1), 66)
    g = ro.Geometry(*gm)
    rng = np.random.default_rng(66)
    K = 300
    X = rng.uniform(-1, 1, size=(K, g.dim)) * 10.0 ** rng.uniform(-150, 150, size=(K, 1))
    Y = rng.uniform(-1, 1, size=(K, g.dim)) * 10.0 ** rng.uniform(-150, 150, size=(K, 1))
    fem = fems(gm)
    got = fem.h10norm(_rows_in_nan(ctx, X, 3), K, u_row0=3)
    ref = np.array([rf.h10_ld(g, x.astype(LD)) for x in X])
    assert np.isfinite(got).all() and (got > 0).all()
    observed("fe 65x65 h10norm, 300 rows 1e-150..1e150: relative error vs long double", np.asarray(np.abs(got.astype(LD) - ref) / ref, dtype=np.float64),
             (g.dim + 4) * U)
    got = fem.h10norm(_rows_in_nan(ctx, X, 0), K, V=_rows_in_nan(ctx, Y, 1), v_row0=1)
    ref = np.array([rf.h10_ld(g, x.astype(LD) - y.astype(LD)) for x, y in zip(X, Y)])
    # (the difference u - v is rounded once more: one more u per entry, inside the slack of the square root)
    observed("fe 65x65 h10norm of differences, 300 rows: relative error vs long double", np.asarray(np.abs(got.astype(LD) - ref) / ref, dtype=np.float64),
             (g.dim + 4) * U)


def test_h10norm_refuses_more_rows_than_one_grid_dimension(ctx, fems):
    """K = 65536 returns ROM_ERR_INVALID with a message (today's contract)."""
    from romhighcontrast_amd import _ffi
    fem = fems(((1, 1), 3))
    Ub = ctx.upload(np.ones(65536 * fem.dim))
    out = np.zeros(65536)
    st = ctx.lib.rom_h10norm(fem.h, Ub.h, 0, None, 0, 65536, out.ctypes.data)
    assert st == _ffi.ROM_ERR_INVALID and b"65535" in ctx.lib.rom_last_error()
    assert np.array_equal(fem.h10norm(Ub, 65535), np.full(65535, math.sqrt(8.0)))   # (and the largest K it takes is right)


# =====================================================================================================================
# d. rom_evaluate_points
# =====================================================================================================================
def _chosen_points(g, seed):
    """Every combination of ix in {0, 1, nc-1, nc}, iy in {0, 1, nr-1, nr} (ring cells and their neighbours) and (tx, ty) on the
    dyadic grid {0, 1/4, 1/2, 3/4, 1}^2 (both triangles and the diagonal tx + ty = 1): 400 points, shuffled."""
    t = [0.0, 0.25, 0.5, 0.75, 1.0]
    pts = [(ix, iy, tx, ty) for ix in (0, 1, g.nc - 1, g.nc) for iy in (0, 1, g.nr - 1, g.nr) for tx in t for ty in t]
    order = np.random.default_rng(seed).permutation(len(pts))
    P = np.array([pts[i] for i in order])
    return P[:, 0].astype(np.int32), P[:, 1].astype(np.int32), P[:, 2].copy(), P[:, 3].copy()


@pytest.mark.parametrize("K", [1, 3])
@pytest.mark.parametrize("gm", [((2, 3), 11), ((1, 1), 66)], ids=ft.geom_id)
def test_evaluate_points_exact(ctx, fems, gm, K):
    """Integer U, dyadic local coordinates: every value is exact in Fractions and the result must EQUAL it -- ring cells,
    both triangles, the diagonal, npts on both sides of the 256-thread block, rows at offset 2."""
    g = ro.Geometry(*gm)
    fem = fems(gm)
    Uh = np.random.default_rng(K).integers(-2 ** 20, 2 ** 20 + 1, size=(K, g.dim)).astype(np.float64)
    Ub = _rows_in_nan(ctx, Uh, 2)
    ix, iy, tx, ty = _chosen_points(g, K)
    ref = np.array([[float(ft.eval_point_frac(g, u, *p)) for p in zip(ix, iy, tx, ty)] for u in Uh])
    for npts in (1, 255, 256, 257, 400):
        got = fem.evaluate_points(Ub, K, ix[:npts], iy[:npts], tx[:npts], ty[:npts], row0=2)
        assert got.shape == (K, npts) and np.array_equal(got, ref[:, :npts]), npts


def test_evaluate_points_refuses_cells_outside_the_ring(ctx, fems):
    from romhighcontrast_amd import _ffi
    gm = ((2, 3), 11)
    fem, g = fems(gm), ro.Geometry(*gm)
    Ub = ctx.upload(np.ones(g.dim))
    for ix, iy in [(-1, 0), (g.nc + 1, 0), (0, -1), (0, g.nr + 1)]:
        out = np.zeros(1)
        i, j, t = np.array([ix], dtype=np.int32), np.array([iy], dtype=np.int32), np.array([0.5])
        st = ctx.lib.rom_evaluate_points(fem.h, Ub.h, 0, 1, 1, i.ctypes.data, j.ctypes.data, t.ctypes.data, t.ctypes.data, out.ctypes.data)
        assert st == _ffi.ROM_ERR_INVALID and b"outside the domain" in ctx.lib.rom_last_error(), (ix, iy)


def test_evaluate_points_more_solutions_than_one_grid_dimension(ctx, fems):
    """K = 65537 > 65535 with npts = 3 on the smallest grid.  (Regression: K went into grid.y.)"""
    gm = ((1, 1), 3)
    g = ro.Geometry(*gm)
    K = 65537
    Uh = np.random.default_rng(3).integers(-2 ** 20, 2 ** 20 + 1, size=(K, g.dim)).astype(np.float64)
    ix, iy = np.array([0, 1, 2], dtype=np.int32), np.array([2, 1, 0], dtype=np.int32)
    tx, ty = np.array([0.25, 0.5, 0.75]), np.array([0.5, 0.5, 0.75])
    got = fems(gm).evaluate_points(_rows_in_nan(ctx, Uh, 1), K, ix, iy, tx, ty, row0=1)
    # the exact values, vectorised: quarters of integers below 2^23 (fe_truth.eval_point_frac on the four named rows)
    V = np.zeros((K, g.nr + 2, g.nc + 2))
    V[:, 1:-1, 1:-1] = Uh.reshape(K, g.nr, g.nc)
    lower = (1 - tx - ty) * V[:, iy, ix] + tx * V[:, iy, ix + 1] + ty * V[:, iy + 1, ix]
    upper = (tx + ty - 1) * V[:, iy + 1, ix + 1] + (1 - tx) * V[:, iy + 1, ix] + (1 - ty) * V[:, iy, ix + 1]
    ref = np.where(tx + ty < 1, lower, upper)
    for k in (0, 65534, 65535, 65536):
        assert [float(ft.eval_point_frac(g, Uh[k], *p)) for p in zip(ix, iy, tx, ty)] == ref[k].tolist()
        assert np.array_equal(got[k], ref[k]), k
    assert np.array_equal(got, ref)


def test_evaluate_solutions_on_cell_corners_and_edges(ctx):
    """SolutionsManagerFEM.evaluate_solutions with points on vertices and on cell edges (where searchsorted puts the point on
    the far side of a cell: tx or ty = 1 up to rounding) against the oracle.  Both evaluate the same three-term formula from
    the same computed (ix, iy, tx, ty): each within gamma_6 sum |weight| |value| of its exact value (two roundings per weight,
    a product, two additions) and the weights of a triangle sum to 1, so they differ by at most 2 gamma_6 max |u|.  On a
    vertex tx = ty = 1 exactly and the value is the nodal one."""
    from romhighcontrast_amd.lib.SolutionsManagers import SolutionsManagerFEM
    blocks, N = (2, 3), 11
    sm, g = SolutionsManagerFEM(blocks, N), ro.Geometry(blocks, N)
    rng = np.random.default_rng(11)
    Uh = rng.standard_normal((3, g.dim))
    cx, cy = rng.integers(1, g.nc_cells - 1, size=60), rng.integers(1, g.nr_cells - 1, size=60)
    vert = np.stack((g.points_c[cx], g.points_r[cy]), axis=1)                                          # vertices
    hedge = np.stack((g.points_c[cx] + rng.uniform(0.05, 0.95, 60) / N, g.points_r[cy]), axis=1)        # on horizontal edges
    vedge = np.stack((g.points_c[cx], g.points_r[cy] - rng.uniform(0.05, 0.95, 60) / N), axis=1)        # on vertical edges
    pts = np.vstack((vert, hedge, vedge))
    got, ref = sm.evaluate_solutions(pts, Uh), ro.evaluate_solutions(g, pts, Uh)
    observed("fe 21x32 evaluate_solutions on vertices / edges vs oracle, / (2 gamma_6 max|u|)",
             np.abs(got - ref) / (2 * ft.gamma(6) * np.abs(Uh).max(axis=1))[:, None], 1.0)
    assert np.array_equal(got[:, :60], Uh.reshape(3, g.nr, g.nc)[:, cy - 1, cx - 1])


# =====================================================================================================================
# e. rom_reduced_solve_batch
# =====================================================================================================================
REDUCED_SIZES = [1, 2, 64, 89, 90, 141, 142, 260]
TWO_LAUNCH = dict(n=512, kb=2, M=513)


def test_reduced_sizes_take_every_route():
    """Pure Python: the sizes above take all three storage routes, sit on both sides of both boundaries, and the two-launch
    case splits as 511 + 2 (a change of the thresholds in rom_launch_reduced_solve shows up here)."""
    routes = {n: ft.reduced_route(n, 5)["route"] for n in REDUCED_SIZES}
    assert set(routes.values()) == {"lds64", "lds160", "global"}
    assert (routes[89], routes[90], routes[141], routes[142]) == ("lds64", "lds160", "lds160", "global")
    assert all(ft.reduced_route(n, 5)["launches"] == 1 for n in REDUCED_SIZES)
    assert ft.reduced_route(TWO_LAUNCH["n"], TWO_LAUNCH["M"]) == dict(route="global", per_launch=511, launches=2)


def _reduced(ctx, n, kb, M, Ahat, w, rhs, per_system):
    c = Guarded(ctx, M * n)   # (the C entry writes from the start of c_out: the band is what follows the M n results)
    ctx.reduced_solve_batch(n, kb, M, ctx.upload(Ahat), ctx.upload(w), ctx.upload(rhs), per_system, c.buf)
    return c.read((M, n))


@pytest.mark.parametrize("family", ["well", "graded"])
@pytest.mark.parametrize("n", REDUCED_SIZES)
def test_reduced_solves_backward_and_forward_error(ctx, n, family):
    """kb in {1, 4}, shared and per-system right-hand sides, M = 5 with different weights per system.  Backward error (80-bit
    residual, normwise) <= n gamma_(3n+1): Higham's bound for a Cholesky / LDL^T solve, the factor n from entrywise to
    Frobenius norm; derived, independent of the conditioning.  Forward error against the 80-bit solution <= 8 x max(LAPACK's
    own on the same inputs, n u): two backward-stable eliminations in different summation orders differ by small
    multiples, a lost digit fails."""
    M = 5
    for kb in (1, 4):
        for per in (False, True):
            Ahat, w, rhs = ft.reduced_case(family, n, kb, M, per)
            got = _reduced(ctx, n, kb, M, Ahat, w, rhs, per)
            assert np.isfinite(got).all()
            truth, back = ft.spd_truth_ld(Ahat, w, rhs, c_hat=got)
            tag = f"fe reduced solve {family} n={n} kb={kb} {'rhs/system' if per else 'one rhs'} ({ft.reduced_route(n, M)['route']})"
            observed(f"{tag}: backward error", back, n * ft.gamma(3 * n + 1))
            e_ref = ft.rel2_ld(ft.lapack_pos(Ahat, w, rhs), truth)
            observed(f"{tag}: LAPACK forward error [reference]", e_ref, 1.0)
            observed(f"{tag}: forward error vs 80-bit", ft.rel2_ld(got, truth), 8 * max(e_ref, n * U))


def test_reduced_solve_in_two_launches(ctx):
    """n = 512, kb = 2, M = 513: matrices in global memory, 511 systems per launch (1 GiB of scratch), so a second launch of two
    systems with the w / rhs / c offsets m0 kb, m0 n, m0 n.  Distinct weights and right-hand sides per system: a wrong
    offset cannot pass.  fp64 LAPACK on systems 0, 510, 511, 512, an fp64 residual on all 513."""
    n, kb, M = TWO_LAUNCH["n"], TWO_LAUNCH["kb"], TWO_LAUNCH["M"]
    assert ft.reduced_route(n, M)["launches"] == 2
    Ahat, w, rhs = ft.reduced_case("well", n, kb, M, True)
    got = _reduced(ctx, n, kb, M, Ahat, w, rhs, True)
    assert np.isfinite(got).all()
    for m in (0, 510, 511, 512):
        A = np.einsum("b,bij->ij", w[m], Ahat)
        ref = scipy.linalg.solve(A, rhs[m], assume_a="pos")
        # (condition <= 4 (3 + 0.05) / 0.05 < 250: two backward-stable solves agree to cond n u -- the reference's own error)
        observed(f"fe reduced solve, two launches, system {m}: vs LAPACK, relative 2-norm", np.linalg.norm(got[m] - ref) / np.linalg.norm(ref),
                 250 * n * U)
    A0, A1 = Ahat[0] @ got.T, Ahat[1] @ got.T                                    # (n, M)
    R = rhs.T - (w[:, 0][None, :] * A0 + w[:, 1][None, :] * A1)
    nA = np.sqrt(w[:, 0] ** 2 * (Ahat[0] ** 2).sum() + w[:, 1] ** 2 * (Ahat[1] ** 2).sum() + 2 * w[:, 0] * w[:, 1] * (Ahat[0] * Ahat[1]).sum())
    back = np.linalg.norm(R, axis=0) / (nA * np.linalg.norm(got, axis=1) + np.linalg.norm(rhs, axis=1))
    # (the residual itself is evaluated in fp64 here: gamma_(n+2) on top of the solve's n gamma_(3n+1))
    observed("fe reduced solve, two launches: fp64 backward error of all 513 systems", back, n * ft.gamma(3 * n + 1) + ft.gamma(n + 2))


def test_reduced_solve_reports_a_non_positive_pivot_once(ctx):
    """One indefinite system at index 0, then at index M - 1: ROM_ERR_NOT_SPD; the SPD call that follows returns 0 (the status
    word is reset)."""
    from romhighcontrast_amd import _ffi
    n, kb, M = 90, 2, 5
    Ahat, w, rhs = ft.reduced_case("well", n, kb, M, False)
    Ahat[1] = -100.0 * np.eye(n)
    Ab, rb, c = ctx.upload(Ahat), ctx.upload(rhs), ctx.alloc(M * n)
    for bad in (0, M - 1):
        wb = np.zeros((M, kb))
        wb[:, 0] = w[:, 0]
        wb[bad, 1] = 1.0                                        # w_0 Ahat_0 - 100 I: indefinite
        wd = ctx.upload(wb)                                     # (held in a name: the raw call below takes the handle only)
        st = ctx.lib.rom_reduced_solve_batch(ctx.h, n, kb, M, Ab.h, wd.h, rb.h, 0, c.h)
        assert st == _ffi.ROM_ERR_NOT_SPD and b"not positive definite" in ctx.lib.rom_last_error(), bad
        wb[bad, 1] = 0.0
        wd = ctx.upload(wb)
        assert ctx.lib.rom_reduced_solve_batch(ctx.h, n, kb, M, Ab.h, wd.h, rb.h, 0, c.h) == _ffi.ROM_OK
        assert ft.rel2_ld(c.download(shape=(M, n)), ft.lapack_pos(Ahat, wb, rhs)) < 1e-12


# =====================================================================================================================
# f. rom_project_h10 and rom_galerkin_rom
# =====================================================================================================================
def _project(ctx, fem, g, Uh, C, offs=(0, 0, 0)):
    u0, c0, o0 = offs
    M, n = len(Uh), len(C)
    out = Guarded(ctx, M * g.dim, lead=o0 * g.dim, tail=g.dim + 3)
    fem.project_h10(_rows_in_nan(ctx, Uh, u0), M, _rows_in_nan(ctx, C, c0), n, out.buf, u_row0=u0, c_row0=c0, out_row0=o0)
    return out.read((M, g.dim))


def _galerkin(ctx, fem, g, a, C, offs=(0, 0)):
    c0, o0 = offs
    M, n = len(a), len(C)
    out = Guarded(ctx, M * g.dim, lead=o0 * g.dim, tail=g.dim + 3)
    fem.galerkin_rom(ctx.upload(a), M, _rows_in_nan(ctx, C, c0), n, out.buf, c_row0=c0, out_row0=o0)
    return out.read((M, g.dim))


BASES = [("qr", n) for n in ft.QR_SIZES] + [("raw", n) for n in ft.RAW_SIZES]


def test_projector_basis_sizes_sit_on_the_reduced_solve_boundaries():
    assert [ft.reduced_route(n)["route"] for n in (89, 90, 141, 142)] == ["lds64", "lds160", "lds160", "global"]
    assert {89, 90, 141, 142} <= set(ft.QR_SIZES) and max(ft.QR_SIZES) <= ro.Geometry(*ft.PROJ_GEOMS[0]).dim


@pytest.mark.parametrize("kind,n", BASES, ids=[f"{k}{n}" for k, n in BASES])
@pytest.mark.parametrize("d", [2, 6])
@pytest.mark.parametrize("gm", ft.PROJ_GEOMS, ids=ft.geom_id)
def test_projectors_against_the_80_bit_truth(ctx, fems, gm, d, kind, n):
    """M in {1, 7} snapshots / parameters 10^U(0, d); QR-orthonormal bases (n on the reduced solve's storage boundaries) and raw
    snapshots (a greedy basis: C A_1 C^T badly conditioned).  max over rows of ||x - truth|| / ||truth|| in H^1_0 (long double)
    <= 8 x max(the oracle's own distance, dim u): the GPU runs the reference's algorithm -- normal equations in the given
    basis -- so the reference's distance from the truth is the yardstick; dim u, the first-order bound of one dim-long dot
    product, is the floor; 8 because two backward-stable routes differ by small multiples while a lost digit must fail."""
    inp = ft.projector_inputs(gm, d)
    g, fem = inp["g"], fems(gm)
    C = inp["Cqr" if kind == "qr" else "Craw"][:n]
    span = ft.projector_span(gm, d, kind)
    Pt, keep = ft.project_truth_ld(g, inp["U"], C, n=n, span=span)
    Gt, _ = ft.galerkin_truth_ld(g, inp["a"], C, n=n, span=span)
    assert keep.all()
    Po, Go = ro.project_solutions(g, inp["U"], C), ro.generate_fm_solutions(g, inp["a"], C)
    tag = f"fe {ft.geom_id(gm)} d={d} {kind} n={n}"
    for M in (1, 7):
        e_ref = ft.rel_h10_ld(g, Po[:M], Pt[:M])
        observed(f"{tag} M={M} project_h10: oracle vs 80-bit [reference]", e_ref, 1.0)
        observed(f"{tag} M={M} project_h10: GPU vs 80-bit", ft.rel_h10_ld(g, _project(ctx, fem, g, inp["U"][:M], C), Pt[:M]), 8 * max(e_ref, g.dim * U))
        e_ref = ft.rel_h10_ld(g, Go[:M], Gt[:M])
        observed(f"{tag} M={M} galerkin_rom: oracle vs 80-bit [reference]", e_ref, 1.0)
        observed(f"{tag} M={M} galerkin_rom: GPU vs 80-bit", ft.rel_h10_ld(g, _galerkin(ctx, fem, g, inp["a"][:M], C), Gt[:M]), 8 * max(e_ref, g.dim * U))


@pytest.mark.parametrize("gm", ft.PROJ_GEOMS, ids=ft.geom_id)
def test_projection_of_a_basis_member_and_offsets(ctx, fems, gm):
    """The projection of a basis member returns it and is idempotent, to the bound of the test above (the oracle's own
    distance from the member as the yardstick); with c_row0, u_row0, out_row0 > 0 both calls give the bits of the
    offset-free call."""
    inp = ft.projector_inputs(gm, 2)
    g, fem = inp["g"], fems(gm)
    for kind, n in (("qr", 90), ("raw", 8)):
        C = inp["Cqr" if kind == "qr" else "Craw"][:n]
        members = C[[0, n // 2, n - 1]]
        P1 = _project(ctx, fem, g, members, C)
        e_ref = ft.rel_h10_ld(g, ro.project_solutions(g, members, C), members)
        bound = 8 * max(e_ref, g.dim * U)
        observed(f"fe {ft.geom_id(gm)} {kind} n={n}: oracle's projection of a basis member [reference]", e_ref, 1.0)
        observed(f"fe {ft.geom_id(gm)} {kind} n={n}: projection of a basis member returns it", ft.rel_h10_ld(g, P1, members), bound)
        observed(f"fe {ft.geom_id(gm)} {kind} n={n}: projecting twice", ft.rel_h10_ld(g, _project(ctx, fem, g, P1, C), P1), bound)
        Uh, a = inp["U"][:3], inp["a"][:3]
        assert same_bits(_project(ctx, fem, g, Uh, C), _project(ctx, fem, g, Uh, C, offs=(1, 2, 3)))
        assert same_bits(_galerkin(ctx, fem, g, a, C), _galerkin(ctx, fem, g, a, C, offs=(2, 1)))


def test_projectors_report_dependent_rows(ctx, fems):
    """Dependent rows return ROM_ERR_NOT_SPD through both calls.  The pivot test is `d > 0` on the computed pivot, so the rows are
    chosen such that the pivot is EXACTLY zero: a zero row, and a duplicated nodal vector e_i inside block (0, 0) with
    power-of-two parameters (C A C^T = 4 a_00 [[1, 1], [1, 1]]: every product of the elimination is exact).  (For general
    duplicates the second pivot is a rounding residue of either sign.)  The call after it succeeds."""
    from romhighcontrast_amd import _ffi
    gm = ft.PROJ_GEOMS[0]
    inp = ft.projector_inputs(gm, 2)
    g, fem = inp["g"], fems(gm)
    e = np.zeros(g.dim)
    e[2 * g.nc + 2] = 1.0                                   # vertex (3, 3) of block (0, 0), N = 8
    a = 2.0 ** np.random.default_rng(0).integers(0, 8, size=(3,) + gm[0])
    for C in (np.stack((e, e)), np.vstack((inp["Cqr"][:3], np.zeros((1, g.dim)), inp["Cqr"][3:5]))):
        n = len(C)
        Cb, Ub, ab, out = ctx.upload(C), ctx.upload(inp["U"][:3]), ctx.upload(a), ctx.alloc(3 * g.dim)
        for st in (ctx.lib.rom_project_h10(fem.h, Ub.h, 0, 3, Cb.h, 0, n, out.h, 0), ctx.lib.rom_galerkin_rom(fem.h, ab.h, 3, Cb.h, 0, n, out.h, 0)):
            assert st == _ffi.ROM_ERR_NOT_SPD and b"not positive definite" in ctx.lib.rom_last_error()
        assert ctx.lib.rom_project_h10(fem.h, Ub.h, 0, 3, Cb.h, 0, 1, out.h, 0) == _ffi.ROM_OK


# =====================================================================================================================
# g. rom_orthonormalize_rows
# =====================================================================================================================
def _ortho(ctx, X, in_place, x_row0=1, q_row0=2):
    n, dim = X.shape
    if in_place:
        host = np.full((x_row0 + n + 1) * dim + 5, SENTINEL)
        host[x_row0 * dim:(x_row0 + n) * dim] = X.ravel()
        buf = ctx.upload(host)
        ctx.orthonormalize_rows(buf, n, dim, buf, x_row0=x_row0, q_row0=x_row0)
        got = buf.download()
        bits = got.view(np.uint64)
        assert (bits[:x_row0 * dim] == SENT_BITS).all() and (bits[(x_row0 + n) * dim:] == SENT_BITS).all()
        return got[x_row0 * dim:(x_row0 + n) * dim].reshape(n, dim)
    Q = Guarded(ctx, n * dim, lead=q_row0 * dim, tail=dim + 5)
    Xb = _rows_in_nan(ctx, X, x_row0)
    ctx.orthonormalize_rows(Xb, n, dim, Q.buf, x_row0=x_row0, q_row0=q_row0)
    assert same_bits(Xb.download(n * dim, offset=x_row0 * dim), X.ravel()), "the input rows changed"
    return Q.read((n, dim))


@pytest.mark.parametrize("graded", [False, True], ids=["random", "graded"])
@pytest.mark.parametrize("n", [1, 4, 65, 130, 230])
def test_orthonormalize_rows(ctx, n, graded):
    """Rows of dimension 225 (230 > dim: the last five are combinations of the others), random or graded over 1e-12 in their
    scale: ||Q Q^T - I||_max <= 8 n u on the non-zero rows; every row within 8 x max(QR's own orthogonality defect, n u) of
    NumPy QR's row in angle, up to sign (long double; fe_truth.ortho_rows keeps the equilibrated block well conditioned, so
    that the rows of a QR are determined to that level); dependent rows exactly zero; in place and out of place the same
    bits."""
    dim = 225
    X = ft.ortho_rows(n, dim, 7, graded)
    Q = _ortho(ctx, X, in_place=False)
    assert same_bits(Q, _ortho(ctx, X, in_place=True)), "in place and out of place differ"
    k = min(n, dim)
    assert not Q[k:].any(), "rows past the dimension of the space must be exactly zero"
    QL = Q[:k].astype(LD)
    tag = f"fe orthonormalize n={n} {'graded' if graded else 'random'}"
    observed(f"{tag}: |Q Q^T - I|_max", np.asarray(np.abs(QL @ QL.T - np.eye(k, dtype=LD)), dtype=np.float64), 8 * n * U)
    R = np.linalg.qr(X[:k].T)[0].T.astype(LD)
    defect = float(np.abs(R @ R.T - np.eye(k, dtype=LD)).max())
    cosines = np.abs((QL * R).sum(axis=1)) / np.sqrt((QL * QL).sum(axis=1) * (R * R).sum(axis=1))
    sines = np.asarray(np.sqrt(((QL - np.sign((QL * R).sum(axis=1))[:, None] * R) ** 2).sum(axis=1)), dtype=np.float64)
    assert (cosines > 0.5).all()
    observed(f"{tag}: QR's own |R R^T - I|_max [reference]", defect, 1.0)
    observed(f"{tag}: angle of every row with NumPy QR's", sines, 8 * max(defect, n * U))


def test_orthonormalize_rows_zeroes_dependent_rows(ctx):
    """A duplicated row and a zero row come out exactly zero; the rows after them are as if they had not been there."""
    dim = 225
    X = ft.ortho_rows(6, dim, 9, False)
    Xd = np.vstack((X[:3], X[1:2], np.zeros((1, dim)), X[3:], 0.5 * X[0:1] - 3.0 * X[4:5]))
    for in_place in (False, True):
        Q = _ortho(ctx, Xd, in_place)
        assert not Q[3].any() and not Q[4].any() and not Q[8].any()
        live = Q[[0, 1, 2, 5, 6, 7]].astype(LD)
        observed(f"fe orthonormalize with dependent rows ({'in place' if in_place else 'out of place'}): |Q Q^T - I|_max on the others",
                 np.asarray(np.abs(live @ live.T - np.eye(6, dtype=LD)), dtype=np.float64), 8 * 9 * U)
        # (the same rows as without the dependent ones: each is determined to a small multiple of u, fe_truth.ortho_rows)
        observed(f"fe orthonormalize with dependent rows ({'in place' if in_place else 'out of place'}): the others vs the call without them",
                 np.abs(Q[[0, 1, 2, 5, 6, 7]] - _ortho(ctx, X, in_place)), 8 * 9 * U)
