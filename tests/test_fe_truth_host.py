"""tests/fe_truth.py proved on the CPU, before tests/test_gpu_fe_ops.py relies on it: the exact cases equal the oracle to the
bit (one ulp for the square root of a norm), the 80-bit truths agree with the oracle where the problem is well conditioned,
and where it is not the REFERENCE's own distance from the truth is finite and below 1 -- "within a factor of the reference"
then means something."""
import math

import numpy as np
import pytest

from oracle import rom_oracle as ro
import fe_truth as ft
import referee as rf

LD = np.longdouble


@pytest.mark.parametrize("gm", ft.GEOMETRIES, ids=ft.geom_id)
def test_exact_cases_equal_the_oracle(gm):
    blocks, N = gm
    g = ro.Geometry(blocks, N)
    for unit in (True, False):
        a, X, Y = ft.exact_stencil_case(blocks, N, 3, seed=N, unit=unit)
        assert np.array_equal(ro.stencil_apply(g, a, X), Y)
    a, diag, east, north = ft.exact_assemble_case(blocks, N, 5, seed=N + 1)
    for m in range(5):
        for got, ref in zip(ro.stencil_arrays(g, a[m]), (diag[m], east[m], north[m])):
            assert got.shape == ref.shape and np.array_equal(got, ref)
    for diff in (False, True):
        U, V, S = ft.exact_norm_case(blocks, N, 3, seed=N + 2, diff=diff)
        got = ro.H10norm(g, U - V if diff else U)
        for k in range(3):
            assert ft.sqrt_ulps_ok(got[k], S[k]) and abs(got[k] - math.sqrt(S[k])) <= math.ulp(got[k])
    assert ft.sqrt_ulps_ok(3.0, 9) and not ft.sqrt_ulps_ok(3.0 + 3 * math.ulp(3.0), 9) and ft.sqrt_ulps_ok(0.0, 0)


def test_exact_point_values_equal_the_oracle():
    blocks, N = (2, 3), 11
    g = ro.Geometry(blocks, N)
    rng = np.random.default_rng(5)
    u = rng.integers(-2 ** 20, 2 ** 20, size=g.dim).astype(np.float64)
    V = np.zeros((g.nr + 2, g.nc + 2))
    V[1:-1, 1:-1] = u.reshape(g.nr, g.nc)
    for ix, iy in [(0, 0), (g.nc, g.nr), (3, 7), (g.nc - 1, 1)]:
        for tx in (0.0, 0.25, 0.5, 1.0):
            for ty in (0.0, 0.75, 1.0):
                lower = (1 - tx - ty) * V[iy, ix] + tx * V[iy, ix + 1] + ty * V[iy + 1, ix]
                upper = (tx + ty - 1) * V[iy + 1, ix + 1] + (1 - tx) * V[iy + 1, ix] + (1 - ty) * V[iy, ix + 1]
                assert float(ft.eval_point_frac(g, u, ix, iy, tx, ty)) == (lower if tx + ty < 1 else upper)


def test_reduced_route_boundaries():
    r = ft.reduced_route
    assert [r(n)["route"] for n in (1, 89, 90, 141, 142, 512)] == ["lds64", "lds64", "lds160", "lds160", "global", "global"]
    assert 89 * 90 * 8 + 16 * 89 == 65504 and 141 * 142 * 8 + 16 * 141 == 162432
    assert r(512, 513) == dict(route="global", per_launch=511, launches=2) and r(141, 513)["launches"] == 1


@pytest.mark.parametrize("gm", ft.PROJ_GEOMS, ids=ft.geom_id)
def test_projector_truths_on_a_well_conditioned_basis(gm):
    """QR-orthonormal basis, contrast <= 1e2: truth and oracle agree to 1e-12 relative H^1_0; a basis member is reproduced;
    the dependent row of a duplicated basis is reported."""
    inp = ft.projector_inputs(gm, 2)
    g, a, U, C = inp["g"], inp["a"], inp["U"], inp["Cqr"][:20]
    P, keep = ft.project_truth_ld(g, U, C)
    assert keep.all() and ft.rel_h10_ld(g, ro.project_solutions(g, U, C), P) < 1e-12
    G, keep = ft.galerkin_truth_ld(g, a, C)
    assert keep.all() and ft.rel_h10_ld(g, ro.generate_fm_solutions(g, a, C), G) < 1e-12
    # nested prefixes of one SpanTruth are the truths of the prefixes
    span = ft.SpanTruth(g, C)
    assert np.array_equal(ft.project_truth_ld(g, U, C, n=5, span=span)[0], ft.project_truth_ld(g, U, C[:5])[0])
    assert np.array_equal(ft.galerkin_truth_ld(g, a, C, n=5, span=span)[0], ft.galerkin_truth_ld(g, a, C[:5])[0])
    # a basis member is its own projection (to the rounding of the result to fp64)
    Pm, _ = ft.project_truth_ld(g, C[3:4], C)
    assert ft.rel_h10_ld(g, Pm, C[3:4]) < 4 * 2.0 ** -53
    # and the Galerkin ROM in a basis that holds the solution returns it
    sol = ro.generate_solutions(g, a[:1])
    Gm, _ = ft.galerkin_truth_ld(g, a[:1], np.vstack((C[:3], sol)))
    assert ft.rel_h10_ld(g, Gm, sol) < 1e-11 * a[:1].max()    # (sol is SuperLU's: its own error, ~ contrast u, is what is left)
    Cd = np.vstack((C[:4], C[1:2], C[4:6]))
    Pd, keep = ft.project_truth_ld(g, U, Cd)
    assert keep.tolist() == [True] * 4 + [False] + [True] * 2
    assert ft.rel_h10_ld(g, Pd, ft.project_truth_ld(g, U, C[:6])[0]) < 4 * 2.0 ** -53
    Gd, keep = ft.galerkin_truth_ld(g, a, Cd)
    assert not keep[4] and ft.rel_h10_ld(g, Gd, ft.galerkin_truth_ld(g, a, C[:6])[0]) < 4 * 2.0 ** -53


@pytest.mark.parametrize("gm", ft.PROJ_GEOMS, ids=ft.geom_id)
@pytest.mark.parametrize("d", [2, 6])
def test_reference_error_on_raw_snapshot_bases_is_below_one(gm, d):
    inp = ft.projector_inputs(gm, d)
    g, a, U = inp["g"], inp["a"], inp["U"]
    span = ft.projector_span(gm, d, "raw")
    assert span.keep.all()
    for n in ft.RAW_SIZES:
        C = inp["Craw"][:n]
        e = ft.rel_h10_ld(g, ro.project_solutions(g, U, C), ft.project_truth_ld(g, U, C, n=n, span=span)[0])
        assert np.isfinite(e) and e < 1, (n, e)
        e = ft.rel_h10_ld(g, ro.generate_fm_solutions(g, a, C), ft.galerkin_truth_ld(g, a, C, n=n, span=span)[0])
        assert np.isfinite(e) and e < 1, (n, e)


def test_spd_truth_on_well_conditioned_systems():
    for n, kb, per in [(1, 1, False), (7, 4, True), (64, 4, False)]:
        Ahat, w, rhs = ft.reduced_case("well", n, kb, 5, per)
        ref = np.array([np.linalg.solve(np.einsum("b,bij->ij", w[m], Ahat), rhs[m] if per else rhs) for m in range(5)])
        c, back = ft.spd_truth_ld(Ahat, w, rhs, c_hat=ref)
        assert ft.rel2_ld(ref, c) < 1e-13 and back.max() < 4 * n * 2.0 ** -53
        assert ft.spd_truth_ld(Ahat, w, rhs, c_hat=1.001 * ref)[1].min() > 1e-5      # a wrong candidate shows


@pytest.mark.parametrize("n", [1, 2, 64, 89, 90, 141, 142, 260])
def test_reference_error_on_graded_systems_is_below_one(n):
    for kb in (1, 4):
        for per in (False, True):
            Ahat, w, rhs = ft.reduced_case("graded", n, kb, 5, per)
            c, _ = ft.spd_truth_ld(Ahat, w, rhs)
            e = ft.rel2_ld(ft.lapack_pos(Ahat, w, rhs), c)
            assert np.isfinite(np.asarray(c, dtype=np.float64)).all() and np.isfinite(e) and e < 1, (n, kb, per, e)


def test_ortho_rows_are_well_conditioned():
    for n, graded in [(130, False), (230, False), (130, True)]:
        X = ft.ortho_rows(n, 225, 1, graded)
        k = min(n, 225)
        Xe = X[:k] / np.linalg.norm(X[:k], axis=1)[:, None]
        assert np.linalg.cond(Xe) < 10
        assert np.linalg.matrix_rank(X[:, :]) == k or graded
