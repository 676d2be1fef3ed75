"""k_solve1 with the cross-lane traffic off the factor wave's chain (back substitution in blocks of four columns, the pivots'
reciprocals parked in LDS), and the panel arithmetic it shares with k_diag_factor.  Needs an MI355X.

Shapes: (2,2) at N = 128 with M in {1, 3, 4, 5, 130} (a lone system, a partial last workgroup whose other waves have no
system, more than one extension group), (2,2) at N = 24 with M = 7 (uncompressed edges), (1,2) at N = 32 with M = 5
(padding unknowns), and (3,3) at N = 24 with M = 40 for the general path.  Parameters 10**U(0,3) from a seeded generator, row 0
replaced by a row of contrast 1e8.  Every shape is compared
  * with the CPU oracle (SuperLU) on a few rows, the contrast row among them, at the snapshot tolerance of
    tests/test_gpu_parity.py (1e-11 relative H^1_0);
  * with the same library under ROMHC_NO_FUSED=1 at 1e-11 relative H^1_0 (the bound of test_algorithm_switches_agree);
  * two-stage (rom_solve_reduced_async + rom_expand_batch_async) against rom_solve_batch, bit for bit.
A non-positive coefficient must still come back as ROM_ERR_NOT_SPD through rom_solve_status.
"""
import numpy as np
import pytest

from conftest import observed
from oracle import rom_oracle as ro

pytestmark = pytest.mark.gpu

SNAP_TOL = 1e-11     # tests/test_gpu_parity.py
SWITCH_TOL = 1e-11   # test_algorithm_switches_agree

FUSED_SHAPES = [((2, 2), 128, 1), ((2, 2), 128, 3), ((2, 2), 128, 4), ((2, 2), 128, 5), ((2, 2), 128, 130),
                ((2, 2), 24, 7), ((1, 2), 32, 5)]
GENERAL_SHAPES = [((3, 3), 24, 40)]
M_MAX = 130


def parameters(blocks, N):
    """The M_MAX rows of a geometry; every case takes the first M of them, so the oracle rows are shared."""
    k = blocks[0] * blocks[1]
    a = 10.0 ** np.random.default_rng(1000 * k + N).uniform(0, 3, size=(M_MAX, k))
    a[0] = 1.0
    a[0, k - 1] = 1e8
    return a


_ORACLE = {}


def oracle_row(blocks, N, i):
    key = (blocks, N, i)
    if key not in _ORACLE:
        g = ro.Geometry(blocks, N)
        _ORACLE[key] = ro.generate_solutions(g, parameters(blocks, N)[i:i + 1].reshape(1, *blocks), "lsqsparse")[0]
    return _ORACLE[key]


def relh10(g, U, Uref):
    return ro.H10norm(g, np.asarray(U) - Uref) / ro.H10norm(g, Uref)


@pytest.fixture(scope="module")
def ctx():
    from romhighcontrast_amd import _ffi
    return _ffi.get_context()


def sweep(ctx, blocks, N, a):
    from romhighcontrast_amd import _ffi
    fem = _ffi.Fem(ctx, blocks[0], blocks[1], N)
    M = a.shape[0]
    U = ctx.alloc(M * fem.dim)
    fem.solve_batch(ctx.upload(a), M, U)
    return fem, U.download(shape=(M, fem.dim))


@pytest.mark.parametrize("blocks,N,M", FUSED_SHAPES + GENERAL_SHAPES)
def test_rows_against_oracle_and_unfused(ctx, blocks, N, M, monkeypatch):
    monkeypatch.delenv("ROMHC_NO_FUSED", raising=False)
    a = parameters(blocks, N)[:M]
    fem, ref = sweep(ctx, blocks, N, a)
    if N == 128:
        assert fem.n_tiles == 1  # the fused single-tile solve
    g = ro.Geometry(blocks, N)
    rows = sorted({0, M // 2, M - 1})
    Uo = np.stack([oracle_row(blocks, N, i) for i in rows])
    observed(f"solve1 chain {blocks} N={N} M={M}: rows {rows} vs the SuperLU oracle (rel H10)", relh10(g, ref[rows], Uo), SNAP_TOL)
    monkeypatch.setenv("ROMHC_NO_FUSED", "1")
    _, alt = sweep(ctx, blocks, N, a)
    monkeypatch.delenv("ROMHC_NO_FUSED", raising=False)
    observed(f"solve1 chain {blocks} N={N} M={M}: fused vs ROMHC_NO_FUSED=1 (rel H10)", relh10(g, alt, ref), SWITCH_TOL)


@pytest.mark.parametrize("blocks,N,M", FUSED_SHAPES)
def test_two_stage_equals_one_call(ctx, blocks, N, M):
    a = parameters(blocks, N)[:M]
    fem, ref = sweep(ctx, blocks, N, a)
    ab = ctx.upload(a)
    Y = ctx.alloc((M + 1) * fem.reduced_stride)
    Y.fill(float("nan"))  # whatever was in the buffer must not matter
    fem.solve_reduced(ab, M, Y, y_row0=1)
    U = ctx.alloc(M * fem.dim)
    fem.expand(ab, M, Y, U, y_row0=1)
    ctx.solve_status()
    assert np.array_equal(U.download(shape=(M, fem.dim)), ref)


def test_non_spd_is_reported(ctx):
    """One block coefficient negative and dominant (the interface matrix is indefinite), first and last system."""
    from romhighcontrast_amd import _ffi
    blocks, N, M = (2, 2), 128, 5
    a = parameters(blocks, N)[:M].copy()
    fem = _ffi.Fem(ctx, blocks[0], blocks[1], N)
    Y = ctx.alloc(M * fem.reduced_stride)
    for bad in (0, M - 1):
        ab = a.copy()
        ab[bad, 1] = -100.0 * a[bad].max()
        ad = ctx.upload(ab)
        assert ctx.lib.rom_solve_reduced_async(fem.h, ad.h, M, Y.h, 0) == _ffi.ROM_OK
        assert ctx.lib.rom_solve_status(ctx.h) == _ffi.ROM_ERR_NOT_SPD, bad
        ad = ctx.upload(a)
        assert ctx.lib.rom_solve_reduced_async(fem.h, ad.h, M, Y.h, 0) == _ffi.ROM_OK
        assert ctx.lib.rom_solve_status(ctx.h) == _ffi.ROM_OK, bad
