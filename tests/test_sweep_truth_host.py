"""tests/sweep_truth.py proved on the CPU, before tests/test_gpu_sweep.py relies on it: the referee converges on every
parameter vector of every case, the SuperLU oracle sits ten times inside SNAP_TOL of the truth (so a GPU failure cannot be
blamed on the input), the batch patterns have the properties the bit comparison needs, and the restated routes cover their
table."""
import numpy as np
import pytest

from oracle import rom_oracle as ro
import referee as rf
import sweep_truth as st

LD = np.longdouble


@pytest.mark.parametrize("case", st.CASES, ids=[c.id for c in st.CASES])
def test_truths_converge_and_the_oracle_is_inside_the_bound(case):
    t = st.truths(case)
    g, a = t["g"], t["a"]
    D = st.n_params(case)
    assert a.shape == (D, case.blocks[0] * case.blocks[1]) and a.min() >= 1.0 and a.max() <= 1e4
    assert len(np.unique(a, axis=0)) == D
    assert D == (4 if g.dim > 30000 else 8)
    Uo = ro.generate_solutions(g, a.reshape((D,) + case.blocks))
    for d in range(D):
        hist = t["hist"][d]
        assert hist[-1] < 1e-16 or (len(hist) > 1 and hist[-1] > 0.5 * hist[-2]), (d, hist)     # converged, or stalled
        assert min(hist) < 1e-16, (d, hist)                                                     # ... at the rounding level
        assert t["err_superlu"][d] <= st.ORACLE_TOL, (d, t["err_superlu"][d])
        e = st.rel_h10_ld(g, Uo[d], t["truth"][d])
        assert e <= st.ORACLE_TOL, (d, e)
        # the truth solves the system: what its rounding to fp64 leaves, |A| |u| 2^-53 <= 8 a_max |u|_inf 2^-53, is
        # 2 x 2^-53 in the normalisation of the all-distinct net
        assert st.residual_norm_ld(g, a[d], t["truth"][d]) < 4 * 2.0 ** -53
    assert st.truths(case) is t                                                                 # cached


def test_distinct_batches_are_distinct_and_a_wrong_row_shows():
    case = st.CASE["2x2-N16"]
    a = st.distinct_params(case)
    assert a.shape == (st.DISTINCT_M, 4) and np.array_equal(a, st.distinct_params(case))
    g = ro.Geometry(case.blocks, case.N)
    U = ro.generate_solutions(g, a[:3].reshape((3,) + case.blocks))
    assert st.residual_norm_ld(g, a[0], U[0]) < 1e-14
    assert st.residual_norm_ld(g, a[0], U[1]) > 1e3 * st.RESID_TOL      # another system's row
    bad = U[0].copy()
    bad[np.argmax(np.abs(bad))] *= 1 + 1e-6                              # one entry, six digits right
    assert st.residual_norm_ld(g, a[0], bad) > 10 * st.RESID_TOL
    assert st.rel_h10_ld(g, bad, U[0]) > 10 * st.SNAP_TOL


def test_idx_patterns():
    for D in (4, 8):
        for M in sorted(set(st.FULL_MS) | {700, 256, st.BIG_M, 6, 7, 8, 9}):
            idx = st.idx_pattern(M, D)
            assert st.check_idx(idx, M, D), (M, D)
            assert np.array_equal(idx, st.idx_pattern(M, D))
            if M >= D:
                assert sorted(set(idx.tolist())) == list(range(D))
            assert not (np.diff(idx) == 0).any()
    assert not st.check_idx([0, 1, 1, 2], 4, 3) and not st.check_idx([0, 1, 0, 1], 4, 3) and st.check_idx([0, 1, 2, 1], 4, 3)


def test_cases_cover_the_batch_edges():
    ids = [c.id for c in st.CASES]
    assert len(set(ids)) == len(ids)
    paths = {c.path for c in st.CASES}
    assert {"single_tile", "tile_cholesky", "closed_form"} <= paths
    for cid in st.FULL_CASES:
        assert st.CASE[cid].Ms == st.FULL_MS
    assert {st.CASE[c].path for c in st.FULL_CASES} == {"single_tile", "tile_cholesky"}
    for c in st.CASES:
        assert 129 in c.Ms and min(c.Ms) < 128 and c.row0 > 0
    assert st.CASE[st.BIG_CASE].path == "tile_cholesky" and st.BIG_M == 2049 and 257 in st.CASE[st.BIG_CASE].Ms
    assert 257 in st.CASE[st.C2_CASE].Ms and (st.CASE[st.C2_CASE].blocks, st.CASE[st.C2_CASE].N) == ((2, 2), 128)
    # the edges of FULL_MS: k_diag_update<2>'s last pair, k_solve1's last workgroup, 64- and 128-system tiles
    M = set(st.FULL_MS)
    assert {1, 2, 3} <= M and {1, 2, 3, 4, 5} <= M and {63, 64, 65, 127, 128, 129} <= M
    assert 257 % 128 == 1 and 193 % 128 == 65 and {193, 257} <= M


def test_extension_tiling_restated():
    t = st.extension_tiling
    # both sides of the Mc = 127 | 128 switch on every case; the three tilings all occur
    seen = set()
    for c in st.CASES:
        n1 = c.N - 1
        assert t(n1, 127) == "t64"
        for M in c.Ms:
            seen.add(t(n1, M))
        assert any(M < 128 for M in c.Ms) and any(M >= 128 for M in c.Ms)
    assert seen == {"t64", "row", "flat"}
    # the numbers behind it, by hand: n1 = 127 -- 127 row tiles, 127 flat tiles: no 3 % saved, rows; n1 = 15 -- 15 row tiles
    # against 2 flat ones; n1 = 64 / 65 -- 64 / 65 row tiles against 32 / 34 flat ones
    assert t(127, 128) == "row" and t(15, 128) == "flat" and t(64, 129) == "flat" and t(65, 129) == "flat"
    assert 100 * 127 >= 97 * 127 and (127 * 127 + 127) // 128 == 127
    # the 97 % rule flips between n1 = 124 (121 flat tiles, 97.6 %: rows) and 123 (119, 96.7 %: flat)
    assert (t(123, 128), t(124, 128)) == ("flat", "row")
    # the 102 % padding rule turns away only n1 = 1 (one 128-tile for one vertex against one 64-tile)
    assert t(1, 128) == "t64" and all(t(n1, 128) != "t64" for n1 in range(2, 300))
    # what the table says about each case agrees with the restatement
    for c in st.CASES:
        tiles = {r for r in c.routes if r.startswith("extend_lr_")}
        if tiles:
            assert tiles == {"extend_lr_128_" + t(c.N - 1, 129)}, c.id
            assert "extend_lr_64" in st.narrow_routes(c.routes)


def test_route_restatement_covers_its_table():
    """Every route of ROUTES is claimed by a case (at 129 systems or below 128) or by one of the three product switches, and
    routes_of_profile names exactly the routes of the table."""
    claimed = {"diag_update_single", "chunked", "chunk_reuse"}
    for c in st.CASES:
        assert set(c.routes) <= set(st.ROUTES), c.id
        claimed |= set(c.routes) | set(st.narrow_routes(c.routes))
    assert claimed == set(st.ROUTES), sorted(set(st.ROUTES) ^ claimed)
    rp = st.routes_of_profile
    tile = {"rhs": 1, "diag_update_j00": 1, "diag_update_j01": 1, "diag_factor_j00": 1, "diag_factor_j01": 1, "factor_panel_j00": 1,
            "backsolve": 1, "coef": 1}
    base = {"rhs", "diag_update", "diag_factor", "factor_panel", "backsolve", "coef"}
    assert rp(dict(tile, extend_lr=1), 39, 129, 6, True) == base | {"expand_folded", "extend_lr_128_flat"}
    assert rp(dict(tile, extend_lr=1, expand=1), 39, 65, 6, True) == base | {"expand", "extend_lr_64"}
    assert rp(dict(tile, extend_lr=1), 32, 129, 20, True) == base | {"expand_folded", "extend_lr_128_flat", "extend_128_multi_launch"}
    assert rp(dict(tile, extend=1, expand=1), 23, 2049, 0, True) == base | {"expand", "extend", "diag_update_single"}
    assert rp({"solve1": 1, "extend_lr": 1}, 127, 257, 4, True) == {"solve1", "expand_folded", "extend_lr_128_row"}
    assert rp({"solve1": 1, "extend_lr": 1}, 127, 257, 4, False) == {"solve1", "extend_lr_128_row"}     # nothing to expand: no fold
    assert rp({"solve1": 1, "extend_lr": 0, "scatter_interface": 2, "back_pre": 1, "edge_transform": 1}, 6, 5, 0, True) \
        == {"solve1", "scatter_interface", "back_pre", "edge_transform"}
    assert st.chunks_of(700, 256) == [256, 256, 188] and st.chunks_of(257, 70) == [70, 70, 70, 47] and st.chunks_of(5, 70) == [5]
    assert st.per_system_workspace(1, 64, 640) == 2 * 4096 * 8 + 2 * 640 * 8      # the figure of test_workspace_chunking_and_streams
    assert st.narrow_routes(("solve1", "expand_folded", "extend_lr_128_row", "extend_128_multi_launch")) == ("expand", "extend_lr_64", "solve1")
