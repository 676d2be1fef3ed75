"""tests/sweep_truth.py proved on the CPU, before tests/test_gpu_sweep.py relies on it: the referee converges on every
parameter vector of every case, the SuperLU oracle sits ten times inside SNAP_TOL of the truth (so a GPU failure cannot be
blamed on the input), the batch patterns have the properties the bit comparison needs, and the restated routes cover their
table."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from oracle import rom_oracle as ro
import referee as rf
import sweep_truth as st

LD = np.longdouble
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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
    # blocks wider than one 128-vertex tile, by hand: n1 = 170 -- 340 row tiles against 226 flat ones; n1 = 139 -- 278 against
    # 151; n1 = 249 -- 498 against 485, 97.4 %: rows; n1 = 256 -- 512 against 512
    for n1, t_row, t_flat, tiling in ((170, 340, 226, "flat"), (139, 278, 151, "flat"), (249, 498, 485, "row"), (256, 512, 512, "row")):
        assert n1 * ((n1 + 127) // 128) == t_row and (n1 * n1 + 127) // 128 == t_flat
        assert (100 * t_flat < 97 * t_row) == (tiling == "flat")
        assert t(n1, 129) == t(n1, 1921) == tiling and t(n1, 127) == "t64"
    assert 97.3 < 100 * 485 / 498 < 97.5
    assert [st.CASE[c].N - 1 for c in st.WIDE_CASES] == [170, 139, 249, 256]
    # the case list holds a flat case with n1 >= 128 odd, one with n1 >= 128 even, and a row case with two column tiles
    wide = [(c.N - 1, t(c.N - 1, 129)) for c in st.CASES if c.N - 1 >= 128]
    assert any(tl == "flat" and n1 % 2 == 1 for n1, tl in wide)
    assert any(tl == "flat" and n1 % 2 == 0 for n1, tl in wide)
    assert any(tl == "row" and (n1 + 127) // 128 == 2 for n1, tl in wide)
    assert any(tl == "row" and (n1 + 127) // 128 == 2 and n1 % 128 for n1, tl in wide)          # ... whose second tile is ragged
    # what the table says about each case agrees with the restatement
    for c in st.CASES:
        tiles = {r for r in c.routes if r.startswith("extend_lr_")}
        if tiles:
            assert tiles == {"extend_lr_128_" + t(c.N - 1, 129)}, c.id
            assert "extend_lr_64" in st.narrow_routes(c.routes)


@pytest.fixture(scope="module")
def planned(tmp_path_factory):
    """{case id: {"tables": {...}, "paths": {...}}} of the wide cases and C2, from the stand-alone program
    tests/c_abi/fem_tables_check.cpp (AddressSanitizer and UBSan; nothing loaded into this process), built and run once."""
    gxx = shutil.which("g++")
    assert gxx, "g++ is part of the image"
    exe = str(tmp_path_factory.mktemp("fem_tables") / "fem_tables_check")
    csrc = os.path.join(ROOT, "romhighcontrast_amd", "csrc")
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I", os.path.join(ROOT, "include"), "-I", csrc, "-x", "c++",
           os.path.join(csrc, "rom_fem_plan.hip"), os.path.join(ROOT, "tests", "c_abi", "fem_tables_check.cpp"),
           "-lpthread", "-o", exe]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0, r.stdout.decode()
    ids = list(st.WIDE_CASES) + [st.C2_CASE]
    r = subprocess.run([exe] + ids, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    out, err = r.stdout.decode(), r.stderr.decode()
    print(out)
    assert r.returncode == 0 and err == "", out + err          # no sanitizer report
    lines = [ln.split() for ln in out.splitlines()]
    assert len(lines) == 2 * len(ids) and all(f[0] in ("tables", "paths") for f in lines), out
    rec = {cid: {} for cid in ids}
    for f in lines:
        rec[f[1]][f[0]] = dict(zip(f[2::2], (int(x) for x in f[3::2])))
    assert all(set(v) == {"tables", "paths"} for v in rec.values()), out
    return rec


def test_system_fast_order_restated(planned):
    """The workgroup order of k_extend128 (sweep_truth.system_fast_order) with the planner's own table sizes: 3x3-N140 holds
    66.0 MiB and switches at 16 system groups, i.e. from 1921 systems on; C2's 2x2-N128 holds 15.8 MiB and keeps the classic
    order at any batch size."""
    fast, c2 = st.CASE[st.SYS_FAST_CASE], st.CASE[st.C2_CASE]
    rec = {cid: v["tables"] for cid, v in planned.items()}
    for c in (fast, c2):
        p, q = c.blocks
        assert rec[c.id]["bytes"] == 8 * rec[c.id]["gstotal"] and rec[c.id]["n1"] == c.N - 1
        assert (rec[c.id]["lr"], rec[c.id]["gen"]) == (p * q, 0)            # every block compressed: one k_extend128 launch
    MiB = float(1 << 20)
    assert abs(rec[fast.id]["bytes"] / MiB - 66.0) < 0.05 and abs(rec[c2.id]["bytes"] / MiB - 15.8) < 0.05
    assert rec[fast.id]["T"] == 5 and rec[c2.id]["T"] == 1
    so = st.system_fast_order
    assert st.SYS_FAST_BYTES == 64 << 20 and st.SYS_FAST_GROUPS == 16 and st.SYS_FAST_M == 128 * 15 + 1
    assert so(rec[fast.id]["bytes"], st.SYS_FAST_M) and not so(rec[fast.id]["bytes"], st.SYS_FAST_M - 1)
    assert not any(so(rec[fast.id]["bytes"], M) for M in fast.Ms)           # the case's own batches run the classic order
    assert not any(so(rec[c2.id]["bytes"], M) for M in (129, 1921, 4096, 1 << 20))
    assert so(64 << 20, 1921) and not so((64 << 20) - 8, 1921) and not so(1 << 40, 1920)
    # the 1921-system sweep is one chunk (the default workspace limit is 24 GiB) and holds every parameter vector
    f = rec[fast.id]
    assert f["nGa"] == 64 * f["T"] and st.SYS_FAST_M * st.per_system_workspace(f["slots"], f["nGa"], f["nGp"]) < 24 << 30
    assert st.check_idx(st.idx_pattern(st.SYS_FAST_M, st.n_params(fast)), st.SYS_FAST_M, st.n_params(fast))
    # the table sizes of the other wide cases (MiB): only 3x3-N140 can switch
    assert [round(rec[cid]["bytes"] / MiB, 1) for cid in st.WIDE_CASES] == [28.2, 66.0, 60.5, 4.0]


def test_wide_cases_reach_their_paths(planned):
    """What the wide cases are in the table for, from x128_skip_counts (the function k_extend128 calls) over every tile and wave
    column of every block in the tiling enqueue_solve picks: the counts on the right are worked out by hand."""
    pa = {cid: planned[cid]["paths"] for cid in st.WIDE_CASES}
    tb = {cid: planned[cid]["tables"] for cid in st.WIDE_CASES}
    for cid in st.WIDE_CASES:
        c = st.CASE[cid]
        n1, kblk = c.N - 1, c.blocks[0] * c.blocks[1]
        flat = st.extension_tiling(n1, 129) == "flat"
        assert pa[cid]["tiling"] == int(flat) and (tb[cid]["lr"], tb[cid]["gen"]) == (kblk, 0)
        assert pa[cid]["tiles"] == kblk * ((n1 * n1 + 127) // 128 if flat else n1 * ((n1 + 127) // 128))
        assert pa[cid]["empty_waves"] == 0 and pa[cid]["more_rows"] == 0      # (n1 >= 128: a flat tile meets two mesh rows at most)
        assert pa[cid]["max_walk"] < 64                                        # the per-wave skipping is on (k_extend128: nseg < 64)
    a, b, c, d = (pa[cid] for cid in st.WIDE_CASES)
    # 2x2-N171 (n1 = 170 even): 226 flat tiles per block, 59 of them inside one mesh row (the one_row / w_one branches), one
    # of which skips a segment of side 2 or 3 as a whole tile; 170^2 = 225 x 128 + 100: the last tile's fourth wave holds 4
    assert (a["tiles"], a["one_row"], a["two_rows"], a["ragged_waves"]) == (904, 4 * 59, 4 * 167, 4) and a["one_row_skip23"] >= 1
    assert sum(1 for t in range(226) if (128 * t) // 170 == min(128 * t + 127, 170 * 170 - 1) // 170) == 59
    # 3x3-N140 (n1 = 139 odd): 151 tiles per block, 14 inside one mesh row; 139^2 = 150 x 128 + 121; pairs (2k, 2k + 1) straddle
    # two mesh rows wherever a row starts at an odd vertex: every second row
    assert (b["tiles"], b["one_row"], b["two_rows"], b["ragged_waves"]) == (1359, 9 * 14, 9 * 137, 9)
    assert sum(1 for t in range(151) if (128 * t) // 139 == min(128 * t + 127, 139 * 139 - 1) // 139) == 14
    assert sum(1 for i in range(1, 139) if (i * 139) % 2 == 1) == 69
    # 2x2-N250 (n1 = 249): two column tiles per mesh row, the second of 121 = 3 x 32 + 25 vertices: one ragged wave per mesh row
    assert (c["tiles"], c["ragged_waves"], c["one_row"], c["two_rows"]) == (4 * 249 * 2, 4 * 249, 0, 0)
    # 1x2-N257 (n1 = 256): two full column tiles, sides of one K chunk, a walk of one segment: nothing for a wave to skip
    assert (d["tiles"], d["ragged_waves"], d["wave_larger"], d["max_walk"]) == (2 * 256 * 2, 0, 0, 1) and tb["1x2-N257"]["lr_nch"] == 1
    for x in (a, b, c):
        assert x["wave_larger"] > 0                       # waves that skip more than their tile: the skip / no-skip comparison bites


def test_route_restatement_covers_its_table():
    """Every route of ROUTES is claimed by a case (at 129 systems or below 128) or by one of the four product switches (the
    fourth: 1921 systems of SYS_FAST_CASE), and routes_of_profile names exactly the routes of the table."""
    claimed = {"diag_update_single", "chunked", "chunk_reuse", "extend_128_sys_fast"}
    assert not any("extend_128_sys_fast" in c.routes for c in st.CASES)      # no batch of the case table reaches 16 system groups
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
    # the system-fast label counts as extend_lr for everything else
    assert rp(dict(tile, extend_lr_sysfast=1), 139, 1921, 9, True) == base | {"expand_folded", "extend_lr_128_flat", "extend_128_sys_fast"}
    assert rp(dict(tile, extend_lr=1), 139, 1921, 9, True) == base | {"expand_folded", "extend_lr_128_flat"}
    assert rp({"solve1": 1, "extend_lr_sysfast": 1}, 255, 4096, 16, True) == {"solve1", "expand_folded", "extend_lr_128_row", "extend_128_sys_fast"}
    assert rp({"solve1": 1, "extend_lr_sysfast": 0, "extend_lr": 1}, 170, 129, 4, True) == {"solve1", "expand_folded", "extend_lr_128_flat"}
    assert rp({"solve1": 1, "extend_lr": 1}, 127, 257, 4, False) == {"solve1", "extend_lr_128_row"}     # nothing to expand: no fold
    assert rp({"solve1": 1, "extend_lr": 0, "scatter_interface": 2, "back_pre": 1, "edge_transform": 1}, 6, 5, 0, True) \
        == {"solve1", "scatter_interface", "back_pre", "edge_transform"}
    assert st.chunks_of(700, 256) == [256, 256, 188] and st.chunks_of(257, 70) == [70, 70, 70, 47] and st.chunks_of(5, 70) == [5]
    assert st.per_system_workspace(1, 64, 640) == 2 * 4096 * 8 + 2 * 640 * 8      # the figure of test_workspace_chunking_and_streams
    assert st.narrow_routes(("solve1", "expand_folded", "extend_lr_128_row", "extend_128_multi_launch")) == ("expand", "extend_lr_64", "solve1")
