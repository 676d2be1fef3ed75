"""The snapshot sweep -- rom_solve_batch and its two stages rom_solve_reduced_async / rom_expand_batch_async -- against
80-bit truths on an MI355X: every row, every route, every batch edge (cases, truths and route restatement:
tests/sweep_truth.py, proved on the CPU by tests/test_sweep_truth_host.py).

* A batch of M systems is built from D = 8 (4 at dim > 30 000) distinct parameter vectors 10^U(0, 4), each with a truth from
  tests/referee.py (SuperLU + refinement with long-double edge-form residuals).  (a) Rows of equal parameters are equal BIT
  FOR BIT wherever they sit in the batch -- and equal to the rows of the same parameters in every other batch size, chunking
  and stage split of the geometry; (b) one row per parameter vector is within SNAP_TOL = 1e-11 of its truth in relative
  H^1_0, evaluated in long double: together every row of every batch is checked against a truth.  The summary lines begin
  with `sweep `; the line ending in [reference] is the SuperLU oracle's own distance from the same truths.  (c) U sits at
  row0 > 0 of a larger buffer whose other rows hold a NaN with a payload, compared by bits afterwards; so does Y in the
  two-stage form, whose nodal part is overwritten with NaN before the expansion (which writes it and must not read it).
* M = 1 ... 257 on both sides of the pair of k_diag_update<2>, the four systems of a k_solve1 workgroup, every 64- and
  128-system tile and the Mc >= 128 switch, on a single-tile geometry and two tile Cholesky ones (general blocks; compressed
  blocks through k_extend128); 129 and a size below 128 on the others.
* Blocks wider than one 128-vertex tile (sweep_truth.WIDE_CASES, n1 = 170 / 139 / 249 / 256): flat tiles inside one mesh row
  with n1 even and odd, row tiles with two column tiles (the second ragged, or exactly full), the longer K walks of C4 and C5.
* Product switches the product build takes by size: 2049 systems (k_diag_update<1>), a workspace limit of 70 systems, a
  sweep of 700 after one of 256 on the same FE space (chunks of 256 + 256 + 188), 1921 systems of 3x3-N140 (tables of
  66 MiB and 16 system groups: k_extend128 with the system group varying fastest).
* 257 all-different systems (129 at dim 249 001): the long-double residual of EVERY row, |r|_inf / (4 a_max |u|_inf) <= 1e-11
  (the bound and normalisation of test_full_size_c2_properties).
* One indefinite system, first or last of five: ROM_ERR_NOT_SPD once, then ROM_OK and the same bits as before.
* The same bits with ROMHC_POISON_WS=1 on a fresh FE space.
* sweep_truth.ROUTES: tests/sweep_child.py confirms the route table from profile names in a child process;
  test_route_table_is_covered fails if the module was run in part.
"""
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest

from conftest import observed
import sweep_truth as st

pytestmark = pytest.mark.gpu

COVERED = set()
RAN = set()
_ID = [c.id for c in st.CASES]


@pytest.fixture(scope="module")
def ctx():
    from romhighcontrast_amd import _ffi
    return _ffi.get_context()


def _fresh(ctx, case):
    from romhighcontrast_amd import _ffi
    return _ffi.Fem(ctx, case.blocks[0], case.blocks[1], case.N)


@pytest.fixture(scope="module")
def fems(ctx):
    """One _ffi.Fem per case, created on first use and shared by the tests that do not ask for a fresh one."""
    cache = {}

    def get(case):
        if case.id not in cache:
            cache[case.id] = _fresh(ctx, case)
        return cache[case.id]
    return get


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


class Guarded:
    """M rows of `width` doubles at row `lead` of a device buffer of lead + M + 2 rows (and three more doubles) filled with
    the sentinel."""

    def __init__(self, ctx, lead, M, width):
        self.lead, self.M, self.width = lead, M, width
        self.buf = ctx.upload(np.full((lead + M + 2) * width + 3, st.SENTINEL))

    def rows(self, what):
        """The window (M, width); asserts that every entry around it kept its bits."""
        got = self.buf.download()
        bits = got.view(np.uint64)
        lo, hi = self.lead * self.width, (self.lead + self.M) * self.width
        assert (bits[:lo] == st.SENT_BITS).all(), f"{what}: an entry in front of row {self.lead} changed"
        assert (bits[hi:] == st.SENT_BITS).all(), f"{what}: an entry behind row {self.lead + self.M - 1} changed"
        return got[lo:hi].reshape(self.M, self.width)


def _batch(case, M):
    idx = st.idx_pattern(M, st.n_params(case))
    return st.params(case)[idx], idx


def _sweep(ctx, fem, a_rows, row0, what):
    M = len(a_rows)
    U = Guarded(ctx, row0, M, fem.dim)
    fem.solve_batch(ctx.upload(a_rows), M, U.buf, row0=row0)
    rows = U.rows(what)
    assert np.isfinite(rows).all(), f"{what}: a row is not finite (or was not written)"
    return rows


def _assert_equal_parameters_equal_bits(rows, idx, what):
    """(a): every row equals, bit for bit, the first row of the batch with the same parameters."""
    first = {}
    for m, d in enumerate(idx.tolist()):
        first.setdefault(d, m)
    ref = rows[[first[d] for d in idx.tolist()]]
    eq = (rows.view(np.uint64) == ref.view(np.uint64)).all(axis=1)
    bad = np.flatnonzero(~eq)
    assert not bad.size, f"{what}: rows {bad[:12].tolist()} (of {bad.size}) differ from the first row of the same parameters " \
                         f"(rows {[first[int(idx[m])] for m in bad[:12]]})"


_ref_rows = {}


def _reference_rows(ctx, fems, case):
    """One row per parameter vector, (D, dim), from the largest sweep of the case's list on the shared FE space (after (a) on
    that sweep): what every other batch size, chunking and stage split of the case must reproduce bit for bit."""
    if case.id not in _ref_rows:
        M = max(case.Ms)
        a_rows, idx = _batch(case, M)
        rows = _sweep(ctx, fems(case), a_rows, case.row0, f"{case.id} M={M}")
        _assert_equal_parameters_equal_bits(rows, idx, f"{case.id} M={M}")
        D = st.n_params(case)
        _ref_rows[case.id] = np.stack([rows[np.flatnonzero(idx == d)[0]] for d in range(D)])
    return _ref_rows[case.id]


def _assert_reference_bits(ctx, fems, case, rows, idx, what):
    ref = _reference_rows(ctx, fems, case)
    eq = (rows.view(np.uint64) == ref[idx].view(np.uint64)).all(axis=1)
    bad = np.flatnonzero(~eq)
    assert not bad.size, f"{what}: rows {bad[:12].tolist()} (of {bad.size}) differ from the rows of the same parameters in the " \
                         f"one-call sweep of {max(case.Ms)} systems"


# =====================================================================================================================
# 1. every batch size of every case: (a) equal bits, (b) distance from the truth, (c) guard bands
# =====================================================================================================================
@pytest.mark.parametrize("cid,M", [(c.id, M) for c in st.CASES for M in c.Ms], ids=lambda v: str(v))
def test_sweep_rows_against_truth(ctx, fems, cid, M):
    case = st.CASE[cid]
    fem = fems(case)
    assert (fem.n_tiles == 1) == (case.path == "single_tile") and (fem.n_tiles > 1) == (case.path == "tile_cholesky")
    t0 = time.perf_counter()
    a_rows, idx = _batch(case, M)
    what = f"{cid} M={M}"
    rows = _sweep(ctx, fem, a_rows, case.row0, what)
    t_gpu = time.perf_counter() - t0
    _assert_equal_parameters_equal_bits(rows, idx, what)
    _assert_reference_bits(ctx, fems, case, rows, idx, what)
    t = st.truths(case)
    present = sorted(set(idx.tolist()))
    last = {d: int(np.flatnonzero(idx == d)[-1]) for d in present}
    err = [st.rel_h10_ld(t["g"], rows[last[d]], t["truth"][d]) for d in present]
    print(f"[sweep] {what}: upload + sweep + download + guard bands {t_gpu:.2f} s, whole case {time.perf_counter() - t0:.2f} s")
    observed(f"sweep {cid}: SuperLU oracle vs 80-bit truth, the same parameters (rel H10) [reference]", t["err_superlu"][present], st.ORACLE_TOL)
    observed(f"sweep {cid} M={M}: one row per parameter vector vs 80-bit truth (rel H10)", err, st.SNAP_TOL)
    RAN.add("rows")


# =====================================================================================================================
# 2. two stages: halves solved in swapped order into Y at row 3, nodal part destroyed, expanded at row 2
# =====================================================================================================================
@pytest.mark.parametrize("cid", _ID)
def test_two_stage_sweep(ctx, fems, cid):
    """(3x3-N24 is the regression case of a defect this test found: k_expand reads its K in chunks of 16, and the last chunk
    of the last edge group of the reduced part -- 188 unknowns in a part of 192, ranks of 23 read as 32 -- reached up to five
    entries into the nodal part, against zero table columns: harmless with finite leftovers, NaN rows with NaN ones.)"""
    case = st.CASE[cid]
    fem = fems(case)
    M = 129
    a_rows, idx = _batch(case, M)
    stride = fem.reduced_stride
    nb, ne = st.nodal_part(fem)
    assert 0 <= nb <= ne <= stride
    Y = Guarded(ctx, 3, M, stride)
    h = M // 2
    fem.solve_reduced(ctx.upload(a_rows[h:]), M - h, Y.buf, y_row0=3 + h)
    fem.solve_reduced(ctx.upload(a_rows[:h]), h, Y.buf, y_row0=3)
    ctx.solve_status()
    Yh = Y.rows(f"{cid}: Y after solve_reduced").copy()
    cols = fem.reduced_inputs
    assert np.isfinite(Yh[:, cols]).all()
    _assert_equal_parameters_equal_bits(np.ascontiguousarray(Yh[:, cols]), idx, f"{cid}: what the expansion reads of the interface vectors")
    if ne > nb:      # the expansion writes the nodal part and must never read it
        Yh[:, nb:ne] = np.nan
        Y.buf.upload(Yh, offset=3 * stride)
    U = Guarded(ctx, 2, M, fem.dim)
    fem.expand(ctx.upload(a_rows), M, Y.buf, U.buf, y_row0=3, row0=2)
    ctx.solve_status()
    rows = U.rows(f"{cid}: U after expand")
    assert np.isfinite(rows).all()
    Y2 = Y.rows(f"{cid}: Y after expand")
    assert same_bits(np.ascontiguousarray(Y2[:, cols]), np.ascontiguousarray(Yh[:, cols])), "the expansion changed its own inputs"
    _assert_reference_bits(ctx, fems, case, rows, idx, f"{cid}: two stages")
    RAN.add("two_stage")


# =====================================================================================================================
# 3. the switches the product build takes by size
# =====================================================================================================================
def test_more_than_2048_systems(ctx, fems):
    """2049 systems on a fresh FE space: the first size at which the tile Cholesky runs k_diag_update<1>.  Every row equals the
    row of the same parameters of the 257-system sweep."""
    case = st.CASE[st.BIG_CASE]
    t0 = time.perf_counter()
    a_rows, idx = _batch(case, st.BIG_M)
    what = f"{case.id} M={st.BIG_M}"
    rows = _sweep(ctx, _fresh(ctx, case), a_rows, case.row0, what)
    _assert_equal_parameters_equal_bits(rows, idx, what)
    _assert_reference_bits(ctx, fems, case, rows, idx, what)
    print(f"[sweep] {what}: {time.perf_counter() - t0:.2f} s")
    RAN.add("big")


def test_system_fast_order_gives_the_same_rows(ctx, fems):
    """1921 systems of 3x3-N140 on a fresh FE space: 16 system groups (the last holds one system) over tables of 66.0 MiB, the
    smallest switch to k_extend128's system-fast workgroup order (tests/sweep_child.py witnesses the order).  Placement only:
    every row equals, bit for bit, the row of the same parameters of the classic-order sweep of 129 systems.  The block is
    2.7 GB: it is filled with the sentinel and compared on the device, in slabs of 128 rows."""
    case = st.CASE[st.SYS_FAST_CASE]
    M, row0 = st.SYS_FAST_M, case.row0
    assert M > max(case.Ms) and (M + 127) // 128 == st.SYS_FAST_GROUPS and M % 128 == 1
    t0 = time.perf_counter()
    ref = _reference_rows(ctx, fems, case)
    D, dim = ref.shape
    ref_d = ctx.upload(ref)
    a_rows, idx = _batch(case, M)
    assert st.check_idx(idx, M, D)
    fem = _fresh(ctx, case)
    assert dim == fem.dim
    U = ctx.alloc((row0 + M + 2) * dim + 3)
    U.fill(st.SENTINEL)
    fem.solve_batch(ctx.upload(a_rows), M, U, row0=row0)
    what = f"{case.id} M={M}"
    front = U.download(n=row0 * dim).view(np.uint64)
    behind = U.download(offset=(row0 + M) * dim).view(np.uint64)
    assert front.size == row0 * dim and (front == st.SENT_BITS).all(), f"{what}: an entry in front of row {row0} changed"
    assert behind.size == 2 * dim + 3 and (behind == st.SENT_BITS).all(), f"{what}: an entry behind row {row0 + M - 1} changed"
    want = ctx.alloc(128 * dim)
    bad = []
    for m0 in range(0, M, 128):
        n = min(128, M - m0)
        want.gather_rows_from(ref_d, idx[m0:m0 + n], dim)
        if not U.same_bits_as(want, n * dim, off=(row0 + m0) * dim):
            got = U.download(n=n * dim, offset=(row0 + m0) * dim, shape=(n, dim))
            eq = (got.view(np.uint64) == ref[idx[m0:m0 + n]].view(np.uint64)).all(axis=1)
            bad += (m0 + np.flatnonzero(~eq)).tolist()
    assert not bad, f"{what}: rows {bad[:12]} (of {len(bad)}) differ from the rows of the same parameters in the classic-order " \
                    f"sweep of {max(case.Ms)} systems"
    t = st.truths(case)
    last = [int(np.flatnonzero(idx == d)[-1]) for d in range(D)]
    err = [st.rel_h10_ld(t["g"], U.download(n=dim, offset=(row0 + m) * dim), t["truth"][d]) for d, m in enumerate(last)]
    print(f"[sweep] {what}: {time.perf_counter() - t0:.2f} s")
    observed(f"sweep {case.id} M={M} (system-fast order): one row per parameter vector vs 80-bit truth (rel H10)", err, st.SNAP_TOL)
    RAN.add("sys_fast")


@pytest.mark.parametrize("cid", st.CHUNK_CASES)
def test_later_larger_sweep_reuses_the_workspace_in_chunks(ctx, fems, cid):
    """256 systems, then 700 on the same FE space: the second runs as 256 + 256 + 188.  The bits of an unchunked sweep of the
    same batch on a fresh FE space."""
    case = st.CASE[cid]
    fem = _fresh(ctx, case)
    a256, idx256 = _batch(case, 256)
    rows = _sweep(ctx, fem, a256, case.row0, f"{cid} M=256")
    _assert_reference_bits(ctx, fems, case, rows, idx256, f"{cid} M=256")
    a700, idx700 = _batch(case, 700)
    rows = _sweep(ctx, fem, a700, case.row0, f"{cid} M=700 in chunks of 256")
    _assert_equal_parameters_equal_bits(rows, idx700, f"{cid} M=700 in chunks of 256")
    whole = _sweep(ctx, _fresh(ctx, case), a700, case.row0, f"{cid} M=700")
    assert same_bits(rows, whole), "chunks of 256 + 256 + 188 and one chunk of 700 differ"
    _assert_reference_bits(ctx, fems, case, rows, idx700, f"{cid} M=700")
    RAN.add("chunk_reuse")


@pytest.mark.parametrize("cid", st.CHUNK_CASES)
def test_workspace_limit_of_70_systems(ctx, fems, cid):
    """257 systems in chunks of 70 + 70 + 70 + 47 (no multiple of a tile; every chunk below the k_extend128 switch)."""
    case = st.CASE[cid]
    fem = _fresh(ctx, case)
    per_sys = st.per_system_workspace(fem.n_tiles, st.nodal_part(fem)[0], fem.reduced_stride)
    a_rows, idx = _batch(case, 257)
    ctx.set_workspace_limit(70 * per_sys)
    try:
        rows = _sweep(ctx, fem, a_rows, case.row0, f"{cid} M=257 in chunks of 70")
    finally:
        ctx.set_workspace_limit(24 << 30)
    _assert_equal_parameters_equal_bits(rows, idx, f"{cid} M=257 in chunks of 70")
    whole = _sweep(ctx, _fresh(ctx, case), a_rows, case.row0, f"{cid} M=257")
    assert same_bits(rows, whole), "chunks of 70 and one chunk of 257 differ"
    _assert_reference_bits(ctx, fems, case, rows, idx, f"{cid} M=257 in chunks of 70")
    RAN.add("chunked")


# =====================================================================================================================
# 4. all parameter vectors different: the residual of every row
# =====================================================================================================================
@pytest.mark.parametrize("cid", st.DISTINCT_CASES)
def test_all_distinct_batch_residuals(ctx, fems, cid):
    case = st.CASE[cid]
    a = st.distinct_params(case)
    rows = _sweep(ctx, fems(case), a, case.row0, f"{cid} all distinct")
    g = st.truths(case)["g"]
    res = [st.residual_norm_ld(g, a[m], rows[m]) for m in range(len(a))]
    observed(f"sweep {cid} M={len(a)} all distinct: long-double residual of every row, |r|_inf / (4 a_max |u|_inf)", res, st.RESID_TOL)
    RAN.add("distinct")


# =====================================================================================================================
# 5. error status
# =====================================================================================================================
@pytest.mark.parametrize("cid", st.CHUNK_CASES)
def test_sweep_reports_an_indefinite_system_once(ctx, fems, cid):
    """One block coefficient of one system negative (and dominant: the interface matrix is indefinite), at index 0 and at index
    M - 1: rom_solve_batch returns ROM_ERR_NOT_SPD; the SPD sweep that follows returns ROM_OK (the status word is reset) and
    gives the bits of the reference rows.  (3x3-N24 is a regression case: the failed sweep leaves NaN in the nodal part of
    the internal interface vectors, and the expansion of the NEXT sweep read some of those entries -- see
    test_two_stage_sweep -- so that its first row came back wrong under ROM_OK.)"""
    from romhighcontrast_amd import _ffi
    case = st.CASE[cid]
    fem = fems(case)
    M = 5
    a_rows, idx = _batch(case, M)
    for bad in (0, M - 1):
        ab = a_rows.copy()
        ab[bad, 0 if bad == 0 else -1] = -100.0 * a_rows[bad].max()
        U = Guarded(ctx, case.row0, M, fem.dim)
        ad = ctx.upload(ab)                                     # (held in a name: the raw call below takes the handle only)
        status = ctx.lib.rom_solve_batch(fem.h, ad.h, M, U.buf.h, case.row0)
        assert status == _ffi.ROM_ERR_NOT_SPD and b"not positive definite" in ctx.lib.rom_last_error(), (bad, status)
        U.rows(f"{cid}: indefinite system at {bad}")
        U = Guarded(ctx, case.row0, M, fem.dim)
        ad = ctx.upload(a_rows)
        assert ctx.lib.rom_solve_batch(fem.h, ad.h, M, U.buf.h, case.row0) == _ffi.ROM_OK, bad
        _assert_reference_bits(ctx, fems, case, U.rows(f"{cid}: after the failure"), idx, f"{cid}: SPD sweep after a failure at {bad}")
    RAN.add("status")


# =====================================================================================================================
# 6. poisoned workspace
# =====================================================================================================================
@pytest.mark.parametrize("cid", ["2x2-N16", "3x3-N24", "2x3-N40", "1x2-N128", "2x2-N171"])
def test_poisoned_workspace_gives_the_same_bits(ctx, fems, cid, monkeypatch):
    """ROMHC_POISON_WS=1 fills the factor workspace of a fresh FE space with NaN patterns before its first sweep."""
    case = st.CASE[cid]
    a_rows, idx = _batch(case, 129)
    monkeypatch.setenv("ROMHC_POISON_WS", "1")
    rows = _sweep(ctx, _fresh(ctx, case), a_rows, case.row0, f"{cid} poisoned")
    monkeypatch.delenv("ROMHC_POISON_WS")
    _assert_reference_bits(ctx, fems, case, rows, idx, f"{cid}: poisoned workspace")
    RAN.add("poison")


# =====================================================================================================================
# 7. routes
# =====================================================================================================================
def test_routes_confirmed_by_profile_names():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, ROMHC_PROF_DETAIL="1")
    r = subprocess.run([sys.executable, os.path.join(root, "tests", "sweep_child.py")], env=env, cwd=root,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    out = r.stdout.decode(errors="replace")
    assert r.returncode == 0 and out.rstrip().endswith("OK"), out[-4000:]
    got = json.loads([ln for ln in out.splitlines() if ln.startswith("ROUTES ")][-1][7:])
    for case in st.CASES:
        rec = got[case.id]
        assert rec["seen"] == rec["want"] == sorted(case.routes), (case.id, rec)
        assert rec["seen_small"] == rec["want_small"], (case.id, rec)
        COVERED.update(rec["seen"], rec["seen_small"])
    assert "diag_update_single" in got["big"]["seen"] and got["big"]["launches"] == 1, got["big"]
    COVERED.add("diag_update_single")
    fast = got["sys_fast"]        # the order is read from the label extend_lr_sysfast, which only that sweep may carry
    assert "extend_128_sys_fast" in fast["seen"] and "extend_lr_sysfast" in fast["profile"] and "extend_lr" not in fast["profile"], fast
    assert fast["M"] == st.SYS_FAST_M and fast["launches"] == 1, fast      # (one chunk: 16 system groups)
    assert sorted(set(fast["seen"]) - {"extend_128_sys_fast"}) == sorted(st.CASE[st.SYS_FAST_CASE].routes), fast
    assert not any("extend_lr_sysfast" in got[c.id]["profile"] + got[c.id]["profile_small"] for c in st.CASES)
    COVERED.add("extend_128_sys_fast")
    for cid in st.CHUNK_CASES:
        for key in ("chunked", "chunk_reuse"):
            assert got[f"{key} {cid}"]["seen"] == [key], (cid, got[f"{key} {cid}"])
            COVERED.add(key)
    COVERED.add("_confirmed")


def test_route_table_is_covered():
    assert "_confirmed" in COVERED, "run the whole module: the child-process confirmation did not run"
    assert set(st.ROUTES) <= COVERED, sorted(set(st.ROUTES) - COVERED)
    want = {"rows", "two_stage", "big", "sys_fast", "chunk_reuse", "chunked", "distinct", "status", "poison"}
    assert want <= RAN, f"run the whole module: {sorted(want - RAN)} did not run"
