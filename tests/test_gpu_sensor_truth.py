"""The point-sensor stage (rom_riesz_h10, rom_riesz_norms_h10, rom_sensor_greedy, select_sensors_pbdw) on an MI355X
against the 80-bit truth of tests/sensor_truth.py (bounds: its module docstring; C = 64, eps = 2^-53; the fp64 NumPy
restatement sits 8x inside every one of them on the CPU, tests/test_sensor_truth_host.py).

* representers, G and squared norms on four grids (7 x 7, 15 x 15, 23 x 15, 71 x 47 across a 64-row tile), npts in
  {1, 17, 65}, every point family; boundary points give exact zeros, G is symmetric to the bit, the Gram-only call gives
  the same bits;
* the split launch of the second representer transform: the 3 x 3 grid with 1 398 081 points (nr npts > 65 535 x 64), which
  is also kr_spectral's stride over more than 65 535 points;
* the greedy, both modes, following the device's picks and alpha: the n routes of the worst-case eigen-solver (1, 2, 32,
  33, 96), n = 128 collective, the refusals of 97 / 129, m in {1, 2, 5, 260}, ncand in {1, 255, 256, 257}, more than
  1024 argmax partials (first occurrence of cyclically repeated points; boundary points in front), dead basis rows first,
  in the middle and last (dead_rows, exact zero columns of A and alpha, beta through select_sensors_pbdw), an all-dead
  basis, a row offset between NaN-payload guard rows, the rel_tol stop as an exact prefix, identical bits on a repeat call
  and under ROMHC_POISON_WS on a fresh FE space;
* ROUTES: tests/sensor_child.py confirms from profile names what names can show; test_route_table_is_covered asserts
  that every route was reached.
With ROMHC_SENSOR_TRUTH_JSON set, every case's observed / bound ratios are appended to that file as "device" lines
(profiles/sensor_truth.json is such a run next to the restatement's).
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import h10_truth as ht
import sensor_truth as st
from sweep_truth import SENTINEL

pytestmark = pytest.mark.gpu

LD = st.LD
ROUTES = {
    "eig_jacobi32": "worst-case mode, n <= 32: the one-wave eigen-solver",
    "eig_lds": "worst-case mode, 33 <= n <= 96: the LDS eigen-solver (ks_select copies its last row)",
    "collective_n128": "collective mode at its largest n",
    "refusals": "n = 97 (worst case) and n = 129 (collective) are refused",
    "prep_beyond_256": "ks_prep's stride over a Cholesky row longer than 256; the unrolled Phi recurrence at that depth",
    "two_workgroups": "more than 256 candidates: partials of more than one workgroup, the last one partial",
    "select_walk": "more than 1024 partials: ks_select's per-thread ascending walk and its tie rule across threads",
    "dead_rows": "dead basis rows: the 2.0 on the diagonal of A^T A, zero columns, n - dead_rows",
    "row_offset": "c_row0 > 0 between guard rows",
    "rel_tol_stop": "the rel_tol stop",
    "split_transform": "a second riesz_transform_c launch (nr npts > 65 535 x 64)",
    "spectral_stride": "kr_spectral's stride over more than 65 535 points",
}
COVERED = set()
SPLIT_NPTS, SPLIT_BASE = 1_398_081, 4_099
WALK_BASE, WALK_FRONT = 509, 262_144
_SM = {}


def _sm(blocks, N, fresh=False):
    from romhighcontrast_amd.lib.SolutionsManagers import SolutionsManagerFEM
    key = (tuple(blocks), N)
    if fresh:
        return SolutionsManagerFEM(*key)
    if key not in _SM:
        sm = SolutionsManagerFEM(*key)
        gr = ht.grid(*key)
        assert np.array_equal(sm.points_c, gr.g.points_c) and np.array_equal(sm.points_r, gr.g.points_r)
        assert (sm.nr_inner_vertices, sm.nc_inner_vertices) == (gr.nr, gr.nc)
        _SM[key] = sm
    return _SM[key]


def hold(tag, measures):
    """Every measure of the case at most its bound; exact ones (bound 0) exactly; all of them recorded."""
    st.hold("device", tag, measures, 1.0)


def _bits(x):
    return None if x is None else np.ascontiguousarray(x).view(np.uint64 if x.dtype == np.float64 else x.dtype)


def same_bits(r1, r2):
    return all((x is None and y is None) or np.array_equal(_bits(x), _bits(y)) for x, y in zip(r1[:4], r2[:4])) and r1[4] == r2[4]


# ---- representers, G, norms ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("npts", (1, 17, 65))
@pytest.mark.parametrize("blocks,N", st.GRIDS, ids=[f"{b[0]}x{b[1]}_N{N}" for b, N in st.GRIDS])
def test_points_against_truth(blocks, N, npts):
    gr, sm = ht.grid(blocks, N), _sm(blocks, N)
    pt = st.PointTruth(gr, st.point_set(gr, npts, seed=npts + N))
    for a, b in zip(pt.loc, sm._locate(pt.pts)):
        assert np.array_equal(a, b)
    Ob = sm._ctx.alloc(npts * gr.dim)
    G = sm._fem.riesz_h10(*pt.loc, OMEGA=Ob, gram=True)
    Om = Ob.download(npts * gr.dim, shape=(npts, gr.dim))
    nu = sm._fem.riesz_norms_h10(*pt.loc)
    hold(f"points {gr.nr}x{gr.nc} npts={npts}", st.check_points(pt, Om, G, nu))
    G2 = sm._fem.riesz_h10(*pt.loc, OMEGA=None, gram=True)
    assert np.array_equal(_bits(G), _bits(G2)), "the Gram-only call must give the same bits"
    if npts > 2:    # the last point repeats the first: the same bits in every output
        assert np.array_equal(_bits(Om[-1]), _bits(Om[0])) and np.array_equal(_bits(G[-1]), _bits(G[0])) and nu[-1] == nu[0]


def run_split(sm, gr):
    """The size case of the split launch: (pt of the base set, reps, OMEGA rows)."""
    pt = st.PointTruth(gr, st.point_set(gr, SPLIT_BASE, seed=5))
    reps = np.arange(SPLIT_NPTS) % SPLIT_BASE
    assert gr.nr * SPLIT_NPTS > st.RZ_MAX_ROWS and SPLIT_NPTS > 65535
    Ob = sm._ctx.alloc(SPLIT_NPTS * gr.dim)
    assert sm._fem.riesz_h10(*[a[reps] for a in pt.loc], OMEGA=Ob, gram=False) is None
    return pt, reps, Ob.download(SPLIT_NPTS * gr.dim, shape=(SPLIT_NPTS, gr.dim))


def test_split_launch_of_the_representer_transform():
    gr, sm = ht.grid(*st.SIZE_GRID), _sm(*st.SIZE_GRID)
    pt, reps, Om = run_split(sm, gr)
    assert pt.zero.any() and not pt.zero.all()
    worst, zeros = 0.0, 0.0
    for r0 in range(0, SPLIT_NPTS, 1 << 17):
        idx = reps[r0:r0 + (1 << 17)]
        err = np.asarray(np.sqrt(np.sum((Om[r0:r0 + len(idx)].astype(LD) - pt.Om[idx]) ** 2, axis=1)), dtype=np.float64)
        live = ~pt.zero[idx]
        worst = max(worst, float(np.max(err[live] / pt.row_bound[idx][live])))
        zeros = max(zeros, float(np.abs(Om[r0:r0 + len(idx)][~live]).max(initial=0.0)))
    hold(f"split transform 3x3 npts={SPLIT_NPTS}", [("representers: row error / riesz_bound of the base point", worst, 1.0),
                                                    ("representers of vanishing functionals: max |entry|", zeros, 0.0)])
    COVERED.update({"split_transform", "spectral_stride"})


# ---- the greedy ------------------------------------------------------------------------------------------------------------
def run_case(sm, tr, case, mode, c_row0=0, Cb=None, m=None, rel_tol=None):
    Cb = Cb if Cb is not None else sm._ctx.upload(np.ascontiguousarray(tr.Cm))
    return sm._fem.sensor_greedy(Cb, tr.n, *tr.pt.loc, case["m"] if m is None else m, mode,
                                 case["rel_tol"] if rel_tol is None else rel_tol, c_row0=c_row0)


CASE_MODES = [(c, mode) for c in st.GREEDY_CASES for mode in c["modes"]]


@pytest.mark.parametrize("case,mode", CASE_MODES, ids=[f"{c['id']}-{st.MODES[m]}" for c, m in CASE_MODES])
def test_greedy_against_truth(case, mode):
    from romhighcontrast_amd.lib.ReducedBasis import select_sensors_pbdw
    tr = st.case_truth(case)
    sm = _sm(*case["grid"])
    res = run_case(sm, tr, case, mode)
    assert res[4]["host_syncs"] == 1
    k = res[4]["picks"]
    # beta through select_sensors_pbdw (sensor_beta_prefix gets n - dead_rows): the same selection, bit for bit
    sel = select_sensors_pbdw(sm, tr.Cm, tr.pt.pts, case["m"], mode=st.MODES[mode], rel_tol=case["rel_tol"])
    assert np.array_equal(sel.picks, res[0][:k]) and np.array_equal(_bits(sel.criterion), _bits(res[1][:k]))
    assert np.array_equal(sel.points, tr.pt.pts[res[0][:k]])
    assert sel.stop_reason == {0: "m", 1: "captured", 2: "no_candidates"}[res[4]["stop_reason"]]
    hold(f"greedy {case['id']} {st.MODES[mode]}", st.check_greedy(tr, mode, case["m"], case["rel_tol"], res, beta=sel.beta))
    if case["dead"]:
        assert res[4]["dead_rows"] == 3
    if case["id"] == "m260":
        assert k == 260 and len(tr.pt.pts) > 256 and len(tr.pt.pts) % 256
    COVERED.update(case["route"])


def test_refusals():
    from romhighcontrast_amd import _ffi
    gr, sm = ht.grid(*st.G15), _sm(*st.G15)
    Cb = sm._ctx.upload(st.basis_rows(gr, 129, "random", 1))
    loc = st.locate(gr, st.vertices(gr))
    msg = r"1 <= n <= 128 \(collective\) or 96 \(worst case\)"
    with pytest.raises(_ffi.RomLibraryError, match=msg):
        sm._fem.sensor_greedy(Cb, 97, *loc, 4, 1, 0.0)
    with pytest.raises(_ffi.RomLibraryError, match=msg):
        sm._fem.sensor_greedy(Cb, 129, *loc, 4, 0, 0.0)
    COVERED.add("refusals")


@pytest.mark.parametrize("mode", (0, 1), ids=list(st.MODES.values()))
def test_more_than_1024_partials(mode):
    """ks_select's per-thread walk: (a) a base set of 509 points repeated cyclically to 262 144 + 256 + 3 candidates
    (1026 workgroups): the picks are the base run's, i.e. the first occurrences; (b) 262 144 boundary points in front of
    the base set: the base run's picks + 262 144.  crit and A of both inside the truth bounds of the base set."""
    gr, sm = ht.grid(*st.G7), _sm(*st.G7)
    n, m = 2, 3
    base = st.point_set(gr, WALK_BASE, seed=17)
    Cm = st.basis_rows(gr, n, "random", 23)
    tr = st.GreedyTruth(gr, Cm, base)
    Cb = sm._ctx.upload(Cm)
    r0 = sm._fem.sensor_greedy(Cb, n, *tr.pt.loc, m, mode, 0.0)
    assert r0[4]["picks"] == m
    hold(f"partials base {st.MODES[mode]}", st.check_greedy(tr, mode, m, 0.0, r0, expect_picks=m))
    K = WALK_FRONT + 256 + 3
    assert (K + st.SG_TPB - 1) // st.SG_TPB > st.SG_SELECT
    reps = np.arange(K) % WALK_BASE
    ra = sm._fem.sensor_greedy(Cb, n, *[a[reps] for a in tr.pt.loc], m, mode, 0.0)
    assert np.array_equal(ra[0], r0[0]), "repeated candidates: the first occurrence is picked"
    hold(f"partials cyclic {st.MODES[mode]}", st.check_greedy(tr, mode, m, 0.0, ra, expect_picks=m))
    front = st.locate(gr, st.boundary_points(gr, WALK_FRONT, seed=29))
    rb = sm._fem.sensor_greedy(Cb, n, *[np.r_[f, a] for f, a in zip(front, tr.pt.loc)], m, mode, 0.0)
    assert np.array_equal(rb[0], r0[0] + WALK_FRONT), "boundary points in front: the base run's picks, shifted"
    hold(f"partials boundary-front {st.MODES[mode]}", st.check_greedy(tr, mode, m, 0.0, (rb[0] - WALK_FRONT,) + rb[1:], expect_picks=m))
    COVERED.add("select_walk")


@pytest.mark.parametrize("mode", ("collective", "worst"))
def test_all_dead_basis(mode):
    from romhighcontrast_amd.lib.ReducedBasis import select_sensors_pbdw
    gr, sm = ht.grid(*st.G15), _sm(*st.G15)
    cand = st.candidates(gr, 10, 1)
    sel = select_sensors_pbdw(sm, np.zeros((2, gr.dim)), cand, 4, mode=mode, rel_tol=0.0)
    assert sel.stop_reason == "no_candidates" and len(sel.picks) == 0 and sel.points.shape == (0, 2) and len(sel.beta) == 0
    r = sm._fem.sensor_greedy(sm._ctx.upload(np.zeros((2, gr.dim))), 2, *st.locate(gr, cand), 4, int(mode == "worst"), 0.0)
    assert r[4] == {"dead_rows": 2, "picks": 0, "stop_reason": 2, "host_syncs": 1}
    assert np.all(r[0] == -1) and not np.any(r[1]) and not np.any(r[2]) and (r[3] is None or not np.any(r[3]))
    COVERED.add("dead_rows")


@pytest.mark.parametrize("case_id", ("n10_m40", "dead_middle"))
def test_row_offset_between_guard_rows(case_id):
    case = st.CASES[case_id]
    tr, sm = st.case_truth(case), _sm(*case["grid"])
    dim = tr.gr.dim
    block = np.vstack([np.full((3, dim), SENTINEL), tr.Cm, np.full((2, dim), SENTINEL)])
    Gb = sm._ctx.upload(block)
    for mode in case["modes"]:
        r0 = run_case(sm, tr, case, mode, m=12)
        r3 = run_case(sm, tr, case, mode, m=12, c_row0=3, Cb=Gb)
        assert same_bits(r0, r3), "c_row0 = 3 must give the bits of c_row0 = 0"
        assert r3[4]["picks"] == 12
    after = Gb.download(block.size, shape=block.shape)
    assert np.array_equal(_bits(after), _bits(block)), "the basis buffer and its guard rows are read-only"
    COVERED.add("row_offset")


@pytest.mark.parametrize("mode", (0, 1), ids=list(st.MODES.values()))
def test_rel_tol_stop_is_an_exact_prefix(mode):
    from romhighcontrast_amd.lib.ReducedBasis import select_sensors_pbdw
    case = st.CASES["n10_m40"]
    tr, sm = st.case_truth(case), _sm(*case["grid"])
    m = case["m"]
    full = run_case(sm, tr, case, mode)
    assert full[4]["picks"] == m
    crit = full[1]
    # the first step >= 8 whose criterion is a new minimum of steps 1 .., clearly below the minimum before it
    ks = [k for k in range(8, m) if crit[k] < 0.99 * crit[1:k].min()]
    assert ks, "no clear new minimum of the criterion in the full run"
    k = ks[0]
    rel_tol = 0.5 * (crit[k] + crit[1:k].min()) / crit[0]
    cut = run_case(sm, tr, case, mode, rel_tol=rel_tol)
    assert cut[4]["picks"] == k and cut[4]["stop_reason"] == 1, cut[4]
    for x, y in zip(full[:4], cut[:4]):
        if x is not None:
            assert np.array_equal(_bits(x[:k]), _bits(y[:k])), "the stopped run is the full run's prefix, bit for bit"
    assert np.all(cut[0][k:] == -1) and not np.any(cut[1][k:]) and not np.any(cut[2][k:])
    assert cut[3] is None or not np.any(cut[3][k:])
    sel = select_sensors_pbdw(sm, tr.Cm, tr.pt.pts, m, mode=st.MODES[mode], rel_tol=rel_tol)
    assert sel.stop_reason == "captured" and np.array_equal(sel.picks, full[0][:k])
    COVERED.add("rel_tol_stop")


@pytest.mark.parametrize("case_id", ("n1", "n32", "n33", "n96", "n128"))
def test_bits_repeat_and_poison(case_id, monkeypatch):
    case = st.CASES[case_id]
    tr, sm = st.case_truth(case), _sm(*case["grid"])
    mode = case["modes"][0]
    r1 = run_case(sm, tr, case, mode)
    assert same_bits(r1, run_case(sm, tr, case, mode)), "repeat calls must give the same bits"
    monkeypatch.setenv("ROMHC_POISON_WS", "1")
    fresh = _sm(*case["grid"], fresh=True)
    assert same_bits(r1, run_case(fresh, tr, case, mode)), "a fresh FE space under ROMHC_POISON_WS must give the same bits"


# ---- routes ------------------------------------------------------------------------------------------------------------------
# (case id, mode) run by tests/sensor_child.py under profiling, next to the split transform
CHILD_CASES = [("n32", 1), ("n33", 1), ("n96", 1), ("n128", 0), ("m260", 0), ("ncand257", 1)]


def child_expectations(case, mode):
    """Launch counts a run of m picks leaves in the profile: m selects, m steps (one before the first pick, none after the
    last), and in the worst-case mode m eigen-solves under the name of its order."""
    m, n = case["m"], case_n(case)
    want = {"sensor_select": m, "sensor_step": m, "sensor_prep": m}
    if mode:
        want[f"small_eig_n{n}_mode0_gram"] = m
    return want


def case_n(case):
    return case["n"] + (3 if case["dead"] else 0)


def test_routes_confirmed_by_profile_names():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, ROMHC_PROF_DETAIL="1")
    env.pop("ROMHC_SENSOR_TRUTH_JSON", None)
    r = subprocess.run([sys.executable, os.path.join(root, "tests", "sensor_child.py")], env=env, cwd=root,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    out = r.stdout.decode(errors="replace")
    assert r.returncode == 0 and out.rstrip().endswith("OK"), out[-4000:]
    got = json.loads([ln for ln in out.splitlines() if ln.startswith("ROUTES ")][-1][7:])
    for cid, mode in CHILD_CASES:
        rec = got[f"{cid}-{st.MODES[mode]}"]
        for name, cnt in rec["want"].items():
            assert rec["seen"].get(name, 0) == cnt, (cid, mode, name, rec)
        if not mode:
            assert not [nm for nm in rec["seen"] if nm.startswith("small_eig")], rec
    assert got["split"]["seen"].get("riesz_transform_c", 0) == 2 and got["split"]["seen"].get("riesz_spectral", 0) == 1, got["split"]
    COVERED.add("_confirmed")


def test_route_table_is_covered():
    assert "_confirmed" in COVERED, "run the whole module: the child-process confirmation did not run"
    assert set(ROUTES) <= COVERED, sorted(set(ROUTES) - COVERED)
