"""tests/sensor_truth.py proved on the CPU (no GPU, no product code).

* the plain fp64 NumPy restatement of rom_riesz_h10, rom_riesz_norms_h10 and rom_sensor_greedy (riesz_host, norms_host,
  greedy_host) against the long-double truth on every case the GPU tests use: every measure at most 1/8 of its bound
  (the margin of tests/test_resid_host.py), printed per case in the terminal summary.  This is what justifies the form of
  u_k = C eps (k + n + nr + nc) kappa_k (1 + kappa_V), which is not derived rigorously;
* the truth's own consistency on the smallest grid: G against the dense A_1 solve in fp64 to 1e-12, and the Cholesky
  prefix property of the incremental state (L L^T = G[picks, picks], A = L^-1 E[picks], every prefix the state of a
  shorter run);
* planted mutations of the restatement, each of which must break a bound by at least 100x, so the GPU tests would bite:
  the k mod 4 tail of the Phi recurrence dropped, only the first 256 entries of the Cholesky row read, ties broken to the
  higher index, a dead row's direction left in alpha, the second block of the split transform started at offset 0, the
  (1,1) table read at (y, x) instead of (y, x - 1) for the (1,-1) pair, the first instead of the last eigenvector row.
With ROMHC_SENSOR_TRUTH_JSON set, every case's ratios are appended to that file as "restatement" lines.
"""
import numpy as np
import pytest

from conftest import observed
import h10_truth as ht
import sensor_truth as st

LD = st.LD
INSIDE = 1.0 / st.MARGIN
NPTS = (1, 17, 65)


def hold(tag, measures):
    st.hold("restatement", tag, measures, INSIDE)


@pytest.mark.parametrize("npts", NPTS)
@pytest.mark.parametrize("blocks,N", st.GRIDS, ids=[f"{b[0]}x{b[1]}_N{N}" for b, N in st.GRIDS])
def test_restatement_points_against_truth(blocks, N, npts):
    gr = ht.grid(blocks, N)
    pt = st.PointTruth(gr, st.point_set(gr, npts, seed=npts + N))
    if npts >= 17:
        assert pt.zero.any() and not pt.zero.all()
    Om, G = st.riesz_host(gr, pt.loc)
    Om2, _ = st.riesz_host(gr, pt.loc, max_rows=64)         # the split of the second transform, every block in place
    assert np.array_equal(Om, Om2)
    hold(f"points {gr.nr}x{gr.nc} npts={npts}", st.check_points(pt, Om, G, st.norms_host(gr, pt.loc)))


def test_restatement_split_transform_size_case():
    """The size case of the split launch, scaled down: the 3 x 3 grid, a base set repeated cyclically, max_rows chosen
    so that the last block holds three rows (as 3 x 1 398 081 rows against 65 535 x 64 on the device)."""
    gr = ht.grid(*st.SIZE_GRID)
    base = st.point_set(gr, 41, seed=3)
    pt = st.PointTruth(gr, base)
    reps = np.arange(129) % len(base)
    loc = [a[reps] for a in pt.loc]
    Om, _ = st.riesz_host(gr, loc, max_rows=3 * 129 - 3, gram=False)
    err = np.asarray(np.sqrt(np.sum((Om.astype(LD) - pt.Om[reps]) ** 2, axis=1)), dtype=np.float64)
    live = ~pt.zero[reps]
    observed("split transform 3x3: row error / riesz_bound", err[live] / pt.row_bound[reps][live], INSIDE)
    assert not np.any(Om[~live])


CASE_MODES = [(c, mode) for c in st.GREEDY_CASES for mode in c["modes"]]


@pytest.mark.parametrize("case,mode", CASE_MODES, ids=[f"{c['id']}-{st.MODES[m]}" for c, m in CASE_MODES])
def test_restatement_greedy_against_truth(case, mode):
    tr = st.case_truth(case)
    res = st.greedy_host(tr.gr, tr.Cm, tr.pt.loc, case["m"], mode, case["rel_tol"])
    k, n_live = res[4]["picks"], tr.n_live
    beta = np.zeros(k)
    for j in range(n_live, k + 1):
        beta[j - 1] = np.linalg.svd(res[2][:j], compute_uv=False)[n_live - 1]
    hold(f"greedy {case['id']} {st.MODES[mode]}", st.check_greedy(tr, mode, case["m"], case["rel_tol"], res, beta=beta))
    if case["dead"]:
        assert res[4]["dead_rows"] == 3 and n_live == case["n"]
    if case["id"] == "m260":
        assert k == 260 and res[1][-1] >= 0.2 * res[1][0], "the criterion of vertex candidates stays near the first one"


def test_all_dead_basis_ends_without_a_pick():
    gr = ht.grid(*st.G15)
    Cm = np.zeros((2, gr.dim))
    cand = st.candidates(gr, 10, 1)
    for mode in (0, 1):
        picks, crit, A, alpha, info = st.greedy_host(gr, Cm, st.locate(gr, cand), 4, mode, 0.0)
        assert info == {"dead_rows": 2, "picks": 0, "stop_reason": 2, "host_syncs": 1}
        assert np.all(picks == -1) and not np.any(A) and not np.any(crit)


# ---- the truth's own consistency ---------------------------------------------------------------------------------------
def test_truth_gram_against_dense_solve():
    gr = ht.grid(*st.GRIDS[0])
    pt = st.PointTruth(gr, st.candidates(gr, 20, 2))
    G = pt.R @ np.linalg.solve(gr.a1_dense(), pt.R.T)
    d = np.sqrt(np.maximum(np.diag(G), 1e-300))
    observed("truth G vs dense fp64 A_1 solve, relative to sqrt(G_ii G_jj)",
             np.abs(G - np.asarray(pt.G, dtype=np.float64)) / (d[:, None] * d[None, :]), 1e-12)
    assert np.array_equal(np.asarray(pt.nu) == 0, pt.zero)
    # the second route to G (R Omega^T through both transforms) agrees to long-double roundoff
    G2 = pt.R.astype(LD) @ pt.Om.T
    assert float(np.abs(G2 - pt.G).max()) < 1e-17


def test_truth_cholesky_prefix_property():
    case = st.CASES["n10_m40"]
    tr = st.case_truth(case)
    picks = st.greedy_host(tr.gr, tr.Cm, tr.pt.loc, case["m"], 0, 0.0)[0]
    state = st.TruthState(tr, 0)
    prefix = {}
    for s, p in enumerate(picks):
        state.push(int(p))
        if s + 1 in (7, 40):
            prefix[s + 1] = (state.A.copy(), state.Res.copy())
    L = state.Phi[:, picks].T                                     # L[k, j] = Phi[j, p_k]
    assert float(np.abs(np.triu(L, 1)).max()) < 1e-17, "psi_j vanishes on the earlier picks' functionals"
    Gp = tr.pt.G[np.ix_(picks, picks)]
    assert float(np.abs(L @ L.T - Gp).max() / np.abs(Gp).max()) < 1e-17
    L64 = np.linalg.cholesky(np.asarray(Gp, dtype=np.float64))
    observed("truth L vs fp64 Cholesky of G[picks, picks]", np.abs(np.asarray(L, dtype=np.float64) - L64) / L64.max(), 1e-12)
    E = np.asarray(tr.Res0[:, picks].T, dtype=np.float64)
    observed("truth A vs fp64 L^-1 E[picks]", np.abs(np.linalg.solve(L64, E) - np.asarray(state.A, dtype=np.float64)), 1e-12)
    short = st.TruthState(tr, 0)
    for p in picks[:7]:
        short.push(int(p))
    assert np.array_equal(short.A, prefix[7][0]) and np.array_equal(short.A, prefix[40][0][:7])
    assert np.array_equal(short.Res, prefix[7][1])


# ---- planted mutations ---------------------------------------------------------------------------------------------------
def _greedy_mutant(case_id, mode, mut, cand2=False):
    case = st.CASES[case_id]
    tr = st.case_truth(case)
    if cand2:       # every candidate twice: whichever point is picked has an exact tie at a higher index
        gr, Cm, cand = st.case_inputs(case)
        tr = st.GreedyTruth(gr, Cm, np.r_[cand, cand])
    clean = st.worst_ratio(st.check_greedy(tr, mode, case["m"], 0.0, st.greedy_host(tr.gr, tr.Cm, tr.pt.loc, case["m"], mode, 0.0)))
    broken = st.worst_ratio(st.check_greedy(tr, mode, case["m"], 0.0, st.greedy_host(tr.gr, tr.Cm, tr.pt.loc, case["m"], mode, 0.0, mut=(mut,))))
    return clean, broken


@pytest.mark.parametrize("mut,case_id,mode,cand2", [
    ("phi_tail", "n10_m40", 0, False), ("phi_tail", "n10_m40", 1, False), ("chol256", "m260", 0, False),
    ("tie_high", "m5", 0, True), ("tie_high", "m5", 1, True), ("dead_alpha", "dead_last", 1, False),
    ("dead_alpha", "dead_middle", 1, False), ("first_row", "n10_m40", 1, False), ("first_row", "n33", 1, False)])
def test_planted_greedy_mutation_is_caught(mut, case_id, mode, cand2):
    clean, broken = _greedy_mutant(case_id, mode, mut, cand2)
    assert clean <= INSIDE
    print(f"mutation {mut} on {case_id} {st.MODES[mode]}: worst ratio {broken:.3g} (clean {clean:.3g})")
    assert broken >= 100.0, (mut, case_id, broken)


def test_planted_split_mutation_is_caught():
    gr = ht.grid(*st.GRIDS[2])
    pt = st.PointTruth(gr, st.point_set(gr, 17, seed=9))
    clean = st.worst_ratio(st.check_points(pt, Om=st.riesz_host(gr, pt.loc, max_rows=64)[0]))
    broken = st.worst_ratio(st.check_points(pt, Om=st.riesz_host(gr, pt.loc, max_rows=64, mut=("split0",))[0]))
    assert clean <= INSIDE and broken >= 100.0, (clean, broken)


@pytest.mark.parametrize("blocks,N", st.GRIDS[1:], ids=[f"{b[0]}x{b[1]}_N{N}" for b, N in st.GRIDS[1:]])
def test_planted_pair_shift_mutation_is_caught(blocks, N):
    gr = ht.grid(blocks, N)
    pt = st.PointTruth(gr, st.point_set(gr, 65, seed=11))
    clean = st.worst_ratio(st.check_points(pt, nu=st.norms_host(gr, pt.loc)))
    broken = st.worst_ratio(st.check_points(pt, nu=st.norms_host(gr, pt.loc, mut=("pair_shift",))))
    assert clean <= INSIDE and broken >= 100.0, (clean, broken)


def test_every_mutation_is_planted():
    import inspect
    src = inspect.getsource(inspect.getmodule(test_every_mutation_is_planted))
    for mut in st.MUTATIONS:
        assert f'"{mut}"' in src, mut
