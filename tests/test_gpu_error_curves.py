"""rom_error_curves (SolutionsManager.error_curves, experiment_statistics(..., all_dims=True)) on an MI355X.

* fixture g8: the all-dimensions statistics reproduce the reference's records within the bounds of
  test_g8_experiment_statistics, and today's per-n loop to 1e-12 relative on ordinary parameters;
* 80-bit truth (tests/referee.py) for greedy, POD and random bases, in squared errors as in test_gpu_greedy_routes: the
  projection curve against u2 - |p|^2 of the exact span of the rows the call kept, |e_n^2 - t_n^2| <= C (n+1) eps
  (1 + kappa_n) ||u||^2, kappa_n the condition number of those rows among the first n in the A_1 norm (CGS2 reproduces
  the span of rows perturbed by eps: angle <= eps kappa); the Galerkin curve against galerkin_truth_nested with
  C (n+1) contrast eps ||u||^2 added (two exact solvers of a reduced system differ by cond x eps); C = 64;
* edge cases (a row equal to a snapshot, a duplicated row, N > M, N = 0, M = 0), row offsets into larger buffers,
  identical bits on a repeat call and under ROMHC_POISON_WS;
* ROUTES: every route of the call; tests/error_curves_child.py confirms them from profile names in a child process and
  test_route_table_is_covered asserts that every route was reached.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import load_golden, observed
from oracle import rom_oracle as ro

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
C_BOUND = 64.0
ROUTES = {
    "pass_nc8": "a pass over the snapshots with 8 basis vectors in registers (N <= 8, or the last <= 8 of a longer basis)",
    "pass_nc16": "a pass with 16 (8 < N <= 16)",
    "pass_nc32": "a pass with 32 (N > 16)",
    "multi_pass": "N > 32: later passes carry the residual through the earlier chunks",
    "galerkin_lds": "nested Galerkin systems in LDS (N <= 64)",
    "galerkin_global": "nested Galerkin systems in global memory (N > 64)",
    "no_galerkin": "projection curves only (a = NULL)",
}
COVERED = set()


def routes_of(N, info, galerkin):
    out = set()
    if N > 32:
        out.add("multi_pass")
    rest = N
    while True:
        nc = 8 if rest <= 8 else 16 if rest <= 16 else 32
        out.add(f"pass_nc{nc}")
        if rest <= nc:
            break
        rest -= nc
    out.add({None: "no_galerkin", "lds": "galerkin_lds", "global": "galerkin_global"}[info["galerkin_route"]] if galerkin
            else "no_galerkin")
    return out


@pytest.fixture(scope="module")
def ctx():
    from romhighcontrast_amd import _ffi
    return _ffi.get_context()


def _snapshots(blocks, N, M, contrast, seed):
    from romhighcontrast_amd.lib.SolutionsManagers import SolutionsManagerFEM
    sm = SolutionsManagerFEM(blocks, N)
    rng = np.random.default_rng(seed)
    a = 10.0 ** rng.uniform(0, np.log10(contrast), size=(M,) + tuple(blocks))
    return sm, a, sm.generate_solutions(a)


def _basis(kind, sm, U, a, n, seed):
    from romhighcontrast_amd.lib.ReducedBasis import GREEDY_FOR_H10, ReducedBasisGreedy, ReducedBasisPCA
    if kind == "greedy":
        return np.asarray(ReducedBasisGreedy(GREEDY_FOR_H10).build(n, sm, U, a, sm.H10norm(U)).basis)
    if kind == "pod":
        return np.asarray(ReducedBasisPCA(add_inf_solutions=False).build(n, sm, U, a).basis)
    return np.random.default_rng(seed).standard_normal((n, U.shape[1]))


def _kappa(g, C, keep):
    """kappa_n of the row-normalised kept rows among the leading n in the A_1 norm, n = 0 .. len(C)."""
    import referee
    G = np.asarray(referee._a1_dots_ld(g, C.astype(referee.LD), C.astype(referee.LD)), dtype=np.float64)
    idx = np.flatnonzero(keep)
    d = np.sqrt(np.diag(G))
    G = G / d[:, None] / d[None, :]
    out = [1.0]
    for n in range(1, len(C) + 1):
        k = idx[idx < n]
        w = np.linalg.eigvalsh(G[np.ix_(k, k)]) if len(k) else np.ones(1)
        out.append(np.sqrt(w[-1] / w[0]) if w[0] > 0 else np.inf)
    return np.array(out)


def _run(ctx, sm, U, C, a=None, u_row0=0, c_row0=0):
    """The device call with U and C inside larger buffers (NaN rows around them) at the given row offsets."""
    dim = sm.vspace_dim
    M, N = len(U), len(C)
    Ub = ctx.upload(np.vstack([np.full((u_row0, dim), np.nan), U, np.full((2, dim), np.nan)]))
    Cb = ctx.upload(np.vstack([np.full((c_row0, dim), np.nan), C, np.full((2, dim), np.nan)])) if N else None
    ab = None
    if a is not None:
        ab = ctx.alloc(max(np.size(a), 1))
        if np.size(a):
            ab.upload(np.ascontiguousarray(a, dtype=np.float64).reshape(M, -1))
    return sm._fem.error_curves(Ub, M, Cb, N, ab, u_row0=u_row0, c_row0=c_row0)


CASES = [
    # id, blocks, mesh N, M, basis kind, basis rows, contrast, galerkin, u_row0, c_row0
    ("sq_random_n1_m1", (2, 2), 8, 1, "random", 1, 1e2, True, 0, 0),
    ("sq_greedy_n50", (2, 2), 8, 300, "greedy", 50, 1e2, True, 3, 5),
    ("sq_greedy_n50_hc", (2, 2), 8, 300, "greedy", 50, 9e7, True, 0, 0),
    ("sq_pod_n12", (2, 2), 8, 257, "pod", 12, 1e2, True, 0, 2),
    ("rect_pod_n40_hc", (1, 3), 8, 300, "pod", 40, 9e7, True, 1, 0),
    ("rect_random_n70", (1, 3), 8, 300, "random", 70, 1e2, True, 0, 0),
    ("rect_greedy_n70_hc", (1, 3), 8, 300, "greedy", 70, 9e7, True, 2, 3),
    ("sq_random_n6_proj", (2, 2), 8, 1, "random", 6, 1e2, False, 0, 0),
]


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_curves_against_80bit_truth(ctx, case):
    import referee
    cid, blocks, Nm, M, kind, n, contrast, gal, u0, c0 = case
    sm, a, U = _snapshots(blocks, Nm, M, contrast, seed=len(cid))
    C = _basis(kind, sm, U, a, n, seed=7)
    g = ro.Geometry(blocks, Nm)
    proj, galc, P, T, info = _run(ctx, sm, U, C, a if gal else None, u0, c0)
    assert proj.shape == (n + 1, M) and P.shape == (M, n) and T.shape == (n, n)
    dead = np.diag(T) == 0.0
    assert info["dependent_rows"] == dead.sum(), info
    assert np.all(T[:, dead] == 0.0) and np.all(P[:, dead] == 0.0)
    assert np.array_equal(T, np.tril(T))
    # the truth is the exact span of the rows the call kept (a dropped row's remainder is below 1e-13 of its norm)
    Ck = C.copy()
    Ck[dead] = 0.0
    Q, keep = referee.a1_orthonormal_span_ld(g, Ck)
    assert np.array_equal(keep, ~dead)
    UL = U.astype(referee.LD)
    u2 = np.array([referee.h10_ld(g, u) ** 2 for u in UL])
    PL = np.asarray(referee._a1_dots_ld(g, UL, Q))
    unorm = np.sqrt(np.asarray(u2, dtype=np.float64))
    kap = _kappa(g, C, ~dead)
    # squared errors, as in test_gpu_greedy_routes: the truth u2 - |p|^2 itself cancels in 80 bits once the residual is
    # far below ||u||, so the comparison is made where both sides are accurate to a multiple of eps ||u||^2
    truth2 = np.array([np.maximum(u2 - np.sum(PL[:, :j] ** 2, axis=1), 0) for j in range(n + 1)], dtype=np.float64)
    bound_p = C_BOUND * (np.arange(n + 1) + 1)[:, None] * EPS * (1 + kap[:, None]) * unorm[None, :] ** 2
    observed(f"curves {cid}: squared projection error vs 80-bit truth, in units of C(n+1) eps (1 + kappa) ||u||^2",
             np.abs(proj ** 2 - truth2) / bound_p, 1.0)
    np.testing.assert_allclose(proj[0], np.asarray(sm._fem.h10norm(ctx.upload(U), M)), rtol=1e-13)
    # the coefficients: C = T W reproduces the rows' A_1 products with the snapshots, P = <U, W>_A
    Pt = np.asarray(PL, dtype=np.float64)
    rel = np.abs(np.abs(P) - np.abs(Pt)).max() / max(1e-300, unorm.max())
    observed(f"curves {cid}: |P| vs 80-bit |<u, q>_A| (relative to ||u||; bounded by eps kappa)", rel, C_BOUND * n * EPS * (1 + kap[-1]))
    if gal:
        sizes = list(range(1, n + 1))
        tg = referee.galerkin_truth_nested(g, a, Ck, U, sizes)
        tg = np.vstack([np.ones(M)] + [tg[j] for j in sizes]) * unorm[None, :]
        bound_g = bound_p + C_BOUND * contrast * EPS * (np.arange(n + 1) + 1)[:, None] * unorm[None, :] ** 2
        observed(f"curves {cid}: squared Galerkin error vs 80-bit truth, in units of C(n+1) eps ((1 + kappa) + contrast) ||u||^2",
                 np.abs(galc ** 2 - tg ** 2) / bound_g, 1.0)
        assert (galc >= proj * (1 - 1e-12)).all()
    else:
        assert galc is None
    COVERED.update(routes_of(n, info, gal))


def test_row_equal_to_snapshot_and_duplicate(ctx):
    sm, a, U = _snapshots((2, 2), 8, 40, 1e2, seed=3)
    C = np.vstack([U[5], U[9], U[5], U[17]])  # row 2 duplicates row 0
    proj, galc, P, T, info = _run(ctx, sm, U, C, a)
    unorm = proj[0]
    assert info["dependent_rows"] == 1
    bound = C_BOUND * 5 * EPS * 1e3 * unorm
    assert proj[1][5] <= bound[5] and proj[2][9] <= bound[9] and proj[4][17] <= bound[17]
    assert galc[1][5] <= 1e-9 * unorm[5]            # the Galerkin solution of the snapshot's own parameter: the snapshot
    np.testing.assert_array_equal(proj[3], proj[2])  # the duplicate adds no direction: flat curve
    np.testing.assert_array_equal(galc[3], galc[2])
    assert T[2, 2] == 0.0 and np.all(T[3:, 2] == 0.0)
    np.testing.assert_allclose(T[2, :2], T[0, :2], rtol=1e-12, atol=1e-12 * abs(T[0, 0]))


def test_n_beyond_m_and_empty(ctx):
    sm, a, U = _snapshots((2, 2), 8, 5, 1e2, seed=4)
    C = np.random.default_rng(1).standard_normal((12, sm.vspace_dim))
    proj, galc, P, T, info = _run(ctx, sm, U, C, a)          # N > M
    assert proj.shape == (13, 5) and (np.diff(proj, axis=0) <= 1e-12 * proj[0]).all()
    h = np.asarray(sm._fem.h10norm(ctx.upload(U), 5))
    p0, g0, P0, T0, i0 = _run(ctx, sm, U, C[:0], a)        # N = 0: only ||u||
    assert p0.shape == (1, 5) and P0.shape == (5, 0) and T0.shape == (0, 0)
    np.testing.assert_allclose(p0[0], h, rtol=1e-14)
    np.testing.assert_array_equal(g0[0], p0[0])
    pe, ge, Pe, Te, ie = _run(ctx, sm, U[:0], C, a[:0])     # M = 0: T still built
    assert pe.shape == (13, 0) and ge.shape == (13, 0) and Pe.shape == (0, 12)
    np.testing.assert_array_equal(Te, T)


def test_bits_repeat_and_poison(ctx, monkeypatch):
    sm, a, U = _snapshots((1, 3), 8, 300, 9e7, seed=5)
    C = _basis("greedy", sm, U, a, 40, 0)
    r1 = _run(ctx, sm, U, C, a, 1, 2)
    r2 = _run(ctx, sm, U, C, a, 1, 2)
    monkeypatch.setenv("ROMHC_POISON_WS", "1")
    r3 = _run(ctx, sm, U, C, a, 1, 2)
    for x, y, z in zip(r1[:4], r2[:4], r3[:4]):
        assert np.array_equal(x, y) and np.array_equal(x, z)


def test_span_only(ctx):
    """Row order within the leading n, scaling and orthonormalize() leave every record of that n unchanged."""
    sm, a, U = _snapshots((2, 2), 8, 64, 1e3, seed=6)
    C = _basis("greedy", sm, U, a, 10, 0)
    p1, g1, *_ = _run(ctx, sm, U, C, a)
    C2 = C.copy()
    C2[:5] = C2[[4, 2, 0, 1, 3]] * np.array([3.0, -0.5, 7.0, 1e-3, 2.0])[:, None]
    p2, g2, *_ = _run(ctx, sm, U, C2, a)
    from romhighcontrast_amd.lib.ReducedBasis import BaseReducedBasis
    rb = BaseReducedBasis()
    rb.set(C, [a[i] for i in range(10)])
    rb.orthonormalize()
    p3, g3, *_ = rb.error_curves(sm, U, a)
    for n, others in ((5, [(p2, g2)]), (10, [(p2, g2), (p3, g3)])):
        for p, gg in others:
            np.testing.assert_allclose(p[n], p1[n], rtol=1e-9, atol=1e-12 * p1[0].max())
            np.testing.assert_allclose(gg[n], g1[n], rtol=1e-9, atol=1e-12 * p1[0].max())


def test_g8_all_dims(ctx):
    """experiment_statistics(..., all_dims=True) on fixture g8: the reference's records within the bounds of
    test_g8_experiment_statistics, and today's per-n loop to 1e-12 relative on ordinary parameters."""
    import referee
    from src.experiments.HighContrast import experiment_statistics, get_a2test_and_train
    from romhighcontrast_amd.lib import ReducedBasis as RB
    z = load_golden("g8_experiment.npz")

    def run(all_dims):
        sm, a, _ = get_a2test_and_train((2, 2), [[(0, 0), (1, 1)], [(0, 1)]], 6, 2, 30, 7, method="lsq")
        builders = [RB.ReducedBasisRandom(), RB.ReducedBasisRandom(False), RB.ReducedBasisGreedy(greedy_for=RB.GREEDY_FOR_H10),
                    RB.ReducedBasisGreedy(greedy_for=RB.GREEDY_FOR_GALERKIN)]
        return sm, a, builders, experiment_statistics(sm, a, builders, vn_max_dim=4, num_measurements=12, all_dims=all_dims)

    sm, a, builders, data = run(True)
    _, _, _, data0 = run(False)
    g = ro.Geometry((2, 2), 6)
    hard = (a == RB.INFINIT_A).any(axis=(1, 2))
    for b in builders:
        key = b.name.replace(" ", "_").replace("$", "").replace("\\", "").replace("^", "").replace("{", "").replace("}", "")
        assert "time2curves" in data[b.name] and "time2curves" not in data0[b.name]
        assert sorted(data[b.name]["errors"]) == [1, 2, 3, 4] and sorted(data[b.name]["times"]) == [1, 2, 3, 4]
        np.testing.assert_array_equal(np.asarray(data[b.name]["basis"].basis), np.asarray(data0[b.name]["basis"].basis))
        for n in range(1, 5):
            e, e0 = data[b.name]["errors"][n], data0[b.name]["errors"][n]
            for f in ("forward_modeling", "projection"):
                got, per_n, ref = np.asarray(getattr(e, f)), np.asarray(getattr(e0, f)), z[f"err_{key}_{n}_{f}"]
                observed(f"g8 all_dims {key} n={n} {f}: relative-error records vs per-n loop, ordinary parameters",
                         np.abs(got - per_n)[~hard], 1e-12)
                observed(f"g8 all_dims {key} n={n} {f}: vs reference, ordinary parameters", np.abs(got - ref)[~hard], 1e-10)
                if f == "projection":
                    observed(f"g8 all_dims {key} n={n} projection: vs reference, INFINIT_A parameters", np.abs(got - ref)[hard], 1e-10)
                else:
                    Qb = np.linalg.qr(np.asarray(data[b.name]["basis"].basis)[:n].T)[0].T
                    conds = [np.linalg.cond(Qb @ ro.stencil_apply(g, am, Qb).T) for am in a[hard]]
                    tol_f = max(1e-10, 1e-14 * max(conds))
                    observed(f"g8 all_dims {key} n={n} forward_modeling: vs reference, INFINIT_A parameters (1e-14 cond)",
                             np.abs(got - ref)[hard], tol_f)
                    t_us = referee.galerkin_truth_nested(g, a, np.asarray(data[b.name]["basis"].basis)[:n], np.asarray(data["solutions"]), [n])[n]
                    t_ref = referee.galerkin_truth_nested(g, a, z["basis_" + key][:n], z["solutions"], [n])[n]
                    d_us, d_ref = np.abs(got - t_us)[hard], np.abs(ref - t_ref)[hard]
                    observed(f"g8 all_dims {key} n={n} forward_modeling, INFINIT_A: vs 80-bit truth in units of max(1e-10, 4 x the reference's distance)",
                             d_us / np.maximum(1e-10, 4 * d_ref.max()), 1.0)
            Eb = sm.evaluate_solutions(data["measurement_points"], np.asarray(data[b.name]["basis"].basis)[:n])
            tol = max(1e-9, 1e-13 * np.linalg.cond(Eb))
            for f in ("state_estimation", "parameter_estimation_inverse", "parameter_estimation_linear"):
                ref, got, per_n = z[f"err_{key}_{n}_{f}"], np.asarray(getattr(e, f)), np.asarray(getattr(e0, f))
                assert got.shape == ref.shape
                scale = max(1.0, np.abs(ref).max())
                observed(f"g8 all_dims {key} n={n} {f}: vs reference (max(1e-9, 1e-13 cond(E)))",
                         np.abs(got - ref).reshape(len(ref), -1).max(axis=1) / scale, tol)
                if f != "state_estimation":   # the same host arithmetic on the same coefficients
                    np.testing.assert_array_equal(got, per_n)
                else:
                    # (the per-n loop forms the estimate c^T C and its difference with u: relative to the record's size,
                    # as the comparison with the reference above: records are large where the basis holds INFINIT_A rows)
                    observed(f"g8 all_dims {key} n={n} state_estimation: records vs per-n loop, ordinary parameters, relative to max(1, |record|) (max(1e-12, 1e-14 cond(E)))",
                             np.abs(got - per_n)[~hard] / max(1.0, np.abs(per_n).max()), max(1e-12, 1e-14 * np.linalg.cond(Eb)))


def test_routes_confirmed_by_profile_names():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, ROMHC_PROF_DETAIL="1")
    r = subprocess.run([sys.executable, os.path.join(root, "tests", "error_curves_child.py")], env=env, cwd=root,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    out = r.stdout.decode(errors="replace")
    assert r.returncode == 0 and out.rstrip().endswith("OK"), out[-4000:]
    got = json.loads([ln for ln in out.splitlines() if ln.startswith("ROUTES ")][-1][7:])
    for cid, N, gal in CHILD_CASES:
        want = got[cid]["want"]
        assert set(want) <= set(got[cid]["seen"]), (cid, want, got[cid]["seen"])
    COVERED.add("_confirmed")


# (id, basis rows, with parameters): run by tests/error_curves_child.py under profiling
CHILD_CASES = [("n4", 4, True), ("n12", 12, True), ("n50", 50, True), ("n70", 70, True), ("n40_proj", 40, False)]


def test_route_table_is_covered():
    assert "_confirmed" in COVERED, "run the whole module: the child-process confirmation did not run"
    assert set(ROUTES) <= COVERED, sorted(set(ROUTES) - COVERED)
