"""Greedy PBDW sensor selection (rom_riesz_norms_h10, rom_sensor_greedy, select_sensors_pbdw) on an MI355X.

* norms: riesz_norms_h10 against sqrt(diag(riesz_gram_h10)) (an independent route: the MFMA Gram of Rhat / sqrt(Lambda))
  and against a dense A_1^-1, for random points, points on cell edges, on vertices and on block interfaces; boundary
  points give exactly 0; all 65 025 vertices of C2 with a subsample against the Gram route;
* host restatements of both greedy modes with dense A_1 and NumPy, following the GPU's picks (and, in the worst-case
  mode, its directions alpha): criterion, A, no repeated or boundary pick, alpha a smallest eigenvector;
* beta against a host restatement and against the independent PBDW route (pbdw_stability), the quality of the
  selection against random subsets and the a-priori bound with the selected points;
* the contract: bit-identical repeats (also under ROMHC_POISON_WS), ndarray / DeviceArray bases, beta_target = prefix
  of the full run, the stop reasons, ValueError for n = 0, "outside the domain".
These are fp64 restatements with flat tolerances on greedy snapshot bases.  The 80-bit truth with derived bounds, the n
routes of the eigen-solver, m > 256, more than 1024 partials, dead rows and row offsets: tests/test_gpu_sensor_truth.py
(truth and bounds: tests/sensor_truth.py).
"""
import numpy as np
import pytest

from conftest import observed

pytestmark = pytest.mark.gpu

_SM, _BASES = {}, {}


def _sm(blocks, N):
    from romhighcontrast_amd.lib.SolutionsManagers import SolutionsManagerFEM
    key = (tuple(blocks), N)
    if key not in _SM:
        _SM[key] = SolutionsManagerFEM(tuple(blocks), N)
    return _SM[key]


def _basis(blocks, N, n, M):
    """H^1_0 greedy basis of n rows from M random parameters, and 4 test states."""
    from romhighcontrast_amd.lib.ReducedBasis import GREEDY_FOR_H10, ReducedBasisGreedy
    key = (tuple(blocks), N, n, M)
    if key not in _BASES:
        sm = _sm(blocks, N)
        rng = np.random.default_rng(21)
        a = 10.0 ** rng.uniform(0, 2, size=(M,) + tuple(blocks))
        U = sm.generate_solutions(a)
        rb = ReducedBasisGreedy(GREEDY_FOR_H10).build(n, sm, U, a, sm.H10norm(U))
        a_test = 10.0 ** rng.uniform(0, 2, size=(4,) + tuple(blocks))
        _BASES[key] = (rb, sm.generate_solutions(a_test))
    return _BASES[key]


def _points(sm, kind, m, seed):
    """The point families of test_gpu_riesz_pbdw.py::_points."""
    rng = np.random.default_rng(seed)
    (x0, x1), (y0, y1) = sm.x_domain, sm.y_domain
    pc, pr = sm.points_c, sm.points_r
    if kind == "random":
        return np.c_[rng.uniform(x0, x1, m), rng.uniform(y0, y1, m)]
    if kind == "edges":
        a = np.c_[pc[rng.integers(1, len(pc) - 1, m)], rng.uniform(y0, y1, m)]
        b = np.c_[rng.uniform(x0, x1, m), pr[rng.integers(1, len(pr) - 1, m)]]
        i, j, t = rng.integers(0, len(pc) - 1, m), rng.integers(0, len(pr) - 1, m), rng.uniform(0, 1, m)
        c = np.c_[pc[i] + t * (pc[i + 1] - pc[i]), pr[j] + (1 - t) * (pr[j + 1] - pr[j])]
        return np.r_[a, b, c]
    if kind == "vertices":
        return np.c_[pc[rng.integers(1, len(pc) - 1, m)], pr[rng.integers(1, len(pr) - 1, m)]]
    if kind == "interfaces":
        nrb, ncb = sm.blocks_geometry
        xi = x0 + rng.integers(1, ncb, m) if ncb > 1 else rng.uniform(x0, x1, m)
        yi = y0 + rng.integers(1, nrb, m) if nrb > 1 else rng.uniform(y0, y1, m)
        return np.r_[np.c_[xi, rng.uniform(y0, y1, m)], np.c_[rng.uniform(x0, x1, m), yi], np.c_[xi, yi]]
    raise ValueError(kind)


def _boundary(sm, m, seed):
    """Points on the east and north edges of the domain (inside it for the locating convention; functional 0)."""
    rng = np.random.default_rng(seed)
    (x0, x1), (y0, y1) = sm.x_domain, sm.y_domain
    return np.r_[np.c_[np.full(m, x1), rng.uniform(y0, y1, m)], np.c_[rng.uniform(x0, x1, m), np.full(m, y1)]][:m]


# ---- 1. norms ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("blocks,N", [((1, 1), 4), ((2, 2), 8), ((3, 2), 5), ((3, 3), 16), ((2, 2), 128)])
def test_norms_against_gram_and_dense(blocks, N):
    sm = _sm(blocks, N)
    pts = np.r_[_points(sm, "random", 20, 1), _points(sm, "edges", 6, 2), _points(sm, "vertices", 8, 3),
                _points(sm, "interfaces", 4, 4)]
    bnd = _boundary(sm, 4, 5)
    nrm = sm.riesz_norms_h10(np.r_[pts, bnd])
    assert nrm.shape == (len(pts) + len(bnd),)
    assert np.all(nrm[len(pts):] == 0.0), "a vanishing functional must give exactly 0"
    nrm = nrm[:len(pts)]
    G = sm.riesz_gram_h10(pts)
    ref = np.sqrt(np.diag(G))
    live = ref > 0
    assert np.array_equal(nrm > 0, live)
    observed(f"sensor norms {blocks} N={N}: vs sqrt(diag(riesz_gram_h10))", np.abs(nrm - ref)[live] / ref[live], 1e-12)
    if sm.vspace_dim <= 4096:
        R = sm.generate_riesz(pts, "l2")
        dense = np.sqrt(np.einsum("ij,ji->i", R, np.linalg.solve(sm.A_preassembled4h1_norm, R.T)))
        observed(f"sensor norms {blocks} N={N}: vs dense A_1^-1", np.abs(nrm - dense)[live] / dense[live], 1e-12)


def test_norms_all_vertices_c2():
    sm = _sm((2, 2), 128)
    V = sm.interior_vertices()
    assert V.shape == (sm.vspace_dim, 2)
    # dof order: evaluating the dofs' index vector at the vertices returns the index
    idx = np.arange(sm.vspace_dim, dtype=np.float64)[None]
    assert np.array_equal(sm.evaluate_solutions(V[::97], idx)[0], idx[0, ::97])
    nrm = sm.riesz_norms_h10(V)
    assert np.all(nrm > 0)
    sub = np.random.default_rng(0).choice(len(V), 2000, replace=False)
    ref = np.sqrt(np.diag(sm.riesz_gram_h10(V[sub])))
    observed("sensor norms C2, all vertices (2000 subsample) vs Gram route", np.abs(nrm[sub] - ref) / ref, 1e-12)


# ---- 2. / 3. host restatements ---------------------------------------------------------------------------------------
def _restatement_setup(blocks, N):
    sm = _sm(blocks, N)
    rb, _ = _basis(blocks, N, 10, 80)
    rng = np.random.default_rng(40)
    rnd = _points(sm, "random", 300, 41)
    cand = np.r_[sm.interior_vertices(), rnd, _boundary(sm, 5, 42), rnd[rng.choice(300, 10, replace=False)]]
    A1 = sm.A_preassembled4h1_norm
    C = np.asarray(rb.basis)
    K = np.linalg.cholesky(C @ A1 @ C.T)
    W = np.linalg.solve(K, C)                       # A_1-orthonormal, the nested spans of C (positive diagonal)
    R = sm.generate_riesz(cand, "l2")
    Om = np.linalg.solve(A1, R.T).T
    Gc = R @ Om.T                                   # <omega_x, omega_y>
    E = R @ W.T                                     # w_i(x), (ncand, n)
    nu = np.diag(Gc).copy()
    return sm, rb, cand, Gc, E, nu


def _host_state(Gc, E, picks):
    """A_k (k, n) and Res (n, ncand) after the picks: psi = L^-1 omega_p, A_k = L^-1 E[p], Res = E^T - A_k^T Psi(x)."""
    if len(picks) == 0:
        return np.zeros((0, E.shape[1])), E.T.copy()
    L = np.linalg.cholesky(Gc[np.ix_(picks, picks)])
    Ak = np.linalg.solve(L, E[picks])
    Psi = np.linalg.solve(L, Gc[picks])             # psi_j(x), (k, ncand)
    return Ak, E.T - Ak.T @ Psi


def _crit(num, nu):
    out = np.zeros_like(nu)
    ok = nu > 0
    out[ok] = num[ok] / nu[ok]
    return out


@pytest.mark.parametrize("blocks,N", [((2, 2), 8), ((3, 2), 5)])
def test_collective_host_restatement(blocks, N):
    sm, rb, cand, Gc, E, nu = _restatement_setup(blocks, N)
    m = 40
    C = sm._ctx.upload(np.ascontiguousarray(rb.basis))
    picks, crit, A, alpha, info = sm._fem.sensor_greedy(C, 10, *sm._locate(cand), m, 0, 1e-10)
    assert alpha is None and info["dead_rows"] == 0 and info["host_syncs"] == 1
    k = info["picks"]
    assert k == m and info["stop_reason"] == 0 and np.all(picks >= 0)
    assert len(set(picks.tolist())) == k, "a candidate was picked twice"
    assert np.all(nu[picks] > 0), "a boundary point was picked"
    worst_tie, worst_crit = 0.0, 0.0
    for s in range(k):
        _, Res = _host_state(Gc, E, picks[:s])
        c = _crit(np.sum(Res ** 2, axis=0), nu)
        worst_tie = max(worst_tie, 1.0 - c[picks[s]] / np.max(c))
        worst_crit = max(worst_crit, abs(crit[s] - c[picks[s]]) / c[picks[s]])
    tag = f"sensor greedy collective {blocks} N={N}"
    observed(f"{tag}: 1 - host c(p_k) / max host c", worst_tie, 1e-9)
    observed(f"{tag}: crit_out vs host, relative", worst_crit, 1e-9)
    Ak, _ = _host_state(Gc, E, picks)
    observed(f"{tag}: A vs host, relative to max|A|", np.abs(A - Ak) / np.max(np.abs(Ak)), 1e-9)


@pytest.mark.parametrize("blocks,N", [((2, 2), 8), ((3, 2), 5)])
def test_worst_case_host_restatement(blocks, N):
    sm, rb, cand, Gc, E, nu = _restatement_setup(blocks, N)
    m = 40
    C = sm._ctx.upload(np.ascontiguousarray(rb.basis))
    picks, crit, A, alpha, info = sm._fem.sensor_greedy(C, 10, *sm._locate(cand), m, 1, 1e-10)
    k = info["picks"]
    assert k == m and info["stop_reason"] == 0
    assert len(set(picks.tolist())) == k and np.all(nu[picks] > 0)
    tag = f"sensor greedy worst-case {blocks} N={N}"
    unit, eig, tie, crit_err = 0.0, 0.0, 0.0, 0.0
    for s in range(k):
        a = alpha[s]
        unit = max(unit, abs(np.linalg.norm(a) - 1.0))
        Ak, Res = _host_state(Gc, E, picks[:s])
        if s:
            lmin = np.linalg.eigvalsh(Ak.T @ Ak)[0]
            eig = max(eig, (np.sum((Ak @ a) ** 2) - lmin) / np.sum(Ak ** 2))
        c = _crit((a @ Res) ** 2, nu)
        tie = max(tie, 1.0 - c[picks[s]] / np.max(c))
        crit_err = max(crit_err, abs(crit[s] - c[picks[s]]) / c[picks[s]])
    observed(f"{tag}: | ||alpha|| - 1 |", unit, 1e-12)
    observed(f"{tag}: (||A_k alpha||^2 - lambda_min) / ||A_k||^2", eig, 1e-12)
    observed(f"{tag}: 1 - host c(p_k) / max host c (GPU alpha)", tie, 1e-9)
    observed(f"{tag}: crit_out vs host, relative", crit_err, 1e-9)
    Ak, _ = _host_state(Gc, E, picks)
    observed(f"{tag}: A vs host, relative to max|A|", np.abs(A - Ak) / np.max(np.abs(Ak)), 1e-9)


# ---- 4. beta against the PBDW route and a host restatement -----------------------------------------------------------
def _a1_sparse(sm):
    import scipy.sparse as sp
    nr, nc = sm.nr_inner_vertices, sm.nc_inner_vertices
    Tr = sp.diags([-np.ones(nr - 1), 2 * np.ones(nr), -np.ones(nr - 1)], [-1, 0, 1])
    Tc = sp.diags([-np.ones(nc - 1), 2 * np.ones(nc), -np.ones(nc - 1)], [-1, 0, 1])
    return (sp.kron(Tr, sp.eye(nc)) + sp.kron(sp.eye(nr), Tc)).tocsc()


@pytest.mark.parametrize("blocks,N", [((2, 2), 32), ((2, 2), 128)])
@pytest.mark.parametrize("mode", ["collective", "worst"])
def test_beta_against_pbdw_stability(blocks, N, mode):
    """beta_j against (a) a host restatement in well-conditioned coordinates -- CGS2 of the basis in the A_1 inner product,
    representers from a sparse LU, A = L^-1 R W^T with G = L L^T -- to 1e-9 relative, and (b) the PBDW route
    pbdw_stability, which goes through the Cholesky factor of the basis' H^1_0 Gram matrix A_V (greedy snapshots:
    cond(A_V) ~ 1e11 at n = 20), so its own error reaches ~1e-7 relative: 1e-6 there."""
    import scipy.sparse.linalg as spla
    from romhighcontrast_amd.lib.ReducedBasis import select_sensors_pbdw
    sm = _sm(blocks, N)
    rb, _ = _basis(blocks, N, 20, 200)
    n = rb.dim
    cand = sm.interior_vertices()
    A1 = _a1_sparse(sm)
    W = np.array(rb.basis, dtype=np.float64)
    for i in range(n):
        for _ in range(2):
            W[i] -= (W[:i] @ (A1 @ W[i])) @ W[:i]
        W[i] /= np.sqrt(W[i] @ (A1 @ W[i]))
    lu = spla.splu(A1)
    host_rel, stab_rel = [], []
    for m in (20, 40):
        sel = select_sensors_pbdw(sm, rb.basis, cand, m, mode=mode)
        assert len(sel.picks) == m and sel.stop_reason == "m" and sel.points.shape == (m, 2)
        assert np.array_equal(sel.points, cand[sel.picks])
        assert np.all(sel.beta[:n - 1] == 0.0) and sel.beta[n - 1] > 0
        R = sm.generate_riesz(sel.points, "l2")
        G = R @ lu.solve(R.T)
        A = np.linalg.solve(np.linalg.cholesky(0.5 * (G + G.T)), R @ W.T)
        for j in range(n, m + 1):
            hb = np.linalg.svd(A[:j], compute_uv=False)[-1]
            ref = rb.pbdw_stability(sm, sel.points[:j])[-1]
            if hb >= 1e-6:
                host_rel.append(abs(sel.beta[j - 1] - hb) / hb)
            if ref >= 1e-6:
                stab_rel.append(abs(sel.beta[j - 1] - ref) / ref)
    assert host_rel and stab_rel, "no beta above 1e-6 to compare"
    observed(f"sensor beta {blocks} N={N} {mode}: vs host restatement (CGS2 + sparse LU), relative", np.array(host_rel), 1e-9)
    observed(f"sensor beta {blocks} N={N} {mode}: vs pbdw_stability, relative", np.array(stab_rel), 1e-6)


# ---- 5. quality --------------------------------------------------------------------------------------------------------
def test_quality_against_random_subsets():
    from romhighcontrast_amd.lib.ReducedBasis import pbdw_state_estimation, select_sensors_pbdw
    blocks, N, m = (2, 2), 128, 40
    sm = _sm(blocks, N)
    rb, U = _basis(blocks, N, 20, 200)
    cand = sm.interior_vertices()
    rand = []
    for seed in range(20):
        sub = np.random.default_rng(1000 + seed).choice(len(cand), m, replace=False)
        try:
            rand.append(rb.pbdw_stability(sm, cand[sub])[-1])
        except ValueError:      # a random subset that does not determine the basis: beta = 0
            rand.append(0.0)
    med, best = float(np.median(rand)), float(np.max(rand))
    observed("sensor quality C2 m=40: best beta of 20 random subsets (recorded)", best, 1.0)
    basis = np.asarray(rb.basis)
    for mode in ("collective", "worst"):
        sel = select_sensors_pbdw(sm, basis, cand, m, mode=mode)
        b = sel.beta[-1]
        observed(f"sensor quality C2 m=40 {mode}: median random beta - selected beta", med - b, 0.0)
        # the a-priori bound of test_pbdw_properties with the selected points
        Y = sm.evaluate_solutions(sel.points, U)
        r = pbdw_state_estimation(sm, basis, sel.points, Y)
        dist_u = sm.H10norm_diff(sm.project_solutions(U, basis), U)
        err = sm.H10norm_diff(r.estimates, U)
        observed(f"sensor quality C2 m=40 {mode}: ||u - u*|| / (dist(u, V_n) / beta_n) - 1",
                 err / (dist_u / r.beta[-1]) - 1.0, 1e-8)


# ---- 6. contract -------------------------------------------------------------------------------------------------------
def test_contract(monkeypatch):
    from romhighcontrast_amd import _ffi
    from romhighcontrast_amd.lib.ReducedBasis import select_sensors_pbdw
    from romhighcontrast_amd.lib.SolutionsManagers import DeviceArray
    blocks, N = (2, 2), 32
    sm = _sm(blocks, N)
    rb, _ = _basis(blocks, N, 20, 200)
    basis = np.asarray(rb.basis)[:12]
    cand = np.r_[sm.interior_vertices(), _points(sm, "random", 200, 60)]
    loc = sm._locate(cand)
    C = sm._ctx.upload(np.ascontiguousarray(basis))
    for mode in (0, 1):
        r1 = sm._fem.sensor_greedy(C, 12, *loc, 60, mode, 1e-10)
        r2 = sm._fem.sensor_greedy(C, 12, *loc, 60, mode, 1e-10)
        monkeypatch.setenv("ROMHC_POISON_WS", "1")
        r3 = sm._fem.sensor_greedy(C, 12, *loc, 60, mode, 1e-10)
        monkeypatch.delenv("ROMHC_POISON_WS")
        for r in (r2, r3):
            for x, y in zip(r1[:4], r[:4]):
                assert (x is None and y is None) or np.array_equal(x, y), "repeat calls must give the same bits"
            assert r[4] == r1[4]
    # ndarray and DeviceArray bases
    s1 = select_sensors_pbdw(sm, basis, cand, 50, mode="worst")
    Cd = DeviceArray(sm._ctx.upload(np.ascontiguousarray(basis)), 12, sm.vspace_dim)
    s2 = select_sensors_pbdw(sm, Cd, cand, 50, mode="worst")
    for x, y in zip(s1, s2):
        assert np.array_equal(x, y)
    sub = rb[:12]
    s3 = sub.select_sensors(sm, cand, 50, mode="worst")
    for x, y in zip(s1, s3):
        assert np.array_equal(x, y)
    # beta_target: exactly the prefix of the full run
    full = select_sensors_pbdw(sm, basis, cand, 50)
    assert full.stop_reason == "m" and len(full.picks) == 50
    target = full.beta[30]
    j = int(np.flatnonzero(full.beta >= target)[0]) + 1
    cut = select_sensors_pbdw(sm, basis, cand, 50, beta_target=target)
    assert cut.stop_reason == "beta_target" and len(cut.picks) == j <= 31
    assert np.array_equal(cut.picks, full.picks[:j]) and np.array_equal(cut.beta, full.beta[:j])
    assert np.array_equal(cut.criterion, full.criterion[:j]) and np.array_equal(cut.points, full.points[:j])
    # stop reasons: every candidate on the boundary; fewer distinct interior candidates than m
    for mode in ("collective", "worst"):
        none = select_sensors_pbdw(sm, basis, _boundary(sm, 12, 61), 10, mode=mode)
        assert none.stop_reason == "no_candidates" and len(none.picks) == 0 and none.points.shape == (0, 2)
        few = _points(sm, "random", 6, 62)
        dup = np.r_[few, few[[0, 3, 5]], _boundary(sm, 3, 63), few[[1]]]
        s = select_sensors_pbdw(sm, basis, dup, 20, mode=mode)
        assert s.stop_reason in ("captured", "no_candidates") and len(s.picks) == 6, (s.stop_reason, s.picks)
        assert len(set(map(tuple, s.points))) == 6
    # n = 0, unknown mode, a point outside the domain, limits
    with pytest.raises(ValueError):
        select_sensors_pbdw(sm, basis[:0], cand, 10)
    with pytest.raises(ValueError):
        select_sensors_pbdw(sm, basis, cand, 10, mode="best")
    bad = np.r_[cand[:5], [[sm.x_domain[0] - 0.5, 0.0]]]
    with pytest.raises(_ffi.RomLibraryError, match="outside the domain"):
        select_sensors_pbdw(sm, basis, bad, 3)
    with pytest.raises(_ffi.RomLibraryError, match="outside the domain"):
        sm.riesz_norms_h10(bad)
    with pytest.raises(_ffi.RomLibraryError, match="1 <= m <= 1024"):
        select_sensors_pbdw(sm, basis, cand, 1025)
