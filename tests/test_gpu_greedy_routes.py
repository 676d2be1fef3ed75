"""Both device routes of the strong greedy (src/lib/ReducedBasis.py:112-139) against the 80-bit greedy of tests/referee.py.

Routes: rows (rom_greedy, csrc/rom_basis.hip) and factored (rom_greedy_factored, csrc/rom_factored.hip, on the compact
interface vectors through the cached energy map).  For every case the device call runs, then referee.greedy_ld follows
the SAME picks in long double and returns the exact error vector e_i of every iteration.  Asserted per iteration i:
  (a) curve  |max_errors[i] - max(e_i)| <= bound_i;   (b) pick  e_i[picks[i]] >= max(e_i) - bound_i;
  (c) the same call twice gives the same picks and the same bits;  (d) on one factored block both routes pick alike
      wherever the long-double margin between the best and the second-best error exceeds 2 bound_i.

Bound model (errors relative to h1; E0 = max_m ||u_m|| / h1_m, the initial error scale; eps = 2^-53; C = 16):
  * H^1_0: each iteration updates the residuals once and forms their squared norms as sums; the squared errors carry an
    absolute error of at most delta_i = C (i + 1) eps E0^2, so |e_dev - e| <= min(sqrt(delta_i), delta_i / max(e_i)).
  * Galerkin: that, plus C contrast eps (i + 1) E0 for the reduced systems (condition <= contrast in an A_1-orthonormal
    basis, one more row per iteration).
  * factored route: plus the energy map's own error on the squared norms, (C Kc eps + (Kc - k1) PC_TOL) ||D y||^2 / h1^2 --
    the factorisation error of the equilibrated form and the trace of the Schur complement it drops at PC_TOL = 1e-14,
    both in the equilibrated coordinates D y (d_i^2 = the H^1_0 norm^2 of compact unit vector i).
"""
import numpy as np
import pytest

from conftest import observed
from oracle import rom_oracle as ro
import referee as rf

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -53
C_MODEL = 16.0
PC_TOL = 1e-14
LD = np.longdouble

_SM = {}


def _sm(blocks, N):
    from src.lib import SolutionsManagers as SM
    if (blocks, N) not in _SM:
        _SM[(blocks, N)] = SM.SolutionsManagerFEM(blocks, N)
    return _SM[(blocks, N)]


def _solve_class(n):
    return "n<=88" if n <= 88 else ("89<=n<=140" if n <= 140 else "n>140")


def _m_class(M):
    return "M=1" if M == 1 else ("M<1024" if M < 1024 else ("M=1024" if M == 1024 else "M>1024"))


COVERED = set()   # (route, mode, solve class, M class) reached by the cases of this module


def _map_scale2(sm, Yc_host, h1):
    """max_m ||D y_m||^2 / h1_m^2 (equilibrated squared norm of the compact coordinates)."""
    from romhighcontrast_amd import factored
    em = factored.expansion_map(sm)
    Kc = em.Kc
    Bt = sm._ctx.alloc(Kc * em.dim)
    em.expand_compact(sm._ctx.upload(np.eye(Kc)), Kc, Bt)
    d2 = sm._fem.h10norm(Bt, Kc) ** 2
    return float(np.max((Yc_host ** 2 @ d2) / np.broadcast_to(h1, (len(Yc_host),)) ** 2))


def _check(name, g, U, a, h1, picks, errs, galerkin, contrast=1.0, map_delta=0.0, route="rows"):
    """(a) and (b) against greedy_ld along the device's picks; returns the long-double error vectors."""
    n, M = len(picks), len(U)
    E, live = rf.greedy_ld(g, U, a, h1, picks, galerkin)
    E = np.asarray(E, dtype=np.float64)
    E0 = E[0].max()
    dev_curve, dev_pick = np.zeros(n), np.zeros(n)
    bounds = np.zeros(n)
    for i in range(n):
        delta = C_MODEL * (i + 1) * EPS * E0 ** 2 + map_delta
        top = E[i].max()
        b = min(np.sqrt(delta), delta / top) if top > 0 else np.sqrt(delta)
        if galerkin:
            b += C_MODEL * contrast * EPS * (i + 1) * E0
        bounds[i] = b
        dev_curve[i] = abs(errs[i] - top) / b
        dev_pick[i] = (top - E[i][picks[i]]) / b
    assert np.all(np.isfinite(errs))
    mode = "Galerkin" if galerkin else "H10"
    cuts = [(0, min(n, 88)), (88, min(n, 140)), (140, n)]
    for lo, hi in cuts:
        if hi <= lo:
            continue
        cls = _solve_class(hi) if galerkin else "-"
        COVERED.add((route, mode, cls, _m_class(M)))
        tag = f"{route}/{mode}/{cls}/{_m_class(M)} {name} it {lo}..{hi - 1}"
        observed(f"greedy {tag}: |curve - 80-bit| / bound", dev_curve[lo:hi], 1.0)
        observed(f"greedy {tag}: pick shortfall / bound", dev_pick[lo:hi], 1.0)
    return E, live, bounds


def _rows_call(sm, U, a, h1, n, galerkin, u_row0=0, Ubuf=None):
    ctx = sm._ctx
    M = len(U)
    if Ubuf is None:
        Ubuf = ctx.upload(U)
    a_dev = ctx.upload(np.ascontiguousarray(a.reshape(M, -1))) if galerkin else None
    return sm._fem.greedy(Ubuf, M, a_dev, h1, galerkin, n, u_row0=u_row0)


def _fact_call(sm, Yc, M, a, h1, n, galerkin, c_row0=0):
    ctx = sm._ctx
    a_dev = ctx.upload(np.ascontiguousarray(a.reshape(M, -1))) if galerkin else None
    return sm._fem.greedy_factored(Yc, M, a_dev, h1, galerkin, n, c_row0=c_row0)


def _random_factored(sm, M, seed):
    """Rows expanded from random interface vectors: (FactoredSnapshots, rows (M, dim), compact block (M, Kc))."""
    from romhighcontrast_amd import factored
    ctx, fem = sm._ctx, sm._fem
    Y = ctx.upload(np.random.default_rng(seed).standard_normal((M, fem.reduced_stride)))
    fs = factored.FactoredSnapshots(sm, Y, M)
    return fs, fs.rows().numpy(), fs.Yc.download(M * fs.map.Kc, shape=(M, fs.map.Kc))


def _snapshots_factored(sm, a):
    from romhighcontrast_amd import factored
    ctx, fem = sm._ctx, sm._fem
    M = len(a)
    Y = ctx.alloc(M * fem.reduced_stride)
    fem.solve_reduced(ctx.upload(a.reshape(M, -1)), M, Y)
    ctx.solve_status()
    fs = factored.FactoredSnapshots(sm, Y, M)
    return fs, fs.rows().numpy(), fs.Yc.download(M * fs.map.Kc, shape=(M, fs.map.Kc))


def _params(blocks, M, seed, decades):
    a = 10.0 ** np.random.default_rng(seed).uniform(0, decades, size=(M,) + blocks)
    return a, float(np.max(a.reshape(M, -1).max(1) / a.reshape(M, -1).min(1)))


# ---- H^1_0 mode: random rows, every M class ------------------------------------------------------------------------
GEO_H10 = ((3, 3), 12)       # dim 1225: n = 150 random directions stay well inside the space
GEO_WIDE = ((2, 2), 8)       # dim 225: the large-M cases


@pytest.mark.parametrize("M,n,h1kind", [(1, 3, "own"), (300, 150, "own"), (1024, 24, "one"), (1500, 24, "vec"), (4097, 16, "own")])
def test_rows_route_h10_random_rows(M, n, h1kind):
    blocks, N = GEO_H10 if M <= 300 else GEO_WIDE
    sm, g = _sm(blocks, N), ro.Geometry(blocks, N)
    rng = np.random.default_rng(M)
    U = rng.standard_normal((M, sm.vspace_dim)) * rng.uniform(0.5, 2.0, size=(M, 1))
    h1 = {"own": sm.H10norm(U), "one": 1.0, "vec": rng.uniform(0.5, 2.0, size=M)}[h1kind]
    a = np.ones((M,) + blocks)
    picks, errs = _rows_call(sm, U, a, h1, n, False)
    if h1kind != "own":
        assert picks[0] == int(np.argmax(sm.H10norm(U) / np.broadcast_to(h1, (M,))))
    _check(f"random rows M={M} h1={h1kind}", g, U, a, h1, picks, errs, False)
    picks2, errs2 = _rows_call(sm, U, a, h1, n, False)                       # (c)
    assert picks2 == picks and np.array_equal(errs2, errs)


# ---- Galerkin mode: snapshots (on random rows the Galerkin error of a picked row does not drop: it would be picked
# again and again), n up to 150 so the reduced solves inside the greedy take all three routes -----------------------
GEO_GAL = ((4, 4), 8)
# geometries with a linear expansion (the factored route), with Kc / k1 / k2 of their energy maps as read on an MI355X:
GEO_F = ((2, 2), 16)         # dim 961, Kc 208 (7 panels), k1 = k2 = 97 (inside panel 4)
GEO_F_BIG = ((3, 3), 40)     # dim 14161, Kc 736 (23 panels: the host's early-stop check runs), k1 = k2 = 551
GEO_LOWRANK = ((1, 1), 8)    # dim 49, Kc 16 (one panel), k1 = k2 = 1
MAP_GEOMETRIES = [GEO_LOWRANK, GEO_F, GEO_F_BIG]


@pytest.mark.parametrize("decades,n", [(2, 150), (8, 40)])
def test_rows_route_galerkin_snapshots(decades, n):
    blocks, N = GEO_GAL
    sm, g = _sm(blocks, N), ro.Geometry(blocks, N)
    M = 200
    a, contrast = _params(blocks, M, 40 + decades, decades)
    U = sm.generate_solutions(a)
    h1 = sm.H10norm(U)
    picks, errs = _rows_call(sm, U, a, h1, n, True)
    _check(f"snapshots contrast {contrast:.0e}", g, U, a, h1, picks, errs, True, contrast=contrast)
    picks2, errs2 = _rows_call(sm, U, a, h1, n, True)
    assert picks2 == picks and np.array_equal(errs2, errs)


# ---- the factored route ---------------------------------------------------------------------------------------------
def _factored_case(blocks, N, M, n, galerkin, decades, seed, h1kind="own"):
    sm, g = _sm(blocks, N), ro.Geometry(blocks, N)
    if not sm._fem.expansion_is_linear:
        pytest.fail(f"{blocks}/{N} has no linear expansion: choose another geometry for the factored cases")
    a, contrast = _params(blocks, M, seed, decades)
    if galerkin:
        fs, U, Ych = _snapshots_factored(sm, a)
    else:
        fs, U, Ych = _random_factored(sm, M, seed)
    h1 = {"own": sm.H10norm(U), "one": 1.0}[h1kind]
    k1, _ = fs.map.build()
    Kc = fs.map.Kc
    map_delta = (C_MODEL * Kc * EPS + max(Kc - k1, 0) * PC_TOL) * _map_scale2(sm, Ych, h1)
    picks, errs = _fact_call(sm, fs.Yc, M, a, h1, n, galerkin)
    E, live, bounds = _check(f"{'snapshots' if galerkin else 'random Y'} {blocks}/{N} Kc={Kc} k1={k1}", g, U, a, h1, picks,
                             errs, galerkin, contrast=contrast, map_delta=map_delta, route="factored")
    picks2, errs2 = _fact_call(sm, fs.Yc, M, a, h1, n, galerkin)
    assert picks2 == picks and np.array_equal(errs2, errs)
    return sm, fs, U, a, h1, picks, errs, E, bounds


@pytest.mark.parametrize("M,n", [(1, 3), (200, 150), (1024, 24), (1500, 20)])
def test_factored_route_h10_random_interface_vectors(M, n):
    blocks, N = GEO_F_BIG if M == 200 else GEO_F
    sm, fs, U, a, h1, picks, errs, E, bounds = _factored_case(blocks, N, M, n, False, 2, 100 + M)
    # (d) both routes on the same block: the same picks wherever the 80-bit margin exceeds twice the bound
    picks_r, errs_r = _rows_call(sm, U, a, h1, n, False)
    for i in range(n):
        if picks_r[:i] != picks[:i]:
            break
        top2 = np.sort(E[i])[-2:] if M > 1 else np.array([0.0, E[i][0]])
        if top2[1] - top2[0] > 2 * bounds[i]:
            assert picks_r[i] == picks[i], (i, picks_r[i], picks[i])


@pytest.mark.parametrize("decades,n", [(2, 150), (8, 40)])
def test_factored_route_galerkin_snapshots(decades, n):
    """(at GEO_F the snapshots span at most k1 = 97 directions: the iterations past that run with dead directions)"""
    blocks, N = GEO_F
    _factored_case(blocks, N, 200, n, True, decades, 60 + decades)


def test_build_default_on_generate_solutions_takes_the_factored_route(monkeypatch):
    """ReducedBasisGreedy.build on the host array generate_solutions returned runs rom_greedy_factored (both modes) and
    matches the 80-bit greedy along its picks."""
    from src.lib import ReducedBasis as RB
    from romhighcontrast_amd import factored
    blocks, N = GEO_F
    sm, g = _sm(blocks, N), ro.Geometry(blocks, N)
    M = 120
    a, contrast = _params(blocks, M, 77, 2)
    U = sm.generate_solutions(a)
    h1 = sm.H10norm(U)
    fs, _, Ych = _snapshots_factored(sm, a)
    k1, _ = fs.map.build()
    map_delta = (C_MODEL * fs.map.Kc * EPS + max(fs.map.Kc - k1, 0) * PC_TOL) * _map_scale2(sm, Ych, h1)
    calls = []
    real = factored.greedy_factored
    monkeypatch.setattr(factored, "greedy_factored", lambda *args, **kw: (calls.append(1), real(*args, **kw))[1])
    for mode, galerkin in ((RB.GREEDY_FOR_H10, False), (RB.GREEDY_FOR_GALERKIN, True)):
        calls.clear()
        rb = RB.ReducedBasisGreedy(mode).build(60, sm, U, a, h1)
        assert len(calls) == 1, mode
        _check("on generate_solutions", g, U, a, h1, rb.picks, rb.max_errors, galerkin, contrast=contrast,
               map_delta=map_delta, route="build-default")


# ---- ties, degenerate paths, offsets --------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ["rows", "factored"])
def test_exact_ties_take_the_first_index(route):
    """Duplicate rows at i < j (j - i = 1, 1024 and 3072: the same thread of kb_greedy_select, and across workgroup
    strides) carry bitwise-equal errors: the pick is the first index.  h1 = 1 makes the duplicated pair the first pick."""
    blocks, N = GEO_F
    sm = _sm(blocks, N)
    M = 4097
    rng = np.random.default_rng(9)
    if route == "rows":
        U = rng.standard_normal((M, sm.vspace_dim))
        for i, j, s in ((5, 3077, 64.0), (700, 1724, 32.0), (2000, 2001, 16.0)):
            U[i] *= s
            U[j] = U[i]
        picks, errs = _rows_call(sm, U, np.ones((M,) + blocks), 1.0, 3, False)
    else:
        from romhighcontrast_amd import factored
        Y = rng.standard_normal((M, sm._fem.reduced_stride))
        for i, j, s in ((5, 3077, 64.0), (700, 1724, 32.0), (2000, 2001, 16.0)):
            Y[i] *= s
            Y[j] = Y[i]
        fs = factored.FactoredSnapshots(sm, sm._ctx.upload(Y), M)
        picks, errs = _fact_call(sm, fs.Yc, M, None, 1.0, 3, False)
    assert picks == [5, 700, 2000], picks


@pytest.mark.parametrize("galerkin", [False, True])
def test_degenerate_picks_rows_and_factored(galerkin):
    """More picks than rows (n > M), duplicates picked at roundoff, and on the factored route n > k1 (rows in a space
    of rank k1): dead directions, finite curves, no failure of the reduced solves, and the curve still equal to the truth
    of the live span (a dead direction has coefficient 0 in Galerkin mode)."""
    blocks, N = GEO_F
    sm, g = _sm(blocks, N), ro.Geometry(blocks, N)
    M = 7
    a, contrast = _params(blocks, M, 5, 2)
    U0 = sm.generate_solutions(a)
    U, a2 = np.vstack((U0, U0[2:3])), np.concatenate((a, a[2:3]))
    h1 = sm.H10norm(U)
    n = M + 5
    picks, errs = _rows_call(sm, U, a2, h1, n, galerkin)
    E, live, _ = _check("duplicate row, n > M", g, U, a2, h1, picks, errs, galerkin, contrast=contrast)
    assert not live[:n - 1].all()
    fs, Uf, Ych = _snapshots_factored(sm, a2)
    picks, errs = _fact_call(sm, fs.Yc, len(a2), a2, h1, n, galerkin)
    k1, _ = fs.map.build()
    map_delta = (C_MODEL * fs.map.Kc * EPS + max(fs.map.Kc - k1, 0) * PC_TOL) * _map_scale2(sm, Ych, h1)
    _check("duplicate row, n > M", g, Uf, a2, h1, picks, errs, galerkin, contrast=contrast, map_delta=map_delta, route="factored")


@pytest.mark.parametrize("galerkin", [False, True])
def test_factored_route_beyond_the_map_rank(galerkin):
    """n > k1 on a geometry whose H^1_0 map has a small rank: the directions past k1 are dead on the device."""
    blocks, N = GEO_LOWRANK
    sm, g = _sm(blocks, N), ro.Geometry(blocks, N)
    k1, _ = sm._fem.energy_map(7)
    M = k1 + 20
    a, contrast = _params(blocks, M, 21, 2)
    fs, U, Ych = _random_factored(sm, M, 22) if not galerkin else _snapshots_factored(sm, a)
    h1 = sm.H10norm(U)
    n = k1 + 8
    picks, errs = _fact_call(sm, fs.Yc, M, a, h1, n, galerkin)
    map_delta = (C_MODEL * fs.map.Kc * EPS + max(fs.map.Kc - k1, 0) * PC_TOL) * _map_scale2(sm, Ych, h1)
    _check(f"n = k1 + 8 = {n}", g, U, a, h1, picks, errs, galerkin, contrast=contrast, map_delta=map_delta, route="factored")
    assert max(errs[k1:]) <= 1e-10 * errs[0], errs          # the rows span k1 directions: nothing left past them


@pytest.mark.parametrize("galerkin", [False, True])
def test_row_offsets_equal_a_copied_out_block(galerkin):
    blocks, N = GEO_F
    sm = _sm(blocks, N)
    ctx = sm._ctx
    M, off, n = 40, 13, 12
    a, _ = _params(blocks, M, 3, 2)
    fs, U, Ych = _snapshots_factored(sm, a)
    h1 = sm.H10norm(U)
    big = np.vstack((np.full((off, U.shape[1]), np.nan), U, np.full((3, U.shape[1]), np.nan)))
    assert _rows_call(sm, U, a, h1, n, galerkin, u_row0=off, Ubuf=ctx.upload(big)) == _rows_call(sm, U, a, h1, n, galerkin)
    bigc = np.vstack((np.full((off, Ych.shape[1]), np.nan), Ych, np.full((3, Ych.shape[1]), np.nan)))
    assert _fact_call(sm, ctx.upload(bigc), M, a, h1, n, galerkin, c_row0=off) == _fact_call(sm, ctx.upload(Ych), M, a, h1, n, galerkin)


# ---- the energy map -------------------------------------------------------------------------------------------------
def test_energy_map_classes_and_factored_norms_and_pod():
    """For every geometry of MAP_GEOMETRIES: Kc, k1, k2 printed; the list must reach one panel (Kc <= 32), several panels
    with k1 inside a panel, >= 9 panels (the host's early-stop check after panel 8), k1 < Kc and k2 < Kc.  Per geometry:
    h10norm_factored of random interface vectors against the 80-bit norm of their rows (bound C Kc eps + (Kc - k1) PC_TOL
    on the squared norm, relative to ||D y||^2), pod_factored against numpy.linalg.svd of the rows (centred and not), and
    take() giving the norms of the full block."""
    from romhighcontrast_amd import factored
    seen = set()
    for blocks, N in MAP_GEOMETRIES:
        sm, g = _sm(blocks, N), ro.Geometry(blocks, N)
        assert sm._fem.expansion_is_linear, (blocks, N)
        fs, U, Ych = _random_factored(sm, 48, N)
        k1, k2 = fs.map.build()
        Kc = fs.map.Kc
        print(f"energy map {blocks}/{N}: dim {sm.vspace_dim} Kc {Kc} k1 {k1} k2 {k2}")
        if Kc <= 32:
            seen.add("one panel")
        if Kc > 32 and k1 % 32 != 0 and k1 < Kc:
            seen.add("several panels, k1 inside a panel")
        if (Kc + 31) // 32 >= 9:
            seen.add(">= 9 panels")
        if k1 < Kc:
            seen.add("k1 < Kc")
        if k2 < Kc:
            seen.add("k2 < Kc")
        ref = np.array([float(rf.h10_ld(g, u.astype(LD))) for u in U])
        d2 = _map_scale2(sm, Ych, ref)
        got = factored.h10norm_factored(fs)
        bound2 = (C_MODEL * Kc * EPS + max(Kc - k1, 0) * PC_TOL) * d2
        observed(f"energy map {blocks}/{N}: |h10norm_factored^2 - 80-bit^2| / ||u||^2 (model {bound2:.1e})",
                 np.abs(got ** 2 / ref ** 2 - 1), bound2)
        sub = fs.take([7, 3, 40])
        assert np.array_equal(factored.h10norm_factored(sub), got[[7, 3, 40]])
        for center in (True, False):
            X = U - U.mean(axis=0) if center else U
            s_ref, Vt = np.linalg.svd(X, full_matrices=False)[1:]
            nm = min(12, k2 + 4, len(U))
            V = sm._ctx.alloc(nm * sm.vspace_dim)
            sig, info = sm._fem.pod_factored(fs.Yc, len(U), nm, V, center=center)
            modes = V.download(nm * sm.vspace_dim, shape=(nm, sm.vspace_dim))
            tol = C_MODEL * EPS * s_ref[0] * np.sqrt(Kc)
            observed(f"energy map {blocks}/{N}: POD centre={center} |sigma - LAPACK| / (C eps sigma_1 sqrt(Kc))",
                     np.abs(sig - s_ref[:nm]) / tol, 1.0)
            observed(f"energy map {blocks}/{N}: POD centre={center} orthonormality", np.abs(modes @ modes.T - np.eye(nm)), 1e-12)
            sep = [j for j in range(nm - 1) if s_ref[j] - s_ref[j + 1] > 1e-6 * s_ref[0] and s_ref[j] > 1e-8 * s_ref[0]]
            if sep:
                r = sep[-1] + 1
                Pm = modes[:r] @ Vt[:r].T
                observed(f"energy map {blocks}/{N}: POD centre={center} subspace of the {r} leading modes vs LAPACK",
                         1 - np.linalg.svd(Pm, compute_uv=False).min(), 1e-8)
    missing = {"one panel", "several panels, k1 inside a panel", ">= 9 panels", "k1 < Kc", "k2 < Kc"} - seen
    assert not missing, missing


def test_route_table_is_covered():
    """Runs last in this module: the cases above reached every route x mode x reduced-solve route x M class."""
    need = {("rows", "H10", "-", c) for c in ("M=1", "M<1024", "M=1024", "M>1024")}
    need |= {("factored", "H10", "-", c) for c in ("M=1", "M<1024", "M=1024", "M>1024")}
    need |= {(r, "Galerkin", c, "M<1024") for r in ("rows", "factored") for c in ("n<=88", "89<=n<=140", "n>140")}
    need |= {("build-default", m, c, "M<1024") for m, c in (("H10", "-"), ("Galerkin", "n<=88"))}
    missing = need - COVERED
    assert not missing, sorted(missing)
