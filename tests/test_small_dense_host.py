"""Host proof of tests/small_dense_truth.py (no GPU): the constructions are exact and their closed-form answers hold in exact
arithmetic; the restated round-robin order agrees with slot(); coverage_triples() covers every slot; the Newton-Schulz cases
sit on the intended sides of the entry condition; every bound has room (the plain fp64 restatement of the device's Jacobi
and numpy.linalg.eigh sit at least 8x inside); and the tests have teeth: the same restatement with the stop rule that
watches only the slots wave 0 of jacobi32_run owns, or with the Newton-Schulz entry at 3, misses by orders of magnitude."""
from fractions import Fraction

import numpy as np
import pytest

import small_dense_truth as sd

ROOM = 8.0
SMALL = [n for n in sd.ORDERS if n <= 98]


def _frac(M):
    return [[Fraction(float(x)) for x in row] for row in np.asarray(M)]


def _matmul(A, B):
    Bt = list(zip(*B))
    return [[sum((a * b for a, b in zip(row, col) if a and b), Fraction(0)) for col in Bt] for row in A]


# ---- the dispatch and the order ----------------------------------------------------------------------------------------
def test_route_table():
    assert [sd.route(n, 0) for n in (1, 32, 33, 96, 97, 2048)] == ["jacobi32", "jacobi32", "lds", "lds", "grid", "grid"]
    assert [sd.route(n, m) for n in (16, 32, 96, 97) for m in (1, 2)] == ["lds"] * 6 + ["grid"] * 2
    assert [sd.route(n, 3) for n in (1, 32, 33, 96)] == ["pivchol"] * 4
    with pytest.raises(AssertionError):
        sd.route(97, 3)
    with pytest.raises(AssertionError):
        sd.route(2049, 0)
    assert len(sd.reachable_cells()) == 3 + 9 + 9 + 1


@pytest.mark.parametrize("n", [2, 3, 16, 17, 31, 32, 33, 96, 97])
def test_slot_is_the_round_robin_order_of_the_kernels(n):
    """The pairs as jacobi32_run / kb_jgrid_round / kb_small_eig form them, round by round: every real pair exactly once per
    sweep, in the slot slot() names."""
    ne = n + (n & 1)
    nm1, half = ne - 1, ne // 2
    seen = {}
    for r in range(nm1):
        used = set()
        for k in range(half):
            p, q = (r, nm1) if k == 0 else sorted(((r + k) % nm1, (r - k) % nm1))
            assert p != q and not {p, q} & used
            used |= {p, q}
            if q < n:
                assert (p, q) not in seen
                seen[(p, q)] = k
    assert len(seen) == n * (n - 1) // 2
    assert all(sd.slot(p, q, n) == k for (p, q), k in seen.items())
    assert sorted(set(seen.values())) == sd.real_slots(n)


def test_wave0_slots():
    assert sd.wave0_slots(16) == list(range(8)) and sd.wave0_slots(32) == [0, 1, 2, 3]
    assert sd.wave0_slots(17) == list(range(8)) and len(sd.real_slots(17)) == 8 and 8 in sd.real_slots(17)
    assert sd.triple_slots((0, 1, 9), 32) == {15, 4, 11}


@pytest.mark.parametrize("n", [17, 24, 31, 32, 33, 95, 96, 97, 98])
def test_coverage_triples_cover_every_slot(n):
    tr = sd.coverage_triples(n)
    sd.assert_coverage(n, tr)
    assert all(0 <= a < b < c < n for a, b, c in tr) and len(set(tr)) == len(tr)
    if n == 32:
        assert tr[0] == (0, 1, 9)
    if n in (24, 31, 32):   # at least one triple none of whose slots wave 0 of jacobi32_run owns
        assert any(not sd.triple_slots(t, n) & set(sd.wave0_slots(n)) for t in tr)


# ---- exact spectra: exact constructions, exact eigenpairs ---------------------------------------------------------------
@pytest.mark.parametrize("n", sd.ORDERS)
def test_exact_cases_are_exact(n):
    for nn, fam in sd.exact_cases([n]):
        c = sd.ExactCase(nn, fam)
        A = c.A
        assert np.array_equal(A, A.T) and np.array_equal(A * 4, np.round(A * 4)) and np.abs(A).max() < 2.0 ** 40, c.id
        assert sorted(c.lam_all.tolist()) == sorted(np.round(c.lam_all).tolist())
        if fam in ("scalar", "null", "diagonal"):
            assert np.array_equal(A, np.diag(c.lam_all))
            continue
        # re-formed in integers: 4 A = (2 Q) B (2 Q) with 2 Q = 2 I - v v^T, permuted
        m, r = c.m, n - c.m
        H = sd.hadamard(m).astype(np.int64)
        B = np.zeros((n, n), dtype=np.int64)
        B[:m, :m] = (H * c.c) @ H.T
        B[m:, m:] = np.diag(c.e)
        v = c.v.astype(np.int64)
        Q2 = 2 * np.eye(n, dtype=np.int64) - np.outer(v, v)
        assert np.array_equal(Q2 @ Q2, 4 * np.eye(n, dtype=np.int64))          # Q is an orthogonal reflection
        A4 = (Q2 @ B @ Q2)[np.ix_(c.perm, c.perm)]
        assert np.array_equal(A4.astype(np.float64), 4 * A) and np.abs(A4).max() < 2 ** 50, c.id
        if n >= 4:
            assert int(np.abs(v).sum()) == 4 and (r == 0 or (np.abs(v[:m]).sum() > 0 and np.abs(v[m:]).sum() > 0))
        # the closed-form eigenpairs: A q = lam q exactly (q = the integer columns of 2 P Q W)
        W2 = c.W2.astype(np.int64)
        assert np.array_equal(W2.astype(np.float64), c.W2)
        lam = c.lam_all.astype(np.int64)
        assert np.array_equal(A4 @ W2, 4 * W2 * lam[None, :]), c.id
        G = W2.T @ W2                                                        # orthogonal columns of the stated norms
        assert np.array_equal(G, np.diag(np.diag(G))) and np.array_equal(np.diag(G), 4 * np.concatenate([np.full(m, m), np.ones(r, dtype=np.int64)]))
        if n <= 17:                                                           # and once more in rationals
            Wf = _frac(c.W2)
            AW = _matmul(_frac(A), Wf)
            assert all(AW[i][k] == Fraction(int(lam[k])) * Wf[i][k] for i in range(n) for k in range(n)), c.id


def test_exact_families_are_what_they_claim():
    for n in (3, 17, 32, 97):
        tri = sd.ExactCase(n, "triple")
        mult = max(len(cols) for _, cols in tri.clusters())
        assert mult == 3 and tri.lam_all.min() > 0
        ind = sd.ExactCase(n, "indefinite")
        assert ind.lam_all.min() < 0 < ind.lam_all.max() and len(set(ind.lam_all.tolist())) == n
        z = sd.ExactCase(n, "zero")
        assert (z.lam_all == 0).sum() == 1 and z.lam_all.min() == 0
        d = sd.ExactCase(n, "distinct")
        assert len(set(d.lam_all.tolist())) == n and d.lam_all.min() > 0
    dg = sd.ExactCase(31, "diagonal")
    assert len(set(dg.lam_all.tolist())) < 31 and list(dg.lam_all) != sorted(dg.lam_all, reverse=True)


# ---- inverse square roots --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [16, 32, 64, 128, 256])
@pytest.mark.parametrize("kind", list(sd.INVSQRT))
def test_invsqrt_cases_are_exact_and_on_their_sides(m, kind):
    c = sd.InvSqrtCase(m, kind)
    H = c.H.astype(np.int64)
    lev = [sd.INVSQRT[kind][i] for i in (8 * np.arange(m)) // m]
    d = np.array([0 if l is None else 4 ** l for l in lev], dtype=np.int64)
    root8 = np.array([0 if l is None else 8 >> l for l in lev], dtype=np.int64)   # 8 x 2^-l
    Gm = (H * d) @ H.T                                                           # m G
    Tm8 = (H * root8) @ H.T                                                      # 8 m G^(-1/2)
    assert np.array_equal(Gm.astype(np.float64), m * c.G) and np.array_equal(Tm8.astype(np.float64), 8 * m * c.Tinv)
    Pm = (H * (d > 0)) @ H.T                                                     # m x the projector on the range
    assert np.array_equal(Tm8 @ Gm @ Tm8, 64 * m * m * Pm)                       # T G T = Pi, in integers
    assert c.rank == (m if kind != "singular" else m - m // 8)
    esum, enter = sd.ns_entry(c.G)
    x = c.spectrum_over_g()
    if kind == "ns_converges":
        assert esum < 2 and enter and 0 < x.min() and x.max() < 2
    elif kind == "ns_above_two":
        assert esum < 2 and enter and 2 < x.max() < 3
    elif kind == "ns_wrong_root":
        assert 2 <= esum < 3 and not enter and 3 < x.max() < 4
    elif kind == "jacobi":
        assert esum >= 3 and not enter
    else:
        assert esum < 2 and enter and x.min() == 0
    if m <= 64:
        st, T = sd.newton_schulz_host(c.G)
        assert st == {"ns_converges": "converged", "ns_above_two": "converged", "ns_wrong_root": "skipped", "jacobi": "skipped",
                      "singular": "abandoned"}[kind]


def test_newton_schulz_entered_below_three_reaches_a_wrong_root():
    """Teeth of the inverse-square-root cases: with the entry condition at 3 the iteration takes G / g with an eigenvalue in
    (3, 4), its defect ||Z Y - I|| falls monotonically, and it converges -- to a root with a NEGATIVE eigenvalue: T G T = I holds,
    T is not G^(-1/2).  Against a bound of C n eps ||T|| ~ 2e-13 the entrywise error is 0.125."""
    c = sd.InvSqrtCase(32, "ns_wrong_root")
    st, T = sd.newton_schulz_host(c.G, entry=3.0)
    assert st == "converged"
    assert np.abs(T @ c.G @ T - np.eye(32)).max() < 1e-13 and np.linalg.eigvalsh(T).min() < -0.2
    assert np.abs(T - c.Tinv).max() > 0.1 > 1e9 * sd.C * 32 * sd.EPS * c.tnorm2
    assert sd.newton_schulz_host(c.G)[0] == "skipped"


# ---- pivoted Cholesky --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("b,variant", sd.pivchol_cases(), ids=[f"{v}-b{b}" for b, v in sd.pivchol_cases()])
def test_pivchol_cases_are_exact(b, variant):
    c = sd.PivCholCase(b, variant)
    r = c.rank
    assert c.X.shape == (b, c.mh)
    assert (variant == "rank") == (r < b) and (variant != "perm" or not np.array_equal(c.rows, np.arange(b)))
    if variant != "perm":
        dg = np.diag(c.G)[:r]
        assert np.all(dg[1:] < dg[:-1])                                       # strictly decreasing: no pivot swaps
    if b <= 62:
        Xf = _frac(c.X)
        Gf = _matmul(Xf, [list(col) for col in zip(*Xf)])
        assert all(Gf[i][j] == Fraction(float(c.G[i, j])) for i in range(b) for j in range(b))       # G = X X^T exactly
        Tf = _frac(c.T)
        TG = _matmul(_matmul(Tf, Gf), [list(col) for col in zip(*Tf)])
        assert all(TG[i][j] == (1 if i == j and i < r else 0) for i in range(b) for j in range(b))   # T G T^T = I_r (+) 0
    # the plain fp64 pivoted Cholesky reproduces the exact transform and pivots bit for bit: every operation on these dyadic
    # entries is exact (square roots of even powers of two, divisions by powers of two, short sums)
    lam, T = sd.pivchol_host(c.G)
    assert np.array_equal(T, c.T) and np.array_equal(lam, c.lam), c.id
    assert not T[r:].any() and not lam[r:].any()


# ---- bounds have room -------------------------------------------------------------------------------------------------------
def _eigh_desc(A):
    w, V = np.linalg.eigh(A)
    return w[::-1].copy(), V[:, ::-1].T.copy()


def _inside(measures, tag):
    for name, v, b in measures:
        assert v * ROOM <= b, (tag, name, v, b)


@pytest.mark.parametrize("n", SMALL + [128, 129, 256])
def test_exact_spectra_bounds_have_room(n):
    """jacobi_host (the device's order and criterion in plain fp64) and LAPACK, 8x inside every bound of the exact-spectrum
    cases; orders above 98 with the distinct family only (the restatement is a Python loop over rounds)."""
    fams = sd.FAMILIES if n <= 98 else ("distinct",)
    for nn, fam in sd.exact_cases([n]):
        if fam not in fams:
            continue
        c = sd.ExactCase(nn, fam)
        for gl in ((0,) if fam in ("indefinite", "diagonal") else (0, 1) if n <= 98 else (1,)):
            lam, T, _ = sd.jacobi_host(c.A, gl)
            _inside(sd.exact_measures(c, lam, T), (c.id, gl, "jacobi_host"))
            if fam in ("scalar", "null", "diagonal"):
                assert np.array_equal(lam, c.sorted_lam()) and np.array_equal(T, np.eye(n)[np.argsort(-c.lam_all, kind="stable")])
        lam, T = _eigh_desc(c.A)
        _inside(sd.exact_measures(c, lam, T), (c.id, "eigh"))


@pytest.fixture(scope="module")
def coupled():
    out = {}
    for n in (17, 24, 31, 32, 33):
        out[n] = [sd.CoupledCase(n, t) for t in sd.coverage_triples(n)]
    for n in (95, 96, 97, 98):
        out[n] = [sd.CoupledCase(n, t) for t in sd.coverage_triples(n)[:3]]
    return out


@pytest.mark.parametrize("n", [17, 24, 31, 32, 33, 95, 96, 97, 98])
def test_pair_coverage_bounds_have_room(coupled, n):
    for c in coupled[n]:
        bound = sd.C * n * sd.EPS * c.norm2
        for gl in (0, 1):
            lam, T, sweeps = sd.jacobi_host(c.A, gl)
            assert np.abs(lam - c.lam).max() * ROOM <= bound and sweeps >= 2, (c.id, gl)
            _inside(sd.eig_measures(c.A, lam, T, c.norm2), (c.id, gl))
        lam, T = _eigh_desc(c.A)
        assert np.abs(lam - c.lam).max() * ROOM <= bound, c.id


def test_wave0_stop_rule_fails_the_pair_coverage_cases(coupled):
    """The restatement with the stop rule jacobi32_run had -- only the rotations of the slots whose threads sit in wave 0 end
    or continue the sweeps -- on the cases the device test runs.  n = 32, triple (0, 1, 9): every rotation of the first sweep
    falls in slots 15, 4, 11; the iteration stops after ONE sweep with an eigenvalue error of 1.5e-3 against a bound of
    7.3e-12."""
    c = coupled[32][0]
    assert c.triple == (0, 1, 9)
    bound = sd.C * 32 * sd.EPS * c.norm2
    assert 7.0e-12 < bound < 7.5e-12
    lam, _, sweeps = sd.jacobi_host(c.A, 1, rule="wave0")
    err = np.abs(lam - c.lam).max()
    assert sweeps == 0 and err >= 1e-4, (sweeps, err)
    lam, _, sweeps = sd.jacobi_host(c.A, 1, rule="all")
    assert sweeps >= 3 and np.abs(lam - c.lam).max() * ROOM <= bound
    for n in (24, 31, 32):      # every order whose slots wave 0 does not all own has cases that fail by orders of magnitude
        worst = max(np.abs(sd.jacobi_host(cc.A, 1, rule="wave0")[0] - cc.lam).max() for cc in coupled[n])
        assert worst > 1e6 * sd.C * n * sd.EPS * coupled[n][0].norm2, (n, worst)


@pytest.mark.parametrize("m", [16, 32, 64, 128])
def test_inverse_square_root_bounds_have_room(m):
    for kind in sd.INVSQRT:
        c = sd.InvSqrtCase(m, kind)
        for mode in (1, 2):
            lam, T, path = sd.small_eig_host(c.G, mode, c.rel_tol, 1)
            tag = (c.id, mode, path)
            if path == "ns" or mode == 2:
                assert np.abs(T - c.Tinv).max() * ROOM <= sd.C * m * sd.EPS * c.tnorm2, tag
            v, b = sd.whitening_measure(c.G, T, c.rank, c.kappa) if not (kind == "singular" and mode == 2) else (0.0, 1.0)
            assert v * ROOM <= b, tag
            if kind == "singular" and mode == 1:
                assert path == "jacobi" and not T[c.rank:].any() and np.abs(lam[c.rank:]).max() < c.rel_tol * lam[0]
            if path == "jacobi":
                assert np.abs(lam - np.sort(c.d)[::-1]).max() * ROOM <= sd.C * m * sd.EPS * c.norm2, tag
            else:
                assert np.array_equal(lam, np.diag(c.G)), tag
        # LAPACK through the same formulas
        w, V = _eigh_desc(c.G)
        T = sd.transform_from_eig(w, V, 2, c.rel_tol)
        assert np.abs(T - c.Tinv).max() * ROOM <= sd.C * m * sd.EPS * c.tnorm2, c.id


@pytest.fixture(scope="module")
def graded():
    return {n: sd.GradedCase(n) for n in (24, 40)}


@pytest.mark.parametrize("n", [24, 40])
def test_graded_bound_has_room(graded, n):
    """Relative accuracy C n eps kappa(B) of every eigenvalue of D B D over 32 decades: the restatement with the relative
    criterion, gram_like 1 and 2, 8x inside.  (LAPACK's eigh promises absolute accuracy only: it is no witness here.)"""
    g = graded[n]
    assert 1 <= g.kappa < 10
    for gl in (1, 2):
        lam, T, _ = sd.jacobi_host(g.A, gl)
        assert (np.abs(lam - g.lam) / g.lam).max() * ROOM <= sd.C * n * sd.EPS * g.kappa, (n, gl)
        assert sd.norm2_ld(np.asarray(T, dtype=sd.LD) @ np.asarray(T, dtype=sd.LD).T - np.eye(n)) * ROOM <= sd.C * n * sd.EPS
