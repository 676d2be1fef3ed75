"""The small dense layer of the basis stage on the device -- ctx.small_eig (rom_small_eig_host) on all four routes and
ctx.symmetric_orthonormalize -- against the truths of tests/small_dense_truth.py (proved on the CPU by
tests/test_small_dense_host.py, where the plain fp64 restatement of the same Jacobi sits 8x inside every bound used here).

  * exact spectra: every order on both sides of the switches 32 | 33 and 96 | 97, odd and even; distinct, triple, indefinite,
    singular, c I, zero and already diagonal matrices; eigenvalues, eigenspaces, orthonormality, residual, order.
  * pair coverage: diag(1..n) + one coupled index triple, over triples that visit every slot of the round-robin order.
  * modes 1 and 2 against exact inverse square roots around the Newton-Schulz entry, on the LDS and the grid route.
  * mode 3 against the exact pivoted-Cholesky transform (plain, permuted, rank deficient).
  * graded matrices over 32 decades: relative accuracy.
  * every call twice and once under ROMHC_POISON_WS: the same bits.
  * the routes confirmed by profile names in a child process (tests/small_dense_child.py).
With ROMHC_SMALL_DENSE_JSON set, one JSON line per case (route, n, mode, observed / bound) is appended to that file."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import referee as rf
import small_dense_truth as sd
from conftest import observed
from small_dense_truth import C, EPS

pytestmark = pytest.mark.gpu

NS_ORDERS = (16, 32, 64, 128, 256)
PAIR_ALL = (17, 24, 31, 32, 33, 95, 96)
PAIR_THREE = (97, 98)
PIVCHOL = sd.pivchol_cases()
GRADED = (24, 40)


def exact_params(n):
    out = []
    for _, fam in sd.exact_cases([n]):
        gls = (0,) if fam in ("indefinite", "diagonal") else (0, 1, 2) if fam == "distinct" else (0, 1)
        out += [(fam, gl) for gl in gls]
    return out


def all_cells():
    """(route, mode, gram_like) of every parametrised call of this module."""
    cells = set()
    for n in sd.ORDERS:
        cells |= {(sd.route(n, 0), 0, gl) for _, gl in exact_params(n)}
    for n in PAIR_ALL + PAIR_THREE:
        cells |= {(sd.route(n, 0), 0, gl) for gl in (0, 1)}
    for m in NS_ORDERS:
        cells |= {(sd.route(m, mode), mode, gl) for mode in (1, 2) for gl in (0, 1, 2)}
    cells |= {(sd.route(b, 3), 3, 1) for b, _ in PIVCHOL}
    cells |= {(sd.route(n, 0), 0, gl) for n in GRADED for gl in (1, 2)}
    return cells


def test_every_reachable_cell_is_reached():
    missing = sd.reachable_cells() - all_cells()
    assert not missing, sorted(missing)
    assert all_cells() == sd.reachable_cells()
    for rt, orders in (("jacobi32", (1, 2, 3, 16, 17, 31, 32)), ("lds", (33, 64, 95, 96)), ("grid", (97, 98, 128, 129, 256))):
        assert all(sd.route(n, 0) == rt for n in orders)


@pytest.fixture(scope="module")
def ctx():
    from romhighcontrast_amd import _ffi
    return _ffi.get_context()


def _bits(x):
    return np.ascontiguousarray(x).tobytes()


def call(ctx, monkeypatch, A, mode, rel_tol, gl, tag):
    """ctx.small_eig three times: as is, again, and with the workspaces poisoned -- the same bits each time."""
    lam, T = ctx.small_eig(A, mode=mode, rel_tol=rel_tol, gram_like=gl)
    lam2, T2 = ctx.small_eig(A, mode=mode, rel_tol=rel_tol, gram_like=gl)
    assert _bits(lam2) == _bits(lam) and _bits(T2) == _bits(T), (tag, "repeat")
    monkeypatch.setenv("ROMHC_POISON_WS", "1")
    lam3, T3 = ctx.small_eig(A, mode=mode, rel_tol=rel_tol, gram_like=gl)
    monkeypatch.delenv("ROMHC_POISON_WS")
    assert _bits(lam3) == _bits(lam) and _bits(T3) == _bits(T), (tag, "poisoned")
    assert np.all(np.isfinite(lam)) and np.all(np.isfinite(T)), tag
    return lam, T


class Worst:
    """Collects (name, observed, bound) over the cases of one test; asserts each through conftest.observed as a ratio."""

    def __init__(self, head):
        self.head, self.rows = head, {}

    def add(self, rt, n, mode, gl, case_id, measures):
        sd.record(rt, n, mode, gl, case_id, measures)
        for name, v, b in measures:
            ratio = v / b if b > 0 else (0.0 if v == 0 else np.inf)
            old = self.rows.get(name)
            if old is None or ratio > old[0]:
                self.rows[name] = (ratio, f"{case_id} gram_like={gl}: {v:.3e} against {b:.3e}")

    def check(self):
        for name, (ratio, detail) in self.rows.items():
            print(f"{self.head}: {name}: {ratio:.3e} of the bound ({detail})")
        for name, (ratio, detail) in self.rows.items():
            observed(f"{self.head}: {name} / bound", ratio, 1.0, detail=detail)


# ---- exact spectra --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", sd.ORDERS)
def test_exact_spectra(ctx, monkeypatch, n):
    """Mode 0.  Eigenvalues within C n eps ||A||; each eigenspace (a spectral projector for the triple eigenvalue) within the
    angle C n eps ||A|| / gap; ||T T^T - I|| and ||T A T^T - diag(lam)|| / ||A|| within C n eps (long double); lam descending.
    c I, the zero matrix and a diagonal matrix with ties return exact values and the permutation that keeps ties in index
    order (the identity for the first two)."""
    rt = sd.route(n, 0)
    w = Worst(f"small_eig exact n={n} ({rt})")
    for fam, gl in exact_params(n):
        c = sd.ExactCase(n, fam)
        lam, T = call(ctx, monkeypatch, c.A, 0, 0.0, gl, (c.id, gl))
        assert np.all(np.diff(lam) <= 0), (c.id, gl, "descending")
        if fam in ("scalar", "null", "diagonal"):
            order = np.argsort(-c.lam_all, kind="stable")
            assert np.array_equal(lam, c.lam_all[order]) and np.array_equal(T, np.eye(n)[order]), (c.id, gl, "exact, ties in index order")
        w.add(rt, n, 0, gl, c.id, sd.exact_measures(c, lam, T))
    w.check()


# ---- pair coverage --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def coupled():
    out = {n: [sd.CoupledCase(n, t) for t in sd.coverage_triples(n)] for n in PAIR_ALL}
    out.update({n: [sd.CoupledCase(n, t) for t in sd.coverage_triples(n)[:3]] for n in PAIR_THREE})
    return out


@pytest.mark.parametrize("n", PAIR_ALL + PAIR_THREE)
def test_pair_coverage(ctx, monkeypatch, coupled, n):
    """diag(1..n) + a dense 3 x 3 coupling on one index triple: the only rotations of the first sweep sit in the slots of the
    triple's three pairs, and the triples between them visit every slot.  A solver whose sweep-end test misses a slot stops
    after one sweep with an error of 1e-3 (n = 32, triple (0, 1, 9): 1.5e-3 in the restatement of that rule)."""
    rt = sd.route(n, 0)
    if n in PAIR_ALL:
        sd.assert_coverage(n, [c.triple for c in coupled[n]])
    w = Worst(f"small_eig pair coverage n={n} ({rt})")
    for c in coupled[n]:
        for gl in (0, 1):
            lam, T = call(ctx, monkeypatch, c.A, 0, 0.0, gl, (c.id, gl))
            m = [("eigenvalues |lam - truth|", float(np.abs(lam - c.lam).max()), C * n * EPS * c.norm2)]
            w.add(rt, n, 0, gl, c.id, m + sd.eig_measures(c.A, lam, T, c.norm2))
    w.check()


# ---- whitening and symmetric inverse square root -------------------------------------------------------------------------------
@pytest.mark.parametrize("m", NS_ORDERS)
def test_whiten_and_lowdin_exact_inverse_square_roots(ctx, monkeypatch, m):
    """G = H diag(4^j) H^T / m with G^(-1/2) = H diag(2^-j) H^T / m exactly, in five situations (small_dense_truth.INVSQRT):
    Newton-Schulz converges; converges with an eigenvalue of G / g above 2; row-sum bound in [2, 3) with an eigenvalue of G / g
    above 3 (an iteration entered there converges to a root with a negative eigenvalue: the result is compared entrywise);
    bound >= 3; singular (entered, abandoned, Jacobi, the zero eigenvalue dropped by rel_tol).  On the fast path the kernel
    reports the diagonal of G as lam and the symmetric root for both modes; that path is predicted by the restatement and
    asserted through lam."""
    w = Worst(f"small_eig modes 1, 2 n={m}")
    for kind in sd.INVSQRT:
        c = sd.InvSqrtCase(m, kind)
        ns = m <= sd.LDS_MAX and sd.newton_schulz_host(c.G)[0] == "converged"
        for mode in (1, 2):
            rt = sd.route(m, mode)
            for gl in (0, 1, 2):
                tag = (c.id, mode, gl)
                lam, T = call(ctx, monkeypatch, c.G, mode, c.rel_tol, gl, tag)
                meas = []
                if ns:
                    assert np.array_equal(lam, np.diag(c.G)), (tag, "fast path: lam is the diagonal")
                else:
                    meas.append(("eigenvalues |lam - truth|", float(np.abs(lam - np.sort(c.d)[::-1]).max()), C * m * EPS * c.norm2))
                if ns or mode == 2:
                    meas.append(("entries of T against the exact G^(-1/2)", float(np.abs(T - c.Tinv).max()), C * m * EPS * c.tnorm2))
                if not (kind == "singular" and mode == 2):
                    v, b = sd.whitening_measure(c.G, T, c.rank, c.kappa)
                    meas.append(("||T G T^T - I||_2 against C n eps kappa(G)", v, b))
                if kind == "singular" and mode == 1:
                    assert not T[c.rank:].any(), (tag, "dropped direction: a zero row")
                    assert np.abs(lam[c.rank:]).max() <= c.rel_tol * lam[0], tag
                w.add(rt, m, mode, gl, c.id, meas)
    w.check()


# ---- pivoted Cholesky --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("b,variant", PIVCHOL, ids=[f"{v}-b{b}" for b, v in PIVCHOL])
def test_pivoted_cholesky_exact_factor(ctx, monkeypatch, b, variant):
    """Mode 3 on X = diag(2^-i) L0 R: T within 2 ulps per entry of L0^-1 diag(2^i) / sqrt(mh), zero entries exactly zero, lam
    the squared pivots, zeros behind the rank.  None of the kernels' operations rounds on these inputs -- the pivots are even
    powers of two (sqrt exact), every division (kb_pivchol_whiten) or multiplication by the reciprocal (kb_pivchol_whiten32) is
    by a power of two, the updates and the forward substitution add dyadic numbers of a few bits -- so the transform is
    expected bit for bit (as the fp64 restatement gives it on the host); the bound stays at the 2 ulps of the contract."""
    c = sd.PivCholCase(b, variant)
    lam, T = call(ctx, monkeypatch, c.G, 3, 0.0, 1, c.id)
    ulp = np.spacing(np.abs(c.T))
    zero = c.T == 0
    assert not T[zero].any(), (c.id, "entries that are exactly zero")
    meas = [("T against the exact transform (ulps)", float((np.abs(T - c.T)[~zero] / ulp[~zero]).max()), 2.0),
            ("lam against the squared pivots (ulps)", float((np.abs(lam - c.lam)[:c.rank] / np.spacing(c.lam[:c.rank])).max()), 2.0)]
    assert not lam[c.rank:].any() and not T[c.rank:].any(), (c.id, "behind the rank")
    w = Worst(f"small_eig mode 3 {variant} b={b}")
    w.add("pivchol", b, 3, 1, c.id, meas)
    w.check()


# ---- graded --------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def graded():
    return {n: sd.GradedCase(n) for n in GRADED}


@pytest.mark.parametrize("n", GRADED)
def test_graded_relative_accuracy(ctx, monkeypatch, graded, n):
    """A = D B D, D = powers of two over sixteen decades (eigenvalues over 32), B well conditioned; truth mpmath.eigsy of the
    exact fp64 matrix at 90 digits.  Every eigenvalue within C n eps kappa(B) RELATIVE, gram_like 1 and 2; n = 24 on
    jacobi32_run, n = 40 in LDS (test_gpu_pca_tall covers n = 81 and 300)."""
    g = graded[n]
    rt = sd.route(n, 0)
    w = Worst(f"small_eig graded n={n} ({rt}), kappa = {g.kappa:.2f}")
    for gl in (1, 2):
        lam, T = call(ctx, monkeypatch, g.A, 0, 0.0, gl, (g.id, gl))
        Tl = np.asarray(T, dtype=sd.LD)
        w.add(rt, n, 0, gl, g.id, [("relative eigenvalue error", float((np.abs(lam - g.lam) / g.lam).max()), C * n * EPS * g.kappa),
                                   ("orthonormality ||T T^T - I||_2", sd.norm2_ld(Tl @ Tl.T - np.eye(n)), C * n * EPS)])
    w.check()


# ---- rom_symmetric_orthonormalize ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["ns_converges", "jacobi"])
@pytest.mark.parametrize("n", [96, 97])
def test_symmetric_orthonormalize_polar_factor(ctx, monkeypatch, n, kind):
    """Rows X = S W with W = n rows of H_256 / 16 (orthonormal, exact) and S = (H diag(2^j) H^T / 64) (+) diag(2^j') symmetric
    positive definite: X is exact, X X^T = S^2 exactly, and the polar factor -- what (X X^T)^(-1/2) X must return -- is W.
    n = 96: kb_small_eig in LDS (Newton-Schulz or Jacobi by `kind`); n = 97: the grid route with its transpose + GEMM.  Error
    of the first round: C n eps ||S^-1|| ||S|| in the 2-norm (the transform within C n eps ||S^-1||, applied to rows of norm
    <= ||S||); the second round leaves it there.  NaN guard rows on both sides of the block stay NaN."""
    dim, m = 256, 64
    c = sd.InvSqrtCase(m, kind)
    lev = np.array(sd.INVSQRT[kind])[(8 * np.arange(m)) // m]
    S = np.zeros((n, n))
    S[:m, :m] = (c.H * 2.0 ** lev) @ c.H.T / m
    S[m:, m:] = np.diag(2.0 ** (np.arange(n - m) % 2))
    Wt = rf.hadamard_columns(dim, np.arange(1, n + 1)).T / 16.0
    X = S @ Wt
    kappa = 2.0 ** lev.max()
    buf = np.full((n + 2, dim), np.nan)
    buf[1:n + 1] = X

    def run():
        V = ctx.upload(buf)
        ctx.symmetric_orthonormalize(V, n, dim, v_row0=1)
        return V.download(shape=(n + 2, dim))

    out = run()
    assert _bits(run()) == _bits(out), "repeat"
    monkeypatch.setenv("ROMHC_POISON_WS", "1")
    out3 = run()
    monkeypatch.delenv("ROMHC_POISON_WS")
    assert _bits(out3) == _bits(out), "poisoned"
    assert np.isnan(out[0]).all() and np.isnan(out[n + 1]).all() and np.isfinite(out[1:n + 1]).all(), "guard rows"
    V = out[1:n + 1]
    Vl = np.asarray(V, dtype=sd.LD)
    rt = sd.route(n, 2)
    w = Worst(f"symmetric_orthonormalize n={n} ({rt}, {kind})")
    w.add(rt, n, 2, 1, f"polar-{kind}-n{n}", [("||V - W||_2 against C n eps kappa(S)", sd.norm2_ld(Vl - Wt), C * n * EPS * kappa),
                                             ("||V V^T - I||_2", sd.norm2_ld(Vl @ Vl.T - np.eye(n)), C * n * EPS)])
    w.check()


# ---- which code ran: a child process (ROMHC_PROF_DETAIL is read once per process) ---------------------------------------------
def test_routes_confirmed_by_profile_names():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k != "ROMHC_POISON_WS"}
    env["ROMHC_PROF_DETAIL"] = "1"
    r = subprocess.run([sys.executable, os.path.join(root, "tests", "small_dense_child.py")], env=env, cwd=root,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    out = r.stdout.decode(errors="replace")
    print(out)
    assert r.returncode == 0 and out.rstrip().endswith("OK"), out[-4000:]
    rows = [json.loads(ln[6:]) for ln in out.splitlines() if ln.startswith("ROUTE ")]
    assert len(rows) >= 3 * len(sd.ORDERS)
    seen = set()
    for row in rows:
        want = sd.route(row["n"], row["mode"])
        told = {"grid": "grid", "pivchol": "pivchol", "jacobi32": "one_workgroup", "lds": "one_workgroup"}[want]
        assert row["profile_says"] == told, row
        seen.add(want)
    assert seen == {"jacobi32", "lds", "grid", "pivchol"}
