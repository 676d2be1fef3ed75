"""Truths for the FE-operator layer (rom_assemble_batch, rom_stencil_apply, rom_h10norm, rom_evaluate_points, the reduced
solves and the two projectors).  TEST INFRASTRUCTURE: imports the oracle and tests/referee.py; nothing in the product path
may import this.  tests/test_fe_truth_host.py proves every helper on the CPU before tests/test_gpu_fe_ops.py relies on it.

EXACT cases.  Block coefficients a = m 2^e with 1 <= m <= 7, |e| <= E = 16, vector entries integers with |x| <= 2^XB,
XB = 14.  In units of q = 2^-(E+1) every coefficient is an even integer <= 7 2^(2E+1); the cell sums k00 + k01 (+ k10 + k11)
and the halved sums -(k11 + k01) / 2 of the stencil are integers below 2^(2E+6); a row of |A| sums to at most twice its
diagonal, < 2^(2E+7); so every product, every partial sum of a row of A x in any order, and the exact value a fused
multiply-add rounds, is an integer multiple of q below 2^(2E+7+XB) q = 2^53 q: representable.  The result of ANY correct
fp64 evaluation equals the integer one.  The helpers compute in int64 (exact: the same bound keeps it far from 2^63), assert
the bound on the numbers they produced (sum |A_ij| |x_j| < 2^53 q entrywise), and recompute a sample of entries -- corners,
block boundaries, seeded random ones -- in Python int / fractions.Fraction arithmetic from the fp64 inputs.

x^T A_1 x = sum over mesh edges of (x_i - x_j)^2 (boundary values 0) is a sum of non-negative integers: exact in any order
while the total stays below 2^53, which the helper asserts; the norm is math.sqrt of that integer (correctly rounded).
"""
import math
from fractions import Fraction

import numpy as np
import scipy.linalg

from oracle import rom_oracle as ro
import referee as rf

LD = np.longdouble
U53 = 2.0 ** -53
E_MAX, XB = 16, 14
Q_UNIT = 2.0 ** -(E_MAX + 1)

# (blocks, N): the smallest geometries at which each mechanism of the stencil-shaped kernels can go wrong
GEOMETRIES = [((1, 2), 2), ((1, 1), 3), ((1, 1), 65), ((1, 1), 66), ((1, 1), 257), ((1, 1), 258), ((2, 3), 11), ((3, 2), 11),
              ((3, 3), 33), ((1, 4), 65), ((4, 1), 65), ((8, 8), 3)]


def geom_id(gm):
    (p, q), N = gm
    return f"{p}x{q}-N{N}"


def gamma(k):
    return k * U53 / (1 - k * U53)


# ---- exact coefficients and operators ---------------------------------------------------------------------------------
def exact_coefficients(rng, shape):
    """a = m 2^e, 1 <= m <= 7, |e| <= E_MAX: (fp64 values, the same in units of Q_UNIT as int64)."""
    m = rng.integers(1, 8, size=shape)
    e = rng.integers(-E_MAX, E_MAX + 1, size=shape)
    ai = m.astype(np.int64) << (e + E_MAX + 1).astype(np.int64)
    a = np.ldexp(m.astype(np.float64), e.astype(np.int32))
    assert np.array_equal(a, ai.astype(np.float64) * Q_UNIT)
    return a, ai


def _stencil_int(g, ai):
    """diag / east / north in units of Q_UNIT (int64) of coefficients ai (..., nrb, ncb) given in the same units."""
    ai = np.asarray(ai, dtype=np.int64).reshape(ai.shape[:-2] + (g.nrb, g.ncb))
    k = np.repeat(np.repeat(ai, g.N, axis=-2), g.N, axis=-1)
    nr, nc = g.nr, g.nc
    diag = k[..., 0:nr, 0:nc] + k[..., 0:nr, 1:nc + 1] + k[..., 1:nr + 1, 0:nc] + k[..., 1:nr + 1, 1:nc + 1]
    es = k[..., 1:nr + 1, 1:nc] + k[..., 0:nr, 1:nc]
    ns = k[..., 1:nr, 1:nc + 1] + k[..., 1:nr, 0:nc]
    assert not (es & 1).any() and not (ns & 1).any()
    return diag, -(es // 2), -(ns // 2)


def _kappa_frac(g, a, line, col):
    """Cell coefficient as a Fraction, 0-based cell (line, col), from the fp64 block coefficients a (nrb, ncb)."""
    return Fraction(float(a[line // g.N][col // g.N]))


def stencil_entry_frac(g, a, r, c):
    """(diag, east, north, west, south) couplings of inner vertex (r, c) (0-based) as Fractions, from fp64 a (nrb, ncb):
    the closed form of the reference's triangle loop, in rational arithmetic."""
    k00, k01 = _kappa_frac(g, a, r, c), _kappa_frac(g, a, r, c + 1)
    k10, k11 = _kappa_frac(g, a, r + 1, c), _kappa_frac(g, a, r + 1, c + 1)
    return k00 + k01 + k10 + k11, -(k11 + k01) / 2, -(k01 + k00) / 2, -(k10 + k00) / 2, -(k11 + k10) / 2


def apply_entry_frac(g, a, x, r, c):
    """(A(a) x)[r, c] as a Fraction; x (nr, nc) of fp64 numbers."""
    d, e, n, w, s = stencil_entry_frac(g, a, r, c)
    at = lambda i, j: Fraction(float(x[i, j])) if 0 <= i < g.nr and 0 <= j < g.nc else Fraction(0)
    return d * at(r, c) + e * at(r, c + 1) + w * at(r, c - 1) + s * at(r + 1, c) + n * at(r - 1, c)


def sample_entries(g, rng, count=24):
    """Inner vertices worth recomputing by hand: corners, both sides of every block boundary, random ones."""
    rows = {0, g.nr - 1} | {r for b in range(1, g.nrb) for r in (b * g.N - 2, b * g.N - 1, b * g.N) if 0 <= r < g.nr}
    cols = {0, g.nc - 1} | {c for b in range(1, g.ncb) for c in (b * g.N - 2, b * g.N - 1, b * g.N) if 0 <= c < g.nc}
    rows, cols = sorted(rows)[:12], sorted(cols)[:12]
    pts = {(r, c) for r in rows for c in cols}
    pts |= {(int(rng.integers(g.nr)), int(rng.integers(g.nc))) for _ in range(count)}
    return sorted(pts)


def exact_assemble_case(blocks, N, M, seed):
    """M exact parameters -> (a (M, nrb, ncb), diag (M, nr, nc), east (M, nr, nc-1), north (M, nr-1, nc)), all fp64 and all
    exact (see the module docstring); a sample of entries is re-derived in Fractions."""
    g = ro.Geometry(blocks, N)
    rng = np.random.default_rng(seed)
    a, ai = exact_coefficients(rng, (M, g.nrb, g.ncb))
    di, ei, ni = _stencil_int(g, ai)
    assert int(np.abs(di).max()) < 2 ** (2 * E_MAX + 6)
    diag, east, north = (v.astype(np.float64) * Q_UNIT for v in (di, ei, ni))
    for m in sorted({0, M - 1, int(rng.integers(M))}):
        for r, c in sample_entries(g, rng, 8):
            d, e, _, _, s = stencil_entry_frac(g, a[m], r, c)
            assert Fraction(float(diag[m, r, c])) == d
            assert c + 1 >= g.nc or Fraction(float(east[m, r, c])) == e
            assert r + 1 >= g.nr or Fraction(float(north[m, r, c])) == s
    return a, diag, east, north


def exact_stencil_case(blocks, N, K, seed, unit=False):
    """(a (nrb, ncb), X (K, dim), Y (K, dim)) with Y = A(a) X EXACTLY: integer X, |x| <= 2^XB, a = m 2^e (all ones when
    `unit`).  Asserts the representability bound on the numbers produced and re-derives a sample of entries in Fractions."""
    g = ro.Geometry(blocks, N)
    rng = np.random.default_rng(seed)
    if unit:
        a = np.ones((g.nrb, g.ncb))
        ai = np.full((g.nrb, g.ncb), 1 << (E_MAX + 1), dtype=np.int64)
    else:
        a, ai = exact_coefficients(rng, (g.nrb, g.ncb))
    di, ei, ni = _stencil_int(g, ai)
    Xi = rng.integers(-(1 << XB), (1 << XB) + 1, size=(K, g.nr, g.nc)).astype(np.int64)
    Yi = di[None] * Xi
    Ab = np.abs(di)[None] * np.abs(Xi)                       # sum_j |A_ij| |x_j|: bounds every partial sum in any order
    Yi[:, :, :-1] += ei[None] * Xi[:, :, 1:]
    Yi[:, :, 1:] += ei[None] * Xi[:, :, :-1]
    Yi[:, :-1, :] += ni[None] * Xi[:, 1:, :]
    Yi[:, 1:, :] += ni[None] * Xi[:, :-1, :]
    Ab[:, :, :-1] += np.abs(ei)[None] * np.abs(Xi[:, :, 1:])
    Ab[:, :, 1:] += np.abs(ei)[None] * np.abs(Xi[:, :, :-1])
    Ab[:, :-1, :] += np.abs(ni)[None] * np.abs(Xi[:, 1:, :])
    Ab[:, 1:, :] += np.abs(ni)[None] * np.abs(Xi[:, :-1, :])
    assert (2 * E_MAX + 7 + XB) <= 53 and int(Ab.max()) < 2 ** 53, "a partial sum could leave the 53-bit range"
    X, Y = Xi.astype(np.float64), Yi.astype(np.float64) * Q_UNIT
    assert np.array_equal(Y / Q_UNIT, Yi.astype(np.float64))
    for k in sorted({0, K - 1}):
        for r, c in sample_entries(g, rng):
            assert Fraction(float(Y[k, r, c])) == apply_entry_frac(g, a, X[k], r, c), (k, r, c)
    return a, X.reshape(K, g.dim), Y.reshape(K, g.dim)


def energy_int(g, Xi):
    """x^T A_1 x of integer rows Xi (K, dim) as Python ints: the edge form, boundary values 0."""
    X = np.asarray(Xi, dtype=np.int64).reshape(-1, g.nr, g.nc)
    assert int(np.abs(X).max(initial=0)) <= 1 << (XB + 1)
    P = np.zeros((X.shape[0], g.nr + 2, g.nc + 2), dtype=np.int64)
    P[:, 1:-1, 1:-1] = X
    s = ((P[:, :, 1:] - P[:, :, :-1]) ** 2).sum(axis=(1, 2)) + ((P[:, 1:, :] - P[:, :-1, :]) ** 2).sum(axis=(1, 2))
    return [int(v) for v in s]


def exact_norm_case(blocks, N, K, seed, diff=False):
    """Integer rows (U, V or None, S) with S[k] = (u_k - v_k)^T A_1 (u_k - v_k) an exact Python int below 2^53 (asserted; every
    partial sum of the edge form is a sum of non-negative integers below it) -- and so is sum_i |d_i| |(A_1 d)_i|, which
    bounds the partial sums of the oracle's d . (A_1 d).  The norm is math.sqrt(S[k]), correctly rounded."""
    g = ro.Geometry(blocks, N)
    rng = np.random.default_rng(seed)
    hi = 1 << (XB - 1 if diff else XB)
    Ui = rng.integers(-hi, hi + 1, size=(K, g.dim)).astype(np.int64)
    Vi = rng.integers(-hi, hi + 1, size=(K, g.dim)).astype(np.int64) if diff else None
    Di = Ui - Vi if diff else Ui
    S = energy_int(g, Di)
    assert max(S) < 2 ** 53
    assert 8 * g.dim * (1 << XB) ** 2 < 2 ** 53      # sum |d_i| |(A_1 d)_i| <= dim 2^XB (8 2^XB)
    # one row again, edge by edge, in Python ints
    d = Di[0].reshape(g.nr, g.nc).tolist()
    at = lambda r, c: d[r][c] if 0 <= r < g.nr and 0 <= c < g.nc else 0
    tot = sum((at(r, c) - at(r, c + 1)) ** 2 for r in range(g.nr) for c in range(-1, g.nc)) \
        + sum((at(r, c) - at(r + 1, c)) ** 2 for r in range(-1, g.nr) for c in range(g.nc))
    assert tot == S[0]
    return Ui.astype(np.float64), (Vi.astype(np.float64) if diff else None), S


def sqrt_ulps_ok(got, S, ulps=1):
    """|got - sqrt(S)| <= `ulps` ulp for the exact integer S, decided in rational arithmetic (math.isqrt brackets it first)."""
    got = float(got)
    if S == 0:
        return got == 0.0
    if not (math.isqrt(S) - 1 <= got <= math.isqrt(S) + 2):
        return False
    u = Fraction(math.ulp(got)) * ulps
    lo, hi = Fraction(got) - u, Fraction(got) + u
    return (lo <= 0 or lo * lo <= S) and S <= hi * hi


def eval_point_frac(g, u, ix, iy, tx, ty):
    """P1 value at local coordinates (tx, ty) of cell (ix, iy) of the vertex grid with its Dirichlet ring, as a Fraction
    (the reference's evaluate_solutions; both triangles give the same value on tx + ty = 1)."""
    V = lambda y, x: Fraction(float(u[(y - 1) * g.nc + (x - 1)])) if 1 <= y <= g.nr and 1 <= x <= g.nc else Fraction(0)
    tx, ty = Fraction(float(tx)), Fraction(float(ty))
    lower = (1 - tx - ty) * V(iy, ix) + tx * V(iy, ix + 1) + ty * V(iy + 1, ix)
    upper = (tx + ty - 1) * V(iy + 1, ix + 1) + (1 - tx) * V(iy + 1, ix) + (1 - ty) * V(iy, ix + 1)
    if tx + ty == 1:
        assert lower == upper
    return lower if tx + ty < 1 else upper


# ---- 80-bit truths ----------------------------------------------------------------------------------------------------
def apply_ld(g, a, X):
    """(A(a) X, |A(a)| |X|) in long double from the oracle's fp64 stencil arrays: the product in the referee's edge form
    (differences first), the entrywise bound term by term."""
    we, wn, wb = rf.edge_weights(g, a)
    d, e, n = (np.abs(v).astype(LD) for v in ro.stencil_arrays(g, a))
    X3 = np.asarray(X, dtype=np.float64).reshape(-1, g.nr, g.nc).astype(LD)
    Y = np.stack([-rf.residual_ld(g, we, wn, wb, np.zeros(g.dim), x.ravel()).reshape(g.nr, g.nc) for x in X3])
    A3 = np.abs(X3)
    B = d[None] * A3
    B[:, :, :-1] += e[None] * A3[:, :, 1:]
    B[:, :, 1:] += e[None] * A3[:, :, :-1]
    B[:, :-1, :] += n[None] * A3[:, 1:, :]
    B[:, 1:, :] += n[None] * A3[:, :-1, :]
    return Y.reshape(-1, g.dim), B.reshape(-1, g.dim)


def rel_h10_ld(g, X, T):
    """max over rows of ||X_m - T_m||_{H10} / ||T_m||_{H10} in long double (fp64 or long-double inputs)."""
    X, T = np.atleast_2d(np.asarray(X)).astype(LD), np.atleast_2d(np.asarray(T)).astype(LD)
    return float(max(rf.h10_ld(g, x - t) / rf.h10_ld(g, t) for x, t in zip(X, T)))


class SpanTruth:
    """A_1-orthonormal long-double basis Q of the exact span of the fp64 rows C (nested in the row order) with its block
    energy forms: everything project_truth_ld / galerkin_truth_ld need, computed once and shared by every prefix C[:n]."""

    def __init__(self, g, C):
        self.g = g
        self.Q, self.keep = rf.a1_orthonormal_span_ld(g, C)
        self._forms = None

    def forms(self):
        if self._forms is None:
            self._forms = rf._energy_forms_ld(self.g, self.Q)
        return self._forms


def project_truth_ld(g, U, C, n=None, span=None):
    """H^1_0-orthogonal projection of the rows U onto span C[:n]: P u = Q^T (Q A_1 u) in long double, rounded once to fp64.
    Returns (P (M, dim) fp64, keep (n,))."""
    span = span or SpanTruth(g, C)
    n = len(span.Q) if n is None else n
    Q = span.Q[:n]
    P = rf._a1_dots_ld(g, np.atleast_2d(np.asarray(U, dtype=np.float64)).astype(LD), Q)
    return np.asarray(P @ Q, dtype=np.float64), span.keep[:n].copy()


def galerkin_truth_ld(g, a, C, n=None, span=None):
    """Galerkin ROM u_n(a) = c^T Q with (sum_b a_b S_b) c = Q B (the construction of referee.galerkin_truth_nested, the
    vectors instead of the error).  Returns (u (M, dim) fp64, keep (n,))."""
    span = span or SpanTruth(g, C)
    n = len(span.Q) if n is None else n
    a = np.asarray(a, dtype=np.float64).reshape(len(a), -1).astype(LD)
    idx = np.flatnonzero(span.keep[:n])
    Q = span.Q[idx]
    forms = span.forms()
    A = sum(a[:, b][:, None, None] * forms[b][np.ix_(idx, idx)][None] for b in range(a.shape[1]))
    c = rf._chol_solve_batched_ld(A, Q @ ro.load_vector(g).astype(LD))
    return np.asarray(c @ Q, dtype=np.float64), span.keep[:n].copy()


def spd_truth_ld(Ahat, w, rhs, c_hat=None):
    """Long-double solutions c (M, n) of (sum_b w[m, b] Ahat[b]) c_m = rhs (n,) or rhs[m]; with an fp64 candidate c_hat (M, n)
    also its normwise backward errors ||rhs - A c_hat||_2 / (||A||_F ||c_hat||_2 + ||rhs||_2) (M,), in long double."""
    Ahat, w = np.asarray(Ahat, dtype=np.float64).astype(LD), np.atleast_2d(np.asarray(w, dtype=np.float64)).astype(LD)
    M, n = w.shape[0], Ahat.shape[-1]
    A = (w[:, :, None, None] * Ahat[None]).sum(axis=1)
    b = np.broadcast_to(np.asarray(rhs, dtype=np.float64).astype(LD), (M, n))
    c = rf._chol_solve_batched_ld(A, b)
    if c_hat is None:
        return c, None
    ch = np.asarray(c_hat, dtype=np.float64).astype(LD).reshape(M, n)
    r = b - (A * ch[:, None, :]).sum(axis=2)
    nrm = lambda v, ax: np.sqrt((v * v).sum(axis=ax))
    return c, np.asarray(nrm(r, 1) / (nrm(A, (1, 2)) * nrm(ch, 1) + nrm(b, 1)), dtype=np.float64)


def rel2_ld(x, t):
    """max over systems of ||x_m - t_m||_2 / ||t_m||_2, long double."""
    x, t = np.asarray(x).astype(LD), np.asarray(t).astype(LD)
    return float(np.max(np.sqrt(((x - t) ** 2).sum(axis=-1)) / np.sqrt((t * t).sum(axis=-1))))


# ---- the reduced-solve cases ---------------------------------------------------------------------------------------------
REDUCED_LDS_DEFAULT, REDUCED_LDS_MAX = 64 * 1024, 160 * 1024


def reduced_route(n, M=1):
    """rom_launch_reduced_solve's decision (rom_ops.hip), restated: where the n x (n + 1) matrix lives and how many systems
    go per launch."""
    mat, vecs = n * (n + 1) * 8, 2 * n * 8
    in_lds = mat + vecs <= REDUCED_LDS_MAX
    route = "lds64" if mat + vecs <= REDUCED_LDS_DEFAULT else "lds160" if in_lds else "global"
    per_launch = M if in_lds else max(1, min(M, (1 << 30) // mat))
    return dict(route=route, per_launch=per_launch, launches=-(-M // per_launch))


def reduced_case(family, n, kb, M, per_system, seed=0):
    """(Ahat (kb, n, n), w (M, kb), rhs): `well` -- F F^T / (n + 3) + 0.05 I, w in [0.5, 3]; `graded` -- D F F^T D / (n + 3) with
    D = diag(10^(-3 i / n)) and w spread over six decades (condition 1e8 ... 1e12, a reduced Galerkin matrix in a
    raw-snapshot basis at contrast 1e6)."""
    rng = np.random.default_rng([seed, n, kb, int(per_system), family == "graded"])
    F = rng.standard_normal((kb, n, n + 3))
    Ahat = np.einsum("bik,bjk->bij", F, F) / (n + 3)
    if family == "well":
        Ahat += 0.05 * np.eye(n)
        w = rng.uniform(0.5, 3.0, size=(M, kb))
    else:
        D = 10.0 ** (-3.0 * np.arange(n) / n)
        Ahat = Ahat * D[None, :, None] * D[None, None, :]
        Ahat = 0.5 * (Ahat + Ahat.transpose(0, 2, 1))
        w = 10.0 ** rng.uniform(0, 6, size=(M, kb))
    rhs = rng.standard_normal((M, n) if per_system else n)
    return Ahat, w, rhs


def lapack_pos(Ahat, w, rhs):
    """scipy.linalg.solve(assume_a='pos') of every system, on the same fp64 inputs."""
    w = np.atleast_2d(w)
    return np.array([scipy.linalg.solve(np.einsum("b,bij->ij", w[m], Ahat), rhs[m] if np.ndim(rhs) == 2 else rhs, assume_a="pos")
                     for m in range(len(w))])


# ---- the projector cases -----------------------------------------------------------------------------------------------------
PROJ_GEOMS = [((2, 2), 8), ((2, 3), 11)]
QR_SIZES = [1, 5, 89, 90, 141, 142]
RAW_SIZES = [4, 8]
_proj_cache = {}


def projector_inputs(gm, d):
    """Inputs of the projector cases on geometry gm with parameters 10^U(0, d): dict with g, a (7 parameters), U (their
    oracle snapshots), Cqr (142 QR-orthonormal random rows: every prefix is a QR basis), Craw (8 raw snapshots of other
    parameters of the same law: the shape of a greedy basis).  Cached."""
    key = (gm, d)
    if key not in _proj_cache:
        blocks, N = gm
        g = ro.Geometry(blocks, N)
        rng = np.random.default_rng([d, N, blocks[0], blocks[1]])
        a = 10.0 ** rng.uniform(0, d, size=(7,) + blocks)
        at = 10.0 ** rng.uniform(0, d, size=(max(RAW_SIZES),) + blocks)
        Cqr = np.linalg.qr(np.random.default_rng([N, 99]).standard_normal((max(QR_SIZES), g.dim)).T)[0].T.copy()
        _proj_cache[key] = dict(g=g, a=a, U=ro.generate_solutions(g, a), Cqr=Cqr, Craw=ro.generate_solutions(g, at))
    return _proj_cache[key]


_span_cache = {}


def projector_span(gm, d, kind):
    """SpanTruth of the QR rows (kind 'qr': independent of d) or the raw snapshots (kind 'raw') of projector_inputs. Cached."""
    key = (gm, None if kind == "qr" else d, kind)
    if key not in _span_cache:
        inp = projector_inputs(gm, d)
        _span_cache[key] = SpanTruth(inp["g"], inp["Cqr" if kind == "qr" else "Craw"])
    return _span_cache[key]


# ---- rows to orthonormalise --------------------------------------------------------------------------------------------------
def ortho_rows(n, dim, seed, graded):
    """n rows of dimension dim whose row-equilibrated block is well conditioned (Gaussian rows plus 4 sqrt(dim) on a
    diagonal: singular values within [2, 6] sqrt(dim), so that row j of ANY QR is determined to a small multiple of u and
    a comparison of two QRs at the n 2^-53 level means something); rows past dim are combinations of the earlier ones.
    graded: row i scaled by 10^(-12 i / (n - 1))."""
    rng = np.random.default_rng([seed, n, dim])
    k = min(n, dim)
    X = rng.standard_normal((k, dim))
    X[np.arange(k), np.arange(k)] += 4 * np.sqrt(dim)
    if n > k:
        X = np.vstack((X, rng.standard_normal((n - k, k)) @ X))
    if graded and n > 1:
        X = X * (10.0 ** (-12.0 * np.arange(n) / (n - 1)))[:, None]
    return X
