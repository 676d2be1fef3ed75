"""Generators and checkers for the launch-split tests (tests/test_launch_limits_host.py, tests/test_gpu_launch_limits.py).
TEST INFRASTRUCTURE: nothing in the product path may import this.

The cases of those files are large in the COUNT of items, not in the data: item i of a block is

    row(i) = 2^e(i) * base[i mod PERIOD],   e(i) = (i mod EXP_PERIOD) - 6,   PERIOD = 67, EXP_PERIOD = 13,

so a block repeats after 67 * 13 = 871 items.  Scaling by a power of two commutes exactly with every linear kernel of the
library (no entry here comes near the ends of the exponent range), so the long-double truth of row(i) is the scaled truth of
its base row -- bit for bit -- and costs 67 rows.  65535 = 9 and 65536 = 10 (mod 67): row(i) differs from row(i - 65535) and
from row(i - 65536), the rows a second launch would read with a lost base pointer, and from row(i - 1).  The host test
asserts these properties of the generators on the blocks the GPU tests use.

A truth is kept as an unevaluated sum hi + lo of two fp64 arrays (hi = the long-double truth rounded, lo = the remainder
rounded): (got - hi) - lo in fp64 is the error to ~2^-100 relative, so the large blocks are compared in fp64 and long double
is spent on the base rows only.
"""
import numpy as np

import h10_truth as ht
import nearest_truth as nt
import referee as rf

LD = np.longdouble
EPS = 2.0 ** -53
LIMIT = 65535                  # the largest grid.y / grid.z: the count one launch takes
RIGHT_ROWS = LIMIT * 64        # rows per launch of the right factor of the sine transform (SP_MAX_ROWS of rom_spectral.hip)
PERIOD, EXP_PERIOD = 67, 13
CYCLE = PERIOD * EXP_PERIOD
GEOM = ((1, 1), 4)             # the smallest geometry h10_truth.grid and the library both take: 3 x 3 inner vertices
CHUNK = CYCLE * 64


K_BATCH = LIMIT + 2             # snapshots: one past the first item of a second launch of k_sine_left (and of every y split)
TRANSFORM_SEED = 4


def right_count(nr):
    """Snapshots whose K nr rows are just above RIGHT_ROWS: the second launch of the right factor holds about 70 of them."""
    return -(-RIGHT_ROWS // nr) + 70


def exponents(idx):
    return (np.asarray(idx) % EXP_PERIOD - 6).astype(np.int32)


def pow2(idx):
    return np.ldexp(1.0, exponents(idx))


def named_rows(K):
    """The rows every message names: 0, both sides of the first split, the last."""
    return sorted({i for i in (0, LIMIT - 1, LIMIT, LIMIT + 1, K - 1) if 0 <= i < K})


def base_rows(dim, seed, cols_scale=True):
    """PERIOD base rows: O(1) entries with a spread of magnitudes over the rows (as h10_truth.transform_rows)."""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((PERIOD, dim))
    return X * 10.0 ** rng.uniform(-3, 3, size=(PERIOD, 1)) if cols_scale else X


def rows(base, K, lo=0, scaled=True):
    """Items lo .. K-1 of the block built from `base` (PERIOD, dim): scaled-periodic, or plainly periodic."""
    idx = np.arange(lo, K)
    X = np.asarray(base, dtype=np.float64)[idx % PERIOD]
    return np.ldexp(X, exponents(idx)[:, None]) if scaled else X.copy()


def split_ld(T):
    """Long-double array -> (hi, lo) fp64 with hi + lo = T to 2^-106."""
    T = np.asarray(T, dtype=LD)
    hi = np.asarray(T, dtype=np.float64)
    return hi, np.asarray(T - hi.astype(LD), dtype=np.float64)


def tile_hi(hi, K, lo=0, scaled=True):
    """The fp64 block whose item i is 2^e(i) hi[i mod PERIOD] (the tiled truth, or a tiled expected output)."""
    return rows(hi, K, lo, scaled)


def flat_shift_differs(base, K, width, split_rows):
    """With the block of K items seen as rows of `width` doubles: does every row q >= split_rows differ from row
    q - split_rows (what a launch that lost its offset would read)?  Only the two ends of the block are built."""
    dim = np.asarray(base).shape[1]
    total = K * dim // width
    assert K * dim % width == 0 and 0 < split_rows < total
    n2 = total - split_rows                                   # rows of the second launch
    it0 = split_rows * width // dim                           # first item the second launch touches
    tail = rows(base, K, lo=it0).reshape(-1)[split_rows * width - it0 * dim:].reshape(n2, width)
    head = rows(base, -(-n2 * width // dim)).reshape(-1)[:n2 * width].reshape(n2, width)
    return not np.any(np.all(tail == head, axis=1))


def _describe(ratio):
    K = len(ratio)
    bad = np.flatnonzero(~(ratio <= 1.0))
    txt = "rows " + ", ".join(f"{i}: {ratio[i]:.3g}" for i in named_rows(K))
    if len(bad):
        txt += f"; {len(bad)} rows over the bound, first {bad[:4].tolist()}, last {int(bad[-1])}"
    return txt


def check_ratios(name, ratio, observed):
    """Every entry of `ratio` (one per row; NaN counts as a failure) <= 1, the named rows in the message."""
    ratio = np.asarray(ratio, dtype=np.float64)
    observed(name, np.where(np.isnan(ratio), np.inf, ratio), 1.0, detail=_describe(ratio))


def check_exact(name, got, want):
    """Every row of got equals the row of want bit for bit."""
    got, want = np.ascontiguousarray(got, dtype=np.float64), np.ascontiguousarray(want, dtype=np.float64)
    assert got.shape == want.shape, (name, got.shape, want.shape)
    g2, w2 = got.reshape(len(got), -1).view(np.uint64), want.reshape(len(want), -1).view(np.uint64)
    bad = np.flatnonzero((g2 != w2).any(axis=1))
    named = {i: bool((g2[i] == w2[i]).all()) for i in named_rows(len(got))}
    assert len(bad) == 0, f"{name}: {len(bad)} rows differ, first {bad[:4].tolist()}, last {int(bad[-1])}; rows equal: {named}"


# ---- the sine transform ------------------------------------------------------------------------------------------------
class TransformTruth:
    """Long-double T_{pre,post} of the base rows on grid `gr`, and h10_truth.Grid.transform_bound of them (C = 64)."""

    def __init__(self, gr, base, pre, post):
        self.gr, self.base, self.pre, self.post = gr, np.asarray(base, dtype=np.float64), pre, post
        self.hi, self.lo = split_ld(gr.transform(base, pre, post))
        self.bound = gr.transform_bound(base, pre, post)
        assert np.all(self.bound > 0)

    def fp64_output(self, K, lo=0):
        """A correct output for the mutation tests: the plain fp64 restatement of the base rows, scaled (exact)."""
        return tile_hi(np.asarray(self.gr.transform(self.base, self.pre, self.post, ld=False), dtype=np.float64), K, lo)

    def ratios(self, got, lo=0):
        """||got_i - truth_i||_2 / bound_i for the items lo .. lo + len(got) - 1."""
        got = np.asarray(got, dtype=np.float64)
        out = np.empty(len(got))
        for c0 in range(0, len(got), CHUNK):
            idx = np.arange(lo + c0, lo + min(len(got), c0 + CHUNK))
            b, s = idx % PERIOD, pow2(idx)[:, None]
            err = (got[c0:c0 + len(idx)] - self.hi[b] * s) - self.lo[b] * s
            out[c0:c0 + len(idx)] = np.sqrt(np.sum(err * err, axis=1)) / (self.bound[b] * s[:, 0])
        return out


def check_transform(name, tt, got, observed):
    check_ratios(f"{name} (pre, post) = ({tt.pre}, {tt.post}) K={len(got)}: row error / (C eps (nr + nc) |L^(pre/2) o X| max L^(post/2))",
                 tt.ratios(got), observed)


# ---- rom_rows_scale, rom_rows_sign_flip ------------------------------------------------------------------------------------
def scale_case(rows_n, dim):
    """(X (rows, dim), factors (rows,), expected): X and the factors scaled-periodic; expected = the fp64 product, ONE rounding of
    the exact one (the host test holds it against long double)."""
    X = rows(base_rows(dim, seed=dim), rows_n)
    fac = rows(base_rows(1, seed=100 + dim, cols_scale=False) * 3.0, rows_n)[:, 0]
    return X, fac, X * fac[:, None]


def sign_base(dim, seed):
    """Base rows for the sign rule: uniform entries; row 0 / 1 a tie of opposite signs between the first and the last column
    (the first wins), row 2 all zeros (no flip, no NaN), row 3 a negative maximum in the last column."""
    B = np.random.default_rng(seed).uniform(-1, 1, size=(PERIOD, dim))
    B[0, 0], B[0, dim - 1] = -9.0, 9.0
    B[1, 0], B[1, dim - 1] = 9.0, -9.0
    B[2] = 0.0
    B[3, dim - 1] = -9.0
    return B


def svd_flip(X):
    """NumPy's rule of sklearn's svd_flip(u_based_decision=False): every row times the sign of its entry of largest
    magnitude, the first one on ties."""
    piv = np.argmax(np.abs(X), axis=1)
    sg = np.where(X[np.arange(len(X)), piv] < 0, -1.0, 1.0)
    return X * sg[:, None]


def sign_case(rows_n, dim):
    X = rows(sign_base(dim, seed=7 * dim), rows_n)
    return X, svd_flip(X)


# ---- rom_nearest -------------------------------------------------------------------------------------------------------------
NN_SPLIT = LIMIT * 16          # queries of one launch of the exhaustive kernel (16 per workgroup, workgroups in grid.y)
NN_K = NN_SPLIT + 17


def nearest_case(r, seed=0):
    """(library Q (40, r), query base (PERIOD, r)): the K queries are rows(base, K)."""
    rng = np.random.default_rng([seed, r])
    return rng.uniform(-2, 2, size=(40, r)), rng.standard_normal((PERIOD, r))


def nearest_windows(K):
    """Windows of one cycle of queries that go through check_neighbours: the first, the one across the split, the last."""
    w = [(0, min(K, CYCLE))]
    if K > NN_SPLIT:
        w.append((max(0, NN_SPLIT - CYCLE // 2), min(K, NN_SPLIT + CYCLE // 2)))
    w.append((max(0, K - CYCLE), K))
    return w


def check_nearest(name, base, Q, idx, dist2, t):
    """nearest_truth.check_neighbours on the windows, and every row against the first cycle: a query with the same data has
    the same neighbours and the same bits of its distances."""
    K = len(idx)
    for lo, hi in nearest_windows(K):
        try:
            nt.check_neighbours(rows(base, hi, lo), Q, idx[lo:hi], dist2[lo:hi], t)
        except AssertionError as e:
            raise AssertionError(f"{name}: queries {lo} .. {hi - 1}: {e}") from None
    cyc = np.arange(K) % CYCLE
    check_exact(f"{name}: indices against the first cycle", idx.astype(np.float64), idx[:CYCLE][cyc].astype(np.float64))
    check_exact(f"{name}: distances against the first cycle", dist2, dist2[:CYCLE][cyc])


# ---- rom_error_curves ----------------------------------------------------------------------------------------------------------
C_CURVES = 64.0
EPS_CURVES = np.finfo(np.float64).eps


def _kappa(g, C, keep):
    """tests/test_gpu_error_curves.py::_kappa: the condition number of the row-normalised kept rows among the leading n."""
    G = np.asarray(rf._a1_dots_ld(g, C.astype(LD), C.astype(LD)), dtype=np.float64)
    idx = np.flatnonzero(keep)
    d = np.sqrt(np.diag(G))
    G = G / d[:, None] / d[None, :]
    out = [1.0]
    for n in range(1, len(C) + 1):
        k = idx[idx < n]
        w = np.linalg.eigvalsh(G[np.ix_(k, k)]) if len(k) else np.ones(1)
        out.append(np.sqrt(w[-1] / w[0]) if w[0] > 0 else np.inf)
    return np.array(out)


class CurvesTruth:
    """The 80-bit truth and the bounds of tests/test_gpu_error_curves.py::test_curves_against_80bit_truth on the PERIOD
    distinct snapshots U with parameters a (or None: projection only) and the basis rows C; `dead`: the rows the call
    dropped."""

    def __init__(self, g, U, C, a, contrast, dead=None):
        n = len(C)
        dead = np.zeros(n, dtype=bool) if dead is None else np.asarray(dead, dtype=bool)
        Ck = np.array(C, dtype=np.float64)
        Ck[dead] = 0.0
        Q, keep = rf.a1_orthonormal_span_ld(g, Ck)
        assert np.array_equal(keep, ~dead)
        UL = np.asarray(U, dtype=np.float64).astype(LD)
        u2 = np.array([rf.h10_ld(g, u) ** 2 for u in UL])
        PL = np.asarray(rf._a1_dots_ld(g, UL, Q))
        self.unorm = np.sqrt(np.asarray(u2, dtype=np.float64))
        self.kap = _kappa(g, np.asarray(C, dtype=np.float64), ~dead)
        self.n = n
        self.proj2 = np.array([np.maximum(u2 - np.sum(PL[:, :j] ** 2, axis=1), 0) for j in range(n + 1)], dtype=np.float64)
        steps = (np.arange(n + 1) + 1)[:, None]
        self.bound_p = C_CURVES * steps * EPS_CURVES * (1 + self.kap[:, None]) * self.unorm[None, :] ** 2
        self.P = np.asarray(PL, dtype=np.float64)
        self.gal2 = self.bound_g = None
        if a is not None:
            sizes = list(range(1, n + 1))
            tg = rf.galerkin_truth_nested(g, a, Ck, U, sizes)
            self.gal2 = (np.vstack([np.ones(len(U))] + [tg[j] for j in sizes]) * self.unorm[None, :]) ** 2
            self.bound_g = self.bound_p + C_CURVES * contrast * EPS_CURVES * steps * self.unorm[None, :] ** 2


CURVES_M = LIMIT + 2
CURVES_DECADES = 2      # parameters 10^U(0, 2): contrast 1e2 in the bound, as the ordinary cases of test_gpu_error_curves.py


def curves_inputs(blocks, dim, N):
    """(a (PERIOD,) + blocks, C (N, dim)): the parameters of the distinct snapshots and random basis rows."""
    rng = np.random.default_rng([N, dim])
    return 10.0 ** rng.uniform(0, CURVES_DECADES, size=(PERIOD,) + tuple(blocks)), rng.standard_normal((N, dim))


def check_curves(name, tr, proj, galc, P, observed):
    """Every column m of the curves against the truth of snapshot m mod PERIOD; identical snapshots give identical bits."""
    M = proj.shape[1]
    b = np.arange(M) % PERIOD
    assert proj.shape == (tr.n + 1, M)
    check_ratios(f"{name}: squared projection error vs 80-bit truth / (C (n+1) eps (1 + kappa) |u|^2)",
                 np.max(np.abs(proj ** 2 - tr.proj2[:, b]) / tr.bound_p[:, b], axis=0), observed)
    if tr.gal2 is not None:
        assert galc is not None and galc.shape == proj.shape
        check_ratios(f"{name}: squared Galerkin error vs 80-bit truth / (C (n+1) eps ((1 + kappa) + contrast) |u|^2)",
                     np.max(np.abs(galc ** 2 - tr.gal2[:, b]) / tr.bound_g[:, b], axis=0), observed)
        check_exact(f"{name}: Galerkin curves of identical snapshots", galc.T, galc.T[:PERIOD][b])
    else:
        assert galc is None
    check_exact(f"{name}: projection curves of identical snapshots", proj.T, proj.T[:PERIOD][b])
    if P is not None and tr.n:
        assert P.shape == (M, tr.n)
        rel = np.max(np.abs(np.abs(P) - np.abs(tr.P[b])), axis=1) / tr.unorm.max()
        check_ratios(f"{name}: |P| vs 80-bit |<u, q>_A| / (C n eps (1 + kappa) max |u|)",
                     rel / (C_CURVES * tr.n * EPS_CURVES * (1 + tr.kap[-1])), observed)
        check_exact(f"{name}: coefficients of identical snapshots", P, P[:PERIOD][b])


# ---- the strong greedy ----------------------------------------------------------------------------------------------------------
C_GREEDY = 16.0   # the bound model of tests/test_gpu_greedy_routes.py


GREEDY_N = 3


def greedy_inputs(dim, seed):
    """(U (PERIOD, dim) random rows, h1 (PERIOD,) normalisations in [0.5, 2]: no two relative errors tie)."""
    rng = np.random.default_rng(seed)
    return rng.standard_normal((PERIOD, dim)) * rng.uniform(0.5, 2.0, size=(PERIOD, 1)), rng.uniform(0.5, 2.0, size=PERIOD)


def greedy_truth(g, U, h1, n, map_delta=0.0):
    """The H^1_0 strong greedy of the PERIOD distinct rows in 80-bit arithmetic (referee.greedy_ld, one pick at a time):
    (picks, max errors, margins between the best and the second-best error, the bounds per iteration in the model of
    tests/test_gpu_greedy_routes.py: delta_i = C (i + 1) eps E0^2 + map_delta on the squared errors)."""
    a = np.ones((len(U), g.nrb * g.ncb))
    picks = []
    for i in range(n):
        E, _ = rf.greedy_ld(g, U, a, h1, picks + [0], False)
        picks.append(int(np.argmax(np.asarray(E[i], dtype=np.float64))))
    E, _ = rf.greedy_ld(g, U, a, h1, picks, False)
    E = np.asarray(E, dtype=np.float64)
    top = E.max(axis=1)
    margin = np.array([np.sort(e)[-1] - np.sort(e)[-2] for e in E])
    bounds = np.zeros(n)
    for i in range(n):
        delta = C_GREEDY * (i + 1) * EPS * E[0].max() ** 2 + map_delta
        bounds[i] = min(np.sqrt(delta), delta / top[i]) if top[i] > 0 else np.sqrt(delta)
    return picks, top, margin, bounds


def check_greedy(name, truth, picks, errs, observed):
    """The picks of a call on the periodic block are the 80-bit picks -- each the lowest index among its equal rows -- and the
    curve is within the bound."""
    t_picks, top, margin, bounds = truth
    assert np.all(margin > 4 * bounds), (name, "the 80-bit margins do not decide the picks", margin, bounds)
    assert list(picks) == list(t_picks), (name, list(picks), list(t_picks))
    observed(f"{name}: |curve - 80-bit| / bound", np.abs(np.asarray(errs) - top) / bounds, 1.0)


# ---- planted mutations -----------------------------------------------------------------------------------------------------------
def lost_offset(out, split, shift=None, last_only=False):
    """`out` (items along axis 0, correct) with every item i >= split replaced by the correct item i - shift: what a second
    launch computes when it reads the first launch's input (shift = split, the default) or is one item off (shift = 1).
    last_only: only the last item is wrong."""
    shift = split if shift is None else shift
    bad = np.array(out, copy=True)
    K = len(bad)
    assert 0 < shift <= split < K
    if last_only:
        bad[K - 1] = out[K - 1 - shift]
    else:
        bad[split:] = out[split - shift:K - shift]
    return bad
