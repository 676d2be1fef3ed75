"""Long-double truth for the H^1_0-POD tests (tests/test_pod_h10_host.py, tests/test_gpu_pod_h10.py).  TEST INFRASTRUCTURE:
nothing in the product path may import this.

A_1 (the 5-point stencil of the interior grid, diagonal 4, neighbours -1) = S Lambda S with S = S_r (x) S_c the symmetric,
orthogonal sine matrices and Lambda[j, k] = lam_r[j] + lam_c[k] (csrc/rom_riesz.hip).  `Grid` holds the tables in 80-bit long
double (argument reduction in integers, as the device builds them) and the transform
    T_{pre,post}(X) = Lambda^(post/2) o (S_r (Lambda^(pre/2) o X) S_c)
in long double or -- `ld=False` -- as the plain fp64 NumPy restatement the bounds are checked against on the CPU.
`H10Truth` crafts an (M, dim) block with an exactly known H^1_0 SVD: W = referee.ExactSVD (exact Euclidean SVD), U_i =
T_{-1,0}(W_i) in long double rounded to fp64, true modes T_{-1,0}(v_k).  Rounding U to fp64 moves W by at most
eps sqrt(lam_max) ||U_i|| <= eps kappa ||W_i||: the kappa of every bound below.
"""
import numpy as np

from oracle import rom_oracle as ro
import referee as rf

LD = np.longdouble
EPS = 2.0 ** -53
C = 64.0
PI = 4 * np.arctan(LD(1))

# (blocks, N) -> nr x nc = (nrb N - 1) x (ncb N - 1): smaller than one MFMA tile; nr != nc; a square one; across a 64-row tile
GRIDS = [((1, 1), 8), ((2, 3), 8), ((2, 2), 16), ((3, 2), 24)]
# the (pre, post) pairs the POD uses, and the two of A_1^-1 on dense rows
PAIRS = [(0, 1), (-1, 0), (0, -2), (0, 0)]


def sine_table_ld(n):
    """S_n[j, p] = sqrt(2 / (n + 1)) sin(pi (j + 1)(p + 1) / (n + 1)) and lam_n[j] = 4 sin^2(pi (j + 1) / (2 (n + 1)))."""
    n1 = n + 1
    j = np.arange(1, n + 1, dtype=np.int64)
    t = (j[:, None] * j[None, :]) % (2 * n1)
    sgn = np.where(t > n1, -1, 1)
    t = np.where(t > n1, t - n1, t)
    t = np.where(2 * t > n1, n1 - t, t)
    S = sgn.astype(LD) * np.sqrt(LD(2) / LD(n1)) * np.sin(PI * t.astype(LD) / LD(n1))
    s = np.sin(PI * j.astype(LD) / LD(2 * n1))
    return S, 4 * s * s


def _pw(lam, e):
    return {2: lam, 1: np.sqrt(lam), 0: None, -1: 1 / np.sqrt(lam), -2: 1 / lam}[e]


class Grid:
    def __init__(self, blocks, N):
        self.blocks, self.N = tuple(blocks), N
        self.nr, self.nc = blocks[0] * N - 1, blocks[1] * N - 1
        self.dim = self.nr * self.nc
        self.Sr, lr = sine_table_ld(self.nr)
        self.Sc, lc = sine_table_ld(self.nc)
        self.lam = lr[:, None] + lc[None, :]
        self.kappa = float(np.sqrt(self.lam.max() / self.lam.min()))
        self.g = ro.Geometry(self.blocks, N)
        assert (self.g.nr, self.g.nc) == (self.nr, self.nc)

    def scale(self, X, e, ld=True):
        """Lambda^(e/2) o X, rows of X as nr x nc arrays."""
        T = LD if ld else np.float64
        X = np.asarray(X).astype(T).reshape(-1, self.nr, self.nc)
        f = _pw(self.lam.astype(T), e)
        return (X if f is None else X * f).reshape(-1, self.dim)

    def transform(self, X, pre=0, post=0, ld=True):
        T = LD if ld else np.float64
        X3 = self.scale(X, pre, ld).reshape(-1, self.nr, self.nc)
        Y = np.matmul(np.matmul(self.Sr.astype(T), X3), self.Sc.astype(T))
        return self.scale(Y, post, ld)

    def pw_max(self, e):
        f = _pw(self.lam, e)
        return 1.0 if f is None else float(f.max())

    def transform_bound(self, X, pre, post):
        """Per row: C eps (nr + nc) ||Lambda^(pre/2) o X_i||_2 max Lambda^(post/2)."""
        return C * EPS * (self.nr + self.nc) * np.linalg.norm(self.scale(X, pre).astype(np.float64), axis=1) * self.pw_max(post)

    def a1_dots(self, X, Y):
        """X A_1 Y^T through the long-double 5-point stencil (edge form: referee._a1_dots_ld), not the tables."""
        return rf._a1_dots_ld(self.g, np.asarray(X).astype(LD), np.asarray(Y).astype(LD))

    def energy(self, X):
        """Long-double coordinates in which the A_1 inner product is Euclidean, from the stencil's edges (not the tables)."""
        return rf._grad_ld(self.g, X)

    def a1_dense(self):
        """The dense 5-point matrix in fp64 (small grids only)."""
        idx = np.arange(self.dim).reshape(self.nr, self.nc)
        A = 4.0 * np.eye(self.dim)
        A[idx[:, :-1], idx[:, 1:]] = A[idx[:, 1:], idx[:, :-1]] = -1.0
        A[idx[:-1, :], idx[1:, :]] = A[idx[1:, :], idx[:-1, :]] = -1.0
        return A


_GRIDS = {}


def grid(blocks, N):
    key = (tuple(blocks), N)
    if key not in _GRIDS:
        _GRIDS[key] = Grid(*key)
    return _GRIDS[key]


def transform_rows(gr, K, seed):
    """K test rows for the transform: O(1) entries with a spread of magnitudes over the rows."""
    rng = np.random.default_rng(seed)
    return rng.standard_normal((K, gr.dim)) * 10.0 ** rng.uniform(-3, 3, size=(K, 1))


def round_trip_bound(gr, X, W):
    """(0,1) then (-1,0) returns X within the sum of the two bounds: bound(0,1)(X) + bound(-1,0)(W), W = the (0,1) output."""
    return gr.transform_bound(X, 0, 1) + gr.transform_bound(W, -1, 0)


RIESZ_FRACTIONS = np.array([[0.31, 0.47], [0.52, 0.77], [0.9, 0.12]])


def riesz_points(gr):
    """Three points (x, y) inside the domain, none on a grid line."""
    lo = np.array([gr.g.points_c[0], gr.g.points_r[0]])
    hi = np.array([gr.g.points_c[-1], gr.g.points_r[-1]])
    return lo + (hi - lo) * RIESZ_FRACTIONS


def evaluation_rows(gr, pts):
    """(m, dim): the P1 evaluation vectors of the points (rows of generate_riesz(points, "l2")), from the oracle."""
    return np.ascontiguousarray(ro.evaluate_solutions(gr.g, pts, np.eye(gr.dim)).T)


def riesz_bound(gr, R, Z):
    """A_1^-1 of the rows R by (0,-2) then (0,0), Z = the (0,-2) output: within bound(0,-2)(R) + bound(0,0)(Z) of the truth
    (S is orthogonal: the first error passes through the second transform unchanged in norm)."""
    return gr.transform_bound(R, 0, -2) + gr.transform_bound(Z, 0, 0)


def _mant(values, M):
    """Dyadic mantissas for relative values (1 = s_1): the largest exponent e with M sum(m) < 2^52 (exact partial sums)."""
    v = np.asarray(values, dtype=np.float64)
    e = int(np.floor(52 - np.log2(M * v.sum()))) - 1
    m = np.round(v * 2.0 ** e).astype(np.int64)
    assert m.min() >= 1
    return m, e


def geo(r, hi, lo):
    return 10.0 ** -np.linspace(hi, lo, r)


class H10Truth:
    """An (M, dim) fp64 block U on `gr` whose H^1_0 SVD is s (r,), V (r, dim, long double, A_1-orthonormal); t: the ExactSVD of
    its energy coordinates W (t.F1 t.F2 = the centred W, exactly)."""

    def __init__(self, gr, M, D, values, seed, mean=False):
        mant, e = _mant(values, M)
        mean_int = None
        if mean:
            mean_int = np.random.default_rng(M + gr.dim).integers(-2 ** 20, 2 ** 20, size=gr.dim)
            assert (int(mant.sum()) + 2 ** 20) * M < 2 ** 53
        self.gr, self.M = gr, M
        self.t = rf.ExactSVD(M, D, gr.dim, mant, e, seed=seed, mean_int=mean_int)
        self.s, self.r = self.t.s, self.t.r
        self.U = np.asarray(gr.transform(self.t.X, -1, 0), dtype=np.float64)
        self.V = gr.transform(self.t.V, -1, 0)


# The crafted POD cases of both files: id, grid, M, D, relative spectrum, n, centre / mean row, rel_floor, x_row0, v_row0
def _case(cid, blocks, N, M, D, values, n, center=False, mean=False, rel_floor=0.0, x_row0=0, v_row0=0):
    return dict(id=cid, blocks=blocks, N=N, M=M, D=D, values=np.asarray(values, dtype=np.float64), n=n, center=center,
                mean=mean, rel_floor=rel_floor, x_row0=x_row0, v_row0=v_row0)


POD_CASES = [
    _case("fast_15x23", (2, 3), 8, 256, 256, geo(20, 0, 6), 16, x_row0=2, v_row0=3),
    # (a dyadic spectrum with exact partial sums ends near 2^-42 s_1: the request goes past the floor through the rank, 14 < 16)
    _case("floor_15x23", (2, 3), 8, 256, 256, geo(14, 0, 12), 16),
    _case("centred_15x23", (2, 3), 8, 256, 256, geo(20, 0, 6), 16, center=True, mean=True, x_row0=1, v_row0=1),
    # a caller's floor: ten values down to 1e-3, eight from 1e-5 on, floor 1e-4 -- ten modes resolved, four completed, "floor"
    _case("relfloor_15x23", (2, 3), 8, 256, 256, np.concatenate([geo(10, 0, 3), geo(8, 5, 8)]), 14, rel_floor=1e-4, v_row0=1),
    _case("fast_71x47", (3, 2), 24, 256, 1024, geo(20, 0, 6), 16, v_row0=2),
    _case("floor_71x47", (3, 2), 24, 256, 1024, geo(14, 0, 12), 16, x_row0=3),
    _case("centred_71x47", (3, 2), 24, 256, 1024, geo(20, 0, 6), 16, center=True, mean=True),
]
NOISE_FLOOR = 1e-13


def pod_truth(case):
    gr = grid(case["blocks"], case["N"])
    return H10Truth(gr, case["M"], case["D"], case["values"], seed=case["M"] * 7 + case["n"], mean=case["mean"])


def check_pod_h10(case, tr, sig, info, V, observed, who="rom_pod_h10"):
    """The assertions of tests/test_gpu_pod_routes.py::check_truth in the H^1_0 geometry (module docstring of
    tests/test_gpu_pod_h10.py) on one call's output; V: the n mode rows (fp64)."""
    gr, cid, n = tr.gr, case["id"], case["n"]
    kap = gr.kappa
    s, s1 = tr.s, tr.s[0]
    fl = max(case["rel_floor"], NOISE_FLOOR)
    gram = info["gram_passes"] > 0
    zeros = min(tr.M - (1 if case["center"] else 0), gr.dim) - tr.r
    s_all = np.concatenate([s, np.zeros(max(zeros, 0))])
    k = int(np.sum(s[:n] > fl * s1))
    assert info["resolved_modes"] == k and info["completed_modes"] == n - k, (cid, info)
    assert info["stop_reason"] == ("filled" if k == n else "floor"), (cid, info)
    st = np.concatenate([s, np.zeros(n)])[:n]
    rel = np.where(st >= 1e-6 * s1, 1e-10, 1e-5) * st
    if gram:
        rel = rel + 1e-14 * s1 ** 2 / np.maximum(st, 1e-300)
    observed(f"{who} {cid}: |sigma - s| / (C eps kappa s_1 + rel)", np.abs(sig[:k] - st[:k]) / (C * EPS * kap * s1 + rel[:k]), 1.0)
    assert np.all(sig[k:] == 0.0), (cid, sig[k:])
    Eg, Et = gr.energy(V[:k]), gr.energy(tr.V[:k])
    ratios = []
    for i in range(k):
        other = np.delete(s_all, i)
        gap = np.min(np.abs(other - s_all[i]))
        gap2 = np.min(np.abs(other ** 2 - s_all[i] ** 2))
        bound = C * EPS * kap * s1 / gap + C * EPS * kap + (2e-14 * s1 ** 2 / gap2 if gram else 0.0)
        c = Eg[i] @ Et[i]
        ratios.append(float(np.sqrt(np.sum((Eg[i] - c * Et[i]) ** 2))) / bound)
    if ratios:
        observed(f"{who} {cid}: H10 mode angle / (C eps kappa s_1 / gap [+ Gram term] + C eps kappa)", np.array(ratios), 1.0)
    G = np.asarray(gr.a1_dots(V, V), dtype=np.float64)
    observed(f"{who} {cid}: |V A_1 V^T - I| (long-double stencil)", np.abs(G - np.eye(n)), 1e-13 + C * EPS * kap)
    piv = np.argmax(np.abs(V), axis=1)
    assert np.all(V[np.arange(n), piv] > 0), (cid, "svd_flip sign convention on the returned rows")
    if k < n:
        Q = np.asarray(gr.transform(V[k:], 0, 1), dtype=np.float64)      # energy coordinates of the completed rows
        res = np.linalg.norm(tr.t.F1[:tr.M] @ (tr.t.F2 @ Q.T), axis=0)   # <x_m - mean, v>_{A_1} through W's exact factors
        observed(f"{who} {cid}: ||X_c v|| (H10 coordinates) of the completed rows / (floor s_1 + C eps kappa s_1)",
                 res / (fl * s1 + C * EPS * kap * s1), 1.0)
