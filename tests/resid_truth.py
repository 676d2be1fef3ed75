"""Long-double truth for the residual-estimator tests (tests/test_resid_host.py, tests/test_gpu_resid.py).  TEST
INFRASTRUCTURE: nothing in the product path may import this.

For an A_1-orthonormal basis W (rows) and coefficients c of u_n = W^T c:
    r = f - A(a) W^T c          edge form in 80 bits (referee.residual_ld),
    ||r||_{H^-1}                through h10_truth.Grid.transform(., 0, -1) (A_1 = S Lambda S),
    S(a, c) = sum_j |z_j| ||g^_j||_2,  z = (1, -c_i a_q), g_0 = f, g_{1+ik+q} = A_q w_i     the scale of the bound
    |Delta - Delta_truth| <= C eps (P + nr + nc) S,  C = 64, eps = 2^-53
(P terms of the thin product R z plus the (nr + nc) of h10_truth.Grid.transform_bound: the project's convention).  The bound
is absolute: the residual of a parameter whose snapshot is in the basis is pure noise.
`NumpyEstimator` is the plain fp64 NumPy restatement of the device algorithm (Householder QR of the g^_j) that the bound is
checked against on the CPU, and `gram_form` the textbook z^T G z that it documents as useless here.
"""
import numpy as np

from oracle import rom_oracle as ro
import h10_truth as ht
import referee as rf

LD = np.longdouble
EPS = 2.0 ** -53
C = 64.0

# id, blocks, mesh N, basis rows n, parameters M, exponent e of a = 10^U(0, e), a_row0 / d_off / coef_row0
CASES = [
    ("sq_n0_m1", (2, 2), 8, 0, 1, 2, 0),
    ("sq_n1_m70", (2, 2), 8, 1, 70, 6, 3),
    ("sq_n5_m300", (2, 2), 8, 5, 300, 2, 0),
    ("sq_n17_m70", (2, 2), 8, 17, 70, 6, 2),
    ("rect_n0_m70", (2, 3), 8, 0, 70, 2, 1),
    ("rect_n1_m1", (2, 3), 8, 1, 1, 6, 0),
    ("rect_n5_m70", (2, 3), 8, 5, 70, 6, 0),
    ("rect_n17_m300", (2, 3), 8, 17, 300, 2, 5),
    ("tall_n5_m70", (3, 2), 24, 5, 70, 2, 0),
    ("tall_n17_m1", (3, 2), 24, 17, 1, 6, 1),
]
DEEP = dict(blocks=(2, 2), N=8, e=2, seed=1, M=48, n=22)
GREEDY = dict(blocks=(2, 2), N=8, e=2, seed=7, M=300, n=10)


def params(blocks, M, e, seed):
    return 10.0 ** np.random.default_rng(seed).uniform(0, e, size=(M,) + tuple(blocks))


def case_inputs(case):
    """(training parameters a (M,) + blocks, basis parameters (n,) + blocks) of a case."""
    cid, blocks, N, n, M, e, _ = case
    return params(blocks, M, e, len(cid)), params(blocks, n, e, 1000 + len(cid))


class Truth:
    def __init__(self, blocks, N):
        self.blocks, self.N = tuple(blocks), N
        self.gr = ht.grid(blocks, N)
        self.g = self.gr.g
        self.k = blocks[0] * blocks[1]
        self.dim = self.gr.dim
        self.f64 = ro.load_vector(self.g)
        self.f = self.f64.astype(LD)
        self.onehots = []
        for q in range(self.k):
            e = np.zeros(self.blocks)
            e[q // blocks[1], q % blocks[1]] = 1.0
            self.onehots.append(e)
        self.ew = [rf.edge_weights(self.g, e) for e in self.onehots]
        self.Aq = [ro.assemble_csc(self.g, e) for e in self.onehots]   # fp64, for the NumPy restatement
        self.zero = np.zeros(self.dim)

    # -- long double ----------------------------------------------------------------------------------------------
    def apply_block(self, q, x):
        we, wn, wb = self.ew[q]
        return -rf.residual_ld(self.g, we, wn, wb, self.zero, np.asarray(x, dtype=LD))

    def functionals(self, W):
        """(1 + k n, dim) long double: f, then A_q w_i, i-major."""
        rows = [self.f]
        for w in np.asarray(W):
            rows += [self.apply_block(q, w) for q in range(self.k)]
        return np.array(rows, dtype=LD)

    def ghat(self, G):
        return self.gr.transform(G, 0, -1)

    def ghat_norms(self, W):
        Gh = self.ghat(self.functionals(W))
        return np.asarray(np.sqrt((Gh * Gh).sum(axis=1)), dtype=np.float64)

    def z(self, a, c):
        a = np.asarray(a, dtype=np.float64).reshape(len(a), -1)
        c = np.asarray(c, dtype=np.float64).reshape(len(a), -1)
        return np.hstack([np.ones((len(a), 1)), (-c[:, :, None] * a[:, None, :]).reshape(len(a), -1)])

    def residuals(self, W, a, c):
        """||f - A(a_m) W^T c_m||_{H^-1} in long double, (M,) float64."""
        a = np.asarray(a, dtype=np.float64).reshape(len(a), -1)
        WL = np.asarray(W).astype(LD).reshape(-1, self.dim)
        cL = np.asarray(c).astype(LD).reshape(len(a), -1)
        R = np.zeros((len(a), self.dim), dtype=LD)
        for m in range(len(a)):
            we, wn, wb = rf.edge_weights(self.g, a[m].reshape(self.blocks))
            x = cL[m] @ WL if WL.shape[0] else np.zeros(self.dim, dtype=LD)
            R[m] = rf.residual_ld(self.g, we, wn, wb, self.f64, x)
        Rh = self.ghat(R)
        return np.asarray(np.sqrt((Rh * Rh).sum(axis=1)), dtype=np.float64)

    def scale(self, W, a, c, norms=None):
        """S(a, c) = sum_j |z_j| ||g^_j||_2, (M,)."""
        norms = self.ghat_norms(W) if norms is None else norms
        return np.abs(self.z(a, c)) @ norms

    def bound(self, W, a, c, norms=None):
        P = 1 + self.k * len(np.asarray(W).reshape(-1, self.dim))
        return C * EPS * (P + self.gr.nr + self.gr.nc) * self.scale(W, a, c, norms)

    def h10(self, V):
        return np.array([float(rf.h10_ld(self.g, np.asarray(v).astype(LD))) for v in np.asarray(V).reshape(-1, self.dim)])

    # -- truth snapshots and the reduced systems in long double ----------------------------------------------------
    def snapshots(self, a):
        """fp64 roundings of the long-double solutions (referee: iterative refinement with 80-bit residuals)."""
        a = np.asarray(a, dtype=np.float64).reshape((-1,) + self.blocks)
        return np.array([rf.referee(self.blocks, self.N, am, verbose=False)[1] for am in a]).reshape(len(a), self.dim)

    def reduced_ld(self, Q, a):
        """c (M, n) long double for the A_1-orthonormal long-double rows Q (zero rows: dead, c = 0)."""
        a = np.asarray(a, dtype=np.float64).reshape(len(a), -1)
        n = len(Q)
        c = np.zeros((len(a), n), dtype=LD)
        live = np.flatnonzero(np.abs(Q).sum(axis=1) > 0)
        if live.size:
            forms = rf._energy_forms_ld(self.g, Q[live])
            A = sum(a.astype(LD)[:, b][:, None, None] * forms[b][None] for b in range(self.k))
            c[:, live] = rf._chol_solve_batched_ld(A, Q[live] @ self.f)
        return c

    def weak_greedy_ld(self, a, n, weights=None):
        """The weak greedy in long double: picks, criteria (n,), top-two gaps relative to the maximum (n,), the truth
        snapshots of the picks (n, dim), per step the criteria of all parameters (n, M; -1 at picked ones), and the bound
        (times the weight) of every pick's criterion (n,)."""
        a2 = np.asarray(a, dtype=np.float64).reshape(len(a), -1)
        w = np.ones(len(a2)) if weights is None else np.asarray(weights, dtype=np.float64)
        picks, crits, gaps, rows, allc, pb = [], [], [], np.zeros((0, self.dim)), [], []
        for step in range(n):
            Q, _ = rf.a1_orthonormal_span_ld(self.g, rows) if len(rows) else (np.zeros((0, self.dim), dtype=LD), None)
            c = self.reduced_ld(Q, a2)
            crit = self.residuals(Q, a2, c) * w
            crit[picks] = -1.0
            order = np.argsort(-crit, kind="stable")
            picks.append(int(order[0]))
            crits.append(float(crit[order[0]]))
            gaps.append(float((crit[order[0]] - crit[order[1]]) / crit[order[0]]) if len(order) > 1 else 1.0)
            allc.append(crit.copy())
            pb.append(float(self.bound(Q, a2[picks[-1]][None], c[picks[-1]][None])[0] * w[picks[-1]]))
            rows = np.vstack([rows, self.snapshots(a2[picks[-1]][None])])
        return picks, np.array(crits), np.array(gaps), rows, np.array(allc), np.array(pb)


_TRUTHS = {}


def truth(blocks, N):
    key = (tuple(blocks), N)
    if key not in _TRUTHS:
        _TRUTHS[key] = Truth(*key)
    return _TRUTHS[key]


# ---- the plain fp64 NumPy restatement ----------------------------------------------------------------------------------
class NumpyEstimator:
    """fp64: W by CGS2 in the A_1 inner product, the reduced systems by LAPACK, g^_j by the fp64 transform of the sparse
    products A_q w_i, R from the Householder QR of the g^_j, Delta = ||R z||_2."""

    def __init__(self, tr: Truth, basis):
        self.tr = tr
        g, dim = tr.g, tr.dim
        A1 = ro.assemble_csc(g, np.ones(tr.blocks))
        W = np.zeros((0, dim))
        for row in np.asarray(basis, dtype=np.float64).reshape(-1, dim):
            v = row.copy()
            for _ in range(2):
                if len(W):
                    v = v - (W @ (A1 @ v)) @ W
            W = np.vstack([W, v / np.sqrt(v @ (A1 @ v))])
        self.W = W
        n = len(W)
        G = [tr.f64] + [tr.Aq[q] @ W[i] for i in range(n) for q in range(tr.k)]
        self.Gh = tr.gr.transform(np.array(G), 0, -1, ld=False)
        self.R = np.linalg.qr(self.Gh.T, mode="r")
        self.forms = [W @ (tr.Aq[q] @ W.T) for q in range(tr.k)] if n else []
        self.bhat = W @ tr.f64 if n else np.zeros(0)

    def coefficients(self, a):
        a = np.asarray(a, dtype=np.float64).reshape(len(a), -1)
        if not len(self.W):
            return np.zeros((len(a), 0))
        return np.array([np.linalg.solve(sum(am[q] * self.forms[q] for q in range(self.tr.k)), self.bhat) for am in a])

    def delta(self, a, c):
        return np.linalg.norm(self.tr.z(a, c) @ self.R.T, axis=1)

    def gram_form(self, a, c):
        z = self.tr.z(a, c)
        G = self.Gh @ self.Gh.T
        return np.sqrt(np.maximum(np.einsum("mi,ij,mj->m", z, G, z), 0.0))


def oracle_snapshots(tr: Truth, a):
    a = np.asarray(a, dtype=np.float64).reshape((-1,) + tr.blocks)
    return np.asarray(ro.generate_solutions(tr.g, a, "lsqsparse")).reshape(len(a), tr.dim) if len(a) else np.zeros((0, tr.dim))
