"""Extended-precision referee shared by tests/golden/make_referee.py (fixtures) and the GPU parity tests (rows checked on
the spot).  TEST INFRASTRUCTURE: imports the oracle; nothing in the product path may import this.

    x_0 = SuperLU solve of the oracle's CSC matrix (the reference's call at src/lib/SolutionsManagers.py:31), then
    x_{k+1} = x_k + LU^-1 (b - A x_k)   with the residual evaluated in 80-bit long double in EDGE form
    (A x)_i = sum_j w_ij (x_i - x_j) + (boundary weights) x_i

(differences of neighbouring values first: inside a block that dominates its neighbours they are ~1/c of the values, so the
products carry no cancellation).  The correction contracts by ~kappa * eps per step; iteration stops when it stalls.
"""
import numpy as np
import scipy.sparse.linalg as spla

from oracle import rom_oracle as ro

LD = np.longdouble


def edge_weights(g, a):
    """diag / east / north of the oracle (fp64, exactly what every solver is given) -> edge weights in long double:
    w_e[r,c] couples (r,c)-(r,c+1), w_n[r,c] couples (r,c)-(r+1,c), w_b[r,c] = diag + sum of off-diagonals = the weight
    of the edges to boundary vertices."""
    d, e, n = ro.stencil_arrays(g, a)
    d, e, n = d.astype(LD), e.astype(LD), n.astype(LD)
    wb = d.copy()
    wb[:, :-1] += e
    wb[:, 1:] += e
    wb[:-1, :] += n
    wb[1:, :] += n
    return -e, -n, wb


def residual_ld(g, we, wn, wb, B, x):
    """b - A x in long double, edge form."""
    X = x.reshape(g.nr, g.nc)
    Ax = wb * X
    dh = X[:, :-1] - X[:, 1:]
    Ax[:, :-1] += we * dh
    Ax[:, 1:] -= we * dh
    dv = X[:-1, :] - X[1:, :]
    Ax[:-1, :] += wn * dv
    Ax[1:, :] -= wn * dv
    return (B.astype(LD).reshape(g.nr, g.nc) - Ax).ravel()


def h10_ld(g, v):
    V = v.reshape(g.nr, g.nc)
    s = (V[:, 0] ** 2).sum() + (V[:, -1] ** 2).sum() + (V[0, :] ** 2).sum() + (V[-1, :] ** 2).sum()
    s += ((V[:, :-1] - V[:, 1:]) ** 2).sum() + ((V[:-1, :] - V[1:, :]) ** 2).sum()
    return np.sqrt(s)


def referee(blocks, N, a, max_steps=12, verbose=True, lu=None):
    g = ro.Geometry(blocks, N)
    B = ro.load_vector(g)
    if lu is None:
        lu = spla.splu(ro.assemble_csc(g, a))
    x0 = lu.solve(B)
    we, wn, wb = edge_weights(g, a)
    x = x0.astype(LD)
    hist = []
    for k in range(max_steps):
        r = residual_ld(g, we, wn, wb, B, x)
        dx = lu.solve(np.asarray(r, dtype=np.float64)).astype(LD)
        rel = float(h10_ld(g, dx) / h10_ld(g, x))
        hist.append(rel)
        x = x + dx
        if verbose:
            print(f"  step {k}: |dx|/|x| (H10) = {rel:.3e}", flush=True)
        if rel < 1e-17 or (k > 0 and rel > 0.5 * hist[-2]):
            break
    truth = np.asarray(x, dtype=np.float64)            # nearest fp64 vector to the long-double solution
    err_superlu = float(h10_ld(g, x0.astype(LD) - x) / h10_ld(g, x))
    return g, truth, x0, err_superlu, hist


# ---- the reduced Galerkin systems (C A(a) C^T) c = C B in extended precision ------------------------------------------
def _energy_forms_ld(g, Q):
    """Per coefficient block b: S_b = Q A_b Q^T (n x n, long double), edge form -- sum_edges w (dq_i)(dq_j) + boundary
    terms -- with the oracle's own fp64 stencil weights of the one-hot coefficient (exact small numbers)."""
    n = Q.shape[0]
    Q3 = Q.reshape(n, g.nr, g.nc)
    Dh = (Q3[:, :, :-1] - Q3[:, :, 1:]).reshape(n, -1)
    Dv = (Q3[:, :-1, :] - Q3[:, 1:, :]).reshape(n, -1)
    Qf = Q3.reshape(n, -1)
    forms = []
    for p, q, e in ro._block_onehots(g):
        we, wn, wb = edge_weights(g, e)
        S = np.einsum("ik,jk->ij", Dh * we.ravel(), Dh) + np.einsum("ik,jk->ij", Dv * wn.ravel(), Dv) \
            + np.einsum("ik,jk->ij", Qf * wb.ravel(), Qf)
        forms.append(0.5 * (S + S.T))
    return forms


def _a1_dots_ld(g, X, Y):
    """X A_1 Y^T in long double (edge form; rows of X, Y are FE vectors)."""
    we, wn, wb = edge_weights(g, np.ones((g.nrb, g.ncb)))
    nx, ny = X.shape[0], Y.shape[0]
    X3, Y3 = X.reshape(nx, g.nr, g.nc), Y.reshape(ny, g.nr, g.nc)
    out = np.einsum("ik,jk->ij", ((X3[:, :, :-1] - X3[:, :, 1:]) * we).reshape(nx, -1), (Y3[:, :, :-1] - Y3[:, :, 1:]).reshape(ny, -1))
    out += np.einsum("ik,jk->ij", ((X3[:, :-1, :] - X3[:, 1:, :]) * wn).reshape(nx, -1), (Y3[:, :-1, :] - Y3[:, 1:, :]).reshape(ny, -1))
    out += np.einsum("ik,jk->ij", (X3 * wb).reshape(nx, -1), Y3.reshape(ny, -1))
    return out


def a1_orthonormal_span_ld(g, C, drop=1e-16):
    """Rows of C (fp64) -> A_1-orthonormal long-double basis of their EXACT span, nested in the row order (modified
    Gram-Schmidt, twice); a row whose remainder is below `drop` of its own norm is reported as dependent (kept as zero)."""
    C = np.asarray(C, dtype=np.float64)
    Q = C.astype(LD).copy()
    keep = np.ones(len(Q), dtype=bool)
    for i in range(len(Q)):
        n0 = np.sqrt(_a1_dots_ld(g, Q[i:i + 1], Q[i:i + 1])[0, 0])
        for _ in range(2):
            if i:
                h = _a1_dots_ld(g, Q[i:i + 1], Q[:i])[0]
                Q[i] -= h @ Q[:i]
        n1 = np.sqrt(_a1_dots_ld(g, Q[i:i + 1], Q[i:i + 1])[0, 0])
        if not n1 > drop * n0:
            keep[i] = False
            Q[i] = 0
        else:
            Q[i] /= n1
    return Q, keep


def _chol_solve_batched_ld(A, b):
    """A (M, n, n) SPD, b (n,) or (M, n): long-double Cholesky + substitutions, batched over M."""
    M, n, _ = A.shape
    Lc = np.zeros_like(A)
    for j in range(n):
        d = A[:, j, j] - np.einsum("mk,mk->m", Lc[:, j, :j], Lc[:, j, :j])
        Lc[:, j, j] = np.sqrt(d)
        if j + 1 < n:
            Lc[:, j + 1:, j] = (A[:, j + 1:, j] - np.einsum("mik,mk->mi", Lc[:, j + 1:, :j], Lc[:, j, :j])) / Lc[:, j, j][:, None]
    y = np.zeros((M, n), dtype=LD)
    bb = np.broadcast_to(np.asarray(b, dtype=LD), (M, n))
    for i in range(n):
        y[:, i] = (bb[:, i] - np.einsum("mk,mk->m", Lc[:, i, :i], y[:, :i])) / Lc[:, i, i]
    x = np.zeros((M, n), dtype=LD)
    for i in range(n - 1, -1, -1):
        x[:, i] = (y[:, i] - np.einsum("mk,mk->m", Lc[:, i + 1:, i], x[:, i + 1:])) / Lc[:, i, i]
    return x


def galerkin_truth_nested(g, a, C, U, sizes):
    """Relative H10 errors of the Galerkin ROM (src/lib/SolutionsManagers.py:88-106) on span{C[0], ..., C[j-1]} for every
    j in `sizes`, in 80-bit arithmetic from the fp64 inputs (basis rows C, snapshots U, parameters a): the truth the fp64
    routes to the same numbers -- reference, oracle, GPU rows, GPU factored -- are measured against where they disagree.
    With an A_1-orthonormal long-double basis Q of the exact span, (sum_b a_b S_b) c = Q B has a condition number <= the
    contrast, and  ||u - Q^T c||^2 = (||u||^2 - |p|^2) + |p - c|^2,  p = Q A_1 u  (a projection residual + a sum of squares).
    Returns {j: errors (M,)} as float64."""
    a = np.asarray(a, dtype=np.float64).reshape(len(a), -1)
    U = np.asarray(U, dtype=np.float64)
    Q, keep = a1_orthonormal_span_ld(g, C)
    forms = _energy_forms_ld(g, Q)
    bhat = Q @ ro.load_vector(g).astype(LD)
    P = _a1_dots_ld(g, U.astype(LD), Q)                      # (M, n)
    u2 = np.array([h10_ld(g, u.astype(LD)) ** 2 for u in U])
    aL = a.astype(LD)
    out = {}
    for j in sizes:
        idx = np.flatnonzero(keep[:j])
        A = sum(aL[:, b][:, None, None] * forms[b][np.ix_(idx, idx)][None] for b in range(a.shape[1]))
        c = _chol_solve_batched_ld(A, bhat[idx])
        Pj = P[:, idx]
        e2 = (u2 - np.einsum("mk,mk->m", Pj, Pj)) + np.einsum("mk,mk->m", Pj - c, Pj - c)
        out[j] = np.asarray(np.sqrt(np.maximum(e2, 0) / u2), dtype=np.float64)
    return out


# ---- the strong greedy along a given pick sequence, in extended precision -------------------------------------------
def _grad_ld(g, X):
    """Rows of X (FE vectors) -> long-double coordinates in which the A_1 inner product is Euclidean: the edge differences
    and the boundary values, each scaled by the square root of its (nonnegative) edge weight."""
    we, wn, wb = edge_weights(g, np.ones((g.nrb, g.ncb)))
    assert we.min() >= 0 and wn.min() >= 0 and wb.min() >= 0
    X3 = np.asarray(X).astype(LD).reshape(len(X), g.nr, g.nc)
    return np.concatenate((((X3[:, :, :-1] - X3[:, :, 1:]) * np.sqrt(we)).reshape(len(X), -1),
                           ((X3[:, :-1, :] - X3[:, 1:, :]) * np.sqrt(wn)).reshape(len(X), -1),
                           (X3 * np.sqrt(wb)).reshape(len(X), -1)), axis=1)


def greedy_ld(g, U, a, h1norm, picks, galerkin, drop=1e-16):
    """The error vectors of the strong greedy (src/lib/ReducedBasis.py:112-139) along the pick sequence `picks` of a device
    call, in 80-bit arithmetic from the fp64 rows U (M, dim): row i of the result (len(picks), M) holds the relative
    errors e_i = ||u_m - approx_m|| / h1norm_m for the EXACT span of picks[:i] -- H^1_0 projection, or (galerkin) the
    Galerkin ROM with parameters a (M, kblk): ||R_m||^2 + |p_m - c_m|^2 as in galerkin_truth_nested.

    The span is carried as an A_1-orthonormal basis built incrementally (Gram-Schmidt twice per pick); the residuals of all
    rows are updated by one vector per iteration, O(M dim) each.  A pick whose remainder is below `drop` of its own norm
    enters as a zero direction (the device's dead-direction convention: no coupling, coefficient 0).  In Galerkin mode the
    reduced matrices sum_b a_mb S_b (condition <= the contrast in this basis) grow by one row per iteration; their
    Cholesky factors and the factors' inverses are bordered, O(M n^2) per iteration.  Returns (errors, live) with live[j]
    False where pick j entered as a zero direction."""
    U = np.asarray(U, dtype=np.float64)
    M, n = U.shape[0], len(picks)
    h1 = np.broadcast_to(np.asarray(h1norm, dtype=np.float64), (M,)).astype(LD)
    GU = _grad_ld(g, U)
    R = GU.copy()                                   # residuals of the projection, A_1 coordinates
    nrm0 = np.sqrt(np.einsum("me,me->m", GU, GU))
    out = np.zeros((n, M), dtype=LD)
    live = np.ones(n, dtype=bool)
    QF = np.zeros((max(n - 1, 0), U.shape[1]), dtype=LD)    # basis as FE vectors
    QG = np.zeros((max(n - 1, 0), GU.shape[1]), dtype=LD)   # and in A_1 coordinates
    if galerkin:
        a = np.asarray(a, dtype=np.float64).reshape(M, -1).astype(LD)
        k = a.shape[1]
        blocks = [edge_weights(g, e) for _, _, e in ro._block_onehots(g)]
        B = ro.load_vector(g).astype(LD)
        nb = max(n - 1, 0)
        Sb = np.zeros((k, nb, nb), dtype=LD)
        Linv = np.zeros((M, nb, nb), dtype=LD)      # inverses of the Cholesky factors of the reduced matrices
        y = np.zeros((M, nb), dtype=LD)             # L^-1 bhat
        P = np.zeros((M, nb), dtype=LD)             # projection coefficients p_mj = <u_m, q_j>_A1
    gap2 = np.zeros(M, dtype=LD)
    for i in range(n):
        e2 = np.einsum("me,me->m", R, R)
        out[i] = np.sqrt(e2 + gap2) / h1
        if i == n - 1:
            break
        p = picks[i]
        qf, qg = U[p].astype(LD), GU[p].copy()
        for _ in range(2):
            if i:
                h = QG[:i] @ qg
                qf -= h @ QF[:i]
                qg -= h @ QG[:i]
        nq = np.sqrt(qg @ qg)
        if not nq > drop * nrm0[p]:
            live[i] = False
            qf[:], qg[:] = 0, 0
        else:
            qf, qg = qf / nq, qg / nq
        QF[i], QG[i] = qf, qg
        pj = R @ qg
        R -= pj[:, None] * qg[None, :]
        if not galerkin:
            continue
        P[:, i] = pj
        # the new row / column of every S_b (q_i^T A_b q_j, edge form) and of bhat
        Q3 = QF[:i + 1].reshape(i + 1, g.nr, g.nc)
        for b, (we, wn, wb) in enumerate(blocks):
            Av = wb * Q3[i]
            dh = Q3[i][:, :-1] - Q3[i][:, 1:]
            Av[:, :-1] += we * dh
            Av[:, 1:] -= we * dh
            dv = Q3[i][:-1, :] - Q3[i][1:, :]
            Av[:-1, :] += wn * dv
            Av[1:, :] -= wn * dv
            col = np.einsum("jrc,rc->j", Q3, Av)
            Sb[b, i, :i + 1] = col
            Sb[b, :i + 1, i] = col
        bh = qf @ B
        if not live[i]:                             # zero direction: unit diagonal, no coupling, coefficient 0
            Linv[:, i, i] = 1
            continue
        Acol = (a[:, :, None] * Sb[None, :, :i + 1, i]).sum(axis=1)  # (M, i+1): column i of every reduced matrix
        # (explicit products and sums: einsum on these strided long-double views has returned NaN at random)
        l = (Linv[:, :i, :i] * Acol[:, None, :i]).sum(axis=2)          # L^-1 A[:i, i]
        d = np.sqrt(Acol[:, i] - (l * l).sum(axis=1))
        r = -(l[:, :, None] * Linv[:, :i, :i]).sum(axis=1) / d[:, None]
        Linv[:, i, :i], Linv[:, i, i] = r, 1 / d
        y[:, i] = (bh - (l * y[:, :i]).sum(axis=1)) / d
        c = (Linv[:, :i + 1, :i + 1] * y[:, :i + 1, None]).sum(axis=1)  # L^-T y
        gap2 = ((P[:, :i + 1] - c) ** 2).sum(axis=1)
    return out, live


# ---- blocks whose SVD is known exactly ------------------------------------------------------------------------------
def hadamard_columns(n, cols):
    """Columns `cols` of the Sylvester Hadamard matrix H_n (n a power of two), as float64 +-1: H[i, j] = (-1)^popcount(i & j)."""
    assert n >= 1 and n & (n - 1) == 0
    cols = np.asarray(cols, dtype=np.int64)
    x = np.arange(n, dtype=np.int64)[:, None] & cols[None, :]
    par = np.zeros(x.shape, dtype=np.int64)
    while x.any():
        par ^= x & 1
        x >>= 1
    return 1.0 - 2.0 * par


class ExactSVD:
    """An (M, dim) fp64 block X = mean + sum_k s_k u_k v_k^T whose SVD is known exactly (tests/test_referee_pod.py proves it).

    u_k = H_M[:, L_k] / sqrt(M) with L_k != 0 (the columns of H_M other than column 0 sum to zero: centring leaves the block
    unchanged), v_k = the column R_k of H_D / sqrt(D) scattered into `dim` coordinates by a seeded injection, s_k = m_k 2^-e
    with integers m_k.  With log2(M D) even, 1 / sqrt(M D) is a power of two; every entry is an integer multiple of
    q = 2^-e / sqrt(M D) below 2^53 q (sum m_k + max |mean| < 2^53), so every partial sum of an entry, of a column sum or
    of a product with the factors is exact in any order.  Rows past M (zero rows, `pad`) are for uncentred cases only.

    Attributes: X (rows, dim) -- or None when built lazily (`factors` then holds F1 (rows, r), F2 (r, dim) with X = F1 F2
    exactly, plus the mean); s (r,) descending; V (r, dim) the true right singular vectors; mean (dim,).

    coherent=True: u_k = e_{L_k} instead, r distinct rows of any M (no mean, uncentred cases only), D a power of four.  Every
    entry is then ONE term s_k (+-1) / sqrt(D), and the Gram matrix X X^T is diagonal: its pivoted Cholesky factor follows
    the squared singular values exactly (Hadamard left vectors are incoherent -- every row mixes every mode -- and its
    pivots fall much more slowly than the spectrum)."""

    def __init__(self, M, D, dim, mant, e, seed=0, mean_int=None, pad=0, build=True, coherent=False):
        if coherent:
            assert D & (D - 1) == 0 and D.bit_length() % 2 == 1 and mean_int is None and pad == 0, "D a power of four"
        else:
            assert M & (M - 1) == 0 and D & (D - 1) == 0 and (M * D).bit_length() % 2 == 1, "log2(M D) must be even"
        mant = np.asarray(mant, dtype=np.int64)
        order = np.argsort(-mant, kind="stable")
        mant = mant[order]
        r = len(mant)
        assert r < M and r <= D and dim >= D and mant.min() >= 0
        rng = np.random.default_rng(seed)
        self.L = rng.choice(M, size=r, replace=False) if coherent else 1 + rng.choice(M - 1, size=r, replace=False)
        self.R = rng.choice(D, size=r, replace=False)
        self.cols = np.sort(rng.choice(dim, size=D, replace=False)) if dim > D else np.arange(dim)
        self.cols = rng.permutation(self.cols)
        self.M, self.D, self.dim, self.r, self.pad, self.e, self.coherent = M, D, dim, r, pad, e, coherent
        self.mant = mant
        lg = ((1 if coherent else M) * D).bit_length() - 1
        self.q = 2.0 ** (-e - lg // 2)                 # the quantum: 2^-e / sqrt(M D)
        self.s = mant.astype(np.float64) * 2.0 ** -e
        bound = int(mant.sum()) + (0 if mean_int is None else int(np.abs(mean_int).max()))
        assert bound * M < 2 ** 53, "entries or column sums would not be exact"
        self.mean_int = np.zeros(dim, dtype=np.int64) if mean_int is None else np.asarray(mean_int, dtype=np.int64)
        self.mean = self.mean_int.astype(np.float64) * self.q
        hd = hadamard_columns(D, self.R)               # (D, r)
        self.F2 = np.zeros((r, dim))
        self.F2[:, self.cols] = hd.T
        self.V = self.F2 / np.sqrt(D)
        if coherent:
            self.F1 = np.zeros((M, r))
            self.F1[self.L, np.arange(r)] = mant.astype(np.float64) * self.q
        else:
            self.F1 = hadamard_columns(M, self.L) * (mant.astype(np.float64) * self.q)[None, :]   # (M, r), exact
        if pad:
            self.F1 = np.vstack((self.F1, np.zeros((pad, r))))
        self.X = self.dense() if build else None

    @property
    def rows(self):
        return self.M + self.pad

    def dense(self):
        X = self.F1 @ self.F2                          # exact: integer multiples of q below 2^53 q in any order
        if self.mean_int.any():
            X[:self.M] += self.mean[None, :]
        return X

    def entry_int(self, i, j):
        """X[i, j] / q in Python integer arithmetic (the proof of exactness)."""
        if i >= self.M:
            return 0
        tot = int(self.mean_int[j])
        where = np.flatnonzero(self.cols == j)
        if where.size:
            c = int(where[0])
            for k in range(self.r):
                if self.coherent:
                    if i != int(self.L[k]):
                        continue
                    hm = 1
                else:
                    hm = -1 if bin(i & int(self.L[k])).count("1") & 1 else 1
                hd = -1 if bin(c & int(self.R[k])).count("1") & 1 else 1
                tot += hm * hd * int(self.mant[k])
        return tot

    def centred(self):
        """The block after centring: the same product without the mean (u_k sum to zero)."""
        assert self.pad == 0 and not self.coherent
        return self.F1 @ self.F2
