"""rom_riesz_h10 (H^1_0 Riesz representers of point sensors) and PBDW state estimation on an MI355X.

Representers:
* small geometries, nr != nc among them: A_1 omega_i = generate_riesz(x, "l2")[i] against a dense fp64 solve, for random
  points, points on cell edges, on mesh vertices and on block interfaces; a point on the boundary gives exactly zero;
* C2 and C4, a referee independent of the method: the residual r_i - A_1 omega_i in long double on the host (integer
  stencil, weights from the same fp64 tx / ty) and its A_1^-1 norm from a sparse direct solve;
* G symmetric to the bit, equal to [l_i(omega_j)], Gram-only call bit-identical to the full call;
* repeat calls and ROMHC_POISON_WS give identical bits; npts = 0 and 1; a point outside the domain raises.
PBDW (greedy basis, n in {0, 1, 10, 20}, m in {20, 50} separated points):
* interpolation, the optimality property dist(u*, V_n) <= dist(u, V_n), H^1_0-orthogonality of the correction,
  the a-priori bound ||u - u*|| <= dist(u, V_n) / beta_n, reproduction of span V_n, n = 0 = minimum-norm interpolant;
* a host restatement (SciPy representers + dense saddle point) at (2,2) N=8;
* ndarray / DeviceArray bases give identical bits, return_coefs feeds the parameter estimators, ValueError cases.
Representers, G and the norms against an 80-bit truth with derived bounds (grids with nr != nc across a 64-row tile, the
split launch of the second transform): tests/test_gpu_sensor_truth.py; it shares _points with this module.
"""
import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

from conftest import observed

pytestmark = pytest.mark.gpu

_SM = {}


def _sm(blocks, N):
    from romhighcontrast_amd.lib.SolutionsManagers import SolutionsManagerFEM
    key = (tuple(blocks), N)
    if key not in _SM:
        _SM[key] = SolutionsManagerFEM(tuple(blocks), N)
    return _SM[key]


def _a1_sparse(sm):
    nr, nc = sm.nr_inner_vertices, sm.nc_inner_vertices
    Tr = sp.diags([-np.ones(nr - 1), 2 * np.ones(nr), -np.ones(nr - 1)], [-1, 0, 1])
    Tc = sp.diags([-np.ones(nc - 1), 2 * np.ones(nc), -np.ones(nc - 1)], [-1, 0, 1])
    return (sp.kron(Tr, sp.eye(nc)) + sp.kron(sp.eye(nr), Tc)).tocsc()


def _eval_rows(sm, pts):
    """The evaluation functionals as (dof indices, fp64 weights) per point: the convention of k_eval_points."""
    ix, iy, tx, ty = sm._locate(pts)
    nr, nc = sm.nr_inner_vertices, sm.nc_inner_vertices
    out = []
    for x0, y0, qx, qy in zip(ix, iy, tx, ty):
        if qx + qy < 1:
            vs = [(1 - qx - qy, y0, x0), (qx, y0, x0 + 1), (qy, y0 + 1, x0)]
        else:
            vs = [(qx + qy - 1, y0 + 1, x0 + 1), (1 - qx, y0 + 1, x0), (1 - qy, y0, x0 + 1)]
        out.append([((y - 1) * nc + (x - 1), w) for w, y, x in vs if 1 <= y <= nr and 1 <= x <= nc])
    return out


def _points(sm, kind, m, seed):
    rng = np.random.default_rng(seed)
    (x0, x1), (y0, y1) = sm.x_domain, sm.y_domain
    pc, pr = sm.points_c, sm.points_r
    if kind == "random":
        return np.c_[rng.uniform(x0, x1, m), rng.uniform(y0, y1, m)]
    if kind == "edges":   # on vertical and horizontal grid lines, and on the diagonals of the SW-NE split
        a = np.c_[pc[rng.integers(1, len(pc) - 1, m)], rng.uniform(y0, y1, m)]
        b = np.c_[rng.uniform(x0, x1, m), pr[rng.integers(1, len(pr) - 1, m)]]
        i, j, t = rng.integers(0, len(pc) - 1, m), rng.integers(0, len(pr) - 1, m), rng.uniform(0, 1, m)
        c = np.c_[pc[i] + t * (pc[i + 1] - pc[i]), pr[j] + (1 - t) * (pr[j + 1] - pr[j])]
        return np.r_[a, b, c]
    if kind == "vertices":
        return np.c_[pc[rng.integers(1, len(pc) - 1, m)], pr[rng.integers(1, len(pr) - 1, m)]]
    if kind == "interfaces":  # block interfaces: integer offsets from the domain corner
        nrb, ncb = sm.blocks_geometry
        xi = x0 + rng.integers(1, ncb, m) if ncb > 1 else rng.uniform(x0, x1, m)
        yi = y0 + rng.integers(1, nrb, m) if nrb > 1 else rng.uniform(y0, y1, m)
        return np.r_[np.c_[xi, rng.uniform(y0, y1, m)], np.c_[rng.uniform(x0, x1, m), yi], np.c_[xi, yi]]
    raise ValueError(kind)


def _separated(sm, m, seed, sep):
    rng = np.random.default_rng(seed)
    (x0, x1), (y0, y1) = sm.x_domain, sm.y_domain
    pts = []
    while len(pts) < m:
        p = np.array([rng.uniform(x0 + 0.05, x1 - 0.05), rng.uniform(y0 + 0.05, y1 - 0.05)])
        if all(np.hypot(*(p - q)) >= sep for q in pts):
            pts.append(p)
    return np.array(pts)


def _h10(A, E):
    """row-wise sqrt(e^T A e)"""
    E = np.atleast_2d(E)
    return np.sqrt(np.maximum(np.einsum("ij,ij->i", E, (A @ E.T).T), 0.0))


# ---- representers ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("blocks,N", [((1, 1), 4), ((2, 2), 8), ((3, 2), 5), ((3, 3), 16)])
def test_representers_small_against_dense_solve(blocks, N):
    sm = _sm(blocks, N)
    pts = np.r_[_points(sm, "random", 6, 1), _points(sm, "edges", 3, 2), _points(sm, "vertices", 4, 3),
                _points(sm, "interfaces", 2, 4), [[sm.x_domain[1], 0.1 * sm.y_domain[1]]]]
    A1 = sm.A_preassembled4h1_norm
    R = sm.generate_riesz(pts, "l2")
    # the host functional rows used by the referees below are the same as generate_riesz's
    Rh = np.zeros_like(R)
    for i, row in enumerate(_eval_rows(sm, pts)):
        for j, w in row:
            Rh[i, j] += w
    assert np.array_equal(Rh, R)
    Om = sm.generate_riesz_h10(pts)
    assert Om.shape == R.shape
    assert not np.any(R[-1])
    # a point on the boundary (and, on coarse meshes, a point in a triangle whose vertices are all on the boundary) has
    # a vanishing functional and an exactly zero representer
    zero = ~np.any(R, axis=1)
    assert zero[-1] and not np.any(Om[zero]), "a vanishing functional must have an exactly zero representer"
    ref = np.linalg.solve(A1, R[~zero].T).T
    rel = _h10(A1, Om[~zero] - ref) / _h10(A1, ref)
    observed(f"riesz {blocks} N={N}: relative H1_0 error vs dense solve", rel, 1e-12)
    res = np.max(np.abs(Om @ A1 - R)) / np.max(np.abs(R))
    observed(f"riesz {blocks} N={N}: max |A_1 omega - r| / max |r|", res, 1e-12)
    # generate_riesz(x, "h10") keeps the reference's behaviour
    with pytest.raises(Exception, match="Not implemented"):
        sm.generate_riesz(pts, "h10")


@pytest.mark.parametrize("blocks,N,m", [((2, 2), 128, 16), ((3, 3), 171, 8)])
def test_representers_referee_long_double(blocks, N, m):
    sm = _sm(blocks, N)
    pts = np.r_[_points(sm, "random", m - 4, 10), _points(sm, "vertices", 2, 11), _points(sm, "edges", 1, 12)[:2]]
    Om_d, G = sm.riesz_h10_device(pts)
    Om = Om_d.numpy()
    nr, nc = sm.nr_inner_vertices, sm.nc_inner_vertices
    ld = np.longdouble
    W = Om.astype(ld).reshape(-1, nr, nc)
    AW = 4 * W
    AW[:, 1:, :] -= W[:, :-1, :]
    AW[:, :-1, :] -= W[:, 1:, :]
    AW[:, :, 1:] -= W[:, :, :-1]
    AW[:, :, :-1] -= W[:, :, 1:]
    res = -AW.reshape(len(pts), -1)
    for i, row in enumerate(_eval_rows(sm, pts)):
        for j, w in row:
            res[i, j] += ld(w)
    res = res.astype(np.float64)
    lu = spla.splu(_a1_sparse(sm))
    e = lu.solve(res.T).T
    err = np.sqrt(np.maximum(np.einsum("ij,ij->i", res, e), 0.0))
    rel = err / np.sqrt(np.diag(G))
    observed(f"riesz {blocks} N={N}: relative H1_0 error, long-double residual referee", rel, 1e-11)


@pytest.mark.parametrize("blocks,N", [((2, 2), 8), ((3, 2), 5), ((2, 2), 128)])
def test_gram(blocks, N):
    sm = _sm(blocks, N)
    pts = np.r_[_points(sm, "random", 12, 5), _points(sm, "vertices", 3, 6)]
    Om_d, G = sm.riesz_h10_device(pts)
    assert np.array_equal(G, G.T), "G must be symmetric to the bit"
    E = sm.evaluate_solutions(pts, Om_d)      # E[j, i] = l_i(omega_j)
    observed(f"riesz {blocks} N={N}: |G - [l_i(omega_j)]| / max|G|", np.abs(G - E.T) / np.max(np.abs(G)), 1e-12)
    G2 = sm.riesz_gram_h10(pts)
    assert np.array_equal(G2, G), "the Gram-only call must give the full call's bits"
    assert np.all(np.linalg.eigvalsh(G) > 0)


def test_repeat_poison_and_edge_sizes(monkeypatch):
    from romhighcontrast_amd import _ffi
    sm = _sm((2, 2), 32)
    pts = _points(sm, "random", 9, 7)
    O1, G1 = sm.riesz_h10_device(pts)
    O2, G2 = sm.riesz_h10_device(pts)
    assert np.array_equal(O1.numpy(), O2.numpy()) and np.array_equal(G1, G2)
    monkeypatch.setenv("ROMHC_POISON_WS", "1")
    O3, G3 = sm.riesz_h10_device(pts)
    assert np.array_equal(O1.numpy(), O3.numpy()) and np.array_equal(G1, G3)
    monkeypatch.delenv("ROMHC_POISON_WS")
    # offsets into a larger buffer: rows row0 .. row0 + m of OMEGA, nothing else written
    dim = sm.vspace_dim
    buf = sm._ctx.alloc((len(pts) + 3) * dim)
    buf.fill(7.0)
    sm._fem.riesz_h10(*sm._locate(pts), OMEGA=buf, row0=2, gram=False)
    host = buf.download((len(pts) + 3) * dim, shape=(len(pts) + 3, dim))
    assert np.all(host[:2] == 7.0) and np.all(host[-1] == 7.0)
    assert np.array_equal(host[2:-1], O1.numpy())
    # npts = 0 and 1
    O0, G0 = sm.riesz_h10_device(np.zeros((0, 2)))
    assert O0.shape == (0, dim) and G0.shape == (0, 0)
    O1p, G1p = sm.riesz_h10_device(pts[:1])
    assert G1p.shape == (1, 1) and G1p[0, 0] > 0
    assert abs(G1p[0, 0] - G1[0, 0]) <= 1e-14 * G1[0, 0]
    assert np.max(np.abs(O1p.numpy()[0] - O1.numpy()[0])) <= 1e-14 * np.max(np.abs(O1.numpy()[0]))
    # a point outside the domain raises, as evaluate_solutions does
    bad = np.array([[sm.x_domain[0] - 0.5, 0.0]])
    with pytest.raises(_ffi.RomLibraryError, match="outside the domain"):
        sm.evaluate_solutions(bad, np.zeros((1, dim)))
    with pytest.raises(_ffi.RomLibraryError, match="outside the domain"):
        sm.riesz_h10_device(bad)


# ---- PBDW --------------------------------------------------------------------------------------------------------------
_BASES = {}


def _greedy(blocks, N, n_max=20, M=200):
    from romhighcontrast_amd.lib.ReducedBasis import GREEDY_FOR_H10, ReducedBasisGreedy
    key = (tuple(blocks), N)
    if key not in _BASES:
        sm = _sm(blocks, N)
        rng = np.random.default_rng(21)
        a = 10.0 ** rng.uniform(0, 2, size=(M,) + tuple(blocks))
        U = sm.generate_solutions(a)
        rb = ReducedBasisGreedy(GREEDY_FOR_H10).build(n_max, sm, U, a, sm.H10norm(U))
        a_test = 10.0 ** rng.uniform(0, 2, size=(4,) + tuple(blocks))
        _BASES[key] = (rb, a_test, sm.generate_solutions(a_test))
    return _BASES[key]


@pytest.mark.parametrize("blocks,N", [((2, 2), 32), ((2, 2), 128)])
@pytest.mark.parametrize("m", [20, 50])
@pytest.mark.parametrize("n", [0, 1, 10, 20])
def test_pbdw_properties(blocks, N, m, n):
    from romhighcontrast_amd.lib.ReducedBasis import pbdw_state_estimation
    sm = _sm(blocks, N)
    rb, _, U = _greedy(blocks, N)
    basis = np.asarray(rb.basis)[:n]
    pts = _separated(sm, m, seed=100 + m, sep=0.18 if m == 50 else 0.3)
    Y = sm.evaluate_solutions(pts, U)                 # (K, m)
    r = pbdw_state_estimation(sm, basis, pts, Y)
    G = sm.riesz_gram_h10(pts)
    assert np.linalg.cond(G) <= 1e4
    est = r.estimates
    tag = f"pbdw {blocks} N={N} m={m} n={n}"
    # 1. interpolation
    observed(f"{tag}: max |l(u*) - y| / max|y|", np.abs(sm.evaluate_solutions(pts, est) - Y) / np.max(np.abs(Y)), 1e-10)
    # 2. optimality: u* is the interpolant closest to V_n
    un = sm.H10norm(U)
    if n:
        dist_u = sm.H10norm_diff(sm.project_solutions(U, basis), U)
        dist_s = sm.H10norm_diff(sm.project_solutions(est, basis), est)
    else:
        dist_u, dist_s = un, sm.H10norm(est)
    excess = (dist_s - dist_u * (1 + 1e-8)) / un
    observed(f"{tag}: (dist(u*, V_n) - dist(u, V_n)(1 + 1e-8)) / ||u||", excess, 1e-12)
    if n:
        L = sm.evaluate_solutions(pts, basis).T
        # (relative to the size of d, or to that of the interpolant's coefficients G^-1 y when n = m makes d vanish)
        dscale = np.linalg.norm(r.d, axis=0) + np.linalg.norm(np.linalg.solve(G, Y.T), axis=0)
        orth = np.abs(L.T @ r.d) / (np.linalg.norm(L, 2) * dscale)
        observed(f"{tag}: |L^T d| / (||L|| (||d|| + ||G^-1 y||)) (correction orthogonal to V_n)", orth, 1e-10)
    # 3. a-priori bound
    beta = r.beta[n - 1] if n else 1.0
    assert np.all(np.diff(r.beta) <= 1e-12) and (n == 0 or beta > 0)
    err = sm.H10norm_diff(est, U)
    observed(f"{tag}: ||u - u*|| / (dist(u, V_n) / beta_n) - 1", err / (dist_u / beta) - 1.0, 1e-8)
    # 4. reproduction of span V_n, and n = 0: the minimum-norm interpolant
    if n:
        coef = np.random.default_rng(n).standard_normal((3, n))
        V = coef @ basis
        rv = pbdw_state_estimation(sm, basis, pts, sm.evaluate_solutions(pts, V))
        rel = sm.H10norm_diff(rv.estimates, V) / sm.H10norm(V)
        observed(f"{tag}: reproduction of span V_n, ||v - v*|| beta_n / ||v||", rel * beta, 1e-10)
    else:
        Om, _ = sm.riesz_h10_device(pts)
        ref = np.linalg.solve(G, Y.T).T @ Om.numpy()
        rel = sm.H10norm_diff(est, ref) / sm.H10norm(ref)
        observed(f"{tag}: minimum-norm interpolant Omega^T G^-1 y", rel, 1e-10)
        assert r.beta.shape == (0,) and r.c.shape == (0, len(U))


def test_pbdw_host_restatement():
    """(2,2) N=8: SciPy representers + the dense saddle-point system, to 1e-9 relative H1_0."""
    from romhighcontrast_amd.lib.ReducedBasis import pbdw_state_estimation
    blocks, N = (2, 2), 8
    sm = _sm(blocks, N)
    rb, _, U = _greedy(blocks, N, n_max=10, M=80)
    A1 = _a1_sparse(sm)
    assert np.array_equal(A1.toarray(), sm.A_preassembled4h1_norm)
    pts = _separated(sm, 20, seed=5, sep=0.3)
    R = sm.generate_riesz(pts, "l2")
    Om = spla.spsolve(A1, R.T).T
    Gh = R @ Om.T
    Y = sm.evaluate_solutions(pts, U)
    for n in (0, 1, 5, 10):
        C = np.asarray(rb.basis)[:n]
        L = R @ C.T
        m = len(pts)
        S = np.block([[Gh, L], [L.T, np.zeros((n, n))]])
        x = np.linalg.solve(S, np.vstack([Y.T, np.zeros((n, len(U)))]))
        ref = x[:m].T @ Om + x[m:].T @ C
        got = pbdw_state_estimation(sm, C, pts, Y).estimates
        rel = _h10(sm.A_preassembled4h1_norm, got - ref) / _h10(sm.A_preassembled4h1_norm, ref)
        observed(f"pbdw (2,2) N=8 n={n}: vs SciPy representers + dense saddle point", rel, 1e-9)


def test_pbdw_api():
    from romhighcontrast_amd.lib.ReducedBasis import pbdw_state_estimation
    from romhighcontrast_amd.lib.SolutionsManagers import DeviceArray
    blocks, N = (2, 2), 32
    sm = _sm(blocks, N)
    rb, _, U = _greedy(blocks, N)
    sub = rb[:10]
    pts = _separated(sm, 20, seed=120, sep=0.3)
    Y = sm.evaluate_solutions(pts, U)
    r1 = pbdw_state_estimation(sm, np.asarray(sub.basis), pts, Y)
    Cd = DeviceArray(sm._ctx.upload(np.ascontiguousarray(sub.basis)), 10, sm.vspace_dim)
    r2 = pbdw_state_estimation(sm, Cd, pts, Y, device=True)
    assert isinstance(r2.estimates, DeviceArray)
    assert np.array_equal(r1.estimates, r2.estimates.numpy())
    assert np.array_equal(r1.c, r2.c) and np.array_equal(r1.d, r2.d) and np.array_equal(r1.beta, r2.beta)
    c, est = sub.state_estimation_pbdw(sm, pts, Y, return_coefs=True)
    assert c.shape == (10, len(U)) and np.array_equal(est, r1.estimates)
    assert np.array_equal(sub.state_estimation_pbdw(sm, pts, Y), est)
    assert sub.parameter_estimation_inverse(c).shape == (len(U),) + tuple(blocks)
    assert sub.parameter_estimation_linear(c).shape == (len(U),) + tuple(blocks)
    beta = rb.pbdw_stability(sm, pts)
    assert beta.shape == (rb.dim,) and np.allclose(beta[:10], r1.beta, rtol=1e-10, atol=0)
    with pytest.raises(ValueError, match="n = 20 > m = 12"):
        rb.state_estimation_pbdw(sm, pts[:12], Y[:, :12])
    dup = np.r_[pts[:8], pts[3:4]]
    with pytest.raises(ValueError, match=r"points \[3, 8\]"):
        sub[:2].state_estimation_pbdw(sm, dup, sm.evaluate_solutions(dup, U))
