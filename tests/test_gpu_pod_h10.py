"""rom_sine_transform, rom_pod_h10 and rom_pod_h10_factored (csrc/rom_spectral.hip, csrc/rom_factored.hip) on the device.

Notation: C = 64, eps = 2^-53, kappa = sqrt(lam_max / lam_min) of the grid (tests/h10_truth.py: the long-double tables, the
long-double transform, the crafted blocks; tests/test_pod_h10_host.py proves the truth against LAPACK and shows a plain fp64
NumPy pipeline inside every bound used here).

1. The transform against the long-double one, on the four grids of h10_truth.GRIDS (7 x 7: below one MFMA tile; 15 x 23:
   nr != nc; 31 x 31; 71 x 47: across a 64-row tile, two row tiles in grid.y), K in {1, 5, 70}, every (pre, post) pair the POD
   uses and the two of A_1^-1, NaN rows around X and OUT.  Per row ||OUT_i - truth||_2 <= C eps (nr + nc) ||Lambda^(pre/2) o
   X_i||_2 max Lambda^(post/2) -- a fraction of the rigorous gamma_(nr + nc) bound of the two products, which carries the
   factor sqrt(nr nc) more.  Round trip (0,1), (-1,0): back at X within the sum of the two bounds, bound(0,1)(X) +
   bound(-1,0)(W).  (0,-2), (0,0) of the P1 evaluation
   vectors r_i against generate_riesz_h10: both are A_1^-1 r_i by two sine transforms, each within b = bound(0,-2)(r_i) +
   bound(0,0)(Lambda^-1 o r_i hat), so they differ by at most 2 b.  Same bits on a repeated call and with ROMHC_POISON_WS.
2. rom_pod_h10 on crafted blocks with an exactly known H^1_0 SVD (h10_truth.POD_CASES: 15 x 23 and 71 x 47; a fast spectrum,
   one down to 1e-12 with a request past the rank, a centred one with a mean row, one with a caller's rel_floor = 1e-4): the assertions of
   tests/test_gpu_pod_routes.py::check_truth in the H^1_0 geometry (h10_truth.check_pod_h10):
     |sigma_i - s_i| <= C eps kappa s_1 + rel_i (same rel_i and Gram-route term);  H^1_0 angle to the true mode <= C eps kappa
     s_1 / gap_i + C eps kappa (+ Gram term);  |V A_1 V^T - I| <= 1e-13 + C eps kappa through the long-double 5-point stencil;
     svd_flip sign on the returned rows;  resolved / completed / stop_reason;  completed rows with sigma = 0 and ||X_c v|| in
     H^1_0 coordinates <= floor s_1 + C eps kappa s_1;  X bit-identical after the call, all sentinels untouched;  the same bits
     on a repeated call and with a poisoned workspace.
3. Sweep blocks: rom_pod_h10 on the expanded rows, rom_pod_h10_factored on the interface vectors, LAPACK on the long-double-
   transformed rows.  Rows: the bounds of 2, Gram-route terms included when the call reports a Gram pass.  Factored: tol =
   delta + C eps kappa s_1 with delta^2 = (C Kc eps + (Kc - k1) 1e-14) sum_m ||D y_m||^2, D = the H^1_0 norms of the expanded compact unit vectors, k1 = the rank of the H^1_0 map (derived as in
   test_pod_factored_vs_lapack_and_rows: the map drops the Schur complement below 1e-14 of the equilibrated form and carries
   its factorisation rounding; Weyl for the values, Wedin for the modes).  A mode the call completed must have a LAPACK value
   below the floor: s_i <= 1e-13 s_1 + tol.  Grids: (2,2)/16, the tile-crossing 71 x 47 and 79 x 79 ((2,2)/40: where a geometry
   has no factored form -- rom_fem_expansion_is_linear = 0 -- the factored call must refuse it and the rows are still checked),
   and (1,1)/8 with n > k1.
4. Optimality in the project's own metric: on the (2,2)/16 sweep block, uncentred, sum_m proj_n(m)^2 of sm.error_curves on the
   H^1_0-POD basis = sum_{i>n} sigma_i^2 for every n <= 20, and <= the same sum for the Euclidean PCA basis and the H^1_0
   greedy basis.  Tolerance: C eps kappa sum sigma_i^2, plus the curve's own bar -- DESIGN 5.3: an error is accurate to 6.1e-14
   of its snapshot's norm, d_m = 6.1e-14 ||u_m||, so a sum of squares moves by sum_m (2 proj_n(m) d_m + d_m^2).  And the
   drop-in class: ReducedBasisPCA(False, inner_product="h10") on a host array, a generate_solutions_device block and a
   FactoredSnapshots span the same space within 3's bound; inner_product="l2" is the default, bit for bit.
"""
import numpy as np
import pytest

from conftest import observed
import h10_truth as ht

pytestmark = pytest.mark.gpu

EPS, C = ht.EPS, ht.C
PC_TOL = 1e-14
_SM = {}


def _sm(blocks, N):
    from src.lib import SolutionsManagers as SM
    if (blocks, N) not in _SM:
        _SM[(blocks, N)] = SM.SolutionsManagerFEM(blocks, N)
    return _SM[(blocks, N)]


def _same_bits(a, b):
    return np.array_equal(np.asarray(a).view(np.uint64), np.asarray(b).view(np.uint64))


def _sentinel(X, before, after=2):
    dim = X.shape[1]
    return np.vstack((np.full((before, dim), np.nan), X, np.full((after, dim), np.nan)))


def _rownorm(D):
    return np.asarray(np.sqrt(np.sum(np.asarray(D) ** 2, axis=1)), dtype=np.float64)


# ---- 1. the transform ------------------------------------------------------------------------------------------------
def _transform(sm, Xb, K, pre, post, x0, o0):
    dim = sm.vspace_dim
    Ob = sm._ctx.alloc((o0 + K + 2) * dim).fill(np.nan)
    sm._fem.sine_transform(Xb, K, Ob, pre=pre, post=post, x_row0=x0, out_row0=o0)
    return Ob


@pytest.mark.parametrize("blocks,N", ht.GRIDS, ids=[f"{b[0]}x{b[1]}_N{N}" for b, N in ht.GRIDS])
def test_sine_transform_against_long_double(blocks, N, monkeypatch):
    sm, gr = _sm(blocks, N), ht.grid(blocks, N)
    ctx, dim = sm._ctx, sm.vspace_dim
    assert (sm.nr_inner_vertices, sm.nc_inner_vertices, dim) == (gr.nr, gr.nc, gr.dim)
    Kmax, x0, o0 = 70, 2, 3
    X = ht.transform_rows(gr, Kmax, seed=gr.dim)
    Xs = _sentinel(X, x0)
    Xb = ctx.upload(Xs)
    tag = f"sine transform {gr.nr}x{gr.nc}"
    for pre, post in ht.PAIRS:
        truth = gr.transform(X, pre, post)
        bound = gr.transform_bound(X, pre, post)
        for K in (1, 5, 70):
            Ob = _transform(sm, Xb, K, pre, post, x0, o0)
            O = Ob.download(shape=(o0 + K + 2, dim))
            assert np.isnan(O[:o0]).all() and np.isnan(O[o0 + K:]).all(), (tag, "OUT sentinels")
            observed(f"{tag} K={K} (pre, post) = ({pre}, {post}): row error / (C eps (nr + nc) |L^(pre/2) o X| max L^(post/2))",
                     _rownorm(O[o0:o0 + K] - truth[:K]) / bound[:K], 1.0)
            if K == 70:   # the same bits again, and with the workspace poisoned
                assert _transform(sm, Xb, K, pre, post, x0, o0).same_bits_as(Ob, Ob.n), (tag, "repeat")
                monkeypatch.setenv("ROMHC_POISON_WS", "1")
                Op = _transform(sm, Xb, K, pre, post, x0, o0)
                monkeypatch.delenv("ROMHC_POISON_WS")
                assert Op.same_bits_as(Ob, Ob.n), (tag, "poisoned workspace")
    assert _same_bits(Xb.download(shape=Xs.shape), Xs), (tag, "X modified")
    # round trip (0,1) then (-1,0)
    Wb = _transform(sm, Xb, Kmax, 0, 1, x0, 0)
    Bb = _transform(sm, Wb, Kmax, -1, 0, 0, 0)
    back = Bb.download(Kmax * dim, shape=(Kmax, dim))
    W = Wb.download(Kmax * dim, shape=(Kmax, dim))
    observed(f"{tag}: round trip (0,1), (-1,0) / (bound(0,1) + bound(-1,0))", _rownorm(back - X) / ht.round_trip_bound(gr, X, W), 1.0)
    # A_1^-1 of dense rows against the Riesz representers of the points whose rows they are
    pts = ht.riesz_points(gr)
    R = sm.generate_riesz(pts, "l2")
    assert R.shape == (3, dim) and np.all(np.abs(R).sum(axis=1) > 0)
    Rb = ctx.upload(R)
    Zb = _transform(sm, Rb, 3, 0, -2, 0, 0)
    Z = Zb.download(3 * dim, shape=(3, dim))
    Om = _transform(sm, Zb, 3, 0, 0, 0, 0).download(3 * dim, shape=(3, dim))
    b = ht.riesz_bound(gr, R, Z)
    observed(f"{tag}: (0,-2), (0,0) of evaluation vectors vs generate_riesz_h10 / 2 (bound(0,-2) + bound(0,0))",
             _rownorm(Om - sm.generate_riesz_h10(pts)) / (2 * b), 1.0)
    # argument checks: ranges, exponents, aliasing
    from romhighcontrast_amd import _ffi
    for kw in (dict(pre=3), dict(post=-3), dict(x_row0=x0 + 3), dict(out_row0=-1)):
        with pytest.raises(_ffi.RomLibraryError):
            sm._fem.sine_transform(Xb, Kmax, ctx.alloc(Kmax * dim), **kw)
    with pytest.raises(_ffi.RomLibraryError):
        sm._fem.sine_transform(Xb, 4, Xb, x_row0=0, out_row0=2)


def test_sine_transform_in_row_chunks_under_a_workspace_limit():
    """A workspace limit below the block: the transform runs in row chunks (here one row at a time) with the same bits."""
    sm, gr = _sm((2, 3), 8), ht.grid((2, 3), 8)
    ctx, dim = sm._ctx, sm.vspace_dim
    Xb = ctx.upload(ht.transform_rows(gr, 5, seed=11))
    want = _transform(sm, Xb, 5, 0, 1, 0, 0)
    ctx.set_workspace_limit(dim * 8 + 8)
    try:
        got = _transform(sm, Xb, 5, 0, 1, 0, 0)
        got2 = _transform(sm, Xb, 5, -1, 2, 0, 0)
    finally:
        ctx.set_workspace_limit(24 << 30)
    assert got.same_bits_as(want, want.n)
    assert got2.same_bits_as(_transform(sm, Xb, 5, -1, 2, 0, 0), want.n)   # (the elementwise pass of pre != 0, post != 0)
    truth = gr.transform(ht.transform_rows(gr, 5, seed=11), -1, 2)
    observed("sine transform 15x23 (pre, post) = (-1, 2): row error / bound",
             _rownorm(got2.download(5 * dim, shape=(5, dim)) - truth) / gr.transform_bound(ht.transform_rows(gr, 5, seed=11), -1, 2), 1.0)


# ---- 2. rom_pod_h10 on crafted blocks ----------------------------------------------------------------------------------
def _run_pod(sm, case, tr, Xs):
    ctx, dim, n, v0 = sm._ctx, sm.vspace_dim, case["n"], case["v_row0"]
    Xb = ctx.upload(Xs)
    Vb = ctx.alloc((v0 + n + 2) * dim).fill(np.nan)
    sig, info = sm._fem.pod_h10(Xb, tr.M, n, Vb, center=case["center"], x_row0=case["x_row0"], v_row0=v0,
                                rel_floor=case["rel_floor"])
    return sig, info, Vb, Xb


@pytest.mark.parametrize("case", ht.POD_CASES, ids=[c["id"] for c in ht.POD_CASES])
def test_pod_h10_on_crafted_blocks(case, monkeypatch):
    sm = _sm(case["blocks"], case["N"])
    tr = ht.pod_truth(case)
    n, dim, v0 = case["n"], sm.vspace_dim, case["v_row0"]
    Xs = _sentinel(tr.U, case["x_row0"])
    sig, info, Vb, Xb = _run_pod(sm, case, tr, Xs)
    print(f"{case['id']}: {info}")
    Vall = Vb.download(shape=(v0 + n + 2, dim))
    assert np.isnan(Vall[:v0]).all() and np.isnan(Vall[v0 + n:]).all(), (case["id"], "mode sentinels")
    assert _same_bits(Xb.download(shape=Xs.shape), Xs), (case["id"], "X modified")
    assert info["executed_flops"] > 0 and info["useful_flops"] > 0
    ht.check_pod_h10(case, tr, sig, info, Vall[v0:v0 + n], observed)
    sig2, info2, Vb2, _ = _run_pod(sm, case, tr, Xs)
    assert _same_bits(sig2, sig) and Vb2.same_bits_as(Vb, Vb.n) and info2 == info, (case["id"], "repeat")
    monkeypatch.setenv("ROMHC_POISON_WS", "1")
    sig3, info3, Vb3, _ = _run_pod(sm, case, tr, Xs)
    monkeypatch.delenv("ROMHC_POISON_WS")
    assert _same_bits(sig3, sig) and Vb3.same_bits_as(Vb, Vb.n) and info3 == info, (case["id"], "poisoned workspace")


def test_pod_h10_argument_checks_and_bad_input():
    from romhighcontrast_amd import _ffi
    from src.lib import ReducedBasis as RB
    from src.lib.SolutionsManagers import DeviceArray
    sm = _sm((1, 1), 8)
    ctx, fem, dim = sm._ctx, sm._fem, sm.vspace_dim
    X = np.random.default_rng(5).standard_normal((6, dim))
    Xb, Vb = ctx.upload(X), ctx.alloc(6 * dim)
    for kw in (dict(M=6, n=7), dict(M=7, n=2), dict(M=6, n=2, x_row0=1), dict(M=6, n=6, v_row0=1), dict(M=0, n=0),
               dict(M=6, n=-1)):
        with pytest.raises(_ffi.RomLibraryError):
            fem.pod_h10(Xb, kw["M"], kw["n"], Vb, x_row0=kw.get("x_row0", 0), v_row0=kw.get("v_row0", 0))
    sig, info = fem.pod_h10(Xb, 6, 0, Vb)      # n = 0: nothing to do, nothing written
    assert sig.size == 0 and info["resolved_modes"] == 0
    bad = X.copy()
    bad[3, 7] = np.nan
    with pytest.raises(ValueError, match="NaN / Inf"):
        RB.pod_modes_h10(sm, DeviceArray(ctx.upload(bad), 6, dim), 2)
    bad[3, 7] = np.inf
    with pytest.raises(ValueError, match="NaN / Inf"):
        RB.pod_modes_h10(sm, DeviceArray(ctx.upload(bad), 6, dim), 2)


# ---- 3. sweep blocks: rows, factored, LAPACK ---------------------------------------------------------------------------
_SWEEPS = {}


def _sweep(blocks, N, M):
    """(fs, rows U (M, dim), compact vectors (M, Kc), parameters a (M, kblk)) of a seeded sweep; computed once, not modified.
    fs and the compact vectors are None on a geometry whose expansion is not a linear map of the interface vectors."""
    key = (blocks, N, M)
    if key not in _SWEEPS:
        sm = _sm(blocks, N)
        a = 10.0 ** np.random.default_rng(M * 3 + N).uniform(0, 2, size=(M, blocks[0] * blocks[1]))
        Ud = sm.generate_solutions_device(a.reshape(M, *blocks))
        fs = Ud.factored
        assert (fs is not None) == sm._fem.expansion_is_linear
        Ych = fs.Yc.download(M * fs.map.Kc, shape=(M, fs.map.Kc)) if fs is not None else None
        _SWEEPS[key] = (fs, Ud.numpy(), Ych, a)
    return _SWEEPS[key]


def _h10_equilibration2(sm, gr, Kc):
    """d_i^2 = ||expansion of compact unit vector i||^2_{H^1_0} (long-double stencil)."""
    from romhighcontrast_amd import factored
    em = factored.expansion_map(sm)
    B = sm._ctx.alloc(Kc * em.dim)
    em.expand_compact(sm._ctx.upload(np.eye(Kc)), Kc, B)
    E = gr.energy(B.download(Kc * em.dim, shape=(Kc, em.dim)))
    return np.asarray(np.sum(E * E, axis=1), dtype=np.float64)


def _lapack_h10(gr, U, center):
    """LAPACK on the long-double-transformed rows: (s, Q^T) with Q^T the modes in energy coordinates."""
    W = gr.transform(U, 0, 1)
    if center:
        W = W - W.mean(axis=0)
    _, s, Qt = np.linalg.svd(np.asarray(W, dtype=np.float64), full_matrices=False)
    return s, Qt


def _factored_tol(sm, gr, Ych, center, k1, s1):
    Kc = Ych.shape[1]
    Yu = Ych - Ych.mean(axis=0) if center else Ych
    d2 = _h10_equilibration2(sm, gr, Kc)
    delta = np.sqrt((C * Kc * EPS + max(Kc - k1, 0) * PC_TOL) * float(np.sum(Yu ** 2 @ d2)))
    return delta + C * EPS * gr.kappa * s1, delta


def _check_against_lapack(tag, gr, sig, info, V, s_ref, Qt, tol, rel_pod):
    """Values, completed modes, H^1_0 angles of the clearly resolved modes, A_1-orthonormality, sign rule."""
    n, s1 = len(sig), s_ref[0]
    s_n = np.concatenate([s_ref, np.zeros(n)])[:n]
    k = info["resolved_modes"]
    assert info["completed_modes"] == n - k and np.all(sig[k:] == 0.0), (tag, info)
    rel = (np.where(s_n >= 1e-6 * s1, 1e-10, 1e-5) * s_n) if rel_pod else 0.0 * s_n
    gram = info["gram_passes"] > 0       # check_truth's Gram-route terms: |sigma^2 - s^2| <= 2e-14 s_1^2 (Bauer-Fike)
    if gram:
        rel = rel + 1e-14 * s1 ** 2 / np.maximum(s_n, 1e-300)
    if k:
        observed(f"{tag}: |sigma - LAPACK| / (tol + rel), tol / s_1 = {tol / s1:.1e}", np.abs(sig[:k] - s_n[:k]) / (tol + rel[:k]), 1.0)
    if k < n:
        observed(f"{tag}: LAPACK's values of the completed modes / (1e-13 s_1 + tol)", s_n[k:] / (1e-13 * s1 + tol), 1.0)
    G = np.asarray(gr.a1_dots(V, V), dtype=np.float64)
    observed(f"{tag}: |V A_1 V^T - I| (long-double stencil)", np.abs(G - np.eye(n)), 1e-13 + C * EPS * gr.kappa)
    piv = np.argmax(np.abs(V), axis=1)
    assert np.all(V[np.arange(n), piv] > 0), (tag, "svd_flip sign convention")
    rank = int(np.sum(s_n[:k] > 1e3 * tol))
    Q = np.asarray(gr.transform(V[:rank], 0, 1), dtype=np.float64)
    s_all = np.concatenate([s_ref, [0.0]])
    ang = []
    for i in range(rank):
        gap = np.min(np.abs(np.delete(s_all, i) - s_all[i]))
        gap2 = np.min(np.abs(np.delete(s_all, i) ** 2 - s_all[i] ** 2))
        c = Q[i] @ Qt[i]
        ang.append(np.linalg.norm(Q[i] - c * Qt[i]) / ((tol + rel[i]) / gap + C * EPS * gr.kappa + (2e-14 * s1 ** 2 / gap2 if gram else 0.0)))
    if ang:
        observed(f"{tag}: H10 mode angle vs LAPACK / ((tol + rel) / gap [+ Gram term] + C eps kappa), {rank} modes", np.array(ang), 1.0)
    return rank


@pytest.mark.parametrize("blocks,N,M,n,center,c_row0,v_row0,claim", [
    ((2, 2), 16, 60, 40, False, 3, 2, ""),
    ((2, 2), 16, 60, 40, True, 0, 0, ""),
    ((3, 2), 24, 64, 48, True, 1, 3, ""),
    ((2, 2), 40, 64, 48, True, 2, 1, ""),        # 79 x 79: the other tile-crossing grid, with a factored form at any rate
    ((1, 1), 8, 40, 6, True, 0, 1, "n>k1"),      # one block: the snapshot manifold is a line; completion past the map's rank
])
def test_pod_h10_rows_vs_factored_vs_lapack(blocks, N, M, n, center, c_row0, v_row0, claim):
    sm, gr = _sm(blocks, N), ht.grid(blocks, N)
    ctx, fem, dim = sm._ctx, sm._fem, sm.vspace_dim
    fs, U, Ych, _ = _sweep(blocks, N, M)
    s_ref, Qt = _lapack_h10(gr, U, center)
    s1 = s_ref[0]
    tag = f"pod_h10 {blocks}/{N} M={M} n={n} centre={center}"
    # rows
    Us = _sentinel(U, 2)
    Ub = ctx.upload(Us)
    Vr = ctx.alloc((v_row0 + n + 2) * dim).fill(np.nan)
    sig_r, info_r = fem.pod_h10(Ub, M, n, Vr, center=center, x_row0=2, v_row0=v_row0)
    Vra = Vr.download(shape=(v_row0 + n + 2, dim))
    assert np.isnan(Vra[:v_row0]).all() and np.isnan(Vra[v_row0 + n:]).all() and _same_bits(Ub.download(shape=Us.shape), Us)
    tol_r = C * EPS * gr.kappa * s1
    _check_against_lapack(f"{tag} rows", gr, sig_r, info_r, Vra[v_row0:v_row0 + n], s_ref, Qt, tol_r, True)
    # factored
    if fs is None:
        # no factored form on this geometry (some edges are recovered node by node): the call says so, as rom_pod_factored does
        from romhighcontrast_amd import _ffi
        assert claim == ""
        with pytest.raises(_ffi.RomLibraryError, match="not a linear map"):
            fem.pod_h10_factored(ctx.alloc(M), M, n, ctx.alloc(n * dim), center=center)
        return
    Kc = fs.map.Kc
    k1, _ = fem.energy_map(1)
    assert k1 >= 1 and (n > k1 if claim == "n>k1" else True), (claim, k1)
    Ys = _sentinel(Ych, c_row0)
    Yb = ctx.upload(Ys)
    Vf = ctx.alloc((v_row0 + n + 2) * dim).fill(np.nan)
    sig_f, info_f = fem.pod_h10_factored(Yb, M, n, Vf, center=center, c_row0=c_row0, v_row0=v_row0)
    Vfa = Vf.download(shape=(v_row0 + n + 2, dim))
    assert np.isnan(Vfa[:v_row0]).all() and np.isnan(Vfa[v_row0 + n:]).all(), "mode sentinels"
    assert _same_bits(Yb.download(shape=Ys.shape), Ys), "interface vectors modified"
    assert info_f["completed_modes"] >= n - min(n, k1, M), (info_f, k1)
    tol_f, delta = _factored_tol(sm, gr, Ych, center, k1, s1)
    print(f"{tag}: Kc {Kc}, k1 {k1}, delta / s_1 {delta / s1:.2e}; rows {info_r}; factored {info_f}")
    _check_against_lapack(f"{tag} factored (Kc {Kc}, k1 {k1})", gr, sig_f, info_f, Vfa[v_row0:v_row0 + n], s_ref, Qt, tol_f, True)
    kk = min(info_r["resolved_modes"], info_f["resolved_modes"])
    if kk:
        s_n = s_ref[:kk]
        rel = np.where(s_n >= 1e-6 * s1, 1e-10, 1e-5) * s_n
        ng = int(info_r["gram_passes"] > 0) + int(info_f["gram_passes"] > 0)
        observed(f"{tag}: |sigma factored - sigma rows| / (tol_f + tol_r + 2 rel [+ Gram terms])",
                 np.abs(sig_f[:kk] - sig_r[:kk]) / (tol_f + tol_r + 2 * rel + ng * 1e-14 * s1 ** 2 / s_n), 1.0)
    Vf2 = ctx.alloc((v_row0 + n + 2) * dim).fill(np.nan)
    sig_f2, info_f2 = fem.pod_h10_factored(Yb, M, n, Vf2, center=center, c_row0=c_row0, v_row0=v_row0)
    assert _same_bits(sig_f2, sig_f) and Vf2.same_bits_as(Vf, Vf.n) and info_f2 == info_f, "repeat"


# ---- 4. optimality in the project's own metric, and the drop-in class ---------------------------------------------------
def test_h10_pod_is_the_lower_envelope_of_the_error_curves():
    from src.lib import ReducedBasis as RB
    from src.lib.SolutionsManagers import DeviceArray
    blocks, N, M, nmax = (2, 2), 16, 60, 20
    sm, gr = _sm(blocks, N), ht.grid(blocks, N)
    ctx, dim = sm._ctx, sm.vspace_dim
    _, U, _, a = _sweep(blocks, N, M)
    a3 = a.reshape(M, *blocks)
    Ud = DeviceArray(ctx.upload(U), M, dim)
    modes, sig = RB.pod_modes_h10(sm, Ud, M, center=False)           # the whole spectrum (values below the floor: 0)
    assert _same_bits(Ud.numpy(), U) and Ud.factored is None
    total = float(np.sum(sig ** 2))
    tails = np.array([np.sum(sig[k:] ** 2) for k in range(nmax + 1)])

    def curve_sums(basis):
        proj = sm.error_curves(U, np.asarray(basis)[:nmax])[0]       # (nmax + 1, M), absolute H^1_0 errors
        d = 6.1e-14 * proj[0]
        return np.sum(proj ** 2, axis=1), C * EPS * gr.kappa * total + np.sum(2 * proj * d + d * d, axis=1)

    mine, tol = curve_sums(modes)
    observed("H10-POD: |sum_m proj_n(m)^2 - sum_{i>n} sigma_i^2| / (C eps kappa sum sigma^2 + the curve's bar), n <= 20",
             np.abs(mine - tails) / tol, 1.0)
    pca = RB.ReducedBasisPCA(add_inf_solutions=False).build(nmax, sm, U.copy(), a3, 1)
    other, tol_o = curve_sums(pca.basis)
    observed("H10-POD against the Euclidean PCA basis: (own sum - other sum) / tolerance, n <= 20", (mine - other) / (tol + tol_o), 1.0)
    assert np.any(other[1:] > mine[1:] + tol[1:] + tol_o[1:]), "the Euclidean PCA is not H^1_0-optimal on this block: the test must see it"
    greedy = RB.ReducedBasisGreedy(RB.GREEDY_FOR_H10).build(nmax, sm, U.copy(), a3, sm.H10norm(U))
    other, tol_o = curve_sums(greedy.basis)
    observed("H10-POD against the H^1_0 greedy basis: (own sum - other sum) / tolerance, n <= 20", (mine - other) / (tol + tol_o), 1.0)


def test_reduced_basis_pca_h10_on_the_three_kinds_of_block():
    from src.lib import ReducedBasis as RB
    blocks, N, M, n = (2, 2), 16, 60, 8
    sm, gr = _sm(blocks, N), ht.grid(blocks, N)
    fs, U, Ych, a = _sweep(blocks, N, M)
    a3 = a.reshape(M, *blocks)
    k1, _ = sm._fem.energy_map(1)
    s_ref, Qt = _lapack_h10(gr, U, True)
    tol_f, _ = _factored_tol(sm, gr, Ych, True, k1, s_ref[0])
    host = RB.ReducedBasisPCA(False, inner_product="h10").build(n, sm, U.copy(), a3, 1)
    Ud = sm.generate_solutions_device(a3)
    assert Ud.factored is not None
    dev = RB.ReducedBasisPCA(False, inner_product="h10").build(n, sm, Ud, a3, 1)
    fac = RB.ReducedBasisPCA(False, inner_product="h10").build(n, sm, fs, a3, 1)
    assert host.name == fac.name == "PCA $H^1_0$"
    gap = s_ref[n - 1] - s_ref[n]
    assert s_ref[n - 1] > 1e3 * tol_f and gap > 1e3 * tol_f, "the leading n modes are clearly resolved and separated"
    Qs = [np.asarray(gr.transform(np.asarray(b.basis), 0, 1), dtype=np.float64) for b in (host, dev, fac)]
    for b, Q in zip((host, dev, fac), Qs):
        assert np.asarray(b.basis).shape == (n, sm.vspace_dim)
        observed("ReducedBasisPCA h10: |sigma - LAPACK| / (tol + rel)", np.abs(b.singular_values_ - s_ref[:n]) / (tol_f + 1e-10 * s_ref[:n]), 1.0)
        observed("ReducedBasisPCA h10: distance of the span from LAPACK's / (tol / gap_n + C eps kappa)",
                 np.linalg.norm(Q - (Q @ Qt[:n].T) @ Qt[:n], 2) / (tol_f / gap + C * EPS * gr.kappa), 1.0)
    for name, Q in (("device block", Qs[1]), ("FactoredSnapshots", Qs[2])):
        observed(f"ReducedBasisPCA h10: span of the host-array build vs the {name} build / (2 tol / gap_n + C eps kappa)",
                 np.linalg.norm(Qs[0] - (Qs[0] @ Q.T) @ Q, 2) / (2 * tol_f / gap + C * EPS * gr.kappa), 1.0)
    # the default is the Euclidean PCA, bit for bit, under either spelling
    d0 = RB.ReducedBasisPCA(False).build(n, sm, U.copy(), a3, 1)
    d1 = RB.ReducedBasisPCA(False, inner_product="l2").build(n, sm, U.copy(), a3, 1)
    assert d0.name == d1.name == "PCA" and _same_bits(d0.basis, d1.basis) and _same_bits(d0.singular_values_, d1.singular_values_)
    observed("ReducedBasisPCA default: Euclidean orthonormality", np.abs(d0.basis @ d0.basis.T - np.eye(n)), 1e-13)
