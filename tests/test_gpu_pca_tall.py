"""rom_pca_tall (csrc/rom_pca_tall.hip) against blocks whose SVD is known exactly (tests/referee.py: ExactSVD), against LAPACK
on the reference's own 25,000 x 81 block (src/experiments/NonLinearROM.py:24-41), against rom_pod where both apply, and
the contract of the C entry.  C = 64, eps = 2^-53 as in test_gpu_pod_routes.py.

Bounds on an exact block (s: true values, descending; r of them, all >= 1e-10 s_1 before their rounding to dyadic
mantissas and > 1e-11 s_1 after it, so every one of them is compared):
  * |sigma_i - s_i| <= C eps s_1 + M eps s_i.  The second term is the worst-case bound gamma_M of a dot product of length M
    in ANY summation order: rigorous, and independent of how the code under test chunks its sums;
  * sin(angle of mode i to the true mode) <= (C eps s_1 + M eps s_i) / gap_i + C eps, gap_i = distance to the nearest other
    singular value (zero included when r < dim), the sine from the residual v - (v . t) t; a cluster of equal values is
    compared through its projector, with the cluster's gap;
  * score column i against +- s_i u_i in the 2-norm: s_i x that angle bound + the sigma bound.  Columns of a cluster are
    compared with Xc v_i formed from the exact factors and the returned v_i: both sides carry at most gamma_dim ||Xc||_F;
  * sigma_i is the measured norm of score column i, also below the floor: within gamma_M of the column's norm in long double;
  * ||V V^T - I||_max <= 1e-13, svd_flip signs, NaN sentinel rows around X, V and S untouched, the centred block and the
    mean exact (every partial sum of an ExactSVD block is exact in any order);
  * info: resolved = min(r, n), stop reason 0, passes <= 4 (three in exact arithmetic: two decompositions and the measuring
    pass; one more is allowed for a different summation order -- here it is the pass that re-measures after the modes at
    noise level were sorted);
  * the same bits on a second call and under ROMHC_POISON_WS.
The relative-accuracy property of the device Jacobi that the method rests on is tested first, on graded matrices of order
81 (one workgroup, LDS) and 300 (grid-wide) against an 80-bit Jacobi.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import observed, rel_h10
import referee as rf

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -53
C = 64.0
LD = np.longdouble


def _mant(values, M):
    v = np.asarray(values, dtype=np.float64)
    e = int(np.floor(52 - np.log2(M * v.sum()))) - 1
    m = np.round(v * 2.0 ** e).astype(np.int64)
    assert m.min() >= 1
    return m, e


def _geo(r, lo):
    return 10.0 ** -np.linspace(0, lo, r)


def _case(cid, M, D, dim, values, n=None, mean=False, x_row0=3, v_row0=2, s_row0=1, pad=0):
    """pad: zero rows past the M rows of the exact block (uncentred cases only): the device call sees M + pad rows."""
    return dict(id=cid, M=M, D=D, dim=dim, values=np.asarray(values, dtype=np.float64), n=dim if n is None else n, mean=mean,
                x_row0=x_row0, v_row0=v_row0, s_row0=s_row0, pad=pad)


CASES = [
    _case("t81_ten_orders", 16384, 64, 81, _geo(40, 10), mean=True),
    _case("t64_full_rank", 16384, 64, 64, _geo(63, 6), mean=True),
    _case("t300_unfused", 65536, 256, 300, _geo(120, 4)),
    _case("t1024_limit", 4096, 1024, 1024, _geo(100, 6), mean=True),
    _case("wide_64x256", 64, 256, 256, _geo(40, 8)),
    _case("t96_cluster", 4096, 64, 96, np.concatenate([_geo(10, 1), np.full(20, 1e-3)]), mean=True),
    _case("t81_n10", 16384, 64, 81, _geo(40, 10), n=10, mean=True),
    # the smallest shapes at which the slab engine (csrc/rom_slab.h) can go wrong: 16-column tiles, 32-row slabs, chunks of slabs
    _case("d1", 4, 1, 1, _geo(1, 0)),                               # one tile, one mode
    _case("d15_33rows", 32, 8, 15, _geo(6, 3), pad=1),              # a partial tile; a second slab of one row
    _case("d16", 16, 16, 16, _geo(12, 4)),                          # exactly one tile; half a slab
    _case("d17_31rows", 16, 16, 17, _geo(10, 4), pad=15),           # two column tiles, the second one column wide; 31 rows
    _case("d65", 64, 64, 65, _geo(40, 6)),                          # five column tiles: a second NT tile for one wave pair only
    _case("d80_8193", 8192, 32, 80, _geo(30, 6), pad=1),            # two slabs per chunk on 256 CUs; the last chunk: one row
    _case("d96_1025", 1024, 64, 96, _geo(50, 6), pad=1),            # the fused limit with a one-row last slab
]


def _truth(case):
    mant, e = _mant(case["values"], case["M"])
    mi = (np.random.default_rng(5).integers(-mant[0], mant[0], size=case["dim"]) // 4) if case["mean"] else None
    return rf.ExactSVD(case["M"], case["D"], case["dim"], mant, e, seed=1, mean_int=mi, pad=case["pad"])


def _sentinel_block(X, before, after=2):
    return np.vstack((np.full((before, X.shape[1]), np.nan), X, np.full((after, X.shape[1]), np.nan)))


def run_tall(ctx, case, t):
    """One device call with NaN rows around X, V and S.  Returns sigma, info and the four buffers."""
    M, dim, n = t.rows, t.dim, case["n"]
    x0, v0, s0 = case["x_row0"], case["v_row0"], case["s_row0"]
    Xb = ctx.upload(_sentinel_block(t.X, x0))
    Vb = ctx.alloc((v0 + n + 2) * dim).fill(np.nan)
    Sb = ctx.alloc((s0 + M + 2) * n).fill(np.nan)
    mb = ctx.alloc(dim + 1).fill(np.nan)
    sig, info = ctx.pca_tall(Xb, M, dim, n, Vb, S=Sb, mean=mb, center=case["mean"], x_row0=x0, v_row0=v0, s_row0=s0)
    return sig, info, Xb, Vb, Sb, mb


def _same_bits(a, b):
    return np.array_equal(np.asarray(a).view(np.uint64), np.asarray(b).view(np.uint64))


def check_truth(case, t, sig, info, V, S):
    cid, n, M, dim = case["id"], case["n"], t.M, t.dim    # (M: the rows that carry the block -- zero rows add nothing to a sum)
    s, r = t.s, t.r
    s1 = s[0]
    assert s.min() > 100 * 1e-13 * s1        # (every true value clearly above the noise floor: resolved = r)
    k = min(r, n)
    print(f"{cid}: {info}  tail sigma / s_1 = {(sig[k:].max() / s1) if n > k else 0.0:.2e}")
    assert info["resolved_modes"] == k, (cid, info, sig[k:k + 3] / s1)
    assert info["stop_reason"] == "converged" and info["passes"] <= 4, (cid, info)
    assert np.all(np.diff(sig) <= 0), (cid, "descending")
    sbound = C * EPS * s1 + M * EPS * s[:k]
    observed(f"pca_tall {cid}: |sigma - s| / (C eps s_1 + M eps s_i)", np.abs(sig[:k] - s[:k]) / sbound, 1.0)
    s_all = np.concatenate([s, np.zeros(1 if r < dim else 0)])
    U = t.F1 * np.sqrt(t.D)              # column i = s_i u_i (X = F1 F2, V = F2 / sqrt(D)); t.rows rows
    ratios, sc_ratios = [], []
    i = 0
    while i < k:
        j = i
        while j + 1 < r and s[j + 1] == s[i]:
            j += 1
        lo, hi = i, j + 1
        other = np.delete(s_all, np.arange(lo, hi))
        gap = np.min(np.abs(other - s[lo])) if other.size else s1
        abound = (C * EPS * s1 + M * EPS * s[lo]) / gap + C * EPS
        Vt, Vd = t.V[lo:hi], V[lo:min(hi, k)]
        if hi - lo == 1:
            c = Vd[0] @ Vt[0]
            ratios.append(np.linalg.norm(Vd[0] - c * Vt[0]) / abound)
            sc_ratios.append(np.linalg.norm(S[:, lo] - np.sign(c) * U[:, lo]) / (s[lo] * abound + sbound[lo]))
        else:
            resid = Vd - (Vd @ Vt.T) @ Vt
            ratios.append(np.linalg.norm(resid, axis=1).max() / abound)
            if hi <= k:
                ratios.append(np.abs(Vd.T @ Vd - Vt.T @ Vt).max() / abound)
            ref = t.F1 @ (t.F2 @ Vd.T)
            fro = np.sqrt(np.sum(s ** 2))
            sc_ratios.append(np.linalg.norm(S[:, lo:lo + len(Vd)] - ref, axis=0).max() / (2 * dim * EPS * fro + sbound[lo]))
        i = hi
    observed(f"pca_tall {cid}: mode angle / ((C eps s_1 + M eps s_i) / gap + C eps)", np.array(ratios), 1.0)
    observed(f"pca_tall {cid}: ||score column -+ s_i u_i|| / (s_i angle bound + sigma bound)", np.array(sc_ratios), 1.0)
    nrm = np.sqrt(np.sum(S.astype(LD) ** 2, axis=0)).astype(np.float64)
    observed(f"pca_tall {cid}: |sigma_i - norm of score column i| / (M eps sigma_i)  [sigma is the measured norm]",
             np.abs(nrm - sig) / np.maximum(M * EPS * sig, 1e-300), 1.0)
    observed(f"pca_tall {cid}: orthonormality of the {n} rows", np.abs(V @ V.T - np.eye(n)), 1e-13)
    piv = np.argmax(np.abs(V), axis=1)
    assert np.all(V[np.arange(n), piv] > 0), (cid, "svd_flip sign convention")


@pytest.fixture(scope="module")
def ctx():
    from romhighcontrast_amd import _ffi
    return _ffi.get_context()


# ---- the property the method rests on: small eigenvalues of graded matrices to high RELATIVE accuracy ---------------------
def _jacobi_ld(A, tol=LD(2) ** -62, sweeps=30):
    """Eigenvalues of a symmetric positive definite matrix by cyclic two-sided Jacobi with the relative stopping rule, in
    80-bit arithmetic (relative accuracy ~ n 2^-64 kappa(scaled matrix), Demmel & Veselic 1992)."""
    A = np.array(A, dtype=LD)
    n = len(A)
    for _ in range(sweeps):
        rotated = False
        for p in range(n - 1):
            for q in range(p + 1, n):
                apq = A[p, q]
                if abs(apq) <= tol * np.sqrt(A[p, p] * A[q, q]):
                    continue
                rotated = True
                theta = (A[q, q] - A[p, p]) / (2 * apq)
                tt = np.sign(theta) / (abs(theta) + np.sqrt(theta * theta + 1)) if theta != 0 else LD(1)
                c = 1 / np.sqrt(tt * tt + 1)
                sn = tt * c
                rp, rq = A[p].copy(), A[q].copy()
                A[p], A[q] = c * rp - sn * rq, sn * rp + c * rq
                cp, cq = A[:, p].copy(), A[:, q].copy()
                A[:, p], A[:, q] = c * cp - sn * cq, sn * cp + c * cq
        if not rotated:
            break
    return np.sort(np.diag(A).astype(np.float64))[::-1]


@pytest.mark.parametrize("gram_like", [1, 2], ids=["n_eps", "tight_16_eps"])
@pytest.mark.parametrize("n", [81, 300])
def test_small_eig_gram_like_is_relatively_accurate_on_graded_matrices(ctx, n, gram_like):
    """A = D B D with D graded over eight orders (eigenvalues over sixteen) and B = L L^T well conditioned.  Demmel-Veselic:
    a Jacobi with the relative rule delivers every eigenvalue with relative error O(n eps kappa(B_scaled)); asserted with
    the constant C.  n = 81: kb_small_eig in LDS; n = 300: the grid-wide Jacobi.  gram_like = 2 is the rotation threshold
    16 eps that rom_pca_tall asks for (1: n eps)."""
    rng = np.random.default_rng(n)
    L = np.eye(n) + 0.25 * np.tril(rng.uniform(-1, 1, (n, n)), -1) / np.sqrt(n)
    d = 10.0 ** -np.linspace(0, 8, n)
    A = (d[:, None] * (L @ L.T)) * d[None, :]
    A = 0.5 * (A + A.T)
    truth = _jacobi_ld(A)
    sc = 1 / np.sqrt(np.diag(A))
    kappa = np.linalg.cond(sc[:, None] * A * sc[None, :])
    lam, T = ctx.small_eig(A, mode=0, gram_like=gram_like)
    assert truth.min() > 0 and truth.max() / truth.min() > 1e14
    observed(f"small_eig gram_like={gram_like} n={n}: max relative eigenvalue error / (C n eps kappa_scaled), kappa = {kappa:.1f}",
             np.abs(lam - truth) / truth / (C * n * EPS * kappa), 1.0)
    observed(f"small_eig gram_like={gram_like} n={n}: orthonormality of the eigenvector rows", np.abs(T @ T.T - np.eye(n)), 1e-13)


# ---- exact blocks ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_exact_block(ctx, case, monkeypatch):
    t = _truth(case)
    M, dim, n = t.rows, t.dim, case["n"]
    x0, v0, s0 = case["x_row0"], case["v_row0"], case["s_row0"]
    sig, info, Xb, Vb, Sb, mb = run_tall(ctx, case, t)
    Vall = Vb.download(shape=(v0 + n + 2, dim))
    Sall = Sb.download(shape=(s0 + M + 2, n))
    Xall = Xb.download(shape=(x0 + M + 2, dim))
    mall = mb.download()
    assert np.isnan(Vall[:v0]).all() and np.isnan(Vall[v0 + n:]).all(), (case["id"], "mode sentinels")
    assert np.isnan(Sall[:s0]).all() and np.isnan(Sall[s0 + M:]).all(), (case["id"], "score sentinels")
    assert np.isnan(Xall[:x0]).all() and np.isnan(Xall[x0 + M:]).all() and np.isnan(mall[dim]), (case["id"], "block sentinels")
    if case["mean"]:
        assert np.array_equal(mall[:dim], t.mean) and np.array_equal(Xall[x0:x0 + M], t.centred()), case["id"]
    else:
        assert not mall[:dim].any() and np.array_equal(Xall[x0:x0 + M], t.X), case["id"]
    check_truth(case, t, sig, info, Vall[v0:v0 + n], Sall[s0:s0 + M])
    sig2, info2, _, Vb2, Sb2, _ = run_tall(ctx, case, t)
    assert _same_bits(sig2, sig) and Vb2.same_bits_as(Vb, Vb.n) and Sb2.same_bits_as(Sb, Sb.n) and info2 == info, (case["id"], "repeat")
    monkeypatch.setenv("ROMHC_POISON_WS", "1")
    sig3, info3, _, Vb3, Sb3, _ = run_tall(ctx, case, t)
    monkeypatch.delenv("ROMHC_POISON_WS")
    assert _same_bits(sig3, sig) and Vb3.same_bits_as(Vb, Vb.n) and Sb3.same_bits_as(Sb, Sb.n) and info3 == info, (case["id"], "poisoned")


def test_zero_block_and_no_scores(ctx):
    M, dim = 500, 40
    Xb = ctx.upload(np.zeros((M, dim)))
    Vb, Sb = ctx.alloc(dim * dim), ctx.alloc(M * dim).fill(np.nan)
    sig, info = ctx.pca_tall(Xb, M, dim, dim, Vb, S=Sb, center=True)
    assert not sig.any() and info["resolved_modes"] == 0 and info["stop_reason"] == "converged", info
    V = Vb.download(shape=(dim, dim))
    observed("pca_tall zero block 500 x 40: orthonormality", np.abs(V @ V.T - np.eye(dim)), 1e-13)
    assert not Sb.download().any()
    # S = NULL, mean = NULL, n = 0
    t = rf.ExactSVD(256, 64, 64, [9, 5, 3], 4, seed=1)
    sig, info = ctx.pca_tall(ctx.upload(t.X), 256, 64, 3, ctx.alloc(3 * 64), center=False)
    observed("pca_tall without scores: |sigma - s| / (C eps s_1 + M eps s_i)", np.abs(sig - t.s) / (C * EPS * t.s[0] + 256 * EPS * t.s), 1.0)
    sig, info = ctx.pca_tall(ctx.upload(t.X), 256, 64, 0, ctx.alloc(1), center=True)
    assert len(sig) == 0 and info["stop_reason"] == "converged"


# ---- the reference's shape ---------------------------------------------------------------------------------------------------
def test_reference_block_25000_by_81(ctx):
    """vn_family_sampler(25000, (2, 2), 1, 100, 5) + do_pca against the oracle (64 sampled rows, the suite's 1e-11) and against
    numpy.linalg.svd of the centred host block.  LAPACK puts exactly 20 modes above 1e-13 sigma_1, then a cliff (asserted on
    its values: the count cannot drift silently); each of the 20 within 2 (C eps sigma_1 + M eps sigma_i) -- both sides
    carry the error."""
    from oracle import rom_oracle as ro
    from src.experiments import NonLinearROM as NL
    M = 25000
    out = NL.vn_family_sampler(M, (2, 2), 1, 100, 5)
    U, a = out["solutions"], out["a"]
    assert U.shape == (M, 81) and len(a) == M and a[0].shape == (2, 2)
    g = ro.Geometry((2, 2), 5)
    rows = np.random.default_rng(0).choice(M, size=64, replace=False)
    observed("NonLinearROM sweep: 64 sampled rows vs the oracle (relative H10)",
             rel_h10(g, U[rows], ro.generate_solutions(g, np.array([a[i] for i in rows]), "lsqsparse")), 1e-11)
    mu = U.mean(axis=0)
    s_ref = np.linalg.svd(U - mu, compute_uv=False)
    s1 = s_ref[0]
    assert np.sum(s_ref > 1e-13 * s1) == 20 and s_ref[19] > 1e-9 * s1 and s_ref[20] < 1e-13 * s1, s_ref[17:23] / s1
    res = NL.do_pca(U)
    pca = NL.do_pca.last
    assert pca.resolved_modes_ == 20 and pca.info["stop_reason"] == "converged", pca.info
    sig = res["singular_values"]
    assert sig.shape == (81,) and res["pca_projections"].shape == (M, 81)
    observed("NonLinearROM do_pca: |sigma - LAPACK| / (2 (C eps s_1 + M eps s_i)), 20 modes",
             np.abs(sig[:20] - s_ref[:20]) / (2 * (C * EPS * s1 + M * EPS * s_ref[:20])), 1.0)
    assert np.array_equal(res["explained_variance"], sig ** 2 / (M - 1))
    V, mean = pca.components_, pca.mean_
    observed("NonLinearROM do_pca: orthonormality of the 81 components", np.abs(V @ V.T - np.eye(81)), 1e-13)
    proj = np.asarray((U.astype(LD) - mean.astype(LD)) @ V.T.astype(LD), dtype=np.float64)
    observed("NonLinearROM do_pca: |pca_projections - (U - mean) V^T in long double| / (C eps s_1)",
             np.abs(res["pca_projections"] - proj) / (C * EPS * s1), 1.0)
    # transform() of new rows is the same map
    observed("TallPCA.transform(rows) vs the scores of the fit / (C eps s_1)",
             np.abs(pca.transform(U[:100]) - res["pca_projections"][:100]) / (C * EPS * s1), 1.0)


# ---- consistency with rom_pod ------------------------------------------------------------------------------------------------
def _compare_with_rom_pod(ctx, tag, X, s, n, with_sign):
    """Both calls on the same block; s: the true (or LAPACK) singular values, all of them.  Singular values within the sum
    of both tests' bounds, modes within the sum of both angle bounds -- as vectors, sign included, when with_sign."""
    M, dim = X.shape
    s1 = s[0]
    Vp, Vt = ctx.alloc(n * dim), ctx.alloc(n * dim)
    sig_p, info_p = ctx.pod(ctx.upload(X), M, dim, n, Vp, center=False)
    sig_t, info_t = ctx.pca_tall(ctx.upload(X), M, dim, n, Vt, center=False)
    assert info_t["stop_reason"] == "converged", info_t
    gram = info_p["gram_passes"] > 0
    rel = np.where(s[:n] >= 1e-6 * s1, 1e-10, 1e-5) * s[:n] + (1e-14 * s1 ** 2 / s[:n] if gram else 0.0)
    b_pod = C * EPS * s1 + rel
    b_tall = C * EPS * s1 + M * EPS * s[:n]
    observed(f"pca_tall vs rom_pod ({tag}, n = {n}): |sigma difference| / (sum of both bounds)", np.abs(sig_t - sig_p) / (b_pod + b_tall), 1.0)
    A, B = Vp.download(shape=(n, dim)), Vt.download(shape=(n, dim))
    s_all = np.concatenate([s, [0.0]]) if len(s) < dim else s
    rat = []
    for i in range(n):
        gap = np.min(np.abs(np.delete(s_all, i) - s[i]))
        gap2 = np.min(np.abs(np.delete(s_all, i) ** 2 - s[i] ** 2))
        a_pod = C * EPS * s1 / gap + C * EPS + (2e-14 * s1 ** 2 / gap2 if gram else 0.0)
        a_tall = (C * EPS * s1 + M * EPS * s[i]) / gap + C * EPS
        diff = np.linalg.norm(A[i] - B[i]) if with_sign else min(np.linalg.norm(A[i] - B[i]), np.linalg.norm(A[i] + B[i]))
        rat.append(diff / (a_pod + a_tall))
    observed(f"pca_tall vs rom_pod ({tag}): ||mode difference|| ({'sign included' if with_sign else 'up to sign: tied entries'}) / "
             "(sum of both angle bounds)", np.array(rat), 1.0)
    for Vm in (A, B):
        piv = np.argmax(np.abs(Vm), axis=1)
        assert np.all(Vm[np.arange(n), piv] > 0), (tag, "svd_flip sign convention")


def test_agrees_with_rom_pod(ctx):
    """Where both calls apply (n = 30 of a 4096 x 300 block).  On the exact block every entry of a true mode has the same
    magnitude 1 / sqrt(D): svd_flip's "entry of largest magnitude" is decided by the rounding of each call, so the modes
    are compared up to sign there (each call's own convention is asserted); on a block whose modes have one clearly
    largest entry the modes must agree as vectors, sign included."""
    M, D, dim, n = 4096, 256, 300, 30
    mant, e = _mant(_geo(40, 4), M)
    t = rf.ExactSVD(M, D, dim, mant, e, seed=3)
    _compare_with_rom_pod(ctx, "exact 4096 x 300", t.X, t.s, n, with_sign=False)
    rng = np.random.default_rng(11)
    Q = np.linalg.qr(rng.standard_normal((M, 40)))[0]
    W = np.linalg.qr(np.eye(dim)[:, :40] + 0.2 * rng.standard_normal((dim, 40)) / np.sqrt(dim))[0]   # mode k: a dominant entry k
    X = (Q * _geo(40, 4)) @ W.T
    s_ref = np.linalg.svd(X, compute_uv=False)[:40]
    _compare_with_rom_pod(ctx, "dominant-entry 4096 x 300", X, s_ref, n, with_sign=True)


# ---- the error cases of the contract -------------------------------------------------------------------------------------------
def test_error_cases(ctx):
    from romhighcontrast_amd import _ffi
    X = ctx.upload(np.ones((10, 8)))
    V = ctx.alloc(64)

    def fails(words, *args, **kw):
        with pytest.raises(_ffi.RomLibraryError) as ei:
            ctx.pca_tall(*args, **kw)
        assert all(w in str(ei.value) for w in words), str(ei.value)

    fails(["n = 9", "dim = 8"], X, 10, 8, 9, V)
    fails(["1024"], ctx.alloc(2 * 1025), 2, 1025, 1, ctx.alloc(1025))
    fails(["X holds"], X, 11, 8, 2, V)
    fails(["V too small"], X, 10, 8, 8, ctx.alloc(63))
    fails(["S too small"], X, 10, 8, 8, V, S=ctx.alloc(79))
    fails(["mean holds"], X, 10, 8, 8, V, mean=ctx.alloc(7))
    fails(["bad sizes"], X, 0, 8, 0, V)
    bad = np.ones((10, 8))
    bad[3, 4] = np.nan
    fails(["NaN / Inf"], ctx.upload(bad), 10, 8, 8, V, center=False)
    from src.lib.ReducedBasis import pca_tall
    with pytest.raises(ValueError):
        pca_tall(ctx, bad)
    fails(["rescale the block"], ctx.upload(np.full((10, 8), 1e200) * np.arange(1, 9)), 10, 8, 8, V, center=False)


# ---- which kernels ran: a child process (ROMHC_PROF_DETAIL is read once per process) ----------------------------------------
def test_forms_confirmed_by_profile_names():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, ROMHC_PROF_DETAIL="1")
    r = subprocess.run([sys.executable, os.path.join(root, "tests", "pca_tall_child.py")], env=env, cwd=root,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    out = r.stdout.decode(errors="replace")
    print(out)
    assert r.returncode == 0 and out.rstrip().endswith("OK"), out[-4000:]
    got = json.loads([ln for ln in out.splitlines() if ln.startswith("FORMS ")][-1][6:])
    assert got["81"]["fused"] == got["81"]["passes"] and got["81"]["rotate"] == 0 and got["81"]["syrk"] == 0, got
    assert got["300"]["fused"] == 0 and got["300"]["syrk"] == got["300"]["passes"], got
    assert got["300"]["rotate"] == got["300"]["passes"] - 1, got      # (the first pass has V = I: no product)
