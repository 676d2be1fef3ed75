"""CPU side of the H^1_0-POD tests: the truth builder of tests/h10_truth.py proved against LAPACK, the bounds of
tests/test_gpu_pod_h10.py checked on a plain fp64 NumPy restatement of the device pipeline, and the bookkeeping of the builders.

  * Truth.  H10Truth claims an exact H^1_0 SVD (s, V) of its fp64 block U.  With A_1 = L L^T (dense Cholesky of the 5-point
    matrix) the H^1_0 SVD of U is the Euclidean SVD of Uc L: LAPACK's values must agree with s to C eps kappa s_1, its modes
    L^-T y_i with V to C eps kappa s_1 / gap_i + C eps kappa in the H^1_0 angle (edge coordinates of the long-double stencil),
    and V must be A_1-orthonormal to C eps.  (kappa: rounding U to fp64 moves its energy coordinates by eps kappa, h10_truth.)
  * Restatement.  transform -> numpy.linalg.svd -> back-transform in fp64 NumPy, through the same check_pod_h10 that judges
    the device, and the fp64 NumPy transform against the long-double one under the per-row bound of the device test, its round
    trip under the sum of the two bounds, and its A_1^-1 of evaluation vectors under the Riesz comparison's bound: the bounds
    are ones that a straightforward fp64 implementation meets on these inputs, with the observed margin in the summary.
  * Bookkeeping without a device: names, the unchanged default, the exception for an unknown inner product.
"""
import numpy as np
import pytest

from conftest import observed
import h10_truth as ht

EPS, C = ht.EPS, ht.C


@pytest.mark.parametrize("case", ht.POD_CASES, ids=[c["id"] for c in ht.POD_CASES])
def test_truth_builder_against_lapack_and_numpy_restatement(case):
    tr = ht.pod_truth(case)
    gr, n, cid = tr.gr, case["n"], case["id"]
    kap, s1 = gr.kappa, tr.s[0]
    Uc = tr.U - tr.U.mean(axis=0) if case["center"] else tr.U
    # the truth is A_1-orthonormal (long-double stencil)
    G = np.asarray(gr.a1_dots(tr.V, tr.V), dtype=np.float64)
    observed(f"h10 truth {cid}: |V A_1 V^T - I| of the true modes", np.abs(G - np.eye(tr.r)), C * EPS)
    # LAPACK on Uc L
    L = np.linalg.cholesky(gr.a1_dense())
    _, sl, Yt = np.linalg.svd(Uc @ L, full_matrices=False)
    observed(f"h10 truth {cid}: |sigma_LAPACK - s| / (C eps kappa s_1)", np.abs(sl[:tr.r] - tr.s) / (C * EPS * kap * s1), 1.0)
    observed(f"h10 truth {cid}: LAPACK's values past the rank / (C eps kappa s_1)", sl[tr.r:] / (C * EPS * kap * s1), 1.0)
    k = int(np.sum(tr.s[:n] > ht.NOISE_FLOOR * s1))
    Vl = np.linalg.solve(L.T, Yt[:k].T).T
    El, Et = gr.energy(Vl), gr.energy(tr.V[:k])
    s_all = np.concatenate([tr.s, [0.0]])
    ratios = []
    for i in range(k):
        gap = np.min(np.abs(np.delete(s_all, i) - s_all[i]))
        c = El[i] @ Et[i]
        ratios.append(float(np.sqrt(np.sum((El[i] - c * Et[i]) ** 2))) / (C * EPS * kap * s1 / gap + C * EPS * kap))
    observed(f"h10 truth {cid}: H10 angle LAPACK mode / truth / (C eps kappa s_1 / gap + C eps kappa)", np.array(ratios), 1.0)
    # the device pipeline restated in fp64 NumPy, judged like the device
    W = gr.transform(tr.U, 0, 1, ld=False)
    if case["center"]:
        W = W - W.mean(axis=0)
    _, sw, Qt = np.linalg.svd(W, full_matrices=False)
    fl = max(case["rel_floor"], ht.NOISE_FLOOR)
    res = int(np.sum(sw[:n] > fl * sw[0]))
    sig = np.where(np.arange(n) < res, sw[:n], 0.0)
    V = gr.transform(Qt[:n], -1, 0, ld=False)
    V = V * np.sign(V[np.arange(n), np.argmax(np.abs(V), axis=1)])[:, None]
    info = dict(resolved_modes=res, completed_modes=n - res, gram_passes=0, stop_reason="filled" if res == n else "floor")
    ht.check_pod_h10(case, tr, sig, info, V, observed, who="fp64 NumPy restatement")


@pytest.mark.parametrize("blocks,N", ht.GRIDS, ids=[f"{b[0]}x{b[1]}_N{N}" for b, N in ht.GRIDS])
def test_numpy_transform_inside_the_device_bound(blocks, N):
    gr = ht.grid(blocks, N)
    X = ht.transform_rows(gr, 70, seed=gr.dim)
    for pre, post in ht.PAIRS:
        truth = gr.transform(X, pre, post)
        got = gr.transform(X, pre, post, ld=False)
        err = np.asarray(np.sqrt(np.sum((got - truth) ** 2, axis=1)), dtype=np.float64)
        observed(f"fp64 NumPy sine transform {gr.nr}x{gr.nc} (pre, post) = ({pre}, {post}): row error / bound",
                 err / gr.transform_bound(X, pre, post), 1.0)
    # round trip (0,1), (-1,0) in fp64 NumPy under the sum of the two bounds, as the device test asserts it
    W = gr.transform(X, 0, 1, ld=False)
    back = gr.transform(W, -1, 0, ld=False)
    observed(f"fp64 NumPy sine transform {gr.nr}x{gr.nc}: round trip (0,1), (-1,0) / (bound(0,1) + bound(-1,0))",
             np.linalg.norm(back - X, axis=1) / ht.round_trip_bound(gr, X, W), 1.0)
    # A_1^-1 of the P1 evaluation vectors by (0,-2), (0,0) in fp64 NumPy against the long-double A_1^-1: each fp64 route is
    # within b of it, so two of them (the device compares its own with generate_riesz_h10) are within 2 b of each other
    R = ht.evaluation_rows(gr, ht.riesz_points(gr))
    assert R.shape == (3, gr.dim) and np.all(np.abs(R).sum(axis=1) > 0)
    Z = gr.transform(R, 0, -2, ld=False)
    Om = gr.transform(Z, 0, 0, ld=False)
    truth = gr.transform(gr.transform(R, 0, -2), 0, 0)
    err = np.asarray(np.sqrt(np.sum((Om - truth) ** 2, axis=1)), dtype=np.float64)
    observed(f"fp64 NumPy sine transform {gr.nr}x{gr.nc}: (0,-2), (0,0) of evaluation vectors vs long-double A_1^-1 r / b",
             err / ht.riesz_bound(gr, R, Z), 1.0)
    resid = np.asarray(gr.a1_dots(truth, np.eye(gr.dim)), dtype=np.float64) - R if gr.dim <= 1000 else np.zeros(1)
    assert float(np.abs(resid).max()) < 1e-15, "the long-double (0,-2), (0,0) is A_1^-1 (stencil residual)"
    # the tables: symmetric, orthogonal, and A_1 = S Lambda S against the dense stencil
    Sr = gr.Sr
    assert float(np.abs(Sr - Sr.T).max()) == 0.0
    assert float(np.abs(Sr @ Sr - np.eye(gr.nr)).max()) < 1e-17 * gr.nr
    if gr.dim <= 400:
        S = np.kron(gr.Sr, gr.Sc)
        A = (S * gr.lam.ravel()) @ S
        assert float(np.abs(A - gr.a1_dense()).max()) < 1e-16


def test_round_trip_and_inverse_identities_in_long_double():
    """(0,1) then (-1,0) is the identity and (0,-2) then (0,0) is A_1^-1: the identities the device tests rely on."""
    gr = ht.grid((2, 3), 8)
    X = ht.transform_rows(gr, 5, seed=3)
    back = gr.transform(gr.transform(X, 0, 1), -1, 0)
    assert float(np.max(np.abs(back - X) / np.abs(X).max(axis=1, keepdims=True))) < 1e-17
    Z = gr.transform(gr.transform(X, 0, -2), 0, 0)
    assert float(np.abs(Z.astype(np.float64) @ gr.a1_dense() - X).max() / np.abs(X).max()) < 1e-13


def test_builder_bookkeeping():
    from src.lib import ReducedBasis as RB
    from romhighcontrast_amd import _ffi, factored
    assert RB.ReducedBasisPCA().name == "PCA $\\infty$" and RB.ReducedBasisPCA(False).name == "PCA"
    assert RB.ReducedBasisPCA().inner_product == "l2"
    assert RB.ReducedBasisPCA(inner_product="h10").name == "PCA $H^1_0$ $\\infty$"
    assert RB.ReducedBasisPCA(False, inner_product="h10").name == "PCA $H^1_0$"
    assert RB.ReducedBasisPCA(True, "h10").add_inf_solutions is True
    with pytest.raises(Exception, match="[Nn]ot implemented"):
        RB.ReducedBasisPCA(False, inner_product="h1").build(3, None, np.zeros((4, 9)), np.ones((4, 1, 1)))
    with pytest.raises(Exception, match="[Nn]ot implemented"):
        factored.pod_modes_factored(None, 3, inner="energy")
    assert callable(RB.pod_modes_h10)
    for name in ("sine_transform", "pod_h10", "pod_h10_factored"):
        assert callable(getattr(_ffi.Fem, name)) and "rom_" + name in _ffi.PROTOTYPES
