"""LocalReducedBasis on the GPU, on (2,2) / N = 8 (dim 225): 1500 training parameters in [1, 100]^4, 300 held out, 8 clusters of
log a with an uncentred H^1_0-POD basis of dimension 8 each.  The bases against their definition, the online operations against
a per-row loop over the existing API (in a permuted order: a wrong inverse permutation fails), the gain over the global basis of
the same dimension (cap 0.5; tests/test_kmeans_host.py recomputes 0.0143 against 0.0590 on the CPU), pickling, and the refusal of
a cluster too small for its basis."""
import pickle

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N_CLUSTERS, N_BASIS = 8, 8


@pytest.fixture(scope="module")
def problem():
    from oracle import rom_oracle as ro
    from romhighcontrast_amd.lib.ReducedBasis import LocalReducedBasis
    from romhighcontrast_amd.lib.SolutionsManagers import SolutionsManagerFEM
    rng = np.random.default_rng(7)
    a = 10.0 ** rng.uniform(0, 2, size=(1800, 2, 2))
    sm = SolutionsManagerFEM((2, 2), 8)
    U = sm.generate_solutions(a)
    lrb = LocalReducedBasis(N_CLUSTERS, inner_product="h10").build(N_BASIS, sm, U[:1500], a[:1500])
    A1 = np.asarray(ro.assemble_dense(ro.Geometry((2, 2), 8), np.ones((2, 2))))
    perm = rng.permutation(300)
    return dict(sm=sm, a=a, U=U, lrb=lrb, A1=A1, a_test=a[1500:][perm], U_test=U[1500:][perm])


def _same_bits(a, b):
    return np.array_equal(np.asarray(a, dtype=np.float64).view(np.uint64), np.asarray(b, dtype=np.float64).view(np.uint64))


def test_bases_are_the_h10_pod_of_their_clusters(problem):
    from romhighcontrast_amd.lib.ReducedBasis import pod_modes_h10
    from romhighcontrast_amd.lib.SolutionsManagers import _as_device
    sm, lrb, A1, U = problem["sm"], problem["lrb"], problem["A1"], problem["U"]
    counts = np.bincount(lrb.labels_, minlength=N_CLUSTERS)
    print("cluster sizes", counts.tolist(), "iterations", lrb.kmeans.n_iter_)
    assert len(lrb.bases) == N_CLUSTERS and counts.min() >= N_BASIS + 1 and counts.sum() == 1500
    assert np.array_equal(lrb.labels_, lrb.classify(problem["a"][:1500]))
    for j, rb in enumerate(lrb.bases):
        B = np.asarray(rb.basis)
        rows = U[:1500][lrb.labels_ == j]
        assert B.shape == (N_BASIS, 225)
        assert abs(B @ A1 @ B.T - np.eye(N_BASIS)).max() <= 1e-12, j
        coef = np.linalg.lstsq(rows.T, B.T, rcond=None)[0]
        assert abs(rows.T @ coef - B.T).max() <= 1e-8 * abs(B).max(), j
        ref, _ = pod_modes_h10(sm, _as_device(sm._ctx, rows, 225), N_BASIS, center=False)
        assert abs(B.T @ B @ A1 - ref.T @ ref @ A1).max() <= 1e-9, j


def test_online_operations_equal_a_per_row_loop_in_input_order(problem):
    sm, lrb, a, U = problem["sm"], problem["lrb"], problem["a_test"], problem["U_test"]
    labels = lrb.classify(a)
    proj, fm = lrb.projection(sm, U, a), lrb.forward_modeling(sm, a)
    assert isinstance(proj, np.ndarray) and proj.shape == fm.shape == U.shape
    ref_p = np.vstack([sm.project_solutions(U[i:i + 1], lrb.bases[labels[i]].basis) for i in range(len(a))])
    ref_f = np.vstack([sm.generate_fm_solutions(a[i:i + 1], lrb.bases[labels[i]].basis) for i in range(len(a))])
    norms = sm.H10norm(U)
    assert (sm.H10norm_diff(proj, ref_p) / norms).max() <= 1e-12
    assert (sm.H10norm_diff(fm, ref_f) / norms).max() <= 1e-12
    ep, eg = lrb.errors(sm, U, a)
    assert np.allclose(ep, sm.H10norm_diff(ref_p, U) / norms, rtol=1e-6, atol=1e-13) and (eg >= ep * (1 - 1e-9)).all()
    from romhighcontrast_amd.lib.SolutionsManagers import DeviceArray, _as_device
    pd = lrb.projection(sm, _as_device(sm._ctx, U, 225), a)
    assert isinstance(pd, DeviceArray) and _same_bits(pd.numpy(), proj)


def test_local_bases_halve_the_held_out_error_of_the_global_basis(problem):
    from romhighcontrast_amd.lib.ReducedBasis import pod_modes_h10
    from romhighcontrast_amd.lib.SolutionsManagers import _as_device
    sm, lrb, a, U = problem["sm"], problem["lrb"], problem["a_test"], problem["U_test"]
    norms = sm.H10norm(U)
    local = np.sqrt(((sm.H10norm_diff(lrb.projection(sm, U, a), U) / norms) ** 2).mean())
    G, _ = pod_modes_h10(sm, _as_device(sm._ctx, problem["U"][:1500], 225), N_BASIS, center=False)
    glob = np.sqrt(((sm.H10norm_diff(sm.project_solutions(U, G), U) / norms) ** 2).mean())
    print(f"held-out rms relative H10 projection error at n = {N_BASIS}: local {local:.4f}, global {glob:.4f}, ratio {local / glob:.3f}")
    assert local <= 0.5 * glob


def test_pickle_round_trip_gives_the_same_bits(problem):
    sm, lrb, a, U = problem["sm"], problem["lrb"], problem["a_test"], problem["U_test"]
    twin = pickle.loads(pickle.dumps(lrb))
    assert twin.kmeans.handle_ is None
    assert np.array_equal(twin.classify(a), lrb.classify(a))
    assert _same_bits(twin.projection(sm, U, a), lrb.projection(sm, U, a))


def test_a_cluster_too_small_for_its_basis_is_refused(problem):
    from romhighcontrast_amd.factored import FactoredSnapshots
    from romhighcontrast_amd.lib.ReducedBasis import LocalReducedBasis
    sm, a, U = problem["sm"], problem["a"], problem["U"]
    with pytest.raises(ValueError, match=r"cluster \d+ has \d+ rows"):
        LocalReducedBasis(N_CLUSTERS).build(N_BASIS, sm, U[:40], a[:40])
    with pytest.raises(TypeError, match="rows"):   # (refused by its type, before anything of the block is looked at)
        LocalReducedBasis(N_CLUSTERS).build(N_BASIS, sm, object.__new__(FactoredSnapshots), a[:40])
