"""Every route of rom_pod_ex (csrc/rom_pod.hip) against blocks whose SVD is known exactly (tests/referee.py: ExactSVD), and
rom_pod_factored (csrc/rom_factored.hip) against LAPACK and rom_pod on the expanded rows of sweep blocks.

ROUTES below is the route table of rom_pod_ex; every case of CASES names the routes it is designed to reach.  Each case runs
the device call once with sentinel (NaN) rows around the block and around the modes, and asserts against the exact truth:
  * singular values  |sigma_i - s_i| <= C eps s_1 + rel_i, rel_i = 1e-10 s_i above 1e-6 s_1 and 1e-5 s_i below (what the
    sketch passes claim: SKETCH_ACCEPT's comment and test_pod_passes_resolve_seven_orders_each); on the Gram route the
    eigenvalues carry the 2e-14 lambda_1 residual of the iteration (Bauer-Fike), |sigma^2 - s^2| <= 2e-14 s_1^2, so
    rel_i += 1e-14 s_1^2 / s_i;
  * modes  sin(angle to the true mode) <= C eps s_1 / gap_i (+ 2e-14 s_1^2 / gap2_i on the Gram route, gap2 = the gap of
    the squared values) + C eps; a cluster of equal values is compared through its projector (or, when the request ends
    inside it, every mode must lie in the cluster's span);
  * rows orthonormal to 1e-13 and in svd_flip's sign convention (largest |entry| positive, first index on ties);
  * completed rows: sigma = 0 and ||X_c v|| <= floor s_1 + C eps s_1;
  * info: resolved = #{s_i > floor s_1} (the spectra keep a clear gap at the floor), completed = n - resolved, the stop
    reason, and the pass counts each case states;
  * the same bits on a repeated call (the block re-uploaded: the call overwrites it when it centres) and with
    ROMHC_POISON_WS set; the NaN rows outside the ranges come back unchanged.
C = 64.  tests/pod_routes_child.py reruns every case with ROMHC_PROF_DETAIL and confirms its routes from the profile
names; test_route_table_is_covered asserts that every route of the table was reached and confirmed.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import observed
import referee as rf

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -53
C = 64.0
NOISE_FLOOR = 1e-13

# ---- the route table of rom_pod_ex ----------------------------------------------------------------------------------
ROUTES = {
    "one_pass": "one sketch pass fills the request (no Gram route)",
    "multi_pass": "several sketch passes; the implicit deflation and the accepted rows through combine_rows",
    "combine_rows": "kp_combine_rows_mma (row blocks <= 64)",
    "pass_gemm": "a pass with b > 64 rows accepting take > 64 modes: the accepted rows through GEMM",
    "pass_gemm_small_take": "a pass with b > 64 rows accepting take <= 64 modes: the accepted rows through GEMM all the same",
    "correction_gemm": "a pass with found > 512: its rank-found corrections through GEMM although b <= 64",
    "final_gemm": "the final Rayleigh-Ritz step with found > 64: the rotation through GEMM",
    "tall_svd_unfused": "the final tall SVD on the parallel path (found > 32 or M > 4096): no kp_tall_svd for it",
    "gram": "the Gram route after a complete first pass (the cost model prefers it)",
    # the eigenpairs of the Gram matrix (top_eigenpairs / lowrank_eigenpairs), by branch of the code:
    "lowrank_first": "the first pivoted-Cholesky factor (<= 32 steps) ends by tolerance and is accepted (one host sync)",
    "lowrank_second": "the first factor gives up; the second (<= 96 steps) ends by tolerance and is accepted",
    "lowrank_rejected": "a factor ends by tolerance but fails LOWRANK_RESIDUAL: the general path follows",
    "subspace_iter": "subspace iteration on a Gram matrix with M <= 2048, converged",
    "full_eig_size": "the whole Gram matrix diagonalised because the request is most of it",
    "subspace_iter_large": "subspace iteration on a Gram matrix with M > 2048",
    "full_eig_stall": "the whole Gram matrix diagonalised after the iteration stalled",
    "pilot": "the first pass abandoned after two products (M dim >= 2.64e8), then the Gram route",
    "best_effort": "a pass with no converged mode: best effort, power = 2 from then on",
    "floor": "stop at the 1e-13 noise floor",
    "floor_rel": "stop at a caller's rel_floor",
    "cliff": "a cliff of more than eight orders with modes below it, found by the next pass",
    "centre_sketch": "the column mean from the first pass's first product",
    "centre_explicit": "explicit centring (n = 0, M = 1 or dim = 1)",
    "complete_fused": "completion on the fused row kernels (rest <= 32 and found <= 512)",
    "complete_general": "completion by rom_complete_orthonormal (rest > 32 or found > 512)",
    "zero_block": "a block of zeros",
    "n_full": "n = min(M, dim)",
    "m_gt_dim": "M > dim",
    "ahead_hit": "the next pass's first product started ahead on the second stream and taken",
    "row_offsets": "x_row0 > 0 and v_row0 > 0 with sentinel rows",
}
EIG_ROUTES = {"lowrank_first", "lowrank_second", "lowrank_rejected", "subspace_iter", "subspace_iter_large", "full_eig_size",
              "full_eig_stall"}
# (not in the table: an ahead product taken for the LEADING rows of a larger one.  The product is started with
# min(M, dim, 32) rows and only when min(M, dim) >= 128, and every pass asks for max(want + 8, 32) rows capped by
# min(M, dim): the next pass always asks for exactly 32 -- sketch_ahead_take's "sa.b > b" cannot happen in rom_pod_ex.)


def _mant(values, M):
    """Dyadic mantissas for relative values (1 = s_1): the largest exponent e with M sum(m) < 2^52 (exact partial sums)."""
    v = np.asarray(values, dtype=np.float64)
    e = int(np.floor(52 - np.log2(M * v.sum()))) - 1
    m = np.round(v * 2.0 ** e).astype(np.int64)
    assert m.min() >= 1
    return m, e


def _geo(r, hi, lo):
    return 10.0 ** -np.linspace(hi, lo, r)


# Each case: id, M, D, dim, relative spectrum, n, centre, mean, rel_floor, x_row0, v_row0, routes, expected info; `eig`: the
# Gram eigen-routes the case must take, exactly (asserted against the profile); `coherent`: unit left vectors (ExactSVD)
def _case(cid, M, D, dim, values, n, center=False, mean=False, rel_floor=0.0, x_row0=0, v_row0=0, routes=(), info=None,
          device_build=False, eig=None, coherent=False):
    eig = set(eig or ())
    return dict(id=cid, M=M, D=D, dim=dim, values=np.asarray(values, dtype=np.float64), n=n, center=center, mean=mean,
                rel_floor=rel_floor, x_row0=x_row0, v_row0=v_row0, routes=set(routes) | eig, info=info or {},
                device_build=device_build, eig=eig, coherent=coherent)


CASES = [
    _case("one_pass", 256, 1024, 1500, _geo(20, 0, 6), 16, center=True, mean=True, x_row0=3, v_row0=2,
          routes={"one_pass", "combine_rows", "centre_sketch", "row_offsets"}, info=dict(gram_passes=0, sketch_passes=1)),
    _case("multi_pass", 512, 2048, 2048, _geo(25, 0, 12), 25, routes={"multi_pass", "combine_rows"},
          info=dict(gram_passes=0)),
    _case("wide_pass", 512, 2048, 2048, _geo(70, 0, 1), 300, x_row0=1, v_row0=5,
          routes={"pass_gemm", "final_gemm", "tall_svd_unfused", "complete_general", "floor", "row_offsets"},
          info=dict(gram_passes=0)),
    # The pivoted-Cholesky factors of lowrank_eigenpairs.  Coherent blocks (u_k = unit vectors): the Gram matrix is diagonal
    # and the pivots ARE the squared singular values.  kp_pivchol_lowrank gives up when the decay so far extrapolates past
    # its cap (at 16 steps: pivots down 1e-7 for the 32-step factor, 4.6e-3 for the 96-step one) and stops by tolerance at
    # the first pivot <= 1e-14 x the first; the first sketch pass must not converge: s_32 > 4.6e-5 s_k already for k = 2.
    #   lowrank_first: s_2..31 from 3e-5 to 3e-7, then nine values ~2e-8 (pivots 4e-16: the factor ends at rank 31, and the
    #   trace they leave, 3e-15, is below LOWRANK_RESIDUAL = 2e-14);  lowrank_rejected: the same with the nine at ~8.5e-8
    #   (pivots 7e-15 < 1e-14, trace 6.5e-14 > 2e-14);  lowrank_second: 49 values from 0.1 to 1e-4 (rank 50; the first
    #   factor gives up at 16 steps, the second does not: 1.3e-4, 1.3e-6, 1.3e-8 at 16, 32, 48 steps).
    _case("lowrank_first", 128, 256, 300, np.concatenate([[1.0], np.geomspace(3e-5, 3e-7, 30), np.geomspace(2e-8, 1.5e-8, 9)]),
          20, routes={"gram"}, eig={"lowrank_first"}, info=dict(gram_passes=1), coherent=True),
    _case("lowrank_rejected", 128, 256, 300, np.concatenate([[1.0], np.geomspace(3e-5, 3e-7, 30), np.geomspace(9e-8, 8e-8, 9)]),
          20, routes={"gram"}, eig={"lowrank_rejected", "subspace_iter"}, info=dict(gram_passes=1), coherent=True),
    _case("lowrank_second", 256, 256, 300, np.concatenate([[1.0], np.geomspace(1e-1, 1e-4, 49)]), 40, routes={"gram"},
          eig={"lowrank_second"}, info=dict(gram_passes=1, sketch_passes=1), coherent=True),
    # Hadamard (incoherent) left vectors: every row of the block mixes every mode, and the pivots fall more slowly than
    # the spectrum.  A centred rank-31 block: the first factor gives up at 16 steps, the second takes it
    _case("gram_centred_rank31", 128, 512, 600, np.concatenate([_geo(16, 0, 3), np.linspace(7e-5, 6e-5, 15)]), 20,
          center=True, mean=True, routes={"gram", "centre_sketch"}, eig={"lowrank_second"},
          info=dict(gram_passes=1, sketch_passes=1)),
    # rank 65 with the same kind of spectrum: both factors give up, the subspace iteration converges
    _case("gram_hadamard_rank65", 256, 256, 300, np.concatenate([_geo(16, 0, 2), _geo(16, 2 + 2 / 15, 4), _geo(33, 4 + 1 / 32, 5)]),
          40, routes={"gram"}, eig={"subspace_iter"}, info=dict(gram_passes=1)),
    # 40 slowly decaying values over a cluster of 400 at 1.5e-8: the Gram route takes the 40, the passes after it find no
    # converged mode in the flat cluster (best effort); a cluster split by the request is checked by span
    _case("gram_cluster_tail", 512, 2048, 2048, np.concatenate([_geo(40, 0, 0.3), np.full(400, 2.0 ** -26)]), 50,
          routes={"gram", "best_effort", "multi_pass"}, eig={"subspace_iter"}, info=dict(gram_passes=1)),
    _case("gram_full_eig_size", 128, 128, 300, _geo(127, 0, 3), 60, routes={"gram"}, eig={"full_eig_size"},
          info=dict(gram_passes=1, sketch_passes=1)),
    _case("gram_subspace_4096", 4096, 4096, 4608, _geo(200, 0, 4), 30, routes={"gram"}, eig={"subspace_iter_large"},
          info=dict(gram_passes=1, sketch_passes=1)),
    _case("gram_full_eig_stall", 1024, 1024, 1100, np.linspace(1.0, 0.9, 1000), 20, routes={"gram"}, eig={"full_eig_stall"},
          info=dict(gram_passes=1, sketch_passes=1)),
    _case("pilot_2GB", 4096, 65536, 65536, _geo(65, 0, 2), 40, routes={"pilot"}, eig={"subspace_iter_large"},
          info=dict(gram_passes=1, sketch_passes=0), device_build=True),
    _case("floor_rel", 256, 1024, 1024, np.concatenate([_geo(12, 0, 4), _geo(18, 8, 10)]), 25, rel_floor=1e-6, v_row0=4,
          routes={"floor_rel", "complete_fused", "row_offsets"}),
    _case("cliff", 256, 1024, 1024, np.concatenate([_geo(10, 0, 1), [1e-11, 8e-12, 6e-12, 4e-12]]), 20,
          routes={"cliff", "multi_pass", "floor", "complete_fused"}, info=dict(gram_passes=0)),
    _case("n_full_m_gt_dim", 256, 64, 64, _geo(63, 0, 5), 64, routes={"n_full", "m_gt_dim", "floor"}),
    _case("ahead", 1024, 4096, 8192, _geo(24, 0, 11.5), 30, routes={"ahead_hit", "multi_pass", "floor"}, info=dict(gram_passes=0)),
    # n = 240: the first pass asks for want = n / 4 = 60 modes with b = 68 > 64 rows and accepts the block's 40 (the other
    # 28 rows are rounding noise: all 40 converged), take = 40 <= 64 < b: Rt Q and Rt Traw through GEMM, 40 x dim x 68 and
    # 40 x M x 68 -- no other product of the call has 68 as its inner size and 40 rows.  The second pass (58 rows) finds
    # the floor; 200 rows are completed
    _case("pass_gemm_small_take", 256, 256, 320, _geo(40, 0, 4), 240,
          routes={"pass_gemm_small_take", "combine_rows", "complete_general", "floor"}, info=dict(gram_passes=0)),
    # found > 512 in front of a pass.  No sequence of passes gets there within M, dim <= 1024 (a first pass with unconverged
    # modes hands over to the Gram route at these sizes, and converged passes cost 4.6 decades each), so the Gram route
    # delivers them: 516 values over three decades (all above GRAM_ACCEPT; the request is most of the Gram matrix: it is
    # diagonalised whole), then 16 values at 1e-8 .. 1e-9 for the pass behind it: 24 modes left, 32 rows, found = 516 --
    # its corrections are 32 x dim x 516 and 32 x M x 516 GEMMs.  It stops at the floor with found = 532; the 8 rows left
    # are completed by rom_complete_orthonormal (8 x dim x 532: found > 512 rules the fused kernels out).  Coherent: the
    # child tells the Gram iteration's products from the sketch's by dim != M, and Hadamard left vectors with r >= 532 and
    # M, dim <= 1024 would need M = dim = 1024
    _case("correction_gemm", 640, 1024, 1024, np.concatenate([np.geomspace(1.0, 1e-3, 516), np.geomspace(1e-8, 1e-9, 16)]), 540,
          routes={"correction_gemm", "gram", "final_gemm", "complete_general", "floor"},
          eig={"full_eig_size"}, info=dict(gram_passes=1), coherent=True),
]
COVERED = set()     # routes reached by cases whose truth checks passed


def _truth(case, build=True):
    M, D, dim = case["M"], case["D"], case["dim"]
    mant, e = _mant(case["values"], M)
    mean_int = None
    if case["mean"]:
        mean_int = np.random.default_rng(M + dim).integers(-2 ** 20, 2 ** 20, size=dim)
        assert (int(mant.sum()) + 2 ** 20) * M < 2 ** 53
    return rf.ExactSVD(M, D, dim, mant, e, seed=M * 7 + case["n"], mean_int=mean_int, build=build, coherent=case["coherent"])


def _sentinel_block(X, before, after=2):
    dim = X.shape[1]
    return np.vstack((np.full((before, dim), np.nan), X, np.full((after, dim), np.nan)))


def _device_block(ctx, case, t):
    """The block in a device buffer with x_row0 NaN rows in front and two behind."""
    M, dim, x0 = t.M, t.dim, case["x_row0"]
    if not case["device_build"]:
        return ctx.upload(_sentinel_block(t.X, x0))
    assert x0 == 0 and not case["mean"]
    Xb = ctx.alloc((M + 2) * dim).fill(np.nan)
    ctx.gemm_nn(M, dim, t.r, ctx.upload(t.F1), 0, t.r, ctx.upload(t.F2), 0, dim, Xb, 0, dim)   # exact (see ExactSVD)
    return Xb


def run_pod(ctx, case, t):
    """One device call.  Returns (sigma, info, V (v_row0 + n + 2, dim) with its sentinels, X after the call)."""
    n, dim, v0 = case["n"], t.dim, case["v_row0"]
    Xb = _device_block(ctx, case, t)
    Vb = ctx.alloc((v0 + n + 2) * dim).fill(np.nan)
    sig, info = ctx.pod(Xb, t.M, dim, n, Vb, center=case["center"], x_row0=case["x_row0"], v_row0=v0,
                        rel_floor=case["rel_floor"])
    return sig, info, Vb, Xb


def _floor(case):
    return max(case["rel_floor"], NOISE_FLOOR)


def check_truth(case, t, sig, info, V):
    """The assertions of the module docstring on one call's output (V: the n mode rows)."""
    cid, n = case["id"], case["n"]
    s = t.s
    s1 = s[0]
    fl = _floor(case)
    gram = info["gram_passes"] > 0
    # every true value, the zero ones included (rank < min(M, dim))
    zeros = min(t.M - (1 if case["center"] else 0), t.dim) - t.r
    s_all = np.concatenate([s, np.zeros(max(zeros, 0))])
    want_resolved = int(np.sum(s[:n] > fl * s1))
    assert info["resolved_modes"] == want_resolved and info["completed_modes"] == n - want_resolved, (cid, info)
    assert info["stop_reason"] == ("filled" if want_resolved == n else "floor"), (cid, info)
    for k, v in case["info"].items():
        assert info[k] == v, (cid, k, info)
    k = want_resolved
    st = np.concatenate([s, np.zeros(n)])[:n]
    rel = np.where(st >= 1e-6 * s1, 1e-10, 1e-5) * st
    if gram:
        rel = rel + 1e-14 * s1 ** 2 / np.maximum(st, 1e-300)
    observed(f"pod route {cid}: |sigma - s| / (C eps s_1 + rel)", np.abs(sig[:k] - st[:k]) / (C * EPS * s1 + rel[:k]), 1.0)
    assert np.all(sig[k:] == 0.0), (cid, sig[k:])
    # modes: isolated ones by angle, clusters by projector / span
    groups = []
    i = 0
    while i < k:
        j = i
        while j + 1 < len(s_all) and s_all[j + 1] == s_all[i]:
            j += 1
        groups.append((i, j + 1))
        i = j + 1
    ratios = []
    for lo, hi in groups:
        g_idx = np.arange(lo, hi)
        other = np.delete(s_all, g_idx)
        gap = np.min(np.abs(other - s_all[lo])) if other.size else s1
        gap2 = np.min(np.abs(other ** 2 - s_all[lo] ** 2)) if other.size else s1 ** 2
        bound = C * EPS * s1 / gap + C * EPS + (2e-14 * s1 ** 2 / gap2 if gram else 0.0)
        Vt = t.V[lo:hi]
        Vd = V[lo:min(hi, k)]
        if hi - lo == 1:
            c = Vd[0] @ Vt[0]
            ratios.append(np.linalg.norm(Vd[0] - c * Vt[0]) / bound)
        else:   # inside the cluster's span (a projector comparison when the cluster is complete)
            resid = Vd - (Vd @ Vt.T) @ Vt
            ratios.append(np.linalg.norm(resid, axis=1).max() / bound)
            if hi <= k:
                ratios.append(np.abs(Vd.T @ Vd - Vt.T @ Vt).max() / bound)
    if ratios:
        observed(f"pod route {cid}: mode angle / (C eps s_1 / gap [+ 2e-14 s_1^2 / gap2] + C eps)", np.array(ratios), 1.0)
    observed(f"pod route {cid}: orthonormality of the {n} rows", np.abs(V @ V.T - np.eye(n)) if n else np.zeros(1), 1e-13)
    piv = np.argmax(np.abs(V), axis=1)
    assert np.all(V[np.arange(n), piv] > 0), (cid, "svd_flip sign convention")
    if k < n:
        res = np.linalg.norm(t.F1[:t.M] @ (t.F2 @ V[k:].T), axis=0)     # X_c v through the exact factors
        observed(f"pod route {cid}: ||X_c v|| of the completed rows / (floor s_1 + C eps s_1)", res / (fl * s1 + C * EPS * s1), 1.0)


def _same_bits(a, b):
    return np.array_equal(np.asarray(a).view(np.uint64), np.asarray(b).view(np.uint64))


@pytest.fixture(scope="module")
def ctx():
    from romhighcontrast_amd import _ffi
    return _ffi.get_context()


@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_route_case(ctx, case, monkeypatch):
    t = _truth(case, build=not case["device_build"])
    n, dim, v0, x0 = case["n"], t.dim, case["v_row0"], case["x_row0"]
    sig, info, Vb, Xb = run_pod(ctx, case, t)
    Vall = Vb.download(shape=(v0 + n + 2, dim))
    assert np.isnan(Vall[:v0]).all() and np.isnan(Vall[v0 + n:]).all(), (case["id"], "mode sentinels")
    if not case["device_build"]:
        Xall = Xb.download(shape=(x0 + t.M + 2, dim))
        assert np.isnan(Xall[:x0]).all() and np.isnan(Xall[x0 + t.M:]).all(), (case["id"], "block sentinels")
        if case["center"]:   # the call leaves the centred block behind: exact here
            assert np.array_equal(Xall[x0:x0 + t.M], t.centred()), case["id"]
    V = Vall[v0:v0 + n]
    print(f"{case['id']}: {info}")
    check_truth(case, t, sig, info, V)
    # repeatability: the same bits again, and with the workspace poisoned
    sig2, info2, Vb2, _ = run_pod(ctx, case, t)
    assert _same_bits(sig2, sig) and Vb2.same_bits_as(Vb, Vb.n) and info2 == info, (case["id"], "repeat")
    monkeypatch.setenv("ROMHC_POISON_WS", "1")
    sig3, info3, Vb3, _ = run_pod(ctx, case, t)
    monkeypatch.delenv("ROMHC_POISON_WS")
    assert _same_bits(sig3, sig) and Vb3.same_bits_as(Vb, Vb.n) and info3 == info, (case["id"], "poisoned workspace")
    if "ahead_hit" in case["routes"]:
        # The ahead product has no witness outside the library (profiling turns it off).  What the case relies on, restated
        # from rom_pod_ex: worth_ahead (>= 64 MB, dim >= 1024, M >= 128); the first pass starts the product for pass 2 (n - want
        # >= 1 and n - 1 <= 96); a second pass ran; it has fewer than 96 modes left, so want <= 24 and it asks for
        # max(want + 8, 32) = 32 rows, the rows of the product
        want = min(n, max(24, n // 4))
        assert t.M * dim * 8 >= 64 << 20 and dim >= 1024 and t.M >= 128 and n - want >= 1 and n - 1 <= 96, case["id"]
        assert info["sketch_passes"] >= 2, (case["id"], info)
        # per-kernel profiling keeps everything on one stream (no product ahead): same kernels, same seeds, same bits
        ctx.profile(True)
        try:
            sig4, info4, Vb4, _ = run_pod(ctx, case, t)
        finally:
            ctx.profile(False)
        assert _same_bits(sig4, sig) and Vb4.same_bits_as(Vb, Vb.n), (case["id"], "with / without the ahead product")
    COVERED.update(case["routes"])


# ---- small and degenerate blocks (explicit centring, zeros, M = 1, dim = 1) ------------------------------------------
def _plain_call(ctx, X, n, center, v_row0=1):
    M, dim = X.shape
    Xb = ctx.upload(_sentinel_block(X, 2))
    Vb = ctx.alloc((v_row0 + n + 2) * dim).fill(np.nan)
    sig, info = ctx.pod(Xb, M, dim, n, Vb, center=center, x_row0=2, v_row0=v_row0)
    Vall = Vb.download(shape=(v_row0 + n + 2, dim))
    assert np.isnan(Vall[:v_row0]).all() and np.isnan(Vall[v_row0 + n:]).all()
    Xall = Xb.download(shape=(M + 4, dim))
    assert np.isnan(Xall[:2]).all() and np.isnan(Xall[2 + M:]).all()
    return sig, info, Vall[v_row0:v_row0 + n], Xall[2:2 + M]


def test_explicit_centring_and_degenerate_blocks(ctx):
    # n = 0: nothing but the centring, explicit; exact on an ExactSVD block with a mean row
    t = rf.ExactSVD(64, 64, 64, [9, 5, 3], 4, seed=1, mean_int=np.arange(64) - 20)
    sig, info, V, Xc = _plain_call(ctx, t.X, 0, True)
    assert np.array_equal(Xc, t.centred()) and info["resolved_modes"] == 0
    # M = 1: the centred row is zero; the one mode is completed
    x = np.arange(1.0, 51.0)[None, :]
    sig, info, V, Xc = _plain_call(ctx, x, 1, True)
    assert not Xc.any() and sig[0] == 0.0 and info["completed_modes"] == 1 and info["stop_reason"] == "floor", info
    assert abs(np.linalg.norm(V[0]) - 1) < 1e-14 and V[0][np.argmax(np.abs(V[0]))] > 0
    # dim = 1: the centred column, sigma = its norm, the mode is +1
    col = np.array([[3.0], [-1.0], [5.0], [1.0]])
    sig, info, V, Xc = _plain_call(ctx, col, 1, True)
    assert np.array_equal(Xc, col - 2.0) and V[0, 0] == 1.0 and info["resolved_modes"] == 1, info
    assert abs(sig[0] - np.sqrt(20.0)) <= 4 * EPS * np.sqrt(20.0), sig
    # a zero block with M > dim and n = min(M, dim): everything completed (rest = 30 <= 32: the fused kernels)
    sig, info, V, Xc = _plain_call(ctx, np.zeros((40, 30)), 30, True)
    assert not sig.any() and info["resolved_modes"] == 0 and info["completed_modes"] == 30 and info["stop_reason"] == "floor"
    observed("pod zero block 40 x 30: orthonormality of the completed rows", np.abs(V @ V.T - np.eye(30)), 1e-13)
    COVERED.update({"centre_explicit", "zero_block", "n_full", "m_gt_dim", "complete_fused"})


# ---- route confirmation in a child process (ROMHC_PROF_DETAIL is read once per process) -------------------------------
def test_routes_confirmed_by_profile_names():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, ROMHC_PROF_DETAIL="1")
    r = subprocess.run([sys.executable, os.path.join(root, "tests", "pod_routes_child.py")], env=env, cwd=root,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    out = r.stdout.decode(errors="replace")
    print(out)
    assert r.returncode == 0 and out.rstrip().endswith("OK"), out[-4000:]
    got = json.loads([ln for ln in out.splitlines() if ln.startswith("ROUTES ")][-1][7:])
    for case in CASES:
        conf = set(got[case["id"]])
        # routes that the profile cannot show (the ahead product is off under profiling; sentinels, cliff: by design)
        want = case["routes"] - {"ahead_hit", "row_offsets", "cliff", "n_full", "m_gt_dim"}
        assert want <= conf, (case["id"], sorted(want - conf), sorted(conf))
        if case["eig"]:   # the Gram eigen-routes a case takes, exactly
            assert conf & EIG_ROUTES == case["eig"], (case["id"], sorted(conf & EIG_ROUTES), sorted(case["eig"]))
    COVERED.add("_confirmed")


# ---- rom_pod_factored ---------------------------------------------------------------------------------------------------
_SM = {}


def _sm(blocks, N):
    from src.lib import SolutionsManagers as SM
    if (blocks, N) not in _SM:
        _SM[(blocks, N)] = SM.SolutionsManagerFEM(blocks, N)
    return _SM[(blocks, N)]


def _sweep_factored(sm, M, seed):
    from romhighcontrast_amd import factored
    ctx, fem = sm._ctx, sm._fem
    kb = fem.reduced_stride
    blocks = sm._fem.nrb, sm._fem.ncb
    a = 10.0 ** np.random.default_rng(seed).uniform(0, 2, size=(M, blocks[0] * blocks[1]))
    Y = ctx.alloc(M * kb)
    fem.solve_reduced(ctx.upload(a), M, Y)
    ctx.solve_status()
    fs = factored.FactoredSnapshots(sm, Y, M)
    return fs, fs.rows().numpy(), fs.Yc.download(M * fs.map.Kc, shape=(M, fs.map.Kc))


def _equilibration2(sm, Kc):
    """d_i^2 = ||expansion of compact unit vector i||_2^2 (the equilibration of the Euclidean energy map)."""
    from romhighcontrast_amd import factored
    em = factored.expansion_map(sm)
    B = sm._ctx.alloc(Kc * em.dim)
    em.expand_compact(sm._ctx.upload(np.eye(Kc)), Kc, B)
    Bh = B.download(Kc * em.dim, shape=(Kc, em.dim))
    return np.einsum("kd,kd->k", Bh, Bh)


PC_TOL = 1e-14


@pytest.mark.parametrize("blocks,N,M,n,center,c_row0,v_row0,claim", [
    ((1, 1), 8, 40, 6, True, 0, 0, "n>k2"),          # k2 = 1: completion past the map rank at once
    ((1, 1), 8, 1, 1, False, 2, 1, "M<=2"),
    ((2, 2), 16, 2, 2, True, 0, 0, "M<=2"),          # centred: rank 1
    ((2, 2), 16, 60, 40, False, 3, 2, ""),
    ((2, 2), 16, 60, 40, True, 0, 0, ""),
    ((2, 2), 16, 150, 120, False, 0, 3, "n>k2"),     # completion past the rank
    ((2, 2), 16, 20, 20, True, 1, 0, "n=M"),         # (n > M is refused by rom_pod_factored: n <= min(M, dim))
    ((3, 3), 40, 64, 48, True, 0, 0, "k2<Kc"),
    ((2, 2), 128, 1024, 40, True, 0, 0, "k2<Kc"),
])
def test_pod_factored_vs_lapack_and_rows(blocks, N, M, n, center, c_row0, v_row0, claim):
    """rom_pod_factored on sweep blocks against numpy.linalg.svd of the expanded rows and against rom_pod on the same rows.

    Bound (Weyl): the POD runs on Z = Yc E2; E2 drops the Schur complement below PC_TOL of the equilibrated Euclidean form
    and carries its factorisation rounding, so ||X - Z E2'||_F^2 <= (C Kc eps + (Kc - k2) PC_TOL) sum_m ||D y_m||^2 =: delta^2
    (D = diag d, d_i = the norm of the expanded compact unit vector i); with tol = delta + C eps s_1, |sigma_i - s_i| <= tol and
    a mode with gap g_i moves by <= tol / g_i (Wedin), plus C eps for forming the angle of two unit vectors in fp64.  The
    rows past the `rank` clearly resolved values (s > 1e3 tol) are orthogonal to the leading `rank` device modes, so
    ||X v|| <= ||X (I - P_dev)|| <= s_{rank+1} + s_1 ||P_dev - P_true|| <= s_{rank+1} + s_1 tol / (s_rank - s_{rank+1})."""
    sm = _sm(blocks, N)
    ctx, fem, dim = sm._ctx, sm._fem, sm.vspace_dim
    fs, U, Ych = _sweep_factored(sm, M, M * 3 + N)
    Kc = fs.map.Kc
    _, k2 = fs.map.build()
    holds = {"n>k2": n > k2, "k2<Kc": k2 < Kc, "n=M": n == M, "M<=2": M <= 2, "": True}[claim]
    assert holds, (claim, dict(n=n, M=M, k2=k2, Kc=Kc))
    Yc_use = Ych - Ych.mean(axis=0) if center else Ych
    d2 = _equilibration2(sm, Kc)
    delta = np.sqrt((C * Kc * EPS + max(Kc - k2, 0) * PC_TOL) * float(np.sum(Yc_use ** 2 @ d2)))
    X = U - U.mean(axis=0) if center else U
    _, s_ref, Vt = np.linalg.svd(X, full_matrices=False)
    s_ref = np.concatenate([s_ref, np.zeros(max(0, n - len(s_ref)))])
    Ybig = ctx.upload(np.vstack((np.full((c_row0, Kc), np.nan), Ych, np.full((2, Kc), np.nan))))
    Vb = ctx.alloc((v_row0 + n + 2) * dim).fill(np.nan)
    sig, info = fem.pod_factored(Ybig, M, n, Vb, center=center, c_row0=c_row0, v_row0=v_row0)
    Vall = Vb.download(shape=(v_row0 + n + 2, dim))
    assert np.isnan(Vall[:v_row0]).all() and np.isnan(Vall[v_row0 + n:]).all(), "mode sentinels"
    V = Vall[v_row0:v_row0 + n]
    assert info["completed_modes"] >= n - min(n, k2, M), (info, k2)   # past the map's rank: completed
    tag = f"pod_factored {blocks}/{N} M={M} n={n} centre={center} (Kc {Kc}, k2 {k2})"
    s1 = max(s_ref[0], 1e-300)
    tol = delta + C * EPS * s1
    observed(f"{tag}: |sigma - LAPACK| / (delta + C eps s_1), delta/s_1 = {delta / s1:.1e}", np.abs(sig - s_ref[:n]) / tol, 1.0)
    observed(f"{tag}: orthonormality", np.abs(V @ V.T - np.eye(n)), 1e-12)
    piv = np.argmax(np.abs(V), axis=1)
    assert np.all(V[np.arange(n), piv] > 0), "svd_flip sign convention"
    rank = int(np.sum(s_ref[:n] > 1e3 * tol))
    ang = []
    for i in range(rank):
        gap = np.min(np.abs(np.delete(np.concatenate([s_ref, [0.0]]), i) - s_ref[i]))
        c = V[i] @ Vt[i]
        ang.append(np.linalg.norm(V[i] - c * Vt[i]) / (tol / gap + C * EPS))
    if ang:
        observed(f"{tag}: mode angle vs LAPACK / (tol / gap + C eps)", np.array(ang), 1.0)
    # the rows past the resolved ones carry no variance beyond what the spectrum and the subspace error allow
    if rank < n:
        bound = s_ref[rank] + (s1 * tol / (s_ref[rank - 1] - s_ref[rank]) if rank else 0.0) + tol
        observed(f"{tag}: ||X v|| of the rows past the resolved ones / (s_(rank+1) + s_1 tol / gap_rank + tol)",
                 np.linalg.norm(X @ V[rank:].T, axis=0) / bound, 1.0)
    # against rom_pod on the downloaded rows
    Vr = ctx.alloc(n * dim)
    sig_r, _ = ctx.pod(ctx.upload(U), M, dim, n, Vr, center=center)
    observed(f"{tag}: |sigma - rom_pod on the rows| / (delta + 2 C eps s_1)", np.abs(sig - sig_r) / (tol + C * EPS * s1), 1.0)
    # repeatability
    Vb2 = ctx.alloc((v_row0 + n + 2) * dim).fill(np.nan)
    sig2, info2 = fem.pod_factored(Ybig, M, n, Vb2, center=center, c_row0=c_row0, v_row0=v_row0)
    assert _same_bits(sig2, sig) and Vb2.same_bits_as(Vb, Vb.n) and info2 == info


def test_route_table_is_covered():
    """Runs last in this module: every route of ROUTES was reached by a case whose truth checks passed, and the child
    confirmed the profiled ones.  It reads COVERED, which the tests above fill: a run of a subset of this module (-k, a
    single parametrised case) fails here by design; run the whole file."""
    missing = set(ROUTES) - COVERED
    assert not missing, sorted(missing)
    assert "_confirmed" in COVERED
