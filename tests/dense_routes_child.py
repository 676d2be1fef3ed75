"""Checks of the dense primitives that need a process of their own: ROMHC_PROF_DETAIL and ROMHC_NO_THIN_GEMM are read once
per process (static locals in csrc/rom_ops.hip).  Run by tests/test_gpu_dense_ops.py in a subprocess:

    ROMHC_PROF_DETAIL=1 python tests/dense_routes_child.py routes     every route of the table, confirmed by profile names
    ROMHC_NO_THIN_GEMM=1 python tests/dense_routes_child.py general   the exact cases on the 64 x 64 engines + a rom_pod
                                                                      whose ahead product splits K

exit code 0 and a last line "OK" on success.  TEST INFRASTRUCTURE."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from romhighcontrast_amd import _ffi  # noqa: E402
import test_gpu_dense_ops as T  # noqa: E402


def expected_names(case, r):
    """Profile records the route must leave (ROM_PROF names with ROMHC_PROF_DETAIL), and whether it reduces partials."""
    op, m, n, k, _ = case
    route, s = r["route"], r["splits"]
    if route == "nt_thin":
        return [f"gemm_nt_thin_{m}x{n}x{k}_s{s}"], True
    if route == "nt_thin_T":
        return [f"gemm_nt_thin_{n}x{m}x{k}_s{s}"], True
    if route.startswith("nt_general"):
        return [f"gemm_nt_{m}x{n}x{k}_s{s}"], s > 1
    if route == "gram_lower":
        return [f"gram_{m}x{m}x{k}_s{s}", "mirror_lower"], s > 1
    if route == "gram128":
        return ["gram128", "gram128_finish"], False
    if route in ("nn_thin", "nn_lift"):
        return [f"gemm_nn_thin_{m}x{n}x{k}"], False
    if route == "nn_general":
        return [f"gemm_nn_{m}x{n}x{k}"], s > 1
    raise AssertionError(route)


def routes(ctx):
    assert os.environ.get("ROMHC_PROF_DETAIL") and not os.environ.get("ROMHC_NO_THIN_GEMM")
    ctx.profile(True)
    for case in T.ROUTE_CASES:
        r = T.route_of(case)
        ctx.profile_reset()
        msg = T.check_exact(ctx, case, T.BETA, seed=T.case_seed(case))
        assert msg is None, msg
        names = {nm for nm, rec in ctx.profile_report().items() if rec["launches"] > 0}
        want, reduces = expected_names(case, r)
        for nm in want:
            assert nm in names, (case, r, nm, sorted(names))
        assert ("splitk_reduce" in names) == reduces, (case, r, sorted(names))
        print(f"{T.case_id(case)}: {r['route']}/{r['reducer']} s={r['splits']}  {sorted(names)}", flush=True)
    ctx.profile(False)


def pod_with_ahead_product(ctx):
    """M = 8192, dim = 1024 (64 MB: the second pass's first product is started ahead on the auxiliary stream), 50 modes of a
    spectrum decaying like 10^(-i / 5): at least two sketch passes.  Against LAPACK as test_pod_fuzz_vs_lapack."""
    M, dim, n = 8192, 1024, 50
    rng = np.random.default_rng(8192)
    s = 10.0 ** (-np.arange(dim) / 5.0)
    Q1, _ = np.linalg.qr(rng.standard_normal((M, dim)))
    Q2, _ = np.linalg.qr(rng.standard_normal((dim, dim)))
    X = (Q1 * s) @ Q2.T
    sv = np.linalg.svd(X, compute_uv=False)
    V = ctx.alloc(n * dim)
    sig, info = ctx.pod(ctx.upload(X), M, dim, n, V, center=False)
    assert info["sketch_passes"] >= 2, info
    comps = V.download(shape=(n, dim))
    noise = 50 * 1.1e-16 * np.linalg.norm(X, 2)
    err = np.abs(sig - sv[:n]) / (1e-7 * sv[:n] + noise)
    assert err.max() <= 1.0, (float(err.max()), int(err.argmax()), info)
    orth = np.abs(comps @ comps.T - np.eye(n)).max()
    assert orth < 1e-12, (orth, info)
    print(f"pod {M}x{dim}, {n} modes: {info['sketch_passes']} sketch passes, worst {err.max():.2e} of the bound, "
          f"orthonormality {orth:.1e}", flush=True)


def general(ctx):
    assert os.environ.get("ROMHC_NO_THIN_GEMM") and not os.environ.get("ROMHC_PROF_DETAIL")
    for case, beta in T.EXACT_PARAMS:
        r = T.route_of(case, no_thin=True)
        assert r["route"] not in ("nt_thin", "nt_thin_T", "nn_thin", "nn_lift"), (case, r)
        msg = T.check_exact(ctx, case, beta, seed=T.case_seed(case))
        assert msg is None, f"{msg}  route {r}"
    print(f"{len(T.EXACT_PARAMS)} exact cases on the general engines: equal", flush=True)
    pod_with_ahead_product(ctx)


if __name__ == "__main__":
    job = sys.argv[1] if len(sys.argv) > 1 else ""
    ctx = _ffi.get_context()
    {"routes": routes, "general": general}[job](ctx)
    print("OK")
