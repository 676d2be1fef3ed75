"""Witness of tests/test_gpu_poly_map.py for the kernels a fit launches: ROMHC_PROF_DETAIL is read once per process, so the
profiled calls run here, in a child process:

    ROMHC_PROF_DETAIL=1 python tests/poly_map_child.py

One fit + predict with one target group (q = 5) and one with two (q = 100: 96 + 4 columns) under per-kernel profiling; the
launches of the pass kernel per target group, of the prediction kernel and of every dense product of the library
(rom_gemm_*, the Gram product, k_syrk_tn) are counted from the profile names.  Prints "KERNELS {json}" and a last line "OK".
TEST INFRASTRUCTURE."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from romhighcontrast_amd import _ffi  # noqa: E402


def main():
    assert os.environ.get("ROMHC_PROF_DETAIL")
    ctx = _ffi.get_context()
    got = {}
    for m, d, M, q in ((4, 3, 1000, 5), (5, 2, 1000, 100)):
        rng = np.random.default_rng(q)
        X, Y = rng.uniform(-1, 1, (M, m)), rng.standard_normal((M, q))
        Xb, Yb, out = ctx.upload(X), ctx.upload(Y), ctx.alloc(M * q)
        P = len(_ffi.poly_terms(m, d))
        ctx.profile(True)
        ctx.profile_reset()
        try:
            pm = ctx.poly_fit(Xb, 0, m, m, Yb, 0, q, q, M, d)
            pm.predict(Xb, 0, m, M, OUT=out)
            prof = ctx.profile_report()
        finally:
            ctx.profile(False)
        names = {nm: rec["launches"] for nm, rec in prof.items() if rec["launches"] > 0}
        count = lambda prefix: sum(v for nm, v in names.items() if nm.startswith(prefix))  # noqa: E731
        groups = [min(96, q - c0) for c0 in range(0, q, 96)]
        got[f"q{q}"] = dict(passes=pm.info["passes"], pass_kernel=count("poly_pass"),
                            per_group=[names.get(f"poly_pass_P{P}_q{qg}", 0) for qg in groups],
                            predict=count(f"poly_predict_P{P}_q{q}"), gemm=count("gemm") + count("gram"), syrk_tn=count("syrk_tn"))
        print(f"q {q}: {pm.info}\n   " + " ".join(f"{nm}:{v}" for nm, v in sorted(names.items())), flush=True)
    print("KERNELS " + json.dumps(got), flush=True)


if __name__ == "__main__":
    main()
    print("OK")
