"""Witness of tests/test_gpu_pca_tall.py for the form a call takes: ROMHC_PROF_DETAIL is read once per process, so the
profiled calls run here, in a child process:

    ROMHC_PROF_DETAIL=1 python tests/pca_tall_child.py

One call at dim = 81 and one at dim = 300 with per-kernel profiling; the launches of the fused kernel, of the rotation
product and of the TN Gram kernel are counted from the profile names.  Prints "FORMS {json}" and a last line "OK".
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
    for M, dim in ((4096, 81), (4096, 300)):
        rng = np.random.default_rng(dim)
        X = rng.standard_normal((M, 24)) @ rng.standard_normal((24, dim)) * 10.0 ** -rng.uniform(0, 3, dim)
        Xb, Vb, Sb = ctx.upload(X), ctx.alloc(dim * dim), ctx.alloc(M * dim)
        ctx.profile(True)
        ctx.profile_reset()
        try:
            sig, info = ctx.pca_tall(Xb, M, dim, dim, Vb, S=Sb, center=True)
            prof = ctx.profile_report()
        finally:
            ctx.profile(False)
        names = {nm: rec["launches"] for nm, rec in prof.items() if rec["launches"] > 0}
        count = lambda prefix: sum(v for nm, v in names.items() if nm.startswith(prefix))  # noqa: E731
        got[str(dim)] = dict(passes=info["passes"], fused=count(f"pca_tall_fused_d{dim}"), rotate=count(f"pca_tall_rotate_d{dim}"),
                             syrk=count(f"syrk_tn_d{dim}"), reduce=count("syrk_tn_reduce"))
        print(f"dim {dim}: {info}\n   " + " ".join(f"{nm}:{v}" for nm, v in sorted(names.items())), flush=True)
    print("FORMS " + json.dumps(got), flush=True)


if __name__ == "__main__":
    main()
    print("OK")
