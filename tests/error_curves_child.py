"""Route witness of tests/test_gpu_error_curves.py: ROMHC_PROF_DETAIL is read once per process, so the profiled runs of
the route cases happen here, in a child process:

    ROMHC_PROF_DETAIL=1 python tests/error_curves_child.py

Every case of CHILD_CASES runs rom_error_curves once with per-kernel profiling; the routes it took are read from the
profile names (curves_pass_nc8/16/32, curves_galerkin_lds/global) and the number of passes from info.  Prints one line
"ROUTES {json: case id -> {want, seen}}" and a last line "OK".  TEST INFRASTRUCTURE."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

from romhighcontrast_amd import _ffi  # noqa: E402
import test_gpu_error_curves as T  # noqa: E402


def main():
    ctx = _ffi.get_context()
    sm, a, U = T._snapshots((1, 3), 8, 300, 1e2, seed=11)
    rng = np.random.default_rng(2)
    out = {}
    for cid, N, gal in T.CHILD_CASES:
        C = rng.standard_normal((N, sm.vspace_dim))
        ctx.profile(True)
        ctx.profile_reset()
        try:
            _, _, _, _, info = T._run(ctx, sm, U, C, a if gal else None)
            prof = ctx.profile_report()
        finally:
            ctx.profile(False)
        names = {nm for nm, rec in prof.items() if rec["launches"] > 0}
        seen = set()
        for nc in (8, 16, 32):
            if f"curves_pass_nc{nc}" in names:
                seen.add(f"pass_nc{nc}")
        if prof.get("curves_pass_nc32", {}).get("launches", 0) + prof.get("curves_pass_nc16", {}).get("launches", 0) \
                + prof.get("curves_pass_nc8", {}).get("launches", 0) >= 2 and info["passes"] >= 2:
            seen.add("multi_pass")
        if "curves_galerkin_lds" in names:
            seen.add("galerkin_lds")
        if "curves_galerkin_global" in names:
            seen.add("galerkin_global")
        if not gal and not names & {"curves_galerkin_lds", "curves_galerkin_global"}:
            seen.add("no_galerkin")
        out[cid] = {"want": sorted(T.routes_of(N, info, gal)), "seen": sorted(seen)}
    print("ROUTES " + json.dumps(out))
    print("OK")


if __name__ == "__main__":
    main()
