"""Route witness of tests/test_gpu_small_dense.py: ROMHC_PROF_DETAIL is read once per process, so the profiled calls happen
here.  Run by the test in a subprocess:

    ROMHC_PROF_DETAIL=1 python tests/small_dense_child.py

For every order of small_dense_truth.ORDERS and every mode it serves, one ctx.small_eig call with profiling on and one line

    ROUTE {"n": ..., "mode": ..., "gram_like": ..., "profile_says": "grid" | "one_workgroup" | "pivchol", "names": [...]}

from the names of the profile records: `jacobi_grid` (one launch per round), `small_eig_n<N>_mode<M>_<gram|sym>` (one
workgroup: kb_jacobi32 or kb_small_eig -- the names cannot tell those two apart) or `pivchol_whiten`.  Exit code 0 and a last
line "OK" on success.  TEST INFRASTRUCTURE."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from romhighcontrast_amd import _ffi  # noqa: E402
import small_dense_truth as sd  # noqa: E402


def main(ctx):
    assert os.environ.get("ROMHC_PROF_DETAIL")
    ctx.profile(True)
    for n in sd.ORDERS:
        A = sd.ExactCase(n, "distinct").A
        for mode in (0, 1, 2, 3):
            if mode == 3 and n > sd.LDS_MAX:
                continue
            gl = 0 if mode == 0 and n % 2 else 1
            ctx.profile_reset()
            ctx.small_eig(A, mode=mode, rel_tol=0.0, gram_like=gl)
            names = sorted(nm for nm, rec in ctx.profile_report().items() if rec["launches"] > 0)
            one = f"small_eig_n{n}_mode{mode}_{'gram' if gl else 'sym'}"
            says = [k for k, nm in (("grid", "jacobi_grid"), ("one_workgroup", one), ("pivchol", "pivchol_whiten")) if nm in names]
            assert len(says) == 1, (n, mode, names)
            assert not any(nm.startswith("small_eig") and nm != one for nm in names), (n, mode, names)
            print("ROUTE " + json.dumps({"n": n, "mode": mode, "gram_like": gl, "profile_says": says[0], "names": names}), flush=True)
    ctx.profile(False)


if __name__ == "__main__":
    main(_ffi.get_context())
    print("OK")
