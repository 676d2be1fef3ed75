"""Route witness of tests/test_gpu_sensor_truth.py: ROMHC_PROF_DETAIL is read once per process, so the profiled runs of
the route cases happen here, in a child process:

    ROMHC_PROF_DETAIL=1 python tests/sensor_child.py

Every case of CHILD_CASES runs rom_sensor_greedy once with per-kernel profiling; what the names can show is read from
the profile: the launch counts of sensor_select / sensor_step / sensor_prep and, in the worst-case mode, of the
eigen-solver under the name of its order (small_eig_n<n>_mode0_gram).  The size case of the split representer transform
runs once: two riesz_transform_c launches behind one riesz_spectral.  Prints one line "ROUTES {json: case -> {want,
seen}}" and a last line "OK".  TEST INFRASTRUCTURE."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import h10_truth as ht  # noqa: E402
import sensor_truth as st  # noqa: E402
import test_gpu_sensor_truth as T  # noqa: E402


def profiled(ctx, fn):
    ctx.profile(True)
    ctx.profile_reset()
    try:
        out = fn()
        prof = ctx.profile_report()
    finally:
        ctx.profile(False)
    return out, {nm: rec["launches"] for nm, rec in prof.items() if rec["launches"] > 0}


def main():
    out = {}
    for cid, mode in T.CHILD_CASES:
        case = st.CASES[cid]
        sm = T._sm(*case["grid"])
        gr, Cm, cand = st.case_inputs(case)
        Cb = sm._ctx.upload(Cm)
        res, seen = profiled(sm._ctx, lambda: sm._fem.sensor_greedy(Cb, len(Cm), *st.locate(gr, cand), case["m"], mode, case["rel_tol"]))
        assert res[4]["picks"] == case["m"], (cid, res[4])
        out[f"{cid}-{st.MODES[mode]}"] = {"want": T.child_expectations(case, mode), "seen": seen}
    gr, sm = ht.grid(*st.SIZE_GRID), T._sm(*st.SIZE_GRID)
    _, seen = profiled(sm._ctx, lambda: T.run_split(sm, gr)[1])
    out["split"] = {"want": {"riesz_transform_c": 2, "riesz_spectral": 1}, "seen": seen}
    print("ROUTES " + json.dumps(out))
    print("OK")


if __name__ == "__main__":
    main()
