"""Route witness of tests/test_gpu_sweep.py: ROMHC_PROF_DETAIL is read once per process, so the profiled sweeps happen
here, in a child process:

    ROMHC_PROF_DETAIL=1 python tests/sweep_child.py

Every case of sweep_truth.CASES sweeps its smallest batch and 129 systems with per-kernel profiling; the routes are read
from the ROM_PROF labels (solve1, rhs, diag_update_jNN, ..., extend_lr; sweep_truth.routes_of_profile adds what the labels
cannot tell -- the tiling of k_extend128, its launch count -- from the restated decision and the block counts that
ROMHC_VERBOSE prints when the FE space is created).  Then the four product switches: more than 2048 systems, 1921 systems
of 3x3-N140 (k_extend128 in the system-fast workgroup order: the label extend_lr_sysfast), a workspace limit of 70 systems, a
sweep of 700 after one of 256 on the same FE space (the number of chunks is the launch count of the first kernel).  Prints
one line "ROUTES {json: id -> {want, seen, want_small, seen_small, ...}}" and a last line "OK".  TEST INFRASTRUCTURE."""
import json
import os
import re
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

from romhighcontrast_amd import _ffi  # noqa: E402
import sweep_truth as st  # noqa: E402


def create_verbose(ctx, case):
    """(_ffi.Fem, what ROMHC_VERBOSE printed while it was created)."""
    sys.stderr.flush()
    with tempfile.TemporaryFile() as tf:
        saved = os.dup(2)
        os.dup2(tf.fileno(), 2)
        os.environ["ROMHC_VERBOSE"] = "1"
        try:
            fem = _ffi.Fem(ctx, case.blocks[0], case.blocks[1], case.N)
        finally:
            del os.environ["ROMHC_VERBOSE"]
            os.dup2(saved, 2)
            os.close(saved)
        tf.seek(0)
        text = tf.read().decode(errors="replace")
    return fem, text


def profiled_sweep(ctx, fem, case, M):
    """{ROM_PROF label: launches} of one sweep of M systems."""
    a = ctx.upload(st.params(case)[st.idx_pattern(M, st.n_params(case))])
    U = ctx.alloc(M * fem.dim)
    ctx.profile(True)
    ctx.profile_reset()
    try:
        fem.solve_batch(a, M, U)
        prof = ctx.profile_report()
    finally:
        ctx.profile(False)
    return {nm: rec["launches"] for nm, rec in prof.items() if rec["launches"] > 0}


def first_kernel_launches(prof):
    return max(prof.get("solve1", 0), prof.get("rhs", 0))


def main():
    ctx = _ffi.get_context()
    out = {}
    for case in st.CASES:
        fem, text = create_verbose(ctx, case)
        m = re.search(r"128-tile kernel: (\d+), general kernel: (\d+)", text)
        n_lr = int(m.group(1)) if m else 0
        n1 = case.N - 1
        small = min(case.Ms)
        p_small = profiled_sweep(ctx, fem, case, small)
        p_129 = profiled_sweep(ctx, fem, case, 129)
        expands = "expand" in p_small
        out[case.id] = {"want": sorted(case.routes), "want_small": sorted(st.narrow_routes(case.routes)), "seen": sorted(st.routes_of_profile(p_129, n1, 129, n_lr, expands)),
                        "seen_small": sorted(st.routes_of_profile(p_small, n1, small, n_lr, expands)), "small": small,
                        "n_tiles": fem.n_tiles, "n_lr_blocks": n_lr, "profile": sorted(p_129), "profile_small": sorted(p_small)}
    # the product switches
    case = st.CASE[st.BIG_CASE]
    fem, _ = create_verbose(ctx, case)
    p = profiled_sweep(ctx, fem, case, st.BIG_M)
    out["big"] = {"seen": sorted(st.routes_of_profile(p, case.N - 1, st.BIG_M, 0, True)), "launches": first_kernel_launches(p)}
    case = st.CASE[st.SYS_FAST_CASE]
    fem, text = create_verbose(ctx, case)
    m = re.search(r"128-tile kernel: (\d+), general kernel: (\d+)", text)
    p = profiled_sweep(ctx, fem, case, st.SYS_FAST_M)
    out["sys_fast"] = {"seen": sorted(st.routes_of_profile(p, case.N - 1, st.SYS_FAST_M, int(m.group(1)) if m else 0, True)),
                       "profile": sorted(p), "M": st.SYS_FAST_M, "launches": first_kernel_launches(p)}
    del fem
    for cid in st.CHUNK_CASES:
        case = st.CASE[cid]
        fem, _ = create_verbose(ctx, case)
        per_sys = st.per_system_workspace(fem.n_tiles, st.nodal_part(fem)[0], fem.reduced_stride)
        ctx.set_workspace_limit(70 * per_sys)
        try:
            p = profiled_sweep(ctx, fem, case, 257)
        finally:
            ctx.set_workspace_limit(24 << 30)
        seen = ["chunked"] if first_kernel_launches(p) == len(st.chunks_of(257, 70)) else []
        out[f"chunked {cid}"] = {"seen": seen, "launches": first_kernel_launches(p)}
        fem, _ = create_verbose(ctx, case)
        p256 = profiled_sweep(ctx, fem, case, 256)
        p700 = profiled_sweep(ctx, fem, case, 700)
        seen = ["chunk_reuse"] if first_kernel_launches(p256) == 1 and first_kernel_launches(p700) == len(st.chunks_of(700, 256)) else []
        out[f"chunk_reuse {cid}"] = {"seen": seen, "launches": [first_kernel_launches(p256), first_kernel_launches(p700)]}
    print("ROUTES " + json.dumps(out))
    print("OK")


if __name__ == "__main__":
    main()
