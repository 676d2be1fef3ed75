"""Route witness of tests/test_gpu_pod_routes.py: ROMHC_PROF_DETAIL is read once per process (static locals in
csrc/rom_ops.hip and csrc/rom_basis.hip), so the profiled reruns of the route cases run here, in a child process:

    ROMHC_PROF_DETAIL=1 python tests/pod_routes_child.py

Every case of CASES runs once with per-kernel profiling; the routes it took are read from the profile names (per-shape
GEMM names, pivchol_lowrank, jacobi_grid, small_eig, combine_rows, center_rows) and from info.  Prints one line
"ROUTES {json: case id -> routes}" and a last line "OK".  TEST INFRASTRUCTURE."""
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from romhighcontrast_amd import _ffi  # noqa: E402
import test_gpu_pod_routes as T  # noqa: E402

GEMM = re.compile(r"^(gemm_nn|gemm_nt)(?:_thin)?_(\d+)x(\d+)x(\d+)")


def routes_of(case, info, prof):
    M, dim, n = case["M"], case["dim"], case["n"]
    assert not (info["gram_passes"] and dim == M), "the Gram iteration's products are told from the sketch's by dim != M"
    names = {nm: rec for nm, rec in prof.items() if rec["launches"] > 0}
    gp, sp = info["gram_passes"], info["sketch_passes"]
    nn_block = nt_iter = 0
    pass_gemm = final_gemm = small_take = correction_gemm = False
    shapes = {(m.group(1), int(m.group(2)), int(m.group(3)), int(m.group(4))) for m in map(GEMM.match, names) if m}
    for nm, rec in names.items():
        m = GEMM.match(nm)
        if not m:
            continue
        op, a, b, k = m.group(1), int(m.group(2)), int(m.group(3)), int(m.group(4))
        if op == "gemm_nn" and b == dim and k == M:
            nn_block += rec["launches"]            # products with the block: (1 + power) per pass, 1 for the Gram lift
        if op == "gemm_nn" and b == dim and a > 64 and k > a:
            pass_gemm = True                       # the accepted rows of a pass with b > 64 rows, take > 64
        if op == "gemm_nn" and b == dim and a > 64 and k == a:
            final_gemm = True                      # the final rotation of found > 64 modes
        # <= 64 rows out of an inner size > 64 that is not the block's M, in dim space AND in M space (the completion's
        # products have no partner in M space): up to 512 the inner size is a pass's b (at most SE_MAX / 4 + 8) and the
        # product its accepted rows Rt Q, Rt Traw; above, it is `found` and the product a pass's correction Cc V, Cc Bt
        if op == "gemm_nn" and b == dim and a <= 64 < k and k != M and dim != M and ("gemm_nn", a, M, k) in shapes:
            if k <= 512:
                small_take = True
            else:
                correction_gemm = True
        if op == "gemm_nt" and b == M and k == M and dim != M:
            nt_iter += rec["launches"]             # Y G: a subspace-iteration step on the Gram matrix
    out = set()
    pilot = gp == 1 and sp == 0 and info["resolved_modes"] > 0
    if sp == 1 and gp == 0:
        out.add("one_pass")
    if sp >= 2:
        out.add("multi_pass")
    if "combine_rows" in names:
        out.add("combine_rows")
    if pass_gemm:
        out.add("pass_gemm")
    if small_take:
        out.add("pass_gemm_small_take")
    if correction_gemm:
        out.add("correction_gemm")
    if final_gemm:
        out.add("final_gemm")
    # the final Rayleigh-Ritz step of `found` rows off the one-workgroup kernel: three rounds of GEMM + small_eig on the
    # found x found Gram matrix (every other small_eig of that name and mode runs once per call)
    found = info["resolved_modes"]
    if names.get(f"small_eig_n{found}_mode0_gram", {}).get("launches", 0) >= 3:
        out.add("tall_svd_unfused")
    if gp and sp >= 1:
        out.add("gram")
    if pilot and nn_block == 2:
        out.add("pilot")
    # The branches of top_eigenpairs / lowrank_eigenpairs.  piv = launches of kp_pivchol_lowrank: 1 -- the first factor
    # (<= 32 steps, its small problem "small_eig" = kp_jacobi32_devn) ended by tolerance: accepted, or rejected by
    # LOWRANK_RESIDUAL (the general path follows); 2 -- the first factor gave up, the second (<= 96 steps) ran: if it ended
    # by tolerance, its rank-r problem runs once (small_eig_n{r}_mode0_gram) and, when accepted, the lift St Lt
    # (gemm_nn r x M x r); the general path is the subspace iteration (Y G products) and/or the whole-matrix Jacobi.
    piv = names.get("pivchol_lowrank", {}).get("launches", 0)
    full = "jacobi_grid" in names or f"small_eig_n{M}_mode0_gram" in names
    general = bool(nt_iter) or full
    ranks = [int(m.group(1)) for m in (re.match(r"^small_eig_n(\d+)_mode0_gram$", nm) for nm in names) if m]
    rank_once = [r for r in ranks if r != M and names[f"small_eig_n{r}_mode0_gram"]["launches"] % 3 != 0]
    lifted = [r for r in rank_once if f"gemm_nn_{r}x{M}x{r}" in names or f"gemm_nn_thin_{r}x{M}x{r}" in names]
    if gp:
        if piv == 1 and "small_eig" in names and not general:
            out.add("lowrank_first")
        if piv == 2 and lifted and not general:
            out.add("lowrank_second")
        if general and ((piv == 1 and "small_eig" in names) or (piv == 2 and rank_once and not lifted)):
            out.add("lowrank_rejected")
        if full and not nt_iter:
            out.add("full_eig_size")
        if full and nt_iter:
            out.add("full_eig_stall")
        if nt_iter and not full:
            out.add("subspace_iter_large" if M > 2048 else "subspace_iter")
    if nn_block - gp - 2 * sp - (1 if pilot else 0) >= 1:
        out.add("best_effort")
    if info["stop_reason"] == "floor":
        out.add("floor_rel" if case["rel_floor"] > T.NOISE_FLOOR else "floor")
    cr = names.get("center_rows")
    if cr:
        out.add("centre_sketch" if cr["flops"] == 1.0 * M * dim * cr["launches"] else "centre_explicit")
    rest = info["completed_modes"]
    if 1 <= rest <= 32 and found <= 512:
        out.add("complete_fused")
    if rest > 32:
        out.add("complete_general")
    # (found > 512 rules the fused completion out whatever `rest`: rom_complete_orthonormal's own correction, rest x dim x found)
    if 1 <= rest <= 32 and found > 512 and ("gemm_nn", rest, dim, found) in shapes:
        out.add("complete_general")
    return out, nn_block, nt_iter, piv


def main():
    assert os.environ.get("ROMHC_PROF_DETAIL")
    ctx = _ffi.get_context()
    got = {}
    for case in T.CASES:
        t = T._truth(case, build=not case["device_build"])
        ctx.profile(True)
        ctx.profile_reset()
        try:
            sig, info, Vb, _ = T.run_pod(ctx, case, t)
            prof = ctx.profile_report()
        finally:
            ctx.profile(False)
        r, nn_block, nt_iter, piv = routes_of(case, info, prof)
        got[case["id"]] = sorted(r)
        print(f"{case['id']}: {sorted(r)}  info {info}  block products {nn_block}, Gram iterations {nt_iter}, "
              f"pivchol {piv}", flush=True)
        print("   " + " ".join(sorted(nm for nm, rec in prof.items() if rec["launches"] > 0)), flush=True)
        del Vb
    print("ROUTES " + json.dumps(got), flush=True)


if __name__ == "__main__":
    main()
    print("OK")
