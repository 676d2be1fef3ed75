"""Timing of the greedy PBDW sensor selection (rom_sensor_greedy, rom_riesz_norms_h10) on the device.

  python tools/gpu_sensor_greedy.py [--out FILE] [--skip-host] [--kernel-stats CSV]

* C2 ((2,2), N = 128): all 65 025 interior vertices as candidates, an H^1_0 greedy basis of n = 20 from the 1024 C2
  parameters, m = 50 and 200, both modes; C4 ((3,3), N = 171) and C5 ((4,4), N = 256) with m = 50, both modes, all
  vertices as candidates, the basis from 256 parameters.  Call time: median of 3 after a warm-up (the call ends with
  its one host synchronisation; the clock starts on a synchronised stream).  Per-kernel HIP-event profile of one call,
  the per-step pass's bytes / s against the 8 TB/s HBM peak, and the table build alone (first call on a fresh FE space);
* host baseline (unless --skip-host): the same collective greedy in SciPy at C2 on a 2 000-candidate subset (splu of
  A_1, one solve per candidate for nu and one per pick for the Green row), with the GPU on the same subset;
* --kernel-stats: a `rocprofv3 --kernel-trace --stats` CSV of a separate run of this tool, merged into the output.
Prints one JSON document (and writes it to --out)."""
import argparse
import csv
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from romhighcontrast_amd import _ffi  # noqa: E402
from romhighcontrast_amd.lib import ReducedBasis as RB  # noqa: E402
from romhighcontrast_amd.lib.SolutionsManagers import SolutionsManagerFEM  # noqa: E402

HBM_PEAK = 8e12
CONFIGS = {"C2": ((2, 2), 128, 1024), "C4": ((3, 3), 171, 256), "C5": ((4, 4), 256, 256)}
MODES = {"collective": 0, "worst": 1}


def _median_ms(fn, reps=3):
    ctx = _ffi.get_context()
    fn()
    ts = []
    for _ in range(reps):
        ctx.synchronize()
        t0 = time.perf_counter()
        fn()
        ts.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(ts)), ts


def _profile(fn):
    ctx = _ffi.get_context()
    ctx.profile(True)
    ctx.profile_reset()
    fn()
    rep = ctx.profile_report()
    ctx.profile(False)
    return {k: {"ms": v["total_ms"], "launches": v["launches"], "flops": v["flops"], "bytes": v["bytes"]}
            for k, v in sorted(rep.items(), key=lambda kv: -kv[1]["total_ms"]) if v["launches"]}


def _basis(sm, M, n=20):
    rng = np.random.default_rng(20240807)
    a = 10.0 ** rng.uniform(0, 2, size=(M,) + tuple(sm.blocks_geometry))
    Ud = sm.generate_solutions_device(a)
    rb = RB.ReducedBasisGreedy(RB.GREEDY_FOR_H10).build(n, sm, Ud, a, sm.H10norm(Ud))
    return np.ascontiguousarray(rb.basis), Ud


def table_build(name):
    """The vertex-pair Green tables alone: the first norm call on a fresh FE space (sine tables included)."""
    blocks, N, _ = CONFIGS[name]
    sm = SolutionsManagerFEM(blocks, N)
    pts = sm.interior_vertices()[:1]
    prof = _profile(lambda: sm.riesz_norms_h10(pts))
    tab = {k: v for k, v in prof.items() if k.startswith(("sensor_pair", "sensor_tables", "riesz_sine"))}
    return {"config": name, "dim": sm.vspace_dim, "tables_ms": sum(v["ms"] for v in tab.values()), "profile": tab,
            "table_flops": sum(v["flops"] for v in tab.values())}


def greedy_cases(name, ms, once=False):
    blocks, N, M = CONFIGS[name]
    sm = SolutionsManagerFEM(blocks, N)
    C, _ = _basis(sm, M)
    n = C.shape[0]
    Cb = sm._ctx.upload(C)
    cand = sm.interior_vertices()
    loc = sm._locate(cand)
    out = []
    for m in ms:
        for mode, code in MODES.items():
            run = lambda: sm._fem.sensor_greedy(Cb, n, *loc, m, code, 1e-10)  # noqa: E731
            if once:
                run()
                continue
            rec = {"config": name, "dim": sm.vspace_dim, "ncand": len(cand), "n": n, "basis_params": M, "m": m, "mode": mode}
            rec["call_ms"], rec["call_ms_all"] = _median_ms(run)
            picks, crit, A, _, info = run()
            rec["info"] = info
            beta, _, _ = RB.sensor_beta_prefix(A[:info["picks"]], n - info["dead_rows"])
            rec["beta_at_m"] = float(beta[-1]) if beta.size else 0.0
            prof = _profile(run)
            rec["profile"] = prof
            st = prof.get("sensor_step")
            if st and st["ms"] > 0:
                rec["step_pass_ms"] = st["ms"]
                rec["step_pass_bytes"] = st["bytes"]
                rec["step_pass_TBps"] = st["bytes"] / (st["ms"] * 1e-3) / 1e12
                rec["step_pass_share_of_8TBps"] = st["bytes"] / (st["ms"] * 1e-3) / HBM_PEAK
                # Phi (m x ncand) and Res (n x ncand): the working set the passes sweep
                rec["working_set_MiB"] = 8.0 * (m + n + 2) * len(cand) / 2 ** 20
            out.append(rec)
    return out


def host_baseline(m=50, ncand=2000):
    """Collective greedy in SciPy on a candidate subset at C2, and the GPU on the same subset."""
    import scipy.sparse as sp
    import scipy.sparse.linalg as spla
    blocks, N, M = CONFIGS["C2"]
    sm = SolutionsManagerFEM(blocks, N)
    C, _ = _basis(sm, M)
    n = C.shape[0]
    nr, nc = sm.nr_inner_vertices, sm.nc_inner_vertices
    Tr = sp.diags([-np.ones(nr - 1), 2 * np.ones(nr), -np.ones(nr - 1)], [-1, 0, 1])
    Tc = sp.diags([-np.ones(nc - 1), 2 * np.ones(nc), -np.ones(nc - 1)], [-1, 0, 1])
    A1 = (sp.kron(Tr, sp.eye(nc)) + sp.kron(sp.eye(nr), Tc)).tocsc()
    V = sm.interior_vertices()
    sub = np.sort(np.random.default_rng(5).choice(len(V), ncand, replace=False))
    cand = V[sub]
    t0 = time.perf_counter()
    lu = spla.splu(A1)
    t1 = time.perf_counter()
    # W: CGS2 in the A_1 inner product; at vertex candidates r_x is a unit vector: w_i(x) = W[i, dof], nu_x = A_1^-1[x, x]
    W = C.copy()
    for i in range(n):
        for _ in range(2):
            W[i] -= (W[:i] @ (A1 @ W[i])) @ W[:i]
        W[i] /= np.sqrt(W[i] @ (A1 @ W[i]))
    E = W[:, sub].copy()                                   # Res at k = 0
    nu = np.empty(ncand)
    for j0 in range(0, ncand, 250):                        # one solve per candidate (blocks of 250 right-hand sides)
        Rb = np.zeros((nr * nc, min(250, ncand - j0)))
        Rb[sub[j0:j0 + 250], np.arange(Rb.shape[1])] = 1.0
        nu[j0:j0 + 250] = lu.solve(Rb)[sub[j0:j0 + 250], np.arange(Rb.shape[1])]
    t2 = time.perf_counter()
    Phi = np.zeros((m, ncand))
    picks = []
    Res = E
    mask = nu.copy()
    for k in range(m):
        c = np.where(mask > 0, np.sum(Res ** 2, axis=0) / np.where(mask > 0, mask, 1.0), 0.0)
        p = int(np.argmax(c))
        picks.append(p)
        L = Phi[:k, p].copy()
        lkk = np.sqrt(nu[p] - L @ L)
        a = Res[:, p] / lkk
        r = np.zeros(nr * nc)
        r[sub[p]] = 1.0
        g = lu.solve(r)[sub]                                # the Green row: one solve, evaluated at the candidates
        Phi[k] = (g - L @ Phi[:k]) / lkk
        Res = Res - np.outer(a, Phi[k])
        mask[p] = 0.0
    t3 = time.perf_counter()
    Cb = sm._ctx.upload(C)
    loc = sm._locate(cand)
    run = lambda: sm._fem.sensor_greedy(Cb, n, *loc, m, 0, 1e-10)  # noqa: E731
    gpu_ms, _ = _median_ms(run)
    gpicks = run()[0]
    return {"config": "C2", "ncand": ncand, "n": n, "m": m, "splu_ms": 1e3 * (t1 - t0),
            "basis_and_norms_ms": 1e3 * (t2 - t1), "greedy_ms": 1e3 * (t3 - t2), "total_ms": 1e3 * (t3 - t0),
            "gpu_same_subset_ms": gpu_ms, "picks_agree_with_gpu": int(np.sum(np.array(picks) == gpicks[:m]))}


def kernel_stats(path, top=16):
    rows = list(csv.DictReader(open(path)))
    rows.sort(key=lambda r: -float(r["TotalDurationNs"]))
    return [{"name": r["Name"][:160], "calls": int(r["Calls"]), "total_ms": float(r["TotalDurationNs"]) * 1e-6,
             "avg_us": float(r["AverageNs"]) * 1e-3, "percent": float(r["Percentage"])} for r in rows[:top]]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--skip-host", action="store_true")
    ap.add_argument("--once", action="store_true", help="one call per case, nothing timed (for a rocprofv3 run)")
    ap.add_argument("--kernel-stats", default=None)
    args = ap.parse_args()
    if args.once:
        greedy_cases("C2", (50, 200), once=True)
        greedy_cases("C4", (50,), once=True)
        return
    res = {"device": _ffi.get_context().device_name(), "hbm_peak_TBps": HBM_PEAK / 1e12}
    res["tables"] = [table_build(c) for c in ("C2", "C4", "C5")]
    res["greedy"] = greedy_cases("C2", (50, 200)) + greedy_cases("C4", (50,)) + greedy_cases("C5", (50,))
    if not args.skip_host:
        res["host_baseline"] = host_baseline()
    if args.kernel_stats:
        res["kernel_stats"] = kernel_stats(args.kernel_stats)
    txt = json.dumps(res, indent=1)
    print(txt)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(txt + "\n")


if __name__ == "__main__":
    main()
