"""Timing of the model selection among local reduced spaces (rom_local_select) beside rom_bvls and the NumPy specification, the
compiler's resource report of its kernels, and the experiment it was built for.

  python tools/gpu_local_select.py [--out profiles/local_select.json] [--reps 10] [--spec-vectors 4]
  python tools/gpu_local_select.py --resources profiles/local_select_resources.txt      (no GPU: compiles the file)
  python tools/gpu_local_select.py --trace        (the timed calls only, for rocprofv3 --kernel-trace --stats -- python ...)
  python tools/gpu_local_select.py --kernel-stats DB CSV    (no GPU: the dispatches in rocprofv3's database of such a run, as CSV)

* rom_local_select for K = 1024 measurement vectors at kc = 16, (n, k, rank) = (8, 4, 33) and (32, 9, 289), and kc = 64 at
  (8, 4, 33), r = n, on the synthetic construction of tests/local_select_truth.py.  The whole call between HIP events on the
  context stream (its three launches, its one synchronisation, the download of the labels and counters and the Python wrapper's
  download of OUT included, as for rom_bvls below; the upload of P is outside), median of --reps after one untimed call.
* beside each, in the same run, two yardsticks of the state solve alone.  A: rom_bvls on the SAME K kc state systems, one call
  per cluster with G_j and the box of cluster j (kc calls of K systems, timed together; the passes must equal those of the state
  solves, which is recorded).  B: ONE rom_bvls call on K kc systems of the same distribution (a one-cluster case of the same
  generator), with its passes -- the call that compares launch for launch.  Then the same rom_local_select call with the
  residual tables cut to rank = k rows (what remains when steps 2 and 3 have next to nothing to read); the kernels' times from
  the library's own event brackets (runs of their own, after the timed ones) and from them the time per factorisation of
  k_local_fit and of k_bvls, and the estimate "k_bvls's time per factorisation x the factorisations of this call's state
  solves", over which k_local_fit's time is the cost of a whole system in units of its state solve (B's systems take another
  number of passes than this call's, so the plain ratio of the two kernels says little); the NumPy specification on the first --spec-vectors vectors by wall clock, scaled to K (NOT
  measured at K).
* the experiment end to end: (2, 2) blocks, N = 8, 600 parameters a ~ U(1, 100) (default_rng(42)), rows 100.. training, rows
  0..99 held out, kc = 4 clusters of dimension 6, 24 sensors at interior vertices (default_rng(3)), noise-free measurements,
  a_box = "global" and "cluster": the share of held-out rows whose label is classify(a_true), and the rms H^1_0 errors of the
  selected estimate, of the estimate in the cluster of a_true, of the best cluster per row, and of the global POD basis of
  the same dimension.
Not measured: other K, hardware counters, the time of LocalReducedBasis.observe.
Prints one JSON document (and writes it to --out)."""
import argparse
import json
import os
import re
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONFIGS = [(16, 8, 4, 33), (16, 32, 9, 289), (64, 8, 4, 33)]   # (kc, n, k, rank), r = n
K_VECTORS = 1024


def _events_median(ctx, fn, reps):
    ts = []
    for i in range(reps + 1):
        ctx.synchronize()
        ctx.timer_start()
        fn()
        t = ctx.timer_stop()
        if i >= 1:
            ts.append(t)
    return float(np.median(ts)), float(np.min(ts)), float(np.max(ts))


def synthetic(n, k, rank, r, kc, K, seed=0):
    """tests/local_select_truth.py::make_case (the generator of the tests, imported so that the two cannot drift apart)."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from local_select_truth import make_case
    return make_case(n, k, rank, r, kc, K, seed=seed)


def measure(ctx, kc, n, k, rank, reps, spec_vectors, trace_only=False):
    from romhighcontrast_amd.inverse import local_select_host
    r, K = n, K_VECTORS
    cs = synthetic(n, k, rank, r, kc, K)
    RT, GR, P, c_lo, c_hi, a_lo, a_hi = cs.args()
    dRT, dGR, dP = ctx.upload(RT), ctx.upload(GR), ctx.upload(P)
    OUT = ctx.alloc(K * kc * (n + k + 5))
    call = lambda: ctx.local_select(kc, n, k, rank, r, dRT, dGR, dP, 0, kc * r, K, c_lo, c_hi, a_lo, a_hi, OUT=OUT)  # noqa: E731
    # yardstick A, the SAME state systems: rom_bvls once per cluster, with G_j and the box of cluster j on its K columns of P
    dG = [ctx.upload(GR[j]) for j in range(kc)]
    OUT1 = ctx.alloc(K * kc * (n + 4))

    def bvls_same():
        return [ctx.bvls(n, r, dG[j], dP, j * r, kc * r, K, c_lo[j], c_hi[j], OUT=OUT1, out_off=j * K * (n + 4), bound=False) for j in range(kc)]
    # yardstick B, ONE rom_bvls call on K kc systems of the same distribution: a one-cluster case of the same generator
    one = synthetic(n, k, k, r, 1, K * kc, seed=2)
    dG1, dP1 = ctx.upload(one.GR[0]), ctx.upload(one.P)
    bvls_one = lambda: ctx.bvls(n, r, dG1, dP1, 0, r, K * kc, one.c_lo[0], one.c_hi[0], OUT=OUT1, bound=False)  # noqa: E731
    # the tables cut to rank = k rows
    dRTk = ctx.upload(np.ascontiguousarray(RT[:, :k]))
    floor = lambda: ctx.local_select(kc, n, k, k, r, dRTk, dGR, dP, 0, kc * r, K, c_lo, c_hi, a_lo, a_hi, OUT=OUT)  # noqa: E731
    if trace_only:
        for fn in (call, bvls_one, floor):
            fn()
            fn()
        return None
    med, tmin, tmax = _events_median(ctx, call, reps)
    s_med, s_min, s_max = _events_median(ctx, bvls_same, reps)
    b_med, b_min, b_max = _events_median(ctx, bvls_one, reps)
    f_med, f_min, f_max = _events_median(ctx, floor, reps)
    res, info = call()
    same = bvls_same()
    same_passes = int(sum(i["passes"] for _, i in same))
    same_equal = bool(all(np.array_equal(rj.iterations, res.passes[:, j, 0]) for j, (rj, _) in enumerate(same)))
    _, b_info = bvls_one()
    ctx.profile(True)
    ctx.profile_reset()
    for _ in range(3):
        call()
    kernels = {name: rec["total_ms"] / rec["launches"] for name, rec in ctx.profile_report().items() if name.startswith("local_select")}
    ctx.profile_reset()
    for _ in range(3):
        bvls_one()
    kernels.update({name: rec["total_ms"] / rec["launches"] for name, rec in ctx.profile_report().items() if name.startswith("bvls")})
    ctx.profile(False)
    rows = min(spec_vectors, K)
    t0 = time.perf_counter()
    host = local_select_host(RT, GR, P[:rows], c_lo, c_hi, a_lo, a_hi)
    spec_ms = 1e3 * (time.perf_counter() - t0)
    systems = K * kc
    state_passes, param_passes = int(res.passes[:, :, 0].sum()), int(res.passes[:, :, 1].sum())
    fit_ms = [v for q, v in kernels.items() if q.startswith("local_select_fit")][0]
    bvls_ms = [v for q, v in kernels.items() if q.startswith("bvls") and q != "bvls_gram"][0]
    return {"kc": kc, "n": n, "k": k, "rank": rank, "r": r, "K": K, "systems": systems, "reps": reps,
            "call_ms_median": med, "call_ms_min": tmin, "call_ms_max": tmax, "us_per_system": 1e3 * med / systems,
            "passes_state": state_passes, "passes_param": param_passes, "factorisations": info["factorisations"],
            "passes_state_mean": state_passes / systems, "passes_param_mean": param_passes / systems,
            "bvls_same_systems": {"calls": kc, "ms_median": s_med, "ms_min": s_min, "ms_max": s_max, "passes": same_passes,
                                  "passes_equal_state_solves": same_equal, "ratio_select_over_it": med / s_med},
            "bvls_one_call": {"ms_median": b_med, "ms_min": b_min, "ms_max": b_max, "passes": b_info["passes"],
                              "passes_mean": b_info["passes"] / systems, "ratio_select_over_it": med / b_med,
                              "kernel_ms_profiled": bvls_ms, "kernel_ratio_fit_over_it": fit_ms / bvls_ms,
                              "kernel_us_per_factorisation": 1e3 * bvls_ms / b_info["factorisations"]},
            "fit_kernel_us_per_factorisation": 1e3 * fit_ms / info["factorisations"],
            # what k_bvls would take for the state solves of this call at yardstick B's time per factorisation (a solve factors
            # once for its start and once per pass), and k_local_fit over it: an estimate, the one figure here that is not timed
            "state_solves_kernel_ms_estimate": bvls_ms / b_info["factorisations"] * (state_passes + systems),
            "fit_kernel_over_state_solves_estimate": fit_ms / (bvls_ms / b_info["factorisations"] * (state_passes + systems)),
            "rank_k_call_ms_median": f_med, "rank_k_call_ms_min": f_min, "rank_k_call_ms_max": f_max,
            "kernel_ms_profiled": kernels, "info": info,
            "status_nonzero": int((res.status != 0).sum()), "table_bytes_per_cluster": 8 * rank * (1 + k * n),
            "spec_vectors": rows, "spec_ms_per_system": spec_ms / (rows * kc), "spec_ms_scaled_to_K": spec_ms / rows * K,
            "spec_scaled_over_device": spec_ms / rows * K / med,
            "labels_equal_spec": bool(np.array_equal(res.labels[:rows], host.labels)),
            "passes_equal_spec": bool(np.array_equal(res.passes[:rows], host.passes)),
            "max_abs_S_device_minus_spec": float(np.abs(res.surrogate_all[:rows] - host.surrogate_all).max())}


def kernel_stats(db_path, csv_path):
    """Every dispatch of the kernels of rom_local_select and rom_bvls in a database written by
    `rocprofv3 --kernel-trace --stats -d DIR -o NAME -- python tools/gpu_local_select.py --trace` (DIR/NAME_results.db, rocprofv3's
    rocpd format: its view `kernels`), in time order, as CSV: dispatch, kernel, workgroups x, y, threads, LDS bytes, duration ns."""
    import csv
    import sqlite3
    db = sqlite3.connect(db_path)
    rows = db.execute("select name, grid_x / workgroup_x, grid_y, workgroup_x, lds_size, duration from kernels "
                      "where name like '%k_local_%' or name like '%k_bvls%' order by start").fetchall()
    with open(csv_path, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["dispatch", "kernel", "workgroups_x", "workgroups_y", "threads", "lds_bytes", "duration_ns"])
        for i, row in enumerate(rows):
            w.writerow([i, row[0].replace("(anonymous namespace)::", "").split("(")[0], *row[1:]])
    print(f"{len(rows)} dispatches -> {csv_path}")


def experiment():
    from romhighcontrast_amd.lib.ReducedBasis import ReducedBasisPCA
    from romhighcontrast_amd.lib.SolutionsManagers import SolutionsManagerFEM
    from romhighcontrast_amd.local import LocalReducedBasis
    sm = SolutionsManagerFEM(blocks_geometry=(2, 2), N=8)
    a = np.random.default_rng(42).uniform(1.0, 100.0, size=(600, 2, 2))
    U = np.asarray(sm.generate_solutions(a))
    held = np.ascontiguousarray(U[:100])
    lrb = LocalReducedBasis(4).build(6, sm, U[100:], a[100:])
    X, Yg = np.meshgrid(sm.points_c[1:-1], sm.points_r[1:-1])
    verts = np.c_[X.ravel(), Yg.ravel()]
    points = verts[np.random.default_rng(3).choice(len(verts), 24, replace=False)]
    Y = np.asarray(sm.evaluate_solutions(points, held))
    jstar = lrb.classify(a[:100])
    err = lambda V: np.asarray(sm.H10norm_diff(np.ascontiguousarray(V), held))  # noqa: E731
    rms = lambda e: float(np.sqrt(np.mean(e ** 2)))  # noqa: E731
    glob = ReducedBasisPCA()
    glob.build(6, sm, U[100:], a[100:])
    rows = []
    for a_box, bounds in (("global", None), ("cluster", None), ("cluster", "training")):
        sensing = lrb.observe(sm, points, a_box=a_box, bounds=bounds)
        est = sensing.estimate(Y, states=True)
        every = np.stack([err(est.coefficients_all[:, j] @ sensing.W[j]) for j in range(4)], axis=1)
        rows.append({"a_box": a_box, "bounds": bounds, "label_is_cluster_of_a_true": float(np.mean(est.labels == jstar)),
                     "label_is_best_cluster": float(np.mean(est.labels == every.argmin(axis=1))), "unlabelled": int((est.labels < 0).sum()),
                     "rms_h10_selected": rms(err(est.states)), "rms_h10_cluster_of_a_true": rms(every[np.arange(100), jstar]),
                     "rms_h10_best_cluster": rms(every.min(axis=1)), "rank": sensing.rank, "lds_bytes": sensing.layout["lds_bytes"]})
    return {"geometry": "(2, 2), N = 8", "train": 500, "test": 100, "clusters": 4, "modes": 6, "sensors": 24,
            "rms_h10_global_pod_same_modes": rms(err(np.asarray(glob.state_estimation(sm, points, Y)))),
            "rms_h10_norm_of_held_out": rms(np.asarray(sm.H10norm(held))), "rows": rows}


def resources(path):
    """The compiler's report on rom_local_select.hip with the Makefile's flags, as a table."""
    csrc = os.path.join(ROOT, "romhighcontrast_amd", "csrc")
    cmd = [os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-I" + os.path.join(ROOT, "include"), "-I" + csrc,
           "-mllvm", "-pragma-unroll-threshold=10000000", "-Rpass-analysis=kernel-resource-usage", "-c",
           os.path.join(csrc, "rom_local_select.hip"), "-o", os.devnull]
    text = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, check=True).stdout.decode()
    kernels, cur = {}, None
    for line in text.splitlines():
        m = re.search(r"remark:\s+(.*?):\s+(\S+) \[-Rpass-analysis", line)
        if not m:
            continue
        key, val = m.group(1).strip(), m.group(2)
        if key == "Function Name":
            cur = kernels.setdefault(val, {})
        elif cur is not None:
            cur[key] = val
    from romhighcontrast_amd._ffi import local_select_layout
    keep = [(nm, rec) for nm, rec in kernels.items() if any(w in nm for w in ("k_local_fit", "k_local_pick", "k_bvls_gram"))]
    lines = ["Kernel resource usage (hipcc -Rpass-analysis=kernel-resource-usage, --offload-arch=gfx950, the Makefile's flags) of the kernels of",
             "rom_local_select.hip.  scratch: bytes per lane; occ: waves per SIMD as the compiler reports it from the registers (the LDS of",
             "k_local_fit is dynamic: below).  SGPR spills go to VGPR lanes, not to memory.", "",
             f"{'kernel':<16}{'VGPRs':>7}{'AGPRs':>7}{'SGPRs':>7}{'SGPR spills':>13}{'VGPR spills':>13}{'scratch':>9}{'static LDS':>12}{'occ':>5}"]
    for nm, rec in keep:
        short = re.search(r"(k_[a-z_]+?)E", nm).group(1)
        short = re.sub(r"^\d+", "", short)
        lines.append(f"{short:<16}{rec['VGPRs']:>7}{rec['AGPRs']:>7}{rec['TotalSGPRs']:>7}{rec['SGPRs Spill']:>13}{rec['VGPRs Spill']:>13}"
                     f"{rec['ScratchSize [bytes/lane]']:>9}{rec['LDS Size [bytes/block]']:>12}{rec['Occupancy [waves/SIMD]']:>5}")
    lines += ["", "Dynamic LDS of k_local_fit (rom_local_select_layout); workgroups per CU: what 160 KB of LDS admit, at most the 7 that the",
              "registers admit (7 waves per SIMD, 4 waves per workgroup, 4 SIMDs):", "",
              f"{'(n, k, rank, r)':<22}{'LDS bytes':>10}{'workgroups / CU':>17}{'rank_max':>10}"]
    for n, k, rank, r in ((8, 4, 33, 8), (32, 9, 289, 32), (32, 9, 289, 96), (64, 4, 257, 96), (8, 16, 129, 8), (64, 16, 64, 96)):
        lay = local_select_layout(n, k, rank, r)
        lines.append(f"{str((n, k, rank, r)):<22}{lay['lds_bytes']:>10}{min(160 * 1024 // lay['lds_bytes'], 7):>17}{lay['rank_max']:>10}")
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--spec-vectors", type=int, default=4)
    ap.add_argument("--resources", default=None)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--kernel-stats", nargs=2, metavar=("DB", "CSV"), default=None)
    args = ap.parse_args()
    if args.kernel_stats:
        kernel_stats(*args.kernel_stats)
        return 0
    if args.resources:
        resources(args.resources)
        return 0
    from romhighcontrast_amd import _ffi
    ctx = _ffi.get_context()
    if args.trace:
        for kc, n, k, rank in CONFIGS:
            measure(ctx, kc, n, k, rank, 0, 0, trace_only=True)
        return 0
    doc = {"device": ctx.device_name(),
           "timed": "whole calls between HIP events; kernels by the library's event brackets in a run of their own; the specification by wall clock",
           "calls": []}
    for kc, n, k, rank in CONFIGS:
        rec = measure(ctx, kc, n, k, rank, args.reps, args.spec_vectors)
        doc["calls"].append(rec)
        print(json.dumps({q: rec[q] for q in ("kc", "n", "k", "rank", "call_ms_median", "passes_state_mean", "bvls_same_systems", "bvls_one_call",
                                              "rank_k_call_ms_median", "kernel_ms_profiled")}), flush=True)
    doc["experiment"] = experiment()
    text = json.dumps(doc, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
