"""Timing of the device polish (rom_lm_polish) and of the library estimate with it, and the gate on the estimate.

  python tools/gpu_lm_polish.py [--out profiles/lm_polish.json] [--reps 10]

* rom_lm_polish at (n, k, r) = (50, 4, 39) and (64, 16, 64), K t = 4096 and 2^15 systems (t = 4): a synthetic reduced model
  (Ahat_q = B B^T / w, the construction of tests/lm_truth.py), ROM-exact data with noise 1e-3 max|p|, starts theta* + 0.1 N(0, 1).
  The whole call between HIP events on the context stream (its one synchronisation and the counters' download included), median
  of --reps after one untimed call; the factorisations the call executed (counted on the device) and the call time per
  factorisation -- a THROUGHPUT figure over all resident workgroups, not the latency of one.
* rom_reduced_solve_batch at the same n and k with M = K t systems, in the same run, the same way: time per solve, and the ratio
  of the two per-factorisation figures (recorded, not gated: the polish adds the Jacobian, the k x k system and the trial's
  residual to every factorisation).
* the library estimate end to end at C2 ((2, 2), N = 128), n = 50, m = 200, a library of 2^17 parameters, K = 1024 measurement
  vectors with noise 1e-3, t = 4: estimate(polish=True) once and estimate(polish="device") (median of 5 after one untimed call),
  wall clock around calls that end synchronised, and the median error in log10 a of each.  THE GATE: the device route at least
  10 x faster, its median error at most 1.1 x the host route's.  Exit status 1 if it is missed.
Prints one JSON document (and writes it to --out)."""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from romhighcontrast_amd import _ffi  # noqa: E402


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


def synth(n, k, r, seed):
    rng = np.random.default_rng(seed)
    w = max(2, math.ceil(2 * n / k))
    B = rng.standard_normal((k, n, w))
    return np.einsum("qiw,qjw->qij", B, B) / w, rng.standard_normal(n), rng.standard_normal((r, n)) / np.sqrt(n)


def measure_kernel(ctx, n, k, r, K, t, reps):
    Ahat, bhat, Gr = synth(n, k, r, 7)
    rng = np.random.default_rng(K)
    hi = np.log(100.0)
    theta = rng.uniform(0.2, hi - 0.2, size=(K, k))
    A = np.einsum("bq,qij->bij", np.exp(theta), Ahat)
    P = np.linalg.solve(A, np.broadcast_to(bhat, (K, n))[..., None])[..., 0] @ Gr.T
    P = P + 1e-3 * np.abs(P).max(axis=1, keepdims=True) * rng.standard_normal(P.shape)
    theta0 = theta[:, None, :] + 0.1 * rng.standard_normal((K, t, k))
    dA, db, dG, dP, dT = ctx.upload(Ahat), ctx.upload(bhat), ctx.upload(Gr), ctx.upload(P), ctx.upload(theta0)
    OUT = ctx.alloc(K * (k + n + 5))
    tol = 2e-3 * np.sqrt(r)
    call = lambda: ctx.lm_polish(n, k, r, dA, db, dG, dP, 0, r, K, t, dT, 0.0, hi, misfit_tol=tol, OUT=OUT)  # noqa: E731
    med, lo, hi_ms = _events_median(ctx, call, reps)
    res, info = call()
    rec = {"n": n, "k": k, "r": r, "K": K, "t": t, "systems": K * t, "call_ms_median": med, "call_ms_min": lo, "call_ms_max": hi_ms,
           "reps": reps, "info": info, "iterations_max": int(res.iterations.max()), "converged": int(res.converged.sum()),
           "median_abs_theta_error": float(np.median(np.abs(res.theta - theta).max(axis=1))),
           "us_per_factorisation": 1e3 * med / info["factorisations"]}
    M = K * t
    W, C = ctx.upload(np.exp(np.clip(theta0, 0.0, np.log(100.0))).reshape(M, k)), ctx.alloc(M * n)
    smed, slo, shi = _events_median(ctx, lambda: ctx.reduced_solve_batch(n, k, M, dA, W, db, False, C), reps)
    rec["reduced_solve_batch"] = {"M": M, "call_ms_median": smed, "call_ms_min": slo, "call_ms_max": shi, "us_per_solve": 1e3 * smed / M}
    rec["factorisation_time_ratio_polish_over_reduced_solve"] = rec["us_per_factorisation"] / rec["reduced_solve_batch"]["us_per_solve"]
    return rec


def library_end_to_end(K=1024, n=50, m=200, M=1 << 17, t=4):
    from romhighcontrast_amd.inverse import ParameterLibrary
    from romhighcontrast_amd.lib.SolutionsManagers import SolutionsManagerFEM
    rng = np.random.default_rng(0)
    sm = SolutionsManagerFEM((2, 2), 128)
    ctx = sm._ctx
    basis = sm.generate_solutions_device(10.0 ** rng.uniform(0, 2, size=(n, 2, 2)))
    a_lib = 10.0 ** rng.uniform(0, 2, size=(M, 4))
    points = rng.uniform(-0.95, 0.95, size=(m, 2))
    a_true = 10.0 ** rng.uniform(0, 2, size=(K, 2, 2))
    Y = sm.evaluate_solutions(points, sm.generate_solutions_device(a_true))
    Y = Y + 1e-3 * np.abs(Y).max(axis=1, keepdims=True) * rng.standard_normal(Y.shape)
    lib = ParameterLibrary(sm, basis, a_lib).observe(points)
    tol = 2e-3 * np.sqrt(m)
    rec = {"geometry": "(2, 2), N = 128", "n": n, "m": m, "M": M, "K": K, "t": t, "noise": 1e-3, "r": int(lib.r)}

    def err_of(est):
        return float(np.median(np.abs(np.log10(est.a) - np.log10(a_true)).reshape(K, 4).max(axis=1)))

    def wall(polish):
        ctx.synchronize()
        t0 = time.perf_counter()
        est = lib.estimate(Y, t=t, polish=polish, misfit_tol=tol)
        ctx.synchronize()
        return 1e3 * (time.perf_counter() - t0), est

    wall("device")
    dev = [wall("device") for _ in range(5)]
    host_ms, host = wall(True)
    dev_ms = float(np.median([d[0] for d in dev]))
    est = dev[0][1]
    ctx.profile(True)
    ctx.profile_reset()
    lib.estimate(Y, t=t, polish="device", misfit_tol=tol)
    prof = {k_: {"ms": v["total_ms"], "launches": v["launches"]} for k_, v in
            sorted(ctx.profile_report().items(), key=lambda kv: -kv[1]["total_ms"]) if v["launches"]}
    ctx.profile(False)
    rec.update(estimate_host_ms=host_ms, estimate_device_ms_median=dev_ms, estimate_device_ms_all=[d[0] for d in dev],
               speedup=host_ms / dev_ms, median_err_host=err_of(host), median_err_device=err_of(est),
               converged_host=int(host.converged.sum()), converged_device=int(est.converged.sum()),
               misfit_difference_max_over_scale=float((np.abs(est.misfit - host.misfit) / np.abs(Y).max(axis=1)).max()),
               queries_with_misfit_within_1e_10=int((np.abs(est.misfit - host.misfit) <= 1e-10 * np.abs(Y).max(axis=1)).sum()),
               device_estimate_kernel_profile=prof)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=10)
    args = ap.parse_args()
    ctx = _ffi.get_context()
    doc = {"device": ctx.device_name(), "kernel": []}
    for n, k, r in ((50, 4, 39), (64, 16, 64)):
        for K in (1024, 8192):
            rec = measure_kernel(ctx, n, k, r, K, 4, args.reps)
            doc["kernel"].append(rec)
            print(json.dumps({q: rec[q] for q in ("n", "k", "r", "systems", "call_ms_median", "us_per_factorisation",
                                                  "factorisation_time_ratio_polish_over_reduced_solve")}), flush=True)
    e2e = library_end_to_end()
    doc["library_estimate_c2"] = e2e
    doc["gate"] = {"speedup": e2e["speedup"], "required_speedup": 10.0,
                   "error_ratio": e2e["median_err_device"] / e2e["median_err_host"], "allowed_error_ratio": 1.1}
    doc["gate"]["met"] = bool(doc["gate"]["speedup"] >= 10.0 and doc["gate"]["error_ratio"] <= 1.1)
    text = json.dumps(doc, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    return 0 if doc["gate"]["met"] else 1


if __name__ == "__main__":
    sys.exit(main())
