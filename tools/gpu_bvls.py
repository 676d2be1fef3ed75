"""Timing of the box-constrained least squares (rom_bvls) beside scipy's BVLS and bvls_host, and the noise experiment it was
built for.

  python tools/gpu_bvls.py [--out profiles/bvls.json] [--reps 10] [--scipy-rows 256]

* rom_bvls for K = 4 096 right-hand sides at (n, r) = (20, 20), (50, 50), (64, 64) on the synthetic construction of
  tests/bvls_truth.py (G = N(0, 1) / sqrt(r), lo = -U(0.2, 1), hi = U(0.2, 1), p = G c* + 0.05 N(0, 1), c* ~ U(-1.5, 1.5)).  The
  whole call between HIP events on the context stream (both launches, its one synchronisation and the counters' download
  included; the upload of P and the download of OUT are outside), median of --reps after one untimed call.  Passes per system
  from the call's own counters.
* scipy.optimize.lsq_linear(method="bvls", tol=1e-14), one call per right-hand side, on the first --scipy-rows rows of the same
  inputs in the same run: wall clock per row, and scaled to K rows (NOT measured at K rows: the loop is linear in them).
  bvls_host (NumPy, batched) on all K rows: wall clock of one call.
* the experiment end to end: (2, 2) blocks, N = 5, 600 parameters a ~ U(1, 100) (default_rng(42)), rows 100.. training, rows
  0..99 held out; the basis: leading right singular vectors of the uncentred training block; sensors at interior vertices
  (default_rng(3)); Gaussian noise (default_rng(5)); the box: min / max of the training coefficients.  The rms H^1_0 error of the
  held-out states for the plain least squares, the box-constrained estimate (device) and the projection.
Not measured: kernel time apart from the call (no profiler run), other K, the PBDW path's time.
Prints one JSON document (and writes it to --out)."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from romhighcontrast_amd import _ffi  # noqa: E402
from romhighcontrast_amd.inverse import bvls_host  # noqa: E402


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


def synthetic(n, r, K):
    g = np.random.default_rng(1000 * n + r)
    G = g.standard_normal((r, n)) / np.sqrt(r)
    lo, hi = -g.uniform(0.2, 1.0, n), g.uniform(0.2, 1.0, n)
    P = g.uniform(-1.5, 1.5, (K, n)) @ G.T + 0.05 * g.standard_normal((K, r))
    return G, P, lo, hi


def measure_kernel(ctx, n, r, K, reps, scipy_rows):
    from scipy.optimize import lsq_linear
    G, P, lo, hi = synthetic(n, r, K)
    dG, dP = ctx.upload(G), ctx.upload(P)
    OUT = ctx.alloc(K * (n + 4))
    call = lambda: ctx.bvls(n, r, dG, dP, 0, r, K, lo, hi, OUT=OUT)  # noqa: E731
    med, tmin, tmax = _events_median(ctx, call, reps)
    res, info = call()
    info = {k: v for k, v in info.items() if k != "bound_variables"}
    t0 = time.perf_counter()
    host = bvls_host(G, P, lo, hi)
    host_ms = 1e3 * (time.perf_counter() - t0)
    rows = min(scipy_rows, K)
    t0 = time.perf_counter()
    ref = np.array([lsq_linear(G, p, bounds=(lo, hi), method="bvls", tol=1e-14).x for p in P[:rows]])
    scipy_ms = 1e3 * (time.perf_counter() - t0)
    return {"n": n, "r": r, "K": K, "call_ms_median": med, "call_ms_min": tmin, "call_ms_max": tmax, "reps": reps, "info": info,
            "passes_per_system_mean": info["passes"] / K, "passes_max": int(res.iterations.max()), "converged": int(res.converged.sum()),
            "bound_variables_mean": float((res.bound != 0).sum(axis=1).mean()),
            "bvls_host_ms": host_ms, "host_converged": int(host.converged.sum()),
            "scipy_rows": rows, "scipy_ms_per_row": scipy_ms / rows, "scipy_ms_scaled_to_K": scipy_ms / rows * K,
            "scipy_scaled_over_device": scipy_ms / rows * K / med, "bvls_host_over_device": host_ms / med,
            "max_abs_c_device_minus_host": float(np.abs(res.c - host.c).max()),
            "max_abs_c_device_minus_scipy": float(np.abs(res.c[:rows] - ref).max()),
            "pass_counts_equal_host": bool(np.array_equal(res.iterations, host.iterations))}


def experiment(ctx):
    from romhighcontrast_amd.lib.ReducedBasis import BaseReducedBasis
    from romhighcontrast_amd.lib.SolutionsManagers import SolutionsManagerFEM
    sm = SolutionsManagerFEM(blocks_geometry=(2, 2), N=5)
    a = np.random.default_rng(42).uniform(1.0, 100.0, size=(600, 2, 2))
    U = np.asarray(sm.generate_solutions(a))
    Vt = np.linalg.svd(U[100:], full_matrices=False)[2]
    X, Yg = np.meshgrid(sm.points_c[1:-1], sm.points_r[1:-1])
    verts = np.c_[X.ravel(), Yg.ravel()]
    rms = lambda W: float(np.sqrt(np.mean(np.asarray(sm.H10norm(np.ascontiguousarray(W - U[:100]))) ** 2)))  # noqa: E731
    rows = []
    for n, m, sigma in ((16, 20, 1e-3), (12, 14, 1e-3), (12, 14, 1e-4), (8, 10, 1e-3)):
        rb = BaseReducedBasis()
        rb.set(np.ascontiguousarray(Vt[:n]), a[100:100 + n])
        points = verts[np.random.default_rng(3).choice(len(verts), m, replace=False)]
        Y = np.asarray(sm.evaluate_solutions(points, U[:100]))
        Y = Y + sigma * np.random.default_rng(5).standard_normal(Y.shape)
        box = rb.coefficient_bounds(sm, U[100:], inflate=0.0)
        rows.append({"modes": n, "sensors": m, "sigma": sigma, "rms_h10_plain_lstsq": rms(rb.state_estimation(sm, points, Y)),
                     "rms_h10_box_device": rms(rb.state_estimation(sm, points, Y, bounds=box)),
                     "rms_h10_box_host": rms(rb.state_estimation(sm, points, Y, bounds=box, device=False)),
                     "rms_h10_pbdw_plain": rms(rb.state_estimation_pbdw(sm, points, Y)),
                     "rms_h10_pbdw_box": rms(rb.state_estimation_pbdw(sm, points, Y, bounds=box)),
                     "rms_h10_projection": rms(np.asarray(rb.projection(sm, U[:100])))})
    return {"geometry": "(2, 2), N = 5", "train": 500, "test": 100, "box": "min / max of the training projection coefficients", "rows": rows}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--scipy-rows", type=int, default=256)
    args = ap.parse_args()
    ctx = _ffi.get_context()
    doc = {"device": ctx.device_name(), "timed": "the whole rom_bvls call between HIP events; scipy and bvls_host by wall clock", "kernel": []}
    for n, r in ((20, 20), (50, 50), (64, 64)):
        rec = measure_kernel(ctx, n, r, 4096, args.reps, args.scipy_rows)
        doc["kernel"].append(rec)
        print(json.dumps({q: rec[q] for q in ("n", "r", "K", "call_ms_median", "passes_per_system_mean", "scipy_ms_per_row", "bvls_host_ms")}),
              flush=True)
    doc["experiment"] = experiment(ctx)
    text = json.dumps(doc, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
