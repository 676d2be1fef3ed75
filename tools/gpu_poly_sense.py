"""Timing of the sensor state estimation on the polynomial manifold (rom_poly_sense) beside the host iteration, and the
experiment it was built for.

  python tools/gpu_poly_sense.py [--out profiles/poly_sense.json] [--reps 10]

* rom_poly_sense at (m, d, r) = (4, 2, 8), (4, 4, 12) and (12, 2, 40), K t = 4096 and 2^15 systems (t = 4): a synthetic G_r
  (N(0, 1), the columns of degree g scaled by 0.3^max(g - 1, 0): the construction of tests/sense_truth.py), data on the manifold
  with noise 1e-3 max|p|, starts t* + 0.1 N(0, 1).  The whole call between HIP events on the context stream (its one
  synchronisation and the counters' download included), median of --reps after one untimed call.
* nonlinear.sense_scores (NumPy) on the same inputs in the same run, wall clock of one call: THE BASELINE of every ratio.
  THE CONDITION: the device call is faster than sense_scores at 4096 systems, for every shape.  Exit status 1 if it is missed.
* the experiment end to end: (2, 2) blocks, N = 5, 1,200 parameters a ~ U(1, 100) (default_rng(42)), the first 100 held out; PCA
  of the other 1,100, the degree-2 map from 4 to 16 score columns, 8 sensors at interior vertices (default_rng(3)); from the exact
  measurements of the held-out states the rms H^1_0 error of the nonlinear estimate (device and host path), of the linear least
  squares on 4 and on 8 modes and of the best 4-mode projection, and the times of estimate(device=True / False).
Prints one JSON document (and writes it to --out)."""
import argparse
import itertools
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from romhighcontrast_amd import _ffi  # noqa: E402
from romhighcontrast_amd.nonlinear import legendre_features, sense_scores  # noqa: E402


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


def measure_kernel(ctx, m, d, r, K, t, reps):
    pw = _ffi.poly_terms(m, d).astype(np.int64)
    rng = np.random.default_rng(7)
    Gr = rng.standard_normal((r, len(pw))) * (0.3 ** np.maximum(pw.sum(axis=1) - 1, 0))[None, :]
    rng = np.random.default_rng(K)
    t_true = rng.uniform(-0.9, 0.9, size=(K, m))
    P = legendre_features(t_true, pw, False)[0] @ Gr.T
    P = P + 1e-3 * np.abs(P).max(axis=1, keepdims=True) * rng.standard_normal(P.shape)
    T0 = t_true[:, None, :] + 0.1 * rng.standard_normal((K, t, m))
    dG, dP, dT = ctx.upload(Gr), ctx.upload(P), ctx.upload(T0)
    OUT = ctx.alloc(K * (m + 5))
    tol = 2e-3 * np.sqrt(r)
    call = lambda: ctx.poly_sense(m, d, r, dG, dP, 0, r, K, t, dT, -1.5, 1.5, misfit_tol=tol, OUT=OUT)  # noqa: E731
    med, lo, hi = _events_median(ctx, call, reps)
    res, info = call()
    t0 = time.perf_counter()
    host = sense_scores(Gr, pw, P, T0, -1.5, 1.5, misfit_tol=tol)
    host_ms = 1e3 * (time.perf_counter() - t0)
    return {"m": m, "d": d, "r": r, "P": len(pw), "K": K, "t": t, "systems": K * t, "call_ms_median": med, "call_ms_min": lo,
            "call_ms_max": hi, "reps": reps, "info": info, "iterations_max": int(res.iterations.max()),
            "converged": int(res.converged.sum()), "host_sense_scores_ms": host_ms, "host_converged": int(host.converged.sum()),
            "host_over_device": host_ms / med, "median_abs_t_error": float(np.median(np.abs(res.t - t_true).max(axis=1))),
            "max_abs_t_device_minus_host": float(np.abs(res.t - host.t).max()),
            "max_rel_misfit_device_minus_host": float((np.abs(res.misfit - host.misfit) / host.misfit).max())}


def experiment(ctx):
    from romhighcontrast_amd.lib.ReducedBasis import pca_tall
    from romhighcontrast_amd.lib.SolutionsManagers import SolutionsManagerFEM
    from romhighcontrast_amd.nonlinear import PolynomialMap, PolynomialSensing
    n_test, m, q, ms = 100, 4, 16, 8
    sm = SolutionsManagerFEM(blocks_geometry=(2, 2), N=5)
    a = np.random.default_rng(42).uniform(1.0, 100.0, size=(1200, 2, 2))
    U = np.asarray(sm.generate_solutions(a))
    pca = pca_tall(ctx, U[n_test:], n=m + q, center=True, scores=True, download=True)
    Z, V, mean = pca.scores, np.asarray(pca.components_), np.asarray(pca.mean_).ravel()
    poly = PolynomialMap(2, ctx=ctx).fit(Z[:, :m], Z[:, m:m + q])
    verts = np.array([(x, y) for y, x in itertools.product(sm.points_r[1:-1], sm.points_c[1:-1])])
    points = verts[np.random.default_rng(3).choice(len(verts), ms, replace=False)]
    Y = np.asarray(sm.evaluate_solutions(points, U[:n_test]))
    sense = PolynomialSensing(sm, pca, poly).observe(points)

    def wall(device):
        ctx.synchronize()
        t0 = time.perf_counter()
        est = sense.estimate(Y, states=True, device=device)
        ctx.synchronize()
        return 1e3 * (time.perf_counter() - t0), est

    wall(True)
    dev = [wall(True) for _ in range(5)]
    host_ms, host = wall(False)
    est = dev[0][1]
    rms = lambda W: float(np.sqrt(np.mean(np.asarray(sm.H10norm(np.ascontiguousarray(W - U[:n_test]))) ** 2)))  # noqa: E731
    E = np.asarray(sm.evaluate_solutions(points, np.vstack([mean[None, :], V[:ms]])))
    z8 = np.linalg.lstsq(E[1:].T, (Y - E[0][None, :]).T, rcond=None)[0].T
    best4 = (U[:n_test] - mean) @ V[:m].T
    return {"geometry": "(2, 2), N = 5", "train": 1100, "test": n_test, "m": m, "q": q, "degree": 2, "sensors": ms, "r": int(sense.r),
            "rms_h10_nonlinear_device": rms(est.states.numpy()), "rms_h10_nonlinear_host": rms(host.states.numpy()),
            "rms_h10_linear_4_modes": rms(mean + est.linear_scores @ V[:m]), "rms_h10_best_4_mode_projection": rms(mean + best4 @ V[:m]),
            "rms_h10_linear_8_modes": rms(mean + z8 @ V[:ms]),
            "known_scores_device_minus_host_over_max": float(np.abs(est.known_scores - host.known_scores).max() / np.abs(host.known_scores).max()),
            "iterations_max": int(est.iterations.max()), "estimate_device_ms_median": float(np.median([d[0] for d in dev])),
            "estimate_device_ms_all": [d[0] for d in dev], "estimate_host_ms": host_ms}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=10)
    args = ap.parse_args()
    ctx = _ffi.get_context()
    doc = {"device": ctx.device_name(), "baseline": "nonlinear.sense_scores (NumPy) on the same inputs in the same run", "kernel": []}
    for m, d, r in ((4, 2, 8), (4, 4, 12), (12, 2, 40)):
        for K in (1024, 8192):
            rec = measure_kernel(ctx, m, d, r, K, 4, args.reps)
            doc["kernel"].append(rec)
            print(json.dumps({q: rec[q] for q in ("m", "d", "r", "systems", "call_ms_median", "host_sense_scores_ms", "host_over_device")}),
                  flush=True)
    doc["experiment"] = experiment(ctx)
    at4096 = [rec["host_over_device"] for rec in doc["kernel"] if rec["systems"] == 4096]
    doc["condition"] = {"host_over_device_at_4096_systems": at4096, "met": bool(min(at4096) > 1.0)}
    text = json.dumps(doc, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    return 0 if doc["condition"]["met"] else 1


if __name__ == "__main__":
    sys.exit(main())
