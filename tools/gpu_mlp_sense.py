"""Timing of the sensor state estimation on the MLP manifold (rom_mlp_sense) beside rom_poly_sense and the host iteration, and
the experiment it was built for.

  python tools/gpu_mlp_sense.py [--out profiles/mlp_sense.json] [--reps 10]

* rom_mlp_sense at (m, hidden, r) = (4, (20, 20), 12), (12, (64, 64, 64), 40) and (16, (64,), 81), tanh, K t = 4096 systems
  (t = 4): the hidden weights MLPMap.initial_weights (seed 7) and G_r ~ N(0, 1) (the construction of tests/mlp_sense_truth.py), data
  on the manifold with noise 1e-3 max|p|, starts t* + 0.1 N(0, 1).  The whole call between HIP events on the context stream (its
  one synchronisation and the counters' download included), median of --reps after one untimed call.
* rom_poly_sense at (m, d, r) = (4, 2, 8) and (12, 2, 40), 4096 systems, the inputs of tools/gpu_poly_sense.py, in the same run: the
  same driver at comparable m and r.  THE RATIO reported: time per executed LM iteration, rom_mlp_sense over rom_poly_sense, beside
  the ratio of the feature flops per iteration (hidden stack: values 2 sum H_{l+1} H_l per forward pass, tangents 16 times that;
  Legendre table: m P products for the values, 16 m P for the tangents).  No threshold is fixed.
* nonlinear.mlp_sense_scores (NumPy) on the same inputs in the same run, wall clock of one call.
* the experiment end to end: (2, 2) blocks, N = 5, 2,000 parameters a ~ U(1, 100) (default_rng(42)), the first 64 held out; PCA of
  the others, MLPMap((20, 20)) from 4 to 8 score columns, 8 sensors at interior vertices (default_rng(3)); from the exact
  measurements of the held-out states the rms H^1_0 error of the manifold estimate and of the linear least squares on 4 and on 8
  modes (no order is expected: it depends on the trained network), device against host scores with the host's own change under
  a permutation of the hidden units, and the times of estimate(device=True / False).
Prints one JSON document (and writes it to --out)."""
import argparse
import copy
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from romhighcontrast_amd import _ffi  # noqa: E402
from romhighcontrast_amd.nonlinear import (MLPMap, _mlp_split, legendre_features, mlp_hidden_features,  # noqa: E402
                                           mlp_sense_scores)


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


def measure_mlp(ctx, m, hidden, r, K, t, reps, activation="tanh"):
    sizes = [m, *hidden]
    WH = MLPMap.initial_weights(sizes, activation, 7)
    layers = _mlp_split(WH, sizes)
    rng = np.random.default_rng(7)
    Gr = rng.standard_normal((r, 1 + m + hidden[-1]))
    rng = np.random.default_rng(K)
    t_true = rng.uniform(-0.9, 0.9, size=(K, m))
    P = mlp_hidden_features(t_true, layers, activation, False)[0] @ Gr.T
    P = P + 1e-3 * np.abs(P).max(axis=1, keepdims=True) * rng.standard_normal(P.shape)
    T0 = t_true[:, None, :] + 0.1 * rng.standard_normal((K, t, m))
    dW, dG, dP, dT = ctx.upload(WH), ctx.upload(Gr), ctx.upload(P), ctx.upload(T0)
    OUT = ctx.alloc(K * (m + 5))
    tol = 2e-3 * np.sqrt(r)
    call = lambda: ctx.mlp_sense(m, hidden, activation, dW, r, dG, dP, 0, r, K, t, dT, -1.5, 1.5, misfit_tol=tol, OUT=OUT)  # noqa: E731
    med, lo, hi = _events_median(ctx, call, reps)
    res, info = call()
    t0 = time.perf_counter()
    host = mlp_sense_scores(Gr, sizes, activation, WH, P, T0, -1.5, 1.5, misfit_tol=tol)
    host_ms = 1e3 * (time.perf_counter() - t0)
    stack = 2 * sum(a * b for a, b in zip(sizes[:-1], sizes[1:]))
    passes_per_iteration = info["evaluations"] / max(info["iterations"], 1)
    return {"kernel": "rom_mlp_sense", "m": m, "hidden": list(hidden), "activation": activation, "r": r, "P": 1 + m + hidden[-1], "K": K,
            "t": t, "systems": K * t, "call_ms_median": med, "call_ms_min": lo, "call_ms_max": hi, "reps": reps, "info": info,
            "us_per_lm_iteration": 1e3 * med / max(info["iterations"], 1), "forward_passes_per_iteration": passes_per_iteration,
            "feature_flops_per_iteration": stack * passes_per_iteration + 16 * stack,
            "iterations_max": int(res.iterations.max()), "converged": int(res.converged.sum()), "host_mlp_sense_scores_ms": host_ms,
            "host_converged": int(host.converged.sum()), "host_over_device": host_ms / med,
            "median_abs_t_error": float(np.median(np.abs(res.t - t_true).max(axis=1))),
            "max_abs_t_device_minus_host": float(np.abs(res.t - host.t).max()),
            "max_rel_misfit_device_minus_host": float((np.abs(res.misfit - host.misfit) / host.misfit).max())}


def measure_poly(ctx, m, d, r, K, t, reps):
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
    passes_per_iteration = info["evaluations"] / max(info["iterations"], 1)
    return {"kernel": "rom_poly_sense", "m": m, "d": d, "r": r, "P": len(pw), "K": K, "t": t, "systems": K * t, "call_ms_median": med,
            "call_ms_min": lo, "call_ms_max": hi, "reps": reps, "info": info,
            "us_per_lm_iteration": 1e3 * med / max(info["iterations"], 1), "table_evaluations_per_iteration": passes_per_iteration,
            "feature_flops_per_iteration": m * len(pw) * passes_per_iteration + 16 * m * len(pw),
            "iterations_max": int(res.iterations.max()), "converged": int(res.converged.sum())}


def permuted_sensing(sense):
    """The same MLPSensing with the hidden units of every layer permuted (host side only)."""
    from romhighcontrast_amd.inverse import reduce_sensors
    other = copy.copy(sense)
    rng = np.random.default_rng(9)
    prev, layers = np.arange(sense.m), []
    for W, b in sense.layers:
        perm = rng.permutation(len(W))
        layers.append((W[perm][:, prev].copy(), b[perm].copy()))
        prev = perm
    other.WH = np.concatenate([W.ravel() for W, _ in layers] + [b for _, b in layers])
    other.layers = _mlp_split(other.WH, other.sizes)
    other.W_out = sense.W_out[:, prev].copy()
    other.S = other._sensing_matrix()
    other.U, other.Gr_host, _ = reduce_sensors(other.S.T, other.weights)
    return other


def experiment(ctx):
    from romhighcontrast_amd.lib.ReducedBasis import pca_tall
    from romhighcontrast_amd.lib.SolutionsManagers import SolutionsManagerFEM
    from romhighcontrast_amd.nonlinear import MLPSensing
    n_test, m, q, ms = 64, 4, 8, 8
    sm = SolutionsManagerFEM(blocks_geometry=(2, 2), N=5)
    a = np.random.default_rng(42).uniform(1.0, 100.0, size=(2000, 2, 2))
    U = np.asarray(sm.generate_solutions(a))
    pca = pca_tall(ctx, U[n_test:], n=m + q, center=True, scores=True, download=True)
    Z, V, mean = pca.scores, np.asarray(pca.components_), np.asarray(pca.mean_).ravel()
    mlp = MLPMap((20, 20), ctx=ctx).fit(Z[:, :m], Z[:, m:m + q])
    X, Yg = np.meshgrid(sm.points_c[1:-1], sm.points_r[1:-1])
    verts = np.c_[X.ravel(), Yg.ravel()]
    points = verts[np.random.default_rng(3).choice(len(verts), ms, replace=False)]
    Y = np.asarray(sm.evaluate_solutions(points, U[:n_test]))
    sense = MLPSensing(sm, pca, mlp).observe(points)

    def wall(device, which=sense, states=True):
        ctx.synchronize()
        t0 = time.perf_counter()
        est = which.estimate(Y, states=states, device=device)
        ctx.synchronize()
        return 1e3 * (time.perf_counter() - t0), est

    wall(True)
    dev = [wall(True) for _ in range(5)]
    host_ms, host = wall(False)
    _, again = wall(False, permuted_sensing(sense), False)
    est = dev[0][1]
    rms = lambda W: float(np.sqrt(np.mean(np.asarray(sm.H10norm(np.ascontiguousarray(W - U[:n_test]))) ** 2)))  # noqa: E731
    E = np.asarray(sm.evaluate_solutions(points, np.vstack([mean[None, :], V[:ms]])))
    z8 = np.linalg.lstsq(E[1:].T, (Y - E[0][None, :]).T, rcond=None)[0].T
    scale = float(np.abs(host.known_scores).max())
    delta = float(np.abs(again.known_scores - host.known_scores).max() / scale)
    return {"geometry": "(2, 2), N = 5", "train": len(U) - n_test, "test": n_test, "m": m, "q": q, "hidden": [20, 20], "activation": "tanh",
            "sensors": ms, "r": int(sense.r), "mlp_fit": {k: mlp.info_[k] for k in ("iterations", "loss", "stop_reason")},
            "rms_h10_manifold_device": rms(est.states.numpy()), "rms_h10_manifold_host": rms(host.states.numpy()),
            "rms_h10_linear_4_modes": rms(mean + est.linear_scores @ V[:m]), "rms_h10_linear_8_modes": rms(mean + z8 @ V[:ms]),
            "known_scores_device_minus_host_over_max": float(np.abs(est.known_scores - host.known_scores).max() / scale),
            "known_scores_host_minus_permuted_host_over_max": delta, "bound_max_1e3_delta_1e-9": max(1e3 * delta, 1e-9),
            "starts_differ": int((est.start != host.start).sum()), "iteration_counts_differ": int((est.iterations != host.iterations).sum()),
            "iterations_max": int(est.iterations.max()), "converged": int(est.converged.sum()),
            "estimate_device_ms_median": float(np.median([d[0] for d in dev])), "estimate_device_ms_all": [d[0] for d in dev],
            "estimate_host_ms": host_ms}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=10)
    args = ap.parse_args()
    ctx = _ffi.get_context()
    doc = {"device": ctx.device_name(), "hidden_weights": "read through L2 (the only placement measured)", "kernel": []}
    show = ("kernel", "m", "r", "P", "systems", "call_ms_median", "us_per_lm_iteration", "feature_flops_per_iteration")
    for m, hidden, r in ((4, (20, 20), 12), (12, (64, 64, 64), 40), (16, (64,), 81)):
        doc["kernel"].append(measure_mlp(ctx, m, hidden, r, 1024, 4, args.reps))
        print(json.dumps({q: doc["kernel"][-1][q] for q in show + ("hidden", "host_over_device")}), flush=True)
    for m, d, r in ((4, 2, 8), (12, 2, 40)):
        doc["kernel"].append(measure_poly(ctx, m, d, r, 1024, 4, args.reps))
        print(json.dumps({q: doc["kernel"][-1][q] for q in show + ("d",)}), flush=True)
    mlp, poly = doc["kernel"][:3], doc["kernel"][3:]
    doc["ratio_per_lm_iteration"] = [
        {"mlp": [a["m"], a["hidden"], a["r"]], "poly": [b["m"], b["d"], b["r"]], "time": a["us_per_lm_iteration"] / b["us_per_lm_iteration"],
         "feature_flops": a["feature_flops_per_iteration"] / b["feature_flops_per_iteration"]}
        for a, b in ((mlp[0], poly[0]), (mlp[1], poly[1]), (mlp[2], poly[1]))]
    doc["experiment"] = experiment(ctx)
    text = json.dumps(doc, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
