"""Timing of the regression trees and forests on PCA scores (rom_tree_fit / rom_tree_predict) on the device.

  python tools/gpu_tree.py [--out profiles/tree_forest.json] [--reps 5] [--skip-host] [--rows 1000,10000,25000] [--synthetic 131072]

Per block -- the scores of the (2, 2) / N = 5 problem of the reference's experiment at the given numbers of samples, and a
synthetic score block (tools/gpu_poly_map.py's) at --synthetic rows -- the map from the 4 leading columns to the next 16, for
a tree (T = 1) and a bootstrap forest of 10:
* the whole fit and the whole prediction of all rows (with Yref and the column sums of squares, nothing of size M x q
  written): wall clock around the synchronous calls after a warm-up, median of --reps;
* the per-kernel split of one fit + predict from the library's HIP-event profile (rom_profile_query): the share of the
  level kernels (tree_gain, tree_tiles, tree_stats, tree_partition, tree_decide) and of the presort;
* unless --skip-host: scikit-learn's DecisionTreeRegressor() / RandomForestRegressor(n_estimators=10) fit and predict on the
  host for the same arrays (wall clock, one run), and both held-out RMSEs on the last 1000 rows of a fit on the others.
Prints one JSON document (and writes it to --out)."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from romhighcontrast_amd import _ffi  # noqa: E402
from romhighcontrast_amd.nonlinear import ForestMap  # noqa: E402
from gpu_poly_map import _profile, score_block  # noqa: E402


def _wall_median(ctx, fn, reps):
    ts = []
    for i in range(reps + 1):
        ctx.synchronize()
        t0 = time.perf_counter()
        fn()
        ctx.synchronize()
        if i >= 1:
            ts.append(1e3 * (time.perf_counter() - t0))
    return {"call_ms_median": float(np.median(ts)), "call_ms_min": float(np.min(ts)), "call_ms_max": float(np.max(ts)), "reps": reps}


def measure(ctx, S, Sh, M, dim, m, q, T, reps, skip_host):
    rec = {"M": M, "m": m, "q": q, "T": T}
    counts = ForestMap.bootstrap_counts(T, M, 0) if T > 1 else None
    fit = lambda: ctx.tree_fit(S, 0, dim, m, S, m, dim, q, M, T, counts)  # noqa: E731
    tm = fit()
    rec["info"] = tm.info
    predict = lambda: tm.predict(S, 0, dim, M, OUT=None, Yref=S, r_off=m, ldr=dim, sumsq=True)  # noqa: E731
    rec["fit"] = _wall_median(ctx, fit, reps)
    rec["predict"] = _wall_median(ctx, predict, reps)
    _, prof = _profile(ctx, lambda: (fit(), predict()))
    rec["profile"] = prof
    total = sum(v["ms"] for v in prof.values())
    rec["kernel_ms_total"] = total
    rec["kernel_share"] = {k: v["ms"] / total for k, v in prof.items()} if total > 0 else {}
    if not skip_host:
        from sklearn.ensemble import RandomForestRegressor
        from sklearn.tree import DecisionTreeRegressor
        make = (lambda: DecisionTreeRegressor()) if T == 1 else (lambda: RandomForestRegressor(n_estimators=T))
        X, Y = Sh[:, :m], Sh[:, m:m + q]
        t0 = time.perf_counter()
        sk = make().fit(X, Y)
        t1 = time.perf_counter()
        sk.predict(X)
        t2 = time.perf_counter()
        rec["sklearn"] = {"fit_wall_ms": 1e3 * (t1 - t0), "predict_wall_ms": 1e3 * (t2 - t1)}
        if M > 2000:   # held-out RMSE (all columns together) of both, fitted on the rows before the last 1000
            n = M - 1000
            cnt = ForestMap.bootstrap_counts(T, n, 0) if T > 1 else None
            tmh = ctx.tree_fit(S, 0, dim, m, S, m, dim, q, n, T, cnt)
            ss = tmh.predict(S, n * dim, dim, 1000, OUT=None, Yref=S, r_off=n * dim + m, ldr=dim, sumsq=True)
            skp = make().fit(X[:n], Y[:n]).predict(X[n:]).reshape(1000, q)
            rec["held_out_rmse"] = {"device": float(np.sqrt(ss.sum() / (1000 * q))),
                                    "sklearn": float(np.sqrt(((skp - Y[n:]) ** 2).mean()))}
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--skip-host", action="store_true")
    ap.add_argument("--rows", default="1000,10000,25000")
    ap.add_argument("--synthetic", type=int, default=1 << 17)
    args = ap.parse_args()
    ctx = _ffi.get_context()
    doc = {"maps": []}
    m, q = 4, 16
    rows = [int(r) for r in args.rows.split(",") if r]
    blocks = []
    if rows:
        from romhighcontrast_amd.nonlinear import vn_family_sampler
        from romhighcontrast_amd.lib.ReducedBasis import pca_tall
        out = vn_family_sampler(max(rows), (2, 2), 1, 100, 5)
        pca = pca_tall(ctx, out["solutions"], center=True, scores=True, download=False)
        blocks += [("scores (2, 2) / N = 5", pca.scores.buf, M, pca.scores.dim) for M in rows]
    if args.synthetic:
        blocks.append(("synthetic", score_block(ctx, args.synthetic, 81, seed=17), args.synthetic, 81))
    for name, S, M, dim in blocks:
        Sh = None if args.skip_host else S.download(M * dim, shape=(M, dim))
        for T in (1, 10):
            rec = measure(ctx, S, Sh, M, dim, m, q, T, args.reps, args.skip_host)
            rec["block"] = name
            doc["maps"].append(rec)
            print(json.dumps({k: rec[k] for k in ("block", "M", "T", "info", "fit", "predict", "sklearn", "held_out_rmse", "kernel_share")
                              if k in rec}), flush=True)
    text = json.dumps(doc, indent=1)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    else:
        print(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
