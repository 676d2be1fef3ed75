"""Timing of the polynomial maps between PCA coordinates (rom_poly_fit / rom_poly_predict) on the device.

  python tools/gpu_poly_map.py [--out profiles/poly_map.json] [--reps 10] [--skip-host] [--rows 25000,1048576]

Per block size -- 25,000 and 2^20 rows of 81 synthetic score columns whose scales fall over six orders, as PCA scores do,
built on the device from a seed -- and per degree d = 1, 2, 4: the map from the 4 leading columns to the 77 others,
* the whole fit and the whole prediction of all rows (with Yref and the column sums of squares, nothing of size M x q
  written): median of --reps calls after a warm-up, HIP events on the context stream;
* the per-kernel split of one fit + predict from the library's HIP-event profile (rom_profile_query), and the flop rate of
  the pass kernel, its executed flops (M (2 P_pad^2 + 512 tiles) per launch, no rotation in pass 1) over its time;
* unless --skip-host: scikit-learn's Pipeline(PolynomialFeatures(d), LinearRegression()) fit and predict on the host
  (wall clock), and the relative RMS distance between its predictions and the device's on the first 1000 rows.
Prints one JSON document (and writes it to --out)."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from romhighcontrast_amd import _ffi  # noqa: E402


def _events_median(ctx, fn, reps):
    ts = []
    for i in range(reps + 2):
        ctx.synchronize()
        ctx.timer_start()
        fn()
        t = ctx.timer_stop()
        if i >= 2:
            ts.append(t)
    return float(np.median(ts)), float(np.min(ts)), float(np.max(ts))


def _profile(ctx, fn):
    ctx.profile(True)
    ctx.profile_reset()
    try:
        out = fn()
        rep = ctx.profile_report()
    finally:
        ctx.profile(False)
    return out, {k: {"ms": v["total_ms"], "launches": v["launches"], "flops": v["flops"], "bytes": v["bytes"]}
                 for k, v in sorted(rep.items(), key=lambda kv: -kv[1]["total_ms"]) if v["launches"]}


def score_block(ctx, M, dim, seed):
    """M x dim: smooth functions of 4 latent uniform coordinates plus noise, column j scaled by 10^(-6 j / dim)."""
    rng = np.random.default_rng(seed)
    Z = rng.uniform(-1, 1, (M, 4))
    feats = np.hstack((Z, Z ** 2, np.sin(2 * Z), Z[:, :1] * Z[:, 1:], 1e-3 * rng.standard_normal((M, 5))))
    mix = rng.standard_normal((feats.shape[1], dim))
    mix[:4, :4] = np.eye(4)
    mix[4:, :4] = 0.0
    S = ctx.alloc(M * dim)
    ctx.gemm_nn(M, dim, feats.shape[1], ctx.upload(feats), 0, feats.shape[1], ctx.upload(mix * 10.0 ** (-6.0 * np.arange(dim) / dim)), 0,
                dim, S, 0, dim)
    return S


def measure(ctx, S, M, dim, m, d, reps, skip_host):
    q = dim - m
    rec = {"M": M, "m": m, "q": q, "d": d}
    fit = lambda: ctx.poly_fit(S, 0, dim, m, S, m, dim, q, M, d)  # noqa: E731
    pm = fit()
    rec["info"] = pm.info
    P = pm.info["P"]
    predict = lambda: pm.predict(S, 0, dim, M, OUT=None, Yref=S, r_off=m, ldr=dim, sumsq=True)  # noqa: E731
    for name, fn in (("fit", fit), ("predict", predict)):
        med, lo, hi = _events_median(ctx, fn, reps)
        rec[name] = {"call_ms_median": med, "call_ms_min": lo, "call_ms_max": hi, "reps": reps}
    _, prof = _profile(ctx, lambda: (fit(), predict()))
    rec["profile"] = prof
    ps = prof.get("poly_pass")
    if ps:
        # (executed flops as the library counts them, M (2 P_pad^2 + 512 tiles) with no rotation in pass 1, over the kernel time)
        rec["pass"] = {"P": P, "launches": ps["launches"], "ms_per_launch": ps["ms"] / ps["launches"],
                       "executed_tflops": ps["flops"] / (ps["ms"] * 1e-3) / 1e12,
                       "useful_flops_per_row_and_pass": 2.0 * P * P + 2.0 * P * (P / 2.0 + q)}
    if not skip_host:
        from sklearn.linear_model import LinearRegression
        from sklearn.pipeline import Pipeline
        from sklearn.preprocessing import PolynomialFeatures
        Sh = S.download(M * dim, shape=(M, dim))
        t0 = time.perf_counter()
        pipe = Pipeline([("poly", PolynomialFeatures(d)), ("LR", LinearRegression())]).fit(Sh[:, :m], Sh[:, m:])
        t1 = time.perf_counter()
        sk = pipe.predict(Sh[:, :m])
        t2 = time.perf_counter()
        out = ctx.alloc(1000 * q)
        pm.predict(S, 0, dim, 1000, OUT=out)
        dev = out.download(shape=(1000, q))
        scale = np.sqrt((Sh[:, m:] ** 2).mean(axis=0))
        rec["sklearn"] = {"fit_wall_ms": 1e3 * (t1 - t0), "predict_wall_ms": 1e3 * (t2 - t1),
                          "worst_column_rms_distance_to_device_rel": float((np.sqrt(((sk[:1000] - dev) ** 2).mean(axis=0)) / scale).max())}
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--skip-host", action="store_true")
    ap.add_argument("--rows", default="25000,1048576")
    args = ap.parse_args()
    ctx = _ffi.get_context()
    doc = {"device": ctx.device_name() if hasattr(ctx, "device_name") else "?", "maps": []}
    dim, m = 81, 4
    for M in (int(r) for r in args.rows.split(",")):
        S = score_block(ctx, M, dim, seed=M % 1000)
        for d in (1, 2, 4):
            rec = measure(ctx, S, M, dim, m, d, args.reps, args.skip_host)
            doc["maps"].append(rec)
            print(json.dumps({k: rec[k] for k in ("M", "d", "fit", "predict", "pass", "sklearn") if k in rec}), flush=True)
        del S
    text = json.dumps(doc, indent=1)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    else:
        print(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
