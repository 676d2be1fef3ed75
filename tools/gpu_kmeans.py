"""Timing of k-means (rom_kmeans_*) and of the local reduced bases built on it.

  python tools/gpu_kmeans.py [--out profiles/kmeans.json] [--reps 10] [--small]

* one Lloyd iteration at M = 2^20 rows for (r, kc) = (4, 16), (16, 64), (64, 64), (32, 256) on Gaussian blobs: the whole call
  rom_kmeans_fit(max_iter = 1) (statistics, one iteration, the final assignment, the downloads of the status), HIP events on the
  context stream, median of --reps; the fused kernel k_km_step alone from the library's HIP-event profile (mean of its launches
  in one call) and its executed flop rate (2 rows r_pad kc_pad + 2 rows kc_pad (r + 1)_pad + 3 M r over that time);
* beside it, on the same block in the same run, k_nn_screen of rom_nearest at K = 128 queries (2 rows r_pad 128 flops): the
  yardstick for a slab-engine kernel with an LDS-resident table;
* the share of rows that needed more than one exact rescore (info of the call over M x passes);
* a fit to convergence at 25 000 x 16, kc = 32 (call time, iterations), ``kmeans_host`` on the same data for information, and
  scikit-learn's KMeans (same initial centroids, algorithm "lloyd") where it is installed;
* LocalReducedBasis.build and forward_modeling at C2 ((2, 2), N = 128), M = 1024 training parameters, kc = 8, n = 20, against the
  global ReducedBasisPCA(inner_product="h10") of n = 20 and n = 40 in the same run (wall clock around a synchronise; rms relative
  H^1_0 error of the Galerkin solutions on 256 held-out parameters).
--small shrinks every size (a rehearsal of the script, not a measurement).  Prints one JSON document (and writes it to --out)."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from romhighcontrast_amd import _ffi  # noqa: E402
from romhighcontrast_amd.local import KMeans, LocalReducedBasis, kmeans_host  # noqa: E402


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


def blobs(M, r, kc, seed):
    rng = np.random.default_rng(seed)
    centres = 3.0 * rng.standard_normal((kc, r))
    X = centres[rng.integers(0, kc, size=M)] + rng.standard_normal((M, r))
    return X, X[rng.choice(M, size=kc, replace=False)].copy()


def one_iteration(ctx, M, r, kc, reps):
    Xh, init = blobs(M, r, kc, r + kc)
    X = ctx.upload(Xh)
    lay = _ffi.kmeans_layout(r, kc)
    call = lambda: ctx.kmeans_fit(X, 0, r, r, M, kc, init, max_iter=1)  # noqa: E731
    med, lo, hi = _events_median(ctx, call, reps)
    h, prof = _profile(ctx, call)
    step = [v for k, v in prof.items() if k.startswith("km_step")]
    ms = sum(v["ms"] for v in step) / max(sum(v["launches"] for v in step), 1)
    fl = sum(v["flops"] for v in step) / max(sum(v["launches"] for v in step), 1)
    rec = {"M": M, "r": r, "kc": kc, "layout": lay, "call_ms_median": med, "call_ms_min": lo, "call_ms_max": hi, "reps": reps,
           "info": h.info, "profile": prof, "km_step_ms": ms, "km_step_tflops": fl / (ms * 1e-3) / 1e12,
           "rows_rescored_more_share": h.info["rows_rescored_more"] / (2.0 * M)}
    # the yardstick: the screen of rom_nearest with 128 queries resident, on the same block
    P = ctx.upload(Xh[:128])
    _, nprof = _profile(ctx, lambda: ctx.nearest(X, 0, r, M, P, 0, r, 128, r, t=1, mode=0))
    scr = [v for k, v in nprof.items() if k.startswith("nn_screen")]
    sms = sum(v["ms"] for v in scr)
    rec["nn_screen_K128"] = {"ms": sms, "tflops": sum(v["flops"] for v in scr) / (sms * 1e-3) / 1e12}
    rec["km_step_over_nn_screen"] = rec["km_step_tflops"] / rec["nn_screen_K128"]["tflops"]
    return rec


def to_convergence(ctx, M, r, kc, reps):
    Xh, init = blobs(M, r, kc, 1)
    X = ctx.upload(Xh)
    call = lambda: ctx.kmeans_fit(X, 0, r, r, M, kc, init, max_iter=300)  # noqa: E731
    med, lo, hi = _events_median(ctx, call, reps)
    h = call()
    rec = {"M": M, "r": r, "kc": kc, "call_ms_median": med, "call_ms_min": lo, "call_ms_max": hi, "info": h.info}
    t0 = time.perf_counter()
    ref = kmeans_host(Xh, init, max_iter=300)
    rec["kmeans_host"] = {"wall_ms": 1e3 * (time.perf_counter() - t0), "iterations": ref.n_iter,
                          "labels_agree": bool(np.array_equal(ref.labels, h.download("labels")))}
    try:
        from sklearn.cluster import KMeans as SkKMeans
        t0 = time.perf_counter()
        sk = SkKMeans(n_clusters=kc, init=init, n_init=1, algorithm="lloyd", tol=0.0, max_iter=300).fit(Xh)
        rec["sklearn"] = {"wall_ms": 1e3 * (time.perf_counter() - t0), "iterations": int(sk.n_iter_), "inertia": float(sk.inertia_)}
    except ImportError:
        rec["sklearn"] = "not installed: not measured"
    rec["inertia"] = float(h.download("inertia")[-1])
    return rec


def local_bases(N, M, kc, n, held_out):
    from romhighcontrast_amd.lib.ReducedBasis import ReducedBasisPCA
    from romhighcontrast_amd.lib.SolutionsManagers import SolutionsManagerFEM
    rng = np.random.default_rng(7)
    sm = SolutionsManagerFEM((2, 2), N)
    ctx = sm._ctx
    a = 10.0 ** rng.uniform(0, 2, size=(M + held_out, 2, 2))
    U = sm.generate_solutions_device(a[:M], keep_interface_vectors=False)
    Ut = sm.generate_solutions_device(a[M:], keep_interface_vectors=False)
    norms = sm.H10norm(Ut)

    def wall(fn):
        ctx.synchronize()
        t0 = time.perf_counter()
        out = fn()
        ctx.synchronize()
        return out, 1e3 * (time.perf_counter() - t0)

    rms = lambda F: float(np.sqrt(((sm.H10norm_diff(F, Ut) / norms) ** 2).mean()))  # noqa: E731
    rec = {"geometry": f"(2, 2), N = {N}", "M": M, "kc": kc, "n": n, "held_out": held_out}
    wall(lambda: LocalReducedBasis(kc).build(n, sm, U, a[:M]))   # (warm-up: code objects, the sine tables)
    lrb, rec["local_build_ms"] = wall(lambda: LocalReducedBasis(kc).build(n, sm, U, a[:M]))
    rec["cluster_sizes"] = np.bincount(lrb.labels_, minlength=kc).tolist()
    wall(lambda: lrb.forward_modeling(sm, a[M:]))
    F, rec["local_forward_ms"] = wall(lambda: lrb.forward_modeling(sm, a[M:]))
    rec["local_galerkin_rms_rel_h10"] = rms(F)
    for ng in (n, 2 * n):
        wall(lambda: ReducedBasisPCA(add_inf_solutions=False, inner_product="h10").build(ng, sm, U, a[:M]))
        rb, tb = wall(lambda: ReducedBasisPCA(add_inf_solutions=False, inner_product="h10").build(ng, sm, U, a[:M]))
        wall(lambda: rb.forward_modeling(sm, a[M:]))
        F, tf = wall(lambda: rb.forward_modeling(sm, a[M:]))
        rec[f"global_n{ng}"] = {"build_ms": tb, "forward_ms": tf, "galerkin_rms_rel_h10": rms(F)}
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--small", action="store_true")
    args = ap.parse_args()
    ctx = _ffi.get_context()
    M = 1 << 14 if args.small else 1 << 20
    doc = {"device": ctx.device_name(), "small": args.small, "one_iteration": []}
    for r, kc in ((4, 16), (16, 64), (64, 64), (32, 256)):
        rec = one_iteration(ctx, M, r, kc, args.reps)
        doc["one_iteration"].append(rec)
        print(json.dumps({k: rec[k] for k in ("r", "kc", "call_ms_median", "km_step_ms", "km_step_tflops", "km_step_over_nn_screen",
                                              "rows_rescored_more_share")}), flush=True)
    doc["to_convergence"] = to_convergence(ctx, 2500 if args.small else 25000, 16, 32, max(2, args.reps // 3))
    print(json.dumps({k: doc["to_convergence"][k] for k in ("call_ms_median", "info")}), flush=True)
    doc["local_bases_c2"] = local_bases(16, 256, 8, 8, 64) if args.small else local_bases(128, 1024, 8, 20, 256)
    text = json.dumps(doc, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
