"""Timing of the nearest-row search (rom_nearest) and of the library-based parameter estimation, and the gate on the screen kernel.

  python tools/gpu_nearest.py [--out profiles/nearest.json] [--reps 10]

* rom_nearest at K = 1024 queries, t = 4, r in {16, 64}, M in {2^16, 2^20} (uniform data): the whole call in mode 0 (screened)
  and mode 1 (exhaustive), HIP events on the context stream around the call (download of the result included), median of
  --reps (mode 1: 2); the per-kernel split of one call from the library's HIP-event profile; the `info` of the call.
* the screen kernel's flop rate, 2 M K r_pad / t, beside rom_gemm_nt forming the K x 2^16 scores of the same r in the same run
  (2 K 2^16 r / t, median of --reps).  THE GATE: at every (r, M) the screen's rate is at least half of rom_gemm_nt's at that
  r -- the same product with 1/32 of the output and a fused reduction.  Exit status 1 if it is missed.
* the baseline a user of the parent commit has, at M = 2^16: rom_gemm_nt in chunks of 2^14 library rows, download of the
  scores, |q|^2 - 2 p.q and numpy.argpartition on the host (wall clock, one run).
* the library estimate end to end at C2 ((2, 2), N = 128), n = 50 basis snapshots, m = 200 sensors, a library of 2^17
  log-uniform parameters over two decades, K = 1024 measurement vectors: building the library (rom_resid_eval), observe, the
  search, the polish on the host (wall clock each).
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


def measure_search(ctx, M, K, r, t, reps, gemm_tf):
    rng = np.random.default_rng(r + M % 1000)
    Q, P = ctx.upload(rng.random((M, r))), ctx.upload(rng.random((K, r)))
    rec = {"M": M, "K": K, "r": r, "t": t}
    answers = []
    for mode, n in ((0, reps), (1, 2)):
        call = lambda: ctx.nearest(Q, 0, r, M, P, 0, r, K, r, t=t, mode=mode)  # noqa: E731
        med, lo, hi = _events_median(ctx, call, n)
        (idx, d2, info), prof = _profile(ctx, call)
        answers.append((idx, d2))
        rec[f"mode{mode}"] = {"call_ms_median": med, "call_ms_min": lo, "call_ms_max": hi, "reps": n, "info": info, "profile": prof}
    rec["modes_agree_bitwise"] = bool(np.array_equal(answers[0][0], answers[1][0]) and
                                      np.array_equal(answers[0][1].view(np.uint64), answers[1][1].view(np.uint64)))
    scr = [v for k, v in rec["mode0"]["profile"].items() if k.startswith("nn_screen")]
    ms = sum(v["ms"] for v in scr)
    rpad = (r + 3) // 4 * 4
    tf = 2.0 * M * K * rpad / (ms * 1e-3) / 1e12
    rec["screen"] = {"ms": ms, "tflops": tf, "rom_gemm_nt_tflops": gemm_tf, "ratio": tf / gemm_tf}
    return rec


def baseline_gemm_argpartition(ctx, M, K, r, t, chunk=1 << 14):
    rng = np.random.default_rng(r)
    Qh, Ph = rng.random((M, r)), rng.random((K, r))
    Q, P, S = ctx.upload(Qh), ctx.upload(Ph), ctx.alloc(K * chunk)
    t0 = time.perf_counter()
    nq = np.einsum("mc,mc->m", Qh, Qh)
    best_s, best_i = np.full((K, 0), np.inf), np.zeros((K, 0), dtype=np.int64)
    for j0 in range(0, M, chunk):
        mc = min(chunk, M - j0)
        ctx.gemm_nt(K, mc, r, P, 0, r, Q, j0 * r, r, S, 0, mc)
        sc = nq[None, j0:j0 + mc] - 2.0 * S.download(K * mc, shape=(K, mc))
        part = np.argpartition(sc, t - 1, axis=1)[:, :t]
        best_s = np.hstack((best_s, np.take_along_axis(sc, part, axis=1)))
        best_i = np.hstack((best_i, part + j0))
    keep = np.argsort(best_s, axis=1)[:, :t]
    idx = np.take_along_axis(best_i, keep, axis=1)
    return {"M": M, "K": K, "r": r, "chunk": chunk, "wall_ms": 1e3 * (time.perf_counter() - t0)}, idx


def library_end_to_end(K=1024, n=50, m=200, M=1 << 17, t=4):
    from romhighcontrast_amd.inverse import ParameterLibrary
    from romhighcontrast_amd.lib.SolutionsManagers import SolutionsManagerFEM
    rng = np.random.default_rng(0)
    sm = SolutionsManagerFEM((2, 2), 128)
    basis = sm.generate_solutions_device(10.0 ** rng.uniform(0, 2, size=(n, 2, 2)))
    a_lib = 10.0 ** rng.uniform(0, 2, size=(M, 4))
    points = rng.uniform(-0.95, 0.95, size=(m, 2))
    a_true = 10.0 ** rng.uniform(0, 2, size=(K, 2, 2))
    Y = sm.evaluate_solutions(points, sm.generate_solutions_device(a_true))
    Y = Y + 1e-3 * np.abs(Y).max(axis=1, keepdims=True) * rng.standard_normal(Y.shape)
    rec = {"geometry": "(2, 2), N = 128", "n": n, "m": m, "M": M, "K": K, "t": t, "noise": 1e-3}
    sm._ctx.synchronize()
    t0 = time.perf_counter()
    lib = ParameterLibrary(sm, basis, a_lib)
    sm._ctx.synchronize()
    rec["library_build_ms"] = 1e3 * (time.perf_counter() - t0)
    t0 = time.perf_counter()
    lib.observe(points)
    sm._ctx.synchronize()
    rec["observe_ms"] = 1e3 * (time.perf_counter() - t0)
    t0 = time.perf_counter()
    idx, misfit, info = lib.search(Y, t=t)
    rec["search_ms"] = 1e3 * (time.perf_counter() - t0)
    rec["search_info"] = info
    t0 = time.perf_counter()
    # (the noise alone leaves a misfit of about 1e-3 sqrt(m) max|y| = 1.4e-2 max|y|: the flag's threshold is twice that)
    est = lib.estimate(Y, t=t, misfit_tol=2e-3 * np.sqrt(m))
    rec["estimate_ms"] = 1e3 * (time.perf_counter() - t0)
    err_lib = np.abs(np.log10(lib.a[idx[:, 0]]) - np.log10(a_true.reshape(K, 4))).max(axis=1)
    err = np.abs(np.log10(est.a) - np.log10(a_true)).reshape(K, 4).max(axis=1)
    rec.update(r=int(lib.r), median_err_library=float(np.median(err_lib)), median_err_polished=float(np.median(err)),
               converged=int(est.converged.sum()), iterations_max=int(est.iterations.max()),
               sigma_min_median=float(np.median(est.sigma_min)), error_bound_upper_median=float(np.median(est.error_bound.upper)))
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=10)
    args = ap.parse_args()
    ctx = _ffi.get_context()
    K, t = 1024, 4
    doc = {"device": ctx.device_name(), "K": K, "t": t, "rom_gemm_nt": [], "search": [], "gates": []}
    for r in (16, 64):
        N = 1 << 16
        rng = np.random.default_rng(r)
        A, B, Cb = ctx.upload(rng.random((K, r))), ctx.upload(rng.random((N, r))), ctx.alloc(K * N)
        med, lo, hi = _events_median(ctx, lambda: ctx.gemm_nt(K, N, r, A, 0, r, B, 0, r, Cb, 0, N), args.reps)
        gemm_tf = 2.0 * K * N * r / (med * 1e-3) / 1e12
        doc["rom_gemm_nt"].append({"m": K, "n": N, "k": r, "ms_median": med, "ms_min": lo, "ms_max": hi, "tflops": gemm_tf})
        del A, B, Cb
        for M in (1 << 16, 1 << 20):
            rec = measure_search(ctx, M, K, r, t, args.reps, gemm_tf)
            doc["search"].append(rec)
            gate = {"r": r, "M": M, "screen_tflops": rec["screen"]["tflops"], "rom_gemm_nt_tflops": gemm_tf,
                    "ratio": rec["screen"]["ratio"], "required": 0.5, "met": rec["screen"]["tflops"] >= 0.5 * gemm_tf}
            doc["gates"].append(gate)
            print(json.dumps(gate), flush=True)
            print(json.dumps({k: rec[k]["call_ms_median"] for k in ("mode0", "mode1")}), flush=True)
    doc["baseline_gemm_argpartition"] = [baseline_gemm_argpartition(ctx, 1 << 16, K, r, t)[0] for r in (16, 64)]
    doc["library_estimate_c2"] = library_end_to_end(K=K)
    text = json.dumps(doc, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    return 0 if all(g["met"] for g in doc["gates"]) else 1


if __name__ == "__main__":
    sys.exit(main())
