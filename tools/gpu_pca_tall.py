"""Timing of the full PCA of tall blocks (rom_pca_tall) on the device, and the gate on its pass kernels.

  python tools/gpu_pca_tall.py [--out profiles/pca_tall.json] [--reps 20] [--skip-host]

Per block -- the reference's 25,000 x 81 (vn_family_sampler(25000, (2, 2), 1, 100, 5)), 2^20 x 81 and 2^20 x 128 (synthetic:
24 directions over six orders plus noise at 1e-9, built on the device from a seed):
* the whole call (n = dim, with scores): median of --reps calls after a warm-up, HIP events on the context stream (the
  block is restored by a device copy before every call, outside the events);
* the per-kernel split of one call from the library's HIP-event profile (rom_profile_query);
* rom_pod (pod_modes, n = min(50, dim)) on the same block with its stop reason -- recorded, not compared: the two calls do
  not return the same thing (rom_pod is unchanged by the tall PCA);
* unless --skip-host: scikit-learn's PCA().fit_transform on the host (wall clock); at 25,000 x 81 also its singular values
  and the device's against a LAPACK SVD of the centred block.
The gate, at 2^20 x 81 and 2^20 x 128: the flop rate of one pass, 3 M dim_pad^2 / t (t = the pass kernels of the profile: the
fused kernel at 81; the rotation product + k_syrk_tn at 128, per pass), must be at least half of what rom_gram reaches in
the same run on a 4096 x 4096 block (m (m + 1) k / t, HIP events, median of --reps).  rom_l2norm over the same block is
recorded as the read floor.  Prints one JSON document (and writes it to --out); exit status 1 if a gate is missed."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from romhighcontrast_amd import _ffi  # noqa: E402
from romhighcontrast_amd.lib import ReducedBasis as RB  # noqa: E402
from romhighcontrast_amd.lib.SolutionsManagers import DeviceArray  # noqa: E402


def _events_median(ctx, fn, reps, before=None):
    ts = []
    for i in range(reps + 2):
        if before:
            before()
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


def synthetic_block(ctx, M, dim, seed):
    rng = np.random.default_rng(seed)
    r = 24
    F1 = np.hstack((rng.standard_normal((M, r)), rng.standard_normal((M, 8)) * 1e-9))
    F2 = np.vstack((rng.standard_normal((r, dim)) * (10.0 ** -np.linspace(0, 6, r))[:, None], rng.standard_normal((8, dim))))
    X = ctx.alloc(M * dim)
    ctx.gemm_nn(M, dim, r + 8, ctx.upload(F1), 0, r + 8, ctx.upload(F2), 0, dim, X, 0, dim)
    mean = ctx.upload(np.ones(M)), ctx.upload(rng.uniform(-1, 1, dim))
    ctx.gemm_nn(M, dim, 1, mean[0], 0, 1, mean[1], 0, dim, X, 0, dim, alpha=1.0, beta=1.0)
    return X


def measure_block(ctx, name, X0, M, dim, reps, host_block=None, skip_host=False):
    rec = {"block": name, "M": M, "dim": dim}
    X, V, S, mean = ctx.alloc(M * dim), ctx.alloc(dim * dim), ctx.alloc(M * dim), ctx.alloc(dim)
    restore = lambda: X.copy_from(X0, M * dim)  # noqa: E731
    call = lambda: ctx.pca_tall(X, M, dim, dim, V, S=S, mean=mean, center=True)  # noqa: E731
    med, lo, hi = _events_median(ctx, call, reps, before=restore)
    restore()
    (sig, info), prof = _profile(ctx, call)
    rec["pca_tall"] = {"call_ms_median": med, "call_ms_min": lo, "call_ms_max": hi, "reps": reps, "info": info, "profile": prof}
    # one pass: the kernels that read the block
    fused = [v for k, v in prof.items() if k.startswith("pca_tall_fused")]
    rot = [v for k, v in prof.items() if k.startswith("pca_tall_rotate")]
    syrk = [v for k, v in prof.items() if k.startswith("syrk_tn") and not k.startswith("syrk_tn_reduce")]
    if fused:
        dpad = (dim + 15) // 16 * 16
        pass_ms = sum(v["ms"] for v in fused) / sum(v["launches"] for v in fused)
        form = "fused"
    else:
        dpad = (dim + 15) // 16 * 16
        pass_ms = sum(v["ms"] for v in rot) / max(sum(v["launches"] for v in rot), 1) + sum(v["ms"] for v in syrk) / sum(v["launches"] for v in syrk)
        form = "rotate + syrk_tn"
    rec["pass"] = {"form": form, "dim_pad": dpad, "ms": pass_ms, "tflops": 3.0 * M * dpad * dpad / (pass_ms * 1e-3) / 1e12,
                   "flops_per_byte_read": 3.0 * dpad * dpad / (8.0 * dim)}
    step = 65535   # (rows per rom_l2norm call)
    med, lo, hi = _events_median(ctx, lambda: [ctx.l2norm(X0, r, min(step, M - r), dim) for r in range(0, M, step)], reps)
    rec["l2norm_read_floor"] = {"ms_median": med, "GBps": 8.0 * M * dim / (med * 1e-3) / 1e9}
    # rom_pod on the same block (unchanged code: what the parent commit offers for this shape)
    n_pod = min(50, dim)
    restore()
    try:
        t0 = time.perf_counter()
        RB.pod_modes(ctx, DeviceArray(X, M, dim), n_pod, center=True, download=False)
        ctx.synchronize()
        rec["rom_pod"] = {"n": n_pod, "wall_ms_first_call": 1e3 * (time.perf_counter() - t0), "info": RB.pod_modes.last_info}
        med, lo, hi = _events_median(ctx, lambda: ctx.pod(X, M, dim, n_pod, V, center=True), (2 if M > 100000 else max(3, reps // 4)),
                                     before=restore)
        rec["rom_pod"]["call_ms_median"] = med
    except Exception as e:   # (rom_pod may refuse the shape: that is the record)
        rec["rom_pod"] = {"n": n_pod, "error": str(e)}
    if not skip_host:
        from sklearn.decomposition import PCA
        Xh = X0.download(M * dim, shape=(M, dim)) if host_block is None else host_block
        t0 = time.perf_counter()
        pca = PCA()
        pca.fit_transform(Xh)
        rec["sklearn"] = {"fit_transform_wall_ms": 1e3 * (time.perf_counter() - t0), "solver": getattr(pca, "_fit_svd_solver", "?")}
        if M <= 100000:
            s_ref = np.linalg.svd(Xh - Xh.mean(axis=0), compute_uv=False)
            above = s_ref > 1e-13 * s_ref[0]
            rel = lambda s: (np.abs(s[:len(s_ref)] - s_ref) / s_ref)  # noqa: E731
            rec["vs_lapack"] = {"modes_above_1e-13": int(above.sum()), "sigma_rel_lapack": (s_ref / s_ref[0]).tolist(),
                                "sklearn_rel_err": rel(pca.singular_values_).tolist(), "pca_tall_rel_err": rel(sig).tolist(),
                                "sklearn_worst_above_floor": float(rel(pca.singular_values_)[above].max()),
                                "pca_tall_worst_above_floor": float(rel(sig)[above].max())}
        else:
            rec["vs_lapack"] = "not measured (the LAPACK SVD of this block is host minutes)"
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--skip-host", action="store_true")
    args = ap.parse_args()
    ctx = _ffi.get_context()
    doc = {"device": ctx.device_name() if hasattr(ctx, "device_name") else "?", "blocks": [], "gates": []}
    # the yardstick of the gate: rom_gram on 4096 x 4096
    m = k = 4096
    A, G = ctx.upload(np.random.default_rng(1).standard_normal((m, k))), ctx.alloc(m * m)
    med, lo, hi = _events_median(ctx, lambda: ctx.gram(m, k, A, 0, k, G, 0, m), args.reps)
    gram_tf = m * (m + 1.0) * k / (med * 1e-3) / 1e12
    doc["rom_gram_4096"] = {"ms_median": med, "ms_min": lo, "ms_max": hi, "tflops": gram_tf}
    del A, G
    from romhighcontrast_amd import nonlinear
    ref = nonlinear.vn_family_sampler(25000, (2, 2), 1, 100, 5)["solutions"]
    doc["blocks"].append(measure_block(ctx, "NonLinearROM 25000 x 81", ctx.upload(ref), 25000, 81, args.reps, host_block=ref,
                                       skip_host=args.skip_host))
    print(json.dumps(doc["blocks"][-1]["pass"]), flush=True)
    for dim in (81, 128):
        M = 1 << 20
        X0 = synthetic_block(ctx, M, dim, seed=dim)
        rec = measure_block(ctx, f"synthetic 2^20 x {dim}", X0, M, dim, args.reps, skip_host=args.skip_host)
        doc["blocks"].append(rec)
        gate = {"block": rec["block"], "pass_tflops": rec["pass"]["tflops"], "rom_gram_tflops": gram_tf,
                "ratio": rec["pass"]["tflops"] / gram_tf, "required": 0.5, "met": rec["pass"]["tflops"] >= 0.5 * gram_tf}
        doc["gates"].append(gate)
        print(json.dumps(gate), flush=True)
        del X0
    text = json.dumps(doc, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    return 0 if all(g["met"] for g in doc["gates"]) else 1


if __name__ == "__main__":
    sys.exit(main())
