"""Timing of the MLP maps between PCA coordinates (rom_mlp_fit / rom_mlp_loss_grad / rom_mlp_predict) on the device.

  python tools/gpu_mlp.py [--out profiles/mlp.json] [--reps 10] [--skip-host] [--rows 25000,1048576]
  python tools/gpu_mlp.py --resources profiles/mlp_resources.txt      (no GPU: the compiler's register / LDS report)

Per block size -- 25,000 and 2^20 rows of synthetic score columns (tools/gpu_poly_map.py's block, built on the device from a
seed) -- and for the two shapes the feature exists for, 4 -> 20 -> 20 -> 77 (tanh, a block of 81 columns) and 16 -> 64 -> 64 ->
16 (tanh, a block of 32 columns):
* one rom_mlp_loss_grad: median of --reps calls after a warm-up, HIP events on the context stream (the call includes its
  download of P + 1 doubles), and the split into k_mlp_eval and k_mlp_reduce from the library's HIP-event profile; the
  executed-flop rate of k_mlp_eval, 6 M sum K^pad N^pad over its time;
* the rate of rom_poly_fit's pass kernel on the same block in the same run (degree 4 from 4 inputs, degree 1 from 16), the
  yardstick: an evaluation at >= half that rate;
* rom_l2norm over the block: the read floor;
* the whole fit (max_iter 200 at 25,000 rows, 20 at 2^20) and the whole prediction with Yref and sums of squares;
* the optimiser's host synchronisations per iteration;
* unless --skip-host, at 25,000 rows: scikit-learn's MLPRegressor(solver="lbfgs") on the same scaled arrays, wall clock and
  final loss -- for information only (another line search, another stopping rule).
Then the observed / bound ratios of tests/test_gpu_mlp.py (loss, gradient and optimiser cases of tests/mlp_truth.py).
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
from romhighcontrast_amd import _ffi  # noqa: E402
from romhighcontrast_amd.nonlinear import MLPMap, mlp_fit_host, mlp_loss_grad_host  # noqa: E402

SHAPES = [dict(name="4-20-20-77", m=4, hidden=[20, 20], q=77, poly_degree=4),
          dict(name="16-64-64-16", m=16, hidden=[64, 64], q=16, poly_degree=1)]


def _events_median(ctx, fn, reps):
    ts = []
    for i in range(reps + 2):
        ctx.synchronize()
        ctx.timer_start()
        fn()
        t = ctx.timer_stop()
        if i >= 2:
            ts.append(t)
    return {"call_ms_median": float(np.median(ts)), "call_ms_min": float(np.min(ts)), "call_ms_max": float(np.max(ts)), "reps": reps}


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


def measure(ctx, shape, M, reps, skip_host):
    m, hidden, q = shape["m"], shape["hidden"], shape["q"]
    dim = m + q
    S = score_block(ctx, M, dim, seed=M % 1000)
    sizes = [m] + hidden + [q]
    lay = _ffi.mlp_layout(m, hidden, q)
    w0 = MLPMap.initial_weights(sizes, "tanh", 0)
    rec = {"shape": shape["name"], "M": M, "P": lay["P"], "padded_weights": lay["padded_weights"], "lds_eval_bytes": lay["lds_eval"],
           "lds_predict_bytes": lay["lds_predict"]}
    fit = lambda it: ctx.mlp_fit(S, 0, dim, m, S, m, dim, q, M, hidden, w0, "tanh", 1e-4, True, it, 1e-6, 10)  # noqa: E731
    h0 = fit(0)
    lg = lambda: h0.loss_grad(S, 0, dim, S, m, dim, M)  # noqa: E731
    rec["loss_grad"] = _events_median(ctx, lg, reps)
    _, prof = _profile(ctx, lg)
    rec["loss_grad"]["profile"] = prof
    flops = 6.0 * M * lay["padded_weights"]
    ev = prof.get("mlp_eval")
    if ev:
        rec["eval_kernel"] = {"ms": ev["ms"] / ev["launches"], "executed_flops": flops,
                              "executed_tflops": flops / (ev["ms"] / ev["launches"] * 1e-3) / 1e12}
    # the yardstick: rom_poly_fit's pass kernel on the same block
    _, pprof = _profile(ctx, lambda: ctx.poly_fit(S, 0, dim, m, S, m, dim, q, M, shape["poly_degree"]))
    ps = pprof.get("poly_pass")
    if ps:
        rec["poly_pass"] = {"degree": shape["poly_degree"], "launches": ps["launches"], "ms_per_launch": ps["ms"] / ps["launches"],
                            "executed_tflops": ps["flops"] / (ps["ms"] * 1e-3) / 1e12}
        if ev:
            rec["eval_rate_over_poly_pass_rate"] = rec["eval_kernel"]["executed_tflops"] / rec["poly_pass"]["executed_tflops"]
            rec["yardstick_half_the_pass_rate_met"] = bool(rec["eval_rate_over_poly_pass_rate"] >= 0.5)
    # the read floor: rom_l2norm over the block (at most 65,535 vectors a call: rows joined in twos until they are that few)
    K = M
    while K > 65535 and K % 2 == 0:
        K //= 2
    l2 = _events_median(ctx, lambda: ctx.l2norm(S, 0, K, dim * (M // K)), reps)
    l2["vectors"] = K
    l2["GB_per_s"] = 8.0 * M * dim / (l2["call_ms_median"] * 1e-3) / 1e9
    rec["l2norm_read_floor"] = l2
    # whole fit and whole prediction
    iters = 200 if M <= 100000 else 20
    hf = fit(iters)
    rec["fit"] = dict(_events_median(ctx, lambda: fit(iters), max(3, reps // 3)), max_iter=iters, info=hf.info,
                      host_syncs_per_iteration=hf.info["host_syncs"] / max(hf.info["iterations"], 1),
                      evaluations_per_iteration=hf.info["evaluations"] / max(hf.info["iterations"], 1))
    rec["predict"] = _events_median(ctx, lambda: hf.predict(S, 0, dim, M, OUT=None, Yref=S, r_off=m, ldr=dim, sumsq=True), reps)
    if not skip_host and M <= 100000:
        from sklearn.neural_network import MLPRegressor
        import mlp_truth as mt
        Sh = S.download(M * dim, shape=(M, dim))
        T = mt.scale_inputs(Sh[:, :m], hf.download("c"), hf.download("h"))
        Ys = mt.scale_targets(Sh[:, m:], hf.download("y_mean"), hf.download("y_scale"))
        t0 = time.perf_counter()
        sk = MLPRegressor(hidden_layer_sizes=tuple(hidden), activation="tanh", solver="lbfgs", alpha=1e-4, max_iter=iters, tol=1e-6,
                          random_state=0).fit(T, Ys)
        t1 = time.perf_counter()
        wsk = np.concatenate([cf.T.ravel() for cf in sk.coefs_] + list(sk.intercepts_))
        rec["sklearn_lbfgs_host"] = {"fit_wall_ms": 1e3 * (t1 - t0), "n_iter": int(sk.n_iter_),
                                     "final_loss_same_formula": float(mlp_loss_grad_host(wsk, sizes, "tanh", T, Ys, 1e-4)[0]),
                                     "device_final_loss": hf.info["loss"], "note": "for information only"}
    return rec


def test_ratios(ctx):
    """observed / bound of the cases of tests/test_gpu_mlp.py"""
    import mlp_truth as mt
    out = {"loss_grad": {}, "optimiser": {}}
    for case in mt.CASES:
        cid, m, hidden, q, M, activation, gain, alpha, seed = case
        X, Y, w, sizes = mt.case_data(case)
        Z = ctx.upload(np.hstack((X, Y)))
        h = ctx.mlp_fit(Z, 0, m + q, m, Z, m, m + q, q, M, hidden, w, activation, alpha, True, 0)
        T = mt.scale_inputs(X[:M], h.download("c"), h.download("h"))
        Ys = mt.scale_targets(Y[:M], h.download("y_mean"), h.download("y_scale"))
        L, g = h.loss_grad(Z, 0, m + q, Z, m, m + q, M)
        Ln, gn = mlp_loss_grad_host(w, sizes, activation, T, Ys, alpha)
        rl, rg = mt.ratios(L, g, w, sizes, activation, T, Ys, alpha)
        nl, ng = mt.ratios(Ln, gn, w, sizes, activation, T, Ys, alpha)
        out["loss_grad"][cid] = {"device_loss": rl, "device_grad": rg, "numpy_fp64_loss": nl, "numpy_fp64_grad": ng}
    for case in mt.OPT_CASES:
        cid, m, hidden, q, M, activation, seed = case
        X, Y, sizes = mt.opt_data(case)
        Z = ctx.upload(np.hstack((X, Y)))
        w0 = MLPMap.initial_weights(sizes, activation, seed)
        for it in (1, 2, 3):
            h = ctx.mlp_fit(Z, 0, m + q, m, Z, m, m + q, q, M, hidden, w0, activation, mt.OPT_ALPHA, True, it, mt.OPT_TOL, mt.OPT_MEMORY)
            T = mt.scale_inputs(X, h.download("c"), h.download("h"))
            Ys = mt.scale_targets(Y, h.download("y_mean"), h.download("y_scale"))
            args = (w0, sizes, activation, T, Ys, mt.OPT_ALPHA, it, mt.OPT_TOL, mt.OPT_MEMORY)
            a, b = mlp_fit_host(*args), mlp_fit_host(*args, dtype=mt.LD)
            w = h.download("w")
            tol = 64 * max(float(np.abs(a["w"] - b["w"]).max()), mt.EPS * float(np.abs(w).max()))
            out["optimiser"][f"{cid}_iter{it}"] = {"ratio": float(np.abs(w.astype(mt.LD) - b["w"]).max()) / tol,
                                                   "evaluations_device": h.info["evaluations"], "evaluations_host": b["evaluations"]}
    return out


def resources(path):
    """The compiler's resource report of the kernels of rom_mlp.hip (the Makefile's flags), no GPU needed."""
    csrc = os.path.join(ROOT, "romhighcontrast_amd", "csrc")
    cmd = ["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", f"-I{ROOT}/include", "-I.", "-Wno-unused-function",
           "-mllvm", "-pragma-unroll-threshold=10000000", "-Rpass-analysis=kernel-resource-usage", "-c", "rom_mlp.hip", "-o", os.devnull]
    err = subprocess.run(cmd, cwd=csrc, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, check=True).stdout.decode()
    rows, cur = [], None
    for line in err.splitlines():
        mm = re.search(r"remark: (?:Function Name: (\S+)|\s*(TotalSGPRs|VGPRs|AGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|"
                       r"SGPRs Spill|VGPRs Spill|LDS Size \[bytes/block\]): (\d+))", line)
        if not mm:
            continue
        if mm.group(1):
            name = re.search(r"k_mlp_[a-z_]+?(?=E)", mm.group(1))
            cur = {"kernel": name.group(0) if name else mm.group(1)}
            rows.append(cur)
        elif cur is not None:
            cur[mm.group(2)] = int(mm.group(3))
    keys = ["TotalSGPRs", "VGPRs", "AGPRs", "SGPRs Spill", "VGPRs Spill", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]",
            "LDS Size [bytes/block]"]
    lines = ["Kernel resource usage (hipcc -Rpass-analysis=kernel-resource-usage, --offload-arch=gfx950, the Makefile's flags) of the kernels of",
             "rom_mlp.hip, written by tools/gpu_mlp.py --resources.  LDS: the STATIC part; k_mlp_eval and k_mlp_predict add the dynamic part",
             "that rom_mlp_layout reports (below for the two flagship shapes, the widest output and two three-hidden-layer shapes near the limit).", "",
             "kernel".ljust(22) + "".join(k.split(" [")[0].rjust(14) for k in keys)]
    for r in rows:
        lines.append(r["kernel"].ljust(22) + "".join(str(r.get(k, "")).rjust(14) for k in keys))
    lines += ["", "static + dynamic LDS (bytes) of k_mlp_eval / k_mlp_predict, one workgroup of 512 threads per CU (160 KB = 163,840):"]
    for m, hidden, q in ((4, [20, 20], 77), (16, [64, 64], 16), (1, [64], 128), (32, [32, 64, 16], 128), (16, [32, 64, 48], 48)):
        lay = _ffi.mlp_layout(m, hidden, q)
        lines.append(f"  {m} -> {' -> '.join(map(str, hidden))} -> {q}:".ljust(34) + f"{lay['lds_eval']:>8} / {lay['lds_predict']:>8}"
                     f"   ({lay['padded_weights']} padded weights, P = {lay['P']})")
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--skip-host", action="store_true")
    ap.add_argument("--rows", default="25000,1048576")
    ap.add_argument("--resources", default=None, help="write the compiler's resource report there and exit (no GPU)")
    args = ap.parse_args()
    if args.resources:
        resources(args.resources)
        return 0
    ctx = _ffi.get_context()
    doc = {"device": ctx.device_name() if hasattr(ctx, "device_name") else "?", "optimiser_batch": 16, "maps": []}
    for M in (int(r) for r in args.rows.split(",")):
        for shape in SHAPES:
            rec = measure(ctx, shape, M, args.reps, args.skip_host)
            doc["maps"].append(rec)
            print(json.dumps({k: rec[k] for k in rec if k not in ("fit",)} | {"fit_ms": rec["fit"]["call_ms_median"]}), flush=True)
    doc["test_ratios"] = test_ratios(ctx)
    text = json.dumps(doc, indent=1)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    else:
        print(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
