"""Timing of the D-optimal sensor design (rom_sensor_dopt) and what it buys.

  python tools/gpu_sensor_dopt.py [--out profiles/sensor_dopt.json] [--reps 10] [--resources profiles/sensor_dopt_resources.txt]

* At C2-like sizes -- n = 50, k = 4 (a synthetic reduced model), ncand = 65 025, M = 1024 and 2^14, m = 50 -- one scoring pass
  (rom_sensor_dopt_scores: HIP events around the call, median of --reps after one untimed call; k_dopt_score and k_dopt_reduce from
  the library's HIP-event brackets) with its executed TFLOP/s, 2 (M kp) n_pad ncand / t; rom_gemm_nt forming the ncand x M kp
  products of the same n in the same run (M kp capped at 2^14 columns: 8.5 GB of output); k_nn_screen (rom_nearest, mode 0) on the
  problem of equal size, ncand queries against M kp rows of n columns; the same scoring pass from libromhc_oed_plain.so
  (`make -C romhighcontrast_amd/csrc oed_plain`: the epilogue without its log1p), in a child process, which gives the share of
  the log1p; the whole design call, init and m = 50 steps; and the NumPy specification's scoring pass timed at ncand = 2048,
  M = 128 and scaled by the product of the sizes.
* At (2, 2) / N = 8 with a POD basis of n = 6, 64 library parameters, all interior vertices as candidates, m = 8 and noise 1e-3:
  the posterior_sd the design predicts beside ParameterLibrary.posterior(...).sd (rom_mcmc) for 16 library entries, and the median
  sd with the D-optimal sensors, with select_sensors_pbdw's and with random ones.
* --resources: VGPRs, LDS and spills of the kernels of rom_oed.hip from the compiler's report (needs hipcc, no GPU).
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
CSRC = os.path.join(ROOT, "romhighcontrast_amd", "csrc")
PLAIN = os.path.join(CSRC, "libromhc_oed_plain.so")
N, K, NCAND, PICKS, SIGMA = 50, 4, 65025, 50, 1e-3


def model(n, k, M, ncand, seed=0):
    """A synthetic reduced model (Ahat_q = B_q B_q^T / w), theta ~ U(0.2, log 100 - 0.2), candidate rows ~ N(0, 1) / sqrt(n)."""
    rng = np.random.default_rng(seed)
    w = max(2, -(-2 * n // k))
    B = rng.standard_normal((k, n, w))
    return dict(Ahat=np.einsum("qiw,qjw->qij", B, B) / w, bhat=rng.standard_normal(n),
                theta=rng.uniform(0.2, np.log(100.0) - 0.2, size=(M, k)), E=rng.standard_normal((ncand, n)) / np.sqrt(n),
                prior=np.full(k, np.log(100.0) ** 2 / 12.0))


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
    return out, {k: {"ms": v["total_ms"], "launches": v["launches"], "flops": v["flops"]}
                 for k, v in sorted(rep.items(), key=lambda kv: -kv[1]["total_ms"]) if v["launches"]}


def score_pass(ctx, M, reps):
    """One scoring pass on the empty state of the synthetic model: (record, STATE, E, the model)."""
    from romhighcontrast_amd.inverse import sensor_prior_factor
    md = model(N, K, M, NCAND)
    lay = ctx.sensor_dopt_layout(N, K)
    T0 = sensor_prior_factor(md["prior"], K)
    STATE, _ = ctx.sensor_dopt_init(N, K, ctx.upload(md["Ahat"]), ctx.upload(md["bhat"]), ctx.upload(md["theta"]), 0, K, M, T0, SIGMA)
    E, SCORE = ctx.upload(md["E"]), ctx.alloc(NCAND)
    call = lambda: ctx.sensor_dopt_scores(N, K, STATE, 0, M, E, 0, N, NCAND, SCORE=SCORE)  # noqa: E731
    med, lo, hi = _events_median(ctx, call, reps)
    _, prof = _profile(ctx, call)
    ms = sum(v["ms"] for k_, v in prof.items() if k_.startswith("dopt_score"))
    flops = 2.0 * M * lay["kp"] * lay["n_padded"] * NCAND
    rec = {"M": M, "ncand": NCAND, "n": N, "k": K, "kp": lay["kp"], "call_ms_median": med, "call_ms_min": lo, "call_ms_max": hi,
           "k_dopt_score_ms": ms, "k_dopt_score_tflops": flops / (ms * 1e-3) / 1e12, "profile": prof,
           "score_checksum": float(SCORE.download(NCAND).sum())}
    return rec, STATE, E, md


def plain_child(reps):
    """(child process, libromhc_oed_plain.so loaded) the scoring pass without log1p at the two sizes."""
    from romhighcontrast_amd import _ffi
    _ffi.load_library(PLAIN)
    ctx = _ffi.get_context()
    out = [{k_: v for k_, v in score_pass(ctx, M, reps)[0].items() if k_ != "profile"} for M in (1024, 1 << 14)]
    print("PLAIN " + json.dumps(out), flush=True)


def design_at_n8(ctx):
    from romhighcontrast_amd.inverse import ParameterLibrary
    from romhighcontrast_amd.lib.ReducedBasis import pod_modes, select_sensors_pbdw
    from romhighcontrast_amd.lib.SolutionsManagers import SolutionsManagerFEM, _as_device
    sm = SolutionsManagerFEM((2, 2), 8)
    rng = np.random.default_rng(5)
    U = sm.generate_solutions(10.0 ** rng.uniform(0.0, 2.0, size=(32, 2, 2)))
    basis, _ = pod_modes(sm._ctx, _as_device(sm._ctx, np.array(U), sm.vspace_dim), 6, center=False)
    a_lib = 10.0 ** rng.uniform(0.0, 2.0, size=(64, 2, 2))
    cand, m, sigma = sm.interior_vertices(), 8, 1e-3
    lib = ParameterLibrary(sm, basis, a_lib)
    des = lib.select_sensors(cand, m, sigma)
    pbdw = select_sensors_pbdw(sm, basis, cand, m)
    sets = {"d_optimal": des.points, "pbdw_greedy": pbdw.points, "random": cand[rng.choice(len(cand), size=m, replace=False)]}
    rows = np.arange(0, 64, 4)
    coef = lib.COEF.download(shape=(lib.M, lib.n))[rows]
    rec = {"geometry": "(2, 2), N = 8", "n": 6, "M": 64, "ncand": len(cand), "m": m, "sigma": sigma, "picks": [int(p) for p in des.picks],
           "information_nats": [float(v) for v in des.information], "pbdw_picks": [int(p) for p in pbdw.picks], "posterior": {}}
    for name, pts in sets.items():
        lib.observe(pts)
        Y = coef @ lib.E + sigma * rng.standard_normal((len(rows), len(pts)))
        post = lib.posterior(Y, sigma, t=4, steps=4000, burn=1000, seed=1)
        rec["posterior"][name] = {"points": len(pts), "median_sd": float(np.median(post.sd)), "mean_sd": float(post.sd.mean()),
                                  "rhat_max": float(np.nanmax(post.rhat))}
        if name == "d_optimal":
            rec["predicted_sd"] = des.posterior_sd[rows[:4]].tolist()
            rec["mcmc_sd"] = post.sd[:4].tolist()
            rec["median_predicted_sd"] = float(np.median(des.posterior_sd[rows]))
    return rec


def resources(path):
    """The compiler's report on the kernels of rom_oed.hip, as a table."""
    cmd = ["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", f"-I{ROOT}/include", f"-I{CSRC}", "-mllvm",
           "-pragma-unroll-threshold=10000000", "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(CSRC, "rom_oed.hip"), "-o", os.devnull]
    text = subprocess.run(cmd, capture_output=True, text=True, check=True).stderr
    rows, cur = [], None
    for line in text.splitlines():
        m = re.search(r"remark:\s+(Function Name|VGPRs|AGPRs|TotalSGPRs|SGPRs Spill|VGPRs Spill|ScratchSize \[bytes/lane\]|"
                      r"Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (\S+)", line)
        if not m:
            continue
        if m.group(1) == "Function Name":
            cur = {"name": subprocess.run(["c++filt", m.group(2)], capture_output=True, text=True).stdout.strip() or m.group(2)}
            rows.append(cur)
        elif cur is not None:
            cur[m.group(1)] = m.group(2)
    rows = [r for r in rows if "k_dopt" in r["name"]]   # (the headers bring kernels of their own along)
    keys = ["VGPRs", "AGPRs", "TotalSGPRs", "SGPRs Spill", "VGPRs Spill", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]", "LDS Size [bytes/block]"]
    lines = ["Kernel resource usage (hipcc -Rpass-analysis=kernel-resource-usage, --offload-arch=gfx950, the Makefile's flags) of the kernels of",
             "rom_oed.hip, written by tools/gpu_sensor_dopt.py --resources.  scratch: bytes per lane; occ: waves per SIMD as the compiler reports",
             "it from the registers; LDS: static bytes per workgroup.  The LDS of k_dopt_score is dynamic (the compiler reports 0):",
             "(128 + 64) (n_pad + 2) doubles -- 82 944 bytes at n = 50, 101 376 at n = 64 -- so one workgroup of 8 waves per CU, opted in above 64 KB.",
             "", f"{'kernel':<34s}  VGPRs  AGPRs  SGPRs  SGPR spills  VGPR spills  scratch  occ  static LDS"]
    for r in rows:
        name = re.sub(r"\(anonymous namespace\)::", "", r["name"]).split("(")[0].replace("void ", "")
        lines.append(f"{name:<34s}  " + "  ".join(f"{r.get(k_, '-'):>{w}s}" for k_, w in zip(keys, (5, 5, 5, 11, 11, 7, 3, 10))))
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--resources", default=None)
    ap.add_argument("--plain-child", action="store_true")
    args = ap.parse_args()
    if args.resources:
        resources(args.resources)
        if not args.out:
            return 0
    if args.plain_child:
        plain_child(args.reps)
        return 0
    from romhighcontrast_amd import _ffi
    from romhighcontrast_amd.inverse import sensor_dopt_scores_host, sensor_prior_factor, sensor_sensitivities_host
    ctx = _ffi.get_context()
    doc = {"device": ctx.device_name(), "n": N, "k": K, "ncand": NCAND, "m": PICKS, "sigma": SIGMA, "score_pass": [], "rom_gemm_nt": [],
           "k_nn_screen": [], "design": []}
    for M in (1024, 1 << 14):
        rec, STATE, E, md = score_pass(ctx, M, args.reps)
        doc["score_pass"].append(rec)
        print(json.dumps({k_: v for k_, v in rec.items() if k_ != "profile"}), flush=True)
        # the whole design: init and m steps
        T0 = sensor_prior_factor(md["prior"], K)
        A, b, TH = ctx.upload(md["Ahat"]), ctx.upload(md["bhat"]), ctx.upload(md["theta"])

        def design():
            ctx.sensor_dopt_init(N, K, A, b, TH, 0, K, M, T0, SIGMA, STATE=STATE)
            return ctx.sensor_dopt(N, K, STATE, 0, M, E, 0, N, NCAND, PICKS)

        med, lo, hi = _events_median(ctx, design, max(2, args.reps // 3))
        (picks, gain, info), prof = _profile(ctx, design)
        doc["design"].append({"M": M, "call_ms_median": med, "call_ms_min": lo, "call_ms_max": hi, "info": info, "profile": prof,
                              "picks": [int(p) for p in picks[:8]], "information_nats": float(gain.sum() / (2.0 * M))})
        print(json.dumps({"design_ms": med, "M": M}), flush=True)
        # rom_gemm_nt on the same product
        cols = min(M * rec["kp"], 1 << 14)
        rng = np.random.default_rng(1)
        Bm, Cb = ctx.upload(rng.random((cols, N))), ctx.alloc(NCAND * cols)
        gm, glo, ghi = _events_median(ctx, lambda: ctx.gemm_nt(NCAND, cols, N, E, 0, N, Bm, 0, N, Cb, 0, cols), args.reps)
        gtf = 2.0 * NCAND * cols * N / (gm * 1e-3) / 1e12
        doc["rom_gemm_nt"].append({"m": NCAND, "n": cols, "k": N, "ms_median": gm, "ms_min": glo, "ms_max": ghi, "tflops": gtf,
                                   "k_dopt_score_over_gemm": rec["k_dopt_score_tflops"] / gtf})
        del Cb
        # k_nn_screen on the problem of equal size
        if M == 1024:
            rows = M * rec["kp"]
            Q = ctx.upload(rng.random((rows, N)))
            (_, _, ninfo), nprof = _profile(ctx, lambda: ctx.nearest(Q, 0, N, rows, E, 0, N, NCAND, N, t=1, mode=0))
            nms = sum(v["ms"] for k_, v in nprof.items() if k_.startswith("nn_screen"))
            ntf = 2.0 * rows * NCAND * ((N + 3) // 4 * 4) / (nms * 1e-3) / 1e12
            doc["k_nn_screen"].append({"rows": rows, "queries": NCAND, "r": N, "ms": nms, "tflops": ntf, "over_gemm": ntf / gtf})
        print(json.dumps(doc["rom_gemm_nt"][-1]), flush=True)
    # the scoring pass without its log1p, in a child process on the A/B library
    if os.path.exists(PLAIN):
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--plain-child", "--reps", str(args.reps)], capture_output=True,
                             text=True, timeout=600)
        line = [ln for ln in out.stdout.splitlines() if ln.startswith("PLAIN ")]
        if line:
            doc["score_pass_without_log1p"] = json.loads(line[0][6:])
            for a, p in zip(doc["score_pass"], doc["score_pass_without_log1p"]):
                a["log1p_share_of_kernel"] = 1.0 - p["k_dopt_score_ms"] / a["k_dopt_score_ms"]
        else:
            doc["score_pass_without_log1p"] = {"error": out.stderr[-400:]}
    else:
        doc["score_pass_without_log1p"] = "not measured: libromhc_oed_plain.so is not built"
    # the NumPy specification's scoring pass, scaled
    md = model(N, K, 128, 2048)
    Z = sensor_sensitivities_host(md["Ahat"], md["bhat"], md["theta"]) @ sensor_prior_factor(md["prior"], K) / SIGMA
    t0 = time.perf_counter()
    sensor_dopt_scores_host(Z, md["E"])
    dt_ = time.perf_counter() - t0
    doc["numpy_specification"] = {"ncand": 2048, "M": 128, "score_pass_s": dt_,
                                  "scaled_score_pass_s": {str(M): dt_ * (NCAND / 2048.0) * (M / 128.0) for M in (1024, 1 << 14)}}
    doc["design_at_n8"] = design_at_n8(ctx)
    text = json.dumps(doc, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
