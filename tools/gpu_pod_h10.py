"""Timing of the H^1_0-POD (rom_pod_h10, rom_pod_h10_factored) and of the batched sine transform under it.

  python tools/gpu_pod_h10.py [--out profiles/pod_h10.json] [--configs C2 C4] [--reps 5]

* C2 ((2,2), N = 128, 1024 x 65 025) and C4 ((3,3), N = 171, 1024 x 262 144), n = 50, a sweep block of the BASELINE kind
  (coefficients 10^U(0,2)), centred;
* HIP-event times (the context's stopwatch around the call) of rom_pod_h10 and of rom_pod on the same block in the same
  process, alternated (rom_pod centres its input in place: it gets a fresh copy each time, made outside the timed region);
  medians and all samples;
* the two stages of the forward transform separately, from the library's per-kernel HIP-event records of one
  rom_sine_transform(0, 1) call over the block (sine_transform_c: the right factor, one NN product over the M nr rows;
  sine_transform_r: the strided-batched left factor), their rates, and the rate of both against the 43.5 TFLOP/s that
  k_gemm_nn reached for the same products in DESIGN.md 5.4;
* rom_pod_h10_factored against rom_pod_factored on the block's interface vectors (alternated), and the one-off cost of the
  H^1_0 map with its way back (rom_fem_energy_map, part 1).
Prints one JSON document (and writes it to --out)."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from romhighcontrast_amd import _ffi  # noqa: E402
from romhighcontrast_amd.lib.SolutionsManagers import SolutionsManagerFEM  # noqa: E402

GEMM_NN_REFERENCE_TFLOPS = 43.5   # k_gemm_nn on the transforms of rom_riesz_h10
PEAK_FP64_MFMA = 78.6e12
CONFIGS = {"C2": ((2, 2), 128, 1024), "C4": ((3, 3), 171, 1024)}


def _event_ms(ctx, fn):
    ctx.synchronize()
    ctx.timer_start()
    fn()
    return ctx.timer_stop()


def case(name, n, reps):
    ctx = _ffi.get_context()
    blocks, N, M = CONFIGS[name]
    sm = SolutionsManagerFEM(blocks, N)
    fem, dim, nr, nc = sm._fem, sm.vspace_dim, sm.nr_inner_vertices, sm.nc_inner_vertices
    a = 10.0 ** np.random.default_rng(20240807).uniform(0, 2, size=(M,) + blocks)
    Ud = sm.generate_solutions_device(a)
    fs = Ud.factored
    X, Xc = Ud.buf, ctx.alloc(M * dim)
    V = ctx.alloc(n * dim)
    out = {"config": name, "M": M, "dim": dim, "nr": nr, "nc": nc, "n": n,
           "transform_flops_block": 2.0 * M * (nr * nr * nc + nr * nc * nc)}
    h10 = lambda: fem.pod_h10(X, M, n, V, center=True)            # noqa: E731
    l2 = lambda: ctx.pod(Xc, M, dim, n, V, center=True)           # noqa: E731
    h10(), Xc.copy_from(X, M * dim), l2()                         # warm-up (tables, allocator)
    t_h, t_l = [], []
    for _ in range(reps):
        t_h.append(_event_ms(ctx, h10))
        Xc.copy_from(X, M * dim)
        t_l.append(_event_ms(ctx, l2))
    sig_h, info_h = h10()
    out["rom_pod_h10_ms"], out["rom_pod_h10_ms_all"] = float(np.median(t_h)), t_h
    out["rom_pod_ms"], out["rom_pod_ms_all"] = float(np.median(t_l)), t_l
    out["rom_pod_h10_info"] = info_h
    out["sigma_h10_first_last"] = [float(sig_h[0]), float(sig_h[-1])]
    # the forward transform alone: event time of the call, and its two stages from the per-kernel records
    W = ctx.alloc(M * dim)
    tr = lambda: fem.sine_transform(X, M, W, pre=0, post=1)       # noqa: E731
    tr()
    t_t = [_event_ms(ctx, tr) for _ in range(reps)]
    out["sine_transform_ms"], out["sine_transform_ms_all"] = float(np.median(t_t)), t_t
    ctx.profile(True)
    ctx.profile_reset()
    tr()
    rep = ctx.profile_report()
    ctx.profile(False)
    stages = {k: {"ms": v["total_ms"], "launches": v["launches"], "flops": v["flops"],
                  "tflops": v["flops"] / (v["total_ms"] * 1e-3) / 1e12 if v["total_ms"] > 0 else None}
              for k, v in rep.items() if k.startswith("sine_transform") and v["launches"]}
    out["stages"] = stages
    ms = sum(v["ms"] for v in stages.values())
    if ms > 0:
        rate = sum(v["flops"] for v in stages.values()) / (ms * 1e-3) / 1e12
        out["transform_tflops"] = rate
        out["transform_vs_gemm_nn_43p5"] = rate / GEMM_NN_REFERENCE_TFLOPS
        out["transform_share_of_fp64_mfma_peak"] = rate * 1e12 / PEAK_FP64_MFMA
    del W
    # factored: the one-off way back through the H^1_0 map, then both calls alternated
    if fs is not None:
        t0 = time.perf_counter()
        k1, _ = fem.energy_map(1)
        out["energy_map_h10_first_call_ms"] = 1e3 * (time.perf_counter() - t0)
        _, k2 = fem.energy_map(4)
        out["Kc"], out["k_h10"], out["k_l2"] = fs.map.Kc, k1, k2
        fh = lambda: fem.pod_h10_factored(fs.Yc, M, n, V, center=True)   # noqa: E731
        fl = lambda: fem.pod_factored(fs.Yc, M, n, V, center=True)       # noqa: E731
        fh(), fl()
        t_fh, t_fl = [], []
        for _ in range(reps):
            t_fh.append(_event_ms(ctx, fh))
            t_fl.append(_event_ms(ctx, fl))
        sig_f, info_f = fh()
        out["rom_pod_h10_factored_ms"], out["rom_pod_h10_factored_ms_all"] = float(np.median(t_fh)), t_fh
        out["rom_pod_factored_ms"], out["rom_pod_factored_ms_all"] = float(np.median(t_fl)), t_fl
        out["rom_pod_h10_factored_info"] = info_f
        k = min(info_h["resolved_modes"], info_f["resolved_modes"])
        out["max_rel_sigma_difference_rows_vs_factored"] = float(np.max(np.abs(sig_f[:k] - sig_h[:k]) / sig_h[0])) if k else None
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--configs", nargs="+", default=["C2", "C4"])
    ap.add_argument("--n", type=int, default=50)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    res = {"device": _ffi.get_context().device_name(), "gemm_nn_reference_tflops": GEMM_NN_REFERENCE_TFLOPS,
           "cases": [case(c, args.n, args.reps) for c in args.configs]}
    txt = json.dumps(res, indent=1)
    print(txt)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(txt + "\n")


if __name__ == "__main__":
    main()
