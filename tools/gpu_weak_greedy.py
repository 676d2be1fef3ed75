"""Timing of the residual estimator (rom_resid_eval) and of the weak greedy (rom_weak_greedy).

  python tools/gpu_weak_greedy.py [--out profiles/weak_greedy.json] [--n 50] [--reps 5] [--skip-c4]

* C2 ((2,2), N = 128, dim 65 025, k = 4): an estimator of n = 50 snapshots (coefficients 10^U(0,2)); rom_resid_eval alone at
  n = 50 for M in {2^10, 2^17, 2^20} (HIP-event times, median of --reps; the two kernels from the per-kernel records:
  reduced_solve and resid_eval, with the rate of the latter against its 2 M P rank flops);
* C2: the weak greedy to n = 50 over 2^17 parameters (wall time, picks, host synchronisations, final rank), and beside it
  the parent route on the same parameters -- sweep + rom_greedy_factored -- at the largest M (a power of two, at most 2^15)
  whose M x dim block fits half of the free device memory;
* C4 ((3,3), N = 171): the weak greedy on the bench's training parameters (bench.workload_parameters("c4")).
Prints one JSON document (and writes it to --out)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from romhighcontrast_amd import _ffi  # noqa: E402
from romhighcontrast_amd.lib.ReducedBasis import GREEDY_FOR_GALERKIN, GREEDY_FOR_RESIDUAL, ReducedBasisGreedy  # noqa: E402
from romhighcontrast_amd.lib.SolutionsManagers import SolutionsManagerFEM  # noqa: E402

SEED = 20240807


def _event_ms(ctx, fn):
    ctx.synchronize()
    ctx.timer_start()
    fn()
    return ctx.timer_stop()


def eval_records(ctx, sm, n, reps):
    blocks = sm.blocks_geometry
    rng = np.random.default_rng(SEED)
    basis = sm.generate_solutions_device(10.0 ** rng.uniform(0, 2, size=(n,) + tuple(blocks)), keep_interface_vectors=False)
    t0 = time.perf_counter()
    h = sm._fem.resid(n)
    h.append(basis.buf, n)
    ctx.synchronize()
    q = h.query()
    out = {"offline_s": time.perf_counter() - t0, "handle": q, "eval": []}
    for M in (1 << 10, 1 << 17, 1 << 20):
        a = ctx.upload(10.0 ** rng.uniform(0, 2, size=(M, q["k"])))
        D, Cf = ctx.alloc(M), ctx.alloc(M * n)
        run = lambda: h.eval(a, M, n, D, COEF=Cf)   # noqa: E731
        run()
        ts = [_event_ms(ctx, run) for _ in range(reps)]
        ctx.profile(True)
        ctx.profile_reset()
        run()
        rep = ctx.profile_report()
        ctx.profile(False)
        rec = {"M": M, "n": n, "P": q["P"], "rank": q["rank"], "ms": float(np.median(ts)), "ms_all": ts,
               "flops_thin_product": 2.0 * M * q["P"] * q["rank"]}
        for name in ("reduced_solve", "resid_eval"):
            if name in rep and rep[name]["launches"]:
                rec[name + "_ms"] = rep[name]["total_ms"]
        if rec.get("resid_eval_ms"):
            rec["resid_eval_tflops"] = rec["flops_thin_product"] / (rec["resid_eval_ms"] * 1e-3) / 1e12
        out["eval"].append(rec)
    h.free()
    return out


def weak_record(sm, a, n):
    t0 = time.perf_counter()
    rb = ReducedBasisGreedy(GREEDY_FOR_RESIDUAL).build(n, sm, None, a, criterion="bound")
    return {"M": len(a), "n": n, "wall_s": time.perf_counter() - t0, "info": rb.info, "picks_first10": rb.picks[:10],
            "criterion_first_last": [rb.max_errors[0], rb.max_errors[-1]]}


def parent_record(ctx, sm, a, n):
    import torch
    free, _ = torch.cuda.mem_get_info()
    M = 1 << 15
    while M > 64 and M * sm.vspace_dim * 8 > free // 2:
        M >>= 1
    a = a[:M]
    t0 = time.perf_counter()
    U = sm.generate_solutions_device(a)
    h1 = sm.H10norm(U)
    ctx.synchronize()
    t1 = time.perf_counter()
    rb = ReducedBasisGreedy(GREEDY_FOR_GALERKIN).build(n, sm, U, a, h1)
    return {"M": M, "n": n, "sweep_s": t1 - t0, "greedy_s": time.perf_counter() - t1, "picks_first10": list(rb.picks[:10])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--n", type=int, default=50)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--skip-c4", action="store_true")
    args = ap.parse_args()
    ctx = _ffi.get_context()
    res = {"device": ctx.device_name()}
    sm = SolutionsManagerFEM((2, 2), 128)
    res["c2_eval"] = eval_records(ctx, sm, args.n, args.reps)
    a = 10.0 ** np.random.default_rng(SEED + 1).uniform(0, 2, size=(1 << 17, 2, 2))
    res["c2_weak_greedy"] = weak_record(sm, a, args.n)
    res["c2_parent_route"] = parent_record(ctx, sm, a, args.n)
    if not args.skip_c4:
        import bench
        cfg = bench.CONFIGS["c4"]
        sm4 = SolutionsManagerFEM(cfg["blocks"], cfg["N"])
        res["c4_weak_greedy"] = weak_record(sm4, bench.workload_parameters("c4", cfg["blocks"], cfg["M"]), args.n)
    txt = json.dumps(res, indent=1)
    print(txt)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(txt + "\n")


if __name__ == "__main__":
    main()
