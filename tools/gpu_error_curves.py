"""Timing of the all-dimensions error curves (rom_error_curves) on the device.

  python tools/gpu_error_curves.py [--per-n-dims K] [--out FILE]

* C2 ((2,2), N = 128, M = 1024, a = 10^U(0, 2) from seed 20240807), four builders (Random, Random without the INFINIT_A
  lead, Greedy H^1_0, Greedy Galerkin) with vn_max_dim = 50: experiment_statistics on the same snapshots and bases, once
  with all_dims=True (n = 1 .. 50) and once with the per-n loop (n = 1 .. K, default 50; the per-n loop costs about the
  same for every n, so a smaller K still gives its cost per n);
* C4 ((3,3), N = 171, M = 1024, the BASELINE parameters, contrast 1e8): the bare call on a greedy basis of n = 50, with
  and without parameters, and the per-kernel profile of the call.
Prints one JSON document (and writes it to --out)."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from romhighcontrast_amd import _ffi  # noqa: E402
from romhighcontrast_amd import experiments as X  # noqa: E402
from romhighcontrast_amd.lib import ReducedBasis as RB  # noqa: E402
from romhighcontrast_amd.lib.SolutionsManagers import SolutionsManagerFEM  # noqa: E402


def c2_statistics(per_n_dims):
    ctx = _ffi.get_context()
    blocks, N, M, nb = (2, 2), 128, 1024, 50
    rng = np.random.default_rng(20240807)
    a = 10.0 ** rng.uniform(0, 2, size=(M,) + blocks)
    sm = SolutionsManagerFEM(blocks, N)
    U = sm.generate_solutions(a)
    h1 = sm.H10norm(U)
    builders = [RB.ReducedBasisRandom(), RB.ReducedBasisRandom(False), RB.ReducedBasisGreedy(RB.GREEDY_FOR_H10),
                RB.ReducedBasisGreedy(RB.GREEDY_FOR_GALERKIN)]
    bases = {b.name: b.build(n=nb, sm=sm, solutions2train=U, a2train=a, solutions2train_h1norm=h1) for b in builders}

    def fresh():
        d = {"solutions": U, "solutions_H1norm": h1, "time2calculate_solutions": 0.0, "time2calculate_h1norm": 0.0}
        for b in builders:
            d[b.name] = {"errors": {}, "times": {}, "basis": bases[b.name], "time2build": 0.0}
        return d

    out = {"config": "C2", "M": M, "dim": sm.vspace_dim, "builders": [b.name for b in builders], "n_max": nb}
    X.experiment_statistics(sm, a, builders, vn_max_dim=4, data=fresh(), all_dims=True)   # warm-up (code objects, allocator)
    ctx.synchronize()
    d = fresh()
    np.random.seed(1)
    t0 = time.perf_counter()
    X.experiment_statistics(sm, a, builders, vn_max_dim=nb, data=d, all_dims=True)
    out["all_dims_s"] = time.perf_counter() - t0
    out["all_dims_time2curves_s"] = {b.name: d[b.name]["time2curves"] for b in builders}
    d0 = fresh()
    np.random.seed(1)
    t0 = time.perf_counter()
    X.experiment_statistics(sm, a, builders, vn_max_dim=nb, vn_max_dim2do_stats=per_n_dims, data=d0)
    out["per_n_dims"] = per_n_dims
    out["per_n_s"] = time.perf_counter() - t0
    out["per_n_s_per_dim"] = out["per_n_s"] / per_n_dims
    worst = 0.0
    for b in builders:
        for n in range(1, per_n_dims + 1):
            for f in ("forward_modeling", "projection"):
                x, y = np.asarray(getattr(d[b.name]["errors"][n], f)), np.asarray(getattr(d0[b.name]["errors"][n], f))
                worst = max(worst, float(np.max(np.abs(x - y))))
    out["max_abs_diff_of_fm_pj_records_vs_per_n"] = worst   # (the records are relative errors)
    return out


def c4_bare_call():
    ctx = _ffi.get_context()
    blocks, N, M, nb = (3, 3), 171, 1024, 50
    rng = np.random.default_rng(20240807)
    a = np.ones((M, 3, 3))
    for j in range(9):
        a[1 + j].flat[j] = 1e8
    a[10] = 1e8
    a[11:] = 10.0 ** rng.uniform(0, 8, size=(M - 11, 3, 3))
    sm = SolutionsManagerFEM(blocks, N)
    Ud = sm.generate_solutions_device(a)
    h1 = sm.H10norm(Ud)
    rb = RB.ReducedBasisGreedy(RB.GREEDY_FOR_H10).build(nb, sm, Ud, a, h1)
    C = np.asarray(rb.basis)
    a_dev = ctx.upload(sm._a_batch(a))
    out = {"config": "C4", "M": M, "dim": sm.vspace_dim, "n": nb}
    for label, aa in (("proj_only", None), ("proj_and_galerkin", a_dev)):
        sm.error_curves(Ud, C, a=aa)
        ts = []
        for _ in range(3):
            ctx.synchronize()
            t0 = time.perf_counter()
            proj, gal, P, T, info = sm.error_curves(Ud, C, a=aa)
            ts.append(time.perf_counter() - t0)
        out[label + "_ms"] = [1e3 * t for t in ts]
        out[label + "_info"] = info
    ctx.profile(True)
    ctx.profile_reset()
    sm.error_curves(Ud, C, a=a_dev)
    rep = ctx.profile_report()
    ctx.profile(False)
    out["profile"] = {k: {"ms": v["total_ms"], "launches": v["launches"], "flops": v["flops"], "bytes": v["bytes"]}
                      for k, v in sorted(rep.items(), key=lambda kv: -kv[1]["total_ms"]) if v["launches"]}
    out["max_rel_proj_err_n50"] = float(np.max(proj[nb] / h1))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--per-n-dims", type=int, default=50)
    ap.add_argument("--out", default=None)
    ap.add_argument("--skip-c2", action="store_true")
    args = ap.parse_args()
    res = {"device": _ffi.get_context().device_name()}
    res["c4"] = c4_bare_call()
    if not args.skip_c2:
        res["c2"] = c2_statistics(args.per_n_dims)
    txt = json.dumps(res, indent=1)
    print(txt)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(txt + "\n")


if __name__ == "__main__":
    main()
