"""Timing of the H^1_0 Riesz representers (rom_riesz_h10) and of PBDW state estimation on the device.

  python tools/gpu_pbdw.py [--out FILE] [--skip-host]

* C2 ((2,2), N = 128), C4 ((3,3), N = 171), C5 ((4,4), N = 256); m = 50 and m = 200 random points; the Gram-only call
  and the call with representers: wall time (median of 3 after a warm-up) and the per-kernel profile of one call (the
  library's HIP-event records, riesz_*); the transforms' share of the fp64 MFMA peak (78.6 TFLOP/s);
* PBDW end to end at C2: M = 1024 snapshots, a greedy H^1_0 basis of n = 20, 50 sensors, the M states estimated;
* host baseline (unless --skip-host): one SciPy sparse LU factorisation of A_1 plus m solves, at C2 and C4.
Prints one JSON document (and writes it to --out)."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from romhighcontrast_amd import _ffi  # noqa: E402
from romhighcontrast_amd.lib import ReducedBasis as RB  # noqa: E402
from romhighcontrast_amd.lib.SolutionsManagers import SolutionsManagerFEM  # noqa: E402

PEAK_FP64_MFMA = 78.6e12
CONFIGS = {"C2": ((2, 2), 128), "C4": ((3, 3), 171), "C5": ((4, 4), 256)}


def _points(sm, m, seed):
    rng = np.random.default_rng(seed)
    return np.c_[rng.uniform(*sm.x_domain, m), rng.uniform(*sm.y_domain, m)]


def _median_ms(fn, reps=3):
    ctx = _ffi.get_context()
    fn()
    ts = []
    for _ in range(reps):
        ctx.synchronize()
        t0 = time.perf_counter()
        fn()
        ts.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(ts)), ts


def riesz_case(name, m):
    ctx = _ffi.get_context()
    blocks, N = CONFIGS[name]
    sm = SolutionsManagerFEM(blocks, N)
    nr, nc, dim = sm.nr_inner_vertices, sm.nc_inner_vertices, sm.vspace_dim
    pts = _points(sm, m, seed=m)
    ix, iy, tx, ty = sm._locate(pts)
    Om = ctx.alloc(m * dim)
    out = {"config": name, "m": m, "dim": dim, "nr": nr, "nc": nc,
           "transform_flops": 2.0 * m * (nr * nr * nc + nr * nc * nc), "gram_flops": float(m) * m * dim}
    out["gram_only_ms"], out["gram_only_ms_all"] = _median_ms(lambda: sm._fem.riesz_h10(ix, iy, tx, ty, OMEGA=None))
    out["full_ms"], out["full_ms_all"] = _median_ms(lambda: sm._fem.riesz_h10(ix, iy, tx, ty, OMEGA=Om))
    ctx.profile(True)
    ctx.profile_reset()
    sm._fem.riesz_h10(ix, iy, tx, ty, OMEGA=Om)
    rep = ctx.profile_report()
    ctx.profile(False)
    prof = {k: {"ms": v["total_ms"], "launches": v["launches"], "flops": v["flops"], "bytes": v["bytes"]}
            for k, v in sorted(rep.items(), key=lambda kv: -kv[1]["total_ms"]) if v["launches"]}
    out["profile"] = prof
    tr = [v for k, v in prof.items() if k.startswith("riesz_transform")]
    t_ms = sum(v["ms"] for v in tr)
    out["transforms_ms"] = t_ms
    if t_ms > 0:
        out["transforms_tflops"] = sum(v["flops"] for v in tr) / (t_ms * 1e-3) / 1e12
        out["transforms_share_of_fp64_mfma_peak"] = out["transforms_tflops"] * 1e12 / PEAK_FP64_MFMA
    del Om
    return out


def host_baseline(name, m):
    import scipy.sparse as sp
    import scipy.sparse.linalg as spla
    blocks, N = CONFIGS[name]
    nr, nc = blocks[0] * N - 1, blocks[1] * N - 1
    Tr = sp.diags([-np.ones(nr - 1), 2 * np.ones(nr), -np.ones(nr - 1)], [-1, 0, 1])
    Tc = sp.diags([-np.ones(nc - 1), 2 * np.ones(nc), -np.ones(nc - 1)], [-1, 0, 1])
    A = (sp.kron(Tr, sp.eye(nc)) + sp.kron(sp.eye(nr), Tc)).tocsc()
    rng = np.random.default_rng(m)
    R = np.zeros((nr * nc, m))
    R[rng.integers(0, nr * nc, m), np.arange(m)] = 1.0
    t0 = time.perf_counter()
    lu = spla.splu(A)
    t1 = time.perf_counter()
    lu.solve(R)
    t2 = time.perf_counter()
    return {"config": name, "m": m, "factor_ms": 1e3 * (t1 - t0), "solves_ms": 1e3 * (t2 - t1),
            "total_ms": 1e3 * (t2 - t0)}


def pbdw_c2():
    ctx = _ffi.get_context()
    blocks, N, M, n, m = (2, 2), 128, 1024, 20, 50
    rng = np.random.default_rng(20240807)
    a = 10.0 ** rng.uniform(0, 2, size=(M,) + blocks)
    sm = SolutionsManagerFEM(blocks, N)
    Ud = sm.generate_solutions_device(a)
    rb = RB.ReducedBasisGreedy(RB.GREEDY_FOR_H10).build(n, sm, Ud, a, sm.H10norm(Ud))
    C = np.asarray(rb.basis)
    pts = _points(sm, m, seed=7)
    Y = sm.evaluate_solutions(pts, Ud)
    out = {"config": "C2", "M": M, "n": n, "m": m}
    run = lambda: RB.pbdw_state_estimation(sm, C, pts, Y, device=True)  # noqa: E731
    out["pbdw_device_ms"], out["pbdw_device_ms_all"] = _median_ms(run)
    r = run()
    out["beta_n"] = float(r.beta[-1])
    err = sm.H10norm_diff(r.estimates, Ud) / sm.H10norm(Ud)
    out["median_rel_h10_error"] = float(np.median(err))
    out["max_rel_h10_error"] = float(np.max(err))
    ctx.profile(True)
    ctx.profile_reset()
    run()
    rep = ctx.profile_report()
    ctx.profile(False)
    out["profile"] = {k: {"ms": v["total_ms"], "launches": v["launches"]}
                      for k, v in sorted(rep.items(), key=lambda kv: -kv[1]["total_ms"]) if v["launches"]}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--skip-host", action="store_true")
    args = ap.parse_args()
    res = {"device": _ffi.get_context().device_name(), "peak_fp64_mfma_tflops": PEAK_FP64_MFMA / 1e12}
    res["riesz"] = [riesz_case(c, m) for c in ("C2", "C4", "C5") for m in (50, 200)]
    res["pbdw_c2"] = pbdw_c2()
    if not args.skip_host:
        res["host_baseline"] = [host_baseline(c, m) for c in ("C2", "C4") for m in (50, 200)]
    txt = json.dumps(res, indent=1)
    print(txt)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(txt + "\n")


if __name__ == "__main__":
    main()
