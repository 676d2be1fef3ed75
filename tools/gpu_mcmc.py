"""Timing of the posterior sampler (rom_mcmc) beside the device polish, and the library posterior end to end.

  python tools/gpu_mcmc.py [--out profiles/mcmc.json] [--reps 10] [--skip-end-to-end]

* rom_mcmc at (n, k, r) = (50, 4, 39) and (64, 16, 64), K t = 4096 and 2^15 chains (t = 4) of 512 steps (burn 128, no samples):
  the synthetic reduced model and the noisy data of tools/gpu_lm_polish.py, sigma = 1e-3 max|p|, L = proposal_factors at theta*.  The whole call between
  HIP events on the context stream, median of --reps after one untimed call; the call time per (chain, step) -- a THROUGHPUT
  figure over all resident workgroups -- and per evaluation of the model (proposals outside the box are not evaluated).
* THE YARDSTICK, in the same run: rom_lm_polish at the same shape and the same systems (measure_kernel of tools/gpu_lm_polish.py),
  its call time per factorisation; the ratio step / factorisation, against the expectation of at most 1.25 (recorded with
  `expectation_met`; no exit status depends on it).
* the specification on the host (inverse.mcmc_host) at (50, 4, 39): 64 chains of 32 steps, wall clock per (chain, step), for
  information.
* the library posterior end to end at C2 ((2, 2), N = 128), n = 50, m = 200, a library of 2^17 parameters, K = 1024 measurement
  vectors with noise 1e-3, t = 4, 2000 steps (burn 500, thin 10): wall clock of ParameterLibrary.posterior, the median R-hat, the
  acceptance, and the coverage of the true log a by the 90 % intervals (the ROM's own error biases it: reported, not gated).
Prints one JSON document (and writes it to --out)."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gpu_lm_polish import _events_median, measure_kernel, synth  # noqa: E402
from romhighcontrast_amd import _ffi  # noqa: E402
from romhighcontrast_amd.inverse import mcmc_host, mcmc_layout, proposal_factors  # noqa: E402

STEPS, BURN = 512, 128


def _case(n, k, r, K, t):
    Ahat, bhat, Gr = synth(n, k, r, 7)
    rng = np.random.default_rng(K)
    hi = np.log(100.0)
    theta = rng.uniform(0.2, hi - 0.2, size=(K, k))
    A = np.einsum("bq,qij->bij", np.exp(theta), Ahat)
    P = np.linalg.solve(A, np.broadcast_to(bhat, (K, n))[..., None])[..., 0] @ Gr.T
    sigma = 1e-3 * np.abs(P).max(axis=1)
    P = P + sigma[:, None] * rng.standard_normal(P.shape)
    theta0 = theta[:, None, :] + 0.1 * rng.standard_normal((K, t, k))
    L = proposal_factors(Ahat, bhat, Gr, theta, 1.0 / sigma ** 2, 0.0, hi)
    return Ahat, bhat, Gr, P, 1.0 / sigma ** 2, theta0, L, hi


def measure_sampler(ctx, n, k, r, K, t, reps):
    Ahat, bhat, Gr, P, invvar, theta0, L, hi = _case(n, k, r, K, t)
    o = mcmc_layout(n, k)
    rows = np.zeros((K * t, o["row"]))
    rows[:, :k] = theta0.reshape(K * t, k)
    dA, db, dG, dP, dI, dL = (ctx.upload(x) for x in (Ahat, bhat, Gr, P, invvar, L))
    STATE = ctx.upload(rows)

    def call():   # (a fresh run every time: step0 = 0 reads the first k columns only, which hold the previous run's last state)
        return ctx.mcmc(n, k, r, dA, db, dG, dP, 0, r, K, t, dI, dL, 0.0, hi, 11, STEPS, BURN, 1, STATE)

    med, lo, hi_ms = _events_median(ctx, call, reps)
    info = call()
    st = STATE.download().reshape(K * t, o["row"])
    return {"n": n, "k": k, "r": r, "K": K, "t": t, "chains": K * t, "steps": STEPS, "burn": BURN, "call_ms_median": med, "call_ms_min": lo,
            "call_ms_max": hi_ms, "reps": reps, "info": info, "acceptance": float((st[:, o["accepted"]] / st[:, o["kept"]]).mean()),
            "outside_share": float(st[:, o["outside"]].sum() / (K * t * STEPS)),
            "us_per_step": 1e3 * med / (K * t * STEPS), "us_per_evaluation": 1e3 * med / info["evaluations"]}


def measure_host(n, k, r, chains=64, steps=32):
    Ahat, bhat, Gr, P, invvar, theta0, L, hi = _case(n, k, r, chains, 1)
    t0 = time.perf_counter()
    mcmc_host(Ahat, bhat, Gr, P, invvar, theta0, L, 0.0, hi, 11, steps, steps // 4, 1, slots=0)
    dt = time.perf_counter() - t0
    return {"n": n, "k": k, "r": r, "chains": chains, "steps": steps, "wall_s": dt, "us_per_step": 1e6 * dt / (chains * steps)}


def library_end_to_end(K=1024, n=50, m=200, M=1 << 17, t=4, steps=2000, burn=500, thin=10):
    from romhighcontrast_amd.inverse import ParameterLibrary
    from romhighcontrast_amd.lib.SolutionsManagers import SolutionsManagerFEM
    rng = np.random.default_rng(0)
    sm = SolutionsManagerFEM((2, 2), 128)
    ctx = sm._ctx
    basis = sm.generate_solutions_device(10.0 ** rng.uniform(0, 2, size=(n, 2, 2)))
    a_lib = 10.0 ** rng.uniform(0, 2, size=(M, 4))
    points = rng.uniform(-0.95, 0.95, size=(m, 2))
    a_true = 10.0 ** rng.uniform(0, 2, size=(K, 2, 2))
    Y = sm.evaluate_solutions(points, sm.generate_solutions_device(a_true))
    sigma = 1e-3 * np.abs(Y).max(axis=1)
    Y = Y + sigma[:, None] * rng.standard_normal(Y.shape)
    lib = ParameterLibrary(sm, basis, a_lib).observe(points)

    def wall():
        ctx.synchronize()
        t0 = time.perf_counter()
        post = lib.posterior(Y, sigma, t=t, steps=steps, burn=burn, thin=thin, seed=1)
        ctx.synchronize()
        return 1e3 * (time.perf_counter() - t0), post

    wall()
    runs = [wall() for _ in range(3)]
    post = runs[0][1]
    q = post.quantiles([0.05, 0.95])
    truth = np.log(a_true.reshape(K, 4))
    return {"geometry": "(2, 2), N = 128", "n": n, "m": m, "M": M, "K": K, "t": t, "noise": 1e-3, "r": int(lib.r), "steps": steps, "burn": burn,
            "thin": thin, "posterior_ms_median": float(np.median([r_[0] for r_ in runs])), "posterior_ms_all": [r_[0] for r_ in runs],
            "rhat_median": float(np.nanmedian(post.rhat)), "rhat_share_below_1p1": float(np.nanmean(post.rhat < 1.1)),
            "acceptance_mean": float(post.acceptance.mean()), "coverage_90": float(((q[0] <= truth) & (truth <= q[1])).mean()),
            "median_sd_log_a": float(np.median(post.sd)), "outside_share": float(post.outside.sum() / (K * t * steps)),
            "not_spd": int(post.not_spd.sum())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--skip-end-to-end", action="store_true")
    args = ap.parse_args()
    ctx = _ffi.get_context()
    doc = {"device": ctx.device_name(), "sampler": [], "expected_ratio_at_most": 1.25}
    for n, k, r in ((50, 4, 39), (64, 16, 64)):
        for K in (1024, 8192):
            rec = measure_sampler(ctx, n, k, r, K, 4, args.reps)
            pol = measure_kernel(ctx, n, k, r, K, 4, args.reps)
            rec["lm_polish_same_run"] = {q: pol[q] for q in ("call_ms_median", "call_ms_min", "call_ms_max", "info", "us_per_factorisation")}
            rec["step_over_factorisation"] = rec["us_per_step"] / pol["us_per_factorisation"]
            rec["evaluation_over_factorisation"] = rec["us_per_evaluation"] / pol["us_per_factorisation"]
            rec["expectation_met"] = bool(rec["step_over_factorisation"] <= 1.25)
            doc["sampler"].append(rec)
            print(json.dumps({q: rec[q] for q in ("n", "k", "r", "chains", "call_ms_median", "us_per_step", "us_per_evaluation",
                                                  "step_over_factorisation", "acceptance")}), flush=True)
    doc["host_specification"] = measure_host(50, 4, 39)
    print(json.dumps(doc["host_specification"]), flush=True)
    if not args.skip_end_to_end:
        doc["library_posterior_c2"] = library_end_to_end()
    text = json.dumps(doc, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
