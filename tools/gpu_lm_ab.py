"""Two builds of libromhc.so side by side on rom_lm_polish and rom_poly_sense: the same bits, the same speed.

  python tools/gpu_lm_ab.py --lib PATH --out RUN.npz [--reps 10]       one process, one library: records a run
  python tools/gpu_lm_ab.py --compare A1.npz A2.npz .. B1.npz B2.npz .. [--out profiles/lm_drive_ab.json]      (host only)

A process loads one library, so a comparison is made of runs recorded by separate processes.  A run holds

* the raw OUT of both entries on seeded inputs, with the info dictionary of every call: rom_lm_polish on the SHAPES of
  tests/test_gpu_lm_polish.py (ROM-exact data at max_iter 0, 1, 2, 30; data with noise 1e-3 max|p| and an aux block at 30) and
  rom_poly_sense on the SHAPES of tests/test_gpu_poly_sense.py (exact data at max_iter 0, 1, 2, 30; at 30 noisy data, one pinned
  coordinate, every coordinate pinned, starts outside the box).  The noisy cases are there to reach rejected trials, the stuck
  rule and the polish's re-factorisation: `reached` records per noisy case whether iterations < max_iter B and (polish)
  factorisations > iterations + B;
* the time of whole calls between device events on the context stream, median of --reps after one untimed call, at 4096 systems
  (K = 1024, t = 4) and the shapes of tools/gpu_lm_polish.py and tools/gpu_poly_sense.py.

--compare takes the runs of library A (the first half of the list) and of library B (the second half).  Bits: every OUT byte and
every info entry of every run must equal those of the first.  Speed, per shape: the spread of A is max / min of its medians; B's
median of medians may exceed A's by no more than that spread; a spread above 10 % marks the comparison as disturbed (repeat it).
Exit status 1 unless the bits are identical and every shape passes."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402


def record(lib_path, out, reps):
    from romhighcontrast_amd import _ffi
    _ffi.load_library(os.path.abspath(lib_path))   # before anything else: every later load_library() returns this one
    import lm_truth as lt
    import sense_truth as st
    import test_gpu_lm_polish
    import test_poly_sense_host
    from gpu_lm_polish import _events_median
    from romhighcontrast_amd.nonlinear import legendre_features
    ctx = _ffi.get_context()
    raw, infos, reached = {}, {}, {}

    def polish(name, model, P, theta0, aux, max_iter):
        n, k, r = model["n"], model["k"], model["r"]
        K, t = theta0.shape[:2]
        OUT = ctx.upload(np.full(K * (k + n + 5), np.nan))
        _, info = ctx.lm_polish(n, k, r, ctx.upload(model["Ahat"]), ctx.upload(model["bhat"]), ctx.upload(model["Gr"]), ctx.upload(P), 0,
                                r, K, t, ctx.upload(theta0), model["lo"], model["hi"], AUX=None if aux is None else ctx.upload(aux),
                                max_iter=max_iter, OUT=OUT)
        raw[name], infos[name] = OUT.download().view(np.uint8), info
        return info

    def sense(name, model, P, T0, max_iter):
        m, d, r = model["m"], model["d"], model["r"]
        K, t = T0.shape[:2]
        OUT = ctx.upload(np.full(K * (m + 5), np.nan))
        _, info = ctx.poly_sense(m, d, r, ctx.upload(model["Gr"]), ctx.upload(P), 0, r, K, t, ctx.upload(T0), model["lo"], model["hi"],
                                 max_iter=max_iter, OUT=OUT)
        raw[name], infos[name] = OUT.download().view(np.uint8), info
        return info

    for n, k, r, K, t in test_gpu_lm_polish.SHAPES:
        tag = f"polish_{n}x{k}x{r}x{K}x{t}"
        model = lt.synth(n, k, r, 7)
        theta_true, P = lt.exact_queries(model, K, 7)
        theta0 = theta_true[:, None, :] + 0.1 * np.random.default_rng(8).standard_normal((K, t, k))
        for max_iter in (0, 1, 2, 30):
            polish(f"{tag}_exact_{max_iter}", model, P, theta0, None, max_iter)
        rng = np.random.default_rng(12)
        noisy = P + 1e-3 * np.abs(P).max(axis=1, keepdims=True) * rng.standard_normal(P.shape)
        aux = np.stack([rng.uniform(0.0, 1e-6, K) * np.abs(noisy).max(axis=1) ** 2, np.abs(noisy).max(axis=1)], axis=1)
        info = polish(f"{tag}_noisy_30", model, noisy, theta0, aux, 30)
        reached[f"{tag}_noisy_30"] = {"stopped_early": info["iterations"] < 30 * K * t,
                                      "rejected_trials": info["factorisations"] > info["iterations"] + K * t}

    for shape in test_poly_sense_host.SHAPES:
        m, d, r, K, t = shape
        tag = "sense_" + "x".join(map(str, shape))
        model, t_true, P, T0 = test_poly_sense_host.case(*shape)
        for max_iter in (0, 1, 2, 30):
            sense(f"{tag}_exact_{max_iter}", model, P, T0, max_iter)
        noisy = P + 1e-3 * np.random.default_rng(12).standard_normal(P.shape)
        info = sense(f"{tag}_noisy_30", model, noisy, T0, 30)
        # (a trial costs one evaluation, an iteration one more, the start and the end one each)
        reached[f"{tag}_noisy_30"] = {"stopped_early": info["iterations"] < 30 * K * t,
                                      "rejected_trials": info["evaluations"] > 2 * info["iterations"] + 2 * K * t}
        one = dict(model, lo=model["lo"].copy(), hi=model["hi"].copy())
        one["lo"][m // 2] = one["hi"][m // 2] = 0.25
        sense(f"{tag}_one_pinned_30", one, P, T0, 30)
        sense(f"{tag}_all_pinned_30", dict(model, lo=np.full(m, 0.25), hi=np.full(m, 0.25)), P, T0, 30)
        wild = T0.copy()
        wild[..., 0] -= 9.0
        wild[..., -1] += 9.0
        sense(f"{tag}_outside_30", model, P, wild, 30)

    timing = {}
    K, t = 1024, 4
    for n, k, r in ((50, 4, 39), (64, 16, 64)):   # tools/gpu_lm_polish.py::measure_kernel
        model = lt.synth(n, k, r, 7)
        Ahat, bhat, Gr = model["Ahat"], model["bhat"], model["Gr"]
        rng = np.random.default_rng(K)
        hi = np.log(100.0)
        theta = rng.uniform(0.2, hi - 0.2, size=(K, k))
        P = lt.coefficients(model, theta) @ Gr.T
        P = P + 1e-3 * np.abs(P).max(axis=1, keepdims=True) * rng.standard_normal(P.shape)
        theta0 = theta[:, None, :] + 0.1 * rng.standard_normal((K, t, k))
        dA, db, dG, dP, dT = ctx.upload(Ahat), ctx.upload(bhat), ctx.upload(Gr), ctx.upload(P), ctx.upload(theta0)
        OUT = ctx.alloc(K * (k + n + 5))
        med, lo, hi_ms = _events_median(
            ctx, lambda: ctx.lm_polish(n, k, r, dA, db, dG, dP, 0, r, K, t, dT, 0.0, hi, misfit_tol=2e-3 * np.sqrt(r), OUT=OUT), reps)
        timing[f"polish_n{n}_k{k}_r{r}"] = {"call_ms_median": med, "call_ms_min": lo, "call_ms_max": hi_ms}
        raw[f"timed_polish_n{n}_k{k}_r{r}"] = OUT.download().view(np.uint8)
    for m, d, r in ((4, 2, 8), (4, 4, 12), (12, 2, 40)):   # tools/gpu_poly_sense.py::measure_kernel
        pw = _ffi.poly_terms(m, d).astype(np.int64)
        Gr = np.random.default_rng(7).standard_normal((r, len(pw))) * (0.3 ** np.maximum(pw.sum(axis=1) - 1, 0))[None, :]
        rng = np.random.default_rng(K)
        t_true = rng.uniform(-0.9, 0.9, size=(K, m))
        P = legendre_features(t_true, pw, False)[0] @ Gr.T
        P = P + 1e-3 * np.abs(P).max(axis=1, keepdims=True) * rng.standard_normal(P.shape)
        T0 = t_true[:, None, :] + 0.1 * rng.standard_normal((K, t, m))
        dG, dP, dT = ctx.upload(Gr), ctx.upload(P), ctx.upload(T0)
        OUT = ctx.alloc(K * (m + 5))
        med, lo, hi_ms = _events_median(
            ctx, lambda: ctx.poly_sense(m, d, r, dG, dP, 0, r, K, t, dT, -1.5, 1.5, misfit_tol=2e-3 * np.sqrt(r), OUT=OUT), reps)
        timing[f"sense_m{m}_d{d}_r{r}"] = {"call_ms_median": med, "call_ms_min": lo, "call_ms_max": hi_ms}
        raw[f"timed_sense_m{m}_d{d}_r{r}"] = OUT.download().view(np.uint8)

    meta = {"lib": lib_path, "device": ctx.device_name(), "reps": reps, "systems_timed": K * t, "info": infos, "reached": reached,
            "timing": timing}
    np.savez(out, meta=np.array(json.dumps(meta)), **raw)
    print(json.dumps({"lib": lib_path, "cases": len(raw), "reached": reached, "timing": timing}, indent=1))
    return 0


def compare(paths, out):
    assert len(paths) >= 2 and len(paths) % 2 == 0, "--compare takes as many runs of library B as of library A"
    runs = [np.load(p) for p in paths]
    metas = [json.loads(str(run["meta"])) for run in runs]
    half = len(paths) // 2
    first, names = runs[0], sorted(q for q in runs[0].files if q != "meta")
    different = []
    for path, run, meta in zip(paths[1:], runs[1:], metas[1:]):
        if sorted(q for q in run.files if q != "meta") != names:
            different.append(f"{path}: other cases")
            continue
        different += [f"{path}: OUT of {q}" for q in names if not np.array_equal(run[q], first[q])]
        different += [f"{path}: info of {q}" for q in metas[0]["info"] if meta["info"][q] != metas[0]["info"][q]]
    doc = {"device": metas[0]["device"], "runs_a": paths[:half], "runs_b": paths[half:], "lib_a": metas[0]["lib"], "lib_b": metas[half]["lib"],
           "cases": len(names), "out_bytes_compared": int(sum(first[q].size for q in names)), "bits_identical": not different,
           "different": different, "reached": metas[0]["reached"],
           "noisy_cases_that_stopped_early": sum(v["stopped_early"] for v in metas[0]["reached"].values()),
           "noisy_cases_with_rejected_trials": sum(v["rejected_trials"] for v in metas[0]["reached"].values()),
           "reps": metas[0]["reps"], "systems_timed": metas[0]["systems_timed"], "timing": {}}
    for shape in metas[0]["timing"]:
        a = [meta["timing"][shape]["call_ms_median"] for meta in metas[:half]]
        b = [meta["timing"][shape]["call_ms_median"] for meta in metas[half:]]
        spread = max(a) / min(a)
        ratio = float(np.median(b) / np.median(a))
        doc["timing"][shape] = {"a_call_ms_medians": a, "b_call_ms_medians": b, "a_spread": spread, "b_over_a": ratio,
                                "disturbed": bool(spread > 1.10), "passes": bool(ratio <= spread)}
    doc["speed_passes"] = all(v["passes"] for v in doc["timing"].values())
    doc["disturbed"] = any(v["disturbed"] for v in doc["timing"].values())
    text = json.dumps(doc, indent=1)
    print(text)
    if out:
        with open(out, "w") as f:
            f.write(text + "\n")
    return 0 if doc["bits_identical"] and doc["speed_passes"] else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=None)
    ap.add_argument("--compare", nargs="+", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=10)
    args = ap.parse_args()
    if args.compare:
        return compare(args.compare, args.out)
    assert args.lib and args.out, "--lib PATH --out RUN.npz, or --compare"
    return record(args.lib, args.out, args.reps)


if __name__ == "__main__":
    sys.exit(main())
