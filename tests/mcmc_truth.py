"""Truth for the posterior sampler rom_mcmc / inverse.mcmc_host (tests/test_mcmc_host.py, tests/test_gpu_mcmc.py): posterior
moments by quadrature in long double, the bound that holds one arithmetic to another's trajectory, and a checker of state rows
that holds for any run.  A helper, not a test file.  TEST INFRASTRUCTURE."""
import numpy as np

import lm_truth as lt

LD = np.longdouble
EPS = lt.EPS

# The trajectory bound.  Two arithmetics that take the same decisions (the comparison stops before the first step whose decision
# margin |log u - l| is below 1e-9) differ in theta only by the rounding of what a step ADDS: theta' = theta + s (L xi) is k
# multiply-adds for a row of L xi, one product with s and one sum -- k + 2 roundings, each of a quantity no larger than
# max(|theta|, hi - lo), since an accepted proposal lies in the box -- and the normals' own rounding (a logarithm, a root, a cosine:
# a few units each) rides on the same terms.  The errors of the steps add up, so after `steps` steps |d theta| <= c steps (k + 2) eps
# max(1, max|theta|, hi - lo).  The n unknowns of the model enter once more through alpha = e^l in the adaptation of the scale
# (ls sums alpha (i + 1)^-0.6, the scale multiplies every later step): the term n eps.  C = 64 is the constant that
# tests/lm_truth.py puts before the n eps of the same factorisation and solve; it was fixed before any run of the device.
TRAJECTORY_C = 64.0
MARGIN = 1e-9


def trajectory_bound(steps, k, n, theta_max, lo, hi):
    """B = C (steps (k + 2) + n) eps max(1, max|theta|, hi - lo)."""
    return TRAJECTORY_C * (steps * (k + 2) + n) * EPS * max(1.0, float(theta_max), float(np.max(np.asarray(hi) - np.asarray(lo))))


def potential(model, p, theta):
    """Phi(theta) = |p - G_r c(theta)|^2 for the rows of theta (B, k) in long double: Gaussian elimination of A(theta) c = bhat
    without pivoting (A is positive definite), one query p (r,) or one per row (B, r)."""
    theta = np.asarray(theta, dtype=LD)
    A = np.einsum("bq,qij->bij", np.exp(theta), model["Ahat"].astype(LD))
    B, n = A.shape[0], A.shape[1]
    b = np.array(np.broadcast_to(model["bhat"].astype(LD), (B, n)))
    for j in range(n):
        f = A[:, j + 1:, j] / A[:, j, j, None]
        A[:, j + 1:, :] -= f[:, :, None] * A[:, j, None, :]
        b[:, j + 1:] -= f * b[:, j, None]
    for j in range(n - 1, -1, -1):
        b[:, j] = (b[:, j] - np.einsum("bi,bi->b", A[:, j, j + 1:], b[:, j + 1:])) / A[:, j, j]
    rho = np.asarray(p, dtype=LD) - b @ model["Gr"].astype(LD).T
    return np.einsum("br,br->b", rho, rho)


def quadrature_moments(model, p, invvar, points=801):
    """(E[theta_q] (k,), E[theta_q theta_p] (k, k)) under the density e^(-invvar Phi / 2) on the box, by the trapezoid rule on
    `points` nodes per axis (k = 1 or 2), Phi in long double."""
    k, lo, hi = model["k"], model["lo"], model["hi"]
    assert k in (1, 2)
    axes = [np.linspace(LD(lo[q]), LD(hi[q]), points) for q in range(k)]
    w1 = np.ones(points, dtype=LD)
    w1[0] = w1[-1] = LD(0.5)
    if k == 1:
        grid, wq = axes[0][:, None], w1
        phi = potential(model, p, grid)
    else:
        phi = np.concatenate([potential(model, p, np.stack([np.full(points, a), axes[1]], axis=1)) for a in axes[0]])
        grid = np.stack([np.repeat(axes[0], points), np.tile(axes[1], points)], axis=1)
        wq = np.outer(w1, w1).ravel()
    dens = wq * np.exp(-LD(0.5) * LD(invvar) * (phi - phi.min()))
    Z = dens.sum()
    m1 = (dens[:, None] * grid).sum(axis=0) / Z
    m2 = np.einsum("g,gq,gp->qp", dens, grid, grid) / Z
    return m1.astype(np.float64), m2.astype(np.float64)


def noisy_query(model, theta_true, sigma, rng):
    """p = G_r c(theta*) + sigma N(0, 1) for the rows of theta_true (K, k)."""
    P = lt.coefficients(model, theta_true) @ model["Gr"].T
    return P + sigma * rng.standard_normal(P.shape)


def chain_moments(state, n, k):
    """Per chain (mean (B, k), second moment E[theta theta^T] (B, k, k)) from the rows: M2 / kept + mean mean^T."""
    from romhighcontrast_amd.inverse import mcmc_layout
    o = mcmc_layout(n, k)
    state = np.asarray(state, dtype=np.float64)
    mean = state[:, o["mean"]:o["mean"] + k]
    M2 = state[:, o["M2"]:o["M2"] + k * k].reshape(-1, k, k)
    return mean, M2 / state[:, o["kept"], None, None] + mean[:, :, None] * mean[:, None, :]


def moments_within(state, n, k, truth, sigmas=5.0):
    """The largest |average over chains - truth| / standard error (standard deviation over chains / sqrt(chains)) over the first
    and second moments, and whether every one is within `sigmas`."""
    mean, second = chain_moments(state, n, k)
    B = len(mean)
    worst = 0.0
    for est, want in ((mean, truth[0]), (second.reshape(B, -1), truth[1].reshape(-1))):
        se = est.std(axis=0, ddof=1) / np.sqrt(B)
        worst = max(worst, float((np.abs(est.mean(axis=0) - want) / se).max()))
    return worst, worst <= sigmas


def first_close_steps(model, P, invvar, theta0, L, seed, steps, burn, run=None, dtype=np.float64, chain0=0):
    """Per chain the first step whose decision margin |log u - l| in mcmc_host is below MARGIN, or `steps`: beyond it a
    legitimate flip may separate two arithmetics.  `run`: the McmcRun of the whole call, if at hand -- its smallest margins
    usually settle that no chain is cut; otherwise the chains are taken one step at a time."""
    from romhighcontrast_amd.inverse import mcmc_host
    args = (model["Ahat"], model["bhat"], model["Gr"], P, invvar)
    box = (model["lo"], model["hi"])
    if run is not None and (run.margin >= MARGIN).all():
        return np.full(len(run.state), steps)
    state = mcmc_host(*args, theta0, L, *box, seed, 0, burn, 1, chain0=chain0, dtype=dtype).state
    cut = np.full(len(state), steps)
    for i in range(steps):
        one = mcmc_host(*args, None, L, *box, seed, 1, burn, 1, chain0=chain0, step0=i, state=state, slots=0, dtype=dtype)
        state = one.state
        cut[(one.margin < MARGIN) & (cut == steps)] = i
    return cut


def compare_runs(ref, got_state, got_samples, cut, steps, burn, n, k, bound):
    """Holds a run (state rows, samples at thin 1) to the reference McmcRun `ref` of the same call: per chain the samples of the
    steps before cut[chain] within `bound`; for a chain that is not cut also kept, accepted, outside, not_spd equal and the mean,
    ls and Phi_min within `bound`.  Returns (largest observed / bound, number of chains cut)."""
    from romhighcontrast_amd.inverse import mcmc_layout
    o = mcmc_layout(n, k)
    rs, gs = np.asarray(ref.state, dtype=np.float64), np.asarray(got_state, dtype=np.float64)
    worst = 0.0
    for b in range(len(rs)):
        upto = max(0, int(cut[b]) - burn)
        if upto and ref.samples is not None:
            d = np.abs(np.asarray(ref.samples[b, :upto], dtype=np.float64) - got_samples[b, :upto]).max()
            assert d <= bound, f"chain {b}: samples differ by {d:.3g} > {bound:.3g} before step {int(cut[b])}"
            worst = max(worst, d / bound)
        if cut[b] < steps:
            continue
        for name in ("kept", "accepted", "outside", "not_spd"):
            assert rs[b, o[name]] == gs[b, o[name]], f"chain {b}: {name} {gs[b, o[name]]} against {rs[b, o[name]]}"
        for name, width in (("theta", k), ("mean", k), ("ls", 1), ("phi_min", 1)):
            d = np.abs(rs[b, o[name]:o[name] + width] - gs[b, o[name]:o[name] + width]).max()
            assert d <= bound, f"chain {b}: {name} differs by {d:.3g} > {bound:.3g}"
            worst = max(worst, d / bound)
    return worst, int((np.asarray(cut) < steps).sum())


def trajectory_case(n, k, r, K, t, seed=7):
    """The inputs of the trajectory tests at a shape: the model lt.synth(n, k, r, seed), theta* of lt.exact_queries, P with noise
    0.02 (default_rng(8)), invvar = 1 / 0.02^2, the starts theta* + 0.1 N(0, 1) (clipped by the call), L = 0.3 I."""
    model = lt.synth(n, k, r, seed)
    theta_true, _ = lt.exact_queries(model, K, seed)
    rng = np.random.default_rng(8)
    P = noisy_query(model, theta_true, 0.02, rng)
    theta0 = theta_true[:, None, :] + 0.1 * rng.standard_normal((K, t, k))
    return model, P, np.full(K, 1.0 / 0.02 ** 2), theta0, np.broadcast_to(0.3 * np.eye(k), (K, k, k)).copy()


def check_rows(model, P, t, state, steps_total, burn, thin=1, samples=None):
    """Raises AssertionError unless every state row (K t, row) is a consistent record of steps_total steps with `burn`:
    (1) kept = max(0, steps_total - burn), 0 <= accepted <= kept, outside + not_spd <= steps_total, all integers;
    (2) theta, theta_min and (kept > 0) the mean inside the box; Phi and Phi_min those of theta and theta_min to
        64 (r + n) eps (|p| + |G_r|_F |c|)^2;
    (3) M2 symmetric to 64 kept eps (hi - lo)^2 and positive semi-definite to the same;
    (4) with samples (K t, slots, k): every written sample inside the box and Phi_min <= its Phi (1 + 1e-12) (long double);
    (5) the mean of c finite."""
    from romhighcontrast_amd.inverse import mcmc_layout
    n, k, r, lo, hi = model["n"], model["k"], model["r"], model["lo"], model["hi"]
    o = mcmc_layout(n, k)
    state = np.asarray(state, dtype=np.float64)
    B = len(state)
    assert state.shape == (B, o["row"]) and np.isfinite(state).all(), "shape or non-finite entries"
    P = np.atleast_2d(np.asarray(P, dtype=np.float64))
    pq = P[np.repeat(np.arange(len(P)), t)]
    kept, acc, out, nspd = (state[:, o[name]] for name in ("kept", "accepted", "outside", "not_spd"))
    for v in (kept, acc, out, nspd):
        assert (v == np.round(v)).all() and (v >= 0).all()
    assert (kept == max(0, steps_total - burn)).all(), (kept, steps_total, burn)
    assert (acc <= kept).all() and (out + nspd <= steps_total).all()
    theta, thmin, mean = state[:, :k], state[:, o["theta_min"]:o["theta_min"] + k], state[:, o["mean"]:o["mean"] + k]
    for name, v in (("theta", theta), ("theta_min", thmin)) + ((("mean", mean),) if kept[0] > 0 else ()):
        assert ((v >= lo) & (v <= hi)).all(), f"{name} outside the box"
    scale = (np.linalg.norm(pq, axis=1) + np.linalg.norm(model["Gr"]) * np.linalg.norm(lt.coefficients(model, theta), axis=1)) ** 2
    tol = 64 * (r + n) * EPS * scale
    assert (np.abs(potential(model, pq, theta).astype(np.float64) - state[:, o["phi"]]) <= tol).all(), "Phi is not that of theta"
    assert (np.abs(potential(model, pq, thmin).astype(np.float64) - state[:, o["phi_min"]]) <= tol).all(), "Phi_min is not that of theta_min"
    M2 = state[:, o["M2"]:o["M2"] + k * k].reshape(B, k, k)
    rnd = 64 * np.maximum(kept, 1.0) * EPS * float(np.max(hi - lo)) ** 2
    assert (np.abs(M2 - M2.transpose(0, 2, 1)).max(axis=(1, 2)) <= rnd).all(), "M2 is not symmetric"
    ev = np.linalg.eigvalsh(0.5 * (M2 + M2.transpose(0, 2, 1)))
    assert (ev.min(axis=1) >= -rnd * k).all(), "M2 is not positive semi-definite"
    assert np.isfinite(state[:, o["mean_c"]:o["mean_c"] + n]).all()
    if samples is not None:
        samples = np.asarray(samples, dtype=np.float64)
        for b in range(B):
            got = samples[b][~np.isnan(samples[b][:, 0])]
            if len(got) == 0:
                continue
            assert ((got >= lo) & (got <= hi)).all(), f"chain {b}: a sample outside the box"
            ph = potential(model, pq[b], got).astype(np.float64)
            assert (state[b, o["phi_min"]] <= ph * (1 + 1e-12) + 1e-300).all(), f"chain {b}: Phi_min above a kept sample's Phi"
