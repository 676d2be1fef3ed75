"""Truth for the sensor state estimation on the polynomial manifold, rom_poly_sense (tests/test_poly_sense_host.py,
tests/test_gpu_poly_sense.py): synthetic models in reduced sensor coordinates, Legendre features and their derivatives in any
dtype by recurrences of their own, the host iteration on them, and a trajectory-free checker of a SenseResult that holds for any
max_iter.  A helper, not a test file.  TEST INFRASTRUCTURE."""
import itertools

import numpy as np

LD = np.longdouble
EPS = 2.0 ** -52
TINY = np.finfo(float).tiny


def powers(m, d):
    """The (P, m) exponent rows of PolynomialFeatures(d).powers_: graded, combinations with replacement in lexicographic order."""
    rows = []
    for deg in range(d + 1):
        for comb in itertools.combinations_with_replacement(range(m), deg):
            rows.append(np.bincount(np.array(comb, dtype=np.int64), minlength=m) if deg else np.zeros(m, dtype=np.int64))
    return np.array(rows, dtype=np.int64).reshape(-1, m)


def synth(m, d, r, seed):
    """G_r ~ N(0, 1) (r, P) with the columns of degree g scaled by 0.3^max(g - 1, 0); the box [-1.5, 1.5]."""
    rng = np.random.default_rng(seed)
    pw = powers(m, d)
    deg = pw.sum(axis=1)
    Gr = rng.standard_normal((r, len(pw))) * (0.3 ** np.maximum(deg - 1, 0))[None, :]
    return dict(m=m, d=d, r=r, powers=pw, Gr=Gr, lo=np.full(m, -1.5), hi=np.full(m, 1.5))


def twin_case(seed=11):
    """synth(4, 2, 8, seed) with the column of the term t_3 = the column of t_2 + 1e-7 N(0, 1): at t = 0 the Jacobian is minus
    the four linear columns, two of them 1e-7 apart.  Returns (model, t (1, 4) = 0)."""
    model = synth(4, 2, 8, seed)
    pw = model["powers"]
    lin = [int(np.flatnonzero((pw.sum(axis=1) == 1) & (pw[:, j] == 1))[0]) for j in range(4)]
    model["Gr"][:, lin[3]] = model["Gr"][:, lin[2]] + 1e-7 * np.random.default_rng(seed + 1).standard_normal(8)
    return model, np.zeros((1, 4))


def legendre(t, d, dtype=np.float64):
    """L_k(t), L'_k(t), k = 0 .. d, in `dtype`: (k + 1) L_{k+1} = (2k + 1) t L_k - k L_{k-1} and L'_{k+1} = (k + 1) L_k + t L'_k
    (not the derivative recurrence of the product).  Two arrays t.shape + (d + 1,)."""
    t = np.asarray(t, dtype=dtype)
    L = np.zeros(t.shape + (d + 1,), dtype=dtype)
    D = np.zeros(t.shape + (d + 1,), dtype=dtype)
    L[..., 0] = 1
    if d >= 1:
        L[..., 1] = t
        D[..., 1] = 1
    for k in range(1, d):
        L[..., k + 1] = ((2 * k + 1) * t * L[..., k] - k * L[..., k - 1]) / (k + 1)
        D[..., k + 1] = (k + 1) * L[..., k] + t * D[..., k]
    return L, D


def features(t, pw, dtype=np.float64, jacobian=True):
    """phi (B, P) and d phi / d t (B, P, m) (or None) at the rows of t (B, m), in `dtype`."""
    t = np.atleast_2d(np.asarray(t, dtype=dtype))
    m = pw.shape[1]
    d = max(int(pw.max()), 1)
    L, D = legendre(t, d, dtype)
    cols = np.arange(m)[None, :]
    sel, dsel = L[:, cols, pw], D[:, cols, pw]
    F = np.ones(sel.shape[:2], dtype=dtype)
    for j in range(m):
        F = F * sel[:, :, j]
    if not jacobian:
        return F, None
    dF = np.ones(sel.shape, dtype=dtype)
    for j in range(m):
        for i in range(m):
            dF[:, :, j] = dF[:, :, j] * (dsel[:, :, i] if i == j else sel[:, :, i])
    return F, dF


def exact_queries(model, K, seed):
    """(t* (K, m) ~ U(-0.9, 0.9), P (K, r) = G_r phi(t*)): data on the manifold."""
    rng = np.random.default_rng(seed)
    t = rng.uniform(-0.9, 0.9, size=(K, model["m"]))
    return t, features(t, model["powers"], jacobian=False)[0] @ model["Gr"].T


def host_sense(model, P, T0, **kw):
    from romhighcontrast_amd.nonlinear import sense_scores
    return sense_scores(model["Gr"], model["powers"], P, T0, model["lo"], model["hi"], **kw)


def default_aux(P):
    P = np.atleast_2d(P)
    return np.stack([np.zeros(len(P)), np.maximum(np.abs(P).max(axis=1), TINY)], axis=1)


def _misfit_ld(model, p, perp2, t):
    """(misfit in long double, the magnitude |p|_2 + | |G_r| phibar |_2 its rounding error is measured against): phibar_p =
    prod_j max(1, max_{i <= alpha_pj} |L_i(t_j)|) bounds every intermediate of the recurrences and products behind phi_p."""
    pw, Gr = model["powers"], model["Gr"]
    F, _ = features(t[None, :], pw, LD, jacobian=False)
    rho = p.astype(LD) - Gr.astype(LD) @ F[0]
    L, _ = legendre(t, max(int(pw.max()), 1))
    run = np.maximum.accumulate(np.maximum(np.abs(L), 1.0), axis=-1)        # (m, d + 1)
    phibar = run[np.arange(len(t))[None, :], pw].prod(axis=1)
    return np.sqrt((rho * rho).sum() + LD(perp2)), float(np.linalg.norm(p) + np.linalg.norm(np.abs(Gr) @ phibar))


def sigma_min_reference(model, t):
    """(sigma of the free columns' smallest singular value, sigma_max, the magnitude | |G_r| |d phi| |_F) from the long-double
    Jacobian J = -G_r d phi / d t at t (m,), its free columns only; 0 when nothing is free or r < the number of free columns."""
    free = model["lo"] < model["hi"]
    kf = int(free.sum())
    _, dF = features(t[None, :], model["powers"], LD)
    J = -(model["Gr"].astype(LD) @ dF[0])[:, free]
    mag = float(np.linalg.norm(np.abs(model["Gr"]) @ np.abs(dF[0].astype(np.float64))[:, free])) if kf else 0.0
    if kf == 0:
        return 0.0, 0.0, mag
    sv = np.linalg.svd(J.astype(np.float64), compute_uv=False)
    return (float(sv[-1]) if model["r"] >= kf else 0.0), float(sv[0]), mag


def check_state(model, P, aux, result, T0=None, misfit_tol=1e-3, max_iter=None):
    """Raises AssertionError unless every row of the SenseResult `result` is a consistent answer for the queries P (K, r) with aux
    (K, 2) = (perp2, scale) (None: 0 and max|p|).  Trajectory-free, sums in numpy.longdouble:
    (1) lo <= t <= hi exactly, so a pinned coordinate (lo_j == hi_j) has that value bit for bit;
    (2) misfit = sqrt(|p - G_r phi(t)|^2 + perp2) to 64 (r + P + d^2) eps (|p| + | |G_r| phibar |): r + P terms per sum, d^2
        for d recurrence steps behind each of at most d factors;
    (3) `converged` implies misfit <= misfit_tol scale, and a misfit <= min(1e-14, misfit_tol) scale implies `converged`; with
        max_iter = 0 the two are equivalent and iterations = 0;
    (4) sigma_min is the smallest singular value of the free columns of the long-double J = -G_r d phi / d t (0 when none is
        free) to 64 (P + d^2) eps max(sigma_max, | |G_r| |d phi| |_F);
    (5) with the starts T0 (K, t, m): start < t and misfit <= (misfit of the clipped chosen start) (1 + 1e-12); with max_iter = 0,
        t IS the clipped chosen start bit for bit and `start` is the argmin of the starts' misfits, the lowest index among those
        within the bound of (2) of the smallest.
    Returns the largest ratio observed / bound of (2) and (4)."""
    m, d, r, pw, Gr, lo, hi = model["m"], model["d"], model["r"], model["powers"], model["Gr"], model["lo"], model["hi"]
    P = np.atleast_2d(np.asarray(P, dtype=np.float64))
    K = len(P)
    aux = default_aux(P) if aux is None else np.asarray(aux, dtype=np.float64)
    assert result.t.shape == (K, m), result.t.shape
    for name in ("misfit", "converged", "iterations", "sigma_min", "start"):
        assert getattr(result, name).shape == (K,), (name, getattr(result, name).shape)
    nP = len(pw)
    worst = 0.0
    for q in range(K):
        t, misfit = result.t[q], float(result.misfit[q])
        perp2, scale = float(aux[q, 0]), float(aux[q, 1])
        assert np.isfinite(t).all() and np.isfinite(misfit) and np.isfinite(result.sigma_min[q]), f"query {q}: non-finite result"
        assert ((t >= lo) & (t <= hi)).all(), f"query {q}: t {t} outside the box [{lo}, {hi}]"
        want, mag = _misfit_ld(model, P[q], perp2, t)
        bound = 64 * (r + nP + d * d) * EPS * mag
        assert abs(LD(misfit) - want) <= bound, f"query {q}: misfit {misfit!r} off sqrt(|p - G phi|^2 + perp2) = {float(want)!r} by more than {bound:.3g}"
        worst = max(worst, float(abs(LD(misfit) - want) / bound)) if bound > 0 else worst
        ref, smax, jmag = sigma_min_reference(model, t)
        bound = 64 * (nP + d * d) * EPS * max(smax, jmag)
        err = abs(float(result.sigma_min[q]) - ref)
        assert err <= bound, f"query {q}: sigma_min {float(result.sigma_min[q])!r} off {ref!r} by {err:.3g} > {bound:.3g}"
        worst = max(worst, err / bound) if bound > 0 else worst
        start, its = int(result.start[q]), int(result.iterations[q])
        assert its >= 0 and start >= 0
        if T0 is not None:
            t0 = np.clip(np.asarray(T0, dtype=np.float64).reshape(K, -1, m)[q], lo, hi)
            assert start < len(t0), f"query {q}: start {start} of {len(t0)}"
            m0 = [_misfit_ld(model, P[q], perp2, s) for s in t0]
            assert misfit <= float(m0[start][0]) * (1 + 1e-12), f"query {q}: misfit {misfit!r} above its start's {float(m0[start][0])!r}"
            if max_iter == 0:
                assert np.array_equal(t.view(np.uint64), t0[start].view(np.uint64)), f"query {q}: t is not its clipped start {start}"
                vals = np.array([float(v[0]) for v in m0])
                slack = 64 * (r + nP + d * d) * EPS * max(v[1] for v in m0)
                near = np.flatnonzero(vals <= vals.min() + 2 * slack)
                assert start in near, f"query {q}: wrong start {start}, the smallest misfit is at {near}"
        conv = bool(result.converged[q])
        if conv:
            assert misfit <= misfit_tol * scale, f"query {q}: converged with misfit {misfit!r} > {misfit_tol} * {scale!r}"
        if misfit <= min(1e-14, misfit_tol) * scale * (1 - 1e-9):
            assert conv, f"query {q}: misfit {misfit!r} at rounding level of {scale!r} but not converged"
        if max_iter == 0:
            assert its == 0, f"query {q}: {its} iterations with max_iter = 0"
            if misfit > 1e-14 * scale * (1 + 1e-9):
                assert not conv, f"query {q}: converged without an iteration at misfit {misfit!r}"
    return worst
