"""Truth for the device polish rom_lm_polish (tests/test_lm_polish_host.py, tests/test_gpu_lm_polish.py): synthetic reduced
models in reduced sensor coordinates, the host polish on them, and a trajectory-free checker of a polish result that holds for
any max_iter.  A helper, not a test file.  TEST INFRASTRUCTURE."""
import math

import numpy as np

LD = np.longdouble
EPS = 2.0 ** -52
TINY = np.finfo(float).tiny


def synth(n, k, r, seed):
    """A reduced model: Ahat_q = B_q B_q^T / w, B_q ~ N(0, 1) (n, w), w = max(2, ceil(2 n / k)) (the sum of the k is positive
    definite); bhat ~ N(0, 1); G_r ~ N(0, 1) / sqrt(n) (r, n); the box [0, log 100]."""
    rng = np.random.default_rng(seed)
    w = max(2, math.ceil(2 * n / k))
    B = rng.standard_normal((k, n, w))
    Ahat = np.einsum("qiw,qjw->qij", B, B) / w
    bhat = rng.standard_normal(n)
    Gr = rng.standard_normal((r, n)) / np.sqrt(n)
    return dict(n=n, k=k, r=r, Ahat=Ahat, bhat=bhat, Gr=Gr, lo=np.zeros(k), hi=np.full(k, np.log(100.0)))


def twin_case(seed=11):
    """synth(33, 9, 20, seed) with Ahat_8 = Ahat_7 + 1e-7 (a fresh B B^T / 8) and theta_8 = theta_7: the columns 7 and 8 of the
    Jacobian differ by 1e-7 relative, sigma_min ~ 8e-9 beside sigma_max ~ 0.06.  Returns (model, theta (1, 9))."""
    model = synth(33, 9, 20, seed)
    rng = np.random.default_rng(seed + 1)
    B = rng.standard_normal((33, 8))
    model["Ahat"][8] = model["Ahat"][7] + 1e-7 * (B @ B.T / 8.0)
    theta = rng.uniform(0.2, np.log(100.0) - 0.2, size=(1, 9))
    theta[0, 8] = theta[0, 7]
    return model, theta


def coefficients(model, theta):
    """c(theta) (B, n) for the rows of theta (B, k)."""
    A = np.einsum("bq,qij->bij", np.exp(theta), model["Ahat"])
    return np.linalg.solve(A, np.broadcast_to(model["bhat"], (len(theta), model["n"]))[..., None])[..., 0]


def exact_queries(model, K, seed):
    """(theta* (K, k) ~ U(0.2, log 100 - 0.2), P (K, r) = G_r c(theta*)): ROM-exact data."""
    rng = np.random.default_rng(seed)
    theta = rng.uniform(0.2, np.log(100.0) - 0.2, size=(K, model["k"]))
    return theta, coefficients(model, theta) @ model["Gr"].T


def host_polish(model, P, theta0, **kw):
    """polish_parameters on the reduced coordinates: E = G_r^T, Y = P."""
    from romhighcontrast_amd.inverse import polish_parameters
    return polish_parameters(model["Ahat"], model["bhat"], model["Gr"].T, P, theta0, model["lo"], model["hi"], **kw)


def jacobian(model, theta):
    """J_r = G_r X (r, k) at one theta (k,), X = A^-1 [e^theta_q Ahat_q c]_q, by NumPy (LU)."""
    ea = np.exp(theta)
    A = np.einsum("q,qij->ij", ea, model["Ahat"])
    c = np.linalg.solve(A, model["bhat"])
    V = np.einsum("qij,j->iq", model["Ahat"], c) * ea[None, :]
    return model["Gr"] @ np.linalg.solve(A, V), A


def sigma_min_reference(J):
    """The k-th singular value of J (r, k): 0 when r < k."""
    r, k = J.shape
    return float(np.linalg.svd(J, compute_uv=False)[-1]) if r >= k else 0.0


def default_aux(P):
    P = np.atleast_2d(P)
    return np.stack([np.zeros(len(P)), np.maximum(np.abs(P).max(axis=1), TINY)], axis=1)


def check_state(model, P, aux, result, theta0=None, misfit_tol=1e-3, max_iter=None):
    """Raises AssertionError unless every row of the PolishResult `result` is a consistent answer for the queries P (K, r) with
    aux (K, 2) = (perp2, scale) (None: 0 and max|p|).  Trajectory-free: (1) lo <= theta <= hi exactly; (2) c solves A(theta) c =
    bhat to 64 n eps |A|_inf |c|_inf; (3) misfit = sqrt(|p - G_r c|^2 + perp2) to 64 (r + n) eps (|p| + |G_r|_F |c|); (4)
    sigma_min is that of J_r at theta by NumPy to 64 eps cond_2(A(theta)) sigma_max(J_r); (5) with the starts theta0 (K, t, k):
    misfit <= (misfit of the clipped chosen start) (1 + 1e-12); (6) `converged` implies misfit <= misfit_tol scale, and a misfit
    <= min(1e-14, misfit_tol) scale implies `converged`; with max_iter = 0 the two are equivalent and iterations = 0.  Sums in
    numpy.longdouble.  Returns the largest ratio observed / bound of (2), (3), (4)."""
    n, k, r = model["n"], model["k"], model["r"]
    Ahat, bhat, Gr, lo, hi = model["Ahat"], model["bhat"], model["Gr"], model["lo"], model["hi"]
    P = np.atleast_2d(np.asarray(P, dtype=np.float64))
    K = len(P)
    aux = default_aux(P) if aux is None else np.asarray(aux, dtype=np.float64)
    assert result.theta.shape == (K, k) and result.coefficients.shape == (K, n), (result.theta.shape, result.coefficients.shape)
    for name in ("misfit", "converged", "iterations", "sigma_min", "start"):
        assert getattr(result, name).shape == (K,), (name, getattr(result, name).shape)
    worst = 0.0
    for q in range(K):
        th, c, misfit = result.theta[q], result.coefficients[q], float(result.misfit[q])
        perp2, scale = float(aux[q, 0]), float(aux[q, 1])
        assert np.isfinite(th).all() and np.isfinite(c).all() and np.isfinite(misfit), f"query {q}: non-finite result"
        assert ((th >= lo) & (th <= hi)).all(), f"query {q}: theta {th} outside the box [{lo}, {hi}]"
        A = np.einsum("q,qij->ij", np.exp(th).astype(LD), Ahat.astype(LD))
        res = np.abs(A @ c.astype(LD) - bhat.astype(LD)).max()
        bound = 64 * n * EPS * np.abs(A).sum(axis=1).max() * np.abs(c).max()
        assert res <= bound, f"query {q}: |A c - bhat|_inf = {float(res):.3g} > {float(bound):.3g}: c does not solve A(theta) c = bhat"
        worst = max(worst, float(res / bound))
        rho = P[q].astype(LD) - Gr.astype(LD) @ c.astype(LD)
        want = np.sqrt((rho * rho).sum() + LD(perp2))
        bound = 64 * (r + n) * EPS * (np.linalg.norm(P[q]) + np.linalg.norm(Gr) * np.linalg.norm(c))
        assert abs(LD(misfit) - want) <= bound, f"query {q}: misfit {misfit!r} off sqrt(|p - G c|^2 + perp2) = {float(want)!r} by more than {bound:.3g}"
        worst = max(worst, float(abs(LD(misfit) - want) / bound)) if bound > 0 else worst
        J, A64 = jacobian(model, th)
        sv = np.linalg.svd(J, compute_uv=False)
        bound = 64 * EPS * np.linalg.cond(A64) * sv[0]
        err = abs(float(result.sigma_min[q]) - sigma_min_reference(J))
        assert err <= bound, f"query {q}: sigma_min {float(result.sigma_min[q])!r} off {sigma_min_reference(J)!r} by {err:.3g} > {bound:.3g}"
        worst = max(worst, err / bound) if bound > 0 else worst
        start, its = int(result.start[q]), int(result.iterations[q])
        assert its >= 0 and start >= 0
        if theta0 is not None:
            t0 = np.asarray(theta0, dtype=np.float64).reshape(K, -1, k)
            assert start < t0.shape[1], f"query {q}: start {start} of {t0.shape[1]}"
            c0 = coefficients(model, np.clip(t0[q, start], lo, hi)[None, :])[0]
            rho0 = P[q].astype(LD) - Gr.astype(LD) @ c0.astype(LD)
            m0 = float(np.sqrt((rho0 * rho0).sum() + LD(perp2)))
            assert misfit <= m0 * (1 + 1e-12), f"query {q}: misfit {misfit!r} above its start's {m0!r}"
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
