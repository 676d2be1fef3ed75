"""Host side of the library-based parameter estimation: the checker of tests/nearest_truth.py tells right answers from wrong
ones, and polish_parameters (pure NumPy) recovers parameters on a reduced model built with the oracle.

The polish cases: geometry (2, 2), N = 8, n = 10 snapshots as the basis, 16 random sensors, a 12^4 grid library in log a.
ROM-exact data over 4 decades: 64 queries off the grid, one start (the library entry of smallest misfit); every query flagged
`converged` must have max |log10 a_est - log10 a*| <= 1e-8 and at most 10 % may be unflagged.  Noise 1e-3 max|y| on truth
snapshots at contrast 1e2 and 1e4: the median error of library + polish must be below EstimatorInv's on the same data (the
NumPy prototype of the method measured it 5-7 x below)."""
import numpy as np
import pytest

import nearest_truth as nt


def test_checker_accepts_brute_force_and_rejects_wrong_answers():
    for kind, M, K, r, t in (("uniform", 300, 7, 5, 4), ("ulp", 200, 5, 3, 6), ("self", 64, 9, 2, 1), ("offset", 97, 3, 8, 8)):
        Q, P = nt.build_case(kind, M, K, r, seed=2)
        idx, d2 = nt.brute_force(P, Q, t)
        nt.check_neighbours(P, Q, idx, d2, t)
    Q, P = nt.build_case("uniform", 300, 7, 5, seed=2)
    idx, d2 = nt.brute_force(P, Q, 4)
    far = nt.brute_force(P, Q, 40)
    swapped_i, swapped_d = idx.copy(), d2.copy()
    swapped_i[3, 3], swapped_d[3, 3] = far[0][3, 39], far[1][3, 39]          # a far row in place of the fourth neighbour
    with pytest.raises(AssertionError, match="left one"):
        nt.check_neighbours(P, Q, swapped_i, swapped_d, 4)
    with pytest.raises(AssertionError, match="not sorted"):
        nt.check_neighbours(P, Q, idx[:, ::-1], d2[:, ::-1], 4)
    bent = d2.copy()
    bent[2, 1] *= 1 + 64 * nt.EPS
    with pytest.raises(AssertionError, match="off the exact"):
        nt.check_neighbours(P, Q, idx, bent, 4)
    twice = idx.copy()
    twice[0, 1] = twice[0, 0]
    with pytest.raises(AssertionError):
        nt.check_neighbours(P, Q, twice, d2, 4)


def _library_starts(rom, lib, Y, t):
    """The t library entries of smallest misfit per row of Y, by brute force on the host: (idx (K, t), log a of them)."""
    pred = nt.rom_coefficients(rom["Ahat"], rom["bhat"], lib) @ rom["E"]
    idx, _ = nt.brute_force(Y, pred, t)
    return idx, np.log(lib[idx])


def test_polish_recovers_rom_exact_parameters():
    from romhighcontrast_amd.inverse import polish_parameters
    rom = nt.oracle_rom(decades=4.0)
    lib = nt.grid_library(rom["k"], 12, 4.0)
    a_true = 10.0 ** np.random.default_rng(1).uniform(0.0, 4.0, size=(64, rom["k"]))
    Y = nt.rom_coefficients(rom["Ahat"], rom["bhat"], a_true) @ rom["E"]
    _, starts = _library_starts(rom, lib, Y, 1)
    res = polish_parameters(rom["Ahat"], rom["bhat"], rom["E"], Y, starts, 0.0, np.log(1e4))
    err = np.abs(res.theta - np.log(a_true)).max(axis=1) / np.log(10.0)
    print(f"flagged {int(res.converged.sum())} of 64; max error of the flagged {err[res.converged].max():.3g}; "
          f"errors of the unflagged {np.sort(err[~res.converged])}; misfit / max|y| of the unflagged "
          f"{res.misfit[~res.converged] / np.abs(Y[~res.converged]).max(axis=1)}; iterations up to {res.iterations.max()}; "
          f"sigma_min {res.sigma_min.min():.3g} .. {res.sigma_min.max():.3g}")
    assert res.theta.shape == (64, rom["k"]) and res.coefficients.shape == (64, 10) and res.sigma_min.shape == (64,)
    assert (err[res.converged] <= 1e-8).all()
    assert (~res.converged).sum() <= 6
    assert (res.sigma_min > 0).all()


@pytest.mark.parametrize("decades", [2.0, 4.0])
def test_library_and_polish_beat_estimator_inv_under_noise(decades):
    from oracle import rom_oracle as ro
    from romhighcontrast_amd.inverse import polish_parameters
    from romhighcontrast_amd.lib.Estimators import EstimatorInv
    rom = nt.oracle_rom(decades=decades)
    g, k = rom["g"], rom["k"]
    lib = nt.grid_library(k, 12, decades)
    rng = np.random.default_rng(2)
    a_true = 10.0 ** rng.uniform(0.0, decades, size=(40,) + rom["blocks"])
    Y = ro.evaluate_solutions(g, rom["points"], ro.generate_solutions(g, a_true, "lsqsparse"))
    Y = Y + 1e-3 * np.abs(Y).max(axis=1, keepdims=True) * rng.standard_normal(Y.shape)
    _, starts = _library_starts(rom, lib, Y, 4)
    res = polish_parameters(rom["Ahat"], rom["bhat"], rom["E"], Y, starts, 0.0, np.log(10.0 ** decades))
    err = np.abs(res.theta - np.log(a_true.reshape(40, k))).max(axis=1) / np.log(10.0)
    c, *_ = np.linalg.lstsq(rom["E_basis"].T, Y.T, rcond=-1)
    a_inv = EstimatorInv(rom["a_basis"]).estimate_parameter(c).reshape(40, k)
    with np.errstate(invalid="ignore", divide="ignore"):
        err_inv = np.abs(np.log10(a_inv) - np.log10(a_true.reshape(40, k)))
    err_inv = np.where(np.isfinite(err_inv), err_inv, np.inf).max(axis=1)   # (a negative estimate has no logarithm)
    print(f"contrast 1e{decades:g}: median error library + polish {np.median(err):.3g}, EstimatorInv {np.median(err_inv):.3g}")
    assert np.median(err) < np.median(err_inv)
