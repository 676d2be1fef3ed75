"""inverse.local_select_host, the NumPy specification of rom_local_select, on the CPU: every case of tests/local_select_truth.py
through its long-double checker (the Karush-Kuhn-Tucker conditions of both solves, S recomputed from the residual table
itself, the selection rule), the statuses of refused and of open solves, and S against an independent minimisation of
||R z(a, c)||_2 over the box.  The stand-alone program tests/c_abi/local_select_host_check.cpp runs the host side of
rom_local_select_layout and the packing of the boxes under AddressSanitizer and UBSan.  No GPU."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import local_select_truth as lt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", list(lt.SHAPES))
def test_specification_against_the_checker(name):
    cs, res = lt.case(name), lt.spec(name)
    assert res.labels.shape == (cs.K,) and res.c_all.shape == (cs.K, cs.kc, cs.n) and res.a_all.shape == (cs.K, cs.kc, cs.k)
    assert (res.status == 0).all() and (res.labels >= 0).all()
    count, worst = lt.check_result(cs, res)
    assert count == cs.K * cs.kc
    gap = lt.label_gap(res.surrogate_all, res.status)
    print(f"{name}: worst ratios to the checker's bounds {worst}; smallest gap between the two best S {gap.min():.3g}")
    assert (gap >= lt.GAP).all()
    assert (res.passes[:, :, 0] <= 5 * cs.n + 10).all() and (res.passes[:, :, 1] <= 5 * cs.k + 10).all()
    if name != "one":   # both sides of the box of a are active somewhere, and something is free
        assert (res.a_all == cs.a_lo[None]).any() and (res.a_all == cs.a_hi[None]).any()
        assert ((res.a_all > cs.a_lo[None]) & (res.a_all < cs.a_hi[None])).any()


def test_checker_refuses_bent_answers():
    cs, res = lt.case("small"), lt.spec("small")
    P = cs.P.reshape(cs.K, cs.kc, cs.r)
    i, j = 1, 2
    args = (cs.RT[j], cs.GR[j], P[i, j], cs.c_lo[j], cs.c_hi[j], cs.a_lo[j], cs.a_hi[j])
    c, a, S, mis = res.c_all[i, j], res.a_all[i, j], res.surrogate_all[i, j], res.misfit_all[i, j]
    lt.check_system(*args, c, a, S, mis)
    with pytest.raises(AssertionError):
        lt.check_system(*args, c, a, S * (1 + 1e-9), mis)
    free = np.flatnonzero((a > cs.a_lo[j]) & (a < cs.a_hi[j]))
    bent = a.copy()
    bent[free[0] if free.size else 0] += 1e-7
    with pytest.raises(AssertionError):
        lt.check_system(*args, c, bent, S, mis)


@pytest.mark.parametrize("n,k,rank", [(1, 1, 3), (3, 1, 6), (3, 2, 9), (5, 4, 24)])
def test_surrogate_is_the_minimum_of_the_residual_norm(n, k, rank):
    """Steps 2 - 3 on a tiny table: S equals, to 1e-12 relative, min over the box of ||R z(a, c)||_2 found independently --
    scipy's lsq_linear on the matrix of the map a -> R z(a, c) built column by column from z itself, and for k = 1 a dense grid
    refined around its minimum."""
    from scipy.optimize import lsq_linear
    from romhighcontrast_amd.inverse import bvls_host, local_select_matrix
    R, c, lo, hi = lt.tiny_table(n, k, rank)

    def z(a):
        return np.concatenate([[1.0], -(c[:, None] * np.asarray(a)[None, :]).reshape(-1)])

    B = local_select_matrix(R, c, k)
    res = bvls_host(B, R[:, 0][None, :], lo, hi)
    S, a = res.misfit[0], res.c[0]
    assert res.converged[0]
    np.testing.assert_allclose(S, np.linalg.norm(R @ z(a)), rtol=1e-13)
    # a -> R z(a) = R z(0) + sum_q a_q (R z(e_q) - R z(0)): the matrix from z itself, not from local_select_matrix
    base = R @ z(np.zeros(k))
    M = np.stack([R @ z(np.eye(k)[q]) - base for q in range(k)], axis=1)
    ref = lsq_linear(M, -base, bounds=(lo, hi), method="bvls", tol=1e-15)
    S_ref = np.linalg.norm(M @ ref.x + base)
    print(f"(n, k, rank) = {(n, k, rank)}: S {S!r}, lsq_linear {S_ref!r}, a {a}, bound states {res.bound[0]}")
    assert abs(S - S_ref) <= 1e-12 * S_ref
    assert S <= S_ref * (1 + 1e-14) or np.allclose(a, ref.x, atol=1e-9)
    if k == 1:
        a_lo, a_hi = lo[0], hi[0]
        for _ in range(6):   # 2001 points, then the two cells around the best one again
            grid = np.linspace(a_lo, a_hi, 2001)
            val = np.array([np.linalg.norm(R @ z([t])) for t in grid])
            b = int(np.argmin(val))
            a_lo, a_hi = grid[max(b - 1, 0)], grid[min(b + 1, 2000)]
        assert abs(S - val.min()) <= 1e-12 * S


def test_refused_and_open_solves_are_statuses():
    from romhighcontrast_amd.inverse import LS_BAD_PARAM, LS_BAD_STATE, LS_OPEN_PARAM, LS_OPEN_STATE, local_select_host
    cs, ref = lt.case("small"), lt.spec("small")
    P = cs.P.copy()
    P[1, cs.r + 1] = np.nan          # vector 1, cluster 1
    P[3] = np.inf                    # vector 3, every cluster
    res = local_select_host(cs.RT, cs.GR, P, cs.c_lo, cs.c_hi, cs.a_lo, cs.a_hi)
    assert res.status[1, 1] == LS_BAD_STATE and (res.status[3] == LS_BAD_STATE).all() and (res.status != 0).sum() == 4
    assert res.labels[3] == -1 and np.isnan(res.coefficients[3]).all() and np.isnan(res.surrogate[3]) and res.labels[1] != 1
    keep = [0, 2, 4]
    assert np.array_equal(res.c_all[keep], ref.c_all[keep]) and np.array_equal(res.surrogate_all[keep], ref.surrogate_all[keep])
    assert np.array_equal(res.labels[keep], ref.labels[keep])
    # a residual table whose B has a zero column: the parameter solve is refused, the state is kept
    RT = cs.RT.copy()
    RT[2, :, 2::cs.k] = 0.0          # block q = 1 of cluster 2
    res = local_select_host(RT, cs.GR, cs.P, cs.c_lo, cs.c_hi, cs.a_lo, cs.a_hi)
    assert (res.status[:, 2] == LS_BAD_PARAM).all() and np.isnan(res.surrogate_all[:, 2]).all() and (res.labels != 2).all()
    assert np.array_equal(res.c_all[:, 2], ref.c_all[:, 2])
    # max_iter = 0: the clipped starts, both solves open, nothing to select
    res = local_select_host(*cs.args(), max_iter=0)
    assert (res.status == (LS_OPEN_STATE | LS_OPEN_PARAM)).all() and (res.labels == -1).all() and (res.passes == 0).all()
    with pytest.raises(ValueError, match="lo <= hi"):
        local_select_host(cs.RT, cs.GR, cs.P, cs.c_hi, cs.c_lo, cs.a_lo, cs.a_hi)


def test_selection_rule():
    """The smallest (S, index) among the entries of status 0 whose S is a number: ties to the lower index, a NaN never wins,
    nothing eligible gives -1."""
    from romhighcontrast_amd.inverse import local_select_labels
    S = np.array([[3.0, 1.0, 1.0], [np.nan, 2.0, 1.0], [0.5, 2.0, 1.0], [np.nan, 1.0, 2.0], [np.nan, np.nan, 5.0], [1.0, 2.0, 3.0]])
    status = np.array([[0, 0, 0], [0, 0, 4], [1, 0, 0], [0, 8, 2], [0, 0, 1], [0, 0, 0]])
    assert local_select_labels(S, status).tolist() == [1, 1, 2, -1, -1, 0]


def test_observe_refuses_a_centred_basis():
    from romhighcontrast_amd.local import LocalReducedBasis
    lrb = LocalReducedBasis(2, inner_product="l2", center=True)
    lrb.kmeans = object()   # (as after build)
    with pytest.raises(ValueError, match="center=True"):
        lrb.observe(None, np.zeros((3, 2)))


def test_zero_rows_added_to_the_table_change_nothing():
    from romhighcontrast_amd.inverse import local_select_host
    cs, ref = lt.case("small"), lt.spec("small")
    RT = np.concatenate([cs.RT, np.zeros((cs.kc, 4, cs.RT.shape[2]))], axis=1)
    res = local_select_host(RT, cs.GR, cs.P, cs.c_lo, cs.c_hi, cs.a_lo, cs.a_hi)
    assert np.array_equal(res.labels, ref.labels) and np.array_equal(res.passes, ref.passes)
    np.testing.assert_allclose(res.surrogate_all, ref.surrogate_all, rtol=1e-14)
    np.testing.assert_allclose(res.a_all, ref.a_all, rtol=0, atol=1e-13)


# ---- the host side of the entry under sanitizers ------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def output(tmp_path_factory):
    gxx = shutil.which("g++")
    assert gxx, "g++ is part of the image"
    exe = str(tmp_path_factory.mktemp("local_select_host") / "local_select_host_check")
    csrc = os.path.join(ROOT, "romhighcontrast_amd", "csrc")
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-I", csrc, os.path.join(ROOT, "tests", "c_abi", "local_select_host_check.cpp"), "-o", exe]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0, r.stdout.decode()
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    return r.returncode, r.stdout.decode(), r.stderr.decode()


def test_layout_and_box_packing_are_clean_under_sanitizers(output):
    code, out, err = output
    assert code == 0, out + err
    assert err == "", err                      # no sanitizer report
    assert out.splitlines()[-1] == "OK" and "FAILED" not in out, out


def test_layout_agrees_with_the_library(output):
    """The LAYOUT lines of the stand-alone program (LDS bytes and largest rank at the two shapes the entry must reach) against
    rom_local_select_layout of the built library."""
    from romhighcontrast_amd._ffi import local_select_layout
    lines = [ln.split() for ln in output[1].splitlines() if ln.startswith("LAYOUT ")]
    assert len(lines) == 2
    for ln in lines:
        n, k, rank, r, lds, top = map(int, ln[1:7])
        lay = local_select_layout(n, k, rank, r)
        assert (lay["lds_bytes"], lay["rank_max"], lay["row_doubles"]) == (lds, top, n + k + 5) and lds <= 64 * 1024 and top >= rank
