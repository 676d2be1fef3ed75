"""The distance truncation of the compressed extension (basis of the reduced unknowns rotated to echelon
form in the sine modes, k_extend128 skipping the K segments that have died out at a tile's distance from a side) on the GPU.

Every case solves a batch of M = 130 systems (the last group of k_solve1 / k_extend128 holds two) twice, each on a fresh Fem:
with the truncation (default) and with ROMHC_NO_EXT_TRUNC (the plan and rows of the library before the truncation).  The D
distinct parameter vectors follow the pattern of the C4 workload of bench.py: all ones, single blocks at 1e8, all 1e8, and
10^U(0, 8); system m carries a_{idx[m]} (tests/sweep_truth.py: idx_pattern), so rows of equal idx must be equal bit for bit
wherever they sit, and one row per d is held against a reference:
  * 2x2 / N = 40 and 3x3 / N = 24: the SuperLU oracle, relative H^1_0 <= SNAP_TOL;
  * 2x2 / N = 64, 3x3 / N = 64, 2x2 / N = 128, 2x2 / N = 171 (flat tiles inside one mesh row), 2x2 / N = 250 (two column tiles
    per mesh row, the second ragged): the 80-bit truth of tests/referee.py, relative H^1_0 in long double <= SNAP_TOL.
The two builds must agree row by row to SNAP_TOL.  Both distances are rounding-level numbers (a wrong cut shows as orders of
magnitude); they are printed, and written as JSON lines to the file ROMHC_EXT_TRUNC_JSON names, if set (profiles/ext_trunc.json
was recorded that way)."""
import json
import os

import numpy as np
import pytest

import sweep_truth as st
from conftest import observed
from oracle import rom_oracle as ro

pytestmark = pytest.mark.gpu

M = 130
SNAP_TOL = st.SNAP_TOL
CASES = [((2, 2), 40, "oracle"), ((3, 3), 24, "oracle"), ((2, 2), 64, "truth"), ((3, 3), 64, "truth"), ((2, 2), 128, "truth"),
         ((2, 2), 171, "truth"), ((2, 2), 250, "truth")]


def parameters(blocks, N):
    """(D, kblk): ones | first block at 1e8 | last block at 1e8 | all 1e8 | two rows 10^U(0, 8)."""
    k = blocks[0] * blocks[1]
    a = np.ones((6, k))
    a[1, 0] = 1e8
    a[2, k - 1] = 1e8
    a[3] = 1e8
    a[4:] = 10.0 ** np.random.default_rng([0xE7, k, N]).uniform(0, 8, size=(2, k))
    return a


def sweep(ctx, blocks, N, ab, monkeypatch, off):
    from romhighcontrast_amd import _ffi
    if off:
        monkeypatch.setenv("ROMHC_NO_EXT_TRUNC", "1")
    else:
        monkeypatch.delenv("ROMHC_NO_EXT_TRUNC", raising=False)
    fem = _ffi.Fem(ctx, blocks[0], blocks[1], N)
    U = ctx.alloc(M * fem.dim)
    fem.solve_batch(ab, M, U)
    rows = U.download(shape=(M, fem.dim))
    monkeypatch.delenv("ROMHC_NO_EXT_TRUNC", raising=False)
    return rows


@pytest.mark.parametrize("blocks,N,ref", CASES, ids=[f"{b[0]}x{b[1]}-N{n}-{r}" for b, n, r in CASES])
def test_truncated_extension_against_reference(blocks, N, ref, monkeypatch):
    from romhighcontrast_amd import _ffi
    ctx = _ffi.get_context()
    a = parameters(blocks, N)
    D = len(a)
    idx = st.idx_pattern(M, D)
    assert st.check_idx(idx, M, D)
    ab = ctx.upload(np.ascontiguousarray(a[idx]))
    rows = {"trunc": sweep(ctx, blocks, N, ab, monkeypatch, False), "no_ext_trunc": sweep(ctx, blocks, N, ab, monkeypatch, True)}
    first = np.array([int(np.flatnonzero(idx == d)[0]) for d in range(D)])
    if ref == "oracle":
        g = ro.Geometry(blocks, N)
        want = ro.generate_solutions(g, a.reshape((D,) + blocks))
        dist = {name: [float(x) for x in ro.H10norm(g, r[first] - want) / ro.H10norm(g, want)] for name, r in rows.items()}
    else:
        out = [st.rf.referee(blocks, N, ad.reshape(blocks), verbose=False) for ad in a]
        g = out[0][0]
        dist = {name: [st.rel_h10_ld(g, r[first[d]], out[d][1]) for d in range(D)] for name, r in rows.items()}
    between = ro.H10norm(g, rows["trunc"] - rows["no_ext_trunc"]) / ro.H10norm(g, rows["no_ext_trunc"])
    rec = dict(test="test_gpu_ext_trunc", blocks=list(blocks), N=N, M=M, reference=ref, tol=SNAP_TOL,
               to_reference={k: max(v) for k, v in dist.items()}, to_reference_rows=dist, between_builds=float(between.max()))
    print(json.dumps(rec))
    if os.environ.get("ROMHC_EXT_TRUNC_JSON"):
        with open(os.environ["ROMHC_EXT_TRUNC_JSON"], "a") as fh:
            fh.write(json.dumps(rec) + "\n")
    name = f"ext_trunc {blocks[0]}x{blocks[1]}/N={N}"
    for build, r in rows.items():
        assert np.isfinite(r).all(), build
        for m in range(M):  # a system's row does not depend on where it sits in the batch
            assert np.array_equal(r[m], r[first[idx[m]]]), (build, m)
        observed(f"{name} {build} vs {ref}", dist[build], SNAP_TOL)
    observed(f"{name} trunc vs no_ext_trunc", between, SNAP_TOL)
