"""The per-wave K-segment skipping of k_extend128 (every wave multiplies only the halves of its tile's walk
that its own 32 vertices need, and nobody fetches or multiplies the zero half of an odd walk) on the GPU.

Every case solves a batch of M = 130 systems (the last system group holds two) on fresh Fems: with the skipping (default), with
ROMHC_NO_EXT_WAVE_SKIP (every wave follows its tile's walk, zero half included: the kernel before the skipping), and both again
with ROMHC_NO_EXT_TRUNC (no thresholds: nothing to skip but the zero half).  The parameters follow tests/test_gpu_ext_trunc.py.
  * 2x2 / N = 128: row tiles, every block with one side its mesh rows run away from;
  * 3x3 / N = 64: FLAT tiles, the centre block with four sides;
  * 2x3 / N = 128;
  * 2x2 / N = 171: FLAT tiles that lie inside one mesh row (n1 = 170), whole tiles skipping segments of the sides their row ends at;
  * 2x2 / N = 250: row tiles, two column tiles per mesh row, the second of 121 vertices (its fourth wave column partly filled).
The skipped products are exact zeros added to sums that start at +0, so the rows with and without the skipping must be equal bit
for bit.  For 2x2 / N = 128 one row per distinct parameter is held against the 80-bit truth of tests/referee.py: relative H^1_0 in
long double <= SNAP_TOL (the rows of the library before the skipping sat at 3e-14 there)."""
import json

import numpy as np
import pytest

import sweep_truth as st
from conftest import observed

pytestmark = pytest.mark.gpu

M = 130
SNAP_TOL = st.SNAP_TOL
CASES = [((2, 2), 128), ((3, 3), 64), ((2, 3), 128), ((2, 2), 171), ((2, 2), 250)]


def parameters(blocks, N):
    """(D, kblk), as tests/test_gpu_ext_trunc.py: ones | first block at 1e8 | last block at 1e8 | all 1e8 | two rows 10^U(0, 8)."""
    k = blocks[0] * blocks[1]
    a = np.ones((6, k))
    a[1, 0] = 1e8
    a[2, k - 1] = 1e8
    a[3] = 1e8
    a[4:] = 10.0 ** np.random.default_rng([0xE7, k, N]).uniform(0, 8, size=(2, k))
    return a


def sweep(ctx, blocks, N, ab, monkeypatch, env):
    from romhighcontrast_amd import _ffi
    for name in ("ROMHC_NO_EXT_WAVE_SKIP", "ROMHC_NO_EXT_TRUNC"):
        if name in env:
            monkeypatch.setenv(name, "1")
        else:
            monkeypatch.delenv(name, raising=False)
    fem = _ffi.Fem(ctx, blocks[0], blocks[1], N)  # (the switches are read once per FE space)
    U = ctx.alloc(M * fem.dim)
    U.fill(float("nan"))
    fem.solve_batch(ab, M, U)
    rows = U.download(shape=(M, fem.dim))
    for name in env:
        monkeypatch.delenv(name, raising=False)
    return rows


@pytest.mark.parametrize("blocks,N", CASES, ids=[f"{b[0]}x{b[1]}-N{n}" for b, n in CASES])
def test_wave_skip_gives_the_same_rows(blocks, N, monkeypatch):
    from romhighcontrast_amd import _ffi
    ctx = _ffi.get_context()
    a = parameters(blocks, N)
    D = len(a)
    idx = st.idx_pattern(M, D)
    assert st.check_idx(idx, M, D)
    ab = ctx.upload(np.ascontiguousarray(a[idx]))
    skip = sweep(ctx, blocks, N, ab, monkeypatch, ())
    plain = sweep(ctx, blocks, N, ab, monkeypatch, ("ROMHC_NO_EXT_WAVE_SKIP",))
    skip_full = sweep(ctx, blocks, N, ab, monkeypatch, ("ROMHC_NO_EXT_TRUNC",))
    plain_full = sweep(ctx, blocks, N, ab, monkeypatch, ("ROMHC_NO_EXT_TRUNC", "ROMHC_NO_EXT_WAVE_SKIP"))
    for name, r in (("skip", skip), ("no_wave_skip", plain), ("skip, no_ext_trunc", skip_full), ("no_wave_skip, no_ext_trunc", plain_full)):
        assert np.isfinite(r).all(), name
    assert np.array_equal(skip, plain)
    assert np.array_equal(skip_full, plain_full)
    if (blocks, N) == ((2, 2), 128):
        first = np.array([int(np.flatnonzero(idx == d)[0]) for d in range(D)])
        out = [st.rf.referee(blocks, N, ad.reshape(blocks), verbose=False) for ad in a]
        g = out[0][0]
        dist = [st.rel_h10_ld(g, skip[first[d]], out[d][1]) for d in range(D)]
        print(json.dumps(dict(test="test_gpu_ext_wave_skip", blocks=list(blocks), N=N, M=M, tol=SNAP_TOL, to_truth_rows=[float(x) for x in dist])))
        observed("ext_wave_skip 2x2/N=128 vs 80-bit truth", dist, SNAP_TOL)
