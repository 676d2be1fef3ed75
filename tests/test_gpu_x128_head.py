"""The compact head of k_extend128 on the GPU: a tile workgroup reads a small leading kernel argument and its tile's record from
the planner (X128Tile, rom_fem_plan.h) instead of the block's side descriptors, and no longer walks the skip thresholds itself.
Placement and bookkeeping changed, no product did, so the rows of every route must be the rows of the default, byte for byte.

Every case solves M = 130 systems (the last system group holds two) on fresh Fems:
  * 2x2 / N = 128: row tiles;
  * 3x3 / N = 64: FLAT tiles, the centre block with four sides;
  * 5x4 / N = 64: 20 blocks, so a second launch with its own block indexing, and the folded expansion riding in the first only.
Routes (tests/x128_head_child.py, in a subprocess with the A/B library, which can force them): ROMHC_NO_EXT_WAVE_SKIP (the mask of
the record is bypassed: a wrong record shows), ROMHC_X128_SYS_FAST = 0 / 1 / 2, ROMHC_EXT_FLAT = 0 / 1 (with and without the masks),
ROMHC_NO_FOLD_EXPAND, ROMHC_NO_EXT_LR.  The product library's default rows, solved in this process, must be the child's too."""
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

import x128_head_child as child

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [(2, 2, 128), (3, 3, 64), (5, 4, 64)]


@pytest.mark.parametrize("nrb,ncb,N", CASES, ids=[f"{r}x{c}-N{n}" for r, c, n in CASES])
def test_every_route_gives_the_default_rows(nrb, ncb, N):
    from romhighcontrast_amd import _ffi
    lib_ab = os.path.join(ROOT, "romhighcontrast_amd", "csrc", "libromhc_ab.so")
    assert os.path.exists(lib_ab), "libromhc_ab.so missing: `make -C romhighcontrast_amd/csrc` builds it beside libromhc.so"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "x128_head_child.py"), str(nrb), str(ncb), str(N)],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    out = r.stdout.decode()
    print(out)
    lines = out.splitlines()
    routes = {ln.split()[1]: int(ln.split()[3]) for ln in lines if ln.startswith("route ")}
    assert set(routes) == {name for name, _ in child.ROUTES}, out[-4000:]
    assert all(v == 0 for v in routes.values()), routes
    assert r.returncode == 0 and lines[-1] == "OK", out[-4000:]
    # the product library, here: the same default rows
    ctx = _ffi.get_context()
    fem = _ffi.Fem(ctx, nrb, ncb, N)
    U = ctx.alloc(child.M * fem.dim)
    U.fill(float("nan"))
    fem.solve_batch(ctx.upload(child.parameters(nrb, ncb, N)), child.M, U)
    rows = U.download(shape=(child.M, fem.dim))
    assert np.isfinite(rows).all()
    digest = [ln.split()[2] for ln in lines if ln.startswith("default sha256 ")]
    assert digest == [hashlib.sha256(rows.tobytes()).hexdigest()]
