"""Child of tests/test_gpu_x128_head.py (a process loads one library: this one loads libromhc_ab.so, whose switches force the
routes of k_extend128).  Solves M = 130 systems of one geometry on a fresh Fem per route and compares every route's rows with the
default's, byte for byte.

    python tests/x128_head_child.py NRB NCB N     prints one line "route <name> differing <doubles>" per route, then
                                                  "default sha256 <digest of the default rows>" and a last line "OK" or "FAILED"
TEST INFRASTRUCTURE."""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from romhighcontrast_amd import _ffi  # noqa: E402

M = 130
ROUTES = (("no_wave_skip", {"ROMHC_NO_EXT_WAVE_SKIP": "1"}), ("sys_fast_0", {"ROMHC_X128_SYS_FAST": "0"}),
          ("sys_fast_1", {"ROMHC_X128_SYS_FAST": "1"}), ("sys_fast_2", {"ROMHC_X128_SYS_FAST": "2"}),
          ("ext_flat_0", {"ROMHC_EXT_FLAT": "0"}), ("ext_flat_1", {"ROMHC_EXT_FLAT": "1"}),
          ("flat_no_wave_skip", {"ROMHC_EXT_FLAT": "1", "ROMHC_NO_EXT_WAVE_SKIP": "1"}),
          ("row_no_wave_skip", {"ROMHC_EXT_FLAT": "0", "ROMHC_NO_EXT_WAVE_SKIP": "1"}),
          ("no_fold_expand", {"ROMHC_NO_FOLD_EXPAND": "1"}), ("no_ext_lr", {"ROMHC_NO_EXT_LR": "1"}))


def parameters(nrb, ncb, N):
    return 10.0 ** np.random.default_rng([0x128, nrb, ncb, N]).uniform(0, 3, size=(M, nrb * ncb))


def sweep(ctx, nrb, ncb, N, ab, env):
    for k, v in env.items():
        os.environ[k] = v
    try:
        fem = _ffi.Fem(ctx, nrb, ncb, N)  # (the switches are read once per FE space)
        U = ctx.alloc(M * fem.dim)
        U.fill(float("nan"))
        fem.solve_batch(ab, M, U)
        return U.download(shape=(M, fem.dim))
    finally:
        for k in env:
            del os.environ[k]


if __name__ == "__main__":
    nrb, ncb, N = (int(x) for x in sys.argv[1:4])
    _ffi.load_library(os.path.join(ROOT, "romhighcontrast_amd", "csrc", "libromhc_ab.so"))
    ctx = _ffi.get_context()
    ab = ctx.upload(parameters(nrb, ncb, N))
    ref = sweep(ctx, nrb, ncb, N, ab, {})
    ok = bool(np.isfinite(ref).all())
    print(f"default finite {ok}", flush=True)
    for name, env in ROUTES:
        rows = sweep(ctx, nrb, ncb, N, ab, env)
        differing = int(np.count_nonzero(rows.view(np.uint64) != ref.view(np.uint64)))
        print(f"route {name} differing {differing}", flush=True)
        ok = ok and differing == 0
    print("default sha256 " + hashlib.sha256(ref.tobytes()).hexdigest())
    print("OK" if ok else "FAILED")
    sys.exit(0 if ok else 1)
