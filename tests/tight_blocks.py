"""The block arguments of a map's fit and predict at the edge of their buffers (shared by test_gpu_poly_map.py, test_gpu_tree.py
and test_gpu_mlp.py): M = 50 rows, m = 2, q = 3, strides ldx = ldy = ldr = 8 and ldo = 5, nonzero offsets.  X, Y, OUT and Yref
each END ON THE LAST DOUBLE of a buffer of their own: every call is accepted and returns the bits of the same call on buffers
with 64 spare doubles; with one double fewer every call is refused with the `holds` message of csrc/rom_block.h."""
import numpy as np
import pytest

M, m, q, LD, LDO = 50, 2, 3, 8, 5
X_OFF, Y_OFF, O_OFF, R_OFF = 3, 5, 2, 1
N_OUT = O_OFF + (M - 1) * LDO + q


def block(ctx, A, off, ld, spare):
    """A's rows from element `off` with stride ld in a buffer that ends `spare` doubles after the last one (-1: one short)."""
    rows, cols = A.shape
    flat = np.zeros(off + (rows - 1) * ld + cols + max(spare, 0))
    for i, row in enumerate(A):
        flat[off + i * ld:off + i * ld + cols] = row
    return ctx.upload(flat[:flat.size + min(spare, 0)])


def data():
    rng = np.random.default_rng(5)
    return rng.uniform(-1, 1, (M, m)), rng.standard_normal((M, q))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def check(ctx, prefix, fit):
    """fit(X, x_off, ldx, m, Y, y_off, ldy, q, M) -> handle.  Returns the handle fitted on the tight buffers and the buffers
    (X, Y, Yref) by spare doubles: 0, 64, -1."""
    from romhighcontrast_amd import _ffi
    X, Y = data()
    bufs = {s: (block(ctx, X, X_OFF, LD, s), block(ctx, Y, Y_OFF, LD, s), block(ctx, Y, R_OFF, LD, s)) for s in (0, 64, -1)}
    assert bufs[0][0].n == X_OFF + (M - 1) * LD + m and bufs[-1][1].n == Y_OFF + (M - 1) * LD + q - 1
    maps = {s: fit(bufs[s][0], X_OFF, LD, m, bufs[s][1], Y_OFF, LD, q, M) for s in (0, 64)}
    for with_ref in (False, True):
        got = {}
        for s in (0, 64):
            out = ctx.alloc(N_OUT + s).fill(0.0)
            ss = maps[s].predict(bufs[s][0], X_OFF, LD, M, OUT=out, o_off=O_OFF, ldo=LDO, Yref=bufs[s][2] if with_ref else None,
                                 r_off=R_OFF, ldr=LD, sumsq=True)
            got[s] = (out, ss)
        assert got[0][0].same_bits_as(got[64][0], N_OUT), with_ref
        assert np.array_equal(_bits(got[0][1]), _bits(got[64][1])) and np.all(got[0][1] > 0.0), with_ref

    def fails(words, fn, *args, **kw):
        with pytest.raises(_ffi.RomLibraryError) as ei:
            fn(*args, **kw)
        assert all(w in str(ei.value) for w in words), str(ei.value)

    Xt, Yt, Rt = bufs[0]
    Xs, Ys, Rs = bufs[-1]
    out = ctx.alloc(N_OUT)
    fails([prefix + "_fit", f"X holds {Xs.n} doubles, 50 rows of 2 at offset 3 with stride 8"], fit, Xs, X_OFF, LD, m, Yt, Y_OFF, LD, q, M)
    fails([prefix + "_fit", f"Y holds {Ys.n} doubles, 50 rows of 3 at offset 5 with stride 8"], fit, Xt, X_OFF, LD, m, Ys, Y_OFF, LD, q, M)
    pred = maps[0].predict
    fails([prefix + "_predict", f"X holds {Xs.n}"], pred, Xs, X_OFF, LD, M, OUT=out, o_off=O_OFF, ldo=LDO)
    fails([prefix + "_predict", f"OUT holds {N_OUT - 1} doubles, 50 rows of 3 at offset 2 with stride 5"], pred, Xt, X_OFF, LD, M,
          OUT=ctx.alloc(N_OUT - 1), o_off=O_OFF, ldo=LDO)
    fails([prefix + "_predict", f"Yref holds {Rs.n}"], pred, Xt, X_OFF, LD, M, OUT=out, o_off=O_OFF, ldo=LDO, Yref=Rs, r_off=R_OFF, ldr=LD)
    return maps[0], bufs
