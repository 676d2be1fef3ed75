"""Reader of the in-kernel cycle stamps of k_extend128 (dev tool; needs a library whose rom_fem_kernels.hip was compiled with
-DROMHC_X128_STAMPS: wave 0 of every workgroup then stores its stamps over the tile's first vertex of its first seven systems).
Prints the table of profiles/r02_extend128_percu_timeline_stamps.txt for C2 and C4.
usage: python tools/dev/gpu_x128_stamps.py path/to/libromhc_x128_stamps.so [c2 c4 ...]"""
import os
import sys
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from romhighcontrast_amd import _ffi

CONFIGS = {"c2": (2, 2, 128, 1024), "c4": (3, 3, 171, 1024), "c5": (4, 4, 256, 4096)}


def pct(name, v):
    print(f"  {name:<32s} mean {v.mean():8.0f}  median {np.median(v):8.0f}  p10 {np.percentile(v, 10):8.0f}  p90 {np.percentile(v, 90):8.0f}")


def run(ctx, nrb, ncb, N, M):
    fem = _ffi.Fem(ctx, nrb, ncb, N)
    a = 10.0 ** np.random.default_rng(20240807).uniform(0, 2, size=(M, nrb * ncb))
    ab = ctx.upload(a)
    Y = ctx.alloc(M * fem.reduced_stride)
    U = ctx.alloc(M * fem.dim)
    fem.solve_reduced(ab, M, Y)
    for _ in range(3):
        fem.expand(ab, M, Y, U)
    ctx.solve_status()
    ctx.timer_start()
    for _ in range(20):
        fem.expand(ab, M, Y, U)
    us = ctx.timer_stop() / 20 * 1e3
    rows = []  # per workgroup: entry, the four later stamps (cycles since entry), HW_ID, XCC_ID
    for m0 in range(0, M, 128):
        if m0 + 7 > M:
            continue
        blk = U.download(7 * fem.dim, offset=m0 * fem.dim).reshape(7, fem.dim)
        cols = np.nonzero(np.abs(blk[0]) > 1e6)[0]  # entry stamps: far above any solution value
        rows.append(blk[:, cols].T)
    st = np.concatenate(rows)
    entry, d = st[:, 0], st[:, 1:5]
    cu = st[:, 6].astype(np.int64) * 256 + ((st[:, 5].astype(np.int64) >> 8) & 0xff)  # XCC | SE, SH, CU
    cus = np.unique(cu)
    print(f"{nrb}x{ncb} blocks, N = {N}, {M} systems: {len(st)} workgroups on {len(cus)} CUs, expansion + extension {us:.1f} us;"
          f" lifetime mean {d[:, 3].mean():.0f} cycles, median {np.median(d[:, 3]):.0f}")
    pct("entry -> first loads issued", d[:, 0])
    pct("-> first barrier passed", d[:, 1] - d[:, 0])
    pct("-> k loop done", d[:, 2] - d[:, 1])
    pct("-> stores issued (end)", d[:, 3] - d[:, 2])
    spans, gaps, share, resident, shown = [], [], np.zeros(4), 0, None
    for c in cus:
        s = st[cu == c]
        s = s[np.argsort(s[:, 0])]
        e0, e1 = s[:, 0], s[:, 0] + s[:, 4]
        spans.append(e1.max() - e0.min())
        ev = sorted([(t, 1) for t in e0] + [(t, -1) for t in e1])
        n = 0
        for _, dn in ev:
            n += dn
            resident = max(resident, n)
        slots = resident if resident > 0 else 2
        ends = np.sort(e1)
        if len(s) > slots:
            gaps.append(e0[slots:] - ends[:len(s) - slots])
        ev = sorted([(t, 1) for t in s[:, 0] + s[:, 1]] + [(t, -1) for t in s[:, 0] + s[:, 3]])
        n, last = 0, e0.min()
        for t, dn in ev + [(e1.max(), 0)]:
            share[min(n, 3)] += t - last
            n, last = n + dn, t
        if shown is None:
            shown = s
    spans = np.array(spans)
    print(f"per-CU span mean {spans.mean():.0f} cycles (max {spans.max():.0f}); workgroups resident at once per CU: max {resident}")
    print("share of the CUs' spans with 0 / 1 / 2 / >=3 workgroups inside the k loop: " + " / ".join(f"{x:.3f}" for x in share / share.sum()))
    if gaps:
        pct("last stamp -> successor's entry", np.concatenate(gaps))
    print("one CU, first workgroups (cycles from the CU's first entry): entry / k loop start / k loop end / stores issued")
    for r in shown[:14]:
        t0 = r[0] - shown[0, 0]
        print(f"  {t0:9.0f} {t0 + r[1]:9.0f} {t0 + r[3]:9.0f} {t0 + r[4]:9.0f}")


if __name__ == "__main__":
    args = sys.argv[1:]
    if args and args[0].endswith(".so"):
        _ffi.load_library(os.path.abspath(args.pop(0)))
    ctx = _ffi.get_context(0)
    for name in args or ["c2", "c4"]:
        run(ctx, *CONFIGS[name])
