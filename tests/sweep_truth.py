"""Cases, truths and route restatement for the snapshot sweep (rom_solve_batch and its two stages rom_solve_reduced_async /
rom_expand_batch_async).  TEST INFRASTRUCTURE: imports the oracle and tests/referee.py; nothing in the product path may import
this.  tests/test_sweep_truth_host.py proves it on the CPU before tests/test_gpu_sweep.py relies on it.

A batch is built from D distinct parameter vectors a_d = 10^U(0, 4) per block, each with an 80-bit truth
(referee.referee: SuperLU + refinement with long-double edge-form residuals); system m of a batch of M carries a_{idx[m]},
idx seeded, containing every d (M >= D) and never the same d twice in a row.  Then
    (a) rows of equal idx must be equal bit for bit wherever they sit in the batch (in a 128-system tile of k_extend128, a
        64-system tile of k_expand / k_extend, the four-system workgroup of k_solve1, the pair of k_diag_update<2>), and
    (b) one row per d within SNAP_TOL of truth_d in relative H^1_0 (long double)
together check EVERY row of the batch against a truth.
"""
from collections import namedtuple

import numpy as np

from oracle import rom_oracle as ro
import referee as rf

LD = np.longdouble
SNAP_TOL = 1e-11          # the project's snapshot bound (tests/test_gpu_parity.py)
RESID_TOL = 1e-11         # |r|_inf / (4 a_max |u|_inf), the bound of test_full_size_c2_properties
ORACLE_TOL = 1e-12        # the SuperLU oracle must sit ten times inside SNAP_TOL of the truth (host test)
SENT_BITS = np.uint64(0x7FF8DEADBEEF0001)             # a NaN with a payload: the guard bands (as tests/test_gpu_fe_ops.py)
SENTINEL = np.array([SENT_BITS], dtype=np.uint64).view(np.float64)[0]

# both sides of: the pair of k_diag_update<2>, the four systems of a k_solve1 workgroup, every 64-system tile, the
# Mc >= 128 switch to k_extend128, a last 128-tile with one system and one with 65
FULL_MS = (1, 2, 3, 4, 5, 63, 64, 65, 127, 128, 129, 193, 257)
DISTINCT_M = 257
BIG_M = 2049              # first size past the Mc > 2048 switch to k_diag_update<1>

Case = namedtuple("Case", "id blocks N Ms row0 path routes")

# `path`: the reduced solve the geometry selects; `routes`: the kernel-level routes of ROUTES that a sweep of 129 systems
# takes (a sweep of fewer than 128: narrow_routes(routes)); tests/sweep_child.py confirms both from the profile names
_ST, _TC, _CF = "single_tile", "tile_cholesky", "closed_form"
_TILE = ("rhs", "diag_update", "diag_factor", "factor_panel", "backsolve", "coef")
_FOLD_FLAT, _FOLD_ROW = ("expand_folded", "extend_lr_128_flat"), ("expand_folded", "extend_lr_128_row")
_SINE = ("expand", "back_pre", "edge_transform", "extend", "scatter_interface")   # an edge in sine modes: general blocks
CASES = [
    Case("2x2-N16", (2, 2), 16, FULL_MS, 1, _ST, ("solve1",) + _FOLD_FLAT),
    Case("2x2-N65", (2, 2), 65, (65, 129), 2, _ST, ("solve1",) + _FOLD_FLAT),          # mesh rows of 64 vertices
    Case("2x2-N66", (2, 2), 66, (63, 129), 1, _ST, ("solve1",) + _FOLD_FLAT),          # ... and of 65
    Case("1x2-N128", (1, 2), 128, (5, 129), 3, _CF, ("rhs", "coef") + _FOLD_ROW),      # the one edge eliminated in closed form
    Case("2x2-N128", (2, 2), 128, (3, 129, 257), 1, _ST, ("solve1",) + _FOLD_ROW),     # C2
    Case("3x3-N24", (3, 3), 24, FULL_MS, 2, _TC, _TILE + _SINE),                       # 6 tiles in 3 tile columns
    Case("2x3-N40", (2, 3), 40, FULL_MS, 1, _TC, _TILE + _FOLD_FLAT),                  # 3 tiles in 2 columns, k_extend128
    Case("5x4-N33", (5, 4), 33, (64, 129), 1, _TC, _TILE + _FOLD_FLAT + ("extend_128_multi_launch",)),   # 20 blocks
    Case("1x1-N8", (1, 1), 8, (5, 129), 2, _CF, ("rhs", "coef", "extend")),            # no interface
    Case("1x3-N7", (1, 3), 7, (5, 129), 1, _ST, ("solve1",) + _SINE),
    Case("2x2-N3", (2, 2), 3, (5, 129), 3, _ST, ("solve1",) + _SINE),                  # two-node edges
    Case("2x2-N2", (2, 2), 2, (5, 129), 1, _ST, ("solve1",) + _SINE),                  # one-node edges, dim 9
    # blocks wider than one 128-vertex tile (n1 >= 128): what k_extend128 does at the sizes of C4 and C5
    Case("2x2-N171", (2, 2), 171, (5, 129, 257), 2, _ST, ("solve1",) + _FOLD_FLAT),    # C4's block: flat tiles inside one mesh row, n1 even
    Case("3x3-N140", (3, 3), 140, (64, 129), 1, _TC, _TILE + _FOLD_FLAT),              # n1 odd: pairs straddle rows; four-sided centre block
    Case("2x2-N250", (2, 2), 250, (3, 129, 257), 3, _ST, ("solve1",) + _FOLD_ROW),     # two column tiles, the second of 121 vertices
    Case("1x2-N257", (1, 2), 257, (5, 129), 1, _CF, ("rhs", "coef") + _FOLD_ROW),      # two full column tiles; sides of one K chunk
]
CASE = {c.id: c for c in CASES}
FULL_CASES = ("2x2-N16", "3x3-N24", "2x3-N40")      # a single-tile and two tile Cholesky geometries (general blocks;
#                                                     compressed blocks: k_extend128) carry FULL_MS
CHUNK_CASES = ("2x2-N16", "3x3-N24")
DISTINCT_CASES = ("2x2-N16", "3x3-N24", "1x2-N128", "2x2-N250")
DISTINCT_MS = {"2x2-N250": 129}     # (dim 249 001: one full 128-system tile and one system more; the others carry DISTINCT_M)
BIG_CASE = "3x3-N24"
C2_CASE = "2x2-N128"
WIDE_CASES = ("2x2-N171", "3x3-N140", "2x2-N250", "1x2-N257")
SYS_FAST_CASE = "3x3-N140"
SYS_FAST_M = 1921         # 16 system groups, the fewest that switch the workgroup order; the last group holds one system
SYS_FAST_BYTES = 64 << 20
SYS_FAST_GROUPS = 16

ROUTES = {
    "solve1": "the whole reduced solve in k_solve1 (single tile)",
    "rhs": "tile Cholesky: k_rhs",
    "diag_update": "tile Cholesky: k_diag_update",
    "diag_factor": "tile Cholesky: k_diag_factor",
    "factor_panel": "tile Cholesky: k_factor_panel (a tile column with tiles below the diagonal)",
    "backsolve": "tile Cholesky: k_backsolve",
    "coef": "tile Cholesky: k_coef",
    "expand": "k_expand as a launch of its own",
    "expand_folded": "the expansion rides in the first k_extend128 launch (extend_lr without expand)",
    "back_pre": "k_back_pre: a closed-form edge recovered node by node",
    "edge_transform": "k_edge_transform: an edge enters the extension in sine modes",
    "extend": "k_extend over general blocks",
    "extend_lr_64": "compressed blocks in 64-vertex tiles of one mesh row (k_extend, fewer than 128 systems or tiles that pad)",
    "extend_lr_128_row": "k_extend128, 128 vertices of one mesh row",
    "extend_lr_128_flat": "k_extend128, 128 consecutive vertices of the block",
    "extend_128_multi_launch": "more than 16 compressed blocks: several k_extend128 launches",
    "extend_128_sys_fast": "k_extend128 with the system group varying fastest (large tables, at least 16 system groups)",
    "scatter_interface": "k_scatter_interface: interface values copied by a kernel of their own",
    "diag_update_single": "more than 2048 systems: k_diag_update<1>",
    "chunked": "a workspace limit splits the sweep into chunks",
    "chunk_reuse": "a later, larger sweep runs in chunks of the workspace an earlier one left (ws_M >= 256)",
}
X128_BLOCKS = 16          # block descriptors per k_extend128 launch (rom_fem_dev.h)
BK = 16                   # K chunk (romhc_internal.h)


def n_params(case):
    g = ro.Geometry(case.blocks, case.N)
    return 4 if g.dim > 30000 else 8


def params(case):
    """The D parameter vectors of a case, (D, kblk), 10^U(0, 4), seeded by the geometry."""
    p, q = case.blocks
    rng = np.random.default_rng([0x5EE9, p, q, case.N])
    return 10.0 ** rng.uniform(0, 4, size=(n_params(case), p * q))


def distinct_params(case, M=None):
    """M (default: DISTINCT_MS[case.id], else DISTINCT_M) parameter vectors, all different (a value-dependent mix-up that
    repeated vectors could mask)."""
    M = DISTINCT_MS.get(case.id, DISTINCT_M) if M is None else M
    p, q = case.blocks
    rng = np.random.default_rng([0xD157, p, q, case.N])
    a = 10.0 ** rng.uniform(0, 4, size=(M, p * q))
    assert len(np.unique(a, axis=0)) == M
    return a


def idx_pattern(M, D):
    """idx (M,) in [0, D): a seeded permutation of the d first (every d occurs when M >= D), then seeded draws that differ
    from their predecessor."""
    rng = np.random.default_rng([0x1D8, M, D])
    out = [int(d) for d in rng.permutation(D)[:M]]
    while len(out) < M:
        d = int(rng.integers(D))
        if d != out[-1]:
            out.append(d)
    return np.array(out, dtype=np.int64)


def check_idx(idx, M, D):
    idx = np.asarray(idx)
    return len(idx) == M and idx.min() >= 0 and idx.max() < D and (M < D or set(idx.tolist()) == set(range(D))) \
        and not (idx[1:] == idx[:-1]).any()


_truths = {}


def truths(case):
    """dict(g, a (D, kblk), truth (D, dim) fp64, err_superlu (D,), hist): the referee's truth of every a_d and the distance of
    its own SuperLU start from it.  Cached per case for the process."""
    if case.id not in _truths:
        a = params(case)
        out = [rf.referee(case.blocks, case.N, ad.reshape(case.blocks), verbose=False) for ad in a]
        _truths[case.id] = dict(g=out[0][0], a=a, truth=np.stack([o[1] for o in out]),
                                err_superlu=np.array([o[3] for o in out]), hist=[o[4] for o in out])
    return _truths[case.id]


def rel_h10_ld(g, x, t):
    """||x - t||_{H10} / ||t||_{H10} of one row, long double."""
    x, t = np.asarray(x).astype(LD), np.asarray(t).astype(LD)
    return float(rf.h10_ld(g, x - t) / rf.h10_ld(g, t))


def residual_norm_ld(g, a, u):
    """|B - A(a) u|_inf / (4 a_max |u|_inf) with the residual in long double, edge form (the normalisation of
    test_full_size_c2_properties)."""
    a = np.asarray(a, dtype=np.float64).reshape(g.nrb, g.ncb)
    we, wn, wb = rf.edge_weights(g, a)
    r = rf.residual_ld(g, we, wn, wb, ro.load_vector(g), np.asarray(u, dtype=np.float64).astype(LD))
    return float(np.abs(r).max() / (4 * a.max() * np.abs(u).max()))


# ---- route restatement --------------------------------------------------------------------------------------------------
def extension_tiling(n1, Mc):
    """enqueue_solve's choice of the tiles of the compressed blocks' extension (rom_fem_solve.hip, `t_row` ... `wide`),
    restated: 'row' | 'flat' (k_extend128) or 't64' (k_extend).  The interface-vector half of `fits32` (128 nGp doubles
    below 4 GB) holds for every geometry the library accepts at these sizes."""
    t_row, t_flat = n1 * ((n1 + 127) // 128), (n1 * n1 + 127) // 128
    flat = 100 * t_flat < 97 * t_row                        # the 97 % rule: flat tiles only where they save 3 % of the tiles
    t128 = t_flat if flat else t_row
    fits32 = n1 * n1 * 64 * BK * 8 < 1 << 32
    wide = Mc >= 128 and fits32 and 100 * 128 * t128 <= 102 * 64 * n1 * ((n1 + 63) // 64)   # the 102 % padding rule
    return ("flat" if flat else "row") if wide else "t64"


def system_fast_order(gs_bytes, Mc):
    """enqueue_solve's choice of k_extend128's workgroup order (rom_fem_solve.hip, `order`), restated: the system group varies
    fastest when the segment-major extension tables (the planner's gstotal doubles) hold at least 64 MiB and the chunk has at
    least 16 groups of 128 systems."""
    return gs_bytes >= SYS_FAST_BYTES and (Mc + 127) // 128 >= SYS_FAST_GROUPS


def narrow_routes(routes):
    """The routes of a sweep of fewer than 128 systems, from those of 129: no k_extend128, hence no fold."""
    swap = {"expand_folded": "expand", "extend_lr_128_row": "extend_lr_64", "extend_lr_128_flat": "extend_lr_64",
            "extend_128_multi_launch": None}
    return tuple(sorted({swap.get(r, r) for r in routes} - {None}))


def chunks_of(M, Mc_max):
    return [min(Mc_max, M - m0) for m0 in range(0, M, Mc_max)]


def nodal_part(fem):
    """[nodal_begin, nodal_end) of an interface vector of the _ffi.Fem: what the expansion writes and never reads."""
    import ctypes
    b, e = ctypes.c_int64(0), ctypes.c_int64(0)
    assert fem.ctx.lib.rom_fem_reduced_layout(fem.h, ctypes.byref(b), ctypes.byref(e)) == 0
    return b.value, e.value


def per_system_workspace(n_tiles, nodal_begin, stride):
    """solve_batch_impl's `per_sys` in bytes: the tiles of L, one inverse per tile column (the reduced part of an interface
    vector is 64 doubles per tile column) and two interface vectors."""
    return (n_tiles * 4096 + (nodal_begin // 64) * 4096 + 2 * stride) * 8


def routes_of_profile(prof, n1, Mc, n_lr_blocks, expands):
    """Routes of ROUTES that one sweep of chunks of Mc systems took, from its profile {name: launches} (ROM_PROF labels;
    under ROMHC_PROF_DETAIL the per-column kernels carry a _jNN suffix and a k_extend128 launch in the system-fast order is
    extend_lr_sysfast: extend_lr for everything else), the number of compressed blocks (ROMHC_VERBOSE
    prints it) and `expands`: whether a sweep of fewer than 128 systems of the same geometry -- which never folds --
    launched k_expand (a geometry with nothing to expand launches it nowhere: that is not a fold)."""
    names = {nm.split("_j")[0] if nm[-4:-2] == "_j" else nm for nm, n in prof.items() if n > 0}
    out = set(names & {"solve1", "rhs", "diag_update", "diag_factor", "factor_panel", "backsolve", "coef", "expand", "back_pre",
                       "edge_transform", "extend", "scatter_interface"})
    if "extend_lr_sysfast" in names:
        names = names - {"extend_lr_sysfast"} | {"extend_lr"}
        out.add("extend_128_sys_fast")
    if "extend_lr" in names:
        t = extension_tiling(n1, Mc)
        out.add({"t64": "extend_lr_64", "row": "extend_lr_128_row", "flat": "extend_lr_128_flat"}[t])
        if t != "t64" and expands and "expand" not in names:
            out.add("expand_folded")
        if t != "t64" and n_lr_blocks > X128_BLOCKS:
            out.add("extend_128_multi_launch")
    if "diag_update" in names and Mc > 2048:
        out.add("diag_update_single")
    return out
