"""rom_nearest on the GPU against the 80-bit checker of tests/nearest_truth.py.

Every case runs the screened search (mode 0) and the exhaustive kernel (mode 1): the two must return identical bits, and both
answers go through check_neighbours (distances within (r + 2) eps of the exact ones, rows sorted by (dist2, index), nothing
nearer left out beyond 1 + 2 (r + 2) eps).  Q and P are column ranges of NaN-filled blocks with wider strides, which must come
back bit for bit.  Shapes: the smallest that reach each edge of the kernels -- one library row; a library shorter than one
32-row slab with r = 1; one row past a slab with one query past a 16-query tile; r = 5 padded to 8 with one query past a
128-query table and a library over several workgroup chunks; r = 128, the widest."""
import numpy as np
import pytest

import nearest_truth as nt

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from romhighcontrast_amd import _ffi
    return _ffi.get_context()


def _same_bits(a, b):
    return np.array_equal(np.asarray(a).view(np.uint64), np.asarray(b).view(np.uint64))


class Block:
    """rows x r values from column `col` of rows [1, 1 + rows) of a NaN block with `extra` more columns."""

    def __init__(self, ctx, X, col, extra):
        rows, r = X.shape
        self.ld = r + extra
        self.off = self.ld + col
        self.host = np.full((rows + 2, self.ld), np.nan)
        self.host[1:1 + rows, col:col + r] = X
        self.buf = ctx.upload(self.host)

    def unchanged(self):
        return _same_bits(self.buf.download(shape=self.host.shape), self.host)


def _search(ctx, Q, P, t, modes=(0, 1)):
    """Both modes on NaN-framed copies of the operands; checks bits, the checker and the operands; returns mode 0's answer."""
    M, r = Q.shape
    K = len(P)
    qb, pb = Block(ctx, Q, 2, 5), Block(ctx, P, 1, 3)
    out = []
    for mode in modes:
        idx, d2, info = ctx.nearest(qb.buf, qb.off, qb.ld, M, pb.buf, pb.off, pb.ld, K, r, t=t, mode=mode)
        nt.check_neighbours(P, Q, idx, d2, t)
        assert info["group_size"] == 32 and info["certified"] + info["fallbacks"] == K, info
        if mode == 1:
            assert info["certified"] == 0 and info["fallbacks"] == K and info["groups_rescored"] == 0, info
        out.append((idx, d2, info))
    assert qb.unchanged() and pb.unchanged()
    for idx, d2, _ in out[1:]:
        assert np.array_equal(idx, out[0][0]), np.argwhere(idx != out[0][0])[:4]
        assert _same_bits(d2, out[0][1])
    return out[0]


#          id                  kind       M     K    r   t
EDGES = [("one_row",          "uniform", 1,    3,   4,   1),
         ("short_slab_r1",    "uniform", 31,   5,   1,   8),
         ("slab_plus_one",    "uniform", 33,   17,  3,   4),
         ("pad_r_table_edge", "uniform", 2049, 129, 5,   8),
         ("widest_r",         "uniform", 257,  16,  128, 4),
         ("ulp_ties",         "ulp",     700,  20,  3,   8),
         ("graded",           "graded",  1500, 24,  8,   4)]


@pytest.mark.parametrize("name,kind,M,K,r,t", EDGES, ids=[c[0] for c in EDGES])
def test_edges(ctx, name, kind, M, K, r, t):
    Q, P = nt.build_case(kind, M, K, r, seed=len(name))
    if kind == "ulp":
        Q = Q[np.random.default_rng(1).permutation(M)]
    _search(ctx, Q, P, t)


@pytest.mark.parametrize("kind", ["uniform", "offset", "graded"])
@pytest.mark.parametrize("t", [1, 8])
def test_screen_certifies_everything(ctx, kind, t):
    """On uniform data, the same at offset 1e8 (the centring) and on graded columns the screen certifies every query."""
    Q, P = nt.build_case(kind, 4133, 64, 16, seed=3)
    _, _, info = _search(ctx, Q, P, t)
    print(info)
    assert info["fallbacks"] == 0 and info["certified"] == 64 and info["groups_rescored"] == t + 4, info


def test_queries_that_are_library_rows(ctx):
    Q, P = nt.build_case("self", 1000, 40, 10, seed=5)
    idx, d2, info = _search(ctx, Q, P, 3)
    assert (d2[:, 0] == 0.0).all() and not np.signbit(d2[:, 0]).any()
    assert np.array_equal(Q[idx[:, 0]], P)
    assert info["fallbacks"] == 0, info


def test_best_row_copied_into_more_groups_than_rescored(ctx):
    """Exact copies of the best row in T' + 2 groups: the lowest rows win the ties, and the screen cannot certify the query."""
    t, K, r = 3, 3, 6
    Q0, P0 = nt.build_case("uniform", 64, 1, r)
    Tp = ctx.nearest(ctx.upload(Q0), 0, r, 64, ctx.upload(P0), 0, r, 1, r, t=t)[2]["groups_rescored"]
    assert Tp >= t
    G = 32
    groups = list(range(2, 2 * (Tp + 2) + 2, 2))
    Q, P, rows = nt.copies_case(G * 40 + 7, K, r, groups, G, seed=7)
    idx, _, info = _search(ctx, Q, P, t)
    assert np.array_equal(idx, np.tile(rows[:t], (K, 1))), (idx, rows)
    assert info["fallbacks"] == K and info["certified"] == 0, info


def test_repeated_call_same_bits_and_query_passes(ctx):
    """The same bits on a repeated call; with a workspace limit of one 128-query table the 129 queries take two passes, and
    with no room for a table every query goes to the exhaustive kernel -- the same answer each time."""
    Q, P = nt.build_case("uniform", 2049, 129, 5, seed=11)
    qb, pb = ctx.upload(Q), ctx.upload(P)
    ref = ctx.nearest(qb, 0, 5, 2049, pb, 0, 5, 129, 5, t=4)
    again = ctx.nearest(qb, 0, 5, 2049, pb, 0, 5, 129, 5, t=4)
    assert np.array_equal(ref[0], again[0]) and _same_bits(ref[1], again[1]) and ref[2] == again[2]
    ngs = -(-(-(-2049 // 32)) // 16) * 16
    try:
        ctx.set_workspace_limit(128 * ngs * 8)
        two = ctx.nearest(qb, 0, 5, 2049, pb, 0, 5, 129, 5, t=4)
        ctx.set_workspace_limit(1000)
        none = ctx.nearest(qb, 0, 5, 2049, pb, 0, 5, 129, 5, t=4)
    finally:
        ctx.set_workspace_limit(24 << 30)
    assert two[2]["launches"] == ref[2]["launches"] + 2 and two[2]["fallbacks"] == ref[2]["fallbacks"], (ref[2], two[2])
    assert none[2]["fallbacks"] == 129 and none[2]["groups_rescored"] == 0, none[2]
    for other in (two, none):
        assert np.array_equal(ref[0], other[0]) and _same_bits(ref[1], other[1])


@pytest.mark.parametrize("where", ["P", "Q"])
@pytest.mark.parametrize("bad", [np.nan, np.inf])
@pytest.mark.parametrize("mode", [0, 1])
def test_non_finite_operands_are_an_error(ctx, where, bad, mode):
    from romhighcontrast_amd import _ffi
    Q, P = nt.build_case("uniform", 100, 5, 4)
    (P if where == "P" else Q)[3, 2] = bad
    with pytest.raises(_ffi.RomLibraryError, match="NaN / Inf"):
        ctx.nearest(ctx.upload(Q), 0, 4, 100, ctx.upload(P), 0, 4, 5, 4, t=2, mode=mode)


def test_argument_limits(ctx):
    from romhighcontrast_amd import _ffi
    Q, P = nt.build_case("uniform", 10, 2, 4)
    qb, pb = ctx.upload(Q), ctx.upload(P)
    idx, d2, info = ctx.nearest(qb, 0, 4, 10, pb, 0, 4, 0, 4, t=2)   # K = 0: a no-op
    assert idx.shape == (0, 2) and d2.shape == (0, 2) and info["launches"] == 0
    for kw in (dict(M=10, r=4, t=9), dict(M=10, r=4, t=0), dict(M=3, r=4, t=4), dict(M=11, r=4, t=1), dict(M=10, r=5, t=1)):
        with pytest.raises(_ffi.RomLibraryError):
            ctx.nearest(qb, 0, 4, kw["M"], pb, 0, 4, 2, kw["r"], t=kw["t"])
