"""Every route of the dense fp64 primitives (rom_gemm_nt, rom_gram, rom_gemm_nn: csrc/rom_ops.hip) against references that
cannot be argued with, plus the row helpers, norms, orthonormalisations and buffer bit operations built on them.  Needs an
MI355X.

  * ROUTES: a restatement of the dispatch conditions of rom_launch_gemm_nt_ex, launch_gemm_nt_thin, rom_launch_gram and
    rom_launch_gemm_nn; the parametrised cases are chosen so that every route x split-K reducer is taken, which a pure
    Python assertion checks (a change of the thresholds shows up as a coverage failure, not as a silent drift).
  * EXACT cases: integer operands in [-8, 8], alpha = -0.75, beta = 0.5 (or 0): every product, partial sum, split-K
    partial and scaling is exact in fp64 for K up to 2^20, whatever the order, so the result must EQUAL NumPy's.  Operands
    and C sit inside larger buffers (leading dimensions beyond the window, odd offsets, NaN in the operand padding, a
    sentinel bit pattern around C) and nothing outside the m x n window of C may change.
  * ROUNDING cases: normal operands scaled over 10^+-8 against a long-double product of the same fp64 inputs, with the
    rigorous bound gamma_(k + s + 3) |alpha| |A||B| + 2 u |beta C| (s: K splits); split routes must also give the same bits
    twice and with the scratch area poisoned (ROMHC_POISON_WS: an unwritten partial would show up as NaN).
  * tests/dense_routes_child.py (a child process: ROMHC_PROF_DETAIL and ROMHC_NO_THIN_GEMM are read once per process)
    confirms every route from the profile names and runs the exact cases and a two-pass rom_pod on the general engine.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import observed

pytestmark = pytest.mark.gpu

BK = 16                       # romhc_internal.h: K chunk of the engines
ALPHA, BETA = -0.75, 0.5
SENTINEL = np.array([0x7FF8DEADBEEF0001], dtype=np.uint64).view(np.float64)[0]   # a NaN with a payload: C's guard band
U = 2.0 ** -53


def _ceil(a, b):
    return -(-a // b)


# =====================================================================================================================
# route table (rom_ops.hip)
# =====================================================================================================================
def _reducer(splits, mn):
    """k_splitk_reduce_{quad,wave,} choice of launch_splitk_reduce (the thin and the general NT routes; the general NN
    route asks for the plain reducer whatever the shape: route_gemm_nn)."""
    if splits <= 1:
        return "none"
    if splits >= 8 and 4096 <= mn <= (1 << 20):
        return "quad"
    if splits >= 16 and mn <= 65536:
        return "wave"
    return "plain"


def _nt_thin(m, n, k, transposed):
    """launch_gemm_nt_thin: (m, n) are the THIN operand's rows and the other's; last: the columns of K in the last split."""
    tiles = _ceil(n, 128)
    splits = max(1, min(_ceil(768, tiles), k // 512))                      # the splits it asks splitk_plan for
    kper = _ceil(_ceil(k, splits), BK) * BK                                 # splitk_plan
    splits = _ceil(k, kper)
    return dict(route="nt_thin_T" if transposed else "nt_thin", mi=min(4, _ceil(m, 16)), splits=splits,  # dispatch_mi
                reducer=_reducer(splits, m * n), kmin=None, last=k - (splits - 1) * kper)


def route_gemm_nt(m, n, k, lda, ldb, a_off, b_off, lower_only=0, no_thin=False):
    """rom_launch_gemm_nt_ex; a_off / b_off: element offsets into 256-byte aligned buffers."""
    if m <= 0 or n <= 0:
        return dict(route="noop", splits=0, reducer="none", mi=None, kmin=None)
    if not lower_only and m <= 64 and n >= 256 and k >= 2048 and lda * 8 * 64 < 2 ** 32 and ldb * 8 * 128 < 2 ** 32 \
            and not no_thin:                                                # thin A
        return _nt_thin(m, n, k, False)
    if not lower_only and n <= 64 and m >= 256 and k >= 2048 and ldb * 8 * 64 < 2 ** 32 and lda * 8 * 128 < 2 ** 32 \
            and not no_thin:                                                # thin B: the transposed product
        return _nt_thin(n, m, k, True)
    nt = _ceil(m, 64)
    tiles = nt * (nt + 1) // 2 if lower_only else nt * _ceil(n, 64)        # tiles that do work
    splits, kmin = 1, None
    if k >= 1024 and tiles < 512:
        kmin = 128 if tiles <= 4 else 512
        splits = max(1, min(_ceil(768, tiles), _ceil(k, kmin)))
    kper = _ceil(_ceil(k, splits), BK) * BK or BK                           # splitk_plan, with its guards for k == 0
    splits = max(1, _ceil(k, kper))
    aligned = lda % 2 == 0 and ldb % 2 == 0 and a_off % 2 == 0 and b_off % 2 == 0 and kper % 4 == 0
    if lower_only:
        route = "gram_lower"
    else:
        route = "nt_general_aligned" if aligned else "nt_general_unaligned"
    return dict(route=route, splits=splits, reducer=_reducer(splits, m * n), mi=None, kmin=kmin if splits > 1 else None)


def route_gram(m, k, lda, a_off):
    """rom_launch_gram: the 128-tile kernel from 512 rows and 4096 columns, else the lower-only engine."""
    if m <= 0:
        return dict(route="noop", splits=0, reducer="none", mi=None, kmin=None)
    if m >= 512 and k >= 4096 and lda * 8 * 128 < 2 ** 32:                 # launch_gram128
        return dict(route="gram128", splits=None, reducer="finish", mi=None, kmin=None)
    return route_gemm_nt(m, m, k, lda, lda, a_off, a_off, lower_only=1)


def route_gemm_nn(m, n, k, lda, ldb, no_thin=False):
    """rom_launch_gemm_nn (gemm_nn_thin / gemm_nn_splits)."""
    if m <= 0 or n <= 0:
        return dict(route="noop", splits=0, reducer="none", mi=None, kmin=None)
    if (k >= 128 if m <= 64 else 16 <= k <= 256) and n >= 1024 and lda * 8 * 64 < 2 ** 32 \
            and ldb * 8 * 16 + 1024 < 2 ** 32 and _ceil(m, 64) <= 65535 and not no_thin:
        return dict(route="nn_thin" if m <= 64 else "nn_lift", mi=_ceil(m, 16) if m <= 64 else 4, splits=1,
                    reducer="none", kmin=None)
    tiles = _ceil(n, 64) * _ceil(m, 64)
    splits = 1
    if tiles <= 32 and k >= 256:                                            # split-K of a handful of tiles
        splits = min(_ceil(256, tiles), k // 64)
        kper = _ceil(_ceil(k, splits), BK) * BK
        splits = _ceil(k, kper)
    return dict(route="nn_general", mi=None, splits=splits, reducer="plain" if splits > 1 else "none", kmin=None)


def route_of(case, no_thin=False):
    op, m, n, k, lay = case
    L = layout(case)
    if op == "nt":
        return route_gemm_nt(m, n, k, L["lda"], L["ldb"], L["a_off"], L["b_off"], no_thin=no_thin)
    if op == "gram":
        return route_gram(m, k, L["lda"], L["a_off"])
    return route_gemm_nn(m, n, k, L["lda"], L["ldb"], no_thin=no_thin)


def tags(r):
    """What a case covers: route / reducer, the 16-row block count of a thin operand, the kmin branch of the split, a last
    split of a thin NT product shorter than one K chunk (no full chunk: the kernel goes from its zero-padded tail straight
    to the store)."""
    t = {f"{r['route']}/{r['reducer']}"}
    if r["mi"] is not None and r["route"] in ("nt_thin", "nt_thin_T", "nn_thin"):
        t.add(f"{r['route']}/mi{r['mi']}")
    if r["kmin"] is not None:
        t.add(f"{r['route']}/kmin{r['kmin']}")
    if r.get("last") is not None and r["last"] < BK:
        t.add(f"{r['route']}/last_split_below_BK")
    return t


REQUIRED = (
    {f"nt_thin/{x}" for x in ("plain", "wave", "quad")} | {f"nt_thin/mi{i}" for i in (1, 2, 3, 4)}
    | {f"nt_thin_T/{x}" for x in ("plain", "wave", "quad")}
    | {"nt_thin/last_split_below_BK", "nt_thin_T/last_split_below_BK"}
    | {f"nt_general_{a}/{x}" for a in ("aligned", "unaligned") for x in ("none", "plain", "wave", "quad")}
    | {f"nt_general_{a}/kmin{q}" for a in ("aligned", "unaligned") for q in (128, 512)}
    | {f"gram_lower/{x}" for x in ("none", "plain", "wave", "quad")} | {"gram_lower/kmin128", "gram_lower/kmin512"}
    | {"gram128/finish"}
    | {f"nn_thin/mi{i}" for i in (1, 2, 3, 4)} | {"nn_thin/none", "nn_lift/none", "nn_general/none", "nn_general/plain"}
)

# (op, m, n, k, layout): layout "al" = even leading dimensions and offsets (16-byte aligned rows), "un" = odd ones
ROUTE_CASES = [
    # thin A (m <= 64, n >= 256, k >= 2048): MI = 1..4 and every reducer
    ("nt", 16, 256, 8192, "un"), ("nt", 1, 257, 8192, "un"), ("nt", 33, 513, 2049, "un"), ("nt", 24, 1024, 4100, "al"),
    ("nt", 64, 300, 2048, "un"), ("nt", 49, 1000, 5007, "al"),
    # 40 splits of 528 columns, the last of ONE column (odd leading dimensions), plain and transposed
    ("nt", 17, 300, 20593, "un"), ("nt", 300, 17, 20593, "al"),
    # thin B: the transposed product (C[c * ldc + r])
    ("nt", 256, 16, 8192, "un"), ("nt", 300, 1, 8192, "al"), ("nt", 1000, 50, 2049, "un"),
    # the general 64 x 64 engine: no split (k < 1024), kmin = 128 (<= 4 tiles), kmin = 512; every reducer
    *[("nt", m, n, k, lay) for lay in ("al", "un") for (m, n, k) in (
        (65, 127, 1000), (129, 65, 1100), (63, 64, 2047), (64, 64, 2049), (129, 129, 4500), (127, 1, 1500),
        (1, 129, 1030), (64, 300, 2047))],
    # Gram: lower-only engine (none / plain / wave / quad; 511 = the largest m below the 128-tile route) and k_gram128
    ("gram", 70, 70, 1000, "al"), ("gram", 200, 200, 1100, "un"), ("gram", 63, 63, 2049, "al"), ("gram", 127, 127, 4096, "un"),
    ("gram", 511, 511, 4096, "al"), ("gram", 512, 512, 4096, "al"), ("gram", 513, 513, 4099, "un"),
    # NN: thin MI = 1..4, the tall-A / short-K lift, general with and without split-K (24 x 272 x 1024: the factored sketch)
    ("nn", 1, 1024, 128, "un"), ("nn", 17, 1029, 129, "un"), ("nn", 33, 2000, 300, "al"), ("nn", 64, 1100, 200, "un"),
    ("nn", 130, 1029, 16, "un"), ("nn", 65, 2000, 256, "al"), ("nn", 50, 300, 100, "un"), ("nn", 24, 272, 1024, "al"),
    ("nn", 24, 272, 1000, "un"), ("nn", 129, 63, 300, "un"),
]
EDGE_CASES = [("nt", 65, 65, 0, "un"), ("nt", 0, 64, 100, "al"), ("nt", 64, 0, 100, "al"), ("gram", 70, 70, 0, "un"),
              ("nn", 65, 127, 0, "un"), ("nn", 0, 1024, 128, "al"), ("nn", 17, 0, 128, "al"), ("gram", 0, 0, 10, "al")]


def layout(case):
    """Leading dimensions beyond the window and offsets into the buffers (odd for "un"; C's offset is always odd)."""
    op, m, n, k, lay = case
    odd = lay == "un"
    lda = k + (3 if odd else 2)
    ldb = (n if op == "nn" else k) + (5 if odd else 4)
    if op == "nt" and not odd and lda % 2:
        lda += 1
    if op == "nt" and not odd and ldb % 2:
        ldb += 1
    if op == "gram":
        ldb = lda
    return dict(lda=lda, ldb=ldb, ldc=(m if op == "gram" else n) + 3, a_off=3 if odd else 2, b_off=5 if odd else 4, c_off=7)


def test_route_table_covers_every_route_and_reducer():
    """Pure Python: the cases above take every route x reducer of the four dispatchers (and both kmin branches)."""
    seen = set()
    for c in ROUTE_CASES:
        seen |= tags(route_of(c))
    assert REQUIRED <= seen, f"routes no case takes: {sorted(REQUIRED - seen)}"
    assert {route_of(c)["route"] for c in EDGE_CASES} >= {"noop", "nt_general_unaligned", "gram_lower", "nn_general"}


# =====================================================================================================================
# exact cases
# =====================================================================================================================
def _embed(M, off, ld, fill, tail=37):
    rows, cols = M.shape
    buf = np.full(off + rows * ld + tail, fill)
    buf[off:off + rows * ld].reshape(rows, ld)[:, :cols] = M
    return buf


def _window(buf, off, ld, rows, cols):
    return buf[off:off + rows * ld].reshape(rows, ld)[:, :cols]


def run_case(ctx, case, A, B, C0, beta, alpha=ALPHA):
    """Enqueue the case on the device with the layout(case) embedding; returns (C window, bits outside the window intact)."""
    op, m, n, k, _ = case
    L = layout(case)
    Ab = _embed(A, L["a_off"], L["lda"], np.nan)
    Bb = _embed(B, L["b_off"], L["ldb"], np.nan) if op != "gram" else None
    cn = m if op == "gram" else n
    Cb = _embed(C0, L["c_off"], L["ldc"], SENTINEL)
    Ad, Cd = ctx.upload(Ab), ctx.upload(Cb)
    if op == "nt":
        Bd = ctx.upload(Bb)
        ctx.gemm_nt(m, n, k, Ad, L["a_off"], L["lda"], Bd, L["b_off"], L["ldb"], Cd, L["c_off"], L["ldc"], alpha=alpha, beta=beta)
    elif op == "nn":
        Bd = ctx.upload(Bb)
        ctx.gemm_nn(m, n, k, Ad, L["a_off"], L["lda"], Bd, L["b_off"], L["ldb"], Cd, L["c_off"], L["ldc"], alpha=alpha, beta=beta)
    else:
        ctx.gram(m, k, Ad, L["a_off"], L["lda"], Cd, L["c_off"], L["ldc"])
    got = Cd.download()
    mask = np.ones(got.size, dtype=bool)
    _window(mask, L["c_off"], L["ldc"], m, cn)[...] = False
    guard_ok = np.array_equal(got[mask].view(np.uint64), Cb[mask].view(np.uint64))
    return _window(got, L["c_off"], L["ldc"], m, cn).copy(), guard_ok


def exact_operands(case, beta, seed):
    op, m, n, k, _ = case
    rng = np.random.default_rng(seed)
    A = rng.integers(-8, 9, size=(m, k)).astype(np.float64)
    if op == "nt":
        B = rng.integers(-8, 9, size=(n, k)).astype(np.float64)
        prod = A @ B.T
    elif op == "nn":
        B = rng.integers(-8, 9, size=(k, n)).astype(np.float64)
        prod = A @ B
    else:
        B, prod = None, A @ A.T
    cn = m if op == "gram" else n
    if op == "gram":   # (rom_gram: C = A A^T, both triangles prefilled with NaN)
        return A, B, np.full((m, cn), np.nan), prod
    if beta == 0.0:
        return A, B, np.full((m, cn), np.nan), ALPHA * prod
    C0 = rng.integers(-8, 9, size=(m, cn)).astype(np.float64)
    return A, B, C0, ALPHA * prod + beta * C0


def check_exact(ctx, case, beta, seed=0):
    """Zero-tolerance check of one case; returns a message or None."""
    A, B, C0, ref = exact_operands(case, beta, seed)
    got, guard_ok = run_case(ctx, case, A, B, C0, beta)
    if not guard_ok:
        return f"{case}: an entry of C outside the m x n window changed"
    if not np.isfinite(got).all():
        return f"{case}: non-finite entries in the window ({int((~np.isfinite(got)).sum())})"
    if not np.array_equal(got, ref):
        bad = np.argwhere(got != ref)
        return f"{case}: {len(bad)} entries differ from the exact product, first at {tuple(bad[0])}"
    if case[0] == "gram" and not np.array_equal(got, got.T):
        return f"{case}: Gram matrix not exactly symmetric"
    return None


@pytest.fixture(scope="module")
def ctx():
    from romhighcontrast_amd import _ffi
    return _ffi.get_context()


def case_id(c):
    return "-".join(map(str, c))


def case_seed(c):
    return c[1] * 7919 + c[2] * 131 + c[3] + (1 if c[4] == "un" else 0)


EXACT_PARAMS = [(c, b) for c in ROUTE_CASES + EDGE_CASES for b in ((BETA,) if c[0] == "gram" else (BETA, 0.0))]


@pytest.mark.parametrize("case,beta", EXACT_PARAMS, ids=[f"{case_id(c)}-b{b}" for c, b in EXACT_PARAMS])
def test_exact_products_on_every_route(ctx, case, beta):
    """Integer operands: the result must EQUAL the exact product on every route and reducer, C outside its window keeps its
    sentinel bits, NaN in the window is not read when beta == 0, k == 0 gives beta C (a Gram matrix of zeros), m or n == 0
    leaves C alone.  (rom_gram has no beta: its cases run once, with all of C prefilled with NaN.)"""
    msg = check_exact(ctx, case, beta, seed=case_seed(case))
    assert msg is None, f"{msg}  route {route_of(case)}"


# =====================================================================================================================
# rounding cases: the rigorous bound against a long-double product; same bits twice and over a poisoned scratch area
# =====================================================================================================================
ROUND_CASES = [("nt", 16, 256, 8192, "un"), ("nt", 1, 257, 8192, "un"), ("nt", 33, 513, 2049, "un"), ("nt", 17, 300, 20593, "un"),
               ("nt", 256, 16, 8192, "un"),
               ("nt", 300, 1, 8192, "al"), ("nt", 65, 127, 1000, "un"), ("nt", 129, 65, 1100, "al"), ("nt", 63, 64, 2047, "al"),
               ("nt", 64, 64, 2049, "un"), ("nt", 129, 129, 4500, "al"), ("gram", 63, 63, 2049, "al"),
               ("gram", 127, 127, 4096, "un"), ("gram", 200, 200, 1100, "un"), ("gram", 70, 70, 1000, "al"),
               ("nn", 24, 272, 1024, "al"), ("nn", 129, 63, 300, "un"), ("nn", 17, 1029, 129, "un"), ("nn", 130, 1029, 16, "un")]


def _scaled(rng, rows, cols, col_scale):
    return 10.0 ** rng.uniform(-8, 8, size=(rows, 1)) * rng.standard_normal((rows, cols)) * col_scale[None, :]


@pytest.mark.parametrize("case", ROUND_CASES, ids=case_id)
def test_rounding_bound_and_determinism(ctx, case, monkeypatch):
    """Normal operands with row and column scales over 10^+-8: |C - ref| <= gamma_(k + s + 3) |alpha| |A||B| + 2 u |beta C|
    entrywise against the long-double product of the same fp64 inputs (s: the K splits of the route).  A split route gives
    the same bits on a second run, and again with the scratch area filled with NaN bytes first (ROMHC_POISON_WS)."""
    op, m, n, k, _ = case
    r = route_of(case)
    rng = np.random.default_rng(case_seed(case))
    ks = 10.0 ** rng.uniform(-4, 4, size=k)
    A = _scaled(rng, m, k, ks)
    if op == "gram":
        alpha, beta, B, C0 = 1.0, 0.0, None, np.zeros((m, m))
        ref = A.astype(np.longdouble) @ A.T.astype(np.longdouble)
        absprod = np.abs(A) @ np.abs(A.T)
    else:
        alpha, beta = ALPHA, BETA
        if op == "nt":
            B = _scaled(rng, n, k, 1.0 / ks)
            Bt = B.T
        else:
            B = (10.0 ** rng.uniform(-8, 8, size=(k, 1))) * rng.standard_normal((k, n)) / ks[:, None] * 10.0 ** rng.uniform(-8, 8, size=n)
            Bt = B
        absprod = np.abs(A) @ np.abs(Bt)
        C0 = rng.standard_normal((m, n)) * absprod * 10.0 ** rng.uniform(-3, 1, size=(m, n))   # (beta C must not hide the product)
        ref = alpha * (A.astype(np.longdouble) @ Bt.astype(np.longdouble)) + beta * C0.astype(np.longdouble)
    s = r["splits"] or 64   # (k_gram128: at most 64 splits)
    g = (k + s + 3) * U / (1 - (k + s + 3) * U)
    bound = g * abs(alpha) * absprod * (1 + 1e-12) + 2 * U * np.abs(beta * C0)
    runs = []
    for poison in (False, False, True):
        if poison:
            monkeypatch.setenv("ROMHC_POISON_WS", "1")
        got, guard_ok = run_case(ctx, case, A, B, C0, beta, alpha=alpha)
        assert guard_ok, f"{case}: C changed outside its window"
        runs.append(got)
    monkeypatch.delenv("ROMHC_POISON_WS", raising=False)
    got = runs[0]
    assert np.isfinite(got).all()
    err = np.abs(got.astype(np.longdouble) - ref).astype(np.float64)
    ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))
    observed(f"dense {case_id(case)} ({r['route']}/{r['reducer']}): |C - ref| / rigorous bound", ratio, 1.0)
    for i, x in enumerate(runs[1:], 1):
        assert np.array_equal(x.view(np.uint64), got.view(np.uint64)), \
            f"{case}: run {i} {'(poisoned scratch) ' if i == 2 else ''}differs in its bits from the first"
    if op == "gram":
        assert np.array_equal(got, got.T)


# =====================================================================================================================
# the route witness and the forced-general variant (child processes: the switches are read once per process)
# =====================================================================================================================
def _child(job, env_add, timeout):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("ROMHC_PROF_DETAIL", "ROMHC_NO_THIN_GEMM", "ROMHC_POISON_WS")}
    env.update(env_add)
    r = subprocess.run([sys.executable, os.path.join(root, "tests", "dense_routes_child.py"), job], env=env, cwd=root,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=timeout)
    out = r.stdout.decode(errors="replace")
    assert r.returncode == 0 and out.rstrip().endswith("OK"), f"exit {r.returncode}\n{out[-4000:]}"
    return out


def test_profile_names_confirm_every_route():
    """ROMHC_PROF_DETAIL=1 with profiling on: every ROUTE_CASES product leaves the kernel names its route predicts
    (_thin_ with the split count, gemm_nn_thin_, _s<splits>, splitk_reduce exactly when it splits, gram128, mirror_lower)."""
    _child("routes", {"ROMHC_PROF_DETAIL": "1"}, 300)


def test_general_engine_exact_and_pod_with_ahead_product():
    """ROMHC_NO_THIN_GEMM=1 (profiling off): the exact cases again on the 64 x 64 engines, and a rom_pod of a 64 MB block whose
    second sketch pass is started ahead on the auxiliary stream with a SPLIT-K product -- it must not take the context's
    scratch area there (which the main stream's kernels use at the same time)."""
    _child("general", {"ROMHC_NO_THIN_GEMM": "1"}, 600)


# =====================================================================================================================
# row helpers, norms, orthonormalisation, buffer bits
# =====================================================================================================================
@pytest.mark.parametrize("dim", [1, 15, 16, 17, 72, 225, 241, 4097, 4353])
def test_rows_sign_flip_exact(ctx, dim):
    """svd_flip: every row times the sign of its entry of largest magnitude (the FIRST on ties, as np.argmax), bit for bit;
    dims with empty segments of the 16-way split (17, 72, 225), ties across segments and 256 columns apart inside one,
    an all-zero row, a negative maximum in the last non-empty segment; the rows end at the end of the buffer."""
    rng = np.random.default_rng(dim)
    row0, rows = 2, 9
    Y = rng.uniform(-1, 1, size=(row0 + rows, dim))
    per = _ceil(dim, 16)
    R = Y[row0:]
    if dim > per:                       # equal magnitude, opposite sign, different segments: the first wins
        R[0, per - 1], R[0, per] = -9.0, 9.0
        R[1, per - 1], R[1, per] = 9.0, -9.0
    if per > 256:                       # the same 256 columns apart within one segment (one thread's stride)
        R[2, 3], R[2, 3 + 256] = -9.0, 9.0
        R[3, per + 5], R[3, per + 5 + 256] = 9.0, -9.0
    R[4] = 0.0                          # no flip, no NaN
    last = (dim - 1) // per             # last non-empty segment
    R[5, last * per + (dim - 1 - last * per) // 2] = -9.0
    R[6, dim - 1] = -9.0
    Yd = ctx.upload(Y)
    ctx.rows_sign_flip(Yd, rows, dim, row0=row0)
    got = Yd.download(shape=Y.shape)
    piv = np.argmax(np.abs(R), axis=1)
    sg = np.where(R[np.arange(rows), piv] < 0, -1.0, 1.0)
    ref = Y.copy()
    ref[row0:] = R * sg[:, None]
    assert np.array_equal(got.view(np.uint64), ref.view(np.uint64)), np.argwhere(got != ref)[:5]


@pytest.mark.parametrize("M", [1, 15, 16, 17])
@pytest.mark.parametrize("dim", [300, 2049])
def test_center_rows_and_rows_scale(ctx, M, dim):
    """Column means of rows [row0, row0 + M) (16 row slabs: M around CENTER_SLABS) against a long-double mean, to an
    ulp-scale bound; the rows outside the range keep their bits; rows_scale on a sub-range is one exact multiplication."""
    rng = np.random.default_rng(M * 1000 + dim)
    row0 = 3
    X = rng.standard_normal((row0 + M + 2, dim)) * 10.0 ** rng.uniform(-3, 3, size=dim) + 5.0
    Xd, mean = ctx.upload(X), ctx.alloc(dim)
    ctx.center_rows(Xd, M, dim, mean, row0=row0)
    got = Xd.download(shape=X.shape)
    blk = X[row0:row0 + M]
    ref_mean = blk.astype(np.longdouble).mean(axis=0)
    colabs = np.abs(blk).mean(axis=0)
    observed(f"center_rows M={M} dim={dim}: |mean - long double| / ((M + 2) u mean|x|)",
             np.abs(mean.download(dim) - ref_mean).astype(np.float64) / ((M + 2) * U * colabs), 1.0)
    cen = (blk.astype(np.longdouble) - ref_mean).astype(np.float64)
    observed(f"center_rows M={M} dim={dim}: centred rows, |x - ref| / ((M + 3) u (|x| + mean|x|))",
             np.abs(got[row0:row0 + M] - cen) / ((M + 3) * U * (np.abs(blk) + colabs)), 1.0)
    outside = np.r_[0:row0, row0 + M:X.shape[0]]
    assert np.array_equal(got[outside].view(np.uint64), X[outside].view(np.uint64))
    fac = rng.uniform(-3, 3, size=M)
    fac[0] = -0.0
    Xd = ctx.upload(X)
    ctx.rows_scale(Xd, M, dim, fac, row0=row0)
    got = Xd.download(shape=X.shape)
    ref = X.copy()
    ref[row0:row0 + M] *= fac[:, None]
    assert np.array_equal(got.view(np.uint64), ref.view(np.uint64))


@pytest.mark.parametrize("dim", [2047, 2048, 2049, 4097])
@pytest.mark.parametrize("K", [1, 300])
def test_l2norm_vs_long_double(ctx, dim, K):
    """Row 2-norms around the 2048-column block of k_sq_partial, against long double: (dim + 8) u / 2 relative plus the
    square root's rounding."""
    rng = np.random.default_rng(dim + K)
    X = rng.standard_normal((K + 1, dim)) * 10.0 ** rng.uniform(-5, 5, size=(K + 1, 1))
    got = ctx.l2norm(ctx.upload(X), 1, K, dim)
    ref = np.sqrt((X[1:].astype(np.longdouble) ** 2).sum(axis=1))
    observed(f"l2norm dim={dim} K={K}: relative error / ((dim + 8) u)",
             np.abs(got - ref).astype(np.float64) / ref.astype(np.float64) / ((dim + 8) * U), 1.0)


@pytest.mark.parametrize("blocks,N", [((2, 2), 16), ((2, 3), 100), ((3, 1), 90)])
def test_h10norm_of_a_difference(ctx, blocks, N):
    """rom_h10norm with a second operand (H10norm_diff): V = U + 1e-9 W, rows at different offsets in U and V; the reference
    is the oracle's norm of the fp64 difference U - V (exact: Sterbenz), and the accuracy is relative to ||U - V||, which a
    |u|^2 - 2 <u, v> + |v|^2 form would miss by eight orders."""
    from oracle import rom_oracle as ro
    from romhighcontrast_amd import _ffi
    g = ro.Geometry(blocks, N)
    fem = _ffi.Fem(ctx, blocks[0], blocks[1], N)
    rng = np.random.default_rng(N)
    K, u0, v0 = 3, 1, 2
    Uh = rng.standard_normal((u0 + K, g.dim)) + 2.0
    Vh = rng.standard_normal((v0 + K, g.dim))
    Vh[v0:] = Uh[u0:] + 1e-9 * rng.standard_normal((K, g.dim))
    D = Uh[u0:] - Vh[v0:]
    got = fem.h10norm(ctx.upload(Uh), K, u_row0=u0, V=ctx.upload(Vh), v_row0=v0)
    ref = ro.H10norm(g, D)
    observed(f"h10norm(U, V) {blocks} N={N}: relative to ||U - V||", np.abs(got - ref) / ref, 1e-12)


@pytest.mark.parametrize("n", [1, 17, 64, 200])
def test_symmetric_orthonormalize_is_the_polar_factor(ctx, n):
    """Loewdin orthonormalisation of orthonormal rows perturbed by 1e-6: orthonormal (1e-14, 4 n u for n > 22) and equal to
    the polar factor U W^T of the input's SVD (the closest orthonormal set) to 1e-12."""
    dim, v0 = 777, 2
    rng = np.random.default_rng(n)
    Q, _ = np.linalg.qr(rng.standard_normal((dim, n)))
    V0 = Q.T + 1e-6 * rng.standard_normal((n, dim))
    buf = np.vstack([rng.standard_normal((v0, dim)), V0, rng.standard_normal((1, dim))])
    Vd = ctx.upload(buf)
    ctx.symmetric_orthonormalize(Vd, n, dim, v_row0=v0)
    out = Vd.download(shape=buf.shape)
    V = out[v0:v0 + n]
    Us, _, Wt = np.linalg.svd(V0, full_matrices=False)
    # (1e-14, or 4 n u for the larger sets: the Gram matrix of n rows carries O(n u) of rounding in fp64)
    observed(f"symmetric_orthonormalize n={n}: |V V^T - I|", np.abs(V @ V.T - np.eye(n)), max(1e-14, 4 * n * U))
    observed(f"symmetric_orthonormalize n={n}: |V - polar factor|", np.abs(V - Us @ Wt), 1e-12)
    keep = np.r_[0:v0, v0 + n:buf.shape[0]]
    assert np.array_equal(out[keep].view(np.uint64), buf[keep].view(np.uint64))


@pytest.mark.parametrize("dim,found,rest", [(300, 20, 30), (64, 20, 44), (50, 0, 7)])
def test_complete_orthonormal(ctx, dim, found, rest):
    """New rows orthonormal and orthogonal to the given ones (1e-14; 1e-13 when they fill the space), the given rows
    bit-identical, two calls the same bits; found + rest == dim works, found + rest > dim is refused."""
    from romhighcontrast_amd import _ffi
    rng = np.random.default_rng(dim + found)
    v0 = 1
    Q, _ = np.linalg.qr(rng.standard_normal((dim, max(found, 1))))
    buf = np.full((v0 + found + rest + 1, dim), np.nan)
    buf[v0:v0 + found] = Q.T[:found]
    outs = []
    for _ in range(2):
        Vd = ctx.upload(buf)
        ctx.complete_orthonormal(Vd, found, rest, dim, v_row0=v0)
        outs.append(Vd.download(shape=buf.shape))
    out = outs[0]
    assert np.array_equal(outs[1].view(np.uint64), out.view(np.uint64))
    keep = np.r_[0:v0 + found, v0 + found + rest:buf.shape[0]]
    assert np.array_equal(out[keep].view(np.uint64), buf[keep].view(np.uint64))
    W = out[v0:v0 + found + rest]
    assert np.isfinite(W).all()
    # (a completion that fills the whole space: its last rows are what is left of random vectors after all the other
    # directions are removed -- a small remainder, renormalised: 1e-13 there)
    observed(f"complete_orthonormal dim={dim} {found}+{rest}: |W W^T - I|", np.abs(W @ W.T - np.eye(found + rest)),
             1e-13 if found + rest == dim else 1e-14)
    with pytest.raises(_ffi.RomLibraryError, match="more rows than the space has dimensions"):
        ctx.complete_orthonormal(ctx.alloc((dim + 1) * dim).fill(0.0), found, dim - found + 1, dim)


@pytest.mark.parametrize("n", [1, 255, 257, 1000, 65537])
def test_buf_equal_and_fill_bits(ctx, n):
    """rom_buf_equal compares storage: +0.0 against -0.0 and NaNs of different payloads differ, one differing element is
    found at the first and at the last index; rom_buf_fill(-0.0) stores -0.0 (not the memset's +0.0)."""
    rng = np.random.default_rng(n)
    x = rng.standard_normal(n)
    a = ctx.upload(x)
    assert a.same_bits_as(ctx.upload(x), n)
    for i in (0, n - 1):
        for v in (np.nextafter(x[i], np.inf), -x[i]):
            y = x.copy()
            y[i] = v
            assert not a.same_bits_as(ctx.upload(y), n), (i, v)
    z = np.zeros(n)
    assert not ctx.upload(z).same_bits_as(ctx.upload(-z), n)
    nan1 = np.full(n, np.nan)
    nan2 = nan1.copy()
    nan2.view(np.uint64)[n - 1] |= 1
    assert not ctx.upload(nan1).same_bits_as(ctx.upload(nan2), n)
    assert ctx.upload(nan2).same_bits_as(ctx.upload(nan2), n)
    f = ctx.alloc(n + 2).fill(7.0)
    f.fill(-0.0, offset=1, n=n)
    got = f.download()
    assert np.array_equal(got[1:n + 1].view(np.uint64), np.full(n, 0x8000000000000000, dtype=np.uint64))
    assert got[0] == 7.0 and got[n + 1] == 7.0
    assert f.same_bits_as(ctx.upload(np.r_[7.0, -z, 7.0]), n + 2)
    f.fill(0.0, offset=1, n=n)
    assert np.array_equal(f.download()[1:n + 1].view(np.uint64), np.zeros(n, dtype=np.uint64))
