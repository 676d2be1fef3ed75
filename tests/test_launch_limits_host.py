"""CPU tests of tests/launch_limits_truth.py and of the prototypes of the binding.

* The generators: on every block the GPU tests build, item i differs from items i - 1, i - 65535 and i - 65536 (and from the
  item a lost offset of the nearest-row scan or of the right factor of the sine transform would read).
* The scaled-periodic truth equals the long-double truth computed directly, bit for bit, on a few hundred rows.
* Planted mutations: for each checker an output that is correct except that everything from item 65535 on was computed from
  the first launch's input (offset lost), and one that is one item off; each also on the last row alone.  Every checker must
  reject every one of them -- and accept the unmutated output.
* include/romhc.h against _ffi.PROTOTYPES, argument by argument and in the return type.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

from oracle import rom_oracle as ro
import h10_truth as ht
import launch_limits_truth as lt

LD = np.longdouble
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIRS = [(0, 1), (-1, 0), (-1, 2)]


def quiet(name, value, bound, *, detail=""):
    """conftest.observed without the record: the planted failures do not belong in the terminal summary."""
    v = float(np.max(value)) if np.size(value) else 0.0
    assert v <= bound, f"{name}: observed {v:.3e} > bound {bound:.3e} {detail}"


def _grid():
    return ht.grid(*lt.GEOM)


# ---- generators ----------------------------------------------------------------------------------------------------------
def _differs(X, shift):
    return not np.any(np.all(X[shift:] == X[:-shift], axis=1))


def _blocks():
    gr = _grid()
    out = {"transform": lt.base_rows(gr.dim, lt.TRANSFORM_SEED)}
    for dim in (3, 17):
        out[f"scale{dim}"] = lt.base_rows(dim, seed=dim)
        out[f"factors{dim}"] = lt.base_rows(1, seed=100 + dim, cols_scale=False) * 3.0
        out[f"sign{dim}"] = lt.sign_base(dim, seed=7 * dim)
    for r in (1, 5):
        out[f"queries{r}"] = lt.nearest_case(r)[1]
    return out


@pytest.mark.parametrize("name", sorted(_blocks()))
def test_an_item_differs_from_the_items_a_lost_offset_would_read(name):
    base = _blocks()[name]
    X = lt.rows(base, lt.K_BATCH + lt.CYCLE)
    for shift in (1, lt.LIMIT, lt.LIMIT + 1):
        assert _differs(X, shift), (name, shift)
    assert np.isfinite(X).all()
    # the block is what the docstring says it is
    i = np.array([0, 1, 66, 67, 870, 871, 65535, 65536])
    assert np.array_equal(X[i], base[i % 67] * (2.0 ** ((i % 13) - 6))[:, None])
    assert lt.LIMIT % lt.PERIOD == 9 and (lt.LIMIT + 1) % lt.PERIOD == 10 and lt.named_rows(lt.K_BATCH) == [0, 65534, 65535, 65536]


def test_plainly_periodic_blocks_differ_too():
    gr = _grid()
    for U in (lt.greedy_inputs(gr.dim, 1)[0], lt.curves_inputs(lt.GEOM[0], gr.dim, 2)[0].reshape(lt.PERIOD, -1)):
        X = lt.rows(U, lt.K_BATCH, scaled=False)
        for shift in (1, lt.LIMIT, lt.LIMIT + 1):
            assert _differs(X, shift)


def test_queries_past_the_split_of_the_exhaustive_scan_differ():
    for r in (1, 5):
        base = lt.nearest_case(r)[1]
        tail = lt.rows(base, lt.NN_K, lo=lt.NN_SPLIT - 16)
        for shift in (lt.NN_SPLIT, lt.NN_SPLIT - 1, 16, 1):      # offset lost; one query / one block of 16 off
            other = lt.rows(base, lt.NN_K - shift, lo=lt.NN_SPLIT - 16 - shift)
            assert not np.any(np.all(tail == other, axis=1)), (r, shift)


def test_the_right_factor_split_reads_other_data_with_a_lost_offset():
    gr = _grid()
    base = lt.base_rows(gr.dim, lt.TRANSFORM_SEED)
    K = lt.right_count(gr.nr)
    assert K * gr.nr > lt.RIGHT_ROWS and (K - 71) * gr.nr < lt.RIGHT_ROWS and K * gr.dim * 8 < 128 << 20
    assert lt.flat_shift_differs(base, K, gr.nc, lt.RIGHT_ROWS)
    assert lt.flat_shift_differs(base, K, gr.nc, lt.RIGHT_ROWS - 1)     # (one row of the product off)
    # every split of the left factor inside that block, too
    for j in range(1, K // lt.LIMIT + 1):
        assert (j * lt.LIMIT) % lt.PERIOD != 0
    # and the helper itself sees a block that does repeat at the split
    assert not lt.flat_shift_differs(np.ones((lt.PERIOD, 4)), 2 * lt.CYCLE + 3, 4, lt.CYCLE)


def test_rows_past_the_row_block_of_the_dense_products_differ():
    """The one-column operand of the GEMM case: row 65535 * 64 differs from row 0 (offset lost) and from the row before it, and
    the checker refuses both on that last row."""
    m = lt.RIGHT_ROWS + 1
    A = lt.rows(lt.base_rows(1, seed=31), m)
    assert lt.RIGHT_ROWS % lt.PERIOD != 0 and A[m - 1, 0] != A[0, 0] and A[m - 1, 0] != A[m - 2, 0]
    want = A * (1.0 / 3.0)
    lt.check_exact("good", want.copy(), want)
    for shift in (lt.RIGHT_ROWS, 1):
        with pytest.raises(AssertionError, match="rows differ"):
            lt.check_exact("bad", lt.lost_offset(want, lt.RIGHT_ROWS, shift), want)


# ---- the scaled truth is the truth ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pre,post", PAIRS)
def test_scaled_transform_truth_is_the_direct_long_double_truth(pre, post):
    gr = _grid()
    base = lt.base_rows(gr.dim, lt.TRANSFORM_SEED)
    tt = lt.TransformTruth(gr, base, pre, post)
    K = 300
    X = lt.rows(base, K)
    direct = gr.transform(X, pre, post)
    idx = np.arange(K)
    s = lt.pow2(idx).astype(LD)[:, None]
    tiled = (tt.hi[idx % lt.PERIOD].astype(LD) + tt.lo[idx % lt.PERIOD].astype(LD)) * s
    assert np.array_equal(tiled, direct)
    assert np.array_equal(gr.transform_bound(X, pre, post), tt.bound[idx % lt.PERIOD] * s[:, 0].astype(np.float64))
    # the fp64 restatement is inside the bound (so is what the mutation tests start from), a row of zeros is not
    out = tt.fp64_output(K)
    assert tt.ratios(out).max() < 1.0
    assert np.array_equal(out, np.asarray(gr.transform(X, pre, post, ld=False), dtype=np.float64))
    assert tt.ratios(np.zeros_like(out)).min() > 1e6
    assert np.array_equal(tt.ratios(out[100:], lo=100), tt.ratios(out)[100:])


def test_expected_rows_of_scale_and_sign_flip():
    for dim in (3, 17):
        X, fac, want = lt.scale_case(400, dim)
        exact = X.astype(LD) * fac.astype(LD)[:, None]
        assert np.all(np.abs(want.astype(LD) - exact) <= LD(2.0 ** -53) * np.abs(exact) * (1 + LD(2.0) ** -9)), "one rounding"
        assert np.array_equal(want, lt.rows(lt.base_rows(dim, seed=dim), 400) * fac[:, None])
        S, flipped = lt.sign_case(400, dim)
        piv = np.argmax(np.abs(flipped), axis=1)
        assert np.all(flipped[np.arange(400), piv] >= 0) and np.array_equal(np.abs(flipped), np.abs(S))
        assert np.all(flipped[0::67][:, 0] == 9 * lt.pow2(np.arange(0, 400, 67)))      # the tie: the first entry decides
        assert np.all(flipped[1::67] == S[1::67]) and np.all(flipped[2::67] == 0) and np.all(flipped[3::67][:, -1] > 0)
        assert not np.array_equal(flipped, S)


# ---- planted mutations ------------------------------------------------------------------------------------------------------
def _mutations(out, split, one_item=1):
    """(label, mutated output): offset lost / one item off, on everything from the split on and on the last row alone."""
    for label, shift in (("offset lost", split), ("one item off", one_item)):
        for last_only in (False, True):
            yield f"{label}{', last row only' if last_only else ''}", lt.lost_offset(out, split, shift, last_only)


@pytest.mark.parametrize("pre,post", PAIRS)
def test_transform_checker_rejects_a_lost_offset_of_the_batch_split(pre, post):
    gr = _grid()
    tt = lt.TransformTruth(gr, lt.base_rows(gr.dim, lt.TRANSFORM_SEED), pre, post)
    out = tt.fp64_output(lt.K_BATCH)
    lt.check_transform("good", tt, out, quiet)
    for label, bad in _mutations(out, lt.LIMIT):
        with pytest.raises(AssertionError, match="6553[56]"):
            lt.check_transform(label, tt, bad, quiet)
    nan = out.copy()
    nan[-1, 0] = np.nan
    with pytest.raises(AssertionError):
        lt.check_transform("a NaN", tt, nan, quiet)


@pytest.mark.parametrize("pre,post", [(0, 1), (-1, 0)])
def test_transform_checker_rejects_a_lost_offset_of_the_right_factor(pre, post):
    """The mutation at flat offset 65535 * 64 * nc of the right factor's operand: the rows of the product from there on come
    from the rows the first launch read (or from one row before their own)."""
    gr = _grid()
    base = lt.base_rows(gr.dim, lt.TRANSFORM_SEED)
    tt = lt.TransformTruth(gr, base, pre, post)
    K = lt.right_count(gr.nr)
    out = tt.fp64_output(K)
    lt.check_transform("good", tt, out, quiet)
    it0 = lt.RIGHT_ROWS // gr.nr                    # the first snapshot the second launch touches
    X = lt.rows(base, K, lo=it0)
    n2 = K * gr.nr - lt.RIGHT_ROWS
    for label, shift in (("offset lost", lt.RIGHT_ROWS), ("one row off", 1)):
        lo = (lt.RIGHT_ROWS - shift) // gr.nr
        src = lt.rows(base, K, lo=lo).reshape(-1, gr.nc)[(lt.RIGHT_ROWS - shift) - lo * gr.nr:][:n2]
        for last_only in (False, True):
            Xm = X.copy().reshape(-1, gr.nc)
            at = lt.RIGHT_ROWS - it0 * gr.nr
            if last_only:
                Xm[-1] = src[-1]
            else:
                Xm[at:] = src
            # (the right factor acts on the rows of Lambda^(pre/2) o X when pre != 0; a row of X in the wrong place is
            # wrong there as well, and the restatement below is exact about which rows are touched)
            bad = out.copy()
            bad[it0:] = np.asarray(gr.transform(Xm.reshape(-1, gr.dim), pre, post, ld=False), dtype=np.float64)
            assert not np.array_equal(bad, out)
            with pytest.raises(AssertionError):
                lt.check_transform(f"{label}{', last row only' if last_only else ''}", tt, bad, quiet)


@pytest.mark.parametrize("dim", [3, 17])
def test_exact_checker_rejects_a_lost_offset(dim):
    for X, want in (lt.scale_case(lt.K_BATCH, dim)[::2], lt.sign_case(lt.K_BATCH, dim)):
        lt.check_exact("good", want.copy(), want)
        for label, bad in _mutations(want, lt.LIMIT):
            with pytest.raises(AssertionError, match="rows differ"):
                lt.check_exact(label, bad, want)
    # a factor read with a lost offset on rows that are in the right place
    X, fac, want = lt.scale_case(lt.K_BATCH, dim)
    bad = want.copy()
    bad[lt.LIMIT:] = X[lt.LIMIT:] * fac[:lt.K_BATCH - lt.LIMIT, None]
    with pytest.raises(AssertionError, match="rows differ"):
        lt.check_exact("factors from the first launch", bad, want)
    z = want.copy()
    z[5, 1] = -z[5, 1] if z[5, 1] != 0 else 1.0
    with pytest.raises(AssertionError, match="rows differ"):
        lt.check_exact("one sign", z, want)


@pytest.mark.parametrize("r,t", [(1, 1), (5, 3)])
def test_nearest_checker_rejects_a_lost_offset(r, t):
    import nearest_truth as nt
    Q, base = lt.nearest_case(r)
    idx_c, d2_c = nt.brute_force(lt.rows(base, lt.CYCLE), Q, t)
    cyc = np.arange(lt.NN_K) % lt.CYCLE
    idx, d2 = idx_c[cyc], d2_c[cyc]
    lt.check_nearest("good", base, Q, idx, d2, t)
    for one in (1, 16):
        for label, bad_i in _mutations(idx, lt.NN_SPLIT, one):
            bad_d = dict(_mutations(d2, lt.NN_SPLIT, one))[label]
            assert not np.array_equal(bad_d, d2)
            with pytest.raises(AssertionError):
                lt.check_nearest(label, base, Q, bad_i, bad_d, t)
    assert lt.nearest_windows(lt.NN_K)[-1][1] == lt.NN_K and any(lo < lt.NN_SPLIT < hi for lo, hi in lt.nearest_windows(lt.NN_K))


@pytest.mark.parametrize("N,with_a", [(2, True), (9, True), (9, False)])
def test_curves_checker_rejects_a_lost_offset(N, with_a):
    blocks, Nm = lt.GEOM
    g = ro.Geometry(blocks, Nm)
    a, Cb = lt.curves_inputs(blocks, g.dim, N)
    U = ro.generate_solutions(g, a, "lsqsparse")
    tr = lt.CurvesTruth(g, U, Cb, a if with_a else None, 10.0 ** lt.CURVES_DECADES)
    M = lt.CURVES_M
    b = np.arange(M) % lt.PERIOD
    proj, P = np.sqrt(tr.proj2[:, b]), tr.P[b]
    galc = np.sqrt(tr.gal2[:, b]) if with_a else None
    lt.check_curves("good", tr, proj, galc, P, quiet)
    for label, bad in _mutations(proj.T, lt.LIMIT):
        with pytest.raises(AssertionError):
            lt.check_curves(label, tr, np.ascontiguousarray(bad.T), galc, P, quiet)
    for label, bad in _mutations(P, lt.LIMIT):
        with pytest.raises(AssertionError):
            lt.check_curves(label, tr, proj, galc, bad, quiet)
    if with_a:
        for label, bad in _mutations(galc.T, lt.LIMIT):
            with pytest.raises(AssertionError):
                lt.check_curves(label, tr, proj, np.ascontiguousarray(bad.T), P, quiet)
        # identical snapshots, different bits: inside every bound, still refused
        g2 = galc.copy()
        g2[1, -1] = np.nextafter(g2[1, -1], np.inf)
        with pytest.raises(AssertionError, match="rows differ"):
            lt.check_curves("one ulp on the last snapshot", tr, proj, g2, P, quiet)


def test_greedy_truth_decides_its_picks():
    """The 80-bit greedy of the distinct rows has margins far above the bound model, so `picks equal` is a fair demand; the
    checker refuses another pick and a copy of the right row at a higher index."""
    blocks, Nm = lt.GEOM
    g = ro.Geometry(blocks, Nm)
    U, h1 = lt.greedy_inputs(g.dim, 1)
    truth = lt.greedy_truth(g, U, h1, lt.GREEDY_N)
    picks, top, margin, bounds = truth
    assert len(set(picks)) == lt.GREEDY_N and np.all(margin > 1e6 * bounds) and np.all(np.diff(top) < 0)
    lt.check_greedy("good", truth, picks, top, quiet)
    for bad in ([picks[0], picks[1], picks[2] + lt.PERIOD], [picks[0] + lt.LIMIT - 9, picks[1], picks[2]], picks[::-1]):
        with pytest.raises(AssertionError):
            lt.check_greedy("bad", truth, bad, top, quiet)
    with pytest.raises(AssertionError):
        lt.check_greedy("curve", truth, picks, top * (1 + 1e-9), quiet)


# ---- include/romhc.h against _ffi.PROTOTYPES ------------------------------------------------------------------------------------
SCALARS = {"int": C.c_int, "int32_t": C.c_int32, "int64_t": C.c_int64, "size_t": C.c_size_t, "double": C.c_double, "long": C.c_long}
HANDLES = {"rom_ctx", "rom_buf", "rom_fem", "rom_resid", "rom_poly", "rom_mlp", "rom_tree"}


def header_prototypes():
    """name -> (return type, [argument types]) as C type strings without names and qualifiers, e.g. 'int64_t', 'rom_buf*'."""
    from test_host_logic import header_symbols
    src = open(os.path.join(ROOT, "include", "romhc.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    src = re.sub(r"^\s*#.*$", "", src, flags=re.M)

    def ctype(text, named):
        toks = re.findall(r"[A-Za-z_][A-Za-z0-9_]*|\*", text)
        toks = [t for t in toks if t not in ("const", "struct")]
        if named and toks and toks[-1] != "*" and len([t for t in toks if t != "*"]) > 1:
            toks = toks[:-1]                              # the argument's name
        base = [t for t in toks if t != "*"]
        assert len(base) == 1, text
        return base[0] + "*" * toks.count("*")

    out = {}
    for ret, name, args in re.findall(r"([A-Za-z_][A-Za-z0-9_\s\*]*?)\b(rom_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", src):
        args = args.strip()
        out[name] = (ctype(ret, False), [] if args in ("", "void") else [ctype(a, True) for a in args.split(",")])
    assert sorted(out) == header_symbols(), sorted(set(header_symbols()) ^ set(out))
    return out


def accepts(ctype, ct):
    """Does the ctypes type `ct` pass a C argument of type `ctype` unchanged?"""
    stars = ctype.count("*")
    base = ctype.rstrip("*")
    if stars == 0:
        assert base in SCALARS, f"no ctypes mapping for {ctype}"
        return ct is SCALARS[base]
    if ct is C.c_void_p:
        return True
    if base == "char" and stars == 1:
        return ct is C.c_char_p
    if base in SCALARS or base in HANDLES or base == "char":
        inner = SCALARS[base] if (stars == 1 and base in SCALARS) else C.c_void_p if base in HANDLES and stars == 2 else \
            C.POINTER(SCALARS[base]) if (stars == 2 and base in SCALARS) else None
        return inner is not None and ct is C.POINTER(inner)
    raise AssertionError(f"no ctypes mapping for {ctype}")


def test_prototypes_agree_with_the_header_argument_by_argument():
    from romhighcontrast_amd import _ffi
    protos = header_prototypes()
    assert sorted(protos) == sorted(_ffi.PROTOTYPES) and len(protos) >= 100
    for name, (ret, args) in protos.items():
        res, argtypes = _ffi.PROTOTYPES[name]
        assert accepts(ret, res) and (ret != "char*" or res is C.c_char_p), f"{name}: returns {ret}, bound as {res}"
        assert len(args) == len(argtypes), f"{name}: {len(args)} arguments in the header, {len(argtypes)} bound"
        for i, (a, ct) in enumerate(zip(args, argtypes)):
            assert accepts(a, ct), f"{name}: argument {i} is {a}, bound as {ct}"


def test_the_conformance_check_sees_a_narrow_count():
    """A c_int where the header says int64_t or size_t, a double for a pointer, a missing argument: all refused."""
    assert accepts("int64_t", C.c_int64) and not accepts("int64_t", C.c_int) and not accepts("size_t", C.c_int)
    assert not accepts("int", C.c_int64) and not accepts("double", C.c_void_p) and not accepts("double*", C.c_double)
    assert accepts("double*", C.POINTER(C.c_double)) and accepts("double*", C.c_void_p) and not accepts("int*", C.POINTER(C.c_double))
    assert accepts("rom_ctx**", C.POINTER(C.c_void_p)) and accepts("rom_buf*", C.c_void_p) and not accepts("rom_buf*", C.c_int64)
    assert accepts("char*", C.c_char_p) and not accepts("double*", C.c_char_p)
    protos = header_prototypes()
    assert protos["rom_nearest"][1][:5] == ["rom_ctx*", "rom_buf*", "size_t", "int64_t", "int64_t"]
    assert protos["rom_last_error"] == ("char*", []) and protos["rom_rows_scale"][1][-1] == "double*"
