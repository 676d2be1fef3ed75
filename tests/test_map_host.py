"""The host side of the map entry points on the CPU, under AddressSanitizer and UBSan: tests/c_abi/map_host_check.cpp is a
stand-alone program over csrc/rom_block.h (the one check of a device block: its two messages, blocks that end on the buffer's
last double, extents that wrap a size_t) and csrc/rom_poly_host.h (the host arithmetic of rom_poly_fit on integer inputs with
exactly representable answers).  It prints the exponent rows and factor tables, which are rebuilt here in the order of
PolynomialFeatures(d).powers_: graded, combinations_with_replacement(range(m), k) in lexicographic order.  No GPU, nothing
loaded into this process."""
import itertools
import math
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PL_MAX, PL_DMAX, PL_NOFAC = 96, 8, 255
CASES = [(1, 1), (2, 3), (3, 2), (16, 1), (2, 8), (4, 4), (5, 3)]     # (5, 3): the largest P <= 96 at m = 5
TABLES = [(2, 3), (3, 2)]


@pytest.fixture(scope="module")
def output(tmp_path_factory):
    gxx = shutil.which("g++")
    assert gxx, "g++ is part of the image"
    exe = str(tmp_path_factory.mktemp("map_host") / "map_host_check")
    csrc = os.path.join(ROOT, "romhighcontrast_amd", "csrc")
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I", os.path.join(ROOT, "include"), "-I", csrc,
           os.path.join(ROOT, "tests", "c_abi", "map_host_check.cpp"), "-o", exe]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0, r.stdout.decode()
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    return r.returncode, r.stdout.decode(), r.stderr.decode()


def powers(m, d):
    rows = []
    for k in range(d + 1):
        for comb in itertools.combinations_with_replacement(range(m), k):
            rows.append([comb.count(j) for j in range(m)])
    return rows


def test_block_checks_and_host_arithmetic_are_clean_under_sanitizers(output):
    code, out, err = output
    assert code == 0, out + err
    assert err == "", err                      # no sanitizer report
    assert out.splitlines()[-1] == "OK" and "FAILED" not in out, out


def test_exponent_rows_are_those_of_polynomial_features(output):
    lines = [ln.split() for ln in output[1].splitlines() if ln.startswith("POWERS ")]
    assert [(int(ln[1]), int(ln[2])) for ln in lines] == CASES
    assert math.comb(5 + 4, 4) > PL_MAX >= math.comb(5 + 3, 3)
    for ln in lines:
        m, d, P = int(ln[1]), int(ln[2]), int(ln[3])
        assert P == math.comb(m + d, d) <= PL_MAX
        got = [int(v) for v in ln[4:]]
        assert got == [e for row in powers(m, d) for e in row], (m, d)


def test_factor_tables_list_the_legendre_entries_in_input_order(output):
    lines = [ln.split() for ln in output[1].splitlines() if ln.startswith("TABLE ")]
    assert [(int(ln[1]), int(ln[2])) for ln in lines] == TABLES
    for ln in lines:
        m, d = int(ln[1]), int(ln[2])
        got = [int(v) for v in ln[3:]]
        want = []
        for row in powers(m, d):
            fac = [j * d + a - 1 for j, a in enumerate(row) if a > 0]
            want += fac + [PL_NOFAC] * (PL_DMAX - len(fac))
        want += [PL_NOFAC] * (PL_DMAX * PL_MAX - len(want))
        assert got == want, (m, d)
