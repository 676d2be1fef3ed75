"""The host-visible rules of the small dense layer on the CPU, under AddressSanitizer and UBSan:
tests/c_abi/small_dense_host_check.cpp is a stand-alone program over csrc/rom_small_dense_host.h.  It checks the LDS layouts
of kb_small_eig and kb_pivchol_whiten (totals equal to the byte counts the launchers used to compute by hand for n = 1 ... 96,
disjoint sub-arrays, aligned doubles, within the opt-in at n = 96), the round-robin pair helper (disjoint covering rounds,
every pair once per sweep, equal to kb_small_eig's earlier modular spelling, for every even order 2 ... 98 and 2048) and the
rotation thresholds against the literal expression.  No GPU, nothing loaded into this process."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def output(tmp_path_factory):
    gxx = shutil.which("g++")
    assert gxx, "g++ is part of the image"
    exe = str(tmp_path_factory.mktemp("small_dense_host") / "small_dense_host_check")
    csrc = os.path.join(ROOT, "romhighcontrast_amd", "csrc")
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-I", csrc, os.path.join(ROOT, "tests", "c_abi", "small_dense_host_check.cpp"), "-o", exe]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0, r.stdout.decode()
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    return r.returncode, r.stdout.decode(), r.stderr.decode()


def test_layouts_pairs_and_thresholds_are_clean_under_sanitizers(output):
    code, out, err = output
    assert code == 0, out + err
    assert err == "", err                      # no sanitizer report
    assert out.splitlines()[-1] == "OK" and "FAILED" not in out, out


def test_lds_totals_at_the_largest_order(output):
    """n = 96, ld = 97: two 96 x 97 matrices of doubles plus the vectors -- the launch sizes written out."""
    line = [ln.split() for ln in output[1].splitlines() if ln.startswith("LAYOUT ")]
    assert len(line) == 1
    mats = 2 * 96 * 97 * 8
    assert int(line[0][2]) == mats + (2 * 48 + 2 * 96 + 8) * 8 + (2 * 48 + 96 + 2) * 4 + 16 == 152152 <= 160 * 1024
    assert int(line[0][4]) == mats + 4 * 8 + (4 + 96) * 4 + 16 == 149440 <= 160 * 1024 - 256
