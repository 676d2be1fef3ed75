"""The extension truncation of the host planner (romhighcontrast_amd/csrc/rom_fem_plan.hip) on the CPU, under AddressSanitizer
and UBSan: tests/c_abi/ext_trunc_check.cpp is a stand-alone program that plans 2x2 at N = 40, 64, 128 and 3x3 at N = 64 and
checks the rotated basis (W^T W = I), the exact zeros below the echelon of the stored sine coefficients, the distance
thresholds, that every geometry has a (table, distance) with fewer K segments than full, and the long-double bound of every
table entry the mask zeroes.  With no_ext_trunc the plan must be the one the planner made before the truncation existed:
tests/golden/ext_trunc_parent_plans.json holds the FNV-1a hashes of those plans.  No GPU, nothing loaded into this process."""
import json
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build(tmp_path):
    gxx = shutil.which("g++")
    assert gxx, "g++ is part of the image"
    exe = str(tmp_path / "ext_trunc_check")
    csrc = os.path.join(ROOT, "romhighcontrast_amd", "csrc")
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I", os.path.join(ROOT, "include"), "-I", csrc, "-x", "c++",
           os.path.join(csrc, "rom_fem_plan.hip"), os.path.join(ROOT, "tests", "c_abi", "ext_trunc_check.cpp"),
           "-lpthread", "-o", exe]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0, r.stdout.decode()
    return exe


def test_extension_truncation_plan(tmp_path):
    exe = _build(tmp_path)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    out, err = r.stdout.decode(), r.stderr.decode()
    assert r.returncode == 0, out + err
    assert err == "", err  # no sanitizer report, no violation
    got = {ln.split()[1]: ln.split()[2] for ln in out.splitlines() if ln.startswith("hash ")}
    with open(os.path.join(ROOT, "tests", "golden", "ext_trunc_parent_plans.json")) as fh:
        want = json.load(fh)
    assert got == want  # no_ext_trunc: the same bytes as a plan of the parent's form
