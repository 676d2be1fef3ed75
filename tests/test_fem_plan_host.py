"""The host planner of rom_fem_create (romhighcontrast_amd/csrc/rom_fem_plan.hip) on the CPU, under AddressSanitizer and
UBSan: tests/c_abi/fem_plan_check.cpp is a stand-alone program that plans every geometry of tests/sweep_truth.py::CASES and
3x3 / N = 24 under each planner switch, twice each, and checks determinism under the host threads, the layout of the
interface vector and what the sweep kernels assume about the tables.  No GPU, nothing loaded into this process."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build_plan_check(tmp_path):
    gxx = shutil.which("g++")
    assert gxx, "g++ is part of the image"
    exe = str(tmp_path / "fem_plan_check")
    csrc = os.path.join(ROOT, "romhighcontrast_amd", "csrc")
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I", os.path.join(ROOT, "include"), "-I", csrc, "-x", "c++",
           os.path.join(csrc, "rom_fem_plan.hip"), os.path.join(ROOT, "tests", "c_abi", "fem_plan_check.cpp"),
           "-lpthread", "-o", exe]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0, r.stdout.decode()
    return exe


def test_planner_is_clean_under_sanitizers(tmp_path):
    exe = _build_plan_check(tmp_path)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    out, err = r.stdout.decode(), r.stderr.decode()
    assert r.returncode == 0, out + err
    assert err == "", err                      # no sanitizer report, no violation
    assert len(out.splitlines()) == 20, out    # sixteen geometries + four switches
