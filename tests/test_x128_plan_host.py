"""The per-tile records of k_extend128 on the CPU, under AddressSanitizer and UBSan: tests/c_abi/x128_plan_check.cpp is a stand-alone
program that plans 2x2 / N = 128 (row tiles), 3x3 / N = 64 (FLAT), 2x2 / N = 171 (FLAT, tiles inside one mesh row), 2x2 / N = 250 (two
column tiles per mesh row, the last partly filled) and 5x4 / N = 64 (20 blocks: two launches) and holds every record of both tilings
(FemPlan::x128_row, x128_flat: what the kernel fetches instead of walking the thresholds) against a fresh x128_skip_counts call, the
masks built bit by bit and by the kernel's former formula, and the block indexing of the launches.  No GPU, nothing loaded into
this process."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# geometry -> (lr blocks, launches, row tiles per block, FLAT tiles per block)
EXPECTED = {"2x2-N128": (4, 1, 127, 127), "3x3-N64": (9, 1, 63, 32), "2x2-N171": (4, 1, 340, 226), "2x2-N250": (4, 1, 498, 485),
            "5x4-N64": (20, 2, 63, 32)}


def _build(tmp_path):
    gxx = shutil.which("g++")
    assert gxx, "g++ is part of the image"
    exe = str(tmp_path / "x128_plan_check")
    csrc = os.path.join(ROOT, "romhighcontrast_amd", "csrc")
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I", os.path.join(ROOT, "include"), "-I", csrc, "-x", "c++",
           os.path.join(csrc, "rom_fem_plan.hip"), os.path.join(ROOT, "tests", "c_abi", "x128_plan_check.cpp"),
           "-lpthread", "-o", exe]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0, r.stdout.decode()
    return exe


def test_tile_records_match_a_fresh_walk(tmp_path):
    exe = _build(tmp_path)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    out, err = r.stdout.decode(), r.stderr.decode()
    print(out)
    assert r.returncode == 0, out + err
    assert err == "", err  # no sanitizer report, no violation
    got = {}
    for ln in out.splitlines():
        f = ln.split()
        if f and f[0] == "records":
            got[f[1]] = (int(f[3]), int(f[5]), int(f[7]), int(f[9]))
            assert int(f[11]) > 0, ln  # some wave of the tiling in use skips something: the masks are not all trivial
    assert got == EXPECTED
