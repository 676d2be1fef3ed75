"""The per-wave K-segment skipping of k_extend128 on the CPU, under AddressSanitizer and UBSan: tests/c_abi/ext_wave_skip_check.cpp
is a stand-alone program that plans 2x2 / N = 128 (row tiles), 3x3 / N = 64 (FLAT; an interior edge with thresholds 29 / 39 / 59),
3x3 / N = 171 (FLAT, n1 = 170), 2x3 / N = 128, 4x4 / N = 256 and the wide cases of tests/sweep_truth.py that have something to skip
(2x2 / N = 171, 3x3 / N = 140, 2x2 / N = 250) and calls x128_skip_counts (rom_fem_plan.h, the function the kernel
calls) for every tile, wave column and side: no vertex of a wave needs a segment in front of the wave's skip count, the wave's count
is at least the tile's, and every geometry has a place where it is larger.  No GPU, nothing loaded into this process.

The counts it prints (one unit = 128 systems x 32 vertices x 8 k) are held against the figures the change was planned with, for
the three geometries of bench.py in the tiling each uses:
    executed while every wave followed its tile's walk   C2 15 456   C4 99 000   C5 463 664   -- reproduced to the unit;
    needed at wave granularity, no zero half             C2 13 676   C4 87 400   C5 420 700   -- the planning figures, the last
two rounded; x128_skip_counts gives 13 672, 87 383 and 420 380 (ratios 0.885 / 0.883 / 0.907 as planned), and these are what the
brute-force check above covers, so these are asserted.  The share of the tile-level count the waves still multiply must be the
planned 0.931 / 0.977 / 0.917 / 0.924 for the first four geometries."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

EXECUTED_TILE = {"2x2-N128": 15456, "3x3-N171": 99000, "4x4-N256": 463664}
NEEDED_WAVE = {"2x2-N128": 13672, "3x3-N171": 87383, "4x4-N256": 420380}
PLANNED_NEEDED = {"2x2-N128": 13676, "3x3-N171": 87400, "4x4-N256": 420700}
TILING = {"2x2-N128": "row", "3x3-N64": "flat", "3x3-N171": "flat", "2x3-N128": "row", "4x4-N256": "row",
          "2x2-N171": "flat", "3x3-N140": "flat", "2x2-N250": "row"}      # (the last three: the wide cases of tests/sweep_truth.py)
WAVE_OVER_TILE = {"2x2-N128": 0.931, "3x3-N64": 0.977, "3x3-N171": 0.917, "2x3-N128": 0.924}


def _build(tmp_path):
    gxx = shutil.which("g++")
    assert gxx, "g++ is part of the image"
    exe = str(tmp_path / "ext_wave_skip_check")
    csrc = os.path.join(ROOT, "romhighcontrast_amd", "csrc")
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I", os.path.join(ROOT, "include"), "-I", csrc, "-x", "c++",
           os.path.join(csrc, "rom_fem_plan.hip"), os.path.join(ROOT, "tests", "c_abi", "ext_wave_skip_check.cpp"),
           "-lpthread", "-o", exe]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0, r.stdout.decode()
    return exe


def test_wave_skip_counts_are_safe_and_as_planned(tmp_path):
    exe = _build(tmp_path)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    out, err = r.stdout.decode(), r.stderr.decode()
    print(out)
    assert r.returncode == 0, out + err
    assert err == "", err  # no sanitizer report, no violation
    counts = {}
    for ln in out.splitlines():
        f = ln.split()
        if f and f[0] == "count":
            counts[f[1]] = dict(tiling=f[2], executed_tile=int(f[4]), needed_wave=int(f[6]), tile_needed=int(f[8]))
    assert {k: v["tiling"] for k, v in counts.items()} == TILING
    assert {k: counts[k]["executed_tile"] for k in EXECUTED_TILE} == EXECUTED_TILE
    assert {k: counts[k]["needed_wave"] for k in NEEDED_WAVE} == NEEDED_WAVE
    for k, planned in PLANNED_NEEDED.items():  # (the planning figures: within a thousandth)
        assert abs(counts[k]["needed_wave"] - planned) <= 1e-3 * planned, (k, counts[k], planned)
    for k, share in WAVE_OVER_TILE.items():
        assert abs(counts[k]["needed_wave"] / counts[k]["tile_needed"] - share) < 5e-4, (k, counts[k], share)
    assert any(ln.startswith("thresholds 3x3-N64 rank") and ln.split(":")[1].split()[:3] == ["29", "39", "59"] for ln in out.splitlines())
