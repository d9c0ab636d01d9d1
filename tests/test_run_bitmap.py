"""csrc/run_bitmap.hpp — the pixel bitmap of a distinct-pixel window that eps_run_counts_kernel and
dbscan_run_kernel share — checked on the CPU with a stand-alone probe (tests/run_bitmap_probe.cpp:
its own main, only that header, no HIP and no libecc): the exact half-widths, the box geometry at
the widths where the words per row and the end word change (1, 31, 32, 33, 63, 64, 65), raster
ranks, and the row-run count of every set pixel against brute force over the pixel list, at
occupancies of 5 %, 50 % and 100 %, for eps from 0 to 70 (chords inside one word, across two and
three, and wider than the box).  Built a second time with the undefined-behaviour sanitizer (the
shift counts), and that program is run directly.
"""
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "event-camera-clustering-and-optical-flow-estimation_amd" / "csrc"
SRC = Path(__file__).with_name("run_bitmap_probe.cpp")


@pytest.mark.parametrize("extra", [[], ["-fsanitize=undefined", "-fno-sanitize-recover"]], ids=["plain", "ubsan"])
def test_run_bitmap_against_brute_force(tmp_path, extra):
    exe = tmp_path / "probe"
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", *extra, f"-I{CSRC}", "-o", str(exe), str(SRC)],
                   check=True, timeout=300)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    assert r.stdout.startswith("OK queries="), r.stdout
    assert int(r.stdout.split("=")[1]) > 50000  # every set pixel of every box, at every eps
