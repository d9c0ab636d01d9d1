"""csrc/corner_decode.hpp — the multiply-high constants with which the corner kernels turn an item
number into (group, tile) and a tile into (row, column) — checked on the CPU with a stand-alone
probe (tests/corner_decode_probe.cpp: its own main, only that header, no HIP and no libecc):
the quotient equals v / d for every divisor up to 8192 at the dividends where such a quotient can
first go wrong, and for every dividend below 2^31 at the tile count 7475.  The probe is also built
with -fsanitize=undefined (the shifts by 31 + ceil(log2 d)) and must print the same text.
"""
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "event-camera-clustering-and-optical-flow-estimation_amd" / "csrc"
SRC = Path(__file__).with_name("corner_decode_probe.cpp")
FLAGS = ["-std=c++17", "-Wall", "-Werror", f"-I{CSRC}"]


def _build_and_run(tmp, name, extra):
    exe = tmp / name
    subprocess.run(["g++", *extra, *FLAGS, "-o", str(exe), str(SRC)], check=True, timeout=300)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    assert r.stderr == ""
    return r.stdout


def test_magic_division_is_exact(tmp_path):
    plain = _build_and_run(tmp_path, "probe", ["-O2"])
    assert plain.startswith("OK checked="), plain
    assert int(plain.split("=")[1]) > (1 << 31)
    ubsan = _build_and_run(tmp_path, "probe_ubsan", ["-O2", "-fsanitize=undefined", "-fno-sanitize-recover=all"])
    assert ubsan == plain
