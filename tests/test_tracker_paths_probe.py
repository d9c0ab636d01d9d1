"""csrc/tracker_paths.hpp — the corner tracker's switch points and pure path rules — checked on the
CPU with a stand-alone probe (tests/tracker_paths_probe.cpp: its own main, only that header, no
HIP and no libecc), built plainly and with -fsanitize=undefined; both must print the same text.

  * the rules over their domains: the lanes per track of tracker_kernel's brute scan (a power of
    two, T * L * 2 <= kNT, at most kLanesMax, one with the grid) and lists_ok; the fast kernel's
    lane shift and chunk width; grid_ok and the cell size of a radius;
  * the property the grid visitor needs: the integer box [p - reach, p + reach] of a prediction
    spans at most 3 cells per axis for every max_distance in [0, 1e5) of the sweep;
  * floor_div equals Python's // for negative numerators; cell_bucket stays inside the table.
"""
import subprocess

import numpy as np
import pytest

import tracker_cases as tc


@pytest.fixture(scope="module")
def exes(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("trk_probe")
    out = {}
    for name, extra in (("plain", ["-O2"]), ("ubsan", ["-O2", "-fsanitize=undefined", "-fno-sanitize-recover=all"])):
        exe = tmp / name
        subprocess.run(["g++", *extra, *tc.PROBE_FLAGS, "-o", str(exe), str(tc.PROBE_SRC)], check=True, timeout=300)
        out[name] = exe
    return out


def both(exes, *args):
    a = tc.probe(*args, exe=exes["plain"])
    assert tc.probe(*args, exe=exes["ubsan"]) == a
    return a


def test_constants(exes):
    k = {n: int(v) for n, v in (l.split("=") for l in both(exes, "consts"))}
    assert k == tc.consts()
    assert set(k) >= {"kFT", "kFList", "kFTailTracks", "kFLaneShiftT", "kFChunkNarrow", "kFChunkWide", "kBrute",
                      "kBuckets", "kLaneList", "kTailCap", "kTailTracks", "kGroupWave", "kNT"}
    assert k["kFT"] <= 256 and k["kBuckets"] & (k["kBuckets"] - 1) == 0
    assert max(k["kTailTracks"], k["kFTailTracks"], k["kGroupWave"]) <= 64  # one lane of a wave each


def test_floor_div_is_pythons(exes):
    rng = np.random.default_rng(1)
    a = [-1, -2, -31, -32, -33, -32768, -32769, -65536, 0, 1, 31, 32, 33, 32767, -(2 ** 31) + 100002, 2 ** 31 - 1]
    a += [int(v) for v in rng.integers(-(2 ** 30), 2 ** 30, 300)]
    b = [1, 2, 3, 31, 32, 33, 1000, 100001]
    pairs = [(x, y) for x in a for y in b]
    got = [int(l) for l in both(exes, "floor_div", *[v for p in pairs for v in p])]
    assert got == [x // y for x, y in pairs]


def test_buckets_in_table(exes):
    rng = np.random.default_rng(2)
    cells = [(int(x), int(y)) for x, y in rng.integers(-40000, 40000, (2000, 2))] + [(0, 0), (-1, -1), (-1024, 1023)]
    got = [int(l) for l in both(exes, "bucket", *[v for c in cells for v in c])]
    assert min(got) >= 0 and max(got) < tc.consts()["kBuckets"]
    assert len(set(got)) > tc.consts()["kBuckets"] // 2  # it spreads


def test_lane_rules(exes):
    k = tc.consts()
    args = [v for T in range(0, 4200) for g in (0, 1) for v in (T, g)]
    rows = [tuple(int(x) for x in l.split()) for l in both(exes, "lanes", *args)]
    for (T, g), (L, ok) in zip([(T, g) for T in range(0, 4200) for g in (0, 1)], rows):
        assert L & (L - 1) == 0 and 1 <= L <= k["kLanesMax"]
        if g:
            assert L == 1
        else:
            assert L == 1 or T * L <= k["kNT"]                      # every lane group has its track
            assert L == k["kLanesMax"] or T * L * 2 > k["kNT"]  # and the loop stopped where it must
        assert ok == (T * L <= k["kNT"])
    fast = [tuple(int(x) for x in l.split()) for l in
            both(exes, "fast", *[v for T in range(0, k["kFT"] + 1) for C in (0, 1, 16, 17, 32, 33, 64, 65, 128, 256) for v in (T, C)])]
    it = iter(fast)
    for T in range(0, k["kFT"] + 1):
        for C in (0, 1, 16, 17, 32, 33, 64, 65, 128, 256):
            sh, chunk = next(it)
            assert sh in (1, 2) and T << sh <= k["kFThreads"]
            assert sh == (2 if T <= k["kFLaneShiftT"] else 1)
            assert chunk == (k["kFChunkNarrow"] if C <= k["kFChunkNarrow"] << sh else k["kFChunkWide"])


def test_grid_rule(exes):
    mds = [0.0, 0.5, 1.0, 12.5, 30.0, tc.down(30.0), tc.up(30.0), 99999.0, tc.down(1.0e5), 1.0e5, tc.up(1.0e5), 1.0e6,
           -0.0, -1.0, tc.down(0.0), tc.NAN, tc.INF, -tc.INF]
    rows = [l.split() for l in both(exes, "grid", *["%08x" % tc.bits(m) for m in mds])]
    for md, (ok, cell, reach) in zip(mds, rows):
        md = np.float32(md)
        want = bool(md >= 0 and md < np.float32(1.0e5))
        assert bool(int(ok)) == want, md
        if want:
            r = md + np.float32(1)
            assert int(reach, 16) == tc.bits(r)
            assert int(cell) == int(np.ceil(r)) + 1 >= 2
        else:
            assert int(cell) == 1


def test_box_spans_three_cells(exes):
    out = both(exes, "span")
    assert len(out) == 1 and out[0].startswith("OK checked="), out
    assert int(out[0].split("=")[1]) > 10 ** 6
