#!/usr/bin/env python3
"""EVT 2.1 decode probe -> profiles/evt21_probe.json.

1. The bench's events (20 M, 346x260, seed 1) written as EVT 2.0 and as EVT 2.1 by the library's
   RAW writer, and a dense stream (rows of 32 consecutive x at equal t, about 20 M events) as
   EVT 2.1.  The three decodes run in turn in one process, after a warm-up, REPS times each;
   times are per-kernel sums of the context's HIP-event timing, as in scripts/ingest_probe.py.
   Algorithmic bytes = 2 x word_bytes x words (read in two passes) + 13 x events (written).
   Expectations: EVT 2.1 bytes/s >= 0.8 x EVT 2.0 bytes/s; dense events/s >= sparse events/s;
   each is recorded with a "met" flag, and the probe exits non-zero when one is missed.
2. With --parent-lib PATH (a libecc.so built from the parent commit): scripts/ingest_probe.py is
   run in turn with that library and with this tree's, ROUNDS times each, and both sets of
   per-kernel times for EVT 2.0 / 3.0 are recorded with their spreads (the unchanged kernels).

Usage: evt21_probe.py [--n N] [--reps R] [--parent-lib PATH] [--rounds K] [--out FILE]"""
import argparse
import json
import os
import re
import subprocess
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "event-camera-clustering-and-optical-flow-estimation_amd"))

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=1221 * 16384)
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--parent-lib", default=None)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--out", default=str(ROOT / "profiles" / "evt21_probe.json"))
args = ap.parse_args()
result = {"n_events": args.n, "reps": args.reps}


def ingest_probe_ab(parent_lib, rounds):
    """scripts/ingest_probe.py with the parent's library and with this tree's, in turn."""
    runs = {"parent": [], "this": []}
    for _ in range(rounds):
        for who in ("parent", "this"):
            env = dict(os.environ)
            env.pop("ECC_LIB", None)
            if who == "parent":
                env["ECC_LIB"] = str(Path(parent_lib).resolve())
            r = subprocess.run([sys.executable, str(ROOT / "scripts" / "ingest_probe.py"), str(args.n)], env=env,
                               capture_output=True, text=True, timeout=600, check=True)
            one = {}
            for line in r.stdout.splitlines():
                m = re.match(r"(EVT[23]) (\d+) (.*)", line)
                if m:
                    one[m.group(1)] = {k: float(v) for k, v in re.findall(r"(\w+) ([\d.]+) us", m.group(3))}
            runs[who].append(one)
            print(who, json.dumps(one), flush=True)
    out = {"rounds": rounds, "unit": "us per launch", "runs": runs, "summary": {}}
    for fmt in ("EVT2", "EVT3"):
        for k in runs["this"][0][fmt]:
            a = [r[fmt][k] for r in runs["parent"]]
            b = [r[fmt][k] for r in runs["this"]]
            out["summary"][f"{fmt}.{k}"] = {
                "parent_median": float(np.median(a)), "this_median": float(np.median(b)),
                "parent_spread": max(a) - min(a), "this_spread": max(b) - min(b),
                "within_spread": abs(float(np.median(a)) - float(np.median(b))) <= max(max(a) - min(a), max(b) - min(b))}
    return out


if args.parent_lib:
    result["unchanged_kernels"] = ingest_probe_ab(args.parent_lib, args.rounds)

import eccpy as ecc  # noqa: E402

ctx = ecc.Context(0)
n = args.n
xy, t, p = ecc.gen_events(n, seed=1, width=346, height=260)
rows = n // 32  # dense: row r is 32 consecutive x from a multiple of 32, one stamp per row
r = np.arange(rows, dtype=np.int64)
dxy = np.repeat((r % 10 * 32 | (r % 260) << 16), 32) + np.tile(np.arange(32), rows)
dense = (dxy.astype(np.uint32), np.repeat(r // 8, 32), np.repeat((r & 1).astype(np.uint8), 32))

streams = {}
for name, fmt, ev in (("evt2", ecc.EVT2, (xy, t, p)), ("evt21", ecc.EVT21, (xy, t, p)), ("evt21_dense", ecc.EVT21, dense)):
    words = ecc.evt_encode(fmt, *ev)
    m = len(ev[0])
    streams[name] = dict(fmt=fmt, n_words=len(words), n_events=m, word_bytes=words.dtype.itemsize,
                         dw=ecc.DeviceArray.from_numpy(words, ctx.stream),
                         out=(ecc.DeviceArray(m, np.uint32), ecc.DeviceArray(m, np.int64), ecc.DeviceArray(m, np.uint8),
                              ecc.DeviceArray(1, np.int64)),
                         runs=[])
    del words


def decode(s):
    ctx.evt_decode(s["fmt"], s["dw"], s["n_words"], s["out"][0], s["out"][1], s["out"][2], s["n_events"], s["out"][3])


for s in streams.values():  # warm-up, and the count
    decode(s)
    decode(s)
    ctx.sync()
    assert int(s["out"][3].numpy()[0]) == s["n_events"] and ctx.evt_status() == 0
ctx.set_timing(True)
for rep in range(args.reps):
    for s in streams.values():
        ctx.timing_reset()
        decode(s)
        st = ctx.timing_report()
        s["runs"].append({k: 1e3 * v["total_ms"] for k, v in st.items()})
ctx.set_timing(False)

for name, s in streams.items():
    kernels = sorted(s["runs"][0])
    per_kernel = {k: float(np.median([r[k] for r in s["runs"]])) for k in kernels}
    totals = [sum(r.values()) for r in s["runs"]]
    total = float(np.median(totals))
    nbytes = 2 * s["word_bytes"] * s["n_words"] + 13 * s["n_events"]
    result[name] = {"n_words": s["n_words"], "n_events": s["n_events"], "algorithmic_bytes": nbytes,
                    "bytes_per_event": nbytes / s["n_events"], "kernel_us_median": per_kernel,
                    "total_us_median": total, "total_us_min": min(totals), "total_us_max": max(totals),
                    "bytes_per_s": nbytes / (total * 1e-6), "events_per_s": s["n_events"] / (total * 1e-6)}
result["ratio_bytes_per_s_evt21_over_evt2"] = result["evt21"]["bytes_per_s"] / result["evt2"]["bytes_per_s"]
result["ratio_events_per_s_dense_over_sparse"] = result["evt21_dense"]["events_per_s"] / result["evt21"]["events_per_s"]
result["expect"] = {k: {"at_least": lo, "met": bool(result[k] >= lo)} for k, lo in
                    (("ratio_bytes_per_s_evt21_over_evt2", 0.8), ("ratio_events_per_s_dense_over_sparse", 1.0))}
Path(args.out).parent.mkdir(parents=True, exist_ok=True)
Path(args.out).write_text(json.dumps(result, indent=1) + "\n")
print(json.dumps({k: v for k, v in result.items() if k != "unchanged_kernels"}, indent=1))
missed = [k for k, v in result["expect"].items() if not v["met"]]
if missed:
    sys.exit("expectation not met: " + ", ".join(missed))
