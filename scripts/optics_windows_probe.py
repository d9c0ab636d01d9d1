#!/usr/bin/env python3
"""Per-window OPTICS (eps 10, min_pts 2, threshold 10: OPT/test/cluster_event_data.cpp:449-454) on
the bench's representatives (20 M events of the 346x260 stream -> 2442 windows of 8192):
  * one ecc_optics_grid launch over all windows, HIP events, warm, median of several repetitions;
  * the per-window ecc_optics_f64 route (GPU eps-balls, list download, host expansion) of the same
    library over a fixed sample of 32 windows, wall clock, scaled to all windows;
and that the two agree on the sampled windows.  Prints one JSON line.
Usage: optics_windows_probe.py [repetitions]"""
import json
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1] / "event-camera-clustering-and-optical-flow-estimation_amd"))
import eccpy as ecc  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 7
n, W, H, WIN = 2442 * 8192, 346, 260, 8192
EPS, MIN_PTS, THR, SAMPLE = 10.0, 2, 10.0, 32
ctx = ecc.Context(0)
xy, _, _ = ecc.gen_events(n, seed=1, width=W, height=H)
d_xy = ecc.DeviceArray.from_numpy(xy, ctx.stream)
rep_xy, rep_idx, uniq, rep, nw = ctx.downsample_hash(d_xy, n)
ctx.sync()
tot = nw * WIN
d_order, d_reach = ecc.DeviceArray(tot, np.int32), ecc.DeviceArray(tot, np.float64)
d_cl, d_ncl = ecc.DeviceArray(tot, np.int32), ecc.DeviceArray(nw, np.int32)


def launch():
    ctx.optics_grid(rep_xy, nw, WIN, uniq, EPS, MIN_PTS, THR, d_order, d_reach, d_cl, d_ncl)


launch()  # warm
ctx.sync()
assert ctx.optics_grid_status() == ecc.OK
times = []
for _ in range(reps):
    tmr = ecc.Timer(ctx.stream)
    tmr.start()
    launch()
    times.append(tmr.stop())
grid_ms = float(np.median(times))

h_xy, h_u = rep_xy.numpy(), uniq.numpy()
h_order, h_reach = d_order.numpy(), d_reach.numpy()
sample = np.linspace(0, nw - 1, SAMPLE).astype(int)
pts = []
for w in sample:
    x, y = ecc.unpack_xy(h_xy[w * WIN: w * WIN + int(h_u[w])])
    pts.append(np.stack([x, y], 1).astype(np.float64))
ctx.optics_f64(pts[0], MIN_PTS, EPS)  # warm (workspace growth)
t0 = time.perf_counter()
host = [ctx.optics_f64(p, MIN_PTS, EPS) for p in pts]
host_sample_ms = (time.perf_counter() - t0) * 1e3
match = all(np.array_equal(o, h_order[w * WIN: w * WIN + len(o)]) and np.array_equal(r, h_reach[w * WIN: w * WIN + len(r)])
            for w, (o, r) in zip(sample, host))
host_ms = host_sample_ms / SAMPLE * nw
print(json.dumps({
    "windows": int(nw), "points": int(h_u.sum()), "eps": EPS, "min_pts": MIN_PTS, "threshold": THR,
    "optics_grid_ms": round(grid_ms, 3), "optics_grid_ms_all": [round(t, 3) for t in times],
    "optics_f64_sample_windows": SAMPLE, "optics_f64_sample_ms": round(host_sample_ms, 2),
    "optics_f64_all_windows_ms": round(host_ms, 1), "ratio": round(host_ms / grid_ms, 1),
    "sample_matches": bool(match), "clusters": int(d_ncl.numpy().sum()),
}))
