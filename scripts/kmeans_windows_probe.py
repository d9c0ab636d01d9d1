#!/usr/bin/env python3
"""k-means per downsample window on the bench's representatives (20 M events of the 346x260 stream
-> 2442 windows of 8192; k = 16 from the 4x4 grid over the frame, threshold 50).  In one run, all
timed with HIP events, warm, median of several repetitions:
  (a) the one ecc_kmeans_windows_xy16 launch over all windows, at tol = -1 / max_iters = 10 and at
      tol = 0.01 / max_iters = 25 (with the histogram of updates per window);
  (b) the route it replaces: ecc_kmeans_run_xy16 window by window on interior pointers (n_segs = 1)
      over a fixed sample of 32 windows, scaled to all windows, and that the sample gives the same
      bytes as (a);
  (c) for context, the global ecc_kmeans_run_xy16_frame over all windows (one problem: k centres
      for the whole batch, not the same result).
Writes one JSON object.  Usage: kmeans_windows_probe.py [repetitions] [out.json]"""
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "event-camera-clustering-and-optical-flow-estimation_amd"))
import eccpy as ecc  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 7
out_path = Path(sys.argv[2]) if len(sys.argv) > 2 else ROOT / "profiles" / "kmeans_windows_probe.json"
n, W, H, WIN = 2442 * 8192, 346, 260, 8192
K, THR, SAMPLE = 16, 50.0, 32
ctx = ecc.Context(0)
xy, _, _ = ecc.gen_events(n, seed=1, width=W, height=H)
d_xy = ecc.DeviceArray.from_numpy(xy, ctx.stream)
rep_xy, rep_idx, uniq, rep, nw = ctx.downsample_hash(d_xy, n)
ctx.sync()
h_u = uniq.numpy()
i = np.arange(K)
init = np.stack([(i % 4 + 0.5) * W / 4, (i // 4 + 0.5) * H / 4], 1).astype(np.float32).ravel()
d_init = ecc.DeviceArray.from_numpy(init)
d_cent, d_lab = ecc.DeviceArray(nw * 2 * K, np.float32), ecc.DeviceArray(nw * WIN, np.uint8)
d_sizes, d_iters = ecc.DeviceArray(nw * K, np.int32), ecc.DeviceArray(nw, np.int32)


def median_ms(fn):
    fn()  # warm
    ctx.sync()
    times = []
    for _ in range(reps):
        tmr = ecc.Timer(ctx.stream)
        tmr.start()
        fn()
        times.append(tmr.stop())
    return float(np.median(times)), [round(t, 3) for t in times]


def windows(cfg):
    ctx.kmeans_windows(rep_xy, nw, WIN, uniq, cfg, d_init, d_cent, d_lab, d_sizes, d_iters)


out = {"windows": int(nw), "points": int(h_u.sum()), "k": K, "threshold": THR, "repetitions": reps}
sample = np.linspace(0, nw - 1, SAMPLE).astype(int)
lds = ((WIN + 3) // 4 * 4 + 2 * 16 + 4 * 3 * 16 + 4) * 4  # the kernel's dynamic LDS at this stride, 16 padded centres
out["lds_bytes_per_workgroup"] = lds
out["workgroups_per_cu_by_lds"] = min(8, 160 * 1024 // lds)
for name, tol, iters in (("fixed_10", -1.0, 10), ("tol_25", 0.01, 25)):
    cfg = ecc.kmeans_cfg(k=K, max_iters=iters, threshold=THR, tol=tol)
    a_ms, a_all = median_ms(lambda: windows(cfg))
    h_cent, h_lab, h_it = d_cent.numpy().reshape(nw, 2 * K), d_lab.numpy().reshape(nw, WIN), d_iters.numpy()
    # (b) window by window through the global entry, every call with its own outputs
    s_cent = [ecc.DeviceArray(2 * K, np.float32) for _ in sample]
    s_lab = [ecc.DeviceArray(WIN, np.uint8) for _ in sample]
    s_it = [ecc.DeviceArray(1, np.int32) for _ in sample]

    def route():
        for j, w in enumerate(sample):
            ecc.check(ecc.lib.ecc_memcpy_d2d(s_cent[j].ptr, d_init.ptr, 8 * K, ctx.stream))
            ecc.check(ecc.lib.ecc_kmeans_run_xy16(ctx.ctx, rep_xy.ptr + 4 * int(w) * WIN, 1, WIN, uniq.ptr + 4 * int(w),
                                                  ecc.C.byref(cfg), s_cent[j].ptr, s_lab[j].ptr, s_it[j].ptr, ctx.stream))

    b_ms, b_all = median_ms(route)
    match = True
    for j, w in enumerate(sample):
        m = int(h_u[w])
        match &= s_cent[j].numpy().tobytes() == h_cent[w].tobytes() and int(s_it[j].numpy()[0]) == int(h_it[w])
        match &= bool((s_lab[j].numpy()[:m] == h_lab[w, :m]).all())
    b_all_windows = b_ms / SAMPLE * nw
    out[name] = {"tol": tol, "max_iters": iters, "windows_launch_ms": round(a_ms, 3), "windows_launch_ms_all": a_all,
                 "per_window_route_sample_windows": SAMPLE, "per_window_route_sample_ms": round(b_ms, 3),
                 "per_window_route_sample_ms_all": b_all, "per_window_route_all_windows_ms": round(b_all_windows, 1),
                 "ratio_route_to_launch": round(b_all_windows / a_ms, 1), "sample_matches": bool(match),
                 "iters_histogram": {str(v): int(c) for v, c in zip(*np.unique(h_it, return_counts=True))}}
    # (c) one global problem over all windows
    d_c = ecc.DeviceArray(2 * K, np.float32)

    def global_run():
        ecc.check(ecc.lib.ecc_memcpy_d2d(d_c.ptr, d_init.ptr, 8 * K, ctx.stream))
        ctx.kmeans_xy16_frame(rep_xy, nw, WIN, uniq, W, H, d_c, cfg, d_lab)

    c_ms, c_all = median_ms(global_run)
    out[name]["global_frame_ms"] = round(c_ms, 3)
    out[name]["ratio_launch_to_global"] = round(a_ms / c_ms, 2)
out_path.parent.mkdir(parents=True, exist_ok=True)
out_path.write_text(json.dumps(out, indent=1) + "\n")
print(json.dumps(out))
