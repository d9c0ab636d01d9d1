#!/usr/bin/env python3
"""The xi-cluster hierarchy (optics.hpp:948-995) of the bench's per-window xi pairs: 20 M events of
the 346x260 stream -> 2442 windows of 8192 -> ecc_optics_grid (eps 10, min_pts 2) -> ecc_optics_xi,
pairs left on the device.  For the reference KATs' two parameter sets (chi 0.1 / min_pts 4, and chi
0.02 / min_pts 5 / steep_area_min_diff 0.15):
  (a) one ecc_optics_xi_tree launch over all windows;
  (b) the route without it: device-to-host copy of the pairs and counts, then
      ecc_optics_xi_tree_host window after window on one thread, wall clock, with identical bytes
      asserted in every window;
  (c) the ecc_optics_xi launch before it.
(a) and (c) are timed in the same run with HIP events around LAUNCHES back-to-back launches, warm,
the two alternating, median of several repetitions.  Writes profiles/optics_tree_probe.json and
prints it.
Usage: optics_tree_probe.py [repetitions]"""
import ctypes as C
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "event-camera-clustering-and-optical-flow-estimation_amd"))
import eccpy as ecc  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 7
LAUNCHES = 20
n, W, H, WIN = 2442 * 8192, 346, 260, 8192
EPS, MIN_PTS = 10.0, 2
PARAMS = [(0.1, 4, 0.0), (0.02, 5, 0.15)]
ctx = ecc.Context(0)
xy, _, _ = ecc.gen_events(n, seed=1, width=W, height=H)
d_xy = ecc.DeviceArray.from_numpy(xy, ctx.stream)
rep_xy, rep_idx, uniq, rep, nw = ctx.downsample_hash(d_xy, n)
ctx.sync()
tot = nw * WIN
d_order, d_reach = ecc.DeviceArray(tot, np.int32), ecc.DeviceArray(tot, np.float64)
ctx.optics_grid(rep_xy, nw, WIN, uniq, EPS, MIN_PTS, 0.0, d_order, d_reach)
assert ctx.optics_grid_status() == ecc.OK


def per_launch_ms(fn):
    tmr = ecc.Timer(ctx.stream)
    tmr.start()
    for _ in range(LAUNCHES):
        fn()
    return tmr.stop() / LAUNCHES


d_ncl = ecc.DeviceArray(nw, np.int32)
out = {"windows": int(nw), "points": int(uniq.numpy().sum()), "eps": EPS, "min_pts": MIN_PTS,
       "launches_per_timing": LAUNCHES, "repetitions": reps, "tree": []}
for chi, mp, samd in PARAMS:
    # the counts first (cap 0 writes no pair), then everything at the largest count
    ctx.optics_xi(d_reach, nw, WIN, uniq, chi, mp, samd, d_ncl, 0, d_ncl)
    ctx.optics_xi_status()
    cap = max(int(d_ncl.numpy().max()), 1)
    d_pairs = ecc.DeviceArray(nw * cap * 2, np.int32)
    d_sorted, d_parent = ecc.DeviceArray(nw * cap * 2, np.int32), ecc.DeviceArray(nw * cap, np.int32)
    d_level, d_roots = ecc.DeviceArray(nw * cap, np.int32), ecc.DeviceArray(nw, np.int32)

    def xi():
        ctx.optics_xi(d_reach, nw, WIN, uniq, chi, mp, samd, d_pairs, cap, d_ncl)

    def tree():
        ctx.optics_xi_tree(d_pairs, cap, d_ncl, nw, d_sorted, d_parent, d_level, d_roots)

    xi(), tree()  # warm
    ctx.sync()
    xi_all, tree_all = [], []
    for _ in range(reps):
        xi_all.append(per_launch_ms(xi))
        tree_all.append(per_launch_ms(tree))
    assert ctx.optics_xi_status() == ecc.OK and ctx.optics_xi_tree_status() == ecc.OK
    xi_ms, tree_ms = float(np.median(xi_all)), float(np.median(tree_all))
    g_sorted, g_parent = d_sorted.numpy().reshape(nw, cap, 2), d_parent.numpy().reshape(nw, cap)
    g_level, g_roots = d_level.numpy().reshape(nw, cap), d_roots.numpy()

    # (b) copy the pairs and counts back, walk every window on one host thread
    t0 = time.perf_counter()
    pairs, counts = d_pairs.numpy().reshape(nw, cap, 2), d_ncl.numpy()
    copy_ms = (time.perf_counter() - t0) * 1e3
    h_sorted, h_parent, h_level = np.zeros((cap, 2), np.int32), np.zeros(cap, np.int32), np.zeros(cap, np.int32)
    k = C.c_int64(0)
    match, deepest = True, 0
    t0 = time.perf_counter()
    for w in range(nw):
        p = int(counts[w])
        rc = ecc.lib.ecc_optics_xi_tree_host(pairs[w].ctypes.data, p, h_sorted.ctypes.data, h_parent.ctypes.data,
                                             h_level.ctypes.data, C.addressof(k))
        match &= (rc == ecc.OK and k.value == g_roots[w] and h_sorted[:p].tobytes() == g_sorted[w, :p].tobytes()
                  and h_parent[:p].tobytes() == g_parent[w, :p].tobytes()
                  and h_level[:p].tobytes() == g_level[w, :p].tobytes())
        deepest = max(deepest, int(h_level[:p].max(initial=0)))
    walk_ms = (time.perf_counter() - t0) * 1e3
    assert match, "the device trees differ from ecc_optics_xi_tree_host"
    out["tree"].append({
        "chi": chi, "min_pts": mp, "steep_area_min_diff": samd,
        "a_optics_xi_tree_ms": round(tree_ms, 4), "a_all": [round(t, 4) for t in tree_all],
        "b_copy_ms": round(copy_ms, 2), "b_host_walk_ms": round(walk_ms, 1),
        "c_optics_xi_ms": round(xi_ms, 4), "c_all": [round(t, 4) for t in xi_all],
        "a_over_b": round(tree_ms / (copy_ms + walk_ms), 5), "b_over_a": round((copy_ms + walk_ms) / tree_ms, 1),
        "a_over_c": round(tree_ms / xi_ms, 4),
        "pairs_total": int(counts.sum()), "pairs_max_per_window": int(counts.max()), "pair_cap": cap,
        "roots_total": int(g_roots.sum()), "deepest_level": deepest, "all_windows_identical": bool(match),
    })
(ROOT / "profiles").mkdir(exist_ok=True)
(ROOT / "profiles" / "optics_tree_probe.json").write_text(json.dumps(out) + "\n")
print(json.dumps(out))
