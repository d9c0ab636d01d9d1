"""Shared by tests/test_ref_cpu.py and tests/test_gpu_ref_cpu.py: the inputs of the reference pins,
and the reference's own answers to them.

The answers come from oracle/_ref/ref_cpu — the reference's CPU code (corner filter, tracker,
detection lambda, simple DBSCAN, AEClustering) compiled from the reference tree behind stand-in
headers by oracle/ref/Makefile — when that binary is built.  Where it is not (the reference tree
was absent at build time) they come from tests/golden/ref_cpu/<case>.npz: what the binary wrote
for the same inputs, stored by running the CPU module with ECC_RECORD_REF_GOLDEN=1 where it is
built.  Every fixture carries a SHA-256 of the generated input it answers, checked on load, so a
changed generator cannot be compared with stale answers.  With neither present a test fails.
A binary that another revision of oracle/ref/ref_cpu.cpp left in oracle/_ref/ (it is kept out of
git, and without the reference tree nothing rebuilds it) counts as not built: `ref_cpu api` must
answer REF_CPU_API.  A binary that answers no interface number at all fails the test.

The final time surface (7 MB) is kept in a fixture as its SHA-256 only; `same_surface` compares
whichever is at hand.
"""
import hashlib
import os
import struct
import subprocess
from pathlib import Path

import numpy as np

import arc_path_cases as ap

ROOT = Path(__file__).resolve().parent.parent
REF_CPU = ROOT / "oracle" / "_ref" / "ref_cpu"
GOLDEN = Path(__file__).resolve().parent / "golden" / "ref_cpu"
W, H = 1280, 720  # the reference's lambda hard-codes this border
SLICE = 16384


def sha(*parts):
    h = hashlib.sha256()
    for p in parts:
        h.update(np.ascontiguousarray(p).tobytes() if isinstance(p, np.ndarray) else repr(p).encode())
        h.update(b"|")
    return h.hexdigest()


REF_CPU_API = 2  # oracle/ref/ref_cpu.cpp:kRefCpuApi
_USABLE = {}


def ref_cpu_usable():
    """oracle/_ref/ref_cpu is there and was built from this tree's oracle/ref/ref_cpu.cpp: `ref_cpu api`
    answers REF_CPU_API.  oracle/_ref/ is kept out of git, so a binary of another revision can lie
    there where the reference tree is absent and nothing rebuilds it.  Only such a binary counts as
    not built (the recorded answers stand in, with a warning): one that answers another number, or
    interface 1, which has no `api` and declines it as an unknown subcommand with status 2.  A binary
    that answers anything else - nothing, no integer, a crash - fails the test."""
    if "ref_cpu" not in _USABLE:
        ok = False
        if REF_CPU.exists():
            r = subprocess.run([str(REF_CPU), "api"], capture_output=True, text=True, timeout=60)
            if r.returncode == 2 and r.stdout == "" and "unknown subcommand" in r.stderr:
                api = 1
            else:
                assert r.returncode == 0 and r.stdout.strip().isdigit(), \
                    f"{REF_CPU} api: status {r.returncode}, {r.stdout[-200:]!r}, {r.stderr[-200:]!r}"
                api = int(r.stdout)
            ok = api == REF_CPU_API
            if not ok:
                import warnings
                warnings.warn(f"{REF_CPU} has interface {api}, oracle/ref/ref_cpu.cpp {REF_CPU_API}: "
                              "the recorded answers of tests/golden/ref_cpu are used instead")
        _USABLE["ref_cpu"] = ok
    return _USABLE["ref_cpu"]


def _ref(case, tmp_path, sub, inputs, args, outputs, digest_only=(), exe=None, store=None, restore=None):
    """Runs `ref_cpu sub` (or loads the stored run).  inputs: {file name: array}; args: the argument
    list with input/output file NAMES in place of paths; outputs: {file name: dtype}.  Returns
    {output name: array}; an output in digest_only is returned whole from a live run and as
    <name>_sha always.  exe: another binary of oracle/_ref/ (tests/ref_optics_cases.py).  store /
    restore: the result dict -> the arrays a fixture keeps, and back (a smaller form of an output,
    which restore must prove equal to what was recorded)."""
    exe = REF_CPU if exe is None else exe
    key = sha(sub, [a for a in args if a not in inputs and a not in outputs],
              *[inputs[k] for k in sorted(inputs)])
    stored = GOLDEN / f"{case}.npz"
    if ref_cpu_usable() if exe == REF_CPU else exe.exists():
        d = tmp_path / f"ref_{case}"
        d.mkdir(exist_ok=True)
        for name, a in inputs.items():
            (d / name).write_bytes(np.ascontiguousarray(a).tobytes())
        argv = [str(d / a) if (a in inputs or a in outputs) else str(a) for a in args]
        r = subprocess.run([str(exe), sub] + argv, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        res = {name: np.frombuffer((d / name).read_bytes(), dt).copy() for name, dt in outputs.items()}
        for name in digest_only:
            res[name + "_sha"] = np.array(sha(res[name]))
        if os.environ.get("ECC_RECORD_REF_GOLDEN") == "1":
            GOLDEN.mkdir(parents=True, exist_ok=True)
            kept = {k: v for k, v in res.items() if k not in digest_only}
            np.savez_compressed(stored, input_sha=np.array(key), **(store(kept) if store else kept))
        return res
    assert stored.exists(), f"neither {exe} (reference tree absent at build time) nor {stored}"
    z = np.load(stored)
    assert str(z["input_sha"]) == key, f"{stored.name} answers another input: the generator changed, record it again"
    kept = {k: z[k] for k in z.files if k != "input_sha"}
    return restore(kept) if restore else kept


def same_surface(ref, got):
    """The reference's final time surface against `got` (int64[H*W])."""
    got = np.ascontiguousarray(got, np.int64)
    if "sae" in ref and not np.array_equal(ref["sae"], got):
        return False
    return str(ref["sae_sha"]) == sha(got)


# ---- lists files -----------------------------------------------------------------------------
def pack_lists(lists, rec):
    words = [len(lists)]
    for l in lists:
        l = np.asarray(l, np.int32).reshape(-1, rec)
        words.append(len(l))
        words.extend(l.ravel().tolist())
    return np.array(words, np.int32)


def unpack_lists(words, rec):
    p, out = 1, []
    for _ in range(int(words[0])):
        n = int(words[p])
        out.append(np.array(words[p + 1: p + 1 + n * rec], np.int32).reshape(n, rec))
        p += 1 + n * rec
    assert p == len(words)
    return out


def unpack_tracker(words):
    """ref_cpu's tracker dump -> per slice (tracks, groups); a track is a dict, floats as bit
    patterns; a group is (id, labels tuple, 5 float bit patterns)."""
    w = np.asarray(words, np.int32)
    u = w.view(np.uint32)
    p, out = 1, []
    for _ in range(int(w[0])):
        nt = int(w[p]); p += 1
        tracks = []
        for _ in range(nt):
            x, y, label, fc, matched, fsld, gid, hl = (int(v) for v in w[p:p + 8]); p += 8
            hist = tuple(int(v) for v in w[p:p + 2 * hl]); p += 2 * hl
            fb = tuple(int(v) for v in u[p:p + 8]); p += 8
            tracks.append(dict(x=x, y=y, label=label, frame_count=fc, is_matched=matched, fsld=fsld, group_id=gid,
                               hist=hist, fbits=fb[:6], damping=fb[6], smoothing=fb[7]))
        ng = int(w[p]); p += 1
        groups = []
        for _ in range(ng):
            gid, nl = int(w[p]), int(w[p + 1]); p += 2
            fb = tuple(int(v) for v in u[p:p + 5]); p += 5
            groups.append((gid, tuple(int(v) for v in w[p:p + nl]), fb)); p += nl
        out.append((tracks, groups))
    assert p == len(w)
    return out


def fbits(v):
    return struct.unpack("<I", struct.pack("<f", v))[0]


def track_key(t):
    """A reference track dict -> the comparable tuple (group_id only where the reference assigns it
    this slice: tracks detected this slice; a missed track keeps a stale id there)."""
    return (t["x"], t["y"], t["label"], t["frame_count"], t["is_matched"], t["fsld"], t["hist"], t["fbits"],
            t["group_id"] if t["fsld"] == 0 else None)


def struct_track_key(t):
    """An ecc_track (oracle or device) -> the same tuple."""
    hist = []
    for k in range(t.hist_len):
        hist += [t.hist_x[k], t.hist_y[k]]
    fsld = t.frames_since_last_detection
    return (t.x, t.y, t.label, t.frame_count, t.is_matched, fsld, tuple(hist),
            tuple(fbits(v) for v in (t.vx, t.vy, t.dir_cur_x, t.dir_cur_y, t.dir_tgt_x, t.dir_tgt_y)),
            t.group_id if fsld == 0 else None)


def struct_group_keys(groups, labels):
    return [(g.id, tuple(int(v) for v in labels[g.first_label_offset: g.first_label_offset + g.n_labels]),
             tuple(fbits(v) for v in (g.avg_vx, g.avg_vy, g.cx, g.cy, g.radius))) for g in groups]


# ---- reference runs ----------------------------------------------------------------------------
def ref_arc(case, tmp_path, xy, t, slice_events=SLICE, flag0=0, sae0=None):
    """The verbatim lambda once per slice -> {corners: per-slice (k, 2) arrays, sae / sae_sha}."""
    inputs = {"xy.u32": np.ascontiguousarray(xy, np.uint32), "t.i64": np.ascontiguousarray(t, np.int64)}
    if sae0 is not None:
        inputs["sae0.i64"] = np.ascontiguousarray(sae0, np.int64)
    r = _ref(case, tmp_path, "arc", inputs,
             ["xy.u32", "t.i64", slice_events, flag0, "sae0.i64" if sae0 is not None else "-", "corners.i32", "sae"],
             {"corners.i32": np.int32, "sae": np.int64}, digest_only=("sae",))
    r["corners"] = unpack_lists(r["corners.i32"], 2)
    return r


def ref_chain(case, tmp_path, xy, t, slice_events=SLICE):
    r = _ref(case, tmp_path, "chain",
             {"xy.u32": np.ascontiguousarray(xy, np.uint32), "t.i64": np.ascontiguousarray(t, np.int64)},
             ["xy.u32", "t.i64", slice_events, "corners.i32", "nms.i32", "track.i32", "sae"],
             {"corners.i32": np.int32, "nms.i32": np.int32, "track.i32": np.int32, "sae": np.int64},
             digest_only=("sae",))
    r["corners"] = unpack_lists(r["corners.i32"], 2)
    r["nms"] = unpack_lists(r["nms.i32"], 3)
    r["track"] = unpack_tracker(r["track.i32"])
    return r


def ref_nms(case, tmp_path, lists):
    r = _ref(case, tmp_path, "nms", {"in.i32": pack_lists(lists, 2)}, ["in.i32", W, H, "out.i32"],
             {"out.i32": np.int32})
    return unpack_lists(r["out.i32"], 3)


def cfg_words(cfg):
    """A tracker configuration (max_distance, max_frames, history_size, frames_to_skip, damping,
    smoothing, group_radius) as ref_cpu's argument: seven hex words, the floats as bit patterns."""
    md, mf, hs, fts, da, sm, gr = cfg
    return ",".join("%08x" % w for w in (fbits(md), mf & 0xffffffff, hs & 0xffffffff, fts & 0xffffffff,
                                        fbits(da), fbits(sm), fbits(gr)))


def ref_track(case, tmp_path, lists3, cfg=None):
    """cfg=None: the reference's own CornerTracker(30, 30, 10, 5, 0.8, 0.3, 100); else the seven
    constructor arguments, which enter the fixture's input hash."""
    args = ["in.i32", "out.i32"] + ([cfg_words(cfg)] if cfg is not None else [])
    r = _ref(case, tmp_path, "track", {"in.i32": pack_lists(lists3, 3)}, args, {"out.i32": np.int32})
    return unpack_tracker(r["out.i32"])


def ref_dbscan(case, tmp_path, pts3, eps, min_pts, min_size, max_size):
    r = _ref(case, tmp_path, "dbscan", {"pts.f32": np.ascontiguousarray(pts3, np.float32)},
             ["pts.f32", repr(float(eps)), min_pts, min_size, max_size, "out.i32"], {"out.i32": np.int32})
    w = r["out.i32"]
    nc = int(w[0])
    sizes = w[1:1 + nc]
    offs = 1 + nc + np.concatenate([[0], np.cumsum(sizes)])
    return [w[offs[c]:offs[c + 1]].copy() for c in range(nc)]


def ref_aec(case, tmp_path, feed, wins):
    """-> per window a list of (id, n, centroid x, y, mu x, y) in cluster-deque order."""
    r = _ref(case, tmp_path, "aec", {"feed.f64": np.ascontiguousarray(feed, np.float64),
                                     "wins.i32": np.ascontiguousarray(wins, np.int32)},
             ["feed.f64", "wins.i32", "out.f64"], {"out.f64": np.float64})
    return unpack_aec(r["out.f64"], len(wins))


def unpack_aec(o, n_windows):
    p, out = 0, []
    for _ in range(n_windows):
        nc = int(o[p]); p += 1
        out.append([tuple(o[p + 6 * c: p + 6 * c + 6]) for c in range(nc)])
        p += 6 * nc
    assert p == len(o)
    return out


# ---- event streams (1280 x 720) --------------------------------------------------------------
def is_border(x, y):
    return (x < 4) | (x >= W - 4) | (y < 4) | (y >= H - 4)


def stream_plain(ecc, n, seed):
    xy, t, _ = ecc.gen_events(n, seed=seed, width=W, height=H)
    return xy, t


def stream_interior(ecc, n, seed):
    """The first n events of the synthetic stream that are no border events (still time-sorted)."""
    xy, t, _ = ecc.gen_events(n + n // 4, seed=seed, width=W, height=H)
    x, y = ecc.unpack_xy(xy)
    keep = np.nonzero(~is_border(x, y))[0][:n]
    assert len(keep) == n
    return xy[keep].copy(), t[keep].copy()


BORDER_AT = ((1, 9000, 2, 300), (3, 12000, 1279, 10), (4, 2000, 640, 719), (5, SLICE - 1, 0, 0))


def stream_border_mid(ecc, n, seed, slice_events=SLICE):
    """stream_interior with single border events planted inside slices 1, 3, 4 and as the last event
    of slice 5: the reference's `break` cuts those slices' tests off there."""
    xy, t = stream_interior(ecc, n, seed)
    for s, k, x, y in BORDER_AT:
        xy[s * slice_events + k] = x | (y << 16)
    return xy, t


def stream_ties(ecc, n, seed, quantum):
    """stream_interior with timestamps rounded down to multiples of `quantum`: long runs of equal
    timestamps, so circle pixels tie (`<` against `>=` in the reference's comparisons)."""
    xy, t = stream_interior(ecc, n, seed)
    return xy, (t // quantum) * quantum


def stream_2p53(ecc, n, seed, cross_at, slice_events=SLICE, bursts_per_slice=150):
    """Timestamps 1-3 ticks apart (odd and even gaps) that pass 2^53 at event `cross_at`: above 2^53
    a double holds even integers only, so neighbouring timestamps round together there.
    For circle neighbours to BE neighbours in time, the pixels are stream_interior's with bursts
    planted over them: 37 consecutive events that write the 36 pixels of both circles around a
    centre — first those outside a chosen arc of each circle, then the arcs — and then the centre.
    In int64 each arc is newer than the rest of its circle by a tick or a few; in double the
    boundary often ties."""
    xy, _ = stream_interior(ecc, n, seed)
    rng = np.random.default_rng(seed)
    for lo in range(0, n, slice_events):
        slots = rng.choice((min(n, lo + slice_events) - lo) // 40, bursts_per_slice, replace=False)
        for k in slots:
            cx, cy = int(rng.integers(8, W - 8)), int(rng.integers(8, H - 8))
            i0, s3, j0, s4 = rng.integers(0, 16), rng.integers(3, 7), rng.integers(0, 20), rng.integers(4, 9)
            arc = [C3[(i0 + a) % 16] for a in range(s3)] + [C4[(j0 + a) % 20] for a in range(s4)]
            rest = [c for c in C3 + C4 if c not in arc]
            order = [rest[i] for i in rng.permutation(len(rest))] + [arc[i] for i in rng.permutation(len(arc))]
            burst = [(cx + dx) | ((cy + dy) << 16) for dy, dx in order] + [cx | (cy << 16)]
            xy[lo + 40 * k: lo + 40 * k + 37] = burst
    gaps = rng.integers(1, 4, n).astype(np.int64)
    rel = np.cumsum(gaps)
    return xy, (1 << 53) - rel[cross_at] + rel


ARC_CASES = ("gen", "border_mid", "interior", "sae0", "ties", "groups40", "raster", "future_sae", "neg_time")
PATCH, PATCH_B = (600, 300), (700, 400)  # where the 56 x 42 streams of tests/arc_path_cases.py sit in the frame
PARK = (100, 100)                        # their off-sensor events: one interior pixel far from the patches


def at_patch(xy, origin):
    """An arc_path_cases stream's pixels moved to `origin`; its events off the 56 x 42 sensor to PARK."""
    x, y = ap.unpack(xy)
    on = (x < ap.W) & (y < ap.H)
    return ap.pack(np.where(on, x + origin[0], PARK[0]), np.where(on, y + origin[1], PARK[1]))


def patch_surface(sae, small, origin):
    sae.reshape(H, W)[origin[1]: origin[1] + ap.H, origin[0]: origin[0] + ap.W] = small.reshape(ap.H, ap.W)
_arc_cache = {}


def arc_case(ecc, name):
    """name -> dict(xy, t, slice, first (first_detect_slice), sae0)."""
    if name in _arc_cache:
        return _arc_cache[name]
    n, sl, first, sae0 = 6 * SLICE, SLICE, 1, None
    if name == "gen":            # the synthetic stream as it comes: border events end most slices early
        xy, t = stream_plain(ecc, n, 1)
    elif name == "border_mid":   # border events in the middle of four slices
        xy, t = stream_border_mid(ecc, n, 2)
    elif name == "interior":     # none: border_mode 0 and 1 agree
        xy, t = stream_interior(ecc, n, 2)
    elif name == "sae0":         # a surface from earlier events, detection from the first slice on
        xy, t = stream_interior(ecc, n, 3)
        rng = np.random.default_rng(3)
        sae0 = rng.integers(int(t[0]) - 4000, int(t[0]) + 2000, W * H).astype(np.int64)
        sae0[rng.random(W * H) < 0.3] = 0
        first = 0
    elif name == "ties":
        xy, t = stream_ties(ecc, n, 4, 64)
    elif name == "groups40":     # 40 slices: two of the device's 32-slice groups
        sl = 4096
        xy, t = stream_interior(ecc, 40 * sl, 5)
    elif name == "raster":       # arc_path_cases.queue_full: more corners in a tile and group than the arc kernels queue
        c = ap.queue_full()
        xy, t, sl, first = at_patch(c["xy"], PATCH), c["t"], c["S"], 0
    elif name == "future_sae":   # arc_path_cases.future_sae c (up to INT64_MAX) at PATCH and d (down to INT64_MIN) at PATCH_B
        c, d = ap.future_sae("c", extra=2), ap.future_sae("d", extra=2)
        sl, first = 2 * c["S"], 0
        xy = np.stack([at_patch(c["xy"], PATCH).reshape(-1, c["S"]), at_patch(d["xy"], PATCH_B).reshape(-1, d["S"])],
                      1).reshape(-1)  # every slice: c's events, then d's (they share no pixel)
        t = ap.rising(len(xy), seed=21)
        sae0 = np.zeros(W * H, np.int64)
        patch_surface(sae0, c["sae0"], PATCH)
        patch_surface(sae0, d["sae0"], PATCH_B)
    elif name == "neg_time":     # arc_path_cases.negative_time: crosses zero inside a slice, over a zero surface
        c = ap.negative_time("cross_zero", extra=3)
        xy, t, sl, first = at_patch(c["xy"], PATCH), c["t"], c["S"], 0
    elif name == "t53":          # passes 2^53 in the middle of slice 2
        xy, t = stream_2p53(ecc, n, 6, 2 * SLICE + 8000)
    elif name == "t53_groups40":  # group 0 below 2^53, group 1 passes it
        sl = 4096
        xy, t = stream_2p53(ecc, 40 * sl, 7, 35 * sl + 1000)
    else:
        raise KeyError(name)
    _arc_cache[name] = dict(xy=xy, t=t, slice=sl, first=first, sae0=sae0)
    return _arc_cache[name]


def final_surface(xy, t, sae0=None):
    """Last writer per pixel (the stream is time-sorted, so the last writer holds the maximum)."""
    sae = np.zeros(W * H, np.int64) if sae0 is None else np.array(sae0, np.int64)
    q = (xy >> 16).astype(np.int64) * W + (xy & 0xffff).astype(np.int64)
    last = np.full(W * H, -1, np.int64)
    np.maximum.at(last, q, np.arange(len(q), dtype=np.int64))
    hit = last >= 0
    sae[hit] = t[last[hit]]
    return sae


def slice_corners_from_flags(ecc, xy, flags, slice_events):
    """Flagged events per slice as (k, 2) (x, y) arrays in event order: the reference's `corners`."""
    x, y = ecc.unpack_xy(xy)
    out = []
    for lo in range(0, len(xy), slice_events):
        f = np.nonzero(flags[lo:lo + slice_events])[0] + lo
        out.append(np.stack([x[f], y[f]], 1).astype(np.int32).reshape(-1, 2))
    return out


def same_lists(a, b):
    return len(a) == len(b) and all(np.array_equal(p, q) for p, q in zip(a, b))


C3 = [(0, 3), (1, 3), (2, 2), (3, 1), (3, 0), (3, -1), (2, -2), (1, -3), (0, -3), (-1, -3), (-2, -2), (-3, -1),
      (-3, 0), (-3, 1), (-2, 2), (-1, 3)]
C4 = [(0, 4), (1, 4), (2, 3), (3, 2), (4, 1), (4, 0), (4, -1), (3, -2), (2, -3), (1, -4), (0, -4), (-1, -4),
      (-2, -3), (-3, -2), (-4, -1), (-4, 0), (-4, 1), (-3, 2), (-2, 3), (-1, 4)]


def arc_int64(sae2d, x, y):
    """The arc test in pure int64 (numpy): a contiguous arc of s values, each greater than every
    value outside it, s in 3..6 on circle 3 and in 4..8 on circle 4."""
    def circle(c, smin, smax):
        v = np.array([sae2d[y + dy, x + dx] for dy, dx in c], np.int64)
        cnt = np.array([(v > v[j]).sum() for j in range(len(v))])
        for s in range(smin, smax + 1):
            m = cnt < s
            if m.sum() == s and (m & ~np.roll(m, 1)).sum() == 1:
                return True
        return False
    return circle(C3, 3, 6) and circle(C4, 4, 8)


# ---- NMS candidates ----------------------------------------------------------------------------
def nms_slices():
    rng = np.random.default_rng(5)
    edges = [(0, 0), (W - 1, H - 1), (7, 7), (W - 8, H - 8), (0, 360), (640, 0), (W - 1, 300), (700, H - 1),
             (5, 100), (W - 5, 200), (300, 4), (400, H - 5), (3, 114), (W - 3, 215), (314, 2), (415, H - 2),
             (6, 500), (21, 500), (W - 7, 600), (W - 22, 600), (900, 6), (900, 22), (1000, H - 7), (1000, H - 23)]
    dup = [(100, 100)] * 5 + [(300, 300), (100, 100), (300, 300), (114, 114), (115, 115)]
    chains = ([(100 + 7 * k, 200) for k in range(12)] + [(100 + 8 * k, 260) for k in range(12)] +
              [(100 + 14 * k, 320) for k in range(8)] + [(100 + 15 * k, 380) for k in range(8)] +
              [(100 + 16 * k, 440) for k in range(8)] + [(800, 100 + 7 * k) for k in range(12)] +
              [(860, 100 + 8 * k) for k in range(12)] + [(920, 100 + 15 * k) for k in range(8)])
    pairs = [(500, 500), (507, 500), (600, 500), (608, 500), (700, 500), (707, 507), (800, 500), (814, 514),
             (900, 500), (915, 500), (1000, 500), (1000, 515), (1100, 500), (1114, 515)]
    rev = [p for k in range(0, len(pairs), 2) for p in (pairs[k + 1], pairs[k])]
    wide = np.stack([rng.integers(0, W, 4096), rng.integers(0, H, 4096)], 1)
    dense = np.stack([rng.integers(500, 760, 4096), rng.integers(200, 420, 4096)], 1)
    return [np.array(s, np.int32).reshape(-1, 2) for s in (edges, dup, chains, pairs, rev, [], wide, dense)]


NMS_SLICE = 4096


def nms_as_events(lists):
    """The candidate lists as an event array with flags for ecc_corner_nms: slices of NMS_SLICE
    events, a slice's candidates first, the rest unflagged filler."""
    xy = np.full(len(lists) * NMS_SLICE, 640 | (360 << 16), np.uint32)
    flags = np.zeros(len(xy), np.uint8)
    for s, l in enumerate(lists):
        assert len(l) <= NMS_SLICE
        xy[s * NMS_SLICE: s * NMS_SLICE + len(l)] = l[:, 0].astype(np.uint32) | (l[:, 1].astype(np.uint32) << 16)
        flags[s * NMS_SLICE: s * NMS_SLICE + len(l)] = 1
    return xy, flags


# ---- tracker detections ------------------------------------------------------------------------
TRACK_SLICES = 60


def tracker_slices(seed=1):
    """60 slices of detections (x, y, label = rank, as the NMS emits them) of 5-40 moving centres:
    random movers with dropouts and limited lives, long-lived ones (frame_count passes 30, the
    history wraps), movers that leave through an image edge and vanish (the miss path predicts on,
    out of the frame), and a resting centre replaced by two detections at equal distance."""
    rng = np.random.default_rng(seed)
    centres = []  # (birth, death, x0, y0, vx, vy, p_drop)
    for k in range(4):  # long-lived, never dropped
        centres.append((0, TRACK_SLICES, 200 + 250 * k, 150 + 90 * k, 2.5 - k, 1.5 * (k % 2) - 0.5, 0.0))
    for k in range(60):  # movers
        b = int(rng.integers(0, 50))
        centres.append((b, b + int(rng.integers(4, 30)), float(rng.uniform(60, W - 60)), float(rng.uniform(60, H - 60)),
                        float(rng.uniform(-9, 9)), float(rng.uniform(-9, 9)), 0.2))
    for k, (x0, y0, vx, vy) in enumerate([(40, 200, -13, 1), (W - 45, 300, 14, -2), (500, 35, 2, -12),
                                          (800, H - 40, -1, 13), (30, 30, -11, -11), (W - 35, H - 30, 12, 11)]):
        centres.append((5 + 7 * k, 5 + 7 * k + 3, x0, y0, vx, vy, 0.0))  # three detections, then gone
    centres.append((10, 15, 1150, 660, 0, 0, 0.0))  # resting, replaced at slice 15 by two detections 10 px either side
    centres.append((15, 22, 1140, 660, 0, 0, 0.0))
    centres.append((15, 22, 1160, 660, 0, 0, 0.0))
    alive_cap = np.linspace(5, 40, TRACK_SLICES).astype(int)
    out = []
    for s in range(TRACK_SLICES):
        det = []
        for b, d, x0, y0, vx, vy, pd in centres:
            if not (b <= s < d) or (pd and rng.random() < pd):
                continue
            x, y = int(round(x0 + vx * (s - b))), int(round(y0 + vy * (s - b)))
            if 0 <= x < W and 0 <= y < H and (x, y) not in det:
                det.append((x, y))
        scripted = [p for p in det if p in ((1150, 660), (1140, 660), (1160, 660))]
        rest = [p for p in det if p not in scripted][:max(0, alive_cap[s] - len(scripted))]
        det = rest[:len(rest) // 2] + scripted + rest[len(rest) // 2:]
        out.append(np.array([(x, y, k) for k, (x, y) in enumerate(det)], np.int32).reshape(-1, 3))
    return out


def tracker_counters(lists3, dump):
    """What the stream exercises, counted from the reference's own dump."""
    c = dict(miss_outside=0, removed_frames=0, removed_misses=0, hist_wrapped=0, equidistant=0, multi_groups=0,
             interleaved_groups=0, first_not_lowest=0)
    prev = {}
    for s, (tracks, groups) in enumerate(dump):
        cur = {t["label"]: t for t in tracks}
        for t in tracks:
            if t["fsld"] > 0 and (t["x"] < 0 or t["y"] < 0 or t["x"] >= W or t["y"] >= H):
                c["miss_outside"] += 1
            p = prev.get(t["label"])
            if p is not None and len(p["hist"]) == 20 and len(t["hist"]) == 20:
                c["hist_wrapped"] += 1
        for lab, p in prev.items():
            if lab not in cur:
                if p["frame_count"] == 30 and p["fsld"] < 5:
                    c["removed_frames"] += 1
                if p["fsld"] == 5 and p["frame_count"] < 30:
                    c["removed_misses"] += 1
            # a track at rest (detected, zero velocity) predicts exactly its own pixel
            if p["fsld"] == 0 and p["fbits"][0] in (0, 0x80000000) and p["fbits"][1] in (0, 0x80000000):
                d2 = sorted((int(x) - p["x"]) ** 2 + (int(y) - p["y"]) ** 2 for x, y, _ in lists3[s])
                if len(d2) >= 2 and d2[0] == d2[1] and d2[0] < 900:
                    c["equidistant"] += 1
        for gid, labels, _ in groups:
            c["multi_groups"] += len(labels) > 1
            c["first_not_lowest"] += labels[0] != min(labels)
        order = [t["label"] for t in tracks if t["fsld"] == 0]
        for gid, labels, _ in groups:
            idx = [order.index(l) for l in labels]
            c["interleaved_groups"] += (max(idx) - min(idx) + 1) != len(idx)
        prev = cur
    return c


# ---- DBSCAN cloud ------------------------------------------------------------------------------
DBSCAN_EPS, DBSCAN_MIN_PTS, DBSCAN_MIN_SIZE, DBSCAN_MAX_SIZE = 3.0, 8, 40, 600


def dbscan_points():
    """~3000 integer-pixel points (z = 0; exact in float, so the device's integer-window path sees
    the same cloud): lattice patches whose neighbours at (3, 0) lie exactly at eps, two clusters of
    equal size, one above max_size and one below min_size (both dropped), a sparse bridge point
    that borders two clusters and is a neighbour of the later cluster's seed (a double membership),
    chains of points exactly eps apart, and noise."""
    rng = np.random.default_rng(9)
    pts = []

    def patch(x0, y0, w, h, step=1):
        return [(x0 + step * i, y0 + step * j) for j in range(h) for i in range(w)]

    pts += patch(100, 100, 20, 15)             # A: 300 points
    pts += [(122, 100)]                        # bridge: exactly eps right of A's corner (119, 100) ... and
    pts += patch(125, 100, 20, 15)             # B: 300 points, its seed (125, 100) exactly eps from the bridge
    pts += patch(300, 100, 30, 25)             # C: 750 points > max_size
    pts += patch(500, 100, 6, 5)               # D: 30 points < min_size
    pts += patch(100, 300, 25, 12, step=2)     # E: spacing 2: (2, 2) neighbours inside eps, (4, 0) outside
    pts += patch(400, 300, 12, 25, step=2)     # F: the same size as E, transposed
    pts += [(700 + 3 * k, 300) for k in range(60)]   # a chain exactly eps apart: 3 in each ball, never core
    pts += patch(700, 400, 40, 3, step=3)      # 3 rows exactly eps apart: 5 in a ball (min_pts 8: noise) ...
    pts += patch(700, 500, 40, 3) + patch(700, 505, 40, 3)  # two strips whose facing rows are exactly eps apart: joined
    blob = np.unique(np.round(rng.normal((1000, 200), 9, (700, 2))).astype(int), axis=0)
    pts += [tuple(p) for p in blob]
    built = np.array(pts, np.int64)
    noise = np.stack([rng.integers(0, W, 400), rng.integers(0, H, 400)], 1)
    far = np.array([np.abs(built - q).max(1).min() > 10 for q in noise])  # noise keeps clear of the built shapes
    pts += [tuple(q) for q in noise[far]]
    p = np.array(pts, np.int32)
    out = np.zeros((len(p), 3), np.float32)
    out[:, :2] = p
    return out


def dbscan_float_points():
    """A second cloud with fractional float coordinates and a real z axis (the reference's own input
    type): quarter-pixel lattices whose (0.75, 0, 0) x 4 neighbours sit exactly at eps = 3, Gaussian
    blobs and noise."""
    rng = np.random.default_rng(10)
    a = np.array([(50 + 0.75 * i, 50 + 0.75 * j, 0.75 * k) for k in range(4) for j in range(12) for i in range(12)])
    b = rng.normal((200, 80, 5), (6, 6, 2), (900, 3))
    c = rng.normal((230, 80, 5), (5, 5, 2), (700, 3))
    d = rng.uniform((0, 0, 0), (400, 200, 10), (400, 3))
    return np.concatenate([a, b, c, d]).astype(np.float32)


def clusters_from_labels(n, lab, dups, nc):
    members = [[] for _ in range(nc)]
    for i in np.nonzero(lab[:n] >= 0)[0]:
        members[lab[i]].append(int(i))
    for p, c in dups:
        members[c].append(int(p))
    return [np.array(sorted(m), np.int32) for m in members]


# ---- AEClustering feed -------------------------------------------------------------------------
def aec_feed(rep_xy, win_unique, stride=8192):
    """The downsample -> clusterer hand-off of DSA/…opencl_store.cpp:435-445: per window the
    representatives k = 0, 2, 4, … with 2k < unique (the i += 4 walk over interleaved ints), each
    as (cumulative unique / 1000, x, y).  -> (feed (m, 3) float64, updates per window)."""
    feed, wins, cumulative = [], [], 0
    for w, diff in enumerate(int(v) for v in win_unique):
        cumulative += diff
        k = 0
        for i in range(0, diff, 4):
            v = int(rep_xy[w * stride + i // 2])
            feed.append((cumulative / 1000.0, float(v & 0xffff), float(v >> 16)))
            k += 1
        wins.append(k)
    return np.array(feed, np.float64).reshape(-1, 3), np.array(wins, np.int32)


def aec_rows(per_window, min_n=10):
    """The slice callback's centroid flow (:466-517) over a cluster dump: rows (window, id, n, cx, cy,
    has_prev, dx, dy) as orc.aec_run lists them, and the clusters per window."""
    prev = {}
    rows, cpw = [], []
    for w, clusters in enumerate(per_window):
        cpw.append(len(clusters))
        for cid, n, cx, cy, _, _ in clusters:
            if n < min_n:
                continue
            px, py = prev.get(int(cid) % 16384, (0.0, 0.0))
            rows.append((float(w), cid, n, cx, cy, 1.0 if (px > 0 and py > 0) else 0.0, cx - px, cy - py))
            prev[int(cid) % 16384] = (cx, cy)
    return np.array(rows, np.float64).reshape(-1, 8), np.array(cpw, np.int32)
