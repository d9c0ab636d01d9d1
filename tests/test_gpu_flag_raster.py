"""The flag pass's raster corner bitmap, scanned candidate ranks and staging list
(csrc/corner_flags.hip, csrc/flag_raster.hpp), at the smallest shapes where they can go wrong.  Every
case compares exactly with the oracle (orc.fast_detect / orc.corner_nms) on every entry point —
ecc_fast_detect, prepare + finish, ecc_fast_detect_nms, prepare + ecc_fast_detect_finish_nms, and
finish + ecc_corner_nms — with output buffers that start as 0xCD.

The streams are built, not drawn: the oracle tests a slice's events against the SAE at the slice's
END, so pixel p is a corner of a slice whose last events lay four consecutive pixels of p's circle
of radius 3 and five of its circle of radius 4 (a streak newer than the rest of either circle), and
every event of the slice at p is then flagged, wherever it stands in the slice.  Each case asserts
on the oracle's own flags that every class it targets holds a flagged event.

  * Row pitch: sensors 33x29, 64x28 (rows word-aligned, tile columns not), 45x31 and 346x260; a
    corner in a tile's first and last pixel column and row (its raster neighbours belong to other
    tiles, and carry events too), in each of the seven segment words (192..195 included), and in
    the partial last tile row and column where the sensor's interior reaches them.
  * Batches: slices of 8192 (one batch), 8196 (a second batch of one quad), 12288 and 16384 events
    with a last slice of 4093..4095; flagged events in both batches and at every quad position.
  * Variants: first_detect_slice 0 and 2, border_mode 1 with the first border event in the second
    batch, a flags pointer offset by 1..3 bytes, a few per cent of the events off the sensor.
  * 1280x720 with two slices of 4096 events: a raster bitmap of 115200 B (the dynamic-LDS opt-in).
  * A slice with no corner, and one whose every event is a corner of one pixel (16384 candidates).
  * A slice with more corner words than the staging list holds.
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

BOX, CAP = 15, 256
# {dy, dx} of the first four pixels of the radius-3 circle and the first five of the radius-4 one
STREAK3 = [(0, 3), (1, 3), (2, 2), (3, 1)]
STREAK4 = [(0, 4), (1, 4), (2, 3), (3, 2), (4, 1)]
STAMP = len(STREAK3) + len(STREAK4)
TAIL = 12


def dev(ecc, a):
    return ecc.DeviceArray.from_numpy(np.ascontiguousarray(a))


def cd(ecc, n, dtype):
    d = ecc.DeviceArray(n, dtype)
    d.fill_bytes(0xCD)
    return d


# ------------------------------------------------------------------------------------ the streams
def build_slice(S, targets, fill, off_sensor=None):
    """S events as (x, y) lists: a body that cycles through every target, its four raster
    neighbours and the `fill` pixels (an odd period, so each of them falls on every position of a
    quad), then the targets' stamps, then TAIL more events at the targets (an event at p is on
    none of p's circles), so that the slice's last quads and its scalar tail hold flagged events
    too.  off_sensor = (W, H): every 29th body event that is no target's own goes off the sensor
    (x >= W, y >= H, 65535)."""
    cycle = []
    for (x, y) in targets:
        cycle += [(x, y), (x + 1, y), (x, y), (x - 1, y), (x, y + 1), (x, y), (x, y - 1)]
    cycle += list(fill)
    if len(cycle) % 2 == 0:
        cycle.append(fill[0])
    body = S - STAMP * len(targets) - TAIL
    assert body >= 2 * len(cycle)
    ev = [cycle[i % len(cycle)] for i in range(body)]
    if off_sensor is not None:
        W, H = off_sensor
        away = [(W + 3, 5), (5, H + 7), (65535, 6), (6, 65535), (65535, 65535), (W, H)]
        k = 0
        for i in range(3, body, 29):
            j = next(j for j in range(i, body) if ev[j] not in targets)
            ev[j] = away[k % len(away)]
            k += 1
    for (x, y) in targets:
        ev += [(x + dx, y + dy) for dy, dx in STREAK3] + [(x + dx, y + dy) for dy, dx in STREAK4]
    ev += [targets[i % len(targets)] for i in range(TAIL)]
    assert len(ev) == S
    return ev


def to_stream(ecc, slices):
    ev = [p for sl in slices for p in sl]
    x = np.array([p[0] for p in ev], np.int64)
    y = np.array([p[1] for p in ev], np.int64)
    return ecc.pack_xy(x, y), np.arange(1, len(ev) + 1, dtype=np.int64) * 3, x, y


def pixel_classes(W, H):
    """class name -> predicate on (x, y), for the classes the sensor's interior can reach."""
    cls = {"col0": lambda x, y: x % 14 == 0, "col13": lambda x, y: x % 14 == 13,
           "row0": lambda x, y: y % 14 == 0, "row13": lambda x, y: y % 14 == 13}
    for k in range(7):  # word 6 is tile pixels 192..195
        cls[f"word{k}"] = lambda x, y, k=k: ((y % 14) * 14 + x % 14) // 32 == k
    if W % 14 and 14 * (W // 14) <= W - 5:
        cls["last_col"] = lambda x, y: x >= 14 * (W // 14)
    if H % 14 and 14 * (H // 14) <= H - 5:
        cls["last_row"] = lambda x, y: y >= 14 * (H // 14)
    return cls


def class_targets(W, H):
    """One interior pixel per class (the last in raster order, so the classes differ)."""
    interior = [(x, y) for y in range(4, H - 4) for x in range(4, W - 4)]
    return {name: [p for p in interior if f(*p)][-1] for name, f in pixel_classes(W, H).items()}


def assert_classes(o_flags, x, y, W, H, names):
    o = o_flags.astype(bool)
    for name in names:
        f = pixel_classes(W, H)[name]
        hit = np.array([f(int(a), int(b)) for a, b in zip(x[o], y[o])], bool)
        assert hit.any(), f"{W}x{H}: the oracle flags no corner of class {name}"


def pitch_stream(ecc, W, H, S=1024):
    """One slice per class of the sensor, its target's corner planted in it."""
    tg = class_targets(W, H)
    fill = [(W // 2, H // 2), (5, 5)]
    slices = [build_slice(S, [p], fill, off_sensor=(W, H)) for p in tg.values()]
    return to_stream(ecc, slices) + (list(tg),)


def spread_targets(W, H, k):
    """k interior pixels at least 9 apart (the stamps and circles of two never touch)."""
    out = [(x, y) for y in range(9, H - 9, 23) for x in range(11, W - 9, 37)]
    return out[:k]


def batch_stream(ecc, W, H, S, last, border_at=None, off_sensor=True):
    """Three slices of S events and one of `last`, six corners in each; border_at: an event at
    x = 1 at that index of every slice."""
    tg = spread_targets(W, H, 6)
    fill = [(W - 20, H - 20), (W // 2 + 3, 7)]
    slices = [build_slice(n, tg, fill, off_sensor=(W, H) if off_sensor else None) for n in (S, S, S, last)]
    if border_at is not None:
        for sl in slices:
            if border_at < len(sl) - STAMP * len(tg):
                sl[border_at] = (1, H // 2)
    return to_stream(ecc, slices)


# -------------------------------------------------------------------------------- the comparison
def check_entries(ecc, orc, ctx, xy, t, W, H, S, offsets=(0,), CAP=CAP, **kw):
    """Every entry point against the oracle; returns the oracle's flags."""
    n = len(xy)
    cfg = ecc.corner_cfg(width=W, height=H, slice_events=S, border_mode=kw.get("border_mode", 0),
                         first_detect_slice=kw.get("first_detect", 1))
    o_flags, o_sae = orc.fast_detect(xy, t, W, H, slice_events=S, **kw)
    o_out, o_cnt, rc = orc.corner_nms(xy, o_flags, W, H, slice_events=S, box=BOX, cap=CAP)
    assert rc == 0
    ns = len(o_cnt)
    L = ecc.lib
    d_xy, d_t = dev(ecc, xy), dev(ecc, t)
    args = (ctx.ctx, d_xy.ptr, d_t.ptr, n, C.byref(cfg))

    def nms_equal(out, cnt, what):
        assert ctx.corner_nms_status() == 0, what
        assert (cnt.numpy() == o_cnt).all(), what
        g_out = out.numpy()
        for s in range(ns):
            assert (g_out[s * CAP: s * CAP + o_cnt[s]] == o_out[s * CAP: s * CAP + o_cnt[s]]).all(), (what, s)

    for entry in ("detect", "prepare_finish", "detect_nms", "prepare_finish_nms"):
        for off in offsets:
            what = f"{entry}, flags + {off}"
            sae = dev(ecc, np.zeros(W * H, np.int64))
            buf = cd(ecc, n + 8, np.uint8)  # flags at buf + off: every flag written, nothing around them
            out, cnt = cd(ecc, ns * CAP, ecc.CORNER_DTYPE), cd(ecc, ns, np.int32)
            if entry.startswith("prepare"):
                local = cd(ecc, W * H, np.int64)
                ecc.check(L.ecc_fast_detect_prepare(*args, local.ptr, ctx.stream), what)
            if entry == "detect":
                ecc.check(L.ecc_fast_detect(*args, sae.ptr, buf.ptr + off, ctx.stream), what)
            elif entry == "prepare_finish":
                ecc.check(L.ecc_fast_detect_finish(*args, sae.ptr, buf.ptr + off, ctx.stream), what)
            elif entry == "detect_nms":
                ecc.check(L.ecc_fast_detect_nms(*args, sae.ptr, buf.ptr + off, BOX, CAP, out.ptr, cnt.ptr, ctx.stream), what)
            else:
                ecc.check(L.ecc_fast_detect_finish_nms(*args, sae.ptr, buf.ptr + off, BOX, CAP, out.ptr, cnt.ptr,
                                                       ctx.stream), what)
            assert ctx.fast_detect_status() == 0, what
            g = buf.numpy()
            bad = int((g[off:off + n] != o_flags).sum())
            assert bad == 0, f"{what}: {bad} corner labels differ"
            assert (g[:off] == 0xCD).all() and (g[off + n:] == 0xCD).all(), f"{what}: wrote outside"
            assert (sae.numpy() == o_sae).all(), what
            if entry.endswith("nms"):
                nms_equal(out, cnt, what)
            elif entry == "prepare_finish" and off == 0:
                # the sharded step's tail: finish, then ecc_corner_nms over the flags it wrote
                flags = dev(ecc, g[:n])
                ctx.corner_nms(d_xy, flags, n, S, W, H, BOX, CAP, out, cnt)
                nms_equal(out, cnt, "finish + corner_nms")
    return o_flags


# ----------------------------------------------------------------------------------------- cases
@pytest.mark.parametrize("wh", [(33, 29), (64, 28), (45, 31), (346, 260)], ids=lambda wh: f"{wh[0]}x{wh[1]}")
def test_row_pitch_and_tile_edges(ecc, orc, gpu, wh):
    """Rows that straddle the raster's words differently; corners whose raster neighbours belong
    to other tiles, in every segment word, and in the partial edge tiles."""
    W, H = wh
    xy, t, x, y, names = pitch_stream(ecc, W, H)
    if wh == (346, 260):
        assert {"last_col", "last_row"} <= set(names)
    assert {"col0", "col13", "row0", "row13", "word6"} <= set(names)
    o = check_entries(ecc, orc, gpu, xy, t, W, H, 1024, first_detect=0)
    assert_classes(o, x, y, W, H, names)


BATCHES = [(8192, 4093), (8196, 4094), (12288, 4095), (16384, 4094)]


def assert_batches(o, S, n_slices=3):
    """Flagged events in both batches of every full slice, and at every position of a quad."""
    for s in range(n_slices):
        f = np.flatnonzero(o[s * S:(s + 1) * S])
        assert set(f[f < 8192] % 4) == {0, 1, 2, 3}, (s, "first batch")
        if S > 8192:
            assert set(f[f >= 8192] % 4) == {0, 1, 2, 3}, (s, "second batch")


@pytest.mark.parametrize("first_detect", [0, 2])
@pytest.mark.parametrize("S,last", BATCHES, ids=[f"S{s}_last{l}" for s, l in BATCHES])
def test_batches_and_candidate_ranks(ecc, orc, gpu, S, last, first_detect):
    """One and two batches per slice, a second batch of one quad, a scalar tail of 1..3 events;
    first_detect_slice 2 leaves two slices with live_end = 0 (nothing staged, every flag written)."""
    W, H = 346, 260
    xy, t, x, y = batch_stream(ecc, W, H, S, last)
    o = check_entries(ecc, orc, gpu, xy, t, W, H, S, first_detect=first_detect)
    if first_detect == 0:
        assert_batches(o, S)
        assert o[3 * S:].sum() > 0
    else:
        assert o[:2 * S].sum() == 0 and o[2 * S:3 * S].sum() > 0


def test_first_border_event_in_the_second_batch(ecc, orc, gpu):
    """border_mode 1: a slice's corners end at its first border event, here at index 9001 (the
    second batch) of slices of 16384 and absent from the last slice of 4094."""
    W, H, S, at = 346, 260, 16384, 9001
    xy, t, x, y = batch_stream(ecc, W, H, S, 4094, border_at=at, off_sensor=False)
    o = check_entries(ecc, orc, gpu, xy, t, W, H, S, border_mode=1, first_detect=0)
    for s in range(3):
        f = np.flatnonzero(o[s * S:(s + 1) * S])
        assert (f < 8192).any() and ((f >= 8192) & (f < at)).any() and not (f >= at).any(), s
    assert o[3 * S:].sum() > 0


@pytest.mark.parametrize("off", [1, 2, 3])
def test_flags_pointer_offset(ecc, orc, gpu, off):
    """flags + 1..3 with S = 8198: which slices run in quads moves with the offset, the others take
    the scalar tail behind the raster staging."""
    W, H, S = 346, 260, 8198
    xy, t, x, y = batch_stream(ecc, W, H, S, 4093)
    o = check_entries(ecc, orc, gpu, xy, t, W, H, S, offsets=(off,), first_detect=0)
    assert all(o[s * S:(s + 1) * S].sum() > 0 for s in range(3))


def test_large_sensor_dynamic_lds(ecc, orc, gpu):
    """1280x720, two slices of 4096 events: the raster bitmap is 115200 B."""
    W, H, S = 1280, 720, 4096
    tg = [(4, 4), (700, 360), (1275, 715), (1259, 4), (13, 713), (14 * 91, 14 * 51)]
    fill = [(640, 100), (100, 600)]
    slices = [build_slice(S, tg[:3], fill, off_sensor=(W, H)), build_slice(S, tg[3:], fill, off_sensor=(W, H))]
    xy, t, x, y = to_stream(ecc, slices)
    o = check_entries(ecc, orc, gpu, xy, t, W, H, S, first_detect=0).astype(bool)
    for p in tg:
        assert o[(x == p[0]) & (y == p[1])].any(), p


def test_no_corner_and_every_event_a_corner(ecc, orc, gpu):
    """Slice 0 lays the streaks of pixel p; every event of slice 1 is at p (16384 candidates of one
    raster bit); every event of slice 2 is at a pixel with an empty neighbourhood (a zeroed bitmap)."""
    W, H, S = 346, 260, 16384
    p, r = (100, 77), (250, 200)
    slices = [build_slice(S, [p], [(30, 200), (31, 200)]), [p] * S, [r] * S]
    xy, t, x, y = to_stream(ecc, slices)
    o = check_entries(ecc, orc, gpu, xy, t, W, H, S, first_detect=0)
    assert o[S:2 * S].sum() == S and o[2 * S:].sum() == 0


def test_more_corner_words_than_the_staging_list_holds(ecc, orc, gpu):
    """The staging pass collects the non-zero segment words of a slice in a list behind the raster
    bitmap, which holds 600 of them on 346x260; a word that finds it full is rastered by the lane
    that loaded it.  700 corners per slice, one per tile column every nine rows: each in a segment
    word of its own (same tile: tile pixels 126 apart)."""
    W, H, S = 346, 260, 16384
    tg = [(4 + 14 * k, 4 + 9 * j) for j in range(28) for k in range(25)]
    slices = [build_slice(S, tg, [(200, 130)]), build_slice(S, tg[::-1], [(201, 131)])]
    xy, t, x, y = to_stream(ecc, slices)
    o = check_entries(ecc, orc, gpu, xy, t, W, H, S, CAP=1024, first_detect=0).astype(bool)
    for s in range(2):
        f = o[s * S:(s + 1) * S]
        xs, ys = x[s * S:(s + 1) * S][f], y[s * S:(s + 1) * S][f]
        words = set(zip(ys // 14 * 25 + xs // 14, ((ys % 14) * 14 + xs % 14) // 32))
        assert len(words) > 650, (s, len(words))
