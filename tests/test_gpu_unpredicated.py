"""The flag pass (csrc/corner_flags.hip) and the hash downsampler (csrc/downsample.hip) without a
branch per event: every event slot is decoded and looked up, and what must not count — events
off the sensor, past `live_end`, past the window's end or over x_max / y_max — is a clamped index
or a sentinel slot plus a mask.  Each case compares exactly with the oracle, at the smallest shapes
where the masks, the clamp and the sentinel slots can go wrong; output buffers start as 0xCD.

Corner detection (ecc_fast_detect, ecc_fast_detect_nms, prepare + finish against orc.fast_detect /
orc.corner_nms): sensors with partial edge tiles (346x260, 33x29); slices of 4096 events with a
last slice of 1021, 1022 and 1023 (a scalar tail of 1, 2, 3 events behind the quads) and slices of
1021 (no slice but the first starts on a 4-B boundary of the flags); a few per cent of the events
off the sensor, 65535 included, at every position of a quad; border_mode 1 with the slice's first
border event at each position of a quad, at index 0 and absent; first_detect_slice 0 and 2; a
flags pointer offset by 1-3 bytes; corners in the last tile row and column and at tile pixels
>= 192 (the last segment word); a slice with every event in one tile; a (group, tile) item that
only one of its 32 slices touches.

Downsample (ecc_downsample_hash against orc.downsample_hash): windows of 16384, 12000, 8192, 4096,
1000 and 5; n no multiple of the window or of 4; events over x_max / y_max at every position of a
quad and a window made only of them; a window of one repeated pixel; a window whose every bucket
has one event; with and without rep_idx; an xy pointer that is only 4-B aligned.
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

BOX, CAP = 15, 256


def dev(ecc, a):
    return ecc.DeviceArray.from_numpy(np.ascontiguousarray(a))


def cd(ecc, n, dtype):
    d = ecc.DeviceArray(n, dtype)
    d.fill_bytes(0xCD)
    return d


# ------------------------------------------------------------------------------- corner detection
def _one_call(ecc, ctx, d_xy, d_t, n, cfg, sae, flags_ptr):
    ecc.check(ecc.lib.ecc_fast_detect(ctx.ctx, d_xy.ptr, d_t.ptr, n, C.byref(cfg), sae.ptr, flags_ptr, ctx.stream))


def _two_calls(ecc, ctx, d_xy, d_t, n, cfg, sae, flags_ptr):
    local = ecc.DeviceArray(cfg.width * cfg.height, np.int64)
    ecc.check(ecc.lib.ecc_fast_detect_prepare(ctx.ctx, d_xy.ptr, d_t.ptr, n, C.byref(cfg), local.ptr, ctx.stream))
    ecc.check(ecc.lib.ecc_fast_detect_finish(ctx.ctx, d_xy.ptr, d_t.ptr, n, C.byref(cfg), sae.ptr, flags_ptr, ctx.stream))


def _check_detect(ecc, orc, ctx, xy, t, W, H, S, offsets=(0,), expect_corners=True, **kw):
    """All three entry points against the oracle; returns the oracle's flags."""
    n = len(xy)
    cfg = ecc.corner_cfg(width=W, height=H, slice_events=S, border_mode=kw.get("border_mode", 0),
                         first_detect_slice=kw.get("first_detect", 1))
    o_flags, o_sae = orc.fast_detect(xy, t, W, H, slice_events=S, **kw)
    if expect_corners:
        assert o_flags.sum() > 0, "the stream should contain corners"
    d_xy, d_t = dev(ecc, xy), dev(ecc, t)
    for run in (_one_call, _two_calls):
        for off in offsets:
            sae = dev(ecc, np.zeros(W * H, np.int64))
            buf = cd(ecc, n + 8, np.uint8)  # flags at buf + off: every flag written, nothing around them
            run(ecc, ctx, d_xy, d_t, n, cfg, sae, buf.ptr + off)
            assert ctx.fast_detect_status() == 0
            g = buf.numpy()
            bad = int((g[off:off + n] != o_flags).sum())
            assert bad == 0, f"{run.__name__}, flags + {off}: {bad} corner labels differ"
            assert (g[:off] == 0xCD).all() and (g[off + n:] == 0xCD).all(), f"{run.__name__}, flags + {off}: wrote outside"
            assert (sae.numpy() == o_sae).all()
    # detection + NMS in one call (the flag pass writes the candidate lists where S % 4 == 0)
    o_out, o_cnt, rc = orc.corner_nms(xy, o_flags, W, H, slice_events=S, box=BOX, cap=CAP)
    assert rc == 0
    ns = len(o_cnt)
    sae = dev(ecc, np.zeros(W * H, np.int64))
    flags, out, cnt = cd(ecc, n, np.uint8), cd(ecc, ns * CAP, ecc.CORNER_DTYPE), cd(ecc, ns, np.int32)
    ctx.fast_detect_nms(d_xy, d_t, n, cfg, sae, flags, BOX, CAP, out, cnt)
    assert ctx.fast_detect_status() == 0 and ctx.corner_nms_status() == 0
    assert (flags.numpy() == o_flags).all() and (sae.numpy() == o_sae).all()
    assert (cnt.numpy() == o_cnt).all()
    g_out = out.numpy()
    for s in range(ns):
        assert (g_out[s * CAP: s * CAP + o_cnt[s]] == o_out[s * CAP: s * CAP + o_cnt[s]]).all(), s
    return o_flags


def _off_sensor(ecc, xy, W, H, every=29):
    """A few per cent of the events off the sensor — x >= W, y >= H or both, 65535 included — the
    stride odd, so they fall on every position of a quad."""
    x, y = ecc.unpack_xy(xy)
    x, y = x.copy(), y.copy()
    idx = np.arange(3, len(xy), every)
    assert set(idx[:16] % 4) == {0, 1, 2, 3}
    kind = np.arange(len(idx)) % 5
    x[idx[kind == 0]] = W + idx[kind == 0] % 50
    y[idx[kind == 1]] = H + idx[kind == 1] % 50
    x[idx[kind == 2]] = 65535
    y[idx[kind == 3]] = 65535
    x[idx[kind == 4]], y[idx[kind == 4]] = 65535, 65535
    return ecc.pack_xy(x, y)


SHAPES = [(4096, 2 * 4096 + 1021), (4096, 2 * 4096 + 1022), (4096, 2 * 4096 + 1023), (1021, 1021 * 9 + 5)]


@pytest.mark.parametrize("first_detect", [0, 2])
@pytest.mark.parametrize("S,n", SHAPES, ids=[f"S{s}_n{n}" for s, n in SHAPES])
@pytest.mark.parametrize("wh", [(346, 260), (33, 29)], ids=["346x260", "33x29"])
def test_detect_ragged_slices_off_sensor_events(ecc, orc, gpu, wh, S, n, first_detect):
    """Partial edge tiles, a scalar tail of 1-3 events, slices that start off a 4-B boundary
    (S = 1021), events off the sensor at every quad position; first_detect_slice 2 leaves the
    first two slices without corners (live_end = 0: nothing staged, every flag still written)."""
    W, H = wh
    xy, t, _ = ecc.gen_events(n, seed=59, width=W, height=H)  # (corners in every case, the last slice of 1021 included)
    xy = _off_sensor(ecc, xy, W, H)
    _check_detect(ecc, orc, gpu, xy, t, W, H, S, first_detect=first_detect)


@pytest.mark.parametrize("off", [1, 2, 3])
def test_detect_flags_pointer_offset(ecc, orc, gpu, off):
    """flags + 1..3: the quads are taken by the store's address, so which slices run in quads moves
    with the offset (S = 4098: slice s starts at byte 2 s of a word)."""
    W, H, S = 346, 260, 4098
    xy, t, _ = ecc.gen_events(3 * S + 2, seed=43, width=W, height=H)
    _check_detect(ecc, orc, gpu, _off_sensor(ecc, xy, W, H), t, W, H, S, offsets=(off,), first_detect=0)


def test_detect_first_border_event_at_each_quad_position(ecc, orc, gpu):
    """border_mode 1: a slice's corners end at its first border event; that event at index 0, at
    each position of a quad (400 .. 403), at the slice's last index, and absent."""
    W, H, S = 346, 260, 4096
    at = [0, 400, 401, 402, 403, S - 1, None]
    xy, t, _ = ecc.gen_events(S * len(at), seed=47, width=W, height=H)
    x, y = ecc.unpack_xy(xy)
    x, y = np.clip(x, 4, W - 5), np.clip(y, 4, H - 5)  # no border event but the planted ones
    for s, i in enumerate(at):
        if i is not None:
            x[s * S + i] = 1
    o = _check_detect(ecc, orc, gpu, ecc.pack_xy(x, y), t, W, H, S, border_mode=1, first_detect=0)
    live = [int(o[s * S:(s + 1) * S].sum()) for s in range(len(at))]
    assert live[0] == 0 and live[-1] > 0 and live[-2] > 0, live
    for s, i in enumerate(at[1:5], start=1):
        assert o[s * S + i:(s + 1) * S].sum() == 0 and o[s * S:s * S + i].sum() > 0, (s, i)


def test_detect_last_tile_row_and_column_and_last_segment_word(ecc, orc, gpu):
    """Events packed into the sensor's bottom right corner: corners in the last (partial) tile row
    and column, and corners at tile pixels >= 192, the bits of a segment's seventh word."""
    W, H, S = 346, 260, 4096
    xy, t, _ = ecc.gen_events(8 * S, seed=53, width=30, height=24)
    x, y = ecc.unpack_xy(xy)
    x, y = x + (W - 30), y + (H - 24)
    xy = ecc.pack_xy(x, y)
    o = _check_detect(ecc, orc, gpu, xy, t, W, H, S, first_detect=0).astype(bool)
    lp = (y % 14) * 14 + x % 14
    assert o[x >= 14 * (W // 14)].sum() > 0 and o[y >= 14 * (H // 14)].sum() > 0
    assert o[lp >= 192].sum() > 0


def test_detect_one_tile_and_single_slice_item(ecc, orc, gpu):
    """A slice with every event in one tile, and a (group, tile) item only one of the group's 32
    slices touches (the other 31 segments empty)."""
    W, H, S = 64, 48, 256
    n = 32 * S
    xy, t, _ = ecc.gen_events(n, seed=59, width=W, height=H)
    x, y = ecc.unpack_xy(xy)
    x, y = x.copy(), y.copy()
    sl = np.arange(n) // S
    in_t = (x // 14 == 1) & (y // 14 == 1) & (sl != 7)  # tile (1, 1) belongs to slice 7 alone
    x[in_t] += 14
    x[sl == 3], y[sl == 3] = 28 + x[sl == 3] % 14, 14 + y[sl == 3] % 14  # slice 3: tile (2, 1) only
    assert ((x // 14 == 1) & (y // 14 == 1) & (sl == 7)).sum() > 0
    _check_detect(ecc, orc, gpu, ecc.pack_xy(x, y), t, W, H, S, first_detect=0)


# ------------------------------------------------------------------------------------- downsample
X_MAX, Y_MAX = 1280, 720


def _check_downsample(ecc, orc, ctx, xy, window, want_idx=True, shift=0, **kw):
    """`shift` events of padding in front of the device copy: shift = 1 leaves xy 4-B aligned only."""
    n = len(xy)
    cfg = ecc.hash_cfg(window=window, **kw)
    o_xy, o_idx, o_u, o_r = orc.downsample_hash(xy, window=window, **kw)
    nw = len(o_u)
    d_in = dev(ecc, np.concatenate([np.zeros(shift, np.uint32), xy]))
    rep_xy, rep_idx = cd(ecc, nw * window, np.uint32), cd(ecc, nw * window, np.uint32)
    uniq, rep = cd(ecc, nw, np.int32), cd(ecc, nw, np.int32)
    ecc.check(ecc.lib.ecc_downsample_hash(ctx.ctx, d_in.ptr + 4 * shift, n, C.byref(cfg), rep_xy.ptr,
                                          rep_idx.ptr if want_idx else None, uniq.ptr, rep.ptr, ctx.stream))
    assert (uniq.numpy() == o_u).all(), (uniq.numpy(), o_u)
    assert (rep.numpy() == o_r).all(), (rep.numpy(), o_r)
    g_xy, g_idx = rep_xy.numpy(), rep_idx.numpy()
    for w in range(nw):
        lo, k = w * window, int(o_u[w])
        assert (g_xy[lo:lo + k] == o_xy[lo:lo + k]).all(), w
        assert (g_xy[lo + k:lo + window] == 0xCDCDCDCD).all(), w  # only the representatives are written
        if want_idx:
            assert (g_idx[lo:lo + k] == o_idx[lo:lo + k]).all(), w
    if not want_idx:
        assert (g_idx == 0xCDCDCDCD).all()
    return o_u, o_r


def _over_max(ecc, xy, every=13):
    """Events over x_max / y_max (and both, and 65535) at every position of a quad."""
    x, y = ecc.unpack_xy(xy)
    x, y = x.copy(), y.copy()
    idx = np.arange(2, len(xy), every)
    assert set(idx[:16] % 4) == {0, 1, 2, 3}
    kind = np.arange(len(idx)) % 4
    x[idx[kind == 0]] = X_MAX + 1
    y[idx[kind == 1]] = Y_MAX + 1
    x[idx[kind == 2]], y[idx[kind == 2]] = 65535, 65535
    y[idx[kind == 3]] = 65535
    return ecc.pack_xy(x, y)


@pytest.mark.parametrize("want_idx", [True, False], ids=["idx", "no_idx"])
@pytest.mark.parametrize("window,n", [(16384, 16384 * 2 + 4001), (12000, 12000 * 2 + 6), (8192, 8192 * 3 + 4094),
                                      (8192, 8192 * 2 + 2731), (4096, 4096 * 5 + 1), (1000, 1000 * 7 + 333), (5, 5 * 41 + 3)])
def test_downsample_windows(ecc, orc, gpu, window, n, want_idx):
    """Ragged last windows (n no multiple of the window; 2731, 1, 333 and 3 leave n no multiple of
    4: the 4-B loads), windows past 8192 (1024 lanes), events over the maxima at every quad position."""
    xy, _, _ = ecc.gen_events(n, seed=61 + window % 11, width=X_MAX + 1, height=Y_MAX + 1)
    o_u, o_r = _check_downsample(ecc, orc, gpu, _over_max(ecc, xy), window, want_idx=want_idx)
    assert o_u.sum() > 0 and (window == 5 or o_r.sum() > 0)


def test_downsample_unaligned_xy_pointer(ecc, orc, gpu):
    """xy + 4 bytes: window and n multiples of 4, but no 16-B loads."""
    xy, _, _ = ecc.gen_events(8192 * 2, seed=67, width=X_MAX + 1, height=Y_MAX + 1)
    _check_downsample(ecc, orc, gpu, _over_max(ecc, xy), 8192, shift=1)


@pytest.mark.parametrize("window", [8192, 1000])
def test_downsample_special_windows(ecc, orc, gpu, window):
    """Window 0: random; window 1: only events over the maxima (nothing takes a bucket: every
    event on a sentinel slot); window 2: one pixel repeated (one representative, one repeated
    bucket); window 3: every event the first and only one of its bucket (x = 0 .. window - 1 at
    y = 0: 1619 is odd, so the buckets differ); window 4: ragged, random."""
    rnd, _, _ = ecc.gen_events(2 * window, seed=71, width=X_MAX + 1, height=Y_MAX + 1)
    i = np.arange(window)
    over = ecc.pack_xy(i % 640, np.where(i % 2 == 0, 65535, Y_MAX + 1 + i % 100))  # (x_max is 65535 here)
    same = ecc.pack_xy(np.full(window, 77), np.full(window, 55))
    distinct = ecc.pack_xy(i, np.zeros(window, np.int64))
    xy = np.concatenate([rnd[:window], over, same, distinct, rnd[window:window + window // 3 + 1]])
    o_u, o_r = _check_downsample(ecc, orc, gpu, xy, window, x_max=65535)
    assert o_u[1] == 0 and o_r[1] == 0
    assert o_u[2] == 1 and o_r[2] == 1
    assert o_u[3] == window and o_r[3] == 0
