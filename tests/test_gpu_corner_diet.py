"""Corner chain: the per-group records, the division-free item decode and the sort kernel's
sentinel bins (csrc/corner_common.hpp, corner_sort.hip), at the smallest shapes where each can go wrong.  Every case
compares the flags and the final SAE with orc.fast_detect exactly.

* Group records: slice_sort's workgroup of a group's first slice writes the group's constants
  (first index, t_first, Lt, dlt, the narrow / 4-byte-key / beyond-double verdicts), pair_build and
  the arc kernels read them.  One batch holds a 4-byte-key group, an index-key group and a wide
  group; it runs as one call and as prepare + finish; batches of 1, 3 and 2 groups follow each
  other on one context, the kinds changing places, so a stale record would be read.
* Item decode: (group, tile) from the item number and (row, column) from the tile by multiply-high
  constants, on tile counts of 12, 4, 475, 4 784 and 7 475, with two and with three groups, so that
  most item counts are no multiple of 8 (the test's docstring lists them).
* Sort predicates: slots without an event (past a short slice's end, dropped by the dedup) go to
  sentinel bins; ranks up to 16 383 in one tile, events outside the sensor, a slice of 5 events,
  the first border event at index 0, at the last index and absent, with and without the dedup bitmap.
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def dev(ecc, a):
    return ecc.DeviceArray.from_numpy(np.ascontiguousarray(a))


def _one_call(ecc, ctx, xy, t, cfg, W, H):
    sae = dev(ecc, np.zeros(W * H, np.int64))
    flags = ecc.DeviceArray(len(xy), np.uint8)
    flags.fill_bytes(0xCD)  # every flag must be written
    ctx.fast_detect(dev(ecc, xy), dev(ecc, t), len(xy), cfg, sae, flags)
    assert ctx.fast_detect_status() == 0
    return flags.numpy(), sae.numpy()


def _two_calls(ecc, ctx, xy, t, cfg, W, H):
    sae = dev(ecc, np.zeros(W * H, np.int64))
    flags = ecc.DeviceArray(len(xy), np.uint8)
    flags.fill_bytes(0xCD)
    local = ecc.DeviceArray(W * H, np.int64)
    d_xy, d_t, n = dev(ecc, xy), dev(ecc, t), len(xy)
    ecc.check(ecc.lib.ecc_fast_detect_prepare(ctx.ctx, d_xy.ptr, d_t.ptr, n, C.byref(cfg), local.ptr, ctx.stream))
    ecc.check(ecc.lib.ecc_fast_detect_finish(ctx.ctx, d_xy.ptr, d_t.ptr, n, C.byref(cfg), sae.ptr, flags.ptr,
                                             ctx.stream))
    assert ctx.fast_detect_status() == 0
    return flags.numpy(), sae.numpy()


def _check(ecc, orc, ctx, xy, t, W, H, run=_one_call, expect_corners=True, **kw):
    cfg = ecc.corner_cfg(width=W, height=H, border_mode=kw.get("border_mode", 0),
                         first_detect_slice=kw.get("first_detect", 1), slice_events=kw.get("slice_events", 16384))
    o_flags, o_sae = orc.fast_detect(xy, t, W, H, **kw)
    g_flags, g_sae = run(ecc, ctx, xy, t, cfg, W, H)
    if expect_corners:
        assert o_flags.sum() > 0, "the stream should contain corners"
    assert (g_flags == o_flags).all(), f"{(g_flags != o_flags).sum()} corner labels differ"
    assert (g_sae == o_sae).all()


# ---------------------------------------------------------------------------------- group records
REC_W, REC_H, REC_S = 64, 48, 256
REC_G = REC_S * 32  # events per group


def _kinds_stream(ecc, beyond):
    """Three whole groups and a ragged tail: group 0 spans < 2^24 ticks (4-byte keys), group 1
    between 2^24 and 2^27 (index keys, t in t32), group 2 above 2^27 (wide: exact tests); with
    `beyond`, groups 2 and 3 also lie past 2^53 (beyond double)."""
    n = REC_G * 3 + 77
    xy, t0, _ = ecc.gen_events(n, seed=17, width=REC_W, height=REC_H)
    t0 = t0.astype(np.int64)
    t = np.empty(n, np.int64)
    end = 0
    for g, span in enumerate((None, 1 << 25, 1 << 29, None)):
        lo, hi = g * REC_G, min(n, (g + 1) * REC_G)
        rel = t0[lo:hi] - t0[lo]
        f = 1 if span is None else span // max(int(rel[-1]), 1) + 1
        t[lo:hi] = end + 1 + rel * f
        end = int(t[hi - 1])
    if beyond:
        t[2 * REC_G:] += 1 << 53
    spans = [int(t[min(n, (g + 1) * REC_G) - 1] - t[g * REC_G]) for g in range(3)]
    assert spans[0] < (1 << 24) - 1 <= spans[1] < (1 << 27) - 1 <= spans[2] < (1 << 32) - 1, spans
    assert (np.diff(t) >= 0).all()
    return xy, t


@pytest.mark.parametrize("beyond", [False, True])
@pytest.mark.parametrize("run", [_one_call, _two_calls], ids=["one_call", "prepare_finish"])
def test_group_records_three_kinds_in_one_batch(ecc, orc, gpu, run, beyond):
    xy, t = _kinds_stream(ecc, beyond)
    _check(ecc, orc, gpu, xy, t, REC_W, REC_H, run=run, slice_events=REC_S)


def test_group_records_are_rewritten_by_every_call(ecc, orc):
    """1 group (wide), then 3 groups, then 2 groups (index keys, wide) on one context: group 0's
    record changes kind from call to call, and the middle call leaves a third record behind."""
    xy, t = _kinds_stream(ecc, False)
    ctx = ecc.Context(0)
    try:
        for lo, hi in ((2 * REC_G, 3 * REC_G), (0, len(xy)), (REC_G, 3 * REC_G)):
            for run in (_one_call, _two_calls):
                _check(ecc, orc, ctx, xy[lo:hi], t[lo:hi], REC_W, REC_H, run=run, slice_events=REC_S, first_detect=0)
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------ item decode
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("n", [40_003, 64_003])  # 41 slices = 2 groups; 65 slices = 3 groups
@pytest.mark.parametrize("wh,tiles", [((29, 43), 12), ((28, 28), 4), ((346, 260), 475), ((1280, 720), 4784),
                                      ((1600, 900), 7475)])
def test_item_decode_tile_counts(ecc, orc, gpu, wh, tiles, n, mode):
    """Items = groups * tiles: 24, 8, 950, 9568, 14950 with two groups and 36, 12, 1425, 14352, 22425
    with three, so arc_kernel's grid (rounded up to a multiple of 8 for its XCD order) has a ragged
    tail in seven of the ten (4784 tiles is a multiple of 16, 24 and 8 are multiples of 8)."""
    W, H = wh
    assert ((W + 13) // 14) * ((H + 13) // 14) == tiles
    S = 1000
    assert (n + S - 1) // S // 32 + 1 == (2 if n < 64_000 else 3)
    xy, t, _ = ecc.gen_events(n, seed=23 + tiles, width=W, height=H)
    # (mode 1 leaves no corner on the smallest sensor: every slice meets a border event early)
    _check(ecc, orc, gpu, xy, t, W, H, expect_corners=(mode == 0), slice_events=S, border_mode=mode)


# -------------------------------------------------------------------------------- sort predicates
SORT_N = 16384 * 3 + 5  # three whole slices and one of 5 events


def _interior(ecc, W, H, seed):
    xy, t, _ = ecc.gen_events(SORT_N, seed=seed, width=W, height=H)
    x, y = ecc.unpack_xy(xy)
    return np.clip(x, 4, W - 5), np.clip(y, 4, H - 5), t


@pytest.mark.parametrize("wh", [(346, 260), (1280, 720)], ids=["dedup", "no_dedup"])
@pytest.mark.parametrize("case", ["one_tile", "third_outside", "first_border"])
def test_sort_predicates(ecc, orc, gpu, wh, case):
    W, H = wh
    x, y, t = _interior(ecc, W, H, seed=31)
    mode = 0
    if case == "one_tile":  # every event in tile (2, 3): ranks up to 16 383 in one bin
        x, y = 28 + x % 14, 42 + y % 14
    elif case == "third_outside":  # bin n_tiles: kept by the sort, never a corner, not in the SAE
        x, y = x.copy(), y.copy()
        x[0::6] = W + (x[0::6] % 50)
        y[3::6] = H + (y[3::6] % 50)
    else:  # border_mode 1: the first border event at index 0, at the last index, absent, and in the slice of 5
        mode = 1
        x = x.copy()
        x[0] = 1                  # slice 0: index 0
        x[2 * 16384 - 1] = W - 2  # slice 1: its last index
        x[SORT_N - 1] = 0         # the slice of 5: its last index (slice 2 has none)
    xy = ecc.pack_xy(x, y)
    _check(ecc, orc, gpu, xy, t, W, H, border_mode=mode, first_detect=0)
