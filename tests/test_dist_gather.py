"""The index step of the multi-rank corner gather (ecc_dist_corner_slices, include/ecc.h §9) at
n_ranks > 1, without a communicator.

ecc_dist_gather_corners is two all-gathers (plain concatenation of the ranks' padded buffers)
followed by this entry point, which turns the gathered {corners, slices} metas and zero-padded
offsets into the (start, count) per slice of the global order that ecc_tracker_update_lists
takes.  The all-gathers need one GPU per rank; everything after them does not, so the tests build
the gathered buffers on the host exactly as the all-gathers would leave them and run the product's
kernel, through the same function and grid computation the gather uses.
Reference anchor: the slice loop FCT/metavision_time_surface_periodic_group_track.cpp:832-850
that the merged tracker restates.
"""
import sys
from pathlib import Path

import numpy as np
import pytest

SENTINEL = -7777
GUARD = 64


def dev(ecc, a):
    return ecc.DeviceArray.from_numpy(np.ascontiguousarray(a))


def _gathered(shard_offsets):
    """metas [R][2], offs [R][ns_max + 1], ns_max, t_max from the ranks' exclusive scans: what the
    meta all-gather and the offsets all-gather of ecc_dist_gather_corners leave on every rank."""
    R = len(shard_offsets)
    ns = [len(o) - 1 for o in shard_offsets]
    ns_max = max(1, max(ns))
    t_max = max(1, max(int(o[-1]) for o in shard_offsets))
    metas = np.zeros((R, 2), np.int64)
    offs = np.zeros((R, ns_max + 1), np.int64)  # a rank's row is zero past its ns_r + 1 entries
    for r, o in enumerate(shard_offsets):
        metas[r] = (o[-1], ns[r])
        offs[r, :ns[r] + 1] = o
    return metas, offs, ns_max, t_max


def _expected(shard_offsets, t_max):
    starts = [r * t_max + o[:-1] for r, o in enumerate(shard_offsets)]
    counts = [np.diff(o) for o in shard_offsets]
    return np.concatenate(starts).astype(np.int64), np.concatenate(counts).astype(np.int32)


def _run_slices(ecc, gpu, metas, offs, ns_max, t_max, n_out):
    d_starts = dev(ecc, np.full(n_out + GUARD, SENTINEL, np.int64))
    d_counts = dev(ecc, np.full(n_out + GUARD, SENTINEL, np.int32))
    d_offs, d_metas = dev(ecc, offs), dev(ecc, metas)  # named: they must outlive the launch
    ecc.check(ecc.lib.ecc_dist_corner_slices(gpu.ctx, d_offs.ptr, d_metas.ptr, len(metas), ns_max, t_max, d_starts.ptr,
                                             d_counts.ptr, gpu.stream), "ecc_dist_corner_slices")
    gpu.sync()
    return d_starts, d_counts


def _scan(counts):
    return np.concatenate([[0], np.cumsum(np.asarray(counts, np.int64))]).astype(np.int64)


def _slice_case(name):
    """Per-rank lists of per-slice corner counts."""
    rng = np.random.default_rng(41)

    def rank(ns, edges=True):
        c = rng.integers(0, 40, ns)
        if edges and ns >= 3:
            c[0] = c[-1] = 0  # empty slices at the start and the end of the rank
        return c

    if name == "r1":
        return [rank(9)]
    if name == "r2_rank_without_corners":
        return [rank(6), np.zeros(4, np.int64)]  # rank 1: slices, no corner
    if name == "r3_empty_middle":
        return [rank(7), np.zeros(0, np.int64), rank(12)]  # rank 1: no slice at all
    if name == "r8_ragged_grid":
        # R * ns_max = 8 * 150 = 1200 items: five blocks of 256, the last with 176
        ns = [3, 150, 0, 17, 1, 64, 5, 40]
        return [np.zeros(n, np.int64) if r == 6 else rank(n, edges=r != 4) for r, n in enumerate(ns)]
    if name == "all_empty":
        return [np.zeros(0, np.int64)] * 3  # the floors ns_max = t_max = 1 apply
    raise KeyError(name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["r1", "r2_rank_without_corners", "r3_empty_middle", "r8_ragged_grid", "all_empty"])
def test_corner_slices_match_numpy(ecc, gpu, name):
    """starts = r * t_max + o_r[s], counts = o_r[s + 1] - o_r[s] in rank order, against plain numpy;
    uneven slice counts, a rank without slices between two with, a rank whose slices hold no
    corner, empty slices at a rank's ends, several blocks with a ragged last one, and no slice
    anywhere.  Nothing past sum(ns_r) is written (guard entries keep their sentinel)."""
    shards = [_scan(c) for c in _slice_case(name)]
    metas, offs, ns_max, t_max = _gathered(shards)
    e_starts, e_counts = _expected(shards, t_max)
    tot = len(e_starts)
    assert tot == int(metas[:, 1].sum())
    if name == "r8_ragged_grid":
        items = len(shards) * ns_max
        assert items > 256 and items % 256 != 0
        assert len({len(o) for o in shards}) == len(shards)  # every rank a different slice count
    if name == "all_empty":
        assert tot == 0 and ns_max == 1 and t_max == 1
    d_starts, d_counts = _run_slices(ecc, gpu, metas, offs, ns_max, t_max, tot)
    g_starts, g_counts = d_starts.numpy(), d_counts.numpy()
    assert np.array_equal(g_starts[:tot], e_starts), (g_starts[:tot], e_starts)
    assert np.array_equal(g_counts[:tot], e_counts), (g_counts[:tot], e_counts)
    assert (g_starts[tot:] == SENTINEL).all() and (g_counts[tot:] == SENTINEL).all()


@pytest.fixture(scope="module")
def stream36(ecc, orc):
    """The stream of test_corner_pack_and_tracker_lists_match_strided: 36 slices of 16384 events at
    346x260, the oracle's flags and NMS lists, and the oracle tracker over all of them."""
    sys.path.insert(0, str(Path(__file__).resolve().parent))
    from test_gpu_parity import _track_key
    W, H, cap = 346, 260, 4096
    n = 16384 * 36
    xy, t, _ = ecc.gen_events(n, seed=23, width=W, height=H)
    o_flags, _ = orc.fast_detect(xy, t, W, H)
    o_out, o_cnt, _ = orc.corner_nms(xy, o_flags, W, H, cap=cap)
    otr = orc.OracleTracker(ecc.tracker_cfg())
    for s in range(len(o_cnt)):
        otr.update(o_out[s * cap: s * cap + o_cnt[s]])
    ref = [_track_key(tr) for tr in otr.tracks(ecc.Track)]
    assert len(o_cnt) == 36 and len(ref) > 0
    return o_out, o_cnt, cap, ref, _track_key


@pytest.mark.gpu
@pytest.mark.parametrize("shard_slices", [(5, 0, 31), (1, 7, 0, 4, 9, 2, 0, 13)], ids=["r3", "r8"])
def test_gathered_shards_drive_tracker_like_one_stream(ecc, gpu, stream36, shard_slices):
    """The stream cut into uneven shards, each packed by ecc_corner_pack on the device; `all`
    (stride t_max) and the padded offsets assembled on the host as the two all-gathers concatenate
    them; ecc_dist_corner_slices; ONE tracker over all / starts / counts.  Its tracks equal the
    oracle tracker's over the whole stream: a wrong base, stride or padding anywhere changes the
    slice order or reads the fill between the ranks' lists."""
    o_out, o_cnt, cap, ref, track_key = stream36
    assert sum(shard_slices) == len(o_cnt)
    d_out, d_cnt = dev(ecc, o_out), dev(ecc, o_cnt)
    shards, lists, a = [], [], 0
    for ns_r in shard_slices:
        if ns_r == 0:  # a rank without slices sends no list and all-zero offsets
            shards.append(np.zeros(1, np.int64))
            lists.append(np.zeros(0, ecc.CORNER_DTYPE))
            continue
        packed, off = ecc.DeviceArray(ns_r * cap, ecc.CORNER_DTYPE), ecc.DeviceArray(ns_r + 1, np.int64)
        gpu.corner_pack(d_out.ptr + a * cap * 12, d_cnt.ptr + a * 4, ns_r, cap, packed, off)
        gpu.sync()
        o = off.numpy()
        assert o[-1] == o_cnt[a: a + ns_r].sum()
        shards.append(o)
        lists.append(packed.numpy()[: o[-1]])
        a += ns_r
    metas, offs, ns_max, t_max = _gathered(shards)
    R, ns = len(shards), len(o_cnt)
    h_all = np.empty(R * t_max, ecc.CORNER_DTYPE)
    h_all[:] = (-12345, -12345, -12345)  # what lies between the ranks' lists must never be read
    for r, pk in enumerate(lists):
        h_all[r * t_max: r * t_max + len(pk)] = pk
    d_starts, d_counts = _run_slices(ecc, gpu, metas, offs, ns_max, t_max, ns)
    assert np.array_equal(d_counts.numpy()[:ns], o_cnt)
    tr = ecc.Tracker(gpu)
    d_all = dev(ecc, h_all)
    tr.update_lists(d_all, d_starts, d_counts, ns)
    gpu.sync()
    assert [track_key(x) for x in tr.tracks()] == ref
    assert tr.status() == 0


def test_corner_slices_rejects_bad_arguments(ecc):
    """ECC_ERR_INVALID before anything is dereferenced or a device is touched (the pointers here
    are not addresses of anything)."""
    f = ecc.lib.ecc_dist_corner_slices
    ctx, offs, metas, starts, counts = 0x1000, 0x2000, 0x3000, 0x4000, 0x5000
    assert f(None, offs, metas, 2, 4, 4, starts, counts, None) == ecc.ERR_INVALID
    assert f(ctx, None, metas, 2, 4, 4, starts, counts, None) == ecc.ERR_INVALID
    assert f(ctx, offs, None, 2, 4, 4, starts, counts, None) == ecc.ERR_INVALID
    assert f(ctx, offs, metas, 2, 4, 4, None, counts, None) == ecc.ERR_INVALID
    assert f(ctx, offs, metas, 2, 4, 4, starts, None, None) == ecc.ERR_INVALID
    for n_ranks, ns_max, t_max in ((0, 4, 4), (-1, 4, 4), (2, 0, 4), (2, -3, 4), (2, 4, 0), (2, 4, -1)):
        assert f(ctx, offs, metas, n_ranks, ns_max, t_max, starts, counts, None) == ecc.ERR_INVALID
