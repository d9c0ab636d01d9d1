"""The corner tracker on the device at its path boundaries and exact thresholds: every case of
tests/tracker_cases.py (tests/test_tracker_cases.py proves on the CPU which path each one takes)
against its expected answer — the oracle's state, which for family A the CPU module proves equal to
the reference's compiled CornerTracker; family A is also compared with the reference's stored dump
directly.  After every launch of the case's split: every field of every track and group
(parity.track_key / parity.group_key, floats as bit patterns), the group label lists, status() and
next_label().  No tolerance anywhere: the tracker's contract is bit equality.
"""
import ctypes as C

import numpy as np
import pytest

import parity
import ref_cpu_cases as rc
import tracker_cases as tc

pytestmark = pytest.mark.gpu

CASES = tc.all_cases()
ids = lambda cs: [c.name for c in cs]


def device_snapshot(ecc, tr, cap):
    tb = (ecc.Track * cap)()
    n = C.c_int32(0)
    rc_ = ecc.lib.ecc_tracker_get_tracks(tr.tr, tb, cap, C.byref(n), tr.ctx.stream)
    assert rc_ == ecc.OK and 0 <= n.value <= cap, (rc_, n.value)
    tracks = np.frombuffer(tb, np.int32, n.value * tc.TRACK_WORDS).reshape(n.value, tc.TRACK_WORDS).copy()
    gb = (ecc.Group * cap)()
    labels = np.full(cap, -7, np.int32)
    g = C.c_int32(0)
    rc_ = ecc.lib.ecc_tracker_get_groups(tr.tr, gb, cap, C.byref(g), labels.ctypes.data, cap, tr.ctx.stream)
    assert rc_ == ecc.OK and 0 <= g.value <= cap, (rc_, g.value)
    groups = np.frombuffer(gb, np.int32, g.value * 8).reshape(g.value, 8).copy()
    nl = int(groups[:, 1].sum()) if g.value else 0
    return tc.Snapshot(tracks, groups, labels[:nl].copy(), tr.next_label())


def assert_same(ecc, got, want, where):
    assert got.next_label == want.next_label, where
    same = (got.tracks.shape == want.tracks.shape and np.array_equal(got.tracks, want.tracks) and
            got.groups.shape == want.groups.shape and np.array_equal(got.groups, want.groups) and
            np.array_equal(got.labels, want.labels))
    if not same:  # the raw words differ: say where, in parity's keys
        gt, gg, gl = tc.snapshot_keys(ecc, parity, got)
        wt, wg, wl = tc.snapshot_keys(ecc, parity, want)
        assert len(gt) == len(wt), (where, len(gt), len(wt))
        for i, (a, b) in enumerate(zip(gt, wt)):
            assert a == b, (where, "track", i)
        assert gg == wg, where
        assert gl == wl, where
        raise AssertionError((where, "words differ outside the keys"))


def run_case(ecc, orc, gpu, case, each=None):
    census, snaps = tc.oracle_run(ecc, orc, case)
    stride = max(1, max(min(len(p), case.max_det) for p in case.slices))
    tr = ecc.Tracker(gpu, tc.ecc_cfg(ecc, case.cfg), max_tracks=case.max_tracks, max_detections=case.max_det)
    try:
        a = 0
        sticky = 0
        for b in case.launch_ends():
            flat = np.zeros((b - a) * stride, ecc.CORNER_DTYPE)
            cnt = np.zeros(b - a, np.int32)
            for s in range(a, b):
                p = case.slices[s][:stride]
                flat[(s - a) * stride: (s - a) * stride + len(p)] = tc.corners_of(ecc, p)
                cnt[s - a] = len(case.slices[s]) if case.counts is None else case.counts[s]
            tr.update(ecc.DeviceArray.from_numpy(flat), ecc.DeviceArray.from_numpy(cnt), b - a, stride)
            gpu.sync()
            over = any(c > case.max_det for c in cnt)
            sticky = ecc.ERR_CAPACITY if over else sticky
            want_status = case.want.get("status", {}).get(b)
            if want_status is not None:
                assert sticky == (ecc.ERR_CAPACITY if want_status == "cap" else 0)
            got = device_snapshot(ecc, tr, max(case.max_tracks, 1))
            want = snaps[b]
            if case.want.get("cut_room") and b == len(case.slices):
                # the oracle has no capacity: its list cut to the kept tracks plus the room there was
                want, short = tc.cut_to_room(snaps[a], want, case.max_tracks)
                assert short == case.want["short"]
                assert tr.status() == (ecc.ERR_CAPACITY if short else 0)
            else:
                assert tr.status() == sticky, (case.name, b)
            assert_same(ecc, got, want, (case.name, "after slice", b - 1))
            if each:
                each(b, tr)
            a = b
    finally:
        tr.close()


@pytest.mark.parametrize("case", CASES, ids=ids(CASES))
def test_tracker_case(ecc, orc, gpu, case):
    run_case(ecc, orc, gpu, case)


A = [c for c in CASES if c.family == "A"]


@pytest.mark.parametrize("case", A, ids=ids(A))
def test_family_a_against_reference_dump(ecc, orc, gpu, case, tmp_path):
    """Slice by slice against what the reference's compiled CornerTracker wrote."""
    dump = rc.ref_track("track_" + case.name, tmp_path, tc.lists3(case.slices), cfg=case.cfg)
    cut = (lambda key: key) if float(case.cfg[6]) >= 0 else (lambda key: key[:-1])

    def each(b, tr):
        tracks, groups = dump[b - 1]
        assert [cut(rc.struct_track_key(t)) for t in tr.tracks()] == [cut(rc.track_key(t)) for t in tracks], b
        assert rc.struct_group_keys(*tr.groups()) == groups, b

    run_case(ecc, orc, gpu, case.per_slice(), each)
