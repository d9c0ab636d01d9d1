"""ecc_cluster_stats_runs / _pairs (size, centroid and variance of every cluster of every segment
on the device) against the literal restatement of OPT/test/cluster_event_data.cpp:472-527
(tests/cluster_stats_ref.py) and the hand values of the reference's clustering_test_1 points.
Outputs are pre-filled with sentinels: records past the runs / pairs of a segment, and past cap,
keep them.  Records are compared as bytes (doubles as their 64-bit patterns); no tolerances.
Padding past a segment's count holds order entries that the kernel would refuse (-1): a read of
them shows as ERR_INVALID."""
import numpy as np
import pytest

import cluster_stats_ref as ref
import optics_xi_ref as xi_ref

pytestmark = pytest.mark.gpu

FILL_BYTE, NST_FILL = 0xA5, -99
TAIL = 3  # sentinel records past the last segment's


def sentinel(n):
    a = np.zeros(n, ref.STAT_DTYPE)
    a.view(np.uint8)[:] = FILL_BYTE
    return a


class Segs:
    """Segments laid out s * stride + i on the device: points, ordering, ids (runs form)."""

    def __init__(self, ecc, segs, stride, full=False):
        """segs: (xy, order, ids) per segment, each of the segment's count."""
        self.segs, self.stride, self.n = segs, stride, len(segs)
        xy = np.full(self.n * stride, 0xDEADBEEF, np.uint32)
        order = np.full(self.n * stride, -1, np.int32)
        ids = np.full(self.n * stride, 0x5A5A5A5A, np.int32)
        self.counts = np.array([len(s[0]) for s in segs], np.int32)
        for s, (sxy, sorder, sids) in enumerate(segs):
            assert len(sxy) == len(sorder) <= stride
            xy[s * stride: s * stride + len(sxy)] = sxy
            order[s * stride: s * stride + len(sxy)] = sorder
            if sids is not None:
                ids[s * stride: s * stride + len(sxy)] = sids
        assert not full or (self.counts == stride).all()
        self.d_xy, self.d_order, self.d_ids = (ecc.DeviceArray.from_numpy(a) for a in (xy, order, ids))
        self.d_cnt = None if full else ecc.DeviceArray.from_numpy(self.counts)

    def want_runs(self):
        return [ref.stats_of(xy, order, ref.runs_of(ids)) for xy, order, ids in self.segs]


def run_runs(ecc, gpu, sg, cap, n_segs=None):
    """One launch over pre-filled outputs: (records[n_segs, cap], tail, n_stats, status)."""
    n = sg.n if n_segs is None else n_segs
    d_stats = ecc.DeviceArray.from_numpy(sentinel(n * cap + TAIL))
    d_nst = ecc.DeviceArray.from_numpy(np.full(n, NST_FILL, np.int32))
    gpu.cluster_stats_runs(sg.d_xy, sg.d_order, sg.d_ids, n, sg.stride, sg.d_cnt, d_stats, cap, d_nst)
    status = gpu.cluster_stats_status()
    h = d_stats.numpy()
    return h[:n * cap].reshape(n, cap), h[n * cap:], d_nst.numpy(), status


def run_pairs(ecc, gpu, sg, pairs, n_pairs, cap):
    """pairs int32[n, cap, 2], n_pairs int32[n] -> (records[n, cap], tail, status)."""
    d_stats = ecc.DeviceArray.from_numpy(sentinel(sg.n * cap + TAIL))
    d_pairs = ecc.DeviceArray.from_numpy(np.ascontiguousarray(pairs, np.int32).reshape(-1))
    d_np = ecc.DeviceArray.from_numpy(np.asarray(n_pairs, np.int32))
    gpu.cluster_stats_pairs(sg.d_xy, sg.d_order, d_pairs, cap, d_np, sg.n, sg.stride, sg.d_cnt, d_stats)
    status = gpu.cluster_stats_status()
    h = d_stats.numpy()
    return h[:sg.n * cap].reshape(sg.n, cap), h[sg.n * cap:], status


def check(recs, tail, want, cap, counts=None):
    """want: the records of every segment; records past them (or past cap) keep the sentinel."""
    fill = sentinel(1)[0]
    assert (tail == fill).all(), "records past the last segment"
    for s, w in enumerate(want):
        k = min(len(w), cap)
        assert ref.same_bits(recs[s, :k], w[:k]), f"records, segment {s}"
        assert (recs[s, k:] == fill).all(), f"records past the clusters, segment {s}"
        if counts is not None:
            assert int(counts[s]) == len(w), f"n_stats, segment {s}"


# ------------------------------------------------------------------------------ 1. the KAT points
def test_kat_points_through_the_grid(ecc, gpu):
    """clustering_test_1's points -> ecc_optics_grid (eps 10, min_pts 2, threshold 10) ->
    ecc_cluster_stats_runs: the hand values and the restatement on the device's own order."""
    xy = ref.kat_xy()
    d_xy = ecc.DeviceArray.from_numpy(xy)
    d_order, d_reach = ecc.DeviceArray(9, np.int32), ecc.DeviceArray(9, np.float64)
    d_cl, d_ncl = ecc.DeviceArray(9, np.int32), ecc.DeviceArray(1, np.int32)
    gpu.optics_grid(d_xy, 1, 9, None, float(ref.KAT["eps"]), ref.KAT["min_pts"], float(ref.KAT["threshold"]),
                    d_order, d_reach, d_cl, d_ncl)
    d_stats = ecc.DeviceArray.from_numpy(sentinel(8))
    d_nst = ecc.DeviceArray.from_numpy(np.full(1, NST_FILL, np.int32))
    gpu.cluster_stats_runs(d_xy, d_order, d_cl, 1, 9, None, d_stats, 8, d_nst)
    assert gpu.cluster_stats_status() == ecc.OK
    order, got = d_order.numpy(), d_stats.numpy()
    assert int(d_nst.numpy()[0]) == int(d_ncl.numpy()[0]) == 3
    assert [int(b) for b in got["begin"][:3]] == [0, 3, 6]
    which = [ref.KAT["clusters"].index(sorted(int(v) for v in order[b:b + 3])) for b in (0, 3, 6)]
    ref.check_kat_hand(got[:3], which)
    check(got[None, :5], got[5:], [ref.stats_of(xy, order, [(0, 2), (3, 5), (6, 8)])], 5)


# ------------------------------------------------------------------------------ 2, 3. tiny segments
def tiny_segments():
    rng = np.random.default_rng(20241020)
    segs = []
    for s in range(300):
        n = s % 65 if s < 195 else int(rng.integers(0, 65))
        segs.append((ref.random_points(rng, n, wide=s % 3 != 0), rng.permutation(n).astype(np.int32),
                     ref.random_ids(rng, n)))
    return segs


@pytest.fixture(scope="module")
def tiny(ecc):
    return Segs(ecc, tiny_segments(), 64)


@pytest.fixture(scope="module")
def tiny_want(tiny):
    return tiny.want_runs()


def test_tiny_segments_runs(ecc, gpu, tiny, tiny_want):
    """300 segments at stride 64 with counts 0, 1, 2 ... 64; all-singleton and one-run segments."""
    assert set(range(65)) <= set(int(c) for c in tiny.counts)
    lens = [len(w) for w, c in zip(tiny_want, tiny.counts) if c > 1]
    assert 1 in lens and any(k == c for k, c in zip(lens, tiny.counts[tiny.counts > 1]))
    # run lengths mostly no powers of two (the all-singleton segments aside)
    sizes = np.concatenate([w["size"] for w, c in zip(tiny_want, tiny.counts) if len(w) != c])
    assert ((sizes & (sizes - 1)) != 0).mean() > 0.5
    recs, tail, nst, status = run_runs(ecc, gpu, tiny, 64)
    assert status == ecc.OK
    check(recs, tail, tiny_want, 64, nst)


def test_tiny_segments_pairs(ecc, gpu, tiny):
    """Nested, identical, single-point and whole-segment intervals; n_pairs above pair_cap in some
    segments: only pair_cap records are written."""
    rng = np.random.default_rng(7)
    cap = 10
    pairs = np.full((tiny.n, cap, 2), -5, np.int32)
    n_pairs, want = np.zeros(tiny.n, np.int32), []
    for s, (xy, order, _) in enumerate(tiny.segs):
        k = 0 if len(xy) == 0 else int(rng.integers(0, 15))
        iv = ref.random_pairs(rng, len(xy), min(k, cap)) if k else []
        pairs[s, :len(iv)] = np.asarray(iv, np.int32).reshape(-1, 2)
        n_pairs[s] = k
        want.append(ref.stats_of(xy, order, iv))
    assert (n_pairs > cap).any() and (n_pairs == 0).any()
    recs, tail, status = run_pairs(ecc, gpu, tiny, pairs, n_pairs, cap)
    assert status == ecc.OK
    check(recs, tail, want, cap)


# ------------------------------------------------------------------------------ 4. capacity
def test_capacity(ecc, gpu, tiny, tiny_want):
    """cap below some segments' run counts: the status says so, n_stats is exact, the first cap
    records are right and nothing past cap is written; a later call that fits clears the status."""
    cap = 5
    assert any(len(w) > cap for w in tiny_want) and any(0 < len(w) <= cap for w in tiny_want)
    recs, tail, nst, status = run_runs(ecc, gpu, tiny, cap)
    assert status == ecc.ERR_CAPACITY
    check(recs, tail, tiny_want, cap, nst)
    recs, tail, nst, status = run_runs(ecc, gpu, tiny, 64)
    assert status == ecc.OK


# ------------------------------------------------------------------------------ 5. long chains
@pytest.fixture(scope="module")
def long(ecc):
    return Segs(ecc, ref.long_segments(), ref.LONG_STRIDE, full=True)


@pytest.fixture(scope="module")
def long_want(long):
    return long.want_runs()


def test_long_chains(ecc, gpu, long, long_want):
    """Stride 8192, seg_counts NULL: one run of 8191 points plus a singleton; runs of 3001, 1000,
    100, 7, 5, 3 and filler; 8192 singletons.  The inputs are those for which
    test_cluster_stats_host.py shows that a reversed, a fused and a pairwise chain give other bits."""
    assert [len(w) for w in long_want] == [2, 686, 8192]
    recs, tail, nst, status = run_runs(ecc, gpu, long, 8192)
    assert status == ecc.OK
    check(recs, tail, long_want, 8192, nst)


def test_long_chains_as_pairs(ecc, gpu, long, long_want):
    """The same long intervals through the pairs form, with the whole segment and a nested one."""
    cap = 12
    pairs = np.full((long.n, cap, 2), -5, np.int32)
    n_pairs, want = np.zeros(long.n, np.int32), []
    for s, (xy, order, ids) in enumerate(long.segs):
        iv = ref.runs_of(ids)[:7] + [(0, ref.LONG_STRIDE - 1), (1000, 4000), (8191, 8191)]
        pairs[s, :len(iv)] = np.asarray(iv, np.int32)
        n_pairs[s] = len(iv)
        want.append(ref.stats_of(xy, order, iv))
    recs, tail, status = run_pairs(ecc, gpu, long, pairs, n_pairs, cap)
    assert status == ecc.OK
    check(recs, tail, want, cap)


# ------------------------------------------------------------------------------ 6. more segments than the grid
def test_more_segments_than_the_grid(ecc, gpu):
    """4500 full segments of stride 16 with seg_counts NULL (the launch grid holds 2048 workgroups)."""
    rng = np.random.default_rng(66)
    segs = [(ref.random_points(rng, 16, wide=bool(s & 1)), rng.permutation(16).astype(np.int32), ref.random_ids(rng, 16))
            for s in range(4500)]
    sg = Segs(ecc, segs, 16, full=True)
    recs, tail, nst, status = run_runs(ecc, gpu, sg, 16)
    assert status == ecc.OK
    check(recs, tail, sg.want_runs(), 16, nst)
    pairs = np.zeros((sg.n, 2, 2), np.int32)
    pairs[:, 0] = (3, 13)
    pairs[:, 1] = (0, 15)
    recs, tail, status = run_pairs(ecc, gpu, sg, pairs, np.full(sg.n, 2, np.int32), 2)
    assert status == ecc.OK
    check(recs, tail, [ref.stats_of(xy, order, [(3, 13), (0, 15)]) for xy, order, _ in segs], 2)


# ------------------------------------------------------------------------------ 7. invalid input is contained
def test_invalid_input_is_contained(ecc, gpu):
    """One segment has an order entry outside it, one pair has end >= count: ERR_INVALID, those
    records are {begin, 0, 0, 0, 0, 0}, everything beside them is exact."""
    rng = np.random.default_rng(3)
    segs = []
    for s in range(5):
        n = 20 + s
        segs.append((ref.random_points(rng, n, True), rng.permutation(n).astype(np.int32),
                     ref.ids_of_runs([3, 5, 7, n - 15])))
    segs[2][1][9] = 22  # segment 2 has 22 points: position 9, inside the run [8, 14], is refused
    sg = Segs(ecc, segs, 32)
    recs, tail, nst, status = run_runs(ecc, gpu, sg, 6)
    assert status == ecc.ERR_INVALID
    want = []
    for s, (xy, order, ids) in enumerate(segs):
        iv = ref.runs_of(ids)
        if s == 2:
            good = ref.stats_of(xy, order, [iv[0], iv[1], iv[3]])
            want.append(np.concatenate([good[:2], ref.records([(8, 0, 0.0, 0.0, 0.0, 0.0)]), good[2:]]))
        else:
            want.append(ref.stats_of(xy, order, iv))
    check(recs, tail, want, 6, nst)

    segs[2][1][9] = segs[2][1][10]  # a valid (repeated) entry again
    sg = Segs(ecc, segs, 32)
    pairs = np.zeros((5, 2, 2), np.int32)
    pairs[:, 0] = (2, 11)
    pairs[:, 1] = (0, 19)
    pairs[3, 0] = (4, 23)   # segment 3 has 23 points
    recs, tail, status = run_pairs(ecc, gpu, sg, pairs, np.full(5, 2, np.int32), 2)
    assert status == ecc.ERR_INVALID
    want = [ref.stats_of(xy, order, [(2, 11), (0, 19)]) for xy, order, _ in segs]
    want[3][0] = (4, 0, 0.0, 0.0, 0.0, 0.0)
    check(recs, tail, want, 2)
    # a later valid call clears the status
    pairs[3, 0] = (4, 22)
    assert run_pairs(ecc, gpu, sg, pairs, np.full(5, 2, np.int32), 2)[2] == ecc.OK


# ------------------------------------------------------------------------------ 8. the chain on the device
def test_windows_to_ordering_to_clusters_to_statistics_on_the_device(ecc, orc, gpu):
    """16384 generated events -> downsample_hash (2 windows) -> optics_grid with clusters ->
    cluster_stats_runs; the same reach -> optics_xi (chi 0.1, min_pts 4) -> cluster_stats_pairs.
    Both against the restatement applied to the oracle's order of each window."""
    xy, _, _ = ecc.gen_events(16384, seed=61)
    rep_xy, _, uniq, _, nw = gpu.downsample_hash(ecc.DeviceArray.from_numpy(xy), len(xy))
    assert nw == 2
    d_order, d_reach = ecc.DeviceArray(nw * 8192, np.int32), ecc.DeviceArray(nw * 8192, np.float64)
    d_cl, d_ncl = ecc.DeviceArray(nw * 8192, np.int32), ecc.DeviceArray(nw, np.int32)
    gpu.optics_grid(rep_xy, nw, 8192, uniq, 10.0, 2, 10.0, d_order, d_reach, d_cl, d_ncl)
    h_xy, h_u = rep_xy.numpy(), uniq.numpy()
    ncl = d_ncl.numpy()
    cap = int(ncl.max()) + 2
    d_stats = ecc.DeviceArray.from_numpy(sentinel(nw * cap + TAIL))
    d_nst = ecc.DeviceArray.from_numpy(np.full(nw, NST_FILL, np.int32))
    gpu.cluster_stats_runs(rep_xy, d_order, d_cl, nw, 8192, uniq, d_stats, cap, d_nst)
    assert gpu.cluster_stats_status() == ecc.OK
    runs = d_stats.numpy()

    xi_cap, params = 1024, (0.1, 4, 0.0)
    d_pairs, d_np = ecc.DeviceArray(nw * xi_cap * 2, np.int32), ecc.DeviceArray(nw, np.int32)
    gpu.optics_xi(d_reach, nw, 8192, uniq, *params, d_pairs, xi_cap, d_np)
    assert gpu.optics_xi_status() == ecc.OK
    d_xstats = ecc.DeviceArray.from_numpy(sentinel(nw * xi_cap + TAIL))
    gpu.cluster_stats_pairs(rep_xy, d_order, d_pairs, xi_cap, d_np, nw, 8192, uniq, d_xstats)
    assert gpu.cluster_stats_status() == ecc.OK
    xis = d_xstats.numpy()

    want_runs, want_xi = [], []
    for w in range(nw):
        wxy = h_xy[w * 8192: w * 8192 + int(h_u[w])]
        x, y = ecc.unpack_xy(wxy)
        assert len(x) > 64
        o_order, o_reach = orc.optics(np.stack([x, y], 1).astype(np.float64), 2, 10.0)
        want_runs.append(ref.stats_of(wxy, o_order, ref.threshold_intervals(o_reach, 10.0)))
        want_xi.append(ref.stats_of(wxy, o_order, xi_ref.chi_clusters(o_reach, *params)))
    assert [len(w) for w in want_runs] == [int(v) for v in ncl] and sum(len(w) for w in want_xi) > 0
    check(runs[:nw * cap].reshape(nw, cap), runs[nw * cap:], want_runs, cap, d_nst.numpy())
    check(xis[:nw * xi_cap].reshape(nw, xi_cap), xis[nw * xi_cap:], want_xi, xi_cap, d_np.numpy())


# ------------------------------------------------------------------------------ 9. determinism
def test_deterministic(ecc, gpu, tiny, long):
    for sg, cap in ((tiny, 64), (long, 8192)):
        a = run_runs(ecc, gpu, sg, cap)
        b = run_runs(ecc, gpu, sg, cap)
        assert a[0].tobytes() == b[0].tobytes() and a[2].tobytes() == b[2].tobytes()


# ------------------------------------------------------------------------------ 10. the host program
@pytest.mark.parametrize("source", ["events", "kat_points"])
def test_program_device_route_prints_what_the_host_route_prints(tmp_path, source):
    """ecc_optics_events --stats --device-order: exactly the host route's text, with and without
    --chi; without --stats, --device-order prints what the host route prints too."""
    base = ref.prog_inputs(tmp_path, source)[0]
    for xi_args in ([], ["--chi", 0.1]):
        host = ref.run_prog(*base, *xi_args, "--stats")
        assert "stats_clusters" in host and ("stats_xi" in host) == bool(xi_args)
        assert ref.run_prog(*base, *xi_args, "--stats", "--device-order") == host
        assert ref.run_prog(*base, *xi_args, "--device-order") == ref.run_prog(*base, *xi_args)
