"""CPU tests of the per-cluster statistics (size, centroid, variance): ecc_cluster_stats_host
against the literal restatement of OPT/test/cluster_event_data.cpp:472-527
(tests/cluster_stats_ref.py), hand values for the reference's clustering_test_1 points, the proof
that the shared long-chain inputs tell a reordered or fused chain apart, and the device entries'
boundary (every invalid argument is rejected on the host, before a device is touched: the
pointers here are not addresses of anything).  Doubles are compared as their 64-bit patterns.
The program test needs a GPU (the program's ordering runs there) and is marked so."""
import numpy as np
import pytest

import cluster_stats_ref as ref

CTX, XY, ORDER, SRC, CNT, STATS, NST = 0x1000, 0x2000, 0x3000, 0x4000, 0x5000, 0x6000, 0x7000


def host(ecc, xy, order, pairs):
    out, rc = ecc.cluster_stats_host(xy, order, pairs)
    assert out.dtype == ref.STAT_DTYPE == ecc.CLUSTER_STAT_DTYPE
    return out, rc


# ------------------------------------------------------------------------------ 1. against the restatement
def test_host_form_matches_restatement_on_random_intervals(ecc):
    rng = np.random.default_rng(472)
    for n in list(range(1, 40)) + [63, 64, 65, 100, 257, 1000, 3001, 20000]:
        xy = ref.random_points(rng, n, wide=n % 2 == 0)
        order = rng.permutation(n).astype(np.int32)
        pairs = ref.random_pairs(rng, n, 12 if n <= 3001 else 4) + [(0, n - 1), (n - 1, n - 1), (0, 0)]
        got, rc = host(ecc, xy, order, pairs)
        assert rc == ecc.OK
        assert ref.same_bits(got, ref.stats_of(xy, order, pairs)), n
    got, rc = host(ecc, np.zeros(0, np.uint32), np.zeros(0, np.int32), np.zeros((0, 2), np.int32))
    assert rc == ecc.OK and len(got) == 0


def test_host_form_contains_invalid_input(ecc):
    """A pair outside the plot, or an interval holding an order entry outside it, gives
    {begin, 0, 0, 0, 0, 0} and ERR_INVALID; the other records are exact."""
    rng = np.random.default_rng(5)
    n = 50
    xy = ref.random_points(rng, n, True)
    order = rng.permutation(n).astype(np.int32)
    order[20] = n          # positions 20 and 30 hold entries outside [0, n)
    order[30] = -1
    pairs = [(0, 19), (21, 29), (31, 49), (5, 4), (-1, 3), (40, 50), (10, 25), (30, 30), (2 ** 31 - 1, 2 ** 31 - 1)]
    got, rc = host(ecc, xy, order, pairs)
    assert rc == ecc.ERR_INVALID
    assert ref.same_bits(got[:3], ref.stats_of(xy, order, pairs[:3]))
    for k in range(3, len(pairs)):
        assert got[k].tolist() == (pairs[k][0], 0, 0.0, 0.0, 0.0, 0.0), k


# ------------------------------------------------------------------------------ 2. hand values
def test_kat_points_hand_values(ecc):
    xy = ref.kat_xy()
    order = np.arange(9, dtype=np.int32)
    pairs = [(0, 2), (3, 5), (6, 8)]
    assert [list(range(b, e + 1)) for b, e in pairs] == ref.KAT["clusters"]
    got, rc = host(ecc, xy, order, pairs)
    assert rc == ecc.OK
    ref.check_kat_hand(got, [0, 1, 2])
    assert ref.same_bits(got, ref.stats_of(xy, order, pairs))
    # any ordering of a cluster's three points: the same centroid
    got2, _ = host(ecc, xy, order[::-1].copy(), pairs)
    ref.check_kat_hand(got2, [2, 1, 0])


# ------------------------------------------------------------------------------ 3. the inputs discriminate
@pytest.fixture(scope="module")
def long_segments():
    return ref.long_segments()


def test_long_chain_inputs_tell_wrong_chains_apart(long_segments):
    """For the clusters of sizes 3, 5, 7, 100, 1000, 3001 and 8191 of the shared long-chain input
    (none a power of two) the restated variance differs in bits from a reversed chain, from a
    fused chain and from numpy's pairwise sum in at least one cluster each."""
    sizes, differs = set(), {"reversed": 0, "fused": 0, "pairwise": 0}
    for xy, order, ids in long_segments[:2]:
        intervals = [iv for iv in ref.runs_of(ids) if iv[1] - iv[0] + 1 in (3, 5, 7, 100, 1000, 3001, 8191)]
        sizes |= {e - b + 1 for b, e in intervals}
        want = ref.var_bits(ref.stats_of(xy, order, intervals))
        for name, var in (("reversed", ref.variance_reversed), ("fused", ref.variance_fused),
                          ("pairwise", ref.variance_pairwise)):
            other = ref.stats_of(xy, order, intervals, var)
            differs[name] += int((ref.var_bits(other) != want).any(axis=1).sum())
    assert sizes == {3, 5, 7, 100, 1000, 3001, 8191}
    assert all(v > 0 for v in differs.values()), differs


def test_host_form_on_the_long_chains(ecc, long_segments):
    for xy, order, ids in long_segments:
        intervals = ref.runs_of(ids)
        if len(intervals) > 1000:
            intervals = intervals[:300] + intervals[-300:]
        got, rc = host(ecc, xy, order, intervals)
        assert rc == ecc.OK
        assert ref.same_bits(got, ref.stats_of(xy, order, intervals))


def test_power_of_two_sizes_would_hide_the_order():
    """Why the tests avoid them: with 64 points the centroid is dyadic and every step is exact."""
    rng = np.random.default_rng(64)
    for _ in range(20):
        vals = rng.integers(0, 346, 64).tolist()
        c = ref.centroid(vals)
        assert ref.variance(vals, c) == ref.variance_reversed(vals, c)


# ------------------------------------------------------------------------------ 4. argument checks
def call_runs(ecc, ctx=CTX, xy=XY, order=ORDER, cluster=SRC, n_segs=2, stride=64, counts=CNT, stats=STATS, cap=16,
              n_stats=NST):
    return ecc.lib.ecc_cluster_stats_runs(ctx, xy, order, cluster, n_segs, stride, counts, stats, cap, n_stats, None)


def call_pairs(ecc, ctx=CTX, xy=XY, order=ORDER, pairs=SRC, pair_cap=16, n_pairs=NST, n_segs=2, stride=64, counts=CNT,
               stats=STATS):
    return ecc.lib.ecc_cluster_stats_pairs(ctx, xy, order, pairs, pair_cap, n_pairs, n_segs, stride, counts, stats, None)


def test_library_exports_cluster_stats(ecc):
    for name in ("ecc_cluster_stats_runs", "ecc_cluster_stats_pairs", "ecc_cluster_stats_status",
                 "ecc_cluster_stats_host"):
        assert hasattr(ecc.lib, name)
    for name in ("cluster_stats_runs", "cluster_stats_pairs", "cluster_stats_status"):
        assert hasattr(ecc.Context, name)
    assert callable(ecc.cluster_stats_host) and ecc.CLUSTER_STAT_DTYPE.itemsize == 40


BAD_RUNS = [dict(ctx=None), dict(xy=None), dict(order=None), dict(cluster=None), dict(stats=None), dict(n_stats=None),
            dict(n_segs=-1), dict(cap=-1), dict(stride=0), dict(stride=8193), dict(stride=-5), dict(stride=2 ** 31)]
BAD_PAIRS = [dict(ctx=None), dict(xy=None), dict(order=None), dict(pairs=None), dict(n_pairs=None), dict(stats=None),
             dict(n_segs=-1), dict(pair_cap=-1), dict(stride=0), dict(stride=8193), dict(stride=-5), dict(stride=2 ** 31)]
IDS = lambda d: ",".join(f"{k}={v}" for k, v in d.items())  # noqa: E731


@pytest.mark.parametrize("bad", BAD_RUNS, ids=IDS)
def test_runs_form_rejects_bad_arguments(ecc, bad):
    assert call_runs(ecc, **bad) == ecc.ERR_INVALID


@pytest.mark.parametrize("bad", BAD_PAIRS, ids=IDS)
def test_pairs_form_rejects_bad_arguments(ecc, bad):
    assert call_pairs(ecc, **bad) == ecc.ERR_INVALID


def test_no_segments(ecc):
    """n_segs == 0 is ECC_OK after the same range checks (only the data pointers may then be NULL)."""
    assert call_runs(ecc, n_segs=0) == ecc.OK and call_pairs(ecc, n_segs=0) == ecc.OK
    assert call_runs(ecc, n_segs=0, xy=None, order=None, cluster=None, counts=None, stats=None, n_stats=None,
                     stride=8192, cap=0) == ecc.OK
    assert call_pairs(ecc, n_segs=0, xy=None, order=None, pairs=None, n_pairs=None, counts=None, stats=None,
                      stride=1, pair_cap=0) == ecc.OK
    for bad in BAD_RUNS:
        if not set(bad) & {"xy", "order", "cluster", "stats", "n_stats", "n_segs"}:
            assert call_runs(ecc, n_segs=0, **bad) == ecc.ERR_INVALID, bad
    for bad in BAD_PAIRS:
        if not set(bad) & {"xy", "order", "pairs", "n_pairs", "stats", "n_segs"}:
            assert call_pairs(ecc, n_segs=0, **bad) == ecc.ERR_INVALID, bad


def test_status_needs_a_context(ecc):
    assert ecc.lib.ecc_cluster_stats_status(None, None) == ecc.ERR_INVALID


def test_host_form_rejects_bad_arguments(ecc):
    xy, order = np.zeros(4, np.uint32), np.arange(4, dtype=np.int32)
    pairs, out = np.array([[0, 3]], np.int32), np.zeros(1, ecc.CLUSTER_STAT_DTYPE)

    def call(xy_p=xy.ctypes.data, order_p=order.ctypes.data, n=4, pairs_p=pairs.ctypes.data, n_pairs=1,
             stats=out.ctypes.data):
        return ecc.lib.ecc_cluster_stats_host(xy_p, order_p, n, pairs_p, n_pairs, stats)

    assert call() == ecc.OK
    for bad in (dict(n=-1), dict(n=2 ** 31), dict(n_pairs=-1), dict(xy_p=None), dict(order_p=None), dict(pairs_p=None),
                dict(stats=None)):
        assert call(**bad) == ecc.ERR_INVALID, bad
    assert call(xy_p=None, order_p=None, n=0, pairs_p=None, n_pairs=0, stats=None) == ecc.OK


# ------------------------------------------------------------------------------ 5. the wrappers, through the program
@pytest.mark.gpu
@pytest.mark.parametrize("source", ["events", "kat_points"])
def test_program_prints_the_restatements_statistics(tmp_path, source):
    """ecc_optics_events --stats (ecc::optics::cluster_statistics, on get_cluster_points): the
    restatement applied to the order the program prints; without --stats the output is unchanged."""
    base, xs, ys, thr = ref.prog_inputs(tmp_path, source)
    for xi_args in ([], ["--chi", 0.1]):
        plain = ref.run_prog(*base, *xi_args)
        assert "stats_" not in plain
        head, order, reach, xi, stats = ref.parse_stats(ref.run_prog(*base, *xi_args, "--stats"))
        assert head == plain
        assert sorted(order) == list(range(len(xs)))
        assert ref.same_bits(stats["stats_clusters"], ref.want_records(xs, ys, order, ref.threshold_intervals(reach, thr)))
        assert ("stats_xi" in stats) == bool(xi_args)
        if xi_args:
            assert ref.same_bits(stats["stats_xi"], ref.want_records(xs, ys, order, xi))
        # the "cluster ..." lines are the same statistics at four decimals
        cl = [l for l in plain.splitlines() if l.startswith("cluster ")]
        for k, r in enumerate(stats["stats_clusters"]):
            assert cl[k] == (f"cluster {k} size {r['size']} centroid ({r['cx']:.4f}, {r['cy']:.4f}) "
                             f"variance ({r['vx']:.4f}, {r['vy']:.4f})")
    if source == "kat_points":
        clusters = [sorted(order[b:e + 1]) for b, e in ref.threshold_intervals(reach, thr)]
        assert sorted(clusters) == sorted(ref.KAT["clusters"])
