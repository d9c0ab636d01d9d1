"""CPU tests of the ecc_dbscan_lists / ecc_cluster_stats_lists boundary: the library exports the
entries and their status calls, and every invalid argument is rejected on the host, before a device
is touched (the pointers here are not addresses of anything)."""
import pytest

CTX, LAB, NCL, DUPS, NDUP, CNT, MEM, NMEM, PAIRS, XY, STATS = (0x1000 * k for k in range(1, 12))
INT32_MAX = 2 ** 31 - 1


def call(ecc, ctx=CTX, labels=LAB, n_clusters=NCL, dups=DUPS, dup_cap=16, n_dups=NDUP, n_segs=2, stride=64,
         counts=CNT, members=MEM, member_stride=64, n_members=NMEM, pairs=PAIRS, pair_cap=8):
    return ecc.lib.ecc_dbscan_lists(ctx, labels, n_clusters, dups, dup_cap, n_dups, n_segs, stride, counts, members,
                                    member_stride, n_members, pairs, pair_cap, None)


def call_stats(ecc, ctx=CTX, xy=XY, members=MEM, member_stride=64, n_members=NMEM, pairs=PAIRS, pair_cap=8,
               n_pairs=NCL, n_segs=2, stride=64, counts=CNT, stats=STATS):
    return ecc.lib.ecc_cluster_stats_lists(ctx, xy, members, member_stride, n_members, pairs, pair_cap, n_pairs,
                                           n_segs, stride, counts, stats, None)


def test_library_exports_dbscan_lists(ecc):
    for name in ("ecc_dbscan_lists", "ecc_dbscan_lists_status", "ecc_dbscan_lists_host", "ecc_cluster_stats_lists"):
        assert hasattr(ecc.lib, name), name
    for name in ("dbscan_lists", "dbscan_lists_status", "cluster_stats_lists"):
        assert hasattr(ecc.Context, name), name
    assert hasattr(ecc, "dbscan_lists_host")


BAD = [
    dict(ctx=None), dict(labels=None), dict(n_clusters=None), dict(n_dups=None), dict(members=None),
    dict(n_members=None), dict(pairs=None), dict(dups=None),
    dict(n_segs=-1), dict(dup_cap=-1), dict(pair_cap=-1),
    dict(stride=0), dict(stride=-5), dict(stride=INT32_MAX + 1),
    dict(member_stride=-1), dict(member_stride=INT32_MAX + 1),
    dict(stride=8193), dict(stride=INT32_MAX),  # more than one segment above the window limit
]


@pytest.mark.parametrize("bad", BAD, ids=lambda d: ",".join(f"{k}={v}" for k, v in d.items()))
def test_dbscan_lists_rejects_bad_arguments(ecc, bad):
    assert call(ecc, **bad) == ecc.ERR_INVALID


def test_dbscan_lists_rejects_bad_arguments_with_no_segments(ecc):
    """The argument ranges hold for an empty call too (only the data pointers may then be NULL)."""
    for bad in (dict(ctx=None), dict(dups=None), dict(dup_cap=-1), dict(pair_cap=-1), dict(stride=0),
                dict(stride=INT32_MAX + 1), dict(member_stride=-1), dict(member_stride=INT32_MAX + 1)):
        assert call(ecc, n_segs=0, **bad) == ecc.ERR_INVALID, bad


def test_dbscan_lists_no_segments_is_ok(ecc):
    assert call(ecc, n_segs=0) == ecc.OK
    assert call(ecc, n_segs=0, labels=None, n_clusters=None, n_dups=None, counts=None, members=None, n_members=None,
                pairs=None) == ecc.OK
    assert call(ecc, n_segs=0, dups=None, dup_cap=0) == ecc.OK
    # the limits themselves are valid
    assert call(ecc, n_segs=0, stride=INT32_MAX, member_stride=INT32_MAX) == ecc.OK
    assert call(ecc, n_segs=0, stride=1, member_stride=0, pair_cap=0) == ecc.OK


def test_dbscan_lists_status_needs_a_context(ecc):
    assert ecc.lib.ecc_dbscan_lists_status(None, None) == ecc.ERR_INVALID


@pytest.mark.parametrize("bad", [
    dict(ctx=None), dict(xy=None), dict(members=None), dict(n_members=None), dict(pairs=None), dict(n_pairs=None),
    dict(stats=None), dict(n_segs=-1), dict(pair_cap=-1), dict(stride=0), dict(stride=8193),
    dict(member_stride=-1), dict(member_stride=INT32_MAX + 1),
], ids=lambda d: ",".join(f"{k}={v}" for k, v in d.items()))
def test_cluster_stats_lists_rejects_bad_arguments(ecc, bad):
    assert call_stats(ecc, **bad) == ecc.ERR_INVALID


def test_cluster_stats_lists_no_segments(ecc):
    assert call_stats(ecc, n_segs=0) == ecc.OK
    assert call_stats(ecc, n_segs=0, xy=None, members=None, n_members=None, pairs=None, n_pairs=None, stats=None) == ecc.OK
    for bad in (dict(ctx=None), dict(stride=8193), dict(pair_cap=-1), dict(member_stride=-1)):
        assert call_stats(ecc, n_segs=0, **bad) == ecc.ERR_INVALID, bad
