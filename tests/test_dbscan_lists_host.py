"""ecc_dbscan_lists_host (no GPU) against the literal restatement in tests/dbscan_lists_ref.py on
fabricated inputs, and against the reference's own lists (orc.dbscan_cloud, DBSCAN_simple.h:27-142)
on ref_cpu_cases.dbscan_points() with the dups derived from them."""
import numpy as np
import pytest

import dbscan_lists_ref as ref
import ref_cpu_cases as cases


def host(ecc, labels, nc, dups, member_cap=None, pair_cap=None):
    return ecc.dbscan_lists_host(labels, nc, dups, member_cap, pair_cap)


def check(ecc, labels, nc, dups, want_status=None):
    lists, invalid = ref.segment_lists(labels, len(labels), nc, dups)
    row, iv = ref.layout(lists)
    members, pairs, nm, rc = host(ecc, labels, nc, dups)
    assert rc == (ecc.ERR_INVALID if invalid else ecc.OK)
    assert want_status is None or rc == want_status
    assert nm == len(row)
    assert members.tobytes() == np.asarray(row, np.int32).tobytes()
    assert pairs.tobytes() == np.asarray(iv, np.int32).reshape(-1, 2).tobytes()
    return row, iv


def test_fabricated_segments(ecc):
    """Counts 0 ... 64, all -1, one cluster, every point its own cluster, random labels; 0 to 3 x count
    dups; the same dups in another order give the same bytes."""
    rng = np.random.default_rng(2790)
    seen_dups = seen_empty = 0
    for s in range(200):
        count = s % 65
        labels, nc, dups = ref.fabricated_segment(rng, count, s % 7)
        row, iv = check(ecc, labels, nc, dups, ecc.OK)
        seen_dups += len(dups) > 0
        seen_empty += any(e < b for b, e in iv)
        if dups:
            again = [dups[i] for i in rng.permutation(len(dups))]
            assert host(ecc, labels, nc, again)[0].tobytes() == np.asarray(row, np.int32).tobytes()
    assert seen_dups > 50 and seen_empty > 10


def test_a_membership_given_twice_is_listed_twice(ecc):
    labels = np.array([0, 1, 0, -1, 1], np.int32)
    row, iv = check(ecc, labels, 2, [(3, 0), (3, 0), (0, 0), (4, 0)], ecc.OK)
    assert row == [0, 0, 2, 3, 3, 4, 1, 4] and iv == [(0, 5), (6, 7)]


def test_hostile_entries_are_ignored(ecc):
    labels = np.array([0, 2, -2, 1, -1, 5], np.int32)
    for nc, dups in ((2, []), (3, [(6, 0)]), (3, [(-1, 0)]), (3, [(0, 3)]), (3, [(0, -1)]), (-4, [(0, 0)])):
        row, iv = check(ecc, labels, nc, dups, ecc.ERR_INVALID)
    assert row == [] and iv == []  # a negative n_clusters counts as 0


def test_capacity_is_all_or_nothing(ecc):
    labels = np.array([0, 1, 0, 1, -1], np.int32)
    dups = [(4, 0), (4, 1)]
    assert host(ecc, labels, 2, dups, 6, 2)[3] == ecc.OK
    for member_cap, pair_cap in ((5, 2), (0, 2), (6, 1), (6, 0)):
        members, pairs, nm, rc = host(ecc, labels, 2, dups, member_cap, pair_cap)
        assert (members, pairs, nm, rc) == (None, None, 6, ecc.ERR_CAPACITY)
    # nothing but *n_members is written
    m, p = np.full(8, ref.MEM_FILL, np.int32), np.full(4, ref.PAIR_FILL, np.int32)
    import ctypes as C
    nm = C.c_int64(-1)
    d = np.asarray(dups, np.int64)
    rc = ecc.lib.ecc_dbscan_lists_host(labels.ctypes.data, 5, 2, d.ctypes.data, 2, m.ctypes.data, 5,
                                       C.addressof(nm), p.ctypes.data, 2)
    assert rc == ecc.ERR_CAPACITY and nm.value == 6 and (m == ref.MEM_FILL).all() and (p == ref.PAIR_FILL).all()


def test_rejected_arguments(ecc):
    import ctypes as C
    nm = C.c_int64(0)
    a = np.zeros(4, np.int32)
    d = np.zeros(4, np.int64)
    f = ecc.lib.ecc_dbscan_lists_host
    ok = dict(labels=a.ctypes.data, n=4, nc=1, dups=d.ctypes.data, nd=0, mem=a.ctypes.data, mcap=4, nm=C.addressof(nm),
              pairs=a.ctypes.data, pcap=2)

    def run(**kw):
        v = dict(ok, **kw)
        return f(v["labels"], v["n"], v["nc"], v["dups"], v["nd"], v["mem"], v["mcap"], v["nm"], v["pairs"], v["pcap"])

    assert run() == ecc.OK
    for bad in (dict(n=-1), dict(n=2 ** 31), dict(nd=-1), dict(mcap=-1), dict(pcap=-1), dict(nm=None),
                dict(labels=None), dict(dups=None, nd=1)):
        assert run(**bad) == ecc.ERR_INVALID, bad
    assert run(n=0, labels=None, nc=0, mem=None, pairs=None, mcap=0, pcap=0) == ecc.OK


@pytest.fixture(scope="module")
def oracle_cloud(orc):
    pts = cases.dbscan_points()
    lab, clusters = orc.dbscan_cloud(pts, cases.DBSCAN_EPS, cases.DBSCAN_MIN_PTS, cases.DBSCAN_MIN_SIZE,
                                     cases.DBSCAN_MAX_SIZE)
    _, unfiltered = orc.dbscan_cloud(pts, cases.DBSCAN_EPS, cases.DBSCAN_MIN_PTS)
    return pts, lab, clusters, unfiltered


def test_reference_lists_of_the_dbscan_points(ecc, oracle_cloud):
    """The reference's labels, with the dups derived as its memberships other than the label, give
    back the reference's lists."""
    pts, lab, clusters, unfiltered = oracle_cloud
    # what makes this input worth the run (checked on the CPU when the test was written)
    assert len(unfiltered) == 9 and len(clusters) == 6
    assert [len(c) for c in clusters] == [451, 301, 301, 300, 300, 240]
    dups = ref.dups_of_clusters(lab, clusters)
    assert len(dups) == 1
    assert all(lab[p] == c for c, m in enumerate(clusters) for p in m if (int(p), c) not in dups)
    assert all(lab[i] < 0 or i in clusters[lab[i]] for i in range(len(lab)))  # every label inside its own list
    members, pairs, nm, rc = host(ecc, lab, len(clusters), dups)
    assert rc == ecc.OK and nm == sum(len(c) for c in clusters)
    for c, m in enumerate(clusters):
        b, e = pairs[c]
        assert members[b:e + 1].tobytes() == np.asarray(m, np.int32).tobytes()
    # and through the restatement
    check(ecc, lab, len(clusters), dups, ecc.OK)
