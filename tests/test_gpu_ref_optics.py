"""The OPTICS family on the device — ecc_optics_grid, ecc_optics_f64 and the device-resident chain
ecc_optics_grid -> ecc_optics_xi -> ecc_optics_xi_tree -> ecc_cluster_stats_runs / _pairs — against
the REFERENCE'S OWN compiled code: oracle/_ref/ref_optics or its recorded answers under
tests/golden/ref_cpu/optics_*.npz (tests/ref_optics_cases.py; the reference tree itself is never
read here).  Every comparison is exact; doubles are compared as their 64-bit patterns.

Cases with equal parameters share one launch.  The two launches at stride 8192 put the full windows
(m == seg_stride == 8192: the dense `full` and the lattice `noise`) between shorter segments.  The
blobs sweep (stride 1024, also full) is the first to launch optics_grid_kernel<16> (min_pts 9, 16)
and to select the last slot of the networks of 8, 16, 32 and 64 (min_pts 8, 16, 32, 64; 64 is the
entry's maximum)."""
import numpy as np
import pytest

import optics_tree_ref as tr
import ref_optics_cases as oc
from test_gpu_optics_grid import CLUSTER_FILL, NCL_FILL, ORDER_FILL, REACH_FILL, Packed, check_against, run_grid

pytestmark = pytest.mark.gpu

# (cases of one launch, stride, pair capacity): every case of a launch has the launch's parameters.  The e2
# launch needs a short segment between its two full ones; event_csv_e2 is the only short case with its
# parameters, so it appears there twice (the same answers are expected in both places).
LAUNCHES = {
    "e10": (("event_csv", "full", "ties", "noise_e10", "kat1"), 8192, 4096),
    "e2": (("event_csv_e2", "full_e2", "event_csv_e2", "noise"), 8192, 4096),
    "ties_e2": (("ties_e2",), 600, 600),
    "kdtree": (("kdtree",), 1024, 600),
    "kat2": (("kat2",), 16, 16),
    **{f"blobs_mp{m}": ((f"blobs_mp{m}",), 1024, 1024) for m in oc.BLOBS_MIN_PTS},
}
PAIR_PAD, STAT_PAD = 0x5A5A5A5A, 0xA5
SORTED_FILL, PARENT_FILL, LEVEL_FILL, ROOTS_FILL, NST_FILL = -71, -72, -73, -74, -75


@pytest.fixture(scope="module")
def shared(tmp_path_factory):
    return tmp_path_factory.mktemp("ref_optics_gpu")


def launch_inputs(ecc, orc, shared, key):
    """-> (names, Packed, (eps, min_pts, thr), the reference's answers per segment)."""
    names, stride, _ = LAUNCHES[key]
    params = {oc.case(ecc, orc, n)[1:4] for n in names}
    assert len(params) == 1, "the cases of one launch share its parameters"
    segs = []
    for n in names:
        p = oc.shift(oc.case(ecc, orc, n)[0])
        segs.append((p[:, 0].astype(np.int32), p[:, 1].astype(np.int32)))
    refs = [oc.reference(ecc, orc, shared, n) for n in names]
    return names, Packed(ecc, segs, stride), params.pop(), refs


def want_of(refs):
    return [(r["order"].astype(np.int64), r["reach"], oc.cluster_ids(r["sizes"]), len(r["sizes"])) for r in refs]


# ---------------------------------------------------------------------------- ecc_optics_grid
@pytest.mark.parametrize("key", list(LAUNCHES))
def test_optics_grid(ecc, orc, gpu, shared, key):
    """order, reach, cluster and n_clusters of every segment equal the reference's; entries past a
    segment's count keep the pre-filled values; the status is OK (asserted by run_grid)."""
    names, pk, (eps, min_pts, thr), refs = launch_inputs(ecc, orc, shared, key)
    if key in ("e10", "e2"):
        assert [int(c) for c in pk.counts][1::2] == [8192, 8192] and pk.stride == 8192
    print(f"{key}: segments {names}, eps {eps}, min_pts {min_pts} (network of "
          f"{next(k for k in (1, 2, 4, 8, 16, 32, 64) if k >= min_pts)}), threshold {thr}")
    check_against(pk, run_grid(ecc, gpu, pk, eps, min_pts, thr), want_of(refs), thr)


def test_optics_grid_is_deterministic(ecc, orc, gpu, shared):
    _, pk, (eps, min_pts, thr), _ = launch_inputs(ecc, orc, shared, "e2")
    a = run_grid(ecc, gpu, pk, eps, min_pts, thr)
    b = run_grid(ecc, gpu, pk, eps, min_pts, thr)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


# ---------------------------------------------------------------------------- ecc_optics_f64
@pytest.mark.parametrize("name", ["ties", "ties_e2", "kdtree", "blobs_mp16", "blobs_mp64"])
def test_optics_f64(ecc, orc, gpu, shared, name):
    p, eps, min_pts, _, _ = oc.case(ecc, orc, name)
    ref = oc.reference(ecc, orc, shared, name)
    order, reach = gpu.optics_f64(p.astype(np.float64), min_pts, eps)
    assert np.array_equal(order, ref["order"].astype(np.int64))
    assert np.array_equal(reach.view(np.uint64), ref["reach"].view(np.uint64))


# ---------------------------------------------------------------------------- the chain, device-resident
def run_chain(ecc, gpu, pk, eps, min_pts, thr, cap):
    """grid -> (runs statistics) and, per xi parameter set, xi -> tree -> pairs statistics; every stage reads
    the device arrays the stage before wrote.  Host copies are taken only after the last launch."""
    n, S = pk.n, pk.stride
    stat = ecc.CLUSTER_STAT_DTYPE
    d_order = ecc.DeviceArray.from_numpy(np.full(n * S, ORDER_FILL, np.int32))
    d_reach = ecc.DeviceArray.from_numpy(np.full(n * S, REACH_FILL, np.float64))
    d_cl = ecc.DeviceArray.from_numpy(np.full(n * S, CLUSTER_FILL, np.int32))
    d_ncl = ecc.DeviceArray.from_numpy(np.full(n, NCL_FILL, np.int32))
    gpu.optics_grid(pk.d_xy, n, S, pk.d_cnt, eps, min_pts, thr, d_order, d_reach, d_cl, d_ncl)
    d_runs = ecc.DeviceArray.from_numpy(np.frombuffer(bytes([STAT_PAD]) * (n * S * stat.itemsize), stat).copy())
    d_nst = ecc.DeviceArray.from_numpy(np.full(n, NST_FILL, np.int32))
    gpu.cluster_stats_runs(pk.d_xy, d_order, d_cl, n, S, pk.d_cnt, d_runs, S, d_nst)
    status = [gpu.optics_grid_status(), gpu.cluster_stats_status()]
    per_xi = []
    for chi, xi_min_pts, samd in oc.XI_PARAMS:
        d_pairs = ecc.DeviceArray.from_numpy(np.full(n * cap * 2, PAIR_PAD, np.int32))
        d_np = ecc.DeviceArray.from_numpy(np.zeros(n, np.int32))
        gpu.optics_xi(d_reach, n, S, pk.d_cnt, chi, xi_min_pts, samd, d_pairs, cap, d_np)
        d_sorted = ecc.DeviceArray.from_numpy(np.full(n * cap * 2, SORTED_FILL, np.int32))
        d_parent = ecc.DeviceArray.from_numpy(np.full(n * cap, PARENT_FILL, np.int32))
        d_level = ecc.DeviceArray.from_numpy(np.full(n * cap, LEVEL_FILL, np.int32))
        d_roots = ecc.DeviceArray.from_numpy(np.full(n, ROOTS_FILL, np.int32))
        gpu.optics_xi_tree(d_pairs, cap, d_np, n, d_sorted, d_parent, d_level, d_roots)
        d_stats = ecc.DeviceArray.from_numpy(np.frombuffer(bytes([STAT_PAD]) * (n * cap * stat.itemsize), stat).copy())
        gpu.cluster_stats_pairs(pk.d_xy, d_order, d_pairs, cap, d_np, n, S, pk.d_cnt, d_stats)
        status += [gpu.optics_xi_status(), gpu.optics_xi_tree_status(), gpu.cluster_stats_status()]
        per_xi.append((d_pairs, d_np, d_sorted, d_parent, d_level, d_roots, d_stats))
    gpu.sync()
    host = dict(order=d_order.numpy(), reach=d_reach.numpy(), runs=d_runs.numpy().reshape(n, S), n_runs=d_nst.numpy(),
                status=status, xi=[])
    for d_pairs, d_np, d_sorted, d_parent, d_level, d_roots, d_stats in per_xi:
        host["xi"].append(dict(pairs=d_pairs.numpy().reshape(n, cap, 2), n_pairs=d_np.numpy(),
                               sorted=d_sorted.numpy().reshape(n, cap, 2), parent=d_parent.numpy().reshape(n, cap),
                               level=d_level.numpy().reshape(n, cap), roots=d_roots.numpy(),
                               stats=d_stats.numpy().reshape(n, cap)))
    return host


def chain_bytes(host):
    return b"".join([host["order"].tobytes(), host["reach"].tobytes(), host["runs"].tobytes(), host["n_runs"].tobytes()] +
                    [v.tobytes() for x in host["xi"] for v in x.values()])


@pytest.mark.parametrize("key", ["e10", "e2", "kdtree", "blobs_mp9", "blobs_mp64"])
def test_chain_on_the_device(ecc, orc, gpu, shared, key):
    """Pairs and their counts, sorted / parent / level / roots and the statistics of the threshold clusters
    and of every pair equal the reference's for the three xi parameter sets; every status is OK; a second
    run gives identical bytes.  The statistics are those of the points as packed: the KAT set, moved to
    non-negative coordinates for the u16 input, is left out of the statistics comparison alone."""
    names, pk, (eps, min_pts, thr), refs = launch_inputs(ecc, orc, shared, key)
    cap = LAUNCHES[key][2]
    assert max(len(x) for r in refs for x in r["xi"]) < cap
    host = run_chain(ecc, gpu, pk, eps, min_pts, thr, cap)
    assert host["status"] == [ecc.OK] * len(host["status"])
    for s, (name, ref) in enumerate(zip(names, refs)):
        m = int(pk.counts[s])
        assert np.array_equal(host["order"][s * pk.stride: s * pk.stride + m], ref["order"]), name
        k_runs = len(ref["sizes"])
        assert int(host["n_runs"][s]) == k_runs, name
        words = [oc.stat_words(host["runs"][s, :k_runs])]
        begins = [host["runs"][s, :k_runs]["begin"]]
        assert (host["runs"][s, k_runs:].view(np.uint8) == STAT_PAD).all(), name
        forests = []
        for x, want in zip(host["xi"], ref["xi"]):
            k = len(want)
            assert int(x["n_pairs"][s]) == k and np.array_equal(x["pairs"][s, :k], want), name
            assert (x["pairs"][s, k:] == PAIR_PAD).all(), name
            placed, par, level = x["sorted"][s, :k], x["parent"][s, :k], x["level"][s, :k]
            assert ((par >= -1) & (par < k)).all() and all(p == -1 or p > i for i, p in enumerate(par.tolist())), name
            forests.append(tr.dfs(tr.forest(placed, par)))
            want_level = np.zeros(k, np.int32)
            for i in range(k - 1, -1, -1):
                want_level[i] = 0 if par[i] < 0 else want_level[par[i]] + 1
            assert np.array_equal(level, want_level) and int(x["roots"][s]) == int((par < 0).sum()), name
            assert (x["sorted"][s, k:] == SORTED_FILL).all() and (x["parent"][s, k:] == PARENT_FILL).all(), name
            assert (x["level"][s, k:] == LEVEL_FILL).all(), name
            words.append(oc.stat_words(x["stats"][s, :k]))
            begins.append(x["stats"][s, :k]["begin"])
        assert oc.same_forest(ref, forests), name
        assert np.array_equal(np.concatenate(begins), [b for b, _ in oc.intervals(ref)]), name
        if not name.startswith("kat"):
            assert oc.same_stats(ref, np.concatenate(words)), name
    assert chain_bytes(run_chain(ecc, gpu, pk, eps, min_pts, thr, cap)) == chain_bytes(host)
