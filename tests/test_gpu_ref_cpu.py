"""The tests of tests/test_ref_cpu.py against the DEVICE: the HIP kernels are compared with the
reference's own CPU code directly (oracle/_ref/ref_cpu, or its recorded outputs under
tests/golden/ref_cpu/), not through the oracle.  Same inputs (tests/ref_cpu_cases.py), every
comparison exact, floats by bit pattern."""
import numpy as np
import pytest

import ref_cpu_cases as rc

pytestmark = pytest.mark.gpu
CAP = 4096


def dev(ecc, a):
    return ecc.DeviceArray.from_numpy(np.ascontiguousarray(a))


def _device_arc(ecc, gpu, c, border_mode=1):
    """ecc_fast_detect -> (per-slice corner lists, final surface)."""
    n = len(c["xy"])
    cfg = ecc.corner_cfg(width=rc.W, height=rc.H, slice_events=c["slice"], border_mode=border_mode,
                         first_detect_slice=c["first"])
    sae = dev(ecc, np.zeros(rc.W * rc.H, np.int64) if c["sae0"] is None else c["sae0"])
    flags = ecc.DeviceArray(n, np.uint8)
    flags.fill_bytes(0xCD)  # every flag must be written
    gpu.fast_detect(dev(ecc, c["xy"]), dev(ecc, c["t"]), n, cfg, sae, flags)
    assert gpu.fast_detect_status() == 0
    f = flags.numpy()
    assert set(np.unique(f).tolist()) <= {0, 1}
    return rc.slice_corners_from_flags(ecc, c["xy"], f, c["slice"]), sae.numpy()


def _ref_arc_case(ecc, tmp_path, name):
    c = rc.arc_case(ecc, name)
    return c, rc.ref_arc(f"arc_{name}", tmp_path, c["xy"], c["t"], c["slice"], flag0=1 if c["first"] == 0 else 0,
                         sae0=c["sae0"])


@pytest.mark.parametrize("name", rc.ARC_CASES)
def test_arc_lambda(ecc, gpu, tmp_path, name):
    """ecc_fast_detect (border_mode 1) against the verbatim lambda run once per slice."""
    c, ref = _ref_arc_case(ecc, tmp_path, name)
    assert sum(len(l) for l in ref["corners"]) > 100
    got, sae = _device_arc(ecc, gpu, c)
    bad = [s for s, (a, b) in enumerate(zip(got, ref["corners"])) if not np.array_equal(a, b)]
    assert not bad, (bad, [(len(got[s]), len(ref["corners"][s])) for s in bad])
    assert rc.same_surface(ref, sae)


def test_arc_lambda_border_break_cuts_slices(ecc, gpu, tmp_path):
    """No border event in the stream: border_mode 0 equals the reference as well."""
    c, ref = _ref_arc_case(ecc, tmp_path, "interior")
    got, sae = _device_arc(ecc, gpu, c, border_mode=0)
    assert rc.same_lists(got, ref["corners"]) and rc.same_surface(ref, sae)


@pytest.mark.parametrize("name", ["t53", "t53_groups40"])
def test_arc_lambda_beyond_2p53(ecc, gpu, tmp_path, name):
    """Timestamps passing 2^53: the device must give the reference's answer (the arc scanned in
    double), which on these streams is not the pure int64 one (tests/test_ref_cpu.py shows it)."""
    c, ref = _ref_arc_case(ecc, tmp_path, name)
    low = rc.ref_arc(f"arc_{name}_low", tmp_path, c["xy"], c["t"] - (1 << 52), c["slice"])
    assert not rc.same_lists(ref["corners"], low["corners"])
    got, sae = _device_arc(ecc, gpu, c)
    n_got, n_ref, n_low = (sum(len(l) for l in x) for x in (got, ref["corners"], low["corners"]))
    print(f"{name}: device {n_got}, reference {n_ref}, int64 {n_low} corners")
    bad = [s for s, (a, b) in enumerate(zip(got, ref["corners"])) if not np.array_equal(a, b)]
    assert not bad, (bad, n_got, n_ref, n_low)
    assert rc.same_surface(ref, sae)
    # the same stream 2^52 earlier takes the integer paths and gives the int64 answer
    c_low = dict(c, t=c["t"] - (1 << 52))
    assert rc.same_lists(_device_arc(ecc, gpu, c_low)[0], low["corners"])


def _device_nms(ecc, gpu, xy, flags, slice_events):
    ns = (len(xy) + slice_events - 1) // slice_events
    out = ecc.DeviceArray(ns * CAP, ecc.CORNER_DTYPE)
    cnt = ecc.DeviceArray(ns, np.int32)
    gpu.corner_nms(dev(ecc, xy), dev(ecc, flags), len(xy), slice_events, rc.W, rc.H, 15, CAP, out, cnt)
    assert gpu.corner_nms_status() == 0
    return out, cnt


def _nms_lists(out, cnt):
    o, k = out.numpy(), cnt.numpy()
    return [np.stack([o["x"][s * CAP: s * CAP + k[s]], o["y"][s * CAP: s * CAP + k[s]],
                      o["label"][s * CAP: s * CAP + k[s]]], 1).reshape(-1, 3) for s in range(len(k))]


def test_corner_filter(ecc, gpu, tmp_path):
    """ecc_corner_nms against CornerFilter::filterCorners per slice (box 15)."""
    lists = rc.nms_slices()
    ref = rc.ref_nms("nms", tmp_path, lists)
    xy, flags = rc.nms_as_events(lists)
    got = _nms_lists(*_device_nms(ecc, gpu, xy, flags, rc.NMS_SLICE))
    for s in range(len(lists)):
        assert np.array_equal(got[s], ref[s]), s


def _check_tracker(ecc, tr, tracks, groups, s):
    assert tr.status() == 0
    assert [rc.struct_track_key(t) for t in tr.tracks()] == [rc.track_key(t) for t in tracks], s
    assert rc.struct_group_keys(*tr.groups()) == groups, s


def test_corner_tracker(ecc, gpu, tmp_path):
    """ecc_tracker_update, one slice per call, with ecc_tracker_get_tracks / _get_groups after each,
    against CornerTracker::updateTrackedCorners and getCornerGroups after each slice; then the 60
    slices in ONE launch must end in the same state."""
    lists = rc.tracker_slices()
    dump = rc.ref_track("track", tmp_path, lists)
    ns = len(lists)
    corners = np.zeros(ns * 64, ecc.CORNER_DTYPE)
    counts = np.array([len(l) for l in lists], np.int32)
    for s, l in enumerate(lists):
        corners["x"][s * 64: s * 64 + len(l)] = l[:, 0]
        corners["y"][s * 64: s * 64 + len(l)] = l[:, 1]
        corners["label"][s * 64: s * 64 + len(l)] = l[:, 2]
    tr = ecc.Tracker(gpu, max_tracks=256, max_detections=64)
    for s in range(ns):
        tr.update(dev(ecc, corners[s * 64: (s + 1) * 64]), dev(ecc, counts[s: s + 1]), 1, 64)
        _check_tracker(ecc, tr, *dump[s], s)
    tr.close()
    tr = ecc.Tracker(gpu, max_tracks=256, max_detections=64)
    tr.update(dev(ecc, corners), dev(ecc, counts), ns, 64)
    _check_tracker(ecc, tr, *dump[-1], ns - 1)
    tr.close()


def test_chain(ecc, gpu, tmp_path):
    """ecc_fast_detect_nms -> ecc_tracker_update over the 8-slice stream against the reference's
    arc -> filterCorners -> updateTrackedCorners: corners and NMS output of every slice, final
    surface, final tracks and groups."""
    xy, t = rc.stream_border_mid(ecc, 8 * rc.SLICE, 8)
    ref = rc.ref_chain("chain", tmp_path, xy, t)
    n, ns = len(xy), 8
    cfg = ecc.corner_cfg(width=rc.W, height=rc.H, border_mode=1)
    sae = ecc.DeviceArray.zeros(rc.W * rc.H, np.int64)
    flags = ecc.DeviceArray(n, np.uint8)
    out = ecc.DeviceArray(ns * CAP, ecc.CORNER_DTYPE)
    cnt = ecc.DeviceArray(ns, np.int32)
    gpu.fast_detect_nms(dev(ecc, xy), dev(ecc, t), n, cfg, sae, flags, 15, CAP, out, cnt)
    assert gpu.fast_detect_status() == 0 and gpu.corner_nms_status() == 0
    assert rc.same_lists(rc.slice_corners_from_flags(ecc, xy, flags.numpy(), rc.SLICE), ref["corners"])
    assert rc.same_surface(ref, sae.numpy())
    got = _nms_lists(out, cnt)
    for s in range(ns):
        assert np.array_equal(got[s], ref["nms"][s]), s
    tr = ecc.Tracker(gpu)
    tr.update(out, cnt, ns, CAP)
    _check_tracker(ecc, tr, *ref["track"][-1], ns - 1)
    tr.close()


def _device_dbscan_cloud(ecc, gpu, pts, eps, min_pts, min_size, max_size):
    n, dim = pts.shape
    dup_cap = 1 << 16
    lab, nc = ecc.DeviceArray(n, np.int32), ecc.DeviceArray(1, np.int32)
    dups, nd = ecc.DeviceArray(2 * dup_cap, np.int64), ecc.DeviceArray(1, np.int64)
    gpu.dbscan_cloud(dev(ecc, pts.ravel()), n, dim, eps, min_pts, min_size, max_size, lab, nc, dups, dup_cap, nd)
    assert gpu.dbscan_cloud_status() == 0
    k = int(nd.numpy()[0])
    return rc.clusters_from_labels(n, lab.numpy(), dups.numpy()[:2 * k].reshape(-1, 2), int(nc.numpy()[0]))


def _device_dbscan_grid(ecc, gpu, pts, eps, min_pts, min_size, max_size):
    n = len(pts)
    xy = (pts[:, 0].astype(np.uint32) | (pts[:, 1].astype(np.uint32) << 16)).astype(np.uint32)
    dup_cap = 1 << 16
    lab, nc = ecc.DeviceArray(n, np.int32), ecc.DeviceArray(1, np.int32)
    dups, nd = ecc.DeviceArray(2 * dup_cap, np.int64), ecc.DeviceArray(1, np.int64)
    gpu.dbscan_grid(dev(ecc, xy), 1, n, None, eps, min_pts, min_size, max_size, lab, nc, dups, dup_cap, nd)
    assert gpu.dbscan_status() == 0
    k = int(nd.numpy()[0])
    return rc.clusters_from_labels(n, lab.numpy(), dups.numpy()[:2 * k].reshape(-1, 2), int(nc.numpy()[0]))


def _same_clusters(got, ref):
    return len(got) == len(ref) and all(np.array_equal(a, b) for a, b in zip(got, ref))


def test_dbscan_simple_integer_cloud(ecc, gpu, tmp_path):
    """ecc_dbscan_cloud_f32 (x, y, 0) and ecc_dbscan_grid (integer pixels) against
    DBSCANSimpleCluster::extract: the clusters in output order, double memberships included."""
    pts = rc.dbscan_points()
    for case, a in (("dbscan_int", (rc.DBSCAN_EPS, rc.DBSCAN_MIN_PTS, rc.DBSCAN_MIN_SIZE, rc.DBSCAN_MAX_SIZE)),
                    ("dbscan_int_all", (rc.DBSCAN_EPS, rc.DBSCAN_MIN_PTS, 1, 1 << 30)),
                    ("dbscan_int_closer", (float(np.nextafter(rc.DBSCAN_EPS, 0)), rc.DBSCAN_MIN_PTS, rc.DBSCAN_MIN_SIZE,
                                           rc.DBSCAN_MAX_SIZE))):
        ref = rc.ref_dbscan(case, tmp_path, pts, *a)
        assert len(ref) >= 5
        assert _same_clusters(_device_dbscan_cloud(ecc, gpu, pts, *a), ref), case
        assert _same_clusters(_device_dbscan_grid(ecc, gpu, pts, *a), ref), case


def test_dbscan_simple_float_cloud(ecc, gpu, tmp_path):
    pts = rc.dbscan_float_points()
    ref = rc.ref_dbscan("dbscan_float", tmp_path, pts, 3.0, 8, 20, 2000)
    assert len(ref) >= 2
    assert _same_clusters(_device_dbscan_cloud(ecc, gpu, pts, 3.0, 8, 20, 2000), ref)
