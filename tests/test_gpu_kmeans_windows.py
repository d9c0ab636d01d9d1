"""ecc_kmeans_windows_xy16 (k-means per downsample window, every window in one launch) against the
oracle's orc_kmeans_run_xy16 on each window's points alone.  Outputs are pre-filled with sentinels:
labels past a window's count and everything past the last window keep them.  Comparisons are exact
(float bits, labels, sizes, iters); there are no tolerances."""
import numpy as np
import pytest

import guarded
import kmeans_windows_cases as kc

pytestmark = pytest.mark.gpu

FILL, TAIL = 0xA5, 5
FILL_I32 = np.frombuffer(bytes([FILL] * 4), np.int32)[0]
FILL_F32_BITS = np.frombuffer(bytes([FILL] * 4), np.uint32)[0]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


class Run:
    """One launch over pre-filled outputs.  starts: float32[2k] (init) or float32[n, 2k] (init =
    NULL, the rows in/out).  counts: a list, or None for full windows."""

    def __init__(self, ecc, gpu, xy, n, stride, counts, k, max_iters, thr, tol, starts, labels=True, sizes=True,
                 iters=True):
        self.n, self.stride, self.k = n, stride, k
        cfg = ecc.kmeans_cfg(k=k, max_iters=max_iters, threshold=thr, tol=tol)
        starts = np.asarray(starts, np.float32)
        d_xy = xy if isinstance(xy, ecc.DeviceArray) else ecc.DeviceArray.from_numpy(xy)
        d_cnt = None if counts is None else ecc.DeviceArray.from_numpy(np.asarray(counts, np.int32))
        cent0 = np.full(n * 2 * k + TAIL, 0, np.uint32)
        cent0[:] = FILL_F32_BITS
        d_init = None
        if starts.ndim == 1:
            d_init = ecc.DeviceArray.from_numpy(starts)
        else:
            cent0[:n * 2 * k] = bits(starts).ravel()
        self.d_cent = ecc.DeviceArray.from_numpy(cent0)
        self.d_lab = ecc.DeviceArray.from_numpy(np.full(n * stride + TAIL, FILL, np.uint8)) if labels else None
        self.d_sizes = ecc.DeviceArray.from_numpy(np.full(n * k + TAIL, FILL_I32, np.int32)) if sizes else None
        self.d_iters = ecc.DeviceArray.from_numpy(np.full(n + TAIL, FILL_I32, np.int32)) if iters else None
        self.launch = lambda: gpu.kmeans_windows(d_xy, n, stride, d_cnt, cfg, d_init, self.d_cent, self.d_lab,
                                                 self.d_sizes, self.d_iters)
        self.launch()
        gpu.sync()
        self.keep = (d_xy, d_cnt, d_init)

    def outputs(self):
        """(centroid bits, labels, sizes, iters), each with its sentinel tail; None where not asked for."""
        return tuple(None if d is None else d.numpy() for d in (self.d_cent, self.d_lab, self.d_sizes, self.d_iters))


def check(run, want, counts):
    cent, lab, sizes, iters = run.outputs()
    n, k, stride = run.n, run.k, run.stride
    assert want.n == n and want.k == k
    assert (cent[n * 2 * k:] == FILL_F32_BITS).all(), "centroids past the last window"
    got_c = cent[:n * 2 * k].reshape(n, 2 * k)
    for w in range(n):
        assert np.array_equal(got_c[w], bits(want.cent[w])), f"centroids, window {w}"
    if iters is not None:
        assert (iters[n:] == FILL_I32).all(), "iters past the last window"
        assert iters[:n].tolist() == want.iters.tolist()
    if sizes is not None:
        assert (sizes[n * k:] == FILL_I32).all(), "sizes past the last window"
        assert np.array_equal(sizes[:n * k].reshape(n, k), want.sizes)
    if lab is not None:
        assert (lab[n * stride:] == FILL).all(), "labels past the last window"
        for w in range(n):
            c = min(max(int(counts[w]), 0), stride) if counts is not None else stride
            row = lab[w * stride:(w + 1) * stride]
            assert np.array_equal(row[:c], want.labels[w]), f"labels, window {w}"
            assert (row[c:] == FILL).all(), f"labels past the count, window {w}"


# ------------------------------------------------------------------------------ 1-3, 9-11: ragged windows
@pytest.fixture(scope="module")
def ragged():
    return kc.ragged_windows()


@pytest.fixture(scope="module")
def ragged_xy(ecc, ragged):
    return ecc.DeviceArray.from_numpy(kc.layout(ragged, kc.RAGGED_STRIDE))


@pytest.fixture(scope="module")
def ragged_want(orc, ragged):
    r = kc.RAGGED
    return kc.Want(orc, ragged, kc.grid_init(r["k"]), r["max_iters"], r["thr"], r["tol"])


def run_ragged(ecc, gpu, ragged_xy, starts=None, **kw):
    r = dict(kc.RAGGED, **{a: kw.pop(a) for a in ("max_iters", "tol") if a in kw})
    return Run(ecc, gpu, ragged_xy, len(kc.RAGGED_COUNTS), kc.RAGGED_STRIDE, kc.RAGGED_COUNTS, r["k"], r["max_iters"],
               r["thr"], r["tol"], kc.grid_init(r["k"]) if starts is None else starts, **kw)


@pytest.fixture(scope="module")
def ragged_run(ecc, gpu, ragged_xy):
    return run_ragged(ecc, gpu, ragged_xy)


def test_ragged_input_exercises_what_it_claims(ragged_want):
    """On the oracle's results: windows stop after different numbers of updates, one of them at
    max_iters; points beyond the threshold (label 255) and centres without points exist."""
    w = ragged_want
    assert len(set(w.iters.tolist())) >= 4
    assert (w.iters == kc.RAGGED["max_iters"]).any() and (w.iters < kc.RAGGED["max_iters"]).any()
    assert any((lab == 255).any() for lab in w.labels)
    assert ((w.sizes == 0) & (np.array(kc.RAGGED_COUNTS)[:, None] > 0)).any()
    assert w.iters[0] == 1 and w.iters[-1] == 1 and (w.sizes[0] == 0).all()  # the empty windows


def test_ragged_windows(ragged_run, ragged_want):
    check(ragged_run, ragged_want, kc.RAGGED_COUNTS)


@pytest.mark.parametrize("tol,max_iters", [(-1.0, 10), (0.01, 5), (0.01, 0), (-1.0, 0)])
def test_ragged_windows_fixed_passes(ecc, gpu, orc, ragged, ragged_xy, tol, max_iters):
    """tol < 0: every window runs all passes; max_iters = 5: several windows stop at the cap, others
    before it; max_iters = 0: labels against the starting centres, iters = 0."""
    r = kc.RAGGED
    want = kc.Want(orc, ragged, kc.grid_init(r["k"]), max_iters, r["thr"], tol)
    if tol < 0 or max_iters == 0:
        assert (want.iters == max_iters).all()
    else:
        assert (want.iters == max_iters).sum() >= 2 and (want.iters < max_iters).sum() >= 2
    check(run_ragged(ecc, gpu, ragged_xy, max_iters=max_iters, tol=tol), want, kc.RAGGED_COUNTS)


def test_init_null_rows_equal_init(ecc, gpu, ragged_xy, ragged_run):
    """init = NULL with every row set to the grid: the same bytes as with init."""
    n, k = len(kc.RAGGED_COUNTS), kc.RAGGED["k"]
    rows = np.tile(kc.grid_init(k), (n, 1))
    got, ref = run_ragged(ecc, gpu, ragged_xy, starts=rows).outputs(), ragged_run.outputs()
    for a, b in zip(got, ref):
        assert np.array_equal(a, b)


def test_init_null_rows_per_window(ecc, gpu, orc, ragged, ragged_xy):
    """Every window from its own first k points (the grid where it has fewer)."""
    n, k, r = len(ragged), kc.RAGGED["k"], kc.RAGGED
    rows = np.tile(kc.grid_init(k), (n, 1))
    for w, p in enumerate(ragged):
        m = min(len(p), k)
        rows[w, 0:2 * m:2], rows[w, 1:2 * m:2] = p[:m] & 0xFFFF, p[:m] >> 16
    assert len({rows[w].tobytes() for w in range(n)}) >= n - 3
    want = kc.Want(orc, ragged, rows, r["max_iters"], r["thr"], r["tol"])
    check(run_ragged(ecc, gpu, ragged_xy, starts=rows), want, kc.RAGGED_COUNTS)


@pytest.mark.parametrize("drop", [("labels",), ("sizes",), ("iters",), ("labels", "sizes", "iters")],
                         ids=lambda d: "+".join(d))
def test_optional_outputs(ecc, gpu, ragged_xy, ragged_run, drop):
    got = run_ragged(ecc, gpu, ragged_xy, **{d: False for d in drop}).outputs()
    for name, a, b in zip(("centroids", "labels", "sizes", "iters"), got, ragged_run.outputs()):
        assert a is None if name in drop else np.array_equal(a, b), name


def test_against_run_xy16_on_the_device(ecc, gpu, ragged_xy, ragged_run):
    """ecc_kmeans_run_xy16 on the interior pointer of a window (n_segs = 1) gives that window's row."""
    r, stride = kc.RAGGED, kc.RAGGED_STRIDE
    cfg = ecc.kmeans_cfg(k=r["k"], max_iters=r["max_iters"], threshold=r["thr"], tol=r["tol"])
    cent, lab, _, iters = ragged_run.outputs()
    d_counts = ecc.DeviceArray.from_numpy(np.asarray(kc.RAGGED_COUNTS, np.int32))
    for w in (4, 8, 12):
        c = kc.RAGGED_COUNTS[w]
        d_c = ecc.DeviceArray.from_numpy(kc.grid_init(r["k"]))
        d_l, d_it = ecc.DeviceArray.from_numpy(np.full(stride, FILL, np.uint8)), ecc.DeviceArray(1, np.int32)
        ecc.check(ecc.lib.ecc_kmeans_run_xy16(gpu.ctx, ragged_xy.ptr + 4 * w * stride, 1, stride, d_counts.ptr + 4 * w,
                                              ecc.C.byref(cfg), d_c.ptr, d_l.ptr, d_it.ptr, gpu.stream))
        gpu.sync()
        assert np.array_equal(bits(d_c.numpy()), cent[w * 2 * r["k"]:(w + 1) * 2 * r["k"]]), w
        assert np.array_equal(d_l.numpy()[:c], lab[w * stride: w * stride + c]), w
        assert int(d_it.numpy()[0]) == int(iters[w]), w


def test_graph_capture(ecc, gpu, ragged_xy, ragged_run):
    """One eager call, then capture and two replays on a created stream: equal outputs each time."""
    lib = ecc.lib
    run = run_ragged(ecc, gpu, ragged_xy)  # eager (and any LDS grant) before the capture
    eager = run.outputs()
    for a, b in zip(eager, ragged_run.outputs()):
        assert np.array_equal(a, b)
    gp = ecc.P()
    ecc.check(lib.ecc_graph_begin(gpu.stream))
    run.launch()
    ecc.check(lib.ecc_graph_end(gpu.stream, ecc.C.byref(gp)))
    try:
        for _ in range(2):
            # poison what the call writes (the centroids are output only: init is given)
            for d, img in zip((run.d_cent, run.d_lab, run.d_sizes, run.d_iters), eager):
                d.copy_from(np.full(img.shape, 0x5A5A5A5A if img.itemsize == 4 else 0xA5).astype(img.dtype),
                            gpu.stream)
            ecc.check(lib.ecc_graph_launch(gp.value, gpu.stream))
            gpu.sync()
            cent, lab, sizes, iters = run.outputs()
            n, k, stride = run.n, run.k, run.stride
            assert np.array_equal(cent[:n * 2 * k], eager[0][:n * 2 * k])
            assert np.array_equal(sizes[:n * k], eager[2][:n * k]) and np.array_equal(iters[:n], eager[3][:n])
            inside = (np.arange(stride)[None, :] < np.clip(kc.RAGGED_COUNTS, 0, stride)[:, None]).ravel()
            assert np.array_equal(lab[:n * stride][inside], eager[1][:n * stride][inside])
            assert (lab[:n * stride][~inside] == 0xA5).all()
    finally:
        ecc.check(lib.ecc_graph_destroy(gp.value))


def test_timing_report_names_the_launch(ecc, gpu, ragged_xy, ragged_run):
    """With per-kernel timing on, the call is one launch under the kernel's name, with the same outputs."""
    gpu.set_timing(True)
    try:
        gpu.timing_reset()
        got = run_ragged(ecc, gpu, ragged_xy).outputs()
        report = gpu.timing_report()
    finally:
        gpu.set_timing(False)
    assert report["kmeans_windows_kernel"]["launches"] == 1 and report["kmeans_windows_kernel"]["total_ms"] > 0
    for a, b in zip(got, ragged_run.outputs()):
        assert np.array_equal(a, b)


# ------------------------------------------------------------------------------ 4. k sweep
@pytest.mark.parametrize("k", [1, 2, 8, 17, 64])
def test_k_sweep(ecc, gpu, orc, k):
    """Every padded centre count (16, 32, 64) and k below, at and above one; 17 and 64 are no squares' grids."""
    rng = np.random.default_rng(kc.SEED + k)
    counts = [65, 300, 1025]
    wins = [kc.blob_window(rng, c) for c in counts]
    start = kc.grid_init(k)
    want = kc.Want(orc, wins, start, 12, 30.0, 0.01)
    assert any((lab == 255).any() for lab in want.labels) or k == 64
    check(Run(ecc, gpu, kc.layout(wins, 1028), 3, 1028, counts, k, 12, 30.0, 0.01, start), want, counts)


# ------------------------------------------------------------------------------ 5. ties and duplicates
def pack(x, y):
    return (np.asarray(x, np.uint32) | (np.asarray(y, np.uint32) << 16)).astype(np.uint32)


def test_ties_and_duplicates(ecc, gpu, orc):
    k, thr = 4, 20.0
    # centres at half-integers; (12, 10) and (10, 12) ... are equidistant from centres 0/1 and 2/3
    start = np.array([10.5, 10.5, 13.5, 10.5, 10.5, 13.5, 30.5, 40.5], np.float32)
    gx, gy = np.meshgrid(np.arange(6, 19), np.arange(6, 19))
    ties = pack(gx.ravel(), gy.ravel())  # the column x = 12 ties centres 0 and 1, the row y = 12 centres 0 and 2
    dup = pack(np.full(300, 31), np.full(300, 41))
    far = pack(np.arange(200) % 50 + 200, np.arange(200) // 50 + 150)
    wins, counts = [ties, dup, far], [len(ties), 300, 200]
    # max_iters = 0: the labels are the assignment against the starting centres
    w0 = kc.Want(orc, wins, start, 0, thr, 0.01)
    on_tie = (gx.ravel() == 12) & (gy.ravel() < 12)
    assert on_tie.sum() == 6 and (w0.labels[0][on_tie] == 0).all(), "the lower index wins a tie"
    check(Run(ecc, gpu, kc.layout(wins, 300), 3, 300, counts, k, 0, thr, 0.01, start), w0, counts)
    want = kc.Want(orc, wins, start, 10, thr, 0.01)
    assert (want.labels[1] == 3).all() and want.sizes[1].tolist() == [0, 0, 0, 300]
    assert np.array_equal(want.cent[1][6:], np.array([31, 41], np.float32))
    # beyond the threshold from every centre: all 255, centres unchanged, one update with tol >= 0
    assert (want.labels[2] == 255).all() and np.array_equal(bits(want.cent[2]), bits(start)) and want.iters[2] == 1
    check(Run(ecc, gpu, kc.layout(wins, 300), 3, 300, counts, k, 10, thr, 0.01, start), want, counts)


# ------------------------------------------------------------------------------ 6. sum range
def test_sum_range_at_the_largest_stride(ecc, gpu, orc):
    """16384 points at (65535, 65535): sums of 2^30 - 16384 per coordinate, exact in 32-bit fields and
    in none narrower than 30 bits; the stride needs the LDS grant above 64 KiB."""
    stride = 16384
    win = np.full(stride, 0xFFFFFFFF, np.uint32)
    start = np.zeros(2, np.float32)
    want = kc.Want(orc, [win], start, 5, 1e9, 0.01)
    assert np.array_equal(want.cent[0], np.array([65535, 65535], np.float32)) and want.sizes[0, 0] == stride
    run = Run(ecc, gpu, win, 1, stride, None, 1, 5, 1e9, 0.01, start)
    check(run, want, None)
    cent = run.outputs()[0][:2].view(np.float32)
    assert cent.tolist() == [65535.0, 65535.0]


# ------------------------------------------------------------------------------ 7. more segments than workgroups
def test_more_segments_than_workgroups(ecc, gpu, orc):
    cap = ecc.KMEANS_WINDOWS_MAX_GRID
    n, stride, k = cap + 37, 8, 2
    rng = np.random.default_rng(kc.SEED + 7)
    counts = [w % 9 for w in range(n)]
    wins = [pack(rng.integers(0, 40, c), rng.integers(0, 40, c)) for c in counts]
    start = np.array([10, 10, 30, 30], np.float32)
    want = kc.Want(orc, wins, start, 6, 25.0, 0.0)
    assert len(set(want.iters.tolist())) >= 2
    check(Run(ecc, gpu, kc.layout(wins, stride), n, stride, counts, k, 6, 25.0, 0.0, start), want, counts)


# ------------------------------------------------------------------------------ 8. extents at bare alignment
@pytest.mark.parametrize("placement", ["aligned", "bare"])
def test_extents(ecc, gpu, orc, placement):
    """Stride 250 (no multiple of 4: window label bases at every residue), 5 windows; inputs with
    hostile tails, outputs between guard bands."""
    n, stride, k = 5, 250, 8
    rng = np.random.default_rng(kc.SEED + 8)
    counts = [250, 0, 249, 7, 130]
    wins = [kc.blob_window(rng, c) for c in counts]
    start = kc.grid_init(k)
    want = kc.Want(orc, wins, start, 8, 40.0, 0.01)
    # the last window's points end at its count: what follows is tail
    xy = kc.layout(wins, stride)[:(n - 1) * stride + counts[-1]]
    g_xy = guarded.guarded_in(ecc, xy, placement, tail=np.full(64, 0x00050005, np.uint32))
    g_cnt = guarded.guarded_in(ecc, np.asarray(counts, np.int32), placement, tail=np.full(16, 250, np.int32))
    g_init = guarded.guarded_in(ecc, start, placement, tail=np.full(16, 100.0, np.float32))
    g_cent = guarded.guarded_out(ecc, np.float32, n * 2 * k, placement)
    g_lab = guarded.guarded_out(ecc, np.uint8, (n - 1) * stride + counts[-1], placement)
    g_sizes = guarded.guarded_out(ecc, np.int32, n * k, placement)
    g_iters = guarded.guarded_out(ecc, np.int32, n, placement)
    if placement == "bare":
        assert g_lab.ptr % 4 == 1 and g_xy.ptr % 16 == 4
    cfg = ecc.kmeans_cfg(k=k, max_iters=8, threshold=40.0, tol=0.01)
    gpu.kmeans_windows(g_xy, n, stride, g_cnt, cfg, g_init, g_cent, g_lab, g_sizes, g_iters)
    gpu.sync()
    guarded.check_all(xy=g_xy, seg_counts=g_cnt, init=g_init, centroids=g_cent, labels=g_lab, sizes=g_sizes,
                      iters=g_iters)
    assert np.array_equal(bits(g_cent.numpy()), bits(want.cent).ravel())
    assert np.array_equal(g_sizes.numpy().reshape(n, k), want.sizes) and g_iters.numpy().tolist() == want.iters.tolist()
    lab, untouched = g_lab.numpy(), g_lab.untouched()
    for w, c in enumerate(counts):
        assert np.array_equal(lab[w * stride: w * stride + c], want.labels[w]), w
        assert untouched[w * stride + c:(w + 1) * stride].all(), f"labels past the count, window {w}"
