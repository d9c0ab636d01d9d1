"""The greedy NMS pass over the candidate lists (csrc/nms.hip, nms_batch_kernel) in each of its build
shapes: one wave per slice taking chunks of 64, several to a round trip (the default), or
ECC_NMS_WAVES waves, where every lane probes one candidate of a batch against the kept-centre grid
as it stood before the batch, the survivors are listed in candidate order, and one wave runs the
greedy chunk code over that list.  Each case is built for one edge of those shapes (batch, chunk and
load-group boundaries, more survivors than one chunk, a survivor dropped by a centre kept earlier
in the same batch, ...), goes through ecc_corner_nms (the candidate lists from nms_compact_kernel)
and, where events can produce it, ecc_fast_detect_nms (the lists from the flag pass), and is
compared with the oracle's orc.corner_nms: kept xy, ranks, counts and the status.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W0, H0 = 346, 260


def dev(ecc, a):
    return ecc.DeviceArray.from_numpy(np.ascontiguousarray(a))


def slices_of(ecc, lists, S, filler=(1, 1)):
    """One slice of S events per candidate list: the list's points flagged, in order, spread evenly
    over the slice's slots, every other event an unflagged filler."""
    xy = np.full(len(lists) * S, ecc.pack_xy(*filler), np.uint32)
    flags = np.zeros(len(lists) * S, np.uint8)
    for s, pts in enumerate(lists):
        pts = np.asarray(pts, np.int64).reshape(-1, 2)
        assert len(pts) <= S
        at = s * S + (np.arange(len(pts)) * S) // max(len(pts), 1)
        xy[at] = ecc.pack_xy(pts[:, 0], pts[:, 1])
        flags[at] = 1
    return xy, flags


def check_nms(ecc, orc, gpu, xy, flags, W, H, S, box=15, cap=4096, o_flags=None, status=None):
    """ecc_corner_nms against orc.corner_nms (on o_flags where the GPU is to skip a candidate)."""
    o_out, o_cnt, rc = orc.corner_nms(xy, flags if o_flags is None else o_flags, W, H, slice_events=S, box=box, cap=cap)
    ns = len(o_cnt)
    d_out = ecc.DeviceArray(max(ns * cap, 1), ecc.CORNER_DTYPE)
    d_cnt = ecc.DeviceArray(ns, np.int32)
    ecc.check(ecc.lib.ecc_memset_async(d_cnt.ptr, 0xA5, d_cnt.nbytes, gpu.stream))
    gpu.corner_nms(dev(ecc, xy), dev(ecc, flags), len(xy), S, W, H, box, cap, d_out, d_cnt)
    want = (ecc.ERR_CAPACITY if rc else 0) if status is None else status
    assert gpu.corner_nms_status() == want
    g_cnt, g_out = d_cnt.numpy(), d_out.numpy()
    assert (g_cnt == o_cnt).all(), (g_cnt, o_cnt)
    for s in range(ns):
        k = o_cnt[s]
        assert (g_out[s * cap: s * cap + k] == o_out[s * cap: s * cap + k]).all(), s
    return o_out, o_cnt


def rand_pts(rng, m, W, H):
    return np.stack([rng.integers(0, W, m), rng.integers(0, H, m)], 1)


LATTICE = np.array([(x, y) for y in range(0, H0, 15) for x in range(0, W0, 15)])  # 24 x 18, all kept at box 15


@pytest.mark.parametrize("nc", [0, 1, 63, 64, 65, 255, 256, 257, 511, 512, 513])
def test_candidate_counts_at_batch_and_chunk_edges(ecc, orc, gpu, nc):
    rng = np.random.default_rng(100 + nc)
    lists = [rand_pts(rng, nc, W0, H0), rand_pts(rng, 300, W0, H0), rand_pts(rng, nc, 90, 70)]
    xy, flags = slices_of(ecc, lists, 1024)
    _, o_cnt = check_nms(ecc, orc, gpu, xy, flags, W0, H0, 1024)
    assert nc == 0 or o_cnt[0] > 0


def test_every_event_a_candidate(ecc, orc, gpu):
    """n_cand == S, in a full slice and in a ragged last one."""
    rng = np.random.default_rng(7)
    S = 1024
    n = 2 * S + 516
    p = rand_pts(rng, n, W0, H0)
    xy, flags = ecc.pack_xy(p[:, 0], p[:, 1]), np.ones(n, np.uint8)
    check_nms(ecc, orc, gpu, xy, flags, W0, H0, S)


def test_more_survivors_than_one_chunk(ecc, orc, gpu):
    """A 15-px lattice: nobody reaches anybody, so the first batch of 256 has 256 survivors."""
    xy, flags = slices_of(ecc, [LATTICE, LATTICE[::-1]], 512)
    _, o_cnt = check_nms(ecc, orc, gpu, xy, flags, W0, H0, 512)
    assert (o_cnt == len(LATTICE)).all() and len(LATTICE) == 432


def test_survivor_dropped_by_a_centre_kept_earlier_in_its_batch(ecc, orc, gpu):
    """Candidates 64 .. 127 survive the batch probe (the grid is empty) and so do 0 .. 63, which are
    all kept; every second one of 64 .. 127 lies within reach of one of those, the others not."""
    first = LATTICE[:64]
    near = np.minimum(first + np.array([3, 5]), [W0 - 1, H0 - 1])
    far = LATTICE[200:264]
    second = np.where((np.arange(64) % 2 == 0)[:, None], near, far)
    xy, flags = slices_of(ecc, [np.concatenate([first, second]), np.concatenate([first, second, near, LATTICE])], 1024)
    _, o_cnt = check_nms(ecc, orc, gpu, xy, flags, W0, H0, 1024)
    assert o_cnt[0] == 64 + 32


def test_chain_at_pitch_8_across_a_batch_boundary(ecc, orc, gpu):
    rows = [np.stack([np.arange(0, W0, 8), np.full(44, y)], 1) for y in range(0, 160, 20)]  # 8 rows of 44
    pts = np.concatenate(rows)
    assert len(pts) > 257 and 256 % 44 not in (0, 43)  # the boundary falls inside a row
    xy, flags = slices_of(ecc, [pts, pts[::-1]], 512)
    _, o_cnt = check_nms(ecc, orc, gpu, xy, flags, W0, H0, 512)
    assert o_cnt[0] == 8 * 22


def test_duplicates_of_one_pixel_over_three_batches(ecc, orc, gpu):
    dup = np.tile([[100, 100]], (600, 1))
    mixed = dup.copy()
    mixed[::97] = LATTICE[:7]
    xy, flags = slices_of(ecc, [dup, mixed], 1024)
    _, o_cnt = check_nms(ecc, orc, gpu, xy, flags, W0, H0, 1024)
    assert o_cnt[0] == 1


@pytest.mark.parametrize("at", [5, 70, 300, 599])
def test_out_of_frame_candidate_is_skipped_and_reported(ecc, orc, gpu, at):
    """The candidate outside the sensor sits in the first batch, in a later chunk or in a later batch;
    its clamped position is within reach of a kept centre, and it is reported all the same."""
    rng = np.random.default_rng(at)
    pts = rand_pts(rng, 600, W0, H0)
    pts[0] = (W0 - 2, 10)
    for bad in ((W0 + 3, 10), (10, H0), (40000, 40000)):
        p = pts.copy()
        p[at] = bad
        xy, flags = slices_of(ecc, [p, pts], 1024)
        skipped = flags.copy()
        skipped[np.flatnonzero(flags)[at]] = 0
        check_nms(ecc, orc, gpu, xy, flags, W0, H0, 1024, o_flags=skipped, status=ecc.ERR_INVALID)
    xy, flags = slices_of(ecc, [pts, pts], 1024)
    check_nms(ecc, orc, gpu, xy, flags, W0, H0, 1024)  # the status word is cleared by the next call


@pytest.mark.parametrize("cap", [0, 1, 100, 431, 432])
def test_capacity_below_the_kept_count(ecc, orc, gpu, cap):
    xy, flags = slices_of(ecc, [LATTICE, LATTICE[:50]], 512)
    _, o_cnt = check_nms(ecc, orc, gpu, xy, flags, W0, H0, 512, cap=cap,
                         status=ecc.ERR_CAPACITY if cap < 432 else 0)
    assert o_cnt[0] == cap and o_cnt[1] == min(cap, 50)


@pytest.mark.parametrize("W,H", [(346, 260), (30, 30), (15, 1)])
@pytest.mark.parametrize("box", [1, 3, 15, 31])
def test_boxes_and_sensors(ecc, orc, gpu, W, H, box):
    rng = np.random.default_rng(box * 1000 + W)
    lists = [rand_pts(rng, m, W, H) for m in (700, 257, 64)]
    xy, flags = slices_of(ecc, lists, 1024, filler=(0, 0))
    check_nms(ecc, orc, gpu, xy, flags, W, H, 1024, box=box)


def test_kept_list_larger_than_the_lds_list(ecc, orc, gpu):
    """Box 3 on 346 x 260 with cap 10000: the grid and a kept list of min(cap, cells) entries pass
    64 KiB of LDS, so the pass stores its corners from inside the loop."""
    rng = np.random.default_rng(3)
    xy, flags = slices_of(ecc, [rand_pts(rng, 4096, W0, H0), rand_pts(rng, 513, W0, H0)], 4096)
    _, o_cnt = check_nms(ecc, orc, gpu, xy, flags, W0, H0, 4096, box=3, cap=10000)
    assert o_cnt[0] > 2000


def test_largest_grid(ecc, orc, gpu):
    """Box 3 on 378 x 378: 128 x 128 padded cells, the most the grid form takes; with the survivor
    lists that is more LDS than a launch gets without asking."""
    rng = np.random.default_rng(5)
    pts = rand_pts(rng, 2000, 378, 378)
    pts[:4] = [(377, 377), (0, 0), (377, 0), (0, 377)]
    xy, flags = slices_of(ecc, [pts, pts[::-1]], 2048)
    check_nms(ecc, orc, gpu, xy, flags, 378, 378, 2048, box=3)


@pytest.mark.parametrize("S", [1001, 1022])
def test_slice_length_not_a_multiple_of_four(ecc, orc, gpu, S):
    rng = np.random.default_rng(S)
    xy, flags = slices_of(ecc, [rand_pts(rng, m, W0, H0) for m in (513, S, 64)], S)
    check_nms(ecc, orc, gpu, xy[:2 * S + 333], flags[:2 * S + 333], W0, H0, S)


@pytest.fixture(scope="module")
def stream(ecc, orc):
    """One event stream and its oracle flags, shared by the fast_detect_nms cases (read only): 65536
    events, because the generator's first 16384 flag fewer corners than one chunk holds."""
    n = 16 * 4096
    xy, t, _ = ecc.gen_events(n, seed=11, width=W0, height=H0)
    return xy, t, {S: orc.fast_detect(xy, t, W0, H0, slice_events=S) for S in (4096, 1001)}


@pytest.mark.parametrize("S,box,cap", [(4096, 1, 4096), (4096, 3, 4096), (4096, 15, 4096), (4096, 31, 4096),
                                       (4096, 15, 5), (4096, 15, 0), (1001, 15, 4096)])
def test_fast_detect_nms_lists(ecc, orc, gpu, stream, S, box, cap):
    """The flag pass's candidate lists (S % 4 == 0) and the two-call path (S = 1001) into the same
    greedy pass."""
    xy, t, by_s = stream
    o_flags, o_sae = by_s[S]
    n = len(xy)
    assert max(o_flags[i: i + S].sum() for i in range(0, n, S)) > (64 if S == 4096 else 16)
    o_out, o_cnt, rc = orc.corner_nms(xy, o_flags, W0, H0, slice_events=S, box=box, cap=cap)
    ns = len(o_cnt)
    cfg = ecc.corner_cfg(width=W0, height=H0, slice_events=S)
    sae = dev(ecc, np.zeros(W0 * H0, np.int64))
    flags = ecc.DeviceArray(n, np.uint8)
    d_out, d_cnt = ecc.DeviceArray(max(ns * cap, 1), ecc.CORNER_DTYPE), ecc.DeviceArray(ns, np.int32)
    gpu.fast_detect_nms(dev(ecc, xy), dev(ecc, t), n, cfg, sae, flags, box, cap, d_out, d_cnt)
    assert gpu.fast_detect_status() == 0
    assert gpu.corner_nms_status() == (ecc.ERR_CAPACITY if rc else 0)
    assert (flags.numpy() == o_flags).all() and (sae.numpy() == o_sae).all()
    assert (d_cnt.numpy() == o_cnt).all()
    g_out = d_out.numpy()
    for s in range(ns):
        assert (g_out[s * cap: s * cap + o_cnt[s]] == o_out[s * cap: s * cap + o_cnt[s]]).all(), s


def test_one_graph_replay_equals_eager(ecc, orc, gpu):
    rng = np.random.default_rng(21)
    S, cap = 1024, 4096
    xy, flags = slices_of(ecc, [rand_pts(rng, 700, W0, H0), LATTICE, rand_pts(rng, 65, W0, H0)], S)
    o_out, o_cnt, _ = orc.corner_nms(xy, flags, W0, H0, slice_events=S, cap=cap)
    d_xy, d_flags = dev(ecc, xy), dev(ecc, flags)
    d_out, d_cnt = ecc.DeviceArray(3 * cap, ecc.CORNER_DTYPE), ecc.DeviceArray(3, np.int32)
    lib = ecc.lib

    def step():
        ecc.check(lib.ecc_memset_async(d_out.ptr, 0, d_out.nbytes, gpu.stream))
        gpu.corner_nms(d_xy, d_flags, len(xy), S, W0, H0, 15, cap, d_out, d_cnt)

    step()
    gpu.sync()
    eager = d_out.numpy().copy(), d_cnt.numpy().copy()
    assert (eager[1] == o_cnt).all()
    gp = ecc.P()
    ecc.check(lib.ecc_graph_begin(gpu.stream))
    step()
    ecc.check(lib.ecc_graph_end(gpu.stream, ecc.C.byref(gp)))
    for a in (d_out, d_cnt):
        ecc.check(lib.ecc_memset_async(a.ptr, 0xA5, a.nbytes, gpu.stream))
    ecc.check(lib.ecc_graph_launch(gp.value, gpu.stream))
    gpu.sync()
    ecc.check(lib.ecc_graph_destroy(gp.value))
    assert (d_out.numpy() == eager[0]).all() and (d_cnt.numpy() == eager[1]).all()
    for s in range(3):
        assert (eager[0][s * cap: s * cap + o_cnt[s]] == o_out[s * cap: s * cap + o_cnt[s]]).all()
