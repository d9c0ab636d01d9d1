"""Extent, over-read and address-path tests of the entry points the timed step and its neighbours use.

Every buffer an entry point sees is a guarded device view (tests/guarded.py): 16384 elements of
0xA5 in front of and behind it, inputs followed by a HOSTILE tail (values that change the result if
a kernel uses what lies past the documented extent; the oracle sees the payload only), outputs
sized exactly and pre-filled with 0xA5.  Each case runs in two placements: `aligned` (payload on a
256-B boundary, what hipMalloc returns) and `bare` (payload at exactly its element type's natural
alignment: include/ecc.h promises no more), so the arms that kernels select by address both run.

Asserted per case: (a) every guard intact and every const input byte-identical after the call,
(b) the documented part of every output bit-equal to the oracle (brute force where the parity
tests use brute force), (c) the two placements agree.  Entries the header leaves undefined (say
rep_xy between win_unique[w] and the window's end) are not compared.  n == 0 / n_segs == 0 writes
nothing but the scalars the header defines for an empty call (k-means iterations = 0, an all-zero
count image).

The cases are built once per process (functools caches), with the oracle alone; each builder
asserts that the condition it exists for holds in its data (a ragged last window, a segment count
that is no multiple of 4, a cap that is reached, a non-empty result).  test_case_conditions_hold
builds them all without a GPU.
"""
import ctypes as C
import functools

import numpy as np
import pytest

from guarded import FILL, check_all, guarded_in, guarded_inout, guarded_out

PLACEMENTS = ("aligned", "bare")
SENSOR_W, SENSOR_H = 64, 48          # 5 x 4 corner tiles
PAY_W = 48                           # payload events use x < PAY_W: the columns beyond are the hostile pixels
INT32_MAX = 2**31 - 1
gpu_test = pytest.mark.gpu


# ------------------------------------------------------------------------------------------ helpers
def _ecc():
    import eccpy
    return eccpy


def _orc():
    import orc
    return orc


def _bucket(xy):
    x, y = (xy & 0xFFFF).astype(np.int64), (xy >> 16).astype(np.int64)
    return (x * 1619 + y * 31) & 8191


def hostile_xy(payload, m, seed, x_lo=SENSOR_W, x_hi=1280, y_lo=0, y_hi=720):
    """m packed coordinates inside the downsampler's inclusive range that name pixels and hash to
    buckets the payload does not use."""
    rng = np.random.default_rng(seed)
    used_b = np.unique(_bucket(np.asarray(payload, np.uint32))) if len(payload) else np.zeros(0, np.int64)
    out = np.zeros(0, np.uint32)
    while len(out) < m:
        x = rng.integers(x_lo, x_hi + 1, 4 * m + 64).astype(np.uint32)
        y = rng.integers(y_lo, y_hi + 1, 4 * m + 64).astype(np.uint32)
        c = x | (y << 16)
        c = c[~np.isin(_bucket(c), used_b) & ~np.isin(c, payload)]
        out = np.concatenate([out, c])
    out = out[:m]
    assert not np.isin(_bucket(out), used_b).any() and not np.isin(out, payload).any()
    return out


def events(n, seed, width=SENSOR_W, height=SENSOR_H):
    xy, t, _ = _ecc().gen_events(n, seed=seed, width=width, height=height)
    return xy, t


def addr_bits(buf, mod):
    return buf.ptr % mod


def assert_placement(placement, **bufs):
    """The address bits each placement is meant to have (bufs: name -> (buffer, modulus, residue))."""
    for name, (b, mod, res) in bufs.items():
        if b is not None:
            assert b.ptr % mod == res, (placement, name, hex(b.ptr), mod, res)


def ragged_sizes(window):
    return sorted({q * window + r for q in (1, 3) for r in (0, 1, 3, window - 1)})


def same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert np.array_equal(a[k], b[k]), f"placements disagree on {k}"


SEG_STRIDES = (1024, 1027, 8192)


def seg_count_sets(stride):
    """Two count vectors of 5 segments drawn from {0, 1, 3, 4, 5, 1023, 1024, 1025, stride}."""
    return ([stride, 0, 1, 1023, 5], [3, 4, min(1025, stride), 1024, stride])


# ------------------------------------------------------------------------------------------ downsample / dedup
DS_WINDOWS = (1, 5, 2047, 2048, 2049, 8192, 8196, 16384)
DD_WINDOWS = (1, 1023, 1024, 1028, 8192)


@functools.lru_cache(maxsize=None)
def downsample_case(window, n):
    xy, _ = events(n, seed=1000 + window)
    tail = hostile_xy(xy, window + 8, seed=n)
    o_xy, o_idx, o_u, o_r = _orc().downsample_hash(xy, window=window)
    nw = len(o_u)
    assert nw == -(-n // window) and o_u.sum() > 0
    if n % window:
        assert n - (nw - 1) * window < window  # a ragged last window
    return xy, tail, (o_xy, o_idx, o_u, o_r)


@functools.lru_cache(maxsize=None)
def dedup_case(window, n):
    xy, _ = events(n, seed=2000 + window)
    tail = hostile_xy(xy, window + 8, seed=n)
    o_idx, o_cnt, o_u = _orc().dedup_exact(xy, window)
    assert o_u.sum() > 0 and (window < 1023 or (o_cnt > 1).any())  # repeats where a window can hold them
    return xy, tail, (o_idx, o_cnt, o_u)


def test_window_sizes_cover_the_quad_selection():
    """n % 4 == 0 with window % 4 == 0 selects 16-B quads by the address alone; both other arms too."""
    for windows in (DS_WINDOWS, DD_WINDOWS):
        kinds = {(w % 4 == 0, n % 4 == 0) for w in windows for n in ragged_sizes(w)}
        assert kinds == {(True, True), (True, False), (False, True), (False, False)}


def _run_downsample(ecc, gpu, window, n, placement, null=None):
    xy, tail, (o_xy, o_idx, o_u, o_r) = downsample_case(window, n)
    nw = len(o_u)
    d_xy = guarded_in(ecc, xy, placement, tail=tail)
    assert_placement(placement, xy=(d_xy, 256, 0) if placement == "aligned" else (d_xy, 16, 4))
    outs = {"rep_xy": guarded_out(ecc, np.uint32, nw * window, placement),
            "rep_idx": guarded_out(ecc, np.uint32, nw * window, placement),
            "uniq": guarded_out(ecc, np.int32, nw, placement), "rep": guarded_out(ecc, np.int32, nw, placement)}
    if null:
        outs[null] = None
    cfg = ecc.hash_cfg(window=window)
    p = {k: (None if v is None else v.ptr) for k, v in outs.items()}
    ecc.check(ecc.lib.ecc_downsample_hash(gpu.ctx, d_xy.ptr, n, C.byref(cfg), p["rep_xy"], p["rep_idx"], p["uniq"],
                                          p["rep"], gpu.stream), "ecc_downsample_hash")
    gpu.sync()
    check_all(xy=d_xy, **outs)
    got = {}
    keep = np.concatenate([np.arange(w * window, w * window + o_u[w]) for w in range(nw)])
    for name, ref in (("rep_xy", o_xy), ("rep_idx", o_idx)):
        if outs[name] is not None:
            got[name] = outs[name].numpy()[keep]
            assert np.array_equal(got[name], ref[keep]), (name, window, n, placement, null)
    for name, ref in (("uniq", o_u), ("rep", o_r)):
        if outs[name] is not None:
            got[name] = outs[name].numpy()
            assert np.array_equal(got[name], ref), (name, window, n, placement, null)
    return got


@gpu_test
@pytest.mark.parametrize("window", DS_WINDOWS)
def test_downsample_hash_extents(ecc, gpu, window):
    for n in ragged_sizes(window):
        for null in (None, "rep_xy", "rep_idx", "uniq", "rep"):
            got = [_run_downsample(ecc, gpu, window, n, pl, null) for pl in PLACEMENTS]
            same(*got)


@gpu_test
@pytest.mark.parametrize("window", DD_WINDOWS)
def test_dedup_exact_extents(ecc, gpu, window):
    for n in ragged_sizes(window):
        xy, tail, (o_idx, o_cnt, o_u) = dedup_case(window, n)
        nw = len(o_u)
        keep = np.concatenate([np.arange(w * window, w * window + o_u[w]) for w in range(nw)])
        got = []
        for pl in PLACEMENTS:
            d_xy = guarded_in(ecc, xy, pl, tail=tail)
            assert_placement(pl, xy=(d_xy, 256, 0) if pl == "aligned" else (d_xy, 16, 4))
            idx, cnt = guarded_out(ecc, np.uint32, nw * window, pl), guarded_out(ecc, np.int32, nw * window, pl)
            u = guarded_out(ecc, np.int32, nw, pl)
            ecc.check(ecc.lib.ecc_dedup_exact(gpu.ctx, d_xy.ptr, n, window, idx.ptr, cnt.ptr, u.ptr, gpu.stream))
            gpu.sync()
            check_all(xy=d_xy, uniq_idx=idx, uniq_cnt=cnt, n_unique=u)
            g = {"idx": idx.numpy()[keep], "cnt": cnt.numpy()[keep], "u": u.numpy()}
            assert np.array_equal(g["u"], o_u), (window, n, pl)
            assert np.array_equal(g["idx"], o_idx[keep]) and np.array_equal(g["cnt"], o_cnt[keep]), (window, n, pl)
            got.append(g)
        same(*got)


@gpu_test
def test_downsample_and_dedup_empty_call_writes_nothing(ecc, gpu):
    for pl in PLACEMENTS:
        d_xy = guarded_in(ecc, np.zeros(0, np.uint32), pl, tail=hostile_xy(np.zeros(0, np.uint32), 64, 1))
        outs = [guarded_out(ecc, np.uint32, 16, pl), guarded_out(ecc, np.uint32, 16, pl),
                guarded_out(ecc, np.int32, 4, pl), guarded_out(ecc, np.int32, 4, pl)]
        cfg = ecc.hash_cfg(window=8)
        ecc.check(ecc.lib.ecc_downsample_hash(gpu.ctx, d_xy.ptr, 0, C.byref(cfg), outs[0].ptr, outs[1].ptr, outs[2].ptr,
                                              outs[3].ptr, gpu.stream))
        ecc.check(ecc.lib.ecc_dedup_exact(gpu.ctx, d_xy.ptr, 0, 8, outs[1].ptr, outs[2].ptr, outs[3].ptr, gpu.stream))
        gpu.sync()
        for o in outs:
            o.check()
            assert o.untouched().all()


# ------------------------------------------------------------------------------------------ k-means, packed points
KM_KS = (1, 16, 17, 33)  # 33: the generic kernel (k > 32), whose load and store forms step 1 touched
KM_ITERS = 3


def centroids0(k, w=SENSOR_W, h=SENSOR_H):
    i = np.arange(k)
    return np.stack([(i * 37 % w) + 0.5, (i * 23 % h) + 0.25], 1).astype(np.float32).ravel() if k > 1 else \
        np.array([w / 2, h / 2], np.float32)


@functools.lru_cache(maxsize=None)
def segments_case(stride, which):
    """5 segments of packed points with hostile padding and tail: (xy, counts, dense, tail)."""
    counts = np.array(seg_count_sets(stride)[which], np.int32)
    assert (counts % 4 != 0).any() and (counts == 0).any() == (which == 0) and counts.max() == stride
    pts, _ = events(int(counts.sum()), seed=3000 + stride + which)
    # padding and tail: pixels next to the payload's (inside every threshold), which it does not use
    pad = hostile_xy(pts, 5 * stride + 64, seed=stride, x_lo=SENSOR_W, x_hi=2 * SENSOR_W - 1, y_lo=0, y_hi=2 * SENSOR_H - 1)
    xy = pad[:5 * stride].copy()
    o = 0
    for s, c in enumerate(counts):
        xy[s * stride: s * stride + c] = pts[o:o + c]
        o += c
    return xy, counts, pts, pad[5 * stride:]


@functools.lru_cache(maxsize=None)
def kmeans_xy16_ref(stride, which, k):
    _, _, dense, _ = segments_case(stride, which)
    c0 = centroids0(k)
    o_c, o_lab, o_it = _orc().kmeans_run_xy16(dense, c0, KM_ITERS)
    assert o_it == KM_ITERS and (o_lab != 255).any() and not np.array_equal(o_c, c0)
    acc = _orc().kmeans_partial_xy16(dense, c0)
    _, lab0, _ = _orc().kmeans_run_xy16(dense, c0, 0)
    assert acc[0::3].sum() > 0
    return c0, o_c, o_lab, acc, lab0


def _valid_index(stride, counts):
    return np.concatenate([np.arange(s * stride, s * stride + c) for s, c in enumerate(counts)])


def _seg_inputs(ecc, stride, which, pl):
    xy, counts, _, tail = segments_case(stride, which)
    d_xy = guarded_in(ecc, xy, pl, tail=tail)
    d_cnt = guarded_in(ecc, counts, pl, tail=np.full(64, INT32_MAX, np.int32))
    assert_placement(pl, xy=(d_xy, 256, 0) if pl == "aligned" else (d_xy, 16, 4),
                     counts=(d_cnt, 256, 0) if pl == "aligned" else (d_cnt, 16, 4))
    return d_xy, d_cnt, counts


def _cent(ecc, c, pl, inout):
    f = guarded_inout if inout else guarded_in
    return f(ecc, c, pl, tail=np.full(16, np.nan, np.float32))


@gpu_test
@pytest.mark.parametrize("k", KM_KS)
@pytest.mark.parametrize("stride", SEG_STRIDES)
@pytest.mark.parametrize("entry", ["run", "frame"])
def test_kmeans_run_xy16_extents(ecc, gpu, entry, stride, k):
    for which in (0, 1):
        c0, o_c, o_lab, _, _ = kmeans_xy16_ref(stride, which, k)
        cfg = ecc.kmeans_cfg(k=k, max_iters=KM_ITERS, tol=-1.0)
        got = []
        for pl in PLACEMENTS:
            d_xy, d_cnt, counts = _seg_inputs(ecc, stride, which, pl)
            d_c = _cent(ecc, c0, pl, True)
            d_lab = guarded_out(ecc, np.uint8, 5 * stride, pl)
            d_it = guarded_out(ecc, np.int32, 1, pl)
            assert d_lab.ptr % 2 == (0 if pl == "aligned" else 1)  # labels at even and at odd addresses
            if entry == "run":
                gpu.kmeans_xy16(d_xy, 5, stride, d_cnt, d_c, cfg, d_lab, d_it)
            else:
                gpu.kmeans_xy16_frame(d_xy, 5, stride, d_cnt, SENSOR_W, SENSOR_H, d_c, cfg, d_lab, d_it)
            gpu.sync()
            check_all(xy=d_xy, seg_counts=d_cnt, centroids=d_c, labels=d_lab, iters=d_it)
            g = {"c": d_c.numpy().view(np.uint32), "lab": d_lab.numpy()[_valid_index(stride, counts)], "it": d_it.numpy()}
            assert np.array_equal(g["c"], o_c.view(np.uint32)), (entry, stride, which, k, pl)
            assert np.array_equal(g["lab"], o_lab) and g["it"][0] == KM_ITERS, (entry, stride, which, k, pl)
            got.append(g)
        same(*got)


@gpu_test
@pytest.mark.parametrize("k", KM_KS)
@pytest.mark.parametrize("stride", SEG_STRIDES)
def test_kmeans_split_entries_xy16_extents(ecc, gpu, stride, k):
    """ecc_kmeans_labels_xy16, ecc_kmeans_accumulate_xy16 and ecc_kmeans_counts_xy16."""
    L = ecc.lib
    FW, FH = 2 * SENSOR_W, 2 * SENSOR_H  # the hostile pixels lie inside this frame: their counts must stay 0
    for which in (0, 1):
        c0, _, _, o_acc, o_lab0 = kmeans_xy16_ref(stride, which, k)
        _, counts, dense, _ = segments_case(stride, which)
        o_img = np.bincount((dense >> 16).astype(np.int64) * FW + (dense & 0xFFFF), minlength=FW * FH).astype(np.uint32)
        got = []
        for pl in PLACEMENTS:
            d_xy, d_cnt, _ = _seg_inputs(ecc, stride, which, pl)
            d_c = _cent(ecc, c0, pl, False)
            d_lab = guarded_out(ecc, np.uint8, 5 * stride, pl)
            ecc.check(L.ecc_kmeans_labels_xy16(gpu.ctx, d_xy.ptr, 5, stride, d_cnt.ptr, d_c.ptr, k, 50.0, d_lab.ptr, gpu.stream))
            d_acc = guarded_inout(ecc, np.zeros(3 * k, np.uint64), pl)
            d_st = guarded_in(ecc, np.zeros(2, np.int32), pl, tail=np.ones(8, np.int32))  # tail: "done"
            ecc.check(L.ecc_kmeans_accumulate_xy16(gpu.ctx, d_xy.ptr, 5, stride, d_cnt.ptr, d_c.ptr, k, 50.0, d_acc.ptr,
                                                   d_st.ptr, gpu.stream))
            d_img = guarded_out(ecc, np.uint32, FW * FH, pl)
            ecc.check(L.ecc_kmeans_counts_xy16(gpu.ctx, d_xy.ptr, 5, stride, d_cnt.ptr, FW, FH, d_img.ptr, gpu.stream))
            assert L.ecc_kmeans_counts_status(gpu.ctx, gpu.stream) == 0
            gpu.sync()
            check_all(xy=d_xy, seg_counts=d_cnt, centroids=d_c, labels=d_lab, acc=d_acc, state=d_st, counts=d_img)
            g = {"lab": d_lab.numpy()[_valid_index(stride, counts)], "acc": d_acc.numpy().astype(np.int64),
                 "img": d_img.numpy()}
            assert np.array_equal(g["lab"], o_lab0), (stride, which, k, pl)
            assert np.array_equal(g["acc"], o_acc), (stride, which, k, pl)
            assert np.array_equal(g["img"], o_img), (stride, which, k, pl)
            got.append(g)
        same(*got)


@functools.lru_cache(maxsize=None)
def count_image_case(w, h, k):
    rng = np.random.default_rng(w * 100 + h)
    img = rng.integers(0, 6, w * h).astype(np.uint32)
    img[0] = max(img[0], 1)
    q = np.repeat(np.arange(w * h), img)
    pts = ((q % w) | ((q // w) << 16)).astype(np.uint32)
    c0 = centroids0(k, max(w, 2), max(h, 2))
    o_c, _, o_it = _orc().kmeans_run_xy16(pts, c0, KM_ITERS)
    assert o_it == KM_ITERS and len(pts) > 0
    return img, c0, o_c


@gpu_test
@pytest.mark.parametrize("k", (1, 16, 17))
@pytest.mark.parametrize("frame", [(1, 1), (5, 3), (64, 48)])
def test_kmeans_run_counts_extents(ecc, gpu, frame, k):
    w, h = frame
    img, c0, o_c = count_image_case(w, h, k)
    cfg = ecc.kmeans_cfg(k=k, max_iters=KM_ITERS, tol=-1.0)
    got = []
    for pl in PLACEMENTS:
        d_img = guarded_in(ecc, img, pl, tail=np.full(256, 7, np.uint32))
        d_c = _cent(ecc, c0, pl, True)
        d_it = guarded_out(ecc, np.int32, 1, pl)
        ecc.check(ecc.lib.ecc_kmeans_run_counts(gpu.ctx, d_img.ptr, w, h, C.byref(cfg), d_c.ptr, d_it.ptr, gpu.stream))
        gpu.sync()
        check_all(counts=d_img, centroids=d_c, iters=d_it)
        g = {"c": d_c.numpy().view(np.uint32), "it": d_it.numpy()}
        assert np.array_equal(g["c"], o_c.view(np.uint32)) and g["it"][0] == KM_ITERS, (frame, k, pl)
        got.append(g)
    same(*got)


@gpu_test
def test_kmeans_xy16_no_segments_writes_nothing(ecc, gpu):
    """n_segs == 0: centroids unchanged, labels untouched; the header's scalars of an empty call are the
    iteration count 0 and an all-zero count image."""
    L = ecc.lib
    for pl in PLACEMENTS:
        c0 = centroids0(16)
        d_xy = guarded_in(ecc, np.zeros(0, np.uint32), pl, tail=hostile_xy(np.zeros(0, np.uint32), 64, 2))
        d_cnt = guarded_in(ecc, np.zeros(0, np.int32), pl, tail=np.full(64, INT32_MAX, np.int32))
        d_c, d_lab, d_it = _cent(ecc, c0, pl, True), guarded_out(ecc, np.uint8, 64, pl), guarded_out(ecc, np.int32, 1, pl)
        cfg = ecc.kmeans_cfg(k=16, max_iters=KM_ITERS, tol=-1.0)
        gpu.kmeans_xy16(d_xy, 0, 1024, d_cnt, d_c, cfg, d_lab, d_it)
        gpu.kmeans_xy16_frame(d_xy, 0, 1024, d_cnt, SENSOR_W, SENSOR_H, d_c, cfg, d_lab, None)
        ecc.check(L.ecc_kmeans_labels_xy16(gpu.ctx, d_xy.ptr, 0, 1024, d_cnt.ptr, d_c.ptr, 16, 50.0, d_lab.ptr, gpu.stream))
        d_acc = guarded_inout(ecc, np.zeros(48, np.uint64), pl)
        d_st = guarded_in(ecc, np.zeros(2, np.int32), pl)
        ecc.check(L.ecc_kmeans_accumulate_xy16(gpu.ctx, d_xy.ptr, 0, 1024, d_cnt.ptr, d_c.ptr, 16, 50.0, d_acc.ptr,
                                               d_st.ptr, gpu.stream))
        d_img = guarded_out(ecc, np.uint32, 15, pl)
        ecc.check(L.ecc_kmeans_counts_xy16(gpu.ctx, d_xy.ptr, 0, 1024, d_cnt.ptr, 5, 3, d_img.ptr, gpu.stream))
        gpu.sync()
        check_all(xy=d_xy, seg_counts=d_cnt, centroids=d_c, labels=d_lab, iters=d_it, acc=d_acc, state=d_st, counts=d_img)
        assert np.array_equal(d_c.numpy().view(np.uint32), c0.view(np.uint32)) and d_lab.untouched().all()
        assert d_it.numpy()[0] == 0 and not d_acc.numpy().any() and not d_img.numpy().any()


# ------------------------------------------------------------------------------------------ k-means, float points
F32_NS = (1, 2, 3, 127, 128, 129, 4097)
F32_KS = (1, 16, 17, 32)
# (xy byte offset from a 256-B boundary, labels: offset or None); 0: hipMalloc's own alignment
F32_LAYOUTS = ((0, 0), (16, 1), (16, 2), (8, 1), (8, 2), (16, None), (8, None))


@functools.lru_cache(maxsize=None)
def f32_case(n, k, iters):
    rng = np.random.default_rng(n * 64 + k)
    pts = rng.integers(0, SENSOR_W, (n, 2)).astype(np.float32)
    pts[:, 1] = rng.integers(0, SENSOR_H, n)
    c0 = centroids0(k)
    o_c, o_lab, o_it = _orc().kmeans_run_f32(pts.ravel(), c0, iters)
    assert o_it == iters and (o_lab != 255).any()
    # hostile tail: copies of payload points (they would add weight to their clusters)
    tail = np.tile(pts[:1], (64, 1)).ravel()
    return pts.ravel(), tail, c0, o_c, o_lab


def _f32_layout(ecc, pts, tail, n, layout):
    xy_skew, lab_skew = layout
    d_xy = guarded_in(ecc, pts, "bare" if xy_skew else "aligned", tail=tail, skew=xy_skew)
    assert d_xy.ptr % 16 == xy_skew % 16 and d_xy.ptr % 256 == xy_skew
    d_lab = None if lab_skew is None else guarded_out(ecc, np.uint8, n, "bare" if lab_skew else "aligned", skew=lab_skew)
    assert d_lab is None or d_lab.ptr % 2 == lab_skew % 2
    return d_xy, d_lab


@gpu_test
@pytest.mark.parametrize("k", F32_KS)
@pytest.mark.parametrize("engine", [None, 1, 2, 3])
def test_kmeans_run_f32_extents(ecc, gpu, engine, k):
    """ecc_kmeans_run_f32 (engine None) and ecc_kmeans_run_f32_engine 1-3: xy at 0 and at 8 mod 16 take
    different kernels (pair / fast; engine 3 falls back to engine 2; the candidate table on / off)."""
    for n in F32_NS:
        for iters in (0, 3):
            pts, tail, c0, o_c, o_lab = f32_case(n, k, iters)
            cfg = ecc.kmeans_cfg(k=k, max_iters=iters, tol=-1.0)
            got, labs = [], []
            for layout in F32_LAYOUTS:
                d_xy, d_lab = _f32_layout(ecc, pts, tail, n, layout)
                pl = "bare" if layout[0] else "aligned"
                d_c, d_it = _cent(ecc, c0, pl, True), guarded_out(ecc, np.int32, 1, pl)
                if engine is None:
                    gpu.kmeans_f32(d_xy, n, d_c, cfg, d_lab, d_it)
                else:
                    gpu.kmeans_f32_engine(d_xy, n, d_c, cfg, engine, d_lab, d_it)
                gpu.sync()
                check_all(xy=d_xy, centroids=d_c, labels=d_lab, iters=d_it)
                g = {"c": d_c.numpy().view(np.uint32), "it": d_it.numpy()}
                assert np.array_equal(g["c"], o_c.view(np.uint32)) and g["it"][0] == iters, (engine, k, n, iters, layout)
                if d_lab is not None:
                    labs.append(d_lab.numpy())
                    assert np.array_equal(labs[-1], o_lab), (engine, k, n, iters, layout)
                got.append(g)
            for g in got[1:]:
                same(got[0], g)
            for lab in labs[1:]:
                assert np.array_equal(labs[0], lab), "layouts disagree on labels"


@gpu_test
@pytest.mark.parametrize("k", F32_KS)
def test_kmeans_assign_f32_extents(ecc, gpu, k):
    for n in F32_NS:
        pts, tail, c0, _, _ = f32_case(n, k, 0)
        o_lab = _orc().kmeans_assign_f32(pts, c0)
        got = []
        for layout in F32_LAYOUTS:
            if layout[1] is None:
                continue
            d_xy, d_lab = _f32_layout(ecc, pts, tail, n, layout)
            d_c = _cent(ecc, c0, "bare" if layout[0] else "aligned", False)
            gpu.kmeans_assign_f32(d_xy, n, d_c, k, 50.0, d_lab)
            gpu.sync()
            check_all(xy=d_xy, centroids=d_c, labels=d_lab)
            got.append({"lab": d_lab.numpy()})
            assert np.array_equal(got[-1]["lab"], o_lab), (k, n, layout)
        for g in got[1:]:
            same(got[0], g)


_RC_C0 = np.array([1, 1, 10, 10, 20, 20, 30, 30, 50, 50, 60, 60, 70, 70, 80, 80], np.float32)


@functools.lru_cache(maxsize=None)
def refcompat_case(n):
    pts = (np.random.default_rng(1000 + n).random(2 * n) * 90).astype(np.float32)
    o_c, o_cnt, o_ss = _RC_C0.copy(), np.zeros(8, np.int32), np.zeros(32, np.float32)
    o_p = _orc().lib.orc_kmeans_refcompat(pts.ctypes.data, n, o_c.ctypes.data, 50, o_cnt.ctypes.data, o_ss.ctypes.data)
    assert 1 <= o_p <= 50 and o_cnt.sum() > 0
    return pts, o_p, o_c, o_cnt, o_ss


@gpu_test
@pytest.mark.parametrize("n", [1, 2047, 2049, 16384])
def test_kmeans_refcompat_extents(ecc, gpu, n):
    pts, o_p, o_c, o_cnt, o_ss = refcompat_case(n)
    got = []
    for pl in PLACEMENTS:
        d_xy = guarded_in(ecc, pts, pl, tail=np.tile(pts[:2], 64))
        d_c = guarded_inout(ecc, _RC_C0, pl, tail=np.full(16, np.nan, np.float32))
        d_p, d_cnt, d_ss = guarded_out(ecc, np.int32, 1, pl), guarded_out(ecc, np.int32, 8, pl), guarded_out(ecc, np.float32, 32, pl)
        assert_placement(pl, xy=(d_xy, 256, 0) if pl == "aligned" else (d_xy, 16, 4))
        ecc.check(ecc.lib.ecc_kmeans_refcompat_f32(gpu.ctx, d_xy.ptr, n, d_c.ptr, 50, d_p.ptr, d_cnt.ptr, d_ss.ptr, gpu.stream))
        gpu.sync()
        check_all(xy=d_xy, centroids=d_c, passes=d_p, bin_counts=d_cnt, partial_sums=d_ss)
        g = {"p": d_p.numpy(), "c": d_c.numpy().view(np.uint32), "cnt": d_cnt.numpy(), "ss": d_ss.numpy().view(np.uint32)}
        assert g["p"][0] == o_p and np.array_equal(g["c"], o_c.view(np.uint32)), (n, pl)
        assert np.array_equal(g["cnt"], o_cnt) and np.array_equal(g["ss"], o_ss.view(np.uint32)), (n, pl)
        got.append(g)
    same(*got)


@gpu_test
def test_kmeans_f32_no_points_writes_nothing(ecc, gpu):
    for layout in ((0, 0), (8, 1)):
        c0 = centroids0(16)
        d_xy, d_lab = _f32_layout(ecc, np.zeros(0, np.float32), np.full(128, 3.0, np.float32), 0, layout)
        d_lab64 = guarded_out(ecc, np.uint8, 64, "bare" if layout[1] else "aligned")
        pl = "bare" if layout[0] else "aligned"
        d_c = _cent(ecc, c0, pl, True)
        cfg = ecc.kmeans_cfg(k=16, max_iters=3, tol=-1.0)
        d_it = guarded_out(ecc, np.int32, 1, pl)
        for eng in (1, 2, 3):
            gpu.kmeans_f32_engine(d_xy, 0, d_c, cfg, eng, d_lab64, None)
        gpu.kmeans_f32(d_xy, 0, d_c, cfg, d_lab64, d_it)
        gpu.kmeans_assign_f32(d_xy, 0, d_c, 16, 50.0, d_lab64)
        gpu.sync()
        check_all(xy=d_xy, centroids=d_c, labels=d_lab64, iters=d_it)
        assert np.array_equal(d_c.numpy().view(np.uint32), c0.view(np.uint32)) and d_lab64.untouched().all()
        assert d_it.numpy()[0] == 0  # the one scalar an empty k-means defines


@gpu_test
def test_kmeans_refcompat_no_points_runs_the_reference_loop(ecc, gpu):
    """n == 0 is defined in full (include/ecc.h): the reference's loop over no points writes every output, as
    the oracle's does; nothing outside them."""
    pts = np.zeros(0, np.float32)
    o_c, o_cnt, o_ss = _RC_C0.copy(), np.zeros(8, np.int32), np.zeros(32, np.float32)
    o_p = _orc().lib.orc_kmeans_refcompat(None, 0, o_c.ctypes.data, 50, o_cnt.ctypes.data, o_ss.ctypes.data)
    assert o_p >= 1 and not o_cnt.any()
    for pl in PLACEMENTS:
        d_xy = guarded_in(ecc, pts, pl, tail=np.full(128, 3.0, np.float32))
        d_c = guarded_inout(ecc, _RC_C0, pl, tail=np.full(16, np.nan, np.float32))
        d_p, d_cnt, d_ss = guarded_out(ecc, np.int32, 1, pl), guarded_out(ecc, np.int32, 8, pl), guarded_out(ecc, np.float32, 32, pl)
        ecc.check(ecc.lib.ecc_kmeans_refcompat_f32(gpu.ctx, d_xy.ptr, 0, d_c.ptr, 50, d_p.ptr, d_cnt.ptr, d_ss.ptr, gpu.stream))
        gpu.sync()
        check_all(xy=d_xy, centroids=d_c, passes=d_p, bin_counts=d_cnt, partial_sums=d_ss)
        assert d_p.numpy()[0] == o_p and np.array_equal(d_c.numpy().view(np.uint32), o_c.view(np.uint32)), pl
        assert np.array_equal(d_cnt.numpy(), o_cnt) and np.array_equal(d_ss.numpy().view(np.uint32), o_ss.view(np.uint32)), pl


# ------------------------------------------------------------------------------------------ SAE, corners, NMS
SLICE_EVENTS = (5, 1000, 1001)
N_SLICES = 33  # two groups of 32
CORNER_MODES = ((0, 1), (1, 0), (0, 0), (1, 1))  # (border_mode, first_detect_slice)


def moving_squares(n, side=5, period=6, pitch=12):
    """Nine squares stepping diagonally (and jumping back every `period` steps): the events of their two
    leading edges, whose common vertex passes the arc test, so that a 1000-event slice holds dozens of
    corners several NMS boxes apart (the synthetic generator's streams give a handful)."""
    origins = [(x, y) for y in range(5, SENSOR_H - side - period - 4, pitch)
               for x in range(5, PAY_W - side - period - 4, pitch)]
    ev, step = [], 0
    while len(ev) < n:
        k = step % period
        for ox, oy in origins:
            x0, y0 = ox + k, oy + k
            ev += [(x0 + side, y0 + j) for j in range(side + 1)] + [(x0 + j, y0 + side) for j in range(side)]
        step += 1
    ev = np.array(ev[:n])
    return (ev[:, 0] | (ev[:, 1] << 16)).astype(np.uint32), (np.arange(n) * 3 + 1).astype(np.int64)


@functools.lru_cache(maxsize=None)
def corner_stream(S, r):
    n = N_SLICES * S + r
    xy, t = moving_squares(n)
    assert ((xy & 0xFFFF) < PAY_W).all() and ((xy >> 16) < SENSOR_H).all()
    # hostile tails: in-sensor pixels of the columns the payload never uses; times below t[n-1]
    # (ECC_ERR_UNSORTED_TIME if read) and far above it
    rng = np.random.default_rng(S + r)
    m = S + 16
    tail_xy = (rng.integers(PAY_W, SENSOR_W, m) | (rng.integers(0, SENSOR_H, m) << 16)).astype(np.uint32)
    tail_t = np.where(np.arange(m) % 2 == 0, t[-1] - 1000 - np.arange(m), t[-1] + 10**12).astype(np.int64)
    if r:
        assert n % S == r  # the last slice is partial
    if S == 1001:
        assert sum((s * S) % 4 != 0 for s in range(N_SLICES)) >= N_SLICES // 2  # slices off a 4-event boundary
    return xy, t, tail_xy, tail_t


@functools.lru_cache(maxsize=None)
def corner_ref(S, r, border_mode, first_detect):
    xy, t, _, _ = corner_stream(S, r)
    flags, sae = _orc().fast_detect(xy, t, SENSOR_W, SENSOR_H, slice_events=S, border_mode=border_mode,
                                    first_detect=first_detect)
    if S >= 1000:
        assert flags.sum() > 0, (S, r, border_mode, first_detect)  # the oracle finds corners
    assert (sae.reshape(SENSOR_H, SENSOR_W)[:, PAY_W:] == 0).all() and sae.max() > 0
    return flags, sae


NMS_BOX = 5


@functools.lru_cache(maxsize=None)
def nms_ref(S, r, cap, border_mode=0, first_detect=1):
    xy = corner_stream(S, r)[0]
    flags, _ = corner_ref(S, r, border_mode, first_detect)
    out, cnt, rc = _orc().corner_nms(xy, flags, SENSOR_W, SENSOR_H, slice_events=S, box=NMS_BOX, cap=cap)
    full = _orc().corner_nms(xy, flags, SENSOR_W, SENSOR_H, slice_events=S, box=NMS_BOX, cap=4096)[1]
    return out, cnt, full


def _kept(cnt, cap):
    return np.concatenate([np.arange(s * cap, s * cap + c) for s, c in enumerate(cnt)]) if len(cnt) else np.zeros(0, np.int64)


def _corner_inputs(ecc, S, r, pl):
    xy, t, tail_xy, tail_t = corner_stream(S, r)
    d_xy, d_t = guarded_in(ecc, xy, pl, tail=tail_xy), guarded_in(ecc, t, pl, tail=tail_t)
    assert_placement(pl, xy=(d_xy, 256, 0) if pl == "aligned" else (d_xy, 16, 4),
                     t=(d_t, 256, 0) if pl == "aligned" else (d_t, 16, 8))
    return d_xy, d_t, len(xy)


@gpu_test
@pytest.mark.parametrize("S", SLICE_EVENTS)
@pytest.mark.parametrize("entry", ["detect", "prepare_finish", "detect_nms", "prepare_finish_nms"])
def test_fast_detect_extents(ecc, gpu, entry, S):
    L = ecc.lib
    cap = 7
    for r in (0, 1, 3):
        for border_mode, first_detect in CORNER_MODES:
            o_flags, o_sae = corner_ref(S, r, border_mode, first_detect)
            o_out, o_cnt, _ = nms_ref(S, r, cap, border_mode, first_detect)
            cfg = ecc.corner_cfg(width=SENSOR_W, height=SENSOR_H, slice_events=S, border_mode=border_mode,
                                 first_detect_slice=first_detect)
            got = []
            for pl in PLACEMENTS:
                d_xy, d_t, n = _corner_inputs(ecc, S, r, pl)
                ns = -(-n // S)
                d_sae = guarded_inout(ecc, np.zeros(SENSOR_W * SENSOR_H, np.int64), pl)
                d_flags = guarded_out(ecc, np.uint8, n, pl)
                assert d_flags.ptr % 4 == (0 if pl == "aligned" else 1)
                d_local = guarded_out(ecc, np.int64, SENSOR_W * SENSOR_H, pl) if entry.startswith("prepare") else None
                nms = entry.endswith("nms")
                d_out = guarded_out(ecc, ecc.CORNER_DTYPE, ns * cap, pl) if nms else None
                d_cnt = guarded_out(ecc, np.int32, ns, pl) if nms else None
                args = (gpu.ctx, d_xy.ptr, d_t.ptr, n, C.byref(cfg))
                if d_local is not None:
                    ecc.check(L.ecc_fast_detect_prepare(*args, d_local.ptr, gpu.stream), "prepare")
                if entry == "detect":
                    ecc.check(L.ecc_fast_detect(*args, d_sae.ptr, d_flags.ptr, gpu.stream), entry)
                elif entry == "prepare_finish":
                    ecc.check(L.ecc_fast_detect_finish(*args, d_sae.ptr, d_flags.ptr, gpu.stream), entry)
                elif entry == "detect_nms":
                    ecc.check(L.ecc_fast_detect_nms(*args, d_sae.ptr, d_flags.ptr, NMS_BOX, cap, d_out.ptr, d_cnt.ptr,
                                                    gpu.stream), entry)
                else:
                    ecc.check(L.ecc_fast_detect_finish_nms(*args, d_sae.ptr, d_flags.ptr, NMS_BOX, cap, d_out.ptr,
                                                           d_cnt.ptr, gpu.stream), entry)
                assert gpu.fast_detect_status() == 0, "hostile timestamps were read"
                gpu.sync()
                check_all(xy=d_xy, t=d_t, sae=d_sae, flags=d_flags, local_last=d_local, out=d_out, counts=d_cnt)
                g = {"flags": d_flags.numpy(), "sae": d_sae.numpy()}
                key = (entry, S, r, border_mode, first_detect, pl)
                assert np.array_equal(g["flags"], o_flags), key
                assert np.array_equal(g["sae"], o_sae), key
                if d_local is not None:
                    g["local"] = d_local.numpy()
                    assert np.array_equal(g["local"], o_sae), key  # from an all-zero SAE the final SAE is the batch's last t
                if nms:
                    g["cnt"] = d_cnt.numpy()
                    g["out"] = d_out.numpy()[_kept(o_cnt, cap)]
                    assert np.array_equal(g["cnt"], o_cnt) and np.array_equal(g["out"], o_out[_kept(o_cnt, cap)]), key
                got.append(g)
            same(*got)


@gpu_test
@pytest.mark.parametrize("cap", [1, 7, 4096])
@pytest.mark.parametrize("S", SLICE_EVENTS)
def test_corner_nms_extents(ecc, gpu, S, cap):
    for r in (0, 1, 3):
        xy, _, tail_xy, _ = corner_stream(S, r)
        o_flags, _ = corner_ref(S, r, 0, 1)
        o_out, o_cnt, full = nms_ref(S, r, cap)
        n, ns = len(xy), len(o_cnt)
        if S >= 1000:
            assert o_cnt.sum() > 0
            if cap < 4096:
                assert (full > cap).any() and (o_cnt == cap).any()  # the clamp to cap is exercised
            else:
                assert (full < cap).all()
        got = []
        for pl in PLACEMENTS:
            d_xy = guarded_in(ecc, xy, pl, tail=tail_xy)
            d_flags = guarded_in(ecc, o_flags, pl, tail=np.ones(S + 16, np.uint8))
            assert d_flags.ptr % 4 == (0 if pl == "aligned" else 1)
            d_out, d_cnt = guarded_out(ecc, ecc.CORNER_DTYPE, ns * cap, pl), guarded_out(ecc, np.int32, ns, pl)
            assert_placement(pl, out=(d_out, 256, 0) if pl == "aligned" else (d_out, 16, 4))
            gpu.corner_nms(d_xy, d_flags, n, S, SENSOR_W, SENSOR_H, NMS_BOX, cap, d_out, d_cnt)
            st = gpu.corner_nms_status()
            assert st == (ecc.ERR_CAPACITY if (full > cap).any() else 0), (S, r, cap, pl, st)
            check_all(xy=d_xy, flags=d_flags, out=d_out, counts=d_cnt)
            g = {"cnt": d_cnt.numpy(), "out": d_out.numpy()[_kept(o_cnt, cap)]}
            assert np.array_equal(g["cnt"], o_cnt) and np.array_equal(g["out"], o_out[_kept(o_cnt, cap)]), (S, r, cap, pl)
            got.append(g)
        same(*got)


@functools.lru_cache(maxsize=None)
def wide_nms_case():
    """A sensor whose 1-pixel NMS grid exceeds the LDS: the one-kernel form reads the flags itself,
    in chunks of 4096 events (two chunks per slice here, the last slice partial)."""
    W = H = 130
    S, n = 4100, 3 * 4100 + 3
    xy, _ = events(n, seed=77, width=W, height=H)
    rng = np.random.default_rng(5)
    flags = (rng.random(n) < 0.3).astype(np.uint8)
    tail_xy = (rng.integers(0, W, S) | (rng.integers(0, H, S) << 16)).astype(np.uint32)
    out, cnt, rc = _orc().corner_nms(xy, flags, W, H, slice_events=S, box=1, cap=4096)
    assert (W + 2) * (H + 2) > 16384 and cnt.sum() > 0 and (cnt < 4096).all() and n % S
    return W, H, S, xy, flags, tail_xy, out, cnt


@gpu_test
def test_corner_nms_one_kernel_form_extents(ecc, gpu):
    W, H, S, xy, flags, tail_xy, o_out, o_cnt = wide_nms_case()
    n, ns, cap = len(xy), len(o_cnt), 4096
    got = []
    for pl in PLACEMENTS:
        d_xy = guarded_in(ecc, xy, pl, tail=tail_xy)
        d_flags = guarded_in(ecc, flags, pl, tail=np.ones(S, np.uint8))
        assert d_flags.ptr % 16 == (0 if pl == "aligned" else 1)
        d_out, d_cnt = guarded_out(ecc, ecc.CORNER_DTYPE, ns * cap, pl), guarded_out(ecc, np.int32, ns, pl)
        gpu.corner_nms(d_xy, d_flags, n, S, W, H, 1, cap, d_out, d_cnt)
        assert gpu.corner_nms_status() == 0
        check_all(xy=d_xy, flags=d_flags, out=d_out, counts=d_cnt)
        g = {"cnt": d_cnt.numpy(), "out": d_out.numpy()[_kept(o_cnt, cap)]}
        assert np.array_equal(g["cnt"], o_cnt) and np.array_equal(g["out"], o_out[_kept(o_cnt, cap)]), pl
        got.append(g)
    same(*got)


@functools.lru_cache(maxsize=None)
def sae_case():
    W, H, n = 7, 9, 1001  # W * H odd
    xy, t = events(n, seed=9, width=W - 2, height=H)
    rng = np.random.default_rng(3)
    tail_xy = (rng.integers(W - 2, W, 64) | (rng.integers(0, H, 64) << 16)).astype(np.uint32)  # unused in-image pixels
    tail_t = np.full(64, t[-1] + 10**12, np.int64)
    sae0 = rng.integers(0, int(t[n // 2]), W * H).astype(np.int64)
    ref = sae0.copy()
    np.maximum.at(ref, (xy >> 16).astype(np.int64) * W + (xy & 0xFFFF), t)
    assert (ref != sae0).any() and (ref == sae0).any()
    images = rng.integers(0, 10**9, 3 * W * H).astype(np.int64)
    return W, H, xy, t, tail_xy, tail_t, sae0, ref, images


@gpu_test
def test_sae_scatter_and_max_combine_extents(ecc, gpu):
    W, H, xy, t, tail_xy, tail_t, sae0, ref, images = sae_case()
    hw = W * H
    got = []
    for pl in PLACEMENTS:
        d_xy, d_t = guarded_in(ecc, xy, pl, tail=tail_xy), guarded_in(ecc, t, pl, tail=tail_t)
        d_sae = guarded_inout(ecc, sae0, pl)
        assert_placement(pl, sae=(d_sae, 256, 0) if pl == "aligned" else (d_sae, 16, 8))
        gpu.sae_scatter(d_xy, d_t, len(xy), W, H, d_sae)
        d_img = guarded_in(ecc, images, pl, tail=np.full(2 * hw, 2**62, np.int64))
        d_out = guarded_out(ecc, np.int64, hw, pl)
        ecc.check(ecc.lib.ecc_sae_max_combine(gpu.ctx, d_img.ptr, 3, hw, d_out.ptr, gpu.stream))
        # n == 0 / no images to combine but the first: nothing past the extent either
        d_none = guarded_inout(ecc, sae0, pl)
        gpu.sae_scatter(d_xy, d_t, 0, W, H, d_none)
        gpu.sync()
        check_all(xy=d_xy, t=d_t, sae=d_sae, images=d_img, out=d_out, sae_empty=d_none)
        g = {"sae": d_sae.numpy(), "max": d_out.numpy()}
        assert np.array_equal(g["sae"], ref) and np.array_equal(g["max"], images.reshape(3, hw).max(0)), pl
        assert np.array_equal(d_none.numpy(), sae0)
        got.append(g)
    same(*got)


@gpu_test
def test_corner_entries_empty_call_writes_nothing(ecc, gpu):
    L = ecc.lib
    for pl in PLACEMENTS:
        xy, t, tail_xy, tail_t = corner_stream(5, 0)
        d_xy = guarded_in(ecc, np.zeros(0, np.uint32), pl, tail=tail_xy)
        d_t = guarded_in(ecc, np.zeros(0, np.int64), pl, tail=tail_t)
        d_fin = guarded_in(ecc, np.zeros(0, np.uint8), pl, tail=np.ones(64, np.uint8))
        sae0 = np.arange(SENSOR_W * SENSOR_H, dtype=np.int64)
        d_sae, d_flags = guarded_inout(ecc, sae0, pl), guarded_out(ecc, np.uint8, 64, pl)
        d_out, d_cnt = guarded_out(ecc, ecc.CORNER_DTYPE, 64, pl), guarded_out(ecc, np.int32, 8, pl)
        d_pk, d_off = guarded_out(ecc, ecc.CORNER_DTYPE, 64, pl), guarded_out(ecc, np.int64, 1, pl)
        cfg = ecc.corner_cfg(width=SENSOR_W, height=SENSOR_H, slice_events=5)
        ecc.check(L.ecc_fast_detect(gpu.ctx, d_xy.ptr, d_t.ptr, 0, C.byref(cfg), d_sae.ptr, d_flags.ptr, gpu.stream))
        ecc.check(L.ecc_fast_detect_nms(gpu.ctx, d_xy.ptr, d_t.ptr, 0, C.byref(cfg), d_sae.ptr, d_flags.ptr, NMS_BOX, 8,
                                        d_out.ptr, d_cnt.ptr, gpu.stream))
        assert gpu.fast_detect_status() == 0
        # the two-call forms: an empty batch's own last-t image is all zero, the finish halves write nothing
        d_local = guarded_out(ecc, np.int64, SENSOR_W * SENSOR_H, pl)
        ecc.check(L.ecc_fast_detect_prepare(gpu.ctx, d_xy.ptr, d_t.ptr, 0, C.byref(cfg), d_local.ptr, gpu.stream))
        ecc.check(L.ecc_fast_detect_finish(gpu.ctx, d_xy.ptr, d_t.ptr, 0, C.byref(cfg), d_sae.ptr, d_flags.ptr, gpu.stream))
        ecc.check(L.ecc_fast_detect_prepare(gpu.ctx, d_xy.ptr, d_t.ptr, 0, C.byref(cfg), d_local.ptr, gpu.stream))
        ecc.check(L.ecc_fast_detect_finish_nms(gpu.ctx, d_xy.ptr, d_t.ptr, 0, C.byref(cfg), d_sae.ptr, d_flags.ptr, NMS_BOX,
                                               8, d_out.ptr, d_cnt.ptr, gpu.stream))
        assert gpu.fast_detect_status() == 0
        gpu.corner_nms(d_xy, d_fin, 0, 5, SENSOR_W, SENSOR_H, NMS_BOX, 8, d_out, d_cnt)
        # no images to combine: the first shard's initial SAE, all zero; no pixels: nothing
        d_img = guarded_in(ecc, np.zeros(0, np.int64), pl, tail=np.full(64, 2**62, np.int64))
        d_max, d_max0 = guarded_out(ecc, np.int64, 63, pl), guarded_out(ecc, np.int64, 63, pl)
        ecc.check(L.ecc_sae_max_combine(gpu.ctx, d_img.ptr, 0, 63, d_max.ptr, gpu.stream))
        ecc.check(L.ecc_sae_max_combine(gpu.ctx, d_img.ptr, 3, 0, d_max0.ptr, gpu.stream))
        gpu.sync()
        check_all(xy=d_xy, t=d_t, flags_in=d_fin, sae=d_sae, flags=d_flags, out=d_out, counts=d_cnt, local_last=d_local,
                  images=d_img, combined=d_max, combined_no_pixels=d_max0)
        assert np.array_equal(d_sae.numpy(), sae0) and not d_local.numpy().any() and not d_max.numpy().any()
        for o in (d_flags, d_out, d_cnt, d_max0):
            assert o.untouched().all()
        # no slices to pack: offsets[0] = 0 is the whole documented output
        gpu.corner_pack(d_out, d_cnt, 0, 8, d_pk, d_off)
        gpu.sync()
        check_all(packed=d_pk, offsets=d_off)
        assert d_pk.untouched().all() and int(d_off.numpy()[0]) == 0


# ------------------------------------------------------------------------------------------ pack, tracker
def _plausible_corners(m, seed):
    rng = np.random.default_rng(seed)
    c = np.zeros(m, np.dtype([("x", np.int32), ("y", np.int32), ("label", np.int32)]))
    c["x"], c["y"], c["label"] = rng.integers(4, SENSOR_W - 4, m), rng.integers(4, SENSOR_H - 4, m), np.arange(m)
    return c


@functools.lru_cache(maxsize=None)
def pack_case(ns):
    cap = 40
    o_out, o_cnt, _ = nms_ref(1000, 3, cap, 0, 0)
    o_out, o_cnt = o_out[:ns * cap].copy(), o_cnt[:ns].copy()
    hostile = _plausible_corners(ns * cap + 64, ns)
    strided = hostile[:ns * cap].copy()
    for s in range(ns):
        strided[s * cap: s * cap + o_cnt[s]] = o_out[s * cap: s * cap + o_cnt[s]]
    assert o_cnt.sum() > 0 and (o_cnt < cap).any()  # some slice has room for hostile corners past its count
    return cap, strided, o_cnt, hostile[ns * cap:]


@gpu_test
@pytest.mark.parametrize("ns", [1, 33])
def test_corner_pack_extents(ecc, gpu, ns):
    cap, strided, o_cnt, tail = pack_case(ns)
    total = int(o_cnt.sum())
    want = np.concatenate([strided[s * cap: s * cap + o_cnt[s]] for s in range(ns)])
    got = []
    for pl in PLACEMENTS:
        d_in = guarded_in(ecc, strided, pl, tail=tail)
        d_cnt = guarded_in(ecc, o_cnt, pl, tail=np.full(64, INT32_MAX, np.int32))
        d_out, d_off = guarded_out(ecc, ecc.CORNER_DTYPE, total, pl), guarded_out(ecc, np.int64, ns + 1, pl)
        assert_placement(pl, corners=(d_in, 256, 0) if pl == "aligned" else (d_in, 16, 4),
                         offsets=(d_off, 256, 0) if pl == "aligned" else (d_off, 16, 8))
        gpu.corner_pack(d_in, d_cnt, ns, cap, d_out, d_off)
        gpu.sync()
        check_all(corners=d_in, counts=d_cnt, out=d_out, offsets=d_off)
        g = {"out": d_out.numpy(), "off": d_off.numpy()}
        assert np.array_equal(g["out"], want), pl
        assert np.array_equal(g["off"], np.concatenate([[0], np.cumsum(o_cnt)])), pl
        got.append(g)
    same(*got)


def _track_key(tr):
    return (tr.x, tr.y, tr.label, tr.frame_count, tr.is_matched, tr.frames_since_last_detection, tr.hist_len,
            tuple(tr.hist_x[:tr.hist_len]), tuple(tr.hist_y[:tr.hist_len]), np.float32(tr.vx).view(np.uint32),
            np.float32(tr.vy).view(np.uint32), np.float32(tr.dir_cur_x).view(np.uint32),
            np.float32(tr.dir_cur_y).view(np.uint32), tr.group_id)


def _group_key(g):
    return (g.id, g.n_labels, g.first_label_offset) + tuple(np.float32(getattr(g, f)).view(np.uint32)
                                                            for f in ("avg_vx", "avg_vy", "cx", "cy", "radius"))


@functools.lru_cache(maxsize=None)
def tracker_case():
    """12 slices of drifting detections, cap-strided with plausible corners past every count."""
    rng = np.random.default_rng(11)
    ns, cap = 12, 16
    centres = rng.uniform([40, 40], [300, 220], (6, 2))
    hostile = _plausible_corners(ns * cap + 64, 4)
    hostile["x"] += 100  # a hostile corner would start a track of its own
    strided, cnt = hostile[:ns * cap].copy(), np.zeros(ns, np.int32)
    for s in range(ns):
        m = int(rng.integers(3, 7))
        sel = rng.choice(6, m, replace=False)
        p = np.rint(centres[sel] + rng.normal(0, 1.0, (m, 2))).astype(np.int32)
        strided["x"][s * cap: s * cap + m], strided["y"][s * cap: s * cap + m] = p[:, 0], p[:, 1]
        strided["label"][s * cap: s * cap + m] = np.arange(m)
        cnt[s] = m
        centres += 2.0
    orc, ecc = _orc(), _ecc()
    otr = orc.OracleTracker(ecc.tracker_cfg())
    for s in range(ns):
        otr.update(strided[s * cap: s * cap + cnt[s]])
    tracks = [_track_key(t) for t in otr.tracks(ecc.Track)]
    og, ol = otr.groups(ecc.Group)
    groups = [_group_key(g) for g in og]
    labels = ol[:sum(g.n_labels for g in og)].copy()
    assert len(tracks) > 0 and len(groups) > 0 and (cnt < cap).all()
    return ns, cap, strided, cnt, hostile[ns * cap:], tracks, groups, labels


@gpu_test
@pytest.mark.parametrize("entry", ["update", "update_lists"])
def test_tracker_inputs_extents(ecc, gpu, entry):
    ns, cap, strided, cnt, tail, tracks, groups, labels = tracker_case()
    for pl in PLACEMENTS:
        d_c = guarded_in(ecc, strided, pl, tail=tail)
        d_n = guarded_in(ecc, cnt, pl, tail=np.full(64, INT32_MAX, np.int32))
        starts = (np.arange(ns) * cap).astype(np.int64)
        d_s = guarded_in(ecc, starts, pl, tail=np.arange(64, dtype=np.int64))
        assert_placement(pl, corners=(d_c, 256, 0) if pl == "aligned" else (d_c, 16, 4),
                         starts=(d_s, 256, 0) if pl == "aligned" else (d_s, 16, 8))
        tr = ecc.Tracker(gpu)
        if entry == "update":
            tr.update(d_c, d_n, 5, cap)  # two launches: state carries over; interior pointers for the second
            ecc.check(ecc.lib.ecc_tracker_update(tr.tr, d_c.ptr + 5 * cap * 12, d_n.ptr + 5 * 4, ns - 5, cap, gpu.stream))
        else:
            tr.update_lists(d_c, d_s, d_n, ns)
        gpu.sync()
        assert tr.status() == 0
        check_all(corners=d_c, counts=d_n, starts=d_s)
        assert [_track_key(t) for t in tr.tracks()] == tracks, (entry, pl)
        gg, gl = tr.groups()
        assert [_group_key(g) for g in gg] == groups and np.array_equal(gl[:len(labels)], labels), (entry, pl)
        tr0 = ecc.Tracker(gpu)  # no slices: no tracks
        tr0.update(d_c, d_n, 0, cap)
        tr0.update_lists(d_c, d_s, d_n, 0)
        assert tr0.status() == 0 and tr0.tracks() == []
        check_all(corners=d_c, counts=d_n, starts=d_s)
        tr.close()
        tr0.close()


# ------------------------------------------------------------------------------------------ eps lists, DBSCAN over windows
EPS_STRIDES = (1027, 4096)
EPS, EPS_MIN_PTS = 2.5, 4


@functools.lru_cache(maxsize=None)
def eps_case(stride, which):
    xy, counts, _, tail = segments_case(stride, which)
    orc = _orc()
    o_cnt, o_core, o_off, o_nbr = orc.eps_neighbours(xy, 5, stride, counts, EPS, EPS_MIN_PTS)
    valid = _valid_index(stride, counts)
    total = int(o_off[-1])
    assert total == o_cnt[valid].sum() > 0 and (o_core[valid] >= 0).any() and (o_core[valid] < 0).any()
    clusters = []
    for s, c in enumerate(counts):
        p = xy[s * stride: s * stride + c]
        clusters.append(orc.dbscan_lists(np.stack([p & 0xFFFF, p >> 16], 1), EPS, EPS_MIN_PTS, 2, 1 << 30))
    n_dups = sum(sum(len(m) for m in cl) - len(np.unique(np.concatenate(cl))) for cl in clusters if cl)
    assert any(len(cl) > 1 for cl in clusters)
    return xy, counts, tail, valid, (o_cnt, o_core, o_off, o_nbr[:total]), clusters, n_dups


def _collect_clusters(stride, counts, lab, nc, dups):
    out = []
    for s, m in enumerate(counts):
        members = [[] for _ in range(nc[s])]
        for j in np.nonzero(lab[s * stride: s * stride + m] >= 0)[0]:
            members[lab[s * stride + j]].append(int(j))
        for p, c in dups[(dups[:, 0] >= s * stride) & (dups[:, 0] < s * stride + m)]:
            members[c].append(int(p - s * stride))
        out.append([np.array(sorted(c), np.int32) for c in members])
    return out


def _same_clusters(got, ref):
    assert len(got) == len(ref)
    for a, b in zip(got, ref):
        assert len(a) == len(b)
        for x, y in zip(a, b):
            assert np.array_equal(x, y)


@gpu_test
@pytest.mark.parametrize("which", (0, 1))
@pytest.mark.parametrize("stride", EPS_STRIDES)
def test_eps_and_window_dbscan_extents(ecc, gpu, stride, which):
    """ecc_eps_counts, ecc_eps_lists (nbr sized exactly offsets[n]), ecc_dbscan_extract and ecc_dbscan_grid
    (dups sized exactly)."""
    xy, counts, tail, valid, (o_cnt, o_core, o_off, o_nbr), clusters, n_dups = eps_case(stride, which)
    n, total = 5 * stride, len(o_nbr)
    got = []
    for pl in PLACEMENTS:
        d_xy = guarded_in(ecc, xy, pl, tail=tail)
        d_sc = guarded_in(ecc, counts, pl, tail=np.full(64, INT32_MAX, np.int32))
        d_cnt, d_core = guarded_out(ecc, np.int32, n, pl), guarded_out(ecc, np.float64, n, pl)
        gpu.eps_counts(d_xy, 5, stride, d_sc, EPS, EPS_MIN_PTS, d_cnt, d_core)
        gpu.sync()
        check_all(xy=d_xy, seg_counts=d_sc, counts=d_cnt, core=d_core)
        g = {"cnt": d_cnt.numpy()[valid], "core": d_core.numpy()[valid].view(np.int64)}
        assert np.array_equal(g["cnt"], o_cnt[valid]) and np.array_equal(g["core"], o_core[valid].view(np.int64)), pl
        # entries past a segment's count: count 0 and core distance -1 (the scan of ecc_eps_lists runs over them)
        rest = np.ones(n, bool)
        rest[valid] = False
        assert not d_cnt.numpy()[rest].any() and (d_core.numpy()[rest] == -1.0).all(), pl
        # lists from the oracle's counts (0 in the padding, as documented), hostile past the array
        cnt_in = np.zeros(n, np.int32)
        cnt_in[valid] = o_cnt[valid]
        d_cin = guarded_in(ecc, cnt_in, pl, tail=np.full(64, 5, np.int32))
        d_off, d_nbr = guarded_out(ecc, np.int64, n + 1, pl), guarded_out(ecc, np.int32, total, pl)
        gpu.eps_lists(d_xy, 5, stride, d_sc, EPS, d_cin, d_off, d_nbr, total)
        gpu.sync()
        check_all(xy=d_xy, seg_counts=d_sc, counts_in=d_cin, offsets=d_off, nbr=d_nbr)
        g["off"], g["nbr"] = d_off.numpy(), d_nbr.numpy()
        assert np.array_equal(g["off"], o_off) and np.array_equal(g["nbr"], o_nbr), pl
        # extraction over guarded lists (hostile tail: valid indices) and straight from the points
        d_off_in = guarded_in(ecc, o_off, pl, tail=np.full(64, total, np.int64))
        d_nbr_in = guarded_in(ecc, o_nbr, pl, tail=np.zeros(4096, np.int32))
        for fused in (False, True):
            d_lab, d_nc = guarded_out(ecc, np.int32, n, pl), guarded_out(ecc, np.int32, 5, pl)
            d_dups, d_nd = guarded_out(ecc, np.int64, 2 * n_dups, pl), guarded_out(ecc, np.int64, 1, pl)
            if fused:
                gpu.dbscan_grid(d_xy, 5, stride, d_sc, EPS, EPS_MIN_PTS, 2, 1 << 30, d_lab, d_nc, d_dups, n_dups, d_nd)
            else:
                ecc.check(ecc.lib.ecc_dbscan_extract(gpu.ctx, 5, stride, d_sc.ptr, d_off_in.ptr, d_nbr_in.ptr, total,
                                                     EPS_MIN_PTS, 2, 1 << 30, d_lab.ptr, d_nc.ptr, d_dups.ptr, n_dups,
                                                     d_nd.ptr, gpu.stream))
            assert gpu.dbscan_status() == 0, gpu.last_error()
            check_all(xy=d_xy, seg_counts=d_sc, offsets=d_off_in, nbr=d_nbr_in, labels=d_lab, n_clusters=d_nc, dups=d_dups,
                      n_dups=d_nd)
            assert int(d_nd.numpy()[0]) == n_dups
            cl = _collect_clusters(stride, counts, d_lab.numpy(), d_nc.numpy(), d_dups.numpy().reshape(-1, 2))
            _same_clusters(cl, clusters)
            g["lab%d" % fused] = d_lab.numpy()[valid]
        got.append(g)
    same(*got)


@gpu_test
def test_eps_and_window_dbscan_no_segments_writes_nothing(ecc, gpu):
    for pl in PLACEMENTS:
        d_xy = guarded_in(ecc, np.zeros(0, np.uint32), pl, tail=hostile_xy(np.zeros(0, np.uint32), 64, 3))
        d_sc = guarded_in(ecc, np.zeros(0, np.int32), pl, tail=np.full(64, INT32_MAX, np.int32))
        outs = [guarded_out(ecc, np.int32, 64, pl), guarded_out(ecc, np.float64, 64, pl), guarded_out(ecc, np.int32, 64, pl),
                guarded_out(ecc, np.int32, 8, pl), guarded_out(ecc, np.int64, 16, pl)]
        d_cnt, d_core, d_lab, d_nc, d_dups = outs
        gpu.eps_counts(d_xy, 0, 1027, d_sc, EPS, EPS_MIN_PTS, d_cnt, d_core)
        d_nd = guarded_out(ecc, np.int64, 1, pl)
        gpu.dbscan_grid(d_xy, 0, 1027, d_sc, EPS, EPS_MIN_PTS, 2, 1 << 30, d_lab, d_nc, d_dups, 8, d_nd)
        assert gpu.dbscan_status() == 0
        # lists and extraction over no segments: offsets[0] = 0 and *n_dups = 0 are all they define
        d_cin = guarded_in(ecc, np.zeros(0, np.int32), pl, tail=np.full(64, 5, np.int32))
        d_off, d_nbr = guarded_out(ecc, np.int64, 1, pl), guarded_out(ecc, np.int32, 64, pl)
        gpu.eps_lists(d_xy, 0, 1027, d_sc, EPS, d_cin, d_off, d_nbr, 64)
        d_off_in = guarded_in(ecc, np.zeros(1, np.int64), pl, tail=np.full(64, 7, np.int64))
        d_nbr_in = guarded_in(ecc, np.zeros(0, np.int32), pl, tail=np.zeros(64, np.int32))
        d_nd2 = guarded_out(ecc, np.int64, 1, pl)
        ecc.check(ecc.lib.ecc_dbscan_extract(gpu.ctx, 0, 1027, d_sc.ptr, d_off_in.ptr, d_nbr_in.ptr, 0, EPS_MIN_PTS, 2,
                                             1 << 30, d_lab.ptr, d_nc.ptr, d_dups.ptr, 8, d_nd2.ptr, gpu.stream))
        assert gpu.dbscan_status() == 0
        check_all(xy=d_xy, seg_counts=d_sc, n_dups=d_nd, counts_in=d_cin, offsets=d_off, nbr=d_nbr, offsets_in=d_off_in,
                  nbr_in=d_nbr_in, n_dups_extract=d_nd2)
        for o in outs + [d_nbr]:
            o.check()
            assert o.untouched().all()
        assert int(d_nd.numpy()[0]) == 0 and int(d_nd2.numpy()[0]) == 0 and int(d_off.numpy()[0]) == 0


# ------------------------------------------------------------------------------------------ clouds
CLOUD_NS = (1, 255, 257, 1025)


@functools.lru_cache(maxsize=None)
def cloud_case(n, dim, dtype):
    rng = np.random.default_rng(n * 8 + dim)
    # a few neighbours per ball: core and non-core points both occur
    side = n // 4 + 2 if dim == 1 else int(np.ceil((2 * n) ** (1.0 / dim))) + 1
    pts = (rng.integers(0, side, (n, dim)) + rng.integers(0, 4, (n, dim)) * 0.25).astype(dtype)
    eps, min_pts = (1.5, 3) if dim > 1 else (0.3, 3)
    p64 = pts.astype(np.float64)
    d2 = np.zeros((n, n))
    for d in range(dim):
        if dtype == np.float32:
            dd = (pts[:, None, d] - pts[None, :, d]).astype(np.float64)  # float difference, widened
        else:
            dd = p64[:, None, d] - p64[None, :, d]
        d2 = d2 + dd * dd
    ball = d2 <= eps * eps
    cnt = ball.sum(1).astype(np.int32)
    core = np.array([np.sqrt(np.sort(d2[i][ball[i]])[min_pts - 1]) if cnt[i] >= min_pts else -1.0 for i in range(n)])
    off = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
    nbr = np.concatenate([np.nonzero(b)[0] for b in ball]).astype(np.int32)  # ascending rows
    rows = np.repeat(np.arange(n), cnt)
    nd = np.sqrt(d2[rows, nbr])
    _, clusters = _orc().dbscan_cloud(pts, eps, min_pts, 1, 1 << 30)
    n_dups = sum(len(c) for c in clusters) - (len(np.unique(np.concatenate(clusters))) if clusters else 0)
    if n > 1:
        assert (cnt > 1).any() and (core >= 0).any() and (core < 0).any() and len(clusters) > 0
    tail = np.tile(pts[:1], (64, 1)).ravel()  # copies of a payload point: neighbours that must not count
    return pts.ravel(), tail, eps, min_pts, cnt, core, off, nbr, nd, clusters, n_dups


@gpu_test
@pytest.mark.parametrize("dim", (1, 2, 3))
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_radius_and_cloud_dbscan_extents(ecc, gpu, dtype, dim):
    """ecc_radius_counts / _lists (f32, f64), ecc_lists_sort_ascending on those lists and ecc_dbscan_cloud,
    with list and duplicate outputs sized exactly, against brute force and the oracle's DBSCAN."""
    f32 = dtype == np.float32
    for n in CLOUD_NS:
        pts, tail, eps, min_pts, o_cnt, o_core, o_off, o_nbr, o_nd, clusters, n_dups = cloud_case(n, dim, dtype)
        total = len(o_nbr)
        got = []
        for pl in PLACEMENTS:
            d_p = guarded_in(ecc, pts, pl, tail=tail)
            assert_placement(pl, pts=(d_p, 256, 0) if pl == "aligned" else (d_p, 16, 4 if f32 else 8))
            d_cnt, d_core = guarded_out(ecc, np.int32, n, pl), guarded_out(ecc, np.float64, n, pl)
            (gpu.radius_counts_f32 if f32 else gpu.radius_counts_f64)(d_p, n, dim, eps, min_pts, d_cnt, d_core)
            gpu.sync()
            check_all(pts=d_p, counts=d_cnt, core=d_core)
            g = {"cnt": d_cnt.numpy(), "core": d_core.numpy().view(np.int64)}
            assert np.array_equal(g["cnt"], o_cnt) and np.array_equal(g["core"], o_core.view(np.int64)), (n, dim, pl)
            d_cin = guarded_in(ecc, o_cnt, pl, tail=np.full(64, 9, np.int32))
            d_off = guarded_out(ecc, np.int64, n + 1, pl)
            d_nbr, d_nd = guarded_out(ecc, np.int32, total, pl), guarded_out(ecc, np.float64, total, pl)
            lists = gpu.radius_lists_f32 if f32 else gpu.radius_lists_f64
            lists(d_p, n, dim, eps, d_cin, d_off, d_nbr, total, d_nd)
            assert gpu.radius_status() == 0
            check_all(pts=d_p, counts=d_cin, offsets=d_off, nbr=d_nbr, nbr_dist=d_nd)
            assert np.array_equal(d_off.numpy(), o_off), (n, dim, pl)
            d_off_in = guarded_in(ecc, o_off, pl, tail=np.full(64, total, np.int64))
            gpu.lists_sort_ascending(n, d_off_in, total, d_nbr, d_nd)
            gpu.sync()
            check_all(offsets=d_off_in, nbr=d_nbr, nbr_dist=d_nd)
            g["nbr"], g["nd"] = d_nbr.numpy(), d_nd.numpy().view(np.int64)
            assert np.array_equal(g["nbr"], o_nbr) and np.array_equal(g["nd"], o_nd.view(np.int64)), (n, dim, pl)
            d_lab, d_nc = guarded_out(ecc, np.int32, n, pl), guarded_out(ecc, np.int32, 1, pl)
            d_dups, d_ndp = guarded_out(ecc, np.int64, 2 * n_dups, pl), guarded_out(ecc, np.int64, 1, pl)
            gpu.dbscan_cloud(d_p, n, dim, eps, min_pts, 1, 1 << 30, d_lab, d_nc, d_dups, n_dups, d_ndp)
            assert gpu.dbscan_cloud_status() == 0, gpu.last_error()
            check_all(pts=d_p, labels=d_lab, n_clusters=d_nc, dups=d_dups, n_dups=d_ndp)
            lab, nc = d_lab.numpy(), int(d_nc.numpy()[0])
            assert int(d_ndp.numpy()[0]) == n_dups and nc == len(clusters), (n, dim, pl)
            members = [[] for _ in range(nc)]
            for i in np.nonzero(lab >= 0)[0]:
                members[lab[i]].append(int(i))
            for p, c in d_dups.numpy().reshape(-1, 2):
                members[c].append(int(p))
            for a, b in zip(members, clusters):
                assert np.array_equal(np.array(sorted(a), np.int32), b), (n, dim, pl)
            g["lab"] = lab
            got.append(g)
        same(*got)


@gpu_test
def test_cloud_entries_no_points_write_nothing(ecc, gpu):
    for pl in PLACEMENTS:
        for dtype in (np.float32, np.float64):
            f32 = dtype == np.float32
            d_p = guarded_in(ecc, np.zeros(0, dtype), pl, tail=np.ones(96, dtype))
            d_cnt, d_core, d_lab = guarded_out(ecc, np.int32, 16, pl), guarded_out(ecc, np.float64, 16, pl), guarded_out(ecc, np.int32, 16, pl)
            d_dups = guarded_out(ecc, np.int64, 16, pl)
            d_nc, d_nd = guarded_out(ecc, np.int32, 1, pl), guarded_out(ecc, np.int64, 1, pl)
            (gpu.radius_counts_f32 if f32 else gpu.radius_counts_f64)(d_p, 0, 3, 1.0, 2, d_cnt, d_core)
            gpu.dbscan_cloud(d_p, 0, 3, 1.0, 2, 1, 10, d_lab, d_nc, d_dups, 8, d_nd)
            assert gpu.dbscan_cloud_status() == 0
            # lists of no points: offsets[0] = 0 alone, as a size query and with list buffers; nothing to sort
            d_cin = guarded_in(ecc, np.zeros(0, np.int32), pl, tail=np.full(64, 9, np.int32))
            d_off, d_off2 = guarded_out(ecc, np.int64, 1, pl), guarded_out(ecc, np.int64, 1, pl)
            d_nbr, d_nbd = guarded_out(ecc, np.int32, 16, pl), guarded_out(ecc, np.float64, 16, pl)
            lists = gpu.radius_lists_f32 if f32 else gpu.radius_lists_f64
            lists(d_p, 0, 3, 1.0, d_cin, d_off, None, 0)
            lists(d_p, 0, 3, 1.0, d_cin, d_off2, d_nbr, 16, d_nbd)
            assert gpu.radius_status() == 0
            d_off_in = guarded_in(ecc, np.zeros(1, np.int64), pl, tail=np.full(64, 16, np.int64))
            gpu.lists_sort_ascending(0, d_off_in, 0, d_nbr, d_nbd)
            gpu.sync()
            check_all(pts=d_p, n_clusters=d_nc, n_dups=d_nd, counts_in=d_cin, offsets=d_off, offsets2=d_off2,
                      offsets_in=d_off_in)
            for o in (d_cnt, d_core, d_lab, d_dups, d_nbr, d_nbd):
                o.check()
                assert o.untouched().all()
            # the scalars of an empty cloud: no clusters, no duplicates, an empty scan
            assert int(d_nc.numpy()[0]) == 0 and int(d_nd.numpy()[0]) == 0
            assert int(d_off.numpy()[0]) == 0 and int(d_off2.numpy()[0]) == 0


# ------------------------------------------------------------------------------------------ the helper itself
@gpu_test
def test_guarded_view_reports_damage_on_both_sides(ecc, gpu):
    """A byte written at ptr - 1 and at ptr + nbytes (both inside the helper's own allocation) is named."""
    for pl in PLACEMENTS:
        for dtype, n in ((np.uint8, 37), (np.uint32, 5), (np.int64, 3), (ecc.CORNER_DTYPE, 2)):
            b = guarded_out(ecc, dtype, n, pl)
            assert b.damage() is None
            ecc.check(ecc.lib.ecc_memset_async(b.ptr - 1, 0, 1, gpu.stream))
            gpu.sync()
            assert b.damage() == -1
            with pytest.raises(AssertionError, match="offset -1 "):
                b.check("probe")
            b = guarded_out(ecc, dtype, n, pl)
            ecc.check(ecc.lib.ecc_memset_async(b.ptr + b.nbytes, 0, 1, gpu.stream))
            gpu.sync()
            assert b.damage() == b.nbytes
            with pytest.raises(AssertionError, match=f"offset {b.nbytes} "):
                b.check("probe")
        # a const input that gets written is caught by comparison, payload and tail alike
        src = np.arange(9, dtype=np.uint32)
        for at in (8, 36 + 4):
            b = guarded_in(ecc, src, pl, tail=np.arange(4, dtype=np.uint32))
            ecc.check(ecc.lib.ecc_memset_async(b.ptr + at, 0xFF, 1, gpu.stream))
            gpu.sync()
            assert b.damage() == at
        assert (FILL, b.ptr % 16) == (0xA5, 0 if pl == "aligned" else 4)


# ------------------------------------------------------------------------------------------ CPU precheck
def test_case_conditions_hold():
    """Builds every case with the oracle alone (no GPU): each builder asserts the condition it exists for."""
    for w in DS_WINDOWS:
        for n in ragged_sizes(w):
            downsample_case(w, n)
    for w in DD_WINDOWS:
        for n in ragged_sizes(w):
            dedup_case(w, n)
    for stride in SEG_STRIDES:
        for which in (0, 1):
            for k in KM_KS:
                kmeans_xy16_ref(stride, which, k)
    for frame in ((1, 1), (5, 3), (64, 48)):
        for k in (1, 16, 17):
            count_image_case(*frame, k)
    for n in F32_NS:
        for k in F32_KS:
            f32_case(n, k, 0), f32_case(n, k, 3)
    for n in (1, 2047, 2049, 16384):
        refcompat_case(n)
    for S in SLICE_EVENTS:
        for r in (0, 1, 3):
            for bm, fd in CORNER_MODES:
                corner_ref(S, r, bm, fd)
                nms_ref(S, r, 7, bm, fd)
            for cap in (1, 7, 4096):
                _, o_cnt, full = nms_ref(S, r, cap)
                if S >= 1000 and cap < 4096:
                    assert (full > cap).any() and (o_cnt == cap).any()
    wide_nms_case(), sae_case(), pack_case(1), pack_case(33), tracker_case()
    for stride in EPS_STRIDES:
        for which in (0, 1):
            eps_case(stride, which)
    for n in CLOUD_NS:
        for dim in (1, 2, 3):
            cloud_case(n, dim, np.float32), cloud_case(n, dim, np.float64)
