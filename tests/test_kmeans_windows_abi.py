"""CPU tests of the ecc_kmeans_windows_xy16 boundary and of ecc_kmeans_windows_flow_host: the
library exports and binds both, every invalid argument is rejected on the host before a device is
touched (the pointers here are not addresses of anything), also for an empty call, and the flow
rule on a hand case."""
import ctypes as C

import numpy as np
import pytest

CTX, XY, CNT, INIT, CENT, LAB, SIZES, ITERS = 0x1000, 0x2000, 0x3000, 0x4000, 0x5000, 0x6000, 0x7000, 0x8000


class _NoCfg:
    """Stands for a NULL cfg pointer; its repr is part of a test id, so it must not hold an address."""

    def __repr__(self):
        return "NULL"


NO_CFG = _NoCfg()


def call(ecc, ctx=CTX, xy=XY, n_segs=2, stride=64, counts=CNT, k=16, max_iters=5, cfg=None, init=INIT, cent=CENT,
         labels=LAB, sizes=SIZES, iters=ITERS):
    c = None if cfg is NO_CFG else C.byref(ecc.kmeans_cfg(k=k, max_iters=max_iters))
    return ecc.lib.ecc_kmeans_windows_xy16(ctx, xy, n_segs, stride, counts, c, init, cent, labels, sizes, iters, None)


def test_library_exports_and_binds_kmeans_windows(ecc):
    assert hasattr(ecc.lib, "ecc_kmeans_windows_xy16") and hasattr(ecc.lib, "ecc_kmeans_windows_flow_host")
    assert hasattr(ecc.Context, "kmeans_windows") and hasattr(ecc, "kmeans_windows_flow")
    assert ecc.KMEANS_WINDOWS_MAX_GRID >= 1


BAD = [dict(ctx=None), dict(cfg=NO_CFG), dict(cent=None), dict(k=0), dict(k=65), dict(max_iters=-1),
       dict(stride=0), dict(stride=-5), dict(stride=16385)]


@pytest.mark.parametrize("n_segs", [2, 0])
@pytest.mark.parametrize("bad", BAD + [dict(n_segs=-1)], ids=lambda d: ",".join(f"{k}={v}" for k, v in d.items()))
def test_kmeans_windows_rejects_bad_arguments(ecc, bad, n_segs):
    assert call(ecc, **{"n_segs": n_segs, **bad}) == ecc.ERR_INVALID


def test_kmeans_windows_needs_points_for_segments(ecc):
    assert call(ecc, xy=None) == ecc.ERR_INVALID
    assert call(ecc, xy=None, n_segs=0) == ecc.OK


def test_kmeans_windows_no_segments_is_ok(ecc):
    assert call(ecc, n_segs=0) == ecc.OK
    # only the data pointers may be NULL
    assert call(ecc, n_segs=0, xy=None, counts=None, init=None, labels=None, sizes=None, iters=None) == ecc.OK
    # the limits themselves are valid
    assert call(ecc, n_segs=0, k=64, stride=16384, max_iters=0) == ecc.OK
    assert call(ecc, n_segs=0, k=1, stride=1) == ecc.OK


# ------------------------------------------------------------------------------ the flow rule
def flow_raw(ecc, cent, sizes, n, k, diff, has_prev):
    p = lambda a: None if a is None else a.ctypes.data
    return ecc.lib.ecc_kmeans_windows_flow_host(p(cent), p(sizes), n, k, p(diff), p(has_prev))


def test_flow_hand_case(ecc):
    """3 windows x 3 centres; centre 1 is empty in the middle window, centre 2 in the first."""
    cent = np.array([[[10, 20], [30, 40], [50, 60]],
                     [[11.5, 18], [30, 40], [55.25, 61]],
                     [[13, 18.5], [33, 44], [54, 70]]], np.float32)
    sizes = np.array([[5, 2, 0], [4, 0, 7], [1, 9, 3]], np.int32)
    diff, has_prev = ecc.kmeans_windows_flow(cent, sizes, 3)
    assert has_prev.tolist() == [[0, 0, 0], [1, 0, 0], [1, 0, 1]]
    want = np.zeros((3, 3, 2), np.float32)
    want[1, 0] = (1.5, -2.0)
    want[2, 0] = (1.5, 0.5)
    want[2, 2] = (-1.25, 9.0)
    assert np.array_equal(diff.view(np.uint32), want.view(np.uint32))
    # the raw call writes every entry, zeros included
    d, h = np.full(18, np.nan, np.float32), np.full(9, 0xA5, np.uint8)
    assert flow_raw(ecc, cent, sizes, 3, 3, d, h) == ecc.OK
    assert np.array_equal(d.view(np.uint32), want.ravel().view(np.uint32)) and h.tolist() == has_prev.ravel().tolist()


def test_flow_is_a_float_subtraction(ecc):
    cent = np.array([[[0.1, 1e8]], [[0.3, 1e8 + 8]]], np.float32)
    diff, has_prev = ecc.kmeans_windows_flow(cent, np.array([[1], [1]], np.int32), 1)
    assert has_prev.tolist() == [[0], [1]]
    assert np.array_equal(diff[1, 0].view(np.uint32), (cent[1, 0] - cent[0, 0]).view(np.uint32))


def test_flow_rejects_bad_arguments(ecc):
    cent, sizes = np.zeros(12, np.float32), np.ones(6, np.int32)
    d, h = np.zeros(12, np.float32), np.zeros(6, np.uint8)
    assert flow_raw(ecc, cent, sizes, 2, 3, d, h) == ecc.OK
    for args in ((None, sizes, 2, 3, d, h), (cent, None, 2, 3, d, h), (cent, sizes, 2, 3, None, h),
                 (cent, sizes, 2, 3, d, None), (cent, sizes, 2, 0, d, h), (cent, sizes, 2, -1, d, h),
                 (cent, sizes, -1, 3, d, h)):
        assert flow_raw(ecc, *args) == ecc.ERR_INVALID, args[2:4]


def test_flow_no_windows_is_ok(ecc):
    d, h = np.full(4, 7, np.float32), np.full(2, 0xA5, np.uint8)
    assert flow_raw(ecc, np.zeros(4, np.float32), np.zeros(2, np.int32), 0, 2, d, h) == ecc.OK
    assert (d == 7).all() and (h == 0xA5).all()  # nothing written
    diff, has_prev = ecc.kmeans_windows_flow(np.zeros((0, 2, 2), np.float32), np.zeros((0, 2), np.int32), 2)
    assert diff.shape == (0, 2, 2) and has_prev.shape == (0, 2)
