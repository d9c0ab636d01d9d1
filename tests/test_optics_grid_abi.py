"""CPU tests of the ecc_optics_grid boundary: the library exports the entry and its status call,
and every invalid argument is rejected on the host, before a device is touched (the pointers
here are not addresses of anything)."""
import math

import pytest

CTX, XY, CNT, ORDER, REACH, CLUSTER, NCL = 0x1000, 0x2000, 0x3000, 0x4000, 0x5000, 0x6000, 0x7000


def call(ecc, ctx=CTX, xy=XY, n_segs=2, stride=64, counts=CNT, eps=10.0, min_pts=2, thr=10.0, order=ORDER,
         reach=REACH, cluster=CLUSTER, n_clusters=NCL):
    return ecc.lib.ecc_optics_grid(ctx, xy, n_segs, stride, counts, eps, min_pts, thr, order, reach, cluster,
                                   n_clusters, None)


def test_library_exports_optics_grid(ecc):
    assert hasattr(ecc.lib, "ecc_optics_grid")
    assert hasattr(ecc.lib, "ecc_optics_grid_status")
    assert hasattr(ecc.Context, "optics_grid") and hasattr(ecc.Context, "optics_grid_status")


@pytest.mark.parametrize("bad", [
    dict(ctx=None), dict(xy=None), dict(order=None), dict(reach=None),
    dict(stride=0), dict(stride=-5), dict(stride=8193),
    dict(eps=0.0), dict(eps=-1.0), dict(eps=32767.5), dict(eps=math.inf), dict(eps=-math.inf), dict(eps=math.nan),
    dict(min_pts=0), dict(min_pts=-3), dict(min_pts=65),
    dict(cluster=None), dict(n_clusters=None),
    dict(n_segs=-1),
], ids=lambda d: ",".join(f"{k}={v}" for k, v in d.items()))
def test_optics_grid_rejects_bad_arguments(ecc, bad):
    assert call(ecc, **bad) == ecc.ERR_INVALID


def test_optics_grid_rejects_bad_arguments_with_no_segments(ecc):
    """The argument ranges hold for an empty call too (only the data pointers may then be NULL)."""
    for bad in (dict(ctx=None), dict(stride=0), dict(stride=8193), dict(eps=0.0), dict(eps=math.nan),
                dict(min_pts=0), dict(min_pts=65), dict(cluster=None), dict(n_clusters=None)):
        assert call(ecc, n_segs=0, **bad) == ecc.ERR_INVALID, bad


def test_optics_grid_no_segments_is_ok(ecc):
    assert call(ecc, n_segs=0) == ecc.OK
    assert call(ecc, n_segs=0, xy=None, counts=None, order=None, reach=None, cluster=None, n_clusters=None) == ecc.OK
    # the limits themselves are valid
    assert call(ecc, n_segs=0, stride=8192, eps=32767.0, min_pts=64) == ecc.OK
    assert call(ecc, n_segs=0, stride=1, eps=0.5, min_pts=1) == ecc.OK


def test_optics_grid_status_needs_a_context(ecc):
    assert ecc.lib.ecc_optics_grid_status(None, None) == ecc.ERR_INVALID
