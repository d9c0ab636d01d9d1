"""The arc kernels' rare exits (csrc/corner_arc.hip) on streams built to take them
(tests/arc_path_cases.py; tests/test_arc_path_cases.py shows on the CPU that they do): the
circle-3 survivor queue overflowing in arc_kernel and in arc_dense_kernel, value runs of up to 32
per pixel in light windows (the second trip of overflow_lines), surface values above the group's
last timestamp up to INT64_MAX and down to INT64_MIN, negative timestamps in stream order, and
clamped values whose true order decides corners.

Every case runs as ecc_fast_detect, as prepare + finish and as ecc_fast_detect_nms (the candidate
form: every slice size here is a multiple of 4 below 16384).  Each run fills the flags with 0xCD
first, compares flags and final surface with orc.fast_detect exactly, and reads the path taken
from ecc_fast_detect_stats()["overflow_items"]: at least the items the case's facts send to the
dense kernel, and exactly that many where the case rules every other exit out.
"""
import ctypes as C

import numpy as np
import pytest

import arc_path_cases as ap

pytestmark = pytest.mark.gpu
CAP = 4096


def dev(ecc, a):
    return ecc.DeviceArray.from_numpy(np.ascontiguousarray(a))


def _surface(ecc, c):
    return dev(ecc, np.zeros(c["W"] * c["H"], np.int64) if c["sae0"] is None else c["sae0"])


def _one_call(ecc, ctx, c, cfg):
    sae, n = _surface(ecc, c), len(c["xy"])
    flags = ecc.DeviceArray(n, np.uint8)
    flags.fill_bytes(0xCD)  # every flag must be written
    ctx.fast_detect(dev(ecc, c["xy"]), dev(ecc, c["t"]), n, cfg, sae, flags)
    return flags.numpy(), sae.numpy(), None


def _two_calls(ecc, ctx, c, cfg):
    sae, n = _surface(ecc, c), len(c["xy"])
    flags = ecc.DeviceArray(n, np.uint8)
    flags.fill_bytes(0xCD)
    local = ecc.DeviceArray(c["W"] * c["H"], np.int64)
    d_xy, d_t = dev(ecc, c["xy"]), dev(ecc, c["t"])
    ecc.check(ecc.lib.ecc_fast_detect_prepare(ctx.ctx, d_xy.ptr, d_t.ptr, n, C.byref(cfg), local.ptr, ctx.stream))
    ecc.check(ecc.lib.ecc_fast_detect_finish(ctx.ctx, d_xy.ptr, d_t.ptr, n, C.byref(cfg), sae.ptr, flags.ptr,
                                             ctx.stream))
    return flags.numpy(), sae.numpy(), None


def _with_nms(ecc, ctx, c, cfg):
    sae, n = _surface(ecc, c), len(c["xy"])
    assert c["S"] % 4 == 0 and c["S"] <= 16384  # the flag pass writes the candidate lists itself
    ns = (n + c["S"] - 1) // c["S"]
    flags = ecc.DeviceArray(n, np.uint8)
    flags.fill_bytes(0xCD)
    out, cnt = ecc.DeviceArray(ns * CAP, ecc.CORNER_DTYPE), ecc.DeviceArray(ns, np.int32)
    ctx.fast_detect_nms(dev(ecc, c["xy"]), dev(ecc, c["t"]), n, cfg, sae, flags, 15, CAP, out, cnt)
    assert ctx.corner_nms_status() == 0
    return flags.numpy(), sae.numpy(), (out.numpy(), cnt.numpy())


RUNS = {"one_call": _one_call, "prepare_finish": _two_calls, "detect_nms": _with_nms}
# the cases whose facts rule out every exit but the counted ones (no clamped value, hence no merged tie)
EXACT_COUNT = ("queue_full", "queue_full_heavy", "deep_runs")
_nms = {}


def _oracle_nms(orc, name, c, o_flags):
    if name not in _nms:
        out, cnt, rc = orc.corner_nms(c["xy"], o_flags, c["W"], c["H"], slice_events=c["S"], cap=CAP)
        assert rc == 0
        _nms[name] = (out, cnt)
    return _nms[name]


@pytest.mark.parametrize("run", list(RUNS))
@pytest.mark.parametrize("name", ap.CASES)
def test_arc_path(ecc, orc, gpu, name, run):
    c = ap.case(name)
    o_flags, o_sae = ap.oracle(orc, name)
    cfg = ecc.corner_cfg(width=c["W"], height=c["H"], border_mode=0, first_detect_slice=c["first"],
                         slice_events=c["S"])
    g_flags, g_sae, nms = RUNS[run](ecc, gpu, c, cfg)
    assert gpu.fast_detect_status() == 0  # stream order, negative or not
    stats = gpu.fast_detect_stats()
    must = int(ap.predicted(name).sum())
    print(f"{name} [{run}]: overflow_items {stats['overflow_items']} of {stats['items']}, predicted "
          f"{'=' if name in EXACT_COUNT else '>='} {must}; {int(o_flags.sum())} corner events")
    assert set(np.unique(g_flags).tolist()) <= {0, 1}, "a flag was not written"
    bad = np.nonzero(g_flags != o_flags)[0]
    assert bad.size == 0, (f"{bad.size} flags differ, first at events {bad[:8].tolist()} (slices "
                           f"{(bad[:8] // c['S']).tolist()}): device {g_flags[bad[:8]].tolist()}")
    assert (g_sae == o_sae).all()
    if nms is not None:
        o_out, o_cnt = _oracle_nms(orc, name, c, o_flags)
        out, cnt = nms
        assert (cnt == o_cnt).all()
        for s in np.nonzero(o_cnt)[0]:
            assert (out[s * CAP: s * CAP + o_cnt[s]] == o_out[s * CAP: s * CAP + o_cnt[s]]).all(), s
    # the path: what the stream was built for happened
    assert stats["items"] == 12 * stats["groups"] and stats["slices"] == len(c["xy"]) // c["S"]
    if name in EXACT_COUNT:
        assert stats["overflow_items"] == must
    elif name == "mixed_clamp":
        assert must == 0 and stats["overflow_items"] > 0  # only merged ties send its items to the exact tests
    else:
        assert stats["overflow_items"] >= must
    assert stats["overflow_items"] <= int(ap.own_events(c["xy"], c["S"], c["W"], c["H"]).sum())
