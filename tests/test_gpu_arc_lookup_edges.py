"""The edges of arc_kernel's window lookups (csrc/corner_arc.hip: byte offsets in the pixel
records, every circle read off one base address) on the streams of tests/arc_lookup_cases.py
(tests/test_arc_lookup_cases.py shows on the CPU that each does what it was built for): a window
exactly at the compact list's capacity, kValCap + kWinPix values, where the highest word any test
can read decides a planted corner, and the same window one value over it, which must go to
arc_dense_kernel; deciding reads at slices 0 and 31; task pixels in every corner and on every edge
of the own tile, in an interior tile and in border tiles whose windows the sensor clips (the
smallest and the largest displacement from the base); a pixel with 32 values right before one no
event touches.

Every case runs as ecc_fast_detect, as prepare + finish and as ecc_fast_detect_nms.  Each run fills
the flags with 0xCD first and compares flags and final surface with orc.fast_detect exactly; the
path taken is read from ecc_fast_detect_stats()["overflow_items"], which these streams pin exactly
(no clamped value, no value above t_last, queues far from full).
"""
import ctypes as C

import numpy as np
import pytest

import arc_lookup_cases as lc
import arc_path_cases as ap

pytestmark = pytest.mark.gpu
CAP = 4096


def dev(ecc, a):
    return ecc.DeviceArray.from_numpy(np.ascontiguousarray(a))


def _buffers(ecc, c):
    n = len(c["xy"])
    flags = ecc.DeviceArray(n, np.uint8)
    flags.fill_bytes(0xCD)  # every flag must be written
    return dev(ecc, np.zeros(c["W"] * c["H"], np.int64)), flags, n


def _one_call(ecc, ctx, c, cfg):
    sae, flags, n = _buffers(ecc, c)
    ctx.fast_detect(dev(ecc, c["xy"]), dev(ecc, c["t"]), n, cfg, sae, flags)
    return flags.numpy(), sae.numpy(), None


def _two_calls(ecc, ctx, c, cfg):
    sae, flags, n = _buffers(ecc, c)
    local = ecc.DeviceArray(c["W"] * c["H"], np.int64)
    d_xy, d_t = dev(ecc, c["xy"]), dev(ecc, c["t"])
    ecc.check(ecc.lib.ecc_fast_detect_prepare(ctx.ctx, d_xy.ptr, d_t.ptr, n, C.byref(cfg), local.ptr, ctx.stream))
    ecc.check(ecc.lib.ecc_fast_detect_finish(ctx.ctx, d_xy.ptr, d_t.ptr, n, C.byref(cfg), sae.ptr, flags.ptr,
                                             ctx.stream))
    return flags.numpy(), sae.numpy(), None


def _with_nms(ecc, ctx, c, cfg):
    sae, flags, n = _buffers(ecc, c)
    assert c["S"] % 4 == 0 and c["S"] <= 16384 and n % c["S"] == 0
    ns = n // c["S"]
    out, cnt = ecc.DeviceArray(ns * CAP, ecc.CORNER_DTYPE), ecc.DeviceArray(ns, np.int32)
    ctx.fast_detect_nms(dev(ecc, c["xy"]), dev(ecc, c["t"]), n, cfg, sae, flags, 15, CAP, out, cnt)
    assert ctx.corner_nms_status() == 0
    return flags.numpy(), sae.numpy(), (out.numpy(), cnt.numpy())


RUNS = {"one_call": _one_call, "prepare_finish": _two_calls, "detect_nms": _with_nms}
_nms = {}


def _oracle_nms(orc, name, c, o_flags):
    if name not in _nms:
        out, cnt, rc = orc.corner_nms(c["xy"], o_flags, c["W"], c["H"], slice_events=c["S"], cap=CAP)
        assert rc == 0
        _nms[name] = (out, cnt)
    return _nms[name]


@pytest.mark.parametrize("run", list(RUNS))
@pytest.mark.parametrize("name", lc.CASES)
def test_arc_lookup_edge(ecc, orc, gpu, name, run):
    c = lc.case(name)
    o_flags, o_sae = lc.oracle(orc, name)
    cfg = ecc.corner_cfg(width=c["W"], height=c["H"], border_mode=0, first_detect_slice=c["first"],
                         slice_events=c["S"])
    g_flags, g_sae, nms = RUNS[run](ecc, gpu, c, cfg)
    assert gpu.fast_detect_status() == 0
    stats = gpu.fast_detect_stats()
    must = int(lc.predicted(name).sum())
    print(f"{name} [{run}]: overflow_items {stats['overflow_items']} of {stats['items']}, predicted = {must}; "
          f"{int(o_flags.sum())} corner events")
    assert set(np.unique(g_flags).tolist()) <= {0, 1}, "a flag was not written"
    bad = np.nonzero(g_flags != o_flags)[0]
    assert bad.size == 0, (f"{bad.size} flags differ, first at events {bad[:8].tolist()} (slices "
                           f"{(bad[:8] // c['S']).tolist()}): device {g_flags[bad[:8]].tolist()}")
    planted = [e for e, *_ in c["probes"]] + [e for e, *_ in c.get("full", [])]
    assert (g_flags[planted] == 1).all()  # the planted corners, by name (implied by the comparison above)
    assert (g_sae == o_sae).all()
    if nms is not None:
        o_out, o_cnt = _oracle_nms(orc, name, c, o_flags)
        out, cnt = nms
        assert (cnt == o_cnt).all()
        for s in np.nonzero(o_cnt)[0]:
            assert (out[s * CAP: s * CAP + o_cnt[s]] == o_out[s * CAP: s * CAP + o_cnt[s]]).all(), s
    # the path: at the capacity the item stays with arc_kernel, one value over it goes to the dense kernel
    assert stats["items"] == 12 * stats["groups"] and stats["slices"] == len(c["xy"]) // c["S"]
    assert must == (1 if name == "cap_over" else 0)
    assert stats["overflow_items"] == must
