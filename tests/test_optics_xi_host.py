"""CPU tests of the xi ("chi") cluster extraction: the reference's chi_test_1 ... chi_test_11 as
data, ecc_optics_xi_host against the literal restatement of optics.hpp:814-944
(tests/optics_xi_ref.py), and the ecc_optics_xi boundary (every invalid argument is rejected on
the host, before a device is touched: the pointers here are not addresses of anything).  Every
comparison is of exact integers."""
import ctypes as C
import math

import numpy as np
import pytest

import optics_xi_ref as ref

CTX, REACH, CNT, CLUSTERS, NCL = 0x1000, 0x2000, 0x3000, 0x4000, 0x5000
SENTINEL = -7


def want(plot, params):
    return ref.pairs_array(ref.chi_clusters(plot, *params))


# ------------------------------------------------------------------------------ the reference KATs
def test_kat_file_holds_the_twelve_calls():
    assert len(ref.KAT_NAMES) == 12
    assert sorted(len(ref.KAT[k]["reach"]) for k in ref.KAT_NAMES)[-2:] == [855, 855]


@pytest.mark.parametrize("name", ref.KAT_NAMES)
def test_restatement_gives_the_reference_pairs(name):
    k = ref.KAT[name]
    got = ref.chi_clusters(k["reach"], k["chi"], k["min_pts"], k["steep_area_min_diff"])
    assert [list(p) for p in got] == k["expected"]


@pytest.mark.parametrize("name", ref.KAT_NAMES)
def test_host_form_gives_the_reference_pairs(ecc, name):
    k = ref.KAT[name]
    got = ecc.optics_xi_host(k["reach"], k["chi"], k["min_pts"], k["steep_area_min_diff"])
    assert got.tolist() == k["expected"]


# ------------------------------------------------------------------------------ host form vs restatement
def host_cases():
    rng = np.random.default_rng(814944)
    plots = [ref.random_plot(rng, n) for n in range(71) for _ in range(3)]
    plots += [ref.random_plot(rng, n) for n in (513, 2000, 20000)]
    # values without the undefined marker, and a denser set around one level
    plots += [ref.random_plot(rng, n, ref.EQ_VALUES[1:]) for n in (33, 64, 65, 700)]
    plots += [ref.random_plot(rng, n, np.array([-1.0, 1.0, 0.75, 0.5625])) for n in (17, 130)]
    return plots


@pytest.fixture(scope="module")
def plots():
    return host_cases()


@pytest.mark.parametrize("params", ref.PARAMS, ids=str)
def test_host_form_matches_restatement_on_random_plots(ecc, plots, params):
    for p in plots:
        assert np.array_equal(ecc.optics_xi_host(p, *params), want(p, params)), (len(p), params)


def test_random_plots_reach_exact_equality(plots):
    """With chi 0.25 over powers of 3/4 and 2, g(i+1) == g(i) * (1 - chi) and
    |start - end| == start * chi both occur in the data above."""
    stats = {}
    for p in plots:
        ref.chi_clusters(p, *ref.PARAMS[0], stats=stats)
    assert stats.get("steep_eq", 0) > 0 and stats.get("in_range_eq", 0) > 0


@pytest.mark.parametrize("n", [2, 3, 64, 65, 1000])
@pytest.mark.parametrize("params", ref.PARAMS, ids=str)
def test_all_undefined_descending_ascending(ecc, n, params):
    for p in (np.full(n, -1.0), np.arange(n, 0, -1, dtype=np.float64), np.arange(1, n + 1, dtype=np.float64),
              0.5 ** np.arange(n, dtype=np.float64), 2.0 ** np.arange(n, dtype=np.float64)):
        assert np.array_equal(ecc.optics_xi_host(p, *params), want(p, params))


def test_fewer_than_two_points_have_no_clusters(ecc):
    for p in (np.zeros(0), np.array([3.0]), np.array([-1.0])):
        assert len(ecc.optics_xi_host(p, 0.1, 4)) == 0


def test_staircase(ecc):
    """8192 points in unit steps of 4: 2048 live steep-down areas, 2048 pairs at one steep-up area."""
    p = ref.staircase()
    w = want(p, (ref.STAIR_CHI, 2, 0.0))
    assert len(w) == 2048
    assert np.array_equal(ecc.optics_xi_host(p, ref.STAIR_CHI, 2), w)


def test_truncated_call(ecc):
    k = ref.KAT["chi_test_11a"]
    r = np.asarray(k["reach"], np.float64)
    cap = 5
    out = np.full((len(k["expected"]) + 3, 2), SENTINEL, np.int32)
    n_out = C.c_int64(-1)
    rc = ecc.lib.ecc_optics_xi_host(r.ctypes.data, r.size, k["chi"], k["min_pts"], k["steep_area_min_diff"],
                                    out.ctypes.data, cap, C.addressof(n_out))
    assert rc == ecc.ERR_CAPACITY
    assert n_out.value == len(k["expected"])
    assert out[:cap].tolist() == k["expected"][:cap]
    assert (out[cap:] == SENTINEL).all()
    # cap equal to the count: complete and OK
    rc = ecc.lib.ecc_optics_xi_host(r.ctypes.data, r.size, k["chi"], k["min_pts"], k["steep_area_min_diff"],
                                    out.ctypes.data, len(k["expected"]), C.addressof(n_out))
    assert rc == ecc.OK and out[:len(k["expected"])].tolist() == k["expected"]
    assert (out[len(k["expected"]):] == SENTINEL).all()


def test_non_finite_values_stay_inside_the_plot(ecc):
    """NaN and infinities: an unspecified result, but every pair inside the plot, n_out and the
    writes bounded by cap."""
    rng = np.random.default_rng(9)
    for p in ref.hostile_plots(rng, list(range(2, 40)) + [257, 1000]):
        for params in ref.PARAMS:
            cap = 16
            out = np.full((cap + 2, 2), SENTINEL, np.int32)
            n_out = C.c_int64(-1)
            rc = ecc.lib.ecc_optics_xi_host(p.ctypes.data, p.size, *params[:2], params[2], out.ctypes.data, cap,
                                            C.addressof(n_out))
            assert rc in (ecc.OK, ecc.ERR_CAPACITY) and n_out.value >= 0
            k = min(n_out.value, cap)
            assert ((out[:k] >= 0) & (out[:k] < p.size)).all() and (out[k:] == SENTINEL).all()


def test_host_form_rejects_bad_arguments(ecc):
    r = np.array([3.0, 1.0, 2.0])
    out = np.zeros((4, 2), np.int32)
    n_out = C.c_int64(0)

    def call(reach=r.ctypes.data, n=3, chi=0.1, min_pts=2, samd=0.0, clusters=out.ctypes.data, cap=4,
             n_out_p=C.addressof(n_out)):
        return ecc.lib.ecc_optics_xi_host(reach, n, chi, min_pts, samd, clusters, cap, n_out_p)

    assert call() == ecc.OK
    for bad in (dict(n=-1), dict(cap=-1), dict(n_out_p=None), dict(reach=None), dict(clusters=None),
                dict(chi=0.0), dict(chi=1.0), dict(chi=math.nan), dict(chi=math.inf), dict(samd=-0.5),
                dict(samd=1.0), dict(samd=math.nan), dict(min_pts=1), dict(min_pts=0), dict(min_pts=-4)):
        assert call(**bad) == ecc.ERR_INVALID, bad
    assert call(reach=None, n=0, clusters=None, cap=0) == ecc.OK and n_out.value == 0


# ------------------------------------------------------------------------------ the device entry's boundary
def call(ecc, ctx=CTX, reach=REACH, n_segs=2, stride=64, counts=CNT, chi=0.1, min_pts=4, samd=0.0,
         clusters=CLUSTERS, cap=16, n_clusters=NCL):
    return ecc.lib.ecc_optics_xi(ctx, reach, n_segs, stride, counts, chi, min_pts, samd, clusters, cap, n_clusters, None)


def test_library_exports_optics_xi(ecc):
    for name in ("ecc_optics_xi", "ecc_optics_xi_status", "ecc_optics_xi_host"):
        assert hasattr(ecc.lib, name)
    assert hasattr(ecc.Context, "optics_xi") and hasattr(ecc.Context, "optics_xi_status")
    assert callable(ecc.optics_xi_host)


BAD = [
    dict(ctx=None), dict(reach=None), dict(clusters=None), dict(n_clusters=None),
    dict(n_segs=-1), dict(cap=-1), dict(stride=0), dict(stride=-5), dict(stride=2 ** 31),
    dict(chi=0.0), dict(chi=1.0), dict(chi=-0.1), dict(chi=1.5), dict(chi=math.nan), dict(chi=math.inf),
    dict(chi=-math.inf),
    dict(samd=-0.01), dict(samd=1.0), dict(samd=2.0), dict(samd=math.nan), dict(samd=math.inf),
    dict(min_pts=1), dict(min_pts=0), dict(min_pts=-3),
]


@pytest.mark.parametrize("bad", BAD, ids=lambda d: ",".join(f"{k}={v}" for k, v in d.items()))
def test_optics_xi_rejects_bad_arguments(ecc, bad):
    assert call(ecc, **bad) == ecc.ERR_INVALID


def test_optics_xi_rejects_bad_arguments_with_no_segments(ecc):
    """The argument ranges hold for an empty call too (only the data pointers may then be NULL)."""
    for bad in BAD:
        if set(bad) & {"reach", "clusters", "n_clusters", "n_segs"}:
            continue
        assert call(ecc, n_segs=0, **bad) == ecc.ERR_INVALID, bad


def test_optics_xi_no_segments_is_ok(ecc):
    assert call(ecc, n_segs=0) == ecc.OK
    assert call(ecc, n_segs=0, reach=None, counts=None, clusters=None, n_clusters=None) == ecc.OK
    # the limits themselves are valid
    assert call(ecc, n_segs=0, stride=2 ** 31 - 1, chi=math.nextafter(1.0, 0.0), samd=math.nextafter(1.0, 0.0),
                min_pts=2, cap=0) == ecc.OK
    assert call(ecc, n_segs=0, stride=1, chi=5e-324, samd=0.0, min_pts=2 ** 31 - 1) == ecc.OK


def test_optics_xi_status_needs_a_context(ecc):
    assert ecc.lib.ecc_optics_xi_status(None, None) == ecc.ERR_INVALID
