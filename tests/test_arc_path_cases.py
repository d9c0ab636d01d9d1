"""The streams of tests/arc_path_cases.py do on the CPU what they were built for: for every case
the oracle's result and the facts, restated from the device code's constants, that send its items
down the intended exit of the arc kernels.  tests/test_gpu_arc_paths.py runs the same streams on
the device and cannot pass vacuously while these hold."""
import numpy as np
import pytest

import arc_path_cases as ap
import ref_cpu_cases as rc

INTERIOR_TILES = (5, 6)  # of the 4 x 3 tiles, the two with no sensor border


def _facts(orc, name):
    c = ap.case(name)
    flags, sae = ap.oracle(orc, name)
    assert len(c["xy"]) <= 100_000 and (np.diff(c["t"]) > 0).all()
    assert ap.tiles_of(c["W"], c["H"]) == (4, 3)
    return c, flags, ap.window_totals(c["xy"], c["S"], c["W"], c["H"])


def test_constants_restate_the_device_code():
    """The numbers the predictions rest on, read back from the source lines they cite."""
    csrc = ap.__file__.rsplit("/tests/", 1)[0] + "/event-camera-clustering-and-optical-flow-estimation_amd/csrc/"
    arc, common = open(csrc + "corner_arc.hip").read(), open(csrc + "corner_common.hpp").read()
    assert f"constexpr int kQ4Cap = {ap.Q4_CAP};" in arc and "#define ECC_ARC_VALCAP 4096" in arc
    assert "total > kValCap + kWinPix" in arc and ap.LIST_CAP == 4580
    for text in (f"constexpr int kGroup = {ap.GROUP};", f"constexpr int kTile = {ap.TILE};",
                 f"constexpr int kHalo = {ap.HALO};", f"constexpr int kRecVals = {ap.REC_VALS};",
                 "constexpr int kVBits = 27;"):
        assert text in common, text


def test_window_totals_and_per_item_on_a_hand_stream():
    """Two slices on the 56 x 42 sensor: pixel (13, 13) twice in slice 0 and once in slice 1 (two
    pairs; in the windows of tiles 0, 1, 4 and 5), pixel (30, 20) once (tile 6's own; in the
    windows of 5 and 6 only: x = 30 is beyond tile 7's halo, y = 20 beyond rows 0 and 2), and an
    event off the sensor."""
    xy = ap.pack([13, 13, 57, 30, 13, 57], [13, 13, 0, 20, 13, 0])
    wt = ap.window_totals(xy, 3, ap.W, ap.H)
    exp = np.full(12, ap.WIN_PIX)
    exp[[0, 1, 4]] += 2
    exp[5] += 3
    exp[6] += 1
    assert wt.shape == (1, 12) and (wt[0] == exp).all()
    own = ap.own_events(xy, 3, ap.W, ap.H)[0]
    assert own.tolist() == [True] + [False] * 5 + [True] + [False] * 5
    flags = np.array([1, 1, 0, 1, 0, 0], np.uint8)  # (13, 13) in slice 0 (one pair), (30, 20) in slice 1
    pi = ap.per_item(flags, xy, 3, ap.W, ap.H)[0]
    assert pi[0] == 1 and pi[6] == 1 and pi.sum() == 2


@pytest.mark.parametrize("name", ["queue_full", "queue_full_heavy"])
def test_queue_full(orc, name):
    c, flags, wt = _facts(orc, name)
    pi = ap.per_item(flags, c["xy"], c["S"], c["W"], c["H"])
    c3 = ap.circle3_survivors(c)
    x, y = ap.unpack(c["xy"])
    tested = (x >= 4) & (x < ap.W - 4) & (y >= 4) & (y < ap.H - 4)
    print(f"{name}: corners per item of group 0 {pi[0].tolist()}, circle-3 survivors {c3[0].tolist()}, window totals "
          f"up to {wt.max()}, {int((tested & (flags == 0)).sum())} tested events are no corners")
    assert (c3 >= pi).all()
    assert (pi[0][list(INTERIOR_TILES)] > ap.Q4_CAP).all()  # hence more than 1024 circle-3 survivors
    assert (tested & (flags == 0)).sum() > 100              # the permuted positions: not everything is a corner
    full = ap.predicted_dense_items(c)
    if name == "queue_full":
        assert wt.max() <= ap.LIST_CAP  # light: arc_kernel keeps the items until its queue overflows
        assert wt.max() == ap.WIN_PIX * 9  # eight rasters in group 0
        assert (full == (c3 > ap.Q4_CAP)).all() and full.sum() >= 2
    else:
        assert (wt[0][list(INTERIOR_TILES)] == ap.WIN_PIX * 33).all()  # 196 * 32 = 6272 tasks in such a tile
        assert wt[0].min() > ap.LIST_CAP and full[0].all()  # group 0: straight to the dense kernel
        assert wt[1].max() <= ap.LIST_CAP and (full[1] == (c3[1] > ap.Q4_CAP)).all()  # group 1 (8 slices): light
        assert (c3[0][list(INTERIOR_TILES)] > ap.Q4_CAP).all()  # whose own queue overflows
    # no clamped value and no tie: nothing but the exits counted above sends an item away
    assert all(n == 0 for n, _ in ap.clamped_values(c))


def test_deep_runs(orc):
    c, flags, wt = _facts(orc, "deep_runs")
    assert wt.max() <= ap.LIST_CAP
    cnt = ap.pair_counts(c["xy"], c["S"], c["W"], c["H"])
    assert sorted({p for _, _, p in c["hot"]}) == list(ap.DEEP_P)
    for hx, hy, p in c["hot"]:
        assert cnt[0, hy, hx] == p and cnt[1, hy, hx] == p, (hx, hy, p)  # exactly p slices of each group
        for g in (0, 1):
            assert cnt[g, hy, hx] == len(c["fired"][(hx, hy, g)])
        if (hx, hy) == (0, 0):
            assert not ap.reads(c["xy"], 0, 0).any()  # no circle reaches the corner pixel: staged, never read
            continue
        r = ap.reads(c["xy"], hx, hy)
        assert set(np.unique(flags[r]).tolist()) == {0, 1}, (hx, hy)  # tests that read it, of both outcomes
        assert set(np.unique(flags[ap.near(c["xy"], hx, hy)]).tolist()) == {0, 1}
    assert any(cnt[0, hy, hx] == 32 and c["fired"][(hx, hy, 0)][-1] == 31 for hx, hy, _ in c["hot"])  # the mask's top bit
    kinds = {}
    for e, hot, g, kind in c["probes"]:
        assert flags[e] == 1 and ap.reads(c["xy"][e:e + 1], *hot)[0], (e, hot)
        kinds.setdefault((hot, g), set()).add(kind)
    p_of = {(hx, hy): p for hx, hy, p in c["hot"]}
    for (hot, g), k in kinds.items():
        assert "in" in k and ("out" in k or p_of[hot] >= 31), (hot, g, k)
    assert len(kinds) == 2 * (len(c["hot"]) - 1)
    # arc_kernel decides everything: narrow 4-byte-key groups, no value clamped (so no merged tie), no
    # value above t_last, light windows, queues far from full
    gf = ap.group_facts(c["t"], c["S"])
    assert len(gf) == 3 and gf[2]["end"] - gf[2]["first"] == 6 * c["S"]  # a ragged third group
    assert all(g["narrow"] and g["t_last"] - g["t_first"] < (1 << 24) - 1 for g in gf)
    assert all(n == 0 for n, _ in ap.clamped_values(c))
    assert ap.circle3_survivors(c).max() < ap.Q4_CAP // 4
    assert not ap.predicted_dense_items(c).any()


@pytest.mark.parametrize("variant", ["a", "b27", "b40", "c", "d"])
def test_future_sae(orc, variant):
    c, flags, wt = _facts(orc, f"future_sae_{variant}")
    assert wt.max() <= ap.LIST_CAP and all(g["narrow"] for g in ap.group_facts(c["t"], c["S"]))
    t_last0 = int(c["t"][ap.GROUP * c["S"] - 1])
    zeroed = c["sae0"].copy()
    for px, py in c["planted"]:
        zeroed[py * ap.W + px] = 0
    f0, _ = ap.run_oracle(orc, c, zeroed)
    got, was = flags[c["probes"]].tolist(), f0[c["probes"]].tolist()
    print(f"future_sae_{variant}: probes {got}, with the planted values zeroed {was}")
    assert was == [0] * 8  # a surface of zeros under one event: everything ties
    sae2d = c["sae0"].reshape(ap.H, ap.W)
    x, y = ap.unpack(c["xy"])
    in_int64 = [int(rc.arc_int64(sae2d, int(x[e]), int(y[e]))) for e in c["probes"][:3]]
    assert in_int64 == [1, 1, 1]  # (slice 0 touches none of these pixels: the initial surface is what the test reads)
    if variant in ("a", "b27", "b40"):
        assert got == [1] * 8  # the value matters at every probe
        lo = {"a": 1, "b27": 1 << 27, "b40": 1 << 40}[variant]
        fut = c["sae0"][c["sae0"] != 0]
        assert fut.min() == t_last0 + lo and fut.max() < t_last0 + lo + 1000 and 0.25 < fut.size / (ap.W * ap.H) < 0.4
    elif variant == "c":
        assert got == [1, 1, 1, 0, 1, 0, 1, 1]
        # probe 3: INT64_MAX over a rest holding INT64_MAX - 1 — a corner in int64 order, none in the reference's doubles
        e = c["probes"][3]
        assert rc.arc_int64(sae2d, int(x[e]), int(y[e]))
        # items 0, 3 and 11 of group 0 see ONE extreme value each, nothing else above t_last
        for tile, v in ((0, ap.I64_MAX), (3, ap.I64_MAX - 1), (11, 1 << 62)):
            tx, ty = tile % 4, tile // 4
            w = sae2d[max(0, ty * 14 - 4): ty * 14 + 18, max(0, tx * 14 - 4): tx * 14 + 18]
            assert set(np.unique(w[w > t_last0]).tolist()) == {v}, tile
        assert t_last0 - ap.V_MAX < 0  # L is negative: INT64_MAX - 1 - L leaves the int64 range
    else:
        assert got == [1, 1, 1, 0, 0, 0, 0, 0]
        for k in (3, 4):  # arcs of INT64_MIN + 1 over INT64_MIN: int64 order finds a corner, the doubles tie
            e = c["probes"][k]
            assert rc.arc_int64(sae2d, int(x[e]), int(y[e]))
        assert (c["sae0"] <= 0).all() and ap.clamped_values(c)[0][1] == 2  # both extremes clamped: "mixed" (L < 0: the zeros are not)
    # the prediction: every group-0 item with events whose window holds a value above t_last
    fut = ap.future_items(c)
    pred = ap.predicted_dense_items(c)
    own = ap.own_events(c["xy"], c["S"], c["W"], c["H"])
    assert (pred[0] == (fut[0] & own[0])).all()
    # (c: tile 7's window holds none of the planted pixels; d: nothing is above t_last)
    assert pred[0].sum() == {"c": 11, "d": 0}.get(variant, 12)


@pytest.mark.parametrize("variant", ap.NEG_VARIANTS)
def test_negative_time(orc, variant):
    c, flags, wt = _facts(orc, f"negative_time_{variant}")
    assert wt.max() <= ap.LIST_CAP and c["sae0"] is None
    gf = ap.group_facts(c["t"], c["S"])
    t = c["t"]
    kinds = [("beyond" if g["beyond"] else "narrow" if g["narrow"] else "wide") for g in gf]
    assert kinds == {"cross_m2p53": ["beyond", "beyond", "narrow"], "i64_min": ["beyond"] * 2,
                     "i64_max": ["beyond"] * 2}.get(variant, ["narrow"] * 2)
    if variant == "small":
        assert t[0] >= -40000 and t[-1] == -1
    elif variant == "cross_zero":
        k = int(np.nonzero(t == 0)[0][0])
        assert k // c["S"] == 12 and 0 < k % c["S"] < c["S"] - 1 and t[0] < 0 < t[-1]
        assert k > c["full"][2] - 37 and k < c["full"][2]  # zero falls inside the test planted in slice 12
    elif variant == "m2p40":
        assert t[0] == -(1 << 40)
    elif variant == "cross_m2p53":
        assert gf[1]["t_first"] < -(1 << 53) < gf[1]["t_last"] and gf[2]["t_last"] < 0
        assert gf[0]["t_first"] <= -(1 << 53)  # the t_first half of beyond_double
    elif variant == "i64_min":
        assert t[0] == ap.I64_MIN
    else:
        assert t[-1] == ap.I64_MAX - 1
    got = [flags[c[k]].tolist() for k in ("zero_arc", "zero_rest", "full")]
    print(f"negative_time_{variant}: zero arcs {got[0]}, zero rest {got[1]}, fully written {got[2]}, "
          f"{int(flags.sum())} corners")
    # slice 0 is negative (0 is the newest value) in every variant but the last
    assert got[0] == ([0] * 3 if variant == "i64_max" else [1] * 3)
    assert got[1] == ([1] * 3 if variant == "i64_max" else [0] * 3)
    # 37 consecutive ticks next to +-2^63 are one double: no arc there; elsewhere a corner
    assert got[2] == ([0] if variant in ("i64_min", "i64_max") else [1]) * len(c["full"])
    # every item of a group that is wide, or narrow and ends below zero with an untouched pixel in its window
    pred = ap.predicted_dense_items(c)
    for g, k in enumerate(kinds):
        if k != "narrow" or variant in ("small", "m2p40") and g == 0:
            assert pred[g].all(), g
    print(f"negative_time_{variant}: predicted items per group {pred.sum(1).tolist()}")
    assert pred[:2].sum() == {"small": 14, "cross_zero": 0, "m2p40": 14}.get(variant, 24)


def test_mixed_clamp(orc):
    c, flags, wt = _facts(orc, "mixed_clamp")
    gf = ap.group_facts(c["t"], c["S"])
    assert all(g["narrow"] for g in gf) and wt.max() <= ap.LIST_CAP
    t_last0 = gf[0]["t_last"]
    s0 = c["sae0"]
    assert s0.max() <= t_last0 - (1 << 27) - 1 and s0.min() >= t_last0 - (1 << 40)
    single = (s0 == t_last0 - (1 << 28)).mean()
    assert 0.2 < single < 0.4
    assert ap.clamped_values(c)[0] == (ap.W * ap.H, np.unique(s0).size) and np.unique(s0).size > 1000
    f_eq, _ = ap.run_oracle(orc, ap.mixed_clamp(all_equal=True))
    got, was = flags[c["probes"]].tolist(), f_eq[c["probes"]].tolist()
    print(f"mixed_clamp: probes {got}, over one single old value {was}; {int((flags != f_eq).sum())} flags differ")
    assert got == [1] * 8 and was == [0] * 8  # the old values' true order decides these corners
    # sparse: most tests see fewer than seven unclamped values on circle 3 (arc_keys cannot decide them on keys)
    cnt = ap.pair_counts(c["xy"], c["S"], c["W"], c["H"])[0]
    assert (cnt == 0).mean() > 0.1
    assert not ap.predicted_dense_items(c).any()  # none of the counted exits: only merged ties send items away
