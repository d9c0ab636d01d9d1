"""The tracker edge cases of tests/tracker_cases.py, on the CPU: every case's census — counted from
the oracle's states around every slice, with the switch points of csrc/tracker_paths.hpp read
through the probe — meets the condition the case was built for, on both sides of

  kFT (which kernel), the fast kernel's lane shift, chunk width, kFList and its 64-track tail;
  kBrute / radius / int16 (grid or not), negative cells and a bucket collision, every change of
  (L, lists_ok), kLaneList, the 64-track tail and kTailCap; the 64-candidate grouping switch; the
  exact max_distance and group_radius.

Every family A case equals the reference's compiled CornerTracker (tests/golden/ref_cpu/
track_<case>.npz, or a live run of oracle/_ref/ref_cpu where it is built) slice by slice in the
oracle; the fixtures' input hashes match the generators; a padded case leaves the case's own tracks
as they were.
"""
import numpy as np
import pytest

import ref_cpu_cases as rc
import tracker_cases as tc

CASES = tc.all_cases()
A = [c for c in CASES if c.family == "A"]
APAD = [c for c in CASES if c.family == "Apad"]
B = [c for c in CASES if c.family == "B" and not c.name.endswith("/slices")]
ids = lambda cs: [c.name for c in cs]


def wide(p):
    return bool(len(p)) and bool((p < -32768).any() or (p > 32767).any())


def uses_grid(case, s, C):
    ok, _ = tc.grid(tc.bits(case.cfg[0]))
    return ok and C > tc.consts()["kBrute"] and not wide(case.slices[s])


def general_lanes(case, s, T, C):
    return 1 if uses_grid(case, s, C) else tc.lanes_table(5000)[T][0]


def check_census(case, census, snaps_of):
    k = tc.consts()
    w = case.want
    kFT = k["kFT"]
    nb = w.get("block", 4)
    second = [(s, census[s]) for s in range(nb - 3, len(census), nb)]  # the [C] slice of every block
    if "pairs" in w:
        assert [(T, C) for _, (T, C, _, _) in second] == w["pairs"]
    if w.get("fast"):
        assert all(T + C <= kFT for T, C, _, _ in census)
    if w.get("general"):
        assert all(T + C > kFT for _, (T, C, _, _) in second)
    if w.get("handover"):
        sums = {T + C for _, (T, C, _, _) in second}
        assert {kFT, kFT + 1} <= sums and max(T for _, (T, _, _, _) in second) > kFT
        ends = case.launch_ends()
        starts = [0] + ends[:-1]
        over = [s for s, (T, C, _, _) in second if T + C > kFT and T <= kFT and census[s - 1][0] + census[s - 1][1] <= kFT]
        assert len(over) >= 3
        for s in over:  # the first slice above kFT: first, in the middle, or last in its launch
            a, b = next((a, b) for a, b in zip(starts, ends) if a <= s < b)
            assert {"first": s == a, "middle": a < s < b - 1, "last": s == b - 1}[w["phase"]], (s, a, b)
        if w["phase"] == "first":  # a launch that begins above kFT tracks, the next one at or under it
            began = [census[a][0] for a in starts]
            assert any(x > kFT and y <= kFT for x, y in zip(began, began[1:]))
    if w.get("fast_rules"):
        assert {tc.fast_rule(T, C) for _, (T, C, _, _) in second} == {(1, k["kFChunkNarrow"]), (1, k["kFChunkWide"]),
                                                                     (2, k["kFChunkNarrow"]), (2, k["kFChunkWide"])}
    blocks = [(s, case.slices[s - 1], case.slices[s]) for s, _ in second]
    if w.get("fast_lists"):
        seen = set()
        for s, P, D in blocks:
            sh, chunk = tc.fast_rule(len(P), len(D))
            r = tc.round0(P, D, 900, 1 << sh, chunk)
            seen.add((int(r["n_in"].max()), bool(r["lane"].max() > k["kFList"])))
        assert {(m, False) for m in range(1, k["kFList"] + 1)} <= seen   # lists that fit
        assert (k["kFList"] + 1, False) in seen                            # the merged list alone overflows
        assert (k["kFList"] + 1, True) in seen and (40, True) in seen      # one lane overflows
    if "unresolved" in w:
        got = []
        for s, P, D in blocks:
            T, C = census[s][:2]
            fast = T + C <= kFT
            L = 1 << tc.fast_rule(T, C)[0] if fast else general_lanes(case, s, T, C)
            r = tc.round0(P, D, w["md2"], L, tc.fast_rule(T, C)[1] if fast else None)
            got.append(len(r["unresolved"]))
            if "tail_total" in w:
                tot = int(r["n_in"][r["unresolved"]].sum())
                assert tot == w["tail_total"][len(got) - 1] and r["lane"].max() <= k["kLaneList"]
                assert tc.lanes_table(5000)[T][1] == 1 and got[-1] <= k["kTailTracks"]
        assert got == w["unresolved"]
    if "grid" in w:
        assert [uses_grid(case, s, c[1]) for s, c in second] == w["grid"]
    if w.get("wide"):
        assert any(wide(p) for p in case.slices)
    if "Ts" in w:
        tab = tc.lanes_table(5000)
        assert [T for _, (T, _, _, _) in second] == w["Ts"]
        assert {tab[t] != tab[t + 1] for t in w["switches"]} == {True} and len(w["switches"]) >= 7
        assert {tab[T][1] for T in w["Ts"]} == {0, 1} and {tab[T][0] for T in w["Ts"]} >= {1, 2, 4, 8, 16, 32, 64}
        crossed = 0
        for s, P, D in blocks:  # ties whose lower index sits in the higher lane
            L = tab[len(P)][0]
            for i in range(min(len(P), 140)):
                d = np.nonzero(((D - P[i]) ** 2).sum(1) == 4)[0]
                assert len(d) == 2
                crossed += L > 1 and d[0] % L > d[1] % L
        assert crossed > 100
    if "lane_max" in w:
        got = [int(tc.round0(P, D, w["md2"], w["L"])["lane"].max()) for _, P, D in blocks]
        assert got == w["lane_max"] and w["L"] == tc.lanes_table()[4][0]
    if "Gs" in w:
        on = lambda T, C: (T + C <= kFT) == (w["kern"] == "fast")
        assert set(w["Gs"]) <= {G for T, C, G, _ in census if on(T, C)}
        _, snaps = snaps_of(tc.by_name(case.name + "/slices"))
        for s, (T, C, G, _) in enumerate(census):
            ng = len(snaps[s + 1].groups)
            if C == 0:
                assert G == 0 and ng == 0  # an empty last slice: an empty group view
            elif G in w["Gs"] and C == G:
                assert ng == {"one": 1, "singletons": G, "interleaved": 2}[w["shape"]]
                if w["shape"] == "interleaved":
                    lab = snaps[s + 1].labels
                    order = snaps[s + 1].tracks[snaps[s + 1].tracks[:, tc.COL_FSLD] == 0][:, 2]
                    assert sorted(lab[:(G + 1) // 2]) == sorted(order[0::2]) and sorted(lab[(G + 1) // 2:]) == sorted(order[1::2])
    if "kern" in w and "Gs" not in w:
        assert all((T + C <= kFT) == (w["kern"] == "fast") for T, C, _, _ in census if T + C > 0)
    if w.get("cut_room"):
        _, snaps = snaps_of(case)
        cut, short = tc.cut_to_room(snaps[2], snaps[3], case.max_tracks)
        T, C, G, M = census[2]
        assert short == w["short"] and T == w["a"] and M == w["a"] // 2
        assert len(cut.tracks) == case.max_tracks - w["a"] // 2 - w["a"] % 2 < case.max_tracks  # room != free slots
        assert len(snaps[3].tracks) - len(cut.tracks) == int(short)
    if w.get("collide"):
        cell = w["cell"]
        hit = 0
        for p in w["tracks"]:
            v = tc.visited_cells((int(p[0]), int(p[1])), cell - 1, cell)
            assert len(v) <= 9
            hit += len(set(tc.buckets(v))) < len(v)
        assert hit >= 1
        xs = np.concatenate(case.slices)
        assert xs.min() == -32769 and xs.max() == 32768 and (-32768 in xs) and (32767 in xs)
        assert all(c[3] == w["matched_all"] for _, c in second)
        assert any(min(a) < 0 for p in w["tracks"] for a in tc.visited_cells((int(p[0]), int(p[1])), cell - 1, cell))


@pytest.fixture(scope="module")
def snaps_of(ecc, orc):
    return lambda case: tc.oracle_run(ecc, orc, case)


@pytest.mark.parametrize("case", B, ids=ids(B))
def test_census_b(case, snaps_of):
    census, snaps = snaps_of(case)
    assert len(census) == len(case.slices) and sorted(snaps) == case.launch_ends()
    nb = case.want.get("block", 4)
    with_dets = sum(census[s][1] > 0 for s in range(nb - 3, len(census), nb))
    live = sum(len(sn.tracks) > 0 for sn in snaps.values())
    assert live >= min(len(snaps), with_dets)  # launches end on live tracks: a wrong match shows
    assert max(max(T, C) for T, C, _, _ in census) <= 4096
    check_census(case, census, snaps_of)


@pytest.mark.parametrize("case", A, ids=ids(A))
def test_family_a_expectations(case, snaps_of):
    """What each threshold case was built to show, in the oracle."""
    census, snaps = snaps_of(case.per_slice())
    assert all(T + C <= tc.consts()["kFT"] and C <= 64 for T, C, _, _ in census)
    for s, m in case.want.get("matched_after", {}).items():
        assert census[s][3] == m, (s, census[s])
    for s, g in case.want.get("groups_after", {}).items():
        assert len(snaps[s + 1].groups) == g, (s, len(snaps[s + 1].groups))
    if case.name == "A_5_frames_0":
        assert all(len(sn.tracks) == 0 for sn in snaps.values()) and snaps[len(census)].next_label == sum(c[1] for c in census)


@pytest.mark.parametrize("case", A, ids=ids(A))
def test_family_a_reference(case, ecc, orc, tmp_path):
    """The reference's compiled CornerTracker (live, or its stored dump) == the oracle, slice by slice;
    the stored dump answers this generator's input and equals a live run."""
    l3 = tc.lists3(case.slices)
    dump = rc.ref_track("track_" + case.name, tmp_path, l3, cfg=case.cfg)
    stored = rc.GOLDEN / f"track_{case.name}.npz"
    assert stored.exists(), f"{stored.name} is not recorded"
    z = np.load(stored)
    assert str(z["input_sha"]) == rc.sha("track", [rc.cfg_words(case.cfg)], rc.pack_lists(l3, 3))
    # With a radius that is not >= 0 no group ever forms, and the reference never assigns a new
    # track's group_id: it dumps an uninitialised int there (the oracle says -1).
    cut = (lambda key: key) if float(case.cfg[6]) >= 0 else (lambda key: key[:-1])
    keys = lambda d: [([cut(rc.track_key(t)) for t in tr], gr) for tr, gr in d]
    assert keys(rc.unpack_tracker(z["out.i32"])) == keys(dump)
    otr = orc.OracleTracker(tc.ecc_cfg(ecc, case.cfg))
    for s, (p, (tracks, groups)) in enumerate(zip(case.slices, dump)):
        otr.update(tc.corners_of(ecc, p))
        assert [cut(rc.struct_track_key(t)) for t in otr.tracks(ecc.Track, 4096)] == [cut(rc.track_key(t)) for t in tracks], s
        assert rc.struct_group_keys(*otr.groups(ecc.Group, 4096)) == groups, s


@pytest.mark.parametrize("case", APAD, ids=ids(APAD))
def test_padding(case, snaps_of):
    k = tc.consts()
    census, snaps = snaps_of(case)
    kind = case.want["pad_kind"]
    later = census[1:]
    if kind == "brute":
        assert all(T + C > k["kFT"] and C <= k["kBrute"] for T, C, _, _ in later)
    else:
        assert all(C > k["kBrute"] for _, C, _, _ in census)
        assert all(wide(p) for p in case.slices) == (kind == "wide")
        assert (min(p.min() for p in case.slices) < -10000) == (kind == "negative")
    if kind in ("grid", "negative"):  # inside int16 with C > kBrute: the radius alone decides
        on = [uses_grid(case, s, c[1]) for s, c in enumerate(census)]
        assert set(on) == {tc.grid(tc.bits(case.cfg[0]))[0]}
        if "md_below_1e5" in case.name:   # grid_ok's upper end: on just below 1e5 (cells of 100002), off at it
            assert on[0] and tc.grid(tc.bits(case.cfg[0]))[1] == 100002
        if "md_1e5" in case.name:
            assert not on[0]
    assert max(T for T, _, _, _ in census) <= 4096
    # The case's own tracks are what they were without the fillers (labels and group ids aside).
    # Not where the fillers are in range of the case (want["interact"]), and not for the shifted
    # scene: a missed track's blended prediction rounds differently far from the origin, so fp32
    # tracking is not translation invariant.  Both are compared with the oracle on the device.
    if kind == "negative" or case.want["interact"]:
        return
    base = tc.by_name(case.name.split("+")[0])
    _, bsn = snaps_of(base)
    want = bsn[len(base.slices)].tracks
    got = snaps[len(case.slices)].tracks
    mine = got[got[:, tc.COL_X] < 2500]
    cols = [c for c in range(tc.TRACK_WORDS) if c not in (2, tc.TRACK_WORDS - 1)]
    assert np.array_equal(mine[:, cols], want[:, cols])
