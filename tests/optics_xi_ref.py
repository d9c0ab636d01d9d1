"""A literal Python restatement of optics::get_chi_clusters_flat (OPT/include/optics/optics.hpp:
814-944), the comparator of the xi-extraction tests.  Python floats are IEEE doubles and every
expression keeps the reference's operation order, so each decision is the reference's bit for bit.
The restatement is itself pinned by the reference's chi_test_1 ... chi_test_11
(tests/golden/optics_chi_kat.json).

Decisions where the reference is not readable or not defined (the quirk register, Q25-Q27):
geom::in_range(a, b, range) is |a - b| <= range; a plot of fewer than 2 points has no clusters;
min_pts < 2 is rejected."""
import json
from pathlib import Path

import numpy as np

KAT = json.loads((Path(__file__).resolve().parent / "golden" / "optics_chi_kat.json").read_text())
KAT_NAMES = [k for k in KAT if not k.startswith("_")]


def chi_clusters(reach, chi, min_pts, steep_area_min_diff=0.0, stats=None):
    """The (begin, end) pairs in the reference's push order.  stats, when a dict, counts the
    comparisons that met exact equality ("steep_eq", "in_range_eq")."""
    reach = [float(r) for r in reach]
    n = len(reach)
    assert min_pts >= 2
    if n < 2:
        return []
    clusters = []
    sdas = []  # [begin, end, mib]
    mib = 0.0
    max_reach = 0.0
    for r in reach:
        if r > max_reach:
            max_reach = r

    def g(idx):
        assert 0 <= idx <= n
        if idx == n or idx == 0:
            return max_reach
        r = reach[idx]
        return 2 * max_reach if r < 0 else r

    def note(key, a, b):
        if stats is not None and a == b:
            stats[key] = stats.get(key, 0) + 1

    def is_steep_down_pt(idx):
        if idx == 0:
            return True
        if idx + 1 >= n:
            return False
        note("steep_eq", g(idx + 1), g(idx) * (1 - chi))
        return g(idx + 1) <= g(idx) * (1 - chi)

    def is_steep_up_pt(idx):
        if idx + 1 >= n:
            return True
        note("steep_eq", g(idx + 1) * (1 - chi), g(idx))
        return g(idx + 1) * (1 - chi) >= g(idx)

    def filter_sdas():
        f = max(chi, steep_area_min_diff)
        sdas[:] = [s for s in sdas if mib <= g(s[0]) * (1 - f)]
        for s in sdas:
            s[2] = max(s[2], mib)

    def get_sda_end(start):
        last, idx = start, start + 1
        while idx < n:
            if idx - last >= min_pts:
                return last
            if g(idx) > g(idx - 1):
                return last
            if is_steep_down_pt(idx):
                last = idx
            idx += 1
        return max(n - 2, last)

    def get_sua_end(start):
        last, idx = start, start + 1
        while idx < n:
            if idx - last >= min_pts:
                return last
            if g(idx) < g(idx - 1):
                return last
            if is_steep_up_pt(idx):
                last = idx
            idx += 1
        return max(n - 2, last)

    def cluster_borders(sda, sua_begin, sua_end):
        start_reach = g(sda[0])
        end_reach = g(min(sua_end + 1, n - 1))
        note("in_range_eq", abs(start_reach - end_reach), start_reach * chi)
        if abs(start_reach - end_reach) <= start_reach * chi:
            return (sda[0], sua_end)
        if start_reach > end_reach:
            start_idx = sda[0] + 1
            while start_idx <= sda[1] and g(start_idx) > end_reach:
                start_idx += 1
            return (start_idx - 1, sua_end)
        if start_reach < end_reach:
            end_idx = sua_end
            while end_idx >= sua_begin and g(end_idx) >= start_reach:
                end_idx -= 1
            return (sda[0], end_idx + 1)
        return (0, 0)

    def valid_combination(sda, sua_begin, sua_end):
        f = max(chi, steep_area_min_diff)
        if sda[2] > g(sua_end + 1) * (1 - f):
            return False
        sda_middle = sda[0] + (sda[1] - sda[0]) // 2
        sua_middle = sua_begin + (sua_end - sua_begin) // 2
        # size_t arithmetic, as the reference has it
        if (sua_middle - sda_middle) % (1 << 64) < (min_pts - 2) % (1 << 64):
            return False
        return True

    idx = 0
    while idx < n:
        reach_i = g(idx)
        if is_steep_down_pt(idx):
            if reach_i > mib:
                mib = reach_i
            filter_sdas()
            sda_end = get_sda_end(idx)
            if reach_i * (1.0 - steep_area_min_diff) < g(sda_end + 1):
                idx += 1
                continue
            sdas.append([idx, sda_end, 0.0])
            idx = sda_end
            if idx < n - 1:
                mib = g(idx + 1)
            idx += 1
            continue
        elif is_steep_up_pt(idx):
            filter_sdas()
            sua_end = get_sua_end(idx)
            if reach_i > g(sua_end + 1) * (1.0 - steep_area_min_diff):
                idx += 1
                continue
            for sda in sdas:
                if valid_combination(sda, idx, sua_end):
                    clusters.append(cluster_borders(sda, idx, sua_end))
            idx = sua_end
            if idx < n - 1:
                mib = g(idx + 1)
        else:
            if reach_i > mib:
                mib = reach_i
        idx += 1
    for b, e in clusters:
        assert 0 <= b <= e < n
    return clusters


def pairs_array(pairs):
    return np.asarray(pairs, np.int32).reshape(-1, 2)


# ------------------------------------------------------------------------------ shared test data
# chi 0.25 with powers of 3/4 and 2: g * (1 - chi) lands exactly on another member of the set, and
# |start - end| == start * chi (e.g. 4 and 3) occurs.
EQ_VALUES = np.array([-1.0, 4.0, 3.0, 2.25, 1.6875, 2.0, 1.5, 1.0, 0.75, 8.0, 6.0, 4.5], np.float64)
PARAMS = [(0.25, 2, 0.0), (0.25, 3, 0.3), (0.1, 4, 0.0)]


def random_plot(rng, n, values=EQ_VALUES):
    return values[rng.integers(0, len(values), n)].copy()


STAIR_CHI = 1e-4  # v - 1 <= v * (1 - 1e-4) for every v <= 10000: each unit step is steep


def staircase(n=8192, step=4):
    """A descending staircase in unit steps (first tread one point long): at STAIR_CHI all
    n / step steep-down areas stay alive and close at the final steep-up point, n / step clusters
    at one steep-up area."""
    k = (np.arange(n) + step - 1) // step
    return (float(n) - k).astype(np.float64)


def hostile_plots(rng, sizes):
    """Plots with NaN and infinities mixed in: the result is unspecified, the bounds are not."""
    vals = np.array([np.nan, np.inf, -np.inf, -1.0, 0.0, -0.0, 1.0, 0.75, 1e308, 5e-324, 4.0, 3.0])
    return [random_plot(rng, n, vals) for n in sizes]
