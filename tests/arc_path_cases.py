"""Event streams built to take the rare exits of the arc kernels (csrc/corner_arc.hip), each with
the facts that make it take its path, computed here on the CPU with numpy alone.

arc_kernel tests a (group of 32 slices, 14x14 tile) item on compact per-pixel value lists and
clamped 32-bit keys and hands everything else to arc_dense_kernel: windows too heavy for the lists,
wide groups, a surface value above the group's last timestamp, ties the clamp may have merged, and
more circle-3 survivors than its queue holds.  Noise streams reach almost none of these.  The
streams below do; tests/test_arc_path_cases.py asserts, on the oracle, that each one does what it
was built for, and tests/test_gpu_arc_paths.py runs them on the device and reads the path taken
from ecc_fast_detect_stats()["overflow_items"].

Every case is a dict: xy, t, W, H, S (slice_events), first (first_detect_slice), sae0 (initial
surface, int64[H*W]) and case-specific facts.  All cases use border_mode 0 and strictly increasing
timestamps.
"""
import numpy as np

# The constants of the device code that the predictions restate.
TILE = 14                 # corner_common.hpp:19   kTile
HALO = 4                  # corner_common.hpp:21   kHalo
WIN = TILE + 2 * HALO     # corner_common.hpp:22   kWin = 22
WIN_PIX = WIN * WIN       # corner_common.hpp:23   kWinPix = 484
GROUP = 32                # corner_common.hpp:18   kGroup
REC_VALS = 4              # corner_common.hpp:43   kRecVals: values a pixel record holds inline
V_MAX = (1 << 27) - 1     # corner_common.hpp:238  kVMax: the clamped keys' range
Q4_CAP = 1024             # corner_arc.hip:37      kQ4Cap: the circle-3 survivor queue
LIST_CAP = 4096 + WIN_PIX  # corner_arc.hip:412, :422, :592  kValCap + kWinPix = 4580: arc_kernel's `total` limit
DOUBLE_EXACT = 1 << 53    # corner_common.hpp:157  kDoubleExact
MARGIN = 4                # ecc_corner_cfg_default: the border, and the circles' reach

W, H = 56, 42             # 4 x 3 tiles
I64_MAX, I64_MIN = np.iinfo(np.int64).max, np.iinfo(np.int64).min


def pack(x, y):
    return (np.asarray(x).astype(np.uint32) | (np.asarray(y).astype(np.uint32) << 16)).astype(np.uint32)


def unpack(xy):
    return (xy & 0xffff).astype(np.int64), (xy >> 16).astype(np.int64)


def tiles_of(Wd, Hd):
    return (Wd + TILE - 1) // TILE, (Hd + TILE - 1) // TILE


def _groups(n, S):
    ns = (n + S - 1) // S
    return ns, (ns + GROUP - 1) // GROUP


def _per_tile(img, Wd, Hd, halo, fn):
    """fn over the part of img[Hd, Wd] inside each tile grown by `halo` -> [n_tiles]."""
    tx_n, ty_n = tiles_of(Wd, Hd)
    out = []
    for ty in range(ty_n):
        for tx in range(tx_n):
            y0, x0 = ty * TILE - halo, tx * TILE - halo
            out.append(fn(img[max(y0, 0): ty * TILE + TILE + halo, max(x0, 0): tx * TILE + TILE + halo]))
    return np.array(out)


def pair_counts(xy, S, Wd, Hd):
    """[n_groups, Hd, Wd]: in how many slices of the group the pixel has an event (the popcount of
    pair_build's slice mask).  Events outside the sensor count nowhere."""
    x, y = unpack(xy)
    ns, ng = _groups(len(xy), S)
    s = np.arange(len(xy)) // S
    inside = (x < Wd) & (y < Hd)
    key = np.unique((s[inside] * Hd + y[inside]) * Wd + x[inside])  # distinct (slice, pixel)
    cnt = np.zeros((ng, Hd * Wd), np.int64)
    np.add.at(cnt, (key // (Hd * Wd) // GROUP, key % (Hd * Wd)), 1)
    return cnt.reshape(ng, Hd, Wd)


def window_totals(xy, slice_events, Wd, Hd):
    """Per (group, tile): 484 plus the distinct (slice, pixel) pairs inside the tile's 22x22 window —
    arc_kernel's `total` (every window lane has a B_g slot, on the sensor or not)."""
    cnt = pair_counts(xy, slice_events, Wd, Hd)
    return np.stack([WIN_PIX + _per_tile(c, Wd, Hd, HALO, np.sum) for c in cnt])


def own_events(xy, slice_events, Wd, Hd):
    """Per (group, tile): the tile holds an event of the group (arc_kernel's any_own)."""
    cnt = pair_counts(xy, slice_events, Wd, Hd)
    return np.stack([_per_tile(c, Wd, Hd, 0, np.sum) > 0 for c in cnt])


def per_item(flags, xy, slice_events, Wd, Hd):
    """The oracle's corners per (group, tile): distinct flagged (slice, pixel) pairs, the unit the
    arc kernels test and queue."""
    f = np.asarray(flags) != 0
    ns, ng = _groups(len(xy), slice_events)
    tx_n, ty_n = tiles_of(Wd, Hd)
    out = np.zeros((ng, tx_n * ty_n), np.int64)
    x, y = unpack(xy)
    s = np.arange(len(xy)) // slice_events
    key = np.unique((s[f] * Hd + y[f]) * Wd + x[f])
    q = key % (Hd * Wd)
    np.add.at(out, (key // (Hd * Wd) // GROUP, (q // Wd // TILE) * tx_n + (q % Wd) // TILE), 1)
    return out


def group_facts(t, S):
    """Per group what group_ref (corner_common.hpp:246-257) derives: first index, t_first, t_last,
    beyond (a timestamp at or past 2^53 in magnitude) and narrow (span below 2^27 - 1, not beyond).
    Python ints: no overflow."""
    n = len(t)
    out = []
    for lo in range(0, n, GROUP * S):
        hi = min(n, lo + GROUP * S)
        t_first, t_last = int(t[lo]), int(t[hi - 1])
        beyond = t_last >= DOUBLE_EXACT or t_first <= -DOUBLE_EXACT
        out.append(dict(first=lo, end=hi, t_first=t_first, t_last=t_last, beyond=beyond,
                        narrow=(not beyond) and t_last - t_first < V_MAX))
    return out


def surfaces_before(xy, t, S, Wd, Hd, sae0):
    """B_g: the surface before each group, [n_groups, Hd, Wd] (last writer in stream order)."""
    x, y = unpack(xy)
    sae = np.zeros(Wd * Hd, np.int64) if sae0 is None else np.array(sae0, np.int64).ravel().copy()
    out = []
    for lo in range(0, len(xy), GROUP * S):
        out.append(sae.reshape(Hd, Wd).copy())
        hi = min(len(xy), lo + GROUP * S)
        m = (x[lo:hi] < Wd) & (y[lo:hi] < Hd)
        q = (y[lo:hi] * Wd + x[lo:hi])[m]
        last = np.full(Wd * Hd, -1, np.int64)
        np.maximum.at(last, q, np.arange(lo, hi)[m])
        hit = last >= 0
        sae[hit] = t[last[hit]]
    return np.stack(out)


def future_items(c):
    """Per (group, tile): the tile's window holds a surface value above the group's last timestamp
    (arc_select.hpp: arc_clamp_value / arc_clamp_rel raise exact_only: the item goes to the exact tests)."""
    B = surfaces_before(c["xy"], c["t"], c["S"], c["W"], c["H"], c["sae0"])
    gf = group_facts(c["t"], c["S"])
    return np.stack([_per_tile(B[g] > gf[g]["t_last"], c["W"], c["H"], HALO, np.any) for g in range(len(gf))])


def circle3_survivors(c):
    """Per (group, tile): the distinct tested (slice, pixel) pairs that pass circle 3 — what both
    arc kernels queue for circle 4.  The values compare as doubles, like the reference's scan
    (exact below 2^53); the count form of the arc test (arc_select.hpp: arc_streak)."""
    xy, t, S, Wd, Hd = c["xy"], c["t"], c["S"], c["W"], c["H"]
    x, y = unpack(xy)
    ns, ng = _groups(len(xy), S)
    tx_n, ty_n = tiles_of(Wd, Hd)
    out = np.zeros((ng, tx_n * ty_n), np.int64)
    sae = (np.zeros(Wd * Hd, np.int64) if c["sae0"] is None else np.array(c["sae0"], np.int64)).reshape(Hd, Wd)
    dy, dx = np.array(C3).T
    for s in range(ns):
        sl = slice(s * S, min(len(xy), (s + 1) * S))
        m = (x[sl] < Wd) & (y[sl] < Hd)
        sae[y[sl][m], x[sl][m]] = t[sl][m]  # stream order: the last writer stays
        if s < c["first"]:
            continue
        q = np.unique(y[sl][m] * Wd + x[sl][m])
        qx, qy = q % Wd, q // Wd
        keep = (qx >= MARGIN) & (qx < Wd - MARGIN) & (qy >= MARGIN) & (qy < Hd - MARGIN)
        qx, qy = qx[keep], qy[keep]
        v = sae[qy[:, None] + dy[None, :], qx[:, None] + dx[None, :]].astype(np.float64)
        cnt = (v[:, None, :] > v[:, :, None]).sum(2)  # cnt[e, j] = values of the circle above v[e, j]
        ok = np.zeros(len(qx), bool)
        for k in range(3, 7):
            top = cnt < k
            ok |= (top.sum(1) == k) & ((top & ~np.roll(top, 1, axis=1)).sum(1) == 1)
        np.add.at(out, (s // GROUP, (qy[ok] // TILE) * tx_n + qx[ok] // TILE), 1)
    return out


def predicted_dense_items(c):
    """The (group, tile) items that the code's uniform exits MUST hand to arc_dense_kernel, as a
    boolean [n_groups, n_tiles]: items with an event in their tile, in a group that is tested, which
    are wide, or heavier than the compact lists, or hold a value above t_last, or have more
    circle-3 survivors than the queue.  A lower bound of overflow_items: ties that the clamp may
    have merged send items there as well (mixed_clamp); where a case rules those out, the count."""
    xy, S, Wd, Hd = c["xy"], c["S"], c["W"], c["H"]
    gf = group_facts(c["t"], S)
    wide = np.array([not g["narrow"] for g in gf])[:, None]
    must = wide | (window_totals(xy, S, Wd, Hd) > LIST_CAP) | future_items(c) | (circle3_survivors(c) > Q4_CAP)
    tested = (np.arange(len(gf)) >= (c["first"] >> 5))[:, None]  # arc_item / arc_dense_item: grp < first_detect >> 5
    return must & own_events(xy, S, Wd, Hd) & tested


def clamped_values(c):
    """Per group: how many surface values before the group lie at or below L = t_last - (2^27 - 1)
    (they share key 0) and how many distinct values those are (more than one: "mixed")."""
    B = surfaces_before(c["xy"], c["t"], c["S"], c["W"], c["H"], c["sae0"])
    out = []
    for g, f in enumerate(group_facts(c["t"], c["S"])):
        low = B[g][B[g] <= f["t_last"] - V_MAX]
        out.append((int(low.size), int(np.unique(low).size)))
    return out


def near(xy, px, py, r=HALO):
    """Events within r px (Chebyshev) of pixel (px, py)."""
    x, y = unpack(xy)
    return (np.abs(x - px) <= r) & (np.abs(y - py) <= r)


def reads(xy, px, py):
    """Events whose circles contain pixel (px, py): the tests that read it (border events are not tested)."""
    x, y = unpack(xy)
    m = np.zeros(len(xy), bool)
    for dy, dx in C3 + C4:
        m |= (x + dx == px) & (y + dy == py)
    return m & (x >= MARGIN) & (x < W - MARGIN) & (y >= MARGIN) & (y < H - MARGIN)


C3 = [(0, 3), (1, 3), (2, 2), (3, 1), (3, 0), (3, -1), (2, -2), (1, -3), (0, -3), (-1, -3), (-2, -2), (-3, -1),
      (-3, 0), (-3, 1), (-2, 2), (-1, 3)]
C4 = [(0, 4), (1, 4), (2, 3), (3, 2), (4, 1), (4, 0), (4, -1), (3, -2), (2, -3), (1, -4), (0, -4), (-1, -4),
      (-2, -3), (-3, -2), (-4, -1), (-4, 0), (-4, 1), (-3, 2), (-2, 3), (-1, 4)]


# ------------------------------------------------------------------------------------ 1, 2: queue
RASTER_S = W * H  # 2352
RASTER_SLICES = 40


def raster_slice(rng, swap=0.01):
    """One event per pixel in raster order; `swap` of the positions trade pixels among themselves."""
    q = np.arange(W * H)
    k = rng.choice(W * H, int(round(swap * W * H)), replace=False)
    q[k] = q[rng.permutation(k)]
    return pack(q % W, q // W)


def queue_full(heavy=False, seed=3):
    """Every fourth slice (every slice when heavy) a raster scan of the sensor with t rising in
    raster order — a plane t = y W + x passes both circles at every interior pixel — the rest S
    events at the off-sensor pixel (W + 1, 0).  The interior tiles hold more than 1024 corners per
    group; light windows (484 + 8 * 484 values at most) stay with arc_kernel until its queue
    overflows, heavy ones (484 * 33) go straight to the dense kernel, whose queue overflows too."""
    rng = np.random.default_rng(seed)
    xy = np.empty(RASTER_SLICES * RASTER_S, np.uint32)
    for s in range(RASTER_SLICES):
        sl = slice(s * RASTER_S, (s + 1) * RASTER_S)
        xy[sl] = raster_slice(rng) if (heavy or s % 4 == 0) else pack(W + 1, 0)
    t = np.arange(1, len(xy) + 1, dtype=np.int64)
    return dict(name="queue_full_heavy" if heavy else "queue_full", xy=xy, t=t, W=W, H=H, S=RASTER_S, first=0,
                sae0=None)


# ------------------------------------------------------------------------------------ noise, planted tests
# Uniform noise alone makes almost no corners (a handful in 30 000 events), so a wrong value would
# rarely change a flag.  The cases therefore PLANT tests whose outcome is known and hangs on the
# values in question: a run of events at a slice's tail that writes the pixels of both circles
# around a centre — first those outside a chosen arc of each circle, then the arcs — and then the
# centre.  Tests see the surface after the whole slice, and nothing follows the tail, so the arcs
# are the newest values of their circles: a corner.  Leaving pixels unwritten makes the outcome
# depend on what the surface held there before.
NOISE_S = 448
HEAD = 64  # a slice's first positions (where deep_runs puts its hot events); planted tests stay behind them


def circles(cx, cy):
    return [(cx + dx, cy + dy) for dy, dx in C3], [(cx + dx, cy + dy) for dy, dx in C4]


def arcs(cx, cy, a3, a4):
    """(arc pixels, rest pixels) of both circles for arcs a3 = (start, length) on circle 3, a4 on circle 4."""
    c3, c4 = circles(cx, cy)
    arc = [c3[(a3[0] + k) % 16] for k in range(a3[1])] + [c4[(a4[0] + k) % 20] for k in range(a4[1])]
    return arc, [p for p in c3 + c4 if p not in arc]


def interior(cx, cy):
    return MARGIN <= cx < W - MARGIN and MARGIN <= cy < H - MARGIN


class Stream:
    """S uniform-random events per slice; no noise event at the pixels `avoid`, nor, in slices
    0 .. last, at the circles and centre of a `protect` entry (cx, cy, last)."""

    def __init__(self, n_slices, seed, S=NOISE_S, avoid=(), protect=()):
        self.S, self.rng = S, np.random.default_rng(seed)
        n = n_slices * S
        self.x, self.y = self.rng.integers(0, W, n), self.rng.integers(0, H, n)
        banned = np.zeros((n_slices, H, W), bool)
        for px, py in avoid:
            banned[:, py, px] = True
        for cx, cy, last in protect:
            c3, c4 = circles(cx, cy)
            for px, py in c3 + c4 + [(cx, cy)]:
                banned[:last + 1, py, px] = True
        s = np.arange(n) // S
        while True:
            bad = banned[s, self.y, self.x]
            if not bad.any():
                break
            self.x[bad], self.y[bad] = self.rng.integers(0, W, bad.sum()), self.rng.integers(0, H, bad.sum())
        self.cursor, self.foot = {}, {}

    def plant(self, s, cx, cy, a3, a4, write=("rest", "arc"), skip=()):
        """Plants a test at the tail of slice s and returns the index of its centre event.  write:
        which of the circles' pixels get an event ("rest": outside the arcs, "arc"); skip: pixels
        that get none either way.  The planted tests of one slice must not share pixels."""
        assert interior(cx, cy)
        arc, rest = arcs(cx, cy, a3, a4)
        foot = set(arc + rest + [(cx, cy)])
        assert not (foot & self.foot.setdefault(s, set())), (s, cx, cy)
        self.foot[s] |= foot
        ev = [p for p in rest if "rest" in write and p not in skip] + \
             [p for p in arc if "arc" in write and p not in skip] + [(cx, cy)]
        hi = self.cursor.get(s, self.S)
        lo = hi - len(ev)
        assert lo >= HEAD
        self.cursor[s] = lo
        for k, (px, py) in enumerate(ev):
            self.x[s * self.S + lo + k], self.y[s * self.S + lo + k] = px, py
        return s * self.S + hi - 1

    def free(self, s, cx, cy):
        """Slice s has room for a test at (cx, cy) that shares no pixel with its other planted tests."""
        c3, c4 = circles(cx, cy)
        return self.cursor.get(s, self.S) - 37 >= HEAD and not (set(c3 + c4 + [(cx, cy)]) & self.foot.get(s, set()))

    def xy(self):
        return pack(self.x, self.y)


EXTRA_CENTRES = tuple((10 + 12 * i, 9 + 11 * j) for j in range(3) for i in range(4))  # footprints 9 x 9: disjoint


def plant_extra(st, n_slices, per_slice):
    """`per_slice` fully written tests in every slice from 1 on, at centres that rotate through a
    grid, where the slice has room: corners whatever the surface held (the reference pins want
    more than a hundred of them)."""
    out = []
    for s in range(1, n_slices):
        for k in range(per_slice):
            cx, cy = EXTRA_CENTRES[(per_slice * s + k) % len(EXTRA_CENTRES)]
            if st.free(s, cx, cy):
                out.append(st.plant(s, cx, cy, A3, A4))
    return out


def rising(n, t0=1000, seed=0):
    """Strictly increasing timestamps, 1-3 ticks apart."""
    return t0 + np.cumsum(np.random.default_rng(seed).integers(1, 4, n)).astype(np.int64)


# ------------------------------------------------------------------------------------ 3: deep runs
DEEP_P = (1, 3, 4, 5, 6, 7, 8, 11, 12, 19, 20, 23, 24, 31, 32)
# (x, y, p): tile interiors, the four-tile seam (13, 13) / (14, 14) (staged by four items), column 3
# and row 3 (border pixels: never tested, read by the tests at (4..7, y) and (x, 4..7)), seams of
# two items, and the corner pixel (0, 0), which no test reads (staging only).
DEEP_HOT = ((6, 7, 1), (20, 6, 3), (34, 8, 4), (48, 7, 5), (7, 21, 6), (21, 20, 7), (35, 22, 8), (49, 21, 11),
            (6, 35, 12), (22, 34, 19), (13, 13, 32), (14, 14, 20), (27, 28, 23), (28, 27, 24), (3, 20, 31),
            (3, 30, 5), (30, 3, 32), (44, 3, 20), (0, 0, 24), (41, 14, 31), (42, 27, 12), (36, 35, 23), (50, 33, 19))
DEEP_SLICES = 70  # two whole groups and a ragged third of 6 slices


def _centre_for(hot, others):
    """A non-border centre with `hot` on one of its circles and no other hot pixel on either (nor
    at the centre): (cx, cy, ring, index of hot on the ring)."""
    for ring, circ in ((3, C3), (4, C4)):
        for i, (dy, dx) in enumerate(circ):
            cx, cy = hot[0] - dx, hot[1] - dy
            if not interior(cx, cy):
                continue
            c3, c4 = circles(cx, cy)
            if not (set(c3 + c4 + [(cx, cy)]) & others):
                return cx, cy, ring, i
    raise AssertionError(hot)


def deep_runs(seed=11):
    """Noise with hot pixels that fire in exactly p slices of group 0 and of group 1, p from 1 to
    32: a record's four inline values (p <= 4), the prefetched overflow line (p <= 7), the first
    trip of four lines (p <= 19) and the second (p >= 20: the k + i < p edges at 20, 23, 24, 31, 32
    and the clamp to the run's last line).  Planted tests read each hot pixel's run: in its first
    and its last firing slice of a group with the hot pixel inside the arc (a value read too low
    loses the corner), and in a later slice where it does not fire with the hot pixel outside the
    arc and unwritten (a value read too high loses it).  Windows stay within the compact lists and
    nothing else sends an item away: arc_kernel decides every item itself."""
    pix = [(hx, hy) for hx, hy, _ in DEEP_HOT]
    st = Stream(DEEP_SLICES, seed, avoid=pix)
    rng = st.rng
    fired, head = {}, {}
    for hx, hy, p in DEEP_HOT:
        for g in (0, 1):
            sl = np.sort(rng.choice(GROUP, p, replace=False)) + g * GROUP
            fired[(hx, hy, g)] = sl
            for s in sl:  # the hot events, among a slice's first HEAD positions
                used = head.setdefault(int(s), set())
                k = int(rng.integers(0, HEAD))
                while k in used:
                    k = int(rng.integers(0, HEAD))
                used.add(k)
                st.x[s * NOISE_S + k], st.y[s * NOISE_S + k] = hx, hy
    probes = []  # (event index, hot pixel, group, "in" / "out")
    for hx, hy, p in DEEP_HOT:
        if (hx, hy) == (0, 0):
            continue
        cx, cy, ring, i = _centre_for((hx, hy), set(pix) - {(hx, hy)})
        a_in = ((i - 1) % 16, 4) if ring == 3 else (0, 4), ((i - 2) % 20, 5) if ring == 4 else (0, 5)
        a_out = ((i + 4) % 16, 4) if ring == 3 else (0, 4), ((i + 6) % 20, 5) if ring == 4 else (0, 5)
        for g in (0, 1):
            sl = [int(s) for s in fired[(hx, hy, g)]]
            ok = [s for s in sl if st.free(s, cx, cy)]  # its first and last firing slice that have room
            for s in sorted({ok[0], ok[-1]}):
                probes.append((st.plant(s, cx, cy, *a_in), (hx, hy), g, "in"))
            quiet = [s for s in range(sl[0] + 1, (g + 1) * GROUP) if s not in sl and st.free(s, cx, cy)]
            if quiet:  # after the last firing where there is such a slice, else between firings
                probes.append((st.plant(quiet[-1], cx, cy, *a_out, skip=[(hx, hy)]), (hx, hy), g, "out"))
    xy = st.xy()
    return dict(name="deep_runs", xy=xy, t=rising(len(xy)), W=W, H=H, S=NOISE_S, first=0, sae0=None, hot=DEEP_HOT,
                fired=fired, probes=probes)


# ------------------------------------------------------------------------------------ 4: future SAE
FUTURE_SLICES = 40
# Centres of the tests planted in slice 0 on the INITIAL surface: the first three lie in ONE item's
# window each (tiles 0, 3 and 11: their circles stay more than 4 px from the neighbouring tiles), so
# that item sees no other planted value; the others sit where windows overlap.
ALONE = ((5, 5), (50, 5), (50, 36))
SHARED = ((27, 6), (27, 16), (27, 26), (27, 36), (9, 22))
A3, A4 = (14, 4), (17, 6)  # the planted arcs: 4 pixels of circle 3, 6 of circle 4


def _surface_test(sae0, cx, cy, arc_vals, rest_vals):
    """Sets the surface on both circles of (cx, cy): the arcs' pixels cycle through arc_vals, the rest through rest_vals."""
    arc, rest = arcs(cx, cy, A3, A4)
    for k, (px, py) in enumerate(arc):
        sae0[py * W + px] = arc_vals[k % len(arc_vals)]
    for k, (px, py) in enumerate(rest):
        sae0[py * W + px] = rest_vals[k % len(rest_vals)]
    return arc + rest


def future_sae(variant, extra=0):
    """Noise over an initial surface that holds values above group 0's last timestamp (a .. c) or
    at the bottom of the int64 range (d).  In slice 0 each centre of ALONE + SHARED gets one event
    and no other event touches its circles, so its test reads the initial surface alone:
      a, b27, b40: 30 % of the pixels hold t_last + 1 .. + 1000, + 2^27 .., + 2^40 ..; around the
         centres the arcs hold such values and the rest 0 (a corner; none once the values are zeroed).
      c: 2^62, INT64_MAX - 1 and INT64_MAX.  ALONE[0]'s arcs hold INT64_MAX, ALONE[1]'s INT64_MAX - 1,
         ALONE[2]'s 2^62 over a rest of 0: corners.  SHARED: arcs of INT64_MAX over a rest that
         holds INT64_MAX - 1 (equal as doubles: no corner, where int64 order would find one), arcs
         that mix all three, and 0-arcs under a rest of extremes.
      d: INT64_MIN and INT64_MIN + 1.  Arcs of 0 over a rest of both: corners, which only the old
         values' order decides (zeroed, everything ties).  Arcs of INT64_MIN + 1 over a rest of
         INT64_MIN: equal as doubles, no corner."""
    centres = ALONE + SHARED
    st = Stream(FUTURE_SLICES, 21, protect=[(cx, cy, 0) for cx, cy in centres])
    rng = np.random.default_rng(22)
    probes = [st.plant(0, cx, cy, A3, A4, write=()) for cx, cy in centres]
    full = plant_extra(st, FUTURE_SLICES, extra)
    xy = st.xy()
    t = rising(len(xy), seed=21)
    t_last0 = int(t[GROUP * NOISE_S - 1])
    sae0 = np.zeros(W * H, np.int64)
    c = dict(name=f"future_sae_{variant}", xy=xy, t=t, W=W, H=H, S=NOISE_S, first=0, probes=probes, full=full)
    planted = []
    if variant in ("a", "b27", "b40"):
        base = t_last0 + {"a": 1, "b27": 1 << 27, "b40": 1 << 40}[variant]
        some = rng.random(W * H) < 0.3
        sae0[some] = base + rng.integers(0, 1000, some.sum())
        for k, (cx, cy) in enumerate(centres):
            vals = [base + int(v) for v in rng.choice(1000, 10, replace=False)]
            if k == 0:
                vals[0] = base  # the smallest value of the kind (a: t_last + 1, the first past the keys' range)
            planted += _surface_test(sae0, cx, cy, vals, [0])
    elif variant == "c":
        M = I64_MAX
        specs = [([M], [0]), ([M - 1], [0]), ([1 << 62], [0]),
                 ([M], [0, M - 1]), ([M, M - 1, 1 << 62], [0]), ([0], [M, M - 1, 1 << 62]), ([M - 1], [1 << 62, 0]),
                 ([M], [1 << 62])]
        for (cx, cy), (av, rv) in zip(centres, specs):
            planted += _surface_test(sae0, cx, cy, av, rv)
    elif variant == "d":
        m = I64_MIN
        specs = [([0], [m]), ([0], [m + 1]), ([0], [m, m + 1]),
                 ([m + 1], [m]), ([0, m + 1], [m]), ([m], [m + 1]), ([0], [m, 0]), ([m + 1, m], [m])]
        for (cx, cy), (av, rv) in zip(centres, specs):
            planted += _surface_test(sae0, cx, cy, av, rv)
    else:
        raise KeyError(variant)
    c["sae0"] = sae0
    c["planted"] = sorted(set(planted))  # the pixels whose initial value the probes' tests read
    return c


# ------------------------------------------------------------------------------------ 5: negative time
NEG_VARIANTS = ("small", "cross_zero", "m2p40", "cross_m2p53", "i64_min", "i64_max")
NEG_ZERO_ARC = ((8, 8), (26, 18), (47, 33))   # slice 0: the rest is written, the arcs keep the surface's 0
NEG_ZERO_REST = ((21, 9), (40, 20), (12, 31))  # slice 0: the arcs are written, the rest keeps 0
NEG_FULL = ((15, 15, 5), (30, 25, 5), (44, 10, 12), (20, 30, 33), (40, 30, 36))  # (cx, cy, slice): all written


def negative_time(variant, extra=0):
    """Noise over a ZERO surface with negative timestamps in stream order: 0 is newer than every
    negative timestamp, so every window of a group that ends below zero holds a value above t_last.
    Planted in slice 0: tests whose arcs keep the surface's 0 under a written rest (a corner exactly
    when the slice's timestamps are negative) and tests with written arcs over a rest of 0 (a
    corner exactly when they are positive); in later slices, tests with every pixel written."""
    ns = 70 if variant == "cross_m2p53" else 40
    st = Stream(ns, 31, protect=[(cx, cy, 0) for cx, cy in NEG_ZERO_ARC + NEG_ZERO_REST])
    zero_arc = [st.plant(0, cx, cy, A3, A4, write=("rest",)) for cx, cy in NEG_ZERO_ARC]
    zero_rest = [st.plant(0, cx, cy, A3, A4, write=("arc",)) for cx, cy in NEG_ZERO_REST]
    full = [st.plant(s, cx, cy, A3, A4) for cx, cy, s in NEG_FULL]
    if variant == "cross_m2p53":
        full.append(st.plant(66, 28, 20, A3, A4))  # in the narrow, negative third group
    full += plant_extra(st, ns, extra)
    xy = st.xy()
    n = len(xy)
    i = np.arange(n, dtype=np.int64)
    if variant == "small":          # [-40000, -1]
        t = -1 - 2 * (n - 1 - i)
    elif variant == "cross_zero":   # crosses zero inside slice 12 (inside group 0), in the middle of a planted test
        t = i - (12 * NOISE_S + NOISE_S - 20)
    elif variant == "m2p40":
        t = -(1 << 40) + i
    elif variant == "cross_m2p53":  # group 1 crosses -2^53 upward; group 2 (ragged) is narrow and negative
        t = -(1 << 53) - (33 * NOISE_S + 100) + i
    elif variant == "i64_min":
        t = I64_MIN + i
    elif variant == "i64_max":
        t = I64_MAX - n + i
    else:
        raise KeyError(variant)
    return dict(name=f"negative_time_{variant}", xy=xy, t=t.astype(np.int64), W=W, H=H, S=NOISE_S, first=0,
                sae0=None, zero_arc=zero_arc, zero_rest=zero_rest, full=full)


# ------------------------------------------------------------------------------------ 6: mixed clamp
MIXED_S = 128
MIXED_SLICES = 40
MIXED_CENTRES = ((8, 8), (26, 18), (47, 33), (21, 9), (40, 20), (12, 31), (33, 33), (48, 8))


def mixed_clamp(all_equal=False):
    """A narrow group (t = 2^30 + 200 i) over a surface whose values all lie at or below
    L = t_last - (2^27 - 1): 70 % of the pixels uniform in [t_last - 2^40, t_last - 2^27 - 1], the
    rest the single value t_last - 2^28.  The clamp merges them all into key 0, and the sparse
    events (128 a slice) leave most circles with fewer than seven unclamped values.  Tests planted
    in slice 0 read circles no event has touched: arcs that hold the largest old values over a rest
    of smaller ones — corners that only the old values' true order decides.  all_equal: the same
    stream over the single old value everywhere (no such corner)."""
    st = Stream(MIXED_SLICES, 41, S=MIXED_S, protect=[(cx, cy, 0) for cx, cy in MIXED_CENTRES[:4]] +
                [(cx, cy, 1) for cx, cy in MIXED_CENTRES[4:]])
    probes = [st.plant(0, cx, cy, A3, A4, write=()) for cx, cy in MIXED_CENTRES[:4]]
    probes += [st.plant(1, cx, cy, A3, A4, write=()) for cx, cy in MIXED_CENTRES[4:]]
    xy = st.xy()
    t = (1 << 30) + 200 * np.arange(len(xy), dtype=np.int64)
    rng = np.random.default_rng(42)
    t_last0 = int(t[GROUP * MIXED_S - 1])
    sae0 = np.full(W * H, t_last0 - (1 << 28), np.int64)
    if not all_equal:
        old = rng.random(W * H) < 0.7
        sae0[old] = rng.integers(t_last0 - (1 << 40), t_last0 - (1 << 27), old.sum())  # the high end is exclusive
        top = t_last0 - (1 << 27) - 1
        for k, (cx, cy) in enumerate(MIXED_CENTRES):
            arc, rest = arcs(cx, cy, A3, A4)
            for j, (px, py) in enumerate(arc):   # the arcs: the top of the old range, distinct
                sae0[py * W + px] = top - j - 16 * k
            for px, py in rest:                  # the rest: anything at least 2^20 lower (70 % random, 30 % the single value)
                sae0[py * W + px] = min(int(sae0[py * W + px]), top - (1 << 20) - int(rng.integers(0, 1 << 30)))
    return dict(name="mixed_clamp", xy=xy, t=t, W=W, H=H, S=MIXED_S, first=0, sae0=sae0, probes=probes)


# ------------------------------------------------------------------------------------ the list
def _make(name):
    if name == "queue_full":
        return queue_full()
    if name == "queue_full_heavy":
        return queue_full(heavy=True)
    if name == "deep_runs":
        return deep_runs()
    if name == "mixed_clamp":
        return mixed_clamp()
    if name.startswith("future_sae_"):
        return future_sae(name[len("future_sae_"):])
    if name.startswith("negative_time_"):
        return negative_time(name[len("negative_time_"):])
    raise KeyError(name)


CASES = ("queue_full", "queue_full_heavy", "deep_runs", "future_sae_a", "future_sae_b27", "future_sae_b40",
         "future_sae_c", "future_sae_d") + tuple(f"negative_time_{v}" for v in NEG_VARIANTS) + ("mixed_clamp",)
_cache = {}


def case(name):
    if name not in _cache:
        _cache[name] = _make(name)
    return _cache[name]


_oracle = {}


def run_oracle(orc, c, sae0="own"):
    return orc.fast_detect(c["xy"], c["t"], c["W"], c["H"], slice_events=c["S"], first_detect=c["first"],
                           sae=c["sae0"] if isinstance(sae0, str) else sae0)


def oracle(orc, name):
    """orc.fast_detect of the case -> (flags, final surface), computed once and shared (read-only)."""
    if name not in _oracle:
        f, s = run_oracle(orc, case(name))
        f.setflags(write=False)
        s.setflags(write=False)
        _oracle[name] = (f, s)
    return _oracle[name]


_predicted = {}


def predicted(name):
    """predicted_dense_items of the case, computed once."""
    if name not in _predicted:
        _predicted[name] = predicted_dense_items(case(name))
    return _predicted[name]
