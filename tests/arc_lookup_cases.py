"""Event streams for the edges of arc_kernel's window lookups (csrc/corner_arc.hip: the pixel
record's byte offset, arc_value_byte, and the circle reads off one base address), built from the
pieces of tests/arc_path_cases.py (the 56 x 42 sensor of 4 x 3 tiles, its noise Stream, its planted
tests).  tests/test_arc_lookup_cases.py asserts on the CPU that every stream does what it was
built for; tests/test_gpu_arc_lookup_edges.py runs them on the device.

A lookup reads the record of a circle pixel (one 8-B read at a displacement from the window pixel
four rows up and four columns left of the task's) and then one value, the word at
offset + 4 * popcount(mask & slices 0 .. j).  What can go wrong is a wrong record (displacement)
or a wrong word (offset, popcount), so every case PLANTS tests whose outcome hangs on one such
read, as arc_path_cases.deep_runs does:
  "in":  in a slice where the hot pixel fires, the test's arc holds it (written again at the
         slice's tail): read one word too low, the pixel's older value or its B_g, the corner is lost;
  "out": in a slice where it does not fire, the hot pixel lies outside the arc, unwritten: read
         too high, a later slice's value, it becomes the newest of the circle and the corner is lost.

The cases:
  cap_exact  tile 5's window (all on the sensor) holds exactly kValCap distinct (slice, pixel)
             pairs in group 0: arc_kernel's total is kValCap + kWinPix, the compact list's
             capacity, and the item stays.  The window's last three pixels are untouched and
             the pixel before them, (28, 31), is the last that any circle reaches (the window's
             corner pixels lie on no circle): its newest value, read by the probe planted at
             (27, 27) in slice 31, is the HIGHEST WORD OF THE LIST THAT ANY TEST CAN READ
             (word capacity - 4; the three B_g slots after it are staged and never read), and the
             last pixel's record holds the largest offset the kernel can produce.
  cap_over   the same construction with one more pair in that window: total capacity + 1, the item goes
             to arc_dense_kernel.
  slots      light windows.  Hot pixels at the smallest and the largest displacement of the one
             base ((13, 10) for the task at tile 5's first pixel (14, 14), word 3 of the window;
             (28, 31) for the task at its last pixel (27, 27), word 480), at the sensor's edge in
             clipped windows ((0, 4) in tile 0, (55, 37) in tile 11), firing in slices that
             include 0 and 31 (the mask's lowest and highest bit decide), one of them in all 32
             slices (33 words) right before a pixel no event touches; fully written tests at the
             own tile's four corners and four edge midpoints of tile 5 and at the corners of the
             testable area of the border tiles 0, 3, 8 and 11.
"""
import numpy as np

import arc_path_cases as ap

W, H, S = ap.W, ap.H, ap.NOISE_S
TILE5 = (14, 14)                      # origin of tile 5, the interior tile under test
WIN5 = (TILE5[0] - ap.HALO, TILE5[1] - ap.HALO)  # its window's first pixel (10, 10); the window ends at (31, 31)
FIRST_READ = (13, 10)                 # window word 3: the lowest any circle reaches (task (14, 14), circle 4 (-4, -1))
LAST_READ = (28, 31)                  # window word 480: the highest any circle reaches (task (27, 27), circle 4 (4, 1))
UNREAD_TAIL = ((29, 31), (30, 31), (31, 31))  # window words 481 .. 483: on no circle of an own-tile task


def window_word(px, py, win=WIN5):
    return (py - win[1]) * ap.WIN + (px - win[0])


def ring_index(hot, centre):
    """(ring, index on the ring) of pixel `hot` on the circles of `centre`."""
    d = (hot[1] - centre[1], hot[0] - centre[0])
    return (3, ap.C3.index(d)) if d in ap.C3 else (4, ap.C4.index(d))


def _arcs_for(hot, centre):
    ring, i = ring_index(hot, centre)
    # "in": the hot pixel is the arc's last (its neighbour on the ring may be one that stays unwritten)
    a_in = ((i - 3) % 16, 4) if ring == 3 else (0, 4), ((i - 4) % 20, 5) if ring == 4 else (0, 5)
    a_out = ((i + 4) % 16, 4) if ring == 3 else (0, 4), ((i + 6) % 20, 5) if ring == 4 else (0, 5)
    return a_in, a_out


def _fire(st, hots):
    """The hot events: pixel (hx, hy) fires in the slices `fired`, among each slice's first HEAD positions."""
    head = {}
    for (hx, hy), _, fired in hots:
        for s in fired:
            used = head.setdefault(s, set())
            k = int(st.rng.integers(0, ap.HEAD))
            while k in used:
                k = int(st.rng.integers(0, ap.HEAD))
            used.add(k)
            st.x[s * st.S + k], st.y[s * st.S + k] = hx, hy


def _probe(st, hots, n_slices, quiet_for=(), never=()):
    """Plants the "in" probes (first and last firing slice) and one "out" probe (a quiet slice between
    two firings) of every hot pixel, and an "out" probe of every untouched pixel of quiet_for
    ((pixel, centre, slice) triples); no planted test writes a pixel of `never`.
    -> [(event index, pixel, slice, kind)]"""
    probes = []
    for hot, centre, fired in hots:
        a_in, a_out = _arcs_for(hot, centre)
        for s in sorted({fired[0], fired[-1]}):
            assert st.free(s, *centre), (hot, s)
            probes.append((st.plant(s, *centre, *a_in, skip=list(never)), hot, s, "in"))
        quiet = [s for s in range(fired[0] + 1, fired[-1]) if s not in fired and st.free(s, *centre)]  # between firings
        if quiet:
            probes.append((st.plant(quiet[-1], *centre, *a_out, skip=[hot] + list(never)), hot, quiet[-1], "out"))
    for pix, centre, s in quiet_for:
        _, a_out = _arcs_for(pix, centre)
        assert st.free(s, *centre)
        probes.append((st.plant(s, *centre, *a_out, skip=[pix] + list(never)), pix, s, "out"))
    return probes


def _window_pixels():
    return [(WIN5[0] + i, WIN5[1] + j) for j in range(ap.WIN) for i in range(ap.WIN)]


CAP_SLICES = 36  # group 0 whole, a ragged group 1 of four slices
CAP_HOT = ((LAST_READ, (27, 27), (3, 12, 31)),)


def capacity(extra=0, seed=51):
    """cap_exact (extra = 0) and cap_over (extra = 1): see the module's text.  Noise stays out of
    tile 5's window; its pairs of group 0 are the hot pixel's, the planted tests' and a fill of
    distinct window pixels per slice (placed ahead of the slice's planted tail, away from the
    tests planted in that slice) that brings them to exactly kValCap + extra."""
    win = _window_pixels()
    st = ap.Stream(CAP_SLICES, seed, avoid=win)
    _fire(st, CAP_HOT)
    probes = _probe(st, CAP_HOT, CAP_SLICES)
    have = np.zeros((ap.GROUP, H, W), bool)  # (slice, pixel) pairs of group 0 so far
    n0 = ap.GROUP * S
    have[np.arange(n0) // S, st.y[:n0], st.x[:n0]] = (st.x[:n0] < W) & (st.y[:n0] < H)
    inwin = np.zeros((H, W), bool)
    inwin[WIN5[1]:WIN5[1] + ap.WIN, WIN5[0]:WIN5[0] + ap.WIN] = True
    need = (ap.LIST_CAP - ap.WIN_PIX) + extra - int((have & inwin).sum())
    keep_off = set(UNREAD_TAIL) | {LAST_READ}
    fill = []
    for s in range(ap.GROUP):
        q = -(-need // (ap.GROUP - s))  # the rest, spread evenly over the slices left
        cand = [p for p in win if p not in keep_off and p not in st.foot.get(s, set()) and not have[s, p[1], p[0]]]
        pick = [cand[k] for k in st.rng.choice(len(cand), q, replace=False)]
        assert ap.HEAD + q <= st.cursor.get(s, S)  # ahead of the planted tail
        for k, (px, py) in enumerate(pick):
            st.x[s * S + ap.HEAD + k], st.y[s * S + ap.HEAD + k] = px, py
        fill.append(q)
        need -= q
    assert need == 0
    xy = st.xy()
    return dict(name="cap_over" if extra else "cap_exact", xy=xy, t=ap.rising(len(xy), seed=seed), W=W, H=H, S=S,
                first=0, sae0=None, hot=CAP_HOT, probes=probes, fill=fill, item=(0, 5))


SLOT_SLICES = 34  # group 0 whole, two slices of group 1
UNTOUCHED = (14, 10)  # window word 4 of tile 5, right after FIRST_READ's 33 words; circle 4 (-4, 0) of (14, 14)
SLOT_HOT = ((FIRST_READ, (14, 14), tuple(range(32))),     # 32 values; "in" at j = 0 and j = 31
            (LAST_READ, (27, 27), (0, 7, 31)),            # the mask's lowest and highest bit
            ((0, 4), (4, 4), (2, 30)),                    # the sensor's left edge, tile 0's clipped window
            ((55, 37), (51, 37), (5, 20)))                # the sensor's right edge, tile 11's clipped window
# fully written tests: tile 5's corners and edge midpoints, the corners of what border tiles 0, 3, 8, 11 can test
SLOT_FULL = ((14, 14), (27, 14), (14, 27), (27, 27), (20, 14), (20, 27), (14, 20), (27, 20),
             (4, 4), (13, 13), (13, 4), (4, 13), (51, 4), (42, 13), (4, 37), (13, 28), (51, 37), (42, 28))


def slots(seed=52):
    st = ap.Stream(SLOT_SLICES, seed, avoid=[h for h, _, _ in SLOT_HOT] + [UNTOUCHED])
    _fire(st, SLOT_HOT)
    probes = _probe(st, SLOT_HOT, SLOT_SLICES, quiet_for=[(UNTOUCHED, (14, 14), 16)], never=[UNTOUCHED])
    full = []
    for k, (cx, cy) in enumerate(SLOT_FULL):  # each in the first two slices from a rotating start that have room
        ok = [s for s in [(3 * k + d) % ap.GROUP for d in range(ap.GROUP)] if st.free(s, cx, cy)][:2]
        assert len(ok) == 2, (cx, cy)
        full += [(st.plant(s, cx, cy, ap.A3, ap.A4, skip=[UNTOUCHED]), (cx, cy), s) for s in ok]
    xy = st.xy()
    return dict(name="slots", xy=xy, t=ap.rising(len(xy), seed=seed), W=W, H=H, S=S, first=0, sae0=None,
                hot=SLOT_HOT, probes=probes, full=full)


CASES = ("cap_exact", "cap_over", "slots")
_cache, _oracle, _predicted = {}, {}, {}


def case(name):
    if name not in _cache:
        _cache[name] = {"cap_exact": lambda: capacity(0), "cap_over": lambda: capacity(1), "slots": slots}[name]()
    return _cache[name]


def oracle(orc, name):
    """orc.fast_detect of the case -> (flags, final surface), computed once and shared (read-only)."""
    if name not in _oracle:
        f, s = ap.run_oracle(orc, case(name))
        f.setflags(write=False)
        s.setflags(write=False)
        _oracle[name] = (f, s)
    return _oracle[name]


def predicted(name):
    if name not in _predicted:
        _predicted[name] = ap.predicted_dense_items(case(name))
    return _predicted[name]
