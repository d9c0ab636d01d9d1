"""RAW ingest on the GPU at every scan boundary (csrc/evt.hip): decoder state placed just before
and used just after the lane / wave / chunk / group boundaries (whole and in pieces through the
carry state), arbitrary words across the group boundary, the densest and the x-wrapping vector
chunks, the documented call forms (NULL outputs, NULL n_out, cap 0, truncation with a carry
state, the shared status word) and the n-µs reslicer's edges and grid-stride loop.

Every comparison is exact equality of xy, t, p, the count and the status.  The decoders are
compared with the oracle (itself held to tests/evt_spec_ref.py by tests/test_ingest_spec.py) and,
for the crafted streams, with the events the stream builder placed or with arithmetic; the
reslicer with np.searchsorted and with the oracle."""
import numpy as np
import pytest

import evt_streams as es
from test_ingest import concat, events_random, events_rows

pytestmark = pytest.mark.gpu

SENT = 0xA5  # byte the outputs are pre-filled with


def _same(got, ref):
    assert len(got[0]) == len(ref[0])
    assert (got[0] == ref[0]).all() and (got[1] == ref[1]).all() and (got[2] == ref[2]).all()


class Decoder:
    """Device-resident words and sentinel-filled outputs of `cap` events; call() decodes
    words[lo:hi) and returns (xy, t, p, n_out, status) with the arrays cut to min(n_out, cap)."""

    def __init__(self, ecc, gpu, fmt, words, cap):
        self.ecc, self.gpu, self.fmt, self.cap = ecc, gpu, fmt, cap
        self.wsz = words.dtype.itemsize
        self.n_words = len(words)
        self.d_words = ecc.DeviceArray.from_numpy(words)
        self.d_xy = ecc.DeviceArray(cap + 1, np.uint32)
        self.d_t = ecc.DeviceArray(cap + 1, np.int64)
        self.d_p = ecc.DeviceArray(cap + 1, np.uint8)
        self.d_n = ecc.DeviceArray(1, np.int64)
        self.state = None

    def with_state(self):
        self.state = self.ecc.DeviceArray.from_numpy(np.zeros(self.ecc.EVT_STATE_BYTES, np.uint8))
        return self

    def call(self, lo=0, hi=None, cap=None, xy=True, t=True, p=True, n_out=True):
        hi = self.n_words if hi is None else hi
        cap = self.cap if cap is None else cap
        assert 0 <= lo <= hi <= self.n_words and cap <= self.cap
        for d in (self.d_xy, self.d_t, self.d_p, self.d_n):
            d.fill_bytes(SENT, self.gpu.stream)
        self.ecc.check(self.ecc.lib.ecc_evt_decode(
            self.gpu.ctx, self.fmt, self.d_words.ptr + lo * self.wsz, hi - lo, self.d_xy.ptr if xy else None,
            self.d_t.ptr if t else None, self.d_p.ptr if p else None, cap, self.d_n.ptr if n_out else None,
            self.state.ptr if self.state is not None else None, self.gpu.stream), "ecc_evt_decode")
        st = self.gpu.evt_status()
        self.raw = (self.d_xy.numpy(), self.d_t.numpy(), self.d_p.numpy())
        k = int(self.d_n.numpy()[0])
        m = min(k, cap) if n_out else cap
        return self.raw[0][:m], self.raw[1][:m], self.raw[2][:m], k, st

    def untouched(self, which, first):
        """Output `which` (0 xy, 1 t, 2 p) still holds the sentinel from entry `first` on."""
        return bool((self.raw[which][first:].view(np.uint8) == SENT).all())


SENT_I64 = int(np.full(8, SENT, np.uint8).view(np.int64)[0])


def _decode_whole(ecc, gpu, fmt, words, ref):
    dec = Decoder(ecc, gpu, fmt, words, len(ref[0]) + 8)
    xy, t, p, k, st = dec.call()
    assert k == len(ref[0]) and st == 0
    _same((xy, t, p), ref)
    assert all(dec.untouched(i, k) for i in range(3))  # nothing written past the count
    return dec


def _decode_pieces(ecc, gpu, fmt, words, cuts, n_total):
    """Decodes words in pieces [0, cuts[0]), [cuts[0], cuts[1]), ... with one carry state; returns
    the concatenated events and the per-piece counts."""
    dec = Decoder(ecc, gpu, fmt, words, n_total + 8).with_state()
    outs, counts, lo = [], [], 0
    for hi in list(cuts) + [len(words)]:
        xy, t, p, k, st = dec.call(lo, hi)
        assert st == 0
        outs.append((xy, t, p))
        counts.append(k)
        lo = hi
    return tuple(np.concatenate([o[i] for o in outs]) for i in range(3)), counts


# ---------------------------------------------------------------------------- B: boundary matrix
BOUNDARY_CASES = [(f, b, d) for f in (2, 3) for b, d in es.boundary_cases(f)]


@pytest.fixture(scope="module")
def boundary(orc):
    """(fmt, B, d) -> (words, placed events, oracle events), built once and left unchanged."""
    cache = {}

    def get(fmt, B, d):
        if (fmt, B, d) not in cache:
            words, placed = es.boundary_stream(fmt, B, d)
            for a in (words, *placed):
                a.setflags(write=False)
            cache[fmt, B, d] = (words, placed, orc.evt_decode(fmt, words))
        return cache[fmt, B, d]
    return get


@pytest.mark.parametrize("fmt,B,d", BOUNDARY_CASES)
def test_gpu_evt_state_crosses_boundary(ecc, gpu, boundary, fmt, B, d):
    """Setters (last y, TIME_LOW, TIME_HIGH, vector base + polarity + a non-zero x advance; EVT 2.0:
    a 28-bit TIME_HIGH) end d words before word B, consumers start at B (EVT 3.0: a TIME_HIGH
    decrease, so the loop cross term of the summary concatenation is what carries the loop), with
    B the lane, wave, chunk and group size.  The result is the oracle's and the builder's."""
    words, placed, ref = boundary(fmt, B, d)
    _same(ref, placed)
    if fmt == 3:
        assert placed[1][-1] >> 24 == 2 and placed[1][0] >> 24 == 0
    _decode_whole(ecc, gpu, fmt, words, placed)


@pytest.mark.parametrize("fmt,B,d", BOUNDARY_CASES)
def test_gpu_evt_state_crosses_boundary_in_pieces(ecc, gpu, boundary, fmt, B, d):
    """The same streams through the carry state: one cut exactly at B (between setter and
    consumer), three consecutive cuts (1-word pieces around B), and a zero-word piece at B, which
    reports n_out = 0 and leaves the state alone."""
    words, placed, _ = boundary(fmt, B, d)
    n = len(placed[0])
    got, counts = _decode_pieces(ecc, gpu, fmt, words, [B], n)
    _same(got, placed)
    assert sum(counts) == n and counts[1] > 0
    got, counts = _decode_pieces(ecc, gpu, fmt, words, [B - 1, B, B + 1], n)
    _same(got, placed)
    got, counts = _decode_pieces(ecc, gpu, fmt, words, [B, B], n)
    assert counts[1] == 0
    _same(got, placed)


@pytest.mark.parametrize("fmt", [2, 3])
def test_gpu_evt_junk_across_group_boundary(ecc, orc, gpu, fmt):
    """513 chunks + 77 uniform random words (seed 40 + fmt): every state variable and the event
    offset cross the group level (evt_group_kernel's totals, evt_carry_kernel's gcarry / goff)
    with arbitrary contents.  513 chunks is the smallest stream with a second group; the
    allocation (4.2 M EVT 3.0 words, about 3 M events) is large for that reason and no other.

    Not covered: evt_carry_kernel's second round starts past 512 groups = 2^31 EVT 3.0 words,
    beyond any test of a few seconds."""
    words = es.junk(fmt, 513 * es.CHUNK[fmt] + 77, seed=40 + fmt)
    ref = orc.evt_decode(fmt, words)
    assert len(ref[0]) > len(words) // (2 if fmt == 3 else 10)
    if fmt == 3:
        assert ref[1][-1] >> 24 > ref[1][512 * es.CHUNK[3] // 2] >> 24 > 0  # loops on both sides
    _decode_whole(ecc, gpu, fmt, words, ref)


# ---------------------------------------------------------------------- C: dense / wrapping
def test_gpu_evt3_dense_vect12_wraps_x(ecc, orc, gpu):
    """3 x 8192 VECT_12 0xFFF after one VECT_BASE_X 2040: 98 304 events in a full chunk (the lane
    prefix's 17-bit count, 48 output windows, 384 events per lane) and an x advance that passes
    2^16 four times (the prefix keeps it modulo 2^16)."""
    words = es.dense_vect12()
    n_vec = 3 * 8192
    ref = orc.evt_decode(3, words)
    dec = _decode_whole(ecc, gpu, 3, words, ref)
    xy, t, p = (a[:12 * n_vec] for a in dec.raw)
    assert len(ref[0]) == 12 * n_vec == 294_912
    i = np.arange(12 * n_vec, dtype=np.int64)
    assert (xy == (((es.DENSE_BASE + i) & 0xFFFF) | (es.DENSE_Y << 16)).astype(np.uint32)).all()
    for c in (1, 2, 3):  # the first event of each later chunk comes from word 8192 c
        first = 12 * (8192 * c - es.DENSE_HEAD)
        assert int(xy[first] & 0xFFFF) == (es.DENSE_BASE + first) % 65536
    assert (es.DENSE_BASE + 12 * n_vec) // 65536 == 4
    assert (t == es.DENSE_T).all() and (p == 1).all()


@pytest.mark.parametrize("name", ["alternating_vect", "all_addr_x", "all_cd_evt2"])
def test_gpu_evt_dense_streams(ecc, orc, gpu, name):
    """2 chunks + 1 word of: VECT_12 0xFFF / VECT_8 0x00 in turn (zero masks still advance x);
    ADDR_X only; EVT 2.0 CD words only (each chunk fills its four 1024-event windows exactly)."""
    fmt, build = es.DENSE[name]
    words = build()
    ref = orc.evt_decode(fmt, words)
    dec = _decode_whole(ecc, gpu, fmt, words, ref)
    if name == "alternating_vect":
        n_pair = (len(words) - es.DENSE_HEAD + 1) // 2
        i = np.arange(12 * n_pair, dtype=np.int64)
        assert len(ref[0]) == 12 * n_pair
        assert (dec.raw[0][:len(i)] & 0xFFFF == (es.DENSE_BASE + i // 12 * 20 + i % 12) & 0xFFFF).all()
    elif name == "all_addr_x":
        assert len(ref[0]) == len(words) - 3
    else:
        assert len(ref[0]) == len(words) == 2 * 4 * 1024 + 1


# --------------------------------------------------------------------------- D: call forms
@pytest.fixture(scope="module")
def encoded(orc):
    """fmt -> (words, oracle events) of an encoded stream with rows, loops and noise words."""
    out = {}
    for fmt in (2, 3):
        ev = concat(events_random(30_000, 61, t_span=1 << 27), events_rows(2000, 62))
        words = orc.evt_encode(fmt, *ev, seed=11, noise_pct=10)
        ref = orc.evt_decode(fmt, words)
        _same(ref, ev)
        for a in (words, *ref):
            a.setflags(write=False)
        out[fmt] = (words, ref)
    return out


@pytest.mark.parametrize("fmt", [2, 3])
def test_gpu_evt_null_outputs(ecc, gpu, encoded, fmt):
    """Each of xy / t / p NULL in turn, and all three: the others and n_out are as in the full
    call; n_out NULL: the arrays are as in the full call."""
    words, ref = encoded[fmt]
    n = len(ref[0])
    assert len(words) > 3 * es.CHUNK[fmt]
    dec = Decoder(ecc, gpu, fmt, words, n + 8)
    for off in ((0,), (1,), (2,), (0, 1, 2)):
        on = [i not in off for i in range(3)]
        got = dec.call(xy=on[0], t=on[1], p=on[2])
        assert got[3] == n and got[4] == 0
        for i in range(3):
            if on[i]:
                assert (got[i] == ref[i]).all() and dec.untouched(i, n)
            else:
                assert dec.untouched(i, 0)
    got = dec.call(n_out=False)
    assert got[4] == 0 and got[3] == SENT_I64
    _same(tuple(a[:n] for a in dec.raw), ref)
    assert all(dec.untouched(i, n) for i in range(3))


@pytest.mark.parametrize("fmt", [2, 3])
def test_gpu_evt_cap_zero(ecc, gpu, encoded, fmt):
    """cap 0: ERR_CAPACITY, the true count, no output entry written."""
    words, ref = encoded[fmt]
    dec = Decoder(ecc, gpu, fmt, words, 64)
    got = dec.call(cap=0)
    assert got[3] == len(ref[0]) and got[4] == ecc.ERR_CAPACITY
    assert all(dec.untouched(i, 0) for i in range(3))


@pytest.mark.parametrize("fmt", [2, 3])
def test_gpu_evt_state_advances_past_truncation(ecc, gpu, encoded, fmt):
    """A piece truncated by cap still advances the carry state over the events it did not write:
    the next piece equals the oracle's tail."""
    words, ref = encoded[fmt]
    n, cut = len(ref[0]), len(words) // 2 + 1
    dec = Decoder(ecc, gpu, fmt, words, n + 8).with_state()
    xy, t, p, k1, st = dec.call(0, cut, cap=1000)
    assert st == ecc.ERR_CAPACITY and 1000 < k1 < n
    _same((xy, t, p), tuple(a[:1000] for a in ref))
    assert all(dec.untouched(i, 1000) for i in range(3))
    xy, t, p, k2, st = dec.call(cut, len(words))
    assert st == 0 and k1 + k2 == n
    _same((xy, t, p), tuple(a[k1:] for a in ref))
    if fmt == 3:
        assert ref[1][k1] >> 24 > 0  # the tail needs the loop count of the truncated piece


@pytest.mark.parametrize("fmt", [2, 3])
def test_gpu_evt_empty_piece_keeps_state(ecc, gpu, encoded, fmt):
    """A zero-word call with a carry state mid-stream: n_out = 0, nothing written, and the rest
    decodes as if the call had not happened."""
    words, ref = encoded[fmt]
    n, cut = len(ref[0]), es.CHUNK[fmt] + 3
    dec = Decoder(ecc, gpu, fmt, words, n + 8).with_state()
    a = dec.call(0, cut)
    e = dec.call(cut, cut)
    assert e[3] == 0 and e[4] == 0 and all(dec.untouched(i, 0) for i in range(3))
    b = dec.call(cut, len(words))
    assert a[3] + b[3] == n and a[4] == 0 and b[4] == 0
    _same(tuple(np.concatenate([a[i], b[i]]) for i in range(3)), ref)


class Reslicer:
    """ecc_reslice_n_us with sentinel-filled bounds and GUARD sentinel entries on both sides."""
    GUARD = 64

    def __init__(self, ecc, gpu, t):
        self.ecc, self.gpu = ecc, gpu
        self.d_t = t if isinstance(t, ecc.DeviceArray) else ecc.DeviceArray.from_numpy(np.asarray(t, np.int64))
        self.n = self.d_t.shape[0]

    def call(self, period, max_slices, n=None, n_slices=True):
        """Returns (bounds[0 .. max_slices], n_slices, status) and checks the guards."""
        ecc, gpu, G = self.ecc, self.gpu, self.GUARD
        d_b = ecc.DeviceArray(max_slices + 1 + 2 * G, np.int64)
        d_ns = ecc.DeviceArray(1, np.int64)
        d_b.fill_bytes(SENT, gpu.stream)
        d_ns.fill_bytes(SENT, gpu.stream)
        ecc.check(ecc.lib.ecc_reslice_n_us(gpu.ctx, self.d_t.ptr, self.n if n is None else n, period,
                                           d_b.ptr + 8 * G, max_slices, d_ns.ptr if n_slices else None,
                                           gpu.stream), "ecc_reslice_n_us")
        st = gpu.evt_status()
        b = d_b.numpy()
        assert (b[:G] == SENT_I64).all() and (b[-G:] == SENT_I64).all()  # nothing outside bounds[]
        return b[G:-G], int(d_ns.numpy()[0]), st


def test_gpu_ingest_status_word_is_shared_and_cleared(ecc, gpu, encoded):
    """Decode and reslicer share one status word: a clean call of either clears the other's
    ERR_CAPACITY (and a clean zero-size call clears it too)."""
    words, ref = encoded[3]
    dec = Decoder(ecc, gpu, 3, words, len(ref[0]) + 8)
    rs = Reslicer(ecc, gpu, np.arange(0, 1000, 10))
    assert dec.call(cap=5)[4] == ecc.ERR_CAPACITY
    assert rs.call(100, 16)[2] == 0
    assert rs.call(100, 3)[2] == ecc.ERR_CAPACITY
    assert dec.call()[4] == 0
    assert rs.call(100, 3)[2] == ecc.ERR_CAPACITY
    assert dec.call(0, 0)[4] == 0
    assert dec.call(cap=5)[4] == ecc.ERR_CAPACITY
    assert rs.call(100, 16, n=0)[2] == 0


# ------------------------------------------------------------------------------ E: reslicer
def _searchsorted_bounds(t, period):
    """bounds[0 .. ns] and ns from np.searchsorted; the base uses Python's floor division."""
    t = np.asarray(t, np.int64)
    base = int(t[0]) // period * period
    ns = (int(t[-1]) - base) // period + 1
    edges = base + period * np.arange(ns, dtype=np.int64)
    return np.concatenate([np.searchsorted(t, edges, "left"), [len(t)]]).astype(np.int64), ns


def _check_reslice(ecc, orc, gpu, t, period, max_slices=None, rs=None, n_slices=True):
    t = np.asarray(t, np.int64)
    ref, ns = _searchsorted_bounds(t, period)
    max_slices = ns if max_slices is None else max_slices
    o_b, o_ns = orc.reslice_n_us(t, period, max_slices)
    b, g_ns, st = (rs or Reslicer(ecc, gpu, t)).call(period, max_slices, n_slices=n_slices)
    m = min(ns, max_slices)
    assert (g_ns == ns if n_slices else g_ns == SENT_I64) and o_ns == ns
    assert (b[:m] == ref[:m]).all() and (o_b[:m] == ref[:m]).all()
    assert b[m] == len(t) == o_b[m]
    assert (b[m + 1:] == SENT_I64).all()
    assert st == (ecc.ERR_CAPACITY if ns > max_slices else 0)
    return b, ns


STRIDE = 8192 * 256  # the reslicer's launch cap: threads of the largest grid


@pytest.fixture(scope="module")
def stride_stamps():
    """2 097 152 + 257 sorted stamps: random ones for the first grid-stride pass, then one new
    777-µs slice per event for the second, then a gap of empty slices before the last three."""
    rng = np.random.default_rng(71)
    head = np.sort(rng.integers(-50_000, 3_000_000, STRIDE)).astype(np.int64)
    tail = 3_000_000 + 777 * np.arange(1, 255, dtype=np.int64)  # each first in a slice of its own
    t = np.concatenate([head, tail, [9_000_000, 9_000_000, 9_000_001]])
    assert len(t) == STRIDE + 257
    t.setflags(write=False)
    return t


def test_gpu_reslice_grid_stride(ecc, orc, gpu, stride_stamps):
    """n past the launch cap of 8192 x 256 threads, so the grid-stride loop takes a second pass;
    the events of that pass each open a slice, and the gap leaves empty ones."""
    rs = Reslicer(ecc, gpu, stride_stamps)
    for period in (777, 50_000):
        b, ns = _check_reslice(ecc, orc, gpu, stride_stamps, period, rs=rs)
        assert (np.diff(b[:ns + 1]) == 0).any()  # empty slices
    b, _ = _check_reslice(ecc, orc, gpu, stride_stamps, 777, rs=rs)
    assert np.isin(np.arange(STRIDE, STRIDE + 254), b).all()


@pytest.mark.parametrize("case", ["one", "two_equal", "many_equal", "multiples", "multiples_negative"])
def test_gpu_reslice_small_and_equal(ecc, orc, gpu, case):
    period = 50
    if case == "one":
        t = [12_345]
    elif case == "two_equal":
        t = [777, 777]
    elif case == "many_equal":
        t = [1_000_003] * 5000
    elif case == "multiples":  # exactly on the period: each event opens its own slice
        t = period * np.arange(4, 1004)
    else:
        t = period * np.arange(-500, 500)
    for per in (period, 1, 7):
        b, ns = _check_reslice(ecc, orc, gpu, t, per)
        if case in ("one", "two_equal", "many_equal"):
            assert ns == 1 and b[0] == 0
    if case.startswith("multiples"):
        b, ns = _check_reslice(ecc, orc, gpu, t, period)
        assert ns == len(t) and (b[:ns] == np.arange(ns)).all()


@pytest.mark.parametrize("t0", [-100, -101, -1, 0, 49, 50])
def test_gpu_reslice_floor_of_first_stamp(ecc, orc, gpu, t0):
    """Both branches of the floor of a negative t[0] (on and off a period multiple)."""
    period = 50
    t = t0 + np.array([0, 1, 49, 50, 51, 100, 149, 150, 260])
    b, ns = _check_reslice(ecc, orc, gpu, t, period)
    base = {-100: -100, -101: -150, -1: -50, 0: 0, 49: 0, 50: 50}[t0]
    assert ns == (t[-1] - base) // period + 1
    assert b[1] == int((t < base + period).sum())


def test_gpu_reslice_max_slices(ecc, orc, gpu):
    """max_slices 0, ns - 1, ns, ns + 1: only slices < max_slices are written, bounds[min(ns,
    max_slices)] = n, ERR_CAPACITY exactly when ns > max_slices; n_slices NULL changes nothing."""
    rng = np.random.default_rng(72)
    t = np.sort(rng.integers(-3000, 40_000, 3000))
    t = np.concatenate([t, [90_000]])
    rs = Reslicer(ecc, gpu, t)
    ns = _searchsorted_bounds(t, 100)[1]
    for max_slices in (0, ns - 1, ns, ns + 1):
        _check_reslice(ecc, orc, gpu, t, 100, max_slices, rs=rs)
        _check_reslice(ecc, orc, gpu, t, 100, max_slices, rs=rs, n_slices=False)


@pytest.mark.parametrize("at", [256, STRIDE])
def test_gpu_reslice_unsorted_pair(ecc, gpu, stride_stamps, at):
    """One decreasing pair (at - 1, at): across a block boundary, and across the grid-stride
    boundary (the second pass's first event compares with the first pass's last)."""
    t = stride_stamps[:STRIDE + 257 if at == STRIDE else 1000].copy()
    t[at] = t[at - 1] - 1
    assert t[at] >= t[0] and (np.diff(t) < 0).sum() == 1
    b, _, st = Reslicer(ecc, gpu, t).call(50_000, 400)
    assert st == ecc.ERR_UNSORTED_TIME


def test_gpu_reslice_unsorted_below_base_stays_in_bounds(ecc, gpu):
    """Unsorted stamps that fall below the first slice's base: ERR_UNSORTED_TIME, and no write
    outside bounds[0 .. max_slices] (such a stamp has no slice; it must not index one)."""
    for t in ([100, 0, 200], [100, 0], [100, 0, 0, 50]):
        b, _, st = Reslicer(ecc, gpu, t).call(2, 60)
        assert st == ecc.ERR_UNSORTED_TIME


def test_gpu_encode_decode_reslice_chain(ecc, orc, gpu):
    """Events -> RAW writer -> GPU decode -> GPU reslice of the device-resident t == searchsorted
    on the original stamps."""
    ev = concat(events_random(60_000, 81, t_span=1 << 26), events_rows(3000, 82))
    n = len(ev[0])
    for fmt in (2, 3):
        dec = Decoder(ecc, gpu, fmt, ecc.evt_encode(fmt, *ev), n + 8)
        got = dec.call()
        assert got[3] == n and got[4] == 0
        _same(got, ev)
        ref, ns = _searchsorted_bounds(ev[1], 50_000)
        b, g_ns, st = Reslicer(ecc, gpu, dec.d_t).call(50_000, ns, n=n)
        assert g_ns == ns and st == 0 and (b[:ns + 1] == ref).all()
