"""Crafted EVT 2.0 / EVT 3.0 word streams for the ingest tests (tests/test_ingest_spec.py on the
CPU, tests/test_gpu_ingest_edges.py on the GPU).

The decoders are a four-level scan (csrc/evt.hip): a lane owns LANE[fmt] words, a wave 64 lanes,
a chunk 256 lanes, a group 512 chunks.  boundary_stream() puts words that SET decoder state just
before one of those boundaries and words that USE it just after, in a background of words that
neither set state nor emit, and returns the events it knows it placed — computed here from the
placed fields, not by any decoder."""
import numpy as np

LANE = {2: 16, 3: 32}
WAVE = {f: 64 * v for f, v in LANE.items()}
CHUNK = {f: 256 * v for f, v in LANE.items()}
GROUP = {f: 512 * v for f, v in CHUNK.items()}
DTYPE = {2: np.uint32, 3: np.uint16}

BOUNDARIES = {f: (LANE[f], WAVE[f], CHUNK[f], GROUP[f]) for f in (2, 3)}
TAIL = 8192 + 5  # words after the boundary: ragged, and one more chunk boundary for EVT 2.0
N_SETTERS = {2: 2, 3: 5}


def distances(fmt):
    """Background words between the last setter and the boundary: 0, a lane, a chunk + 1."""
    return (0, LANE[fmt], CHUNK[fmt] + 1)


def boundary_cases(fmt):
    """(B, d) pairs whose first setter is not before word 0."""
    return [(b, d) for b in BOUNDARIES[fmt] for d in distances(fmt) if b - d - N_SETTERS[fmt] >= 0]


# EVT 3.0 word constructors (format table: include/ecc.h §8)
def addr_y(y): return 0x0000 | y
def addr_x(x, p): return 0x2000 | (p << 11) | x
def vect_base_x(x, p): return 0x3000 | (p << 11) | x
def vect_12(mask): return 0x4000 | mask
def vect_8(mask): return 0x5000 | mask
def time_low(v): return 0x6000 | v
def time_high(v): return 0x8000 | v


def _bits(mask):
    return [b for b in range(12) if mask >> b & 1]


def _evt3_boundary(B, d):
    n = B + TAIL
    w = np.full(n, 0xE000, np.uint16)  # OTHERS: no state, no event
    w[1::3] = 0xE5A5                   # (its payload is free)
    Y, TL, X0, XA = 345, 0x9C7, 700, 1234
    M0, M8, M12 = 0b101000000011, 0b10010110, 0b110000000001
    s = B - 1 - d  # the last setter
    w[s - 4], w[s - 3], w[s - 2] = time_high(5), time_low(TL), addr_y(Y)
    w[s - 1], w[s] = vect_base_x(X0, 1), vect_12(M0)
    w[B], w[B + 1], w[B + 2], w[B + 3] = time_high(3), addr_x(XA, 0), vect_8(M8), vect_12(M12)
    later = B + 4100  # second decrease, past the next chunk boundary when B is one
    w[later], w[later + 1] = time_high(1), addr_x(7, 1)
    w[n - 1] = addr_x(2047, 1)  # the last word of the ragged tail
    ev = []  # (x, y, p, t)
    t0, t1, t2 = 5 << 12 | TL, 1 << 24 | 3 << 12 | TL, 2 << 24 | 1 << 12 | TL
    ev += [(X0 + b, Y, 1, t0) for b in _bits(M0)]
    ev += [(XA, Y, 0, t1)]
    ev += [(X0 + 12 + b, Y, 1, t1) for b in _bits(M8)]
    ev += [(X0 + 20 + b, Y, 1, t1) for b in _bits(M12)]
    ev += [(7, Y, 1, t2), (2047, Y, 1, t2)]
    return w, ev


def _evt2_cd(p, lsb, x, y):
    return (p << 28) | (lsb << 22) | (x << 11) | y


def _evt2_boundary(B, d):
    n = B + TAIL
    w = np.full(n, 0xE0000000, np.uint32)  # OTHERS
    w[1::3] = 0xE5A5A5A5
    TH = 0x0FFFFFFF  # all 28 bits: the top bit of the field is set
    s = B - 1 - d
    w[s - 1] = _evt2_cd(1, 9, 11, 12)  # before any TIME_HIGH: time-high 0
    w[s] = 0x80000000 | TH
    w[B], w[B + 1] = _evt2_cd(1, 63, 2047, 0), _evt2_cd(0, 0, 0, 2047)
    later = B + 4100
    w[later], w[later + 1] = 0x80000000 | 77, _evt2_cd(0, 5, 640, 480)
    w[n - 1] = _evt2_cd(1, 1, 2, 3)
    ev = [(11, 12, 1, 9), (2047, 0, 1, TH << 6 | 63), (0, 2047, 0, TH << 6), (640, 480, 0, 77 << 6 | 5),
          (2, 3, 1, 77 << 6 | 1)]
    return w, ev


def boundary_stream(fmt, B, d):
    """words, and the placed events as (xy u32, t i64, p u8) arrays."""
    w, ev = (_evt2_boundary if fmt == 2 else _evt3_boundary)(B, d)
    xy = np.array([x | y << 16 for x, y, _, _ in ev], np.uint32)
    return w, (xy, np.array([e[3] for e in ev], np.int64), np.array([e[2] for e in ev], np.uint8))


def junk(fmt, n, seed):
    """n uniform random words."""
    rng = np.random.default_rng(seed)
    return rng.integers(0, 1 << (32 if fmt == 2 else 16), n, dtype=np.uint64).astype(DTYPE[fmt])


# ---- dense and wrapping streams ---------------------------------------------------------------
DENSE_HEAD = 4     # TIME_HIGH, TIME_LOW, ADDR_Y, VECT_BASE_X
DENSE_BASE = 2040
DENSE_Y, DENSE_T = 719, 0x123 << 12 | 0x456


def _evt3_head(n_body, base_word=None):
    head = [time_high(0x123), time_low(0x456), addr_y(DENSE_Y)] + ([base_word] if base_word is not None else [])
    w = np.empty(len(head) + n_body, np.uint16)
    w[:len(head)] = head
    return w, len(head)


def dense_vect12():
    """One VECT_BASE_X 2040, then 3 x 8192 VECT_12 0xFFF: 12 events per word (98 304 in a full
    chunk, the 17-bit count's worst case) and an x advance of 294 912, past 65 536 four times."""
    w, h = _evt3_head(3 * 8192, vect_base_x(DENSE_BASE, 1))
    w[h:] = vect_12(0xFFF)
    return w


def alternating_vect():
    """VECT_12 0xFFF / VECT_8 0x00 in turn, 2 chunks + 1 word."""
    w, h = _evt3_head(2 * 8192 + 1 - DENSE_HEAD, vect_base_x(DENSE_BASE, 0))
    w[h::2], w[h + 1::2] = vect_12(0xFFF), vect_8(0x00)
    return w


def all_addr_x():
    """Every word after the three-word header is an ADDR_X, 2 chunks + 1 word."""
    w, h = _evt3_head(2 * 8192 + 1 - 3)
    i = np.arange(len(w) - h)
    w[h:] = 0x2000 | ((i & 1) << 11) | (i * 7 % 2048)
    return w


def all_cd_evt2():
    """2 chunks + 1 of pure EVT 2.0 CD words: every chunk fills its four 1024-event windows."""
    i = np.arange(2 * 4096 + 1, dtype=np.uint32)
    return ((i & 1) << 28) | ((i % 64) << 22) | ((i * 5 % 2048) << 11) | (i * 3 % 2048)


DENSE = {"dense_vect12": (3, dense_vect12), "alternating_vect": (3, alternating_vect),
         "all_addr_x": (3, all_addr_x), "all_cd_evt2": (2, all_cd_evt2)}
