"""EVT 2.1 RAW ingest, host side (include/ecc.h §8): the header probe (EVT21 is not EVT2), the
word format on hand-written words, the numpy comparator against the per-word loop, and the RAW
writer's round trip.  No GPU: the HIP decoder is held to the same comparator in
tests/test_gpu_evt21.py.  Parity against OpenEB is unpinned, as for EVT 2.0 / 3.0."""
import numpy as np
import pytest

import evt21_spec_ref as ref
from test_ingest import concat, events_random


def _same(got, want):
    assert len(got[0]) == len(want[0])
    assert (got[0] == want[0]).all() and (got[1] == want[1]).all() and (got[2] == want[2]).all()


# ------------------------------------------------------------------------------ header probing
def _probe(ecc, tmp_path, header, payload=b"\x00" * 43):
    path = tmp_path / "h.raw"
    path.write_bytes(header.encode() + payload)
    return ecc.raw_probe(path), len(header), len(payload)


@pytest.mark.parametrize("header,fmt", [
    ("% format EVT21;height=720;width=1280\n% end\n", 21),
    ("% date 2024-01-01\n% evt 2.1\n% geometry 1280x720\n% end\n", 21),
    ("% evt 2.1\n% format EVT21;height=720;width=1280\n", 21),
    ("% format EVT21;endianness=legacy;height=720;width=1280\n% end\n", 22),
    ("% evt 2.1\n% format EVT21;height=720;width=1280;endianness=legacy\n% end\n", 22),
    ("% format EVT21;height=720;width=1280;endianness=little\n% end\n", 21),
])
def test_probe_evt21_headers(ecc, tmp_path, header, fmt):
    info, hlen, plen = _probe(ecc, tmp_path, header)
    assert info.format == fmt and info.word_bytes == 8
    assert info.header_bytes == hlen and info.n_words == plen // 8 == 5
    assert (info.width, info.height) == (1280, 720)
    assert ecc.EVT21 == 21 and ecc.EVT21_LEGACY == 22


def test_probe_evt2_and_evt3_keep_their_meaning(ecc, tmp_path):
    info, _, plen = _probe(ecc, tmp_path, "% format EVT2;height=480;width=640\n% end\n")
    assert info.format == 2 and info.word_bytes == 4 and info.n_words == plen // 4
    assert (info.width, info.height) == (640, 480)
    assert _probe(ecc, tmp_path, "% evt 2.0\n")[0].format == 2
    assert _probe(ecc, tmp_path, "% evt 3.0\n% format EVT3;height=720;width=1280\n% end\n")[0].format == 3
    for bad in ("% evt 4.0\n% end\n", "% format EVT22;height=1;width=1\n", "% evt 2.10\n"):
        with pytest.raises(ecc.EccError):
            _probe(ecc, tmp_path, bad)


def test_raw_read_words_evt21(ecc, tmp_path):
    words = ref.junk(1000, 3)
    path = tmp_path / "w.raw"
    path.write_bytes(b"% format EVT21;height=720;width=1280\n% end\n" + words.tobytes() + b"\x01\x02\x03")
    info = ecc.raw_probe(path)
    assert info.n_words == 1000
    got = ecc.raw_read_words(path, info)
    assert got.dtype == np.uint64 and (got == words).all()
    assert (ecc.raw_read_words(path, info, 100, 50) == words[100:150]).all()


# ---------------------------------------------------------------------------------- known words
KNOWN = [
    ref.cd(0, 5, 96, 7, 0b101),               # before any TIME_HIGH: th = 0, t = 5
    ref.time_high(0x0FFFFFFF),                # a 28-bit TIME_HIGH of all ones
    ref.cd(1, 63, 64, 2047, 0x80000001),      # EVT_POS at x = 64: x 64 and 95
    ref.cd(1, 1, 32, 9, 0),                   # mask 0: no event
    (0xA << 60) | 0x123456789,                # trigger between two CD words
    ref.cd(0, 2, 2016, 3, 1 << 31),           # x 2047
    ref.time_high(2),
    (0xF << 60) | (1 << 59) | 0xFFFFFFFF,     # continued: no event, no state
    ref.cd(0, 0, 2047, 0, (1 << 31) | 1),     # junk x: 2047 and 2078
]
KNOWN_XY = [(96, 7), (98, 7), (64, 2047), (95, 2047), (2047, 3), (2047, 0), (2078, 0)]
T1 = (0x0FFFFFFF << 6) | 63
KNOWN_T = [5, 5, T1, T1, (0x0FFFFFFF << 6) | 2, 2 << 6, 2 << 6]
KNOWN_P = [0, 0, 1, 1, 0, 0, 0]


@pytest.mark.parametrize("legacy", [False, True])
@pytest.mark.parametrize("decoder", [ref.decode_evt21, ref.decode_evt21_np])
def test_known_words(decoder, legacy):
    words = np.array(KNOWN, np.uint64)
    if legacy:
        words = ref.swap_halves(words)
        assert int(words[1]) == 0x8FFFFFFF  # the half with the type sits in the low 32 bits
    xy, t, p = decoder(words, legacy=legacy)
    assert [(int(v) & 0xFFFF, int(v) >> 16) for v in xy] == KNOWN_XY
    assert list(t) == KNOWN_T and list(p) == KNOWN_P


# ------------------------------------------------------------------- numpy form == the loop form
@pytest.mark.parametrize("legacy", [False, True])
@pytest.mark.parametrize("case", ["junk", "sparse", "dense", "empty", "no_cd", "all_masks_zero"])
def test_numpy_form_equals_loop_form(case, legacy):
    if case == "junk":
        words = ref.junk(50_000, 1)
    elif case == "sparse":
        words = ref.sparse(50_000, 2)
    elif case == "dense":
        words = np.full(3000, ref.cd(1, 9, 2047, 5, 0xFFFFFFFF), np.uint64)
        words[::700] = ref.time_high(77)
    elif case == "empty":
        words = np.zeros(0, np.uint64)
    elif case == "no_cd":
        words = ref.junk(5000, 4) | np.uint64(0x8 << 60)
    else:
        words = ref.sparse(5000, 5) & np.uint64(0xFFFFFFFF00000000)
    if legacy:
        words = ref.swap_halves(words)
    want = ref.decode_evt21(words, legacy=legacy)
    _same(ref.decode_evt21_np(words, legacy=legacy), want)
    if case in ("junk", "sparse", "dense"):
        assert len(want[0]) > len(words)
    else:
        assert len(want[0]) == 0


# ----------------------------------------------------------------------------- writer round trip
def events_row_runs(n_runs, seed, wh=(1280, 720)):
    """Rows of consecutive x at equal (t, y, p), 20 to 90 long, from any x."""
    rng = np.random.default_rng(seed)
    xs, ys, ts, ps = [], [], [], []
    t = 0
    for _ in range(n_runs):
        t += int(rng.integers(0, 50))
        m = int(rng.integers(20, 90))
        x = int(rng.integers(0, wh[0] - m)) + np.arange(m)
        xs.append(x); ys.append(np.full(m, rng.integers(0, wh[1]))); ts.append(np.full(m, t))
        ps.append(np.full(m, rng.integers(0, 2)))
    x, y = np.concatenate(xs), np.concatenate(ys)
    return (x | (y << 16)).astype(np.uint32), np.concatenate(ts).astype(np.int64), np.concatenate(ps).astype(np.uint8)


def _popcounts(words, fmt):
    w = ref.swap_halves(words) if fmt == 22 else words
    cd = (w >> np.uint64(61)) == 0
    m = (w[cd] & np.uint64(0xFFFFFFFF)).astype("<u4")
    return np.unpackbits(m.view(np.uint8).reshape(-1, 4), axis=1).sum(axis=1)


@pytest.mark.parametrize("fmt", [21, 22])
@pytest.mark.parametrize("case", ["random", "rows", "duplicates", "decreasing_x", "late"])
def test_writer_roundtrip(ecc, fmt, case):
    """ecc_evt_encode(21 | 22) -> the Python decoder == the events, in their order."""
    if case == "random":
        ev = events_random(20_000, 51, t_span=1 << 27)
    elif case == "rows":
        ev = events_row_runs(400, 52)
    elif case == "duplicates":  # equal t, same pixel twice running, and again after another pixel
        x = np.array([5, 5, 6, 5, 5, 40, 40, 7], np.uint32)
        ev = (x | np.uint32(3 << 16), np.full(8, 1000, np.int64), np.ones(8, np.uint8))
    elif case == "decreasing_x":  # inside one 32-block, equal t, y, p
        x = np.array([30, 29, 28, 3, 2, 1, 0, 31], np.uint32)
        ev = (x + np.uint32(64) | np.uint32(9 << 16), np.full(8, 77, np.int64), np.zeros(8, np.uint8))
    else:  # the last stamp the format holds, and x, y at their limits
        ev = (np.array([2047 | (2047 << 16)] * 2, np.uint32), np.array([0, (1 << 34) - 1], np.int64),
              np.array([1, 0], np.uint8))
    words = ecc.evt_encode(fmt, *ev)
    assert words.dtype == np.uint64 and len(words) <= 2 * len(ev[0]) + 1
    _same(ref.decode(fmt, words), ev)
    first = int(ref.swap_halves(words[:1])[0] if fmt == 22 else words[0])
    assert first >> 60 == 0x8  # a TIME_HIGH opens the stream
    pc = _popcounts(words, fmt)
    assert pc.sum() == len(ev[0]) and pc.min() >= 1
    if case == "rows":
        assert (pc > 8).sum() >= 400 and pc.max() == 32
    if case == "duplicates":
        assert list(pc) == [1, 2, 1, 1, 1, 1, 1]
    if case == "decreasing_x":
        assert list(pc) == [1, 1, 1, 1, 1, 1, 2]


@pytest.mark.parametrize("fmt", [21, 22])
def test_writer_is_deterministic_and_legacy_is_the_swap(ecc, fmt):
    ev = concat(events_random(5000, 53), events_row_runs(50, 54))
    a, b = ecc.evt_encode(21, *ev), ecc.evt_encode(22, *ev)
    assert (ecc.evt_encode(fmt, *ev) == (a if fmt == 21 else b)).all()
    assert (ref.swap_halves(a) == b).all()


@pytest.mark.parametrize("fmt", [21, 22])
def test_writer_refuses_bad_input(ecc, fmt):
    xy, p = np.zeros(3, np.uint32), np.zeros(3, np.uint8)
    with pytest.raises(ecc.EccError) as e:
        ecc.evt_encode(fmt, xy, np.array([5, 4, 6], np.int64), p)
    assert e.value.rc == ecc.ERR_UNSORTED_TIME
    for t in ([0, 1, 1 << 34], [-1, 0, 1]):
        with pytest.raises(ecc.EccError):
            ecc.evt_encode(fmt, xy, np.array(t, np.int64), p)
    assert len(ecc.evt_encode(fmt, xy[:0], np.zeros(0, np.int64), p[:0])) == 0
