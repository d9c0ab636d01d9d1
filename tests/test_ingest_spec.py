"""The oracle's EVT decoders (oracle/oracle.cpp) and the product RAW writer against a plain decoder
written from the word tables (tests/evt_spec_ref.py).  Every GPU ingest check compares with the
oracle, and the oracle was so far checked only by its own encoder's round trip and two hand-made
word lists; here it has to agree with an independent reading of include/ecc.h §8, on arbitrary
words, on the encoder's streams and on the crafted boundary / dense streams that
tests/test_gpu_ingest_edges.py decodes on the GPU.  Exact equality throughout."""
import numpy as np
import pytest

import evt_spec_ref as spec
import evt_streams as es
from test_ingest import concat, events_random, events_rows

CUT = 20_000  # longer crafted streams: their first and last CUT words


def _same(got, ref):
    assert len(got[0]) == len(ref[0])
    for g, r in zip(got, ref):
        assert g.dtype == r.dtype and (g == r).all()


def _check_oracle(orc, fmt, words):
    _same(orc.evt_decode(fmt, words), spec.decode(fmt, words))


def _first(ev, n):
    assert len(ev[0]) >= n
    return tuple(a[:n] for a in ev)


def _cuts(words):
    return [words] if len(words) <= CUT else [words[:CUT], words[-CUT:]]


@pytest.mark.parametrize("fmt", [2, 3])
def test_oracle_matches_spec_on_junk(orc, fmt):
    """50 000 uniform random words (seed 20 + fmt): every type nibble, every state order."""
    words = es.junk(fmt, 50_000, seed=20 + fmt)
    ref = spec.decode(fmt, words)
    assert len(ref[0]) > (20_000 if fmt == 3 else 5_000)  # the stream does emit
    if fmt == 3:
        assert ref[1].max() >> 24 > 100             # time loops happen
        assert (ref[0] & 0xFFFF).max() > 2047 + 12  # vector runs leave the 11-bit range
    _same(orc.evt_decode(fmt, words), ref)


@pytest.mark.parametrize("fmt", [2, 3])
@pytest.mark.parametrize("case", ["rows", "loops", "noise"])
def test_oracle_matches_spec_on_encoded(orc, fmt, case):
    if case == "rows":
        ev = events_rows(1200, 2)
    elif case == "loops":
        ev = concat(events_random(3000, 3, t_span=1 << 27), _first(events_rows(250, 4), 2000))
    else:
        ev = concat(events_random(3000, 5), _first(events_rows(250, 6), 2000))
    ev = _first(ev, 5000)
    assert len(ev[0]) == 5000
    words = orc.evt_encode(fmt, *ev, seed=7, noise_pct=30 if case == "noise" else 5)
    assert len(words) <= spec.MAX_WORDS
    got = spec.decode(fmt, words)
    _same(got, ev)  # the plain decoder reads the encoder's stream back, loops included
    _same(orc.evt_decode(fmt, words), got)
    if case == "loops" and fmt == 3:
        assert got[1].max() >> 24 >= 4


@pytest.mark.parametrize("fmt,B,d", [(f, b, d) for f in (2, 3) for b, d in es.boundary_cases(f)])
def test_oracle_matches_spec_on_boundary_streams(orc, fmt, B, d):
    """The boundary-matrix streams of the GPU tests: the oracle, the plain decoder and the
    builder's own list of placed events agree."""
    words, placed = es.boundary_stream(fmt, B, d)
    assert len(words) == B + es.TAIL and words.dtype == es.DTYPE[fmt]
    whole = orc.evt_decode(fmt, words)
    _same(whole, placed)
    for part in _cuts(words):
        _check_oracle(orc, fmt, part)
    if len(words) <= CUT:
        _same(spec.decode(fmt, words), placed)


@pytest.mark.parametrize("name", list(es.DENSE))
def test_oracle_matches_spec_on_dense_streams(orc, name):
    fmt, build = es.DENSE[name]
    words = build()
    for part in _cuts(words):
        _check_oracle(orc, fmt, part)


def test_oracle_matches_spec_on_group_junk_ends(orc):
    """The first and last 20 000 words of the junk streams that cross the group boundary on
    the GPU."""
    for fmt in (2, 3):
        words = es.junk(fmt, 513 * es.CHUNK[fmt] + 77, seed=40 + fmt)
        for part in _cuts(words):
            _check_oracle(orc, fmt, part)


def test_spec_known_words():
    """The plain decoder on the words of include/ecc.h §8, by hand (no oracle)."""
    w3 = [es.time_high(1), es.time_low(0x23), es.addr_y(17), es.addr_x(5, 1), 0xA0FF, es.vect_base_x(2040, 0),
          es.vect_12(0b100000000101), es.vect_8(0b10000001), es.addr_x(7, 0), es.time_high(0), es.addr_x(9, 0),
          0x7123, 0xF456, 0x1000, 0x9000, 0xB000, 0xC000, 0xD000, es.addr_x(1, 1)]
    xy, t, p = spec.decode_evt3(np.array(w3, np.uint16))
    assert list(xy & 0xFFFF) == [5, 2040, 2042, 2051, 2052, 2059, 7, 9, 1] and (xy >> 16 == 17).all()
    assert list(p) == [1, 0, 0, 0, 0, 0, 0, 0, 1]
    assert list(t) == [1 << 12 | 0x23] * 7 + [1 << 24 | 0x23] * 2
    # an x that passes 2^16 is masked only when packed
    run = [es.vect_base_x(2047, 1)] + [es.vect_12(0)] * 5290 + [es.vect_12(1 << 11)] * 2
    xy, t, p = spec.decode_evt3(np.array(run, np.uint16))
    assert [int(v) for v in xy] == [(2047 + 12 * 5290 + 11) & 0xFFFF, (2047 + 12 * 5291 + 11) & 0xFFFF] == [2, 14]
    w2 = [1 << 28 | 5 << 22 | 3 << 11 | 4, 0x8 << 28 | 0x0FFFFFFF, 63 << 22 | 2047 << 11 | 2047, 0xE << 28 | 12345,
          0xA << 28, 0xF << 28 | 1, 0x2 << 28 | 1, 0x7 << 28 | 1, 0x9 << 28 | 1]
    xy, t, p = spec.decode_evt2(np.array(w2, np.uint32))
    assert list(xy) == [3 | 4 << 16, 2047 | 2047 << 16] and list(p) == [1, 0]
    assert list(t) == [5, 0x0FFFFFFF << 6 | 63]


@pytest.mark.parametrize("fmt", [2, 3])
def test_raw_writer_matches_spec(ecc, fmt):
    """Product RAW writer (ecc_evt_encode) -> the plain decoder == the events."""
    ev = concat(events_random(4000, 51, t_span=1 << 27), _first(events_rows(400, 52), 2000))
    words = ecc.evt_encode(fmt, *ev)
    assert len(words) <= spec.MAX_WORDS
    _same(spec.decode(fmt, words), ev)
    if fmt == 3:
        assert ((words >> 12) == 4).sum() > 50 and ev[1].max() >> 24 >= 4
