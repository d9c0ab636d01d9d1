"""A plain EVT 2.0 / EVT 3.0 decoder written from the word tables of include/ecc.h §8 (and the
header comments of csrc/evt.hip), the comparator that keeps the oracle's decoder from checking
itself.  One Python loop per word, Python integers (no width limits anywhere): a vector base
that grows past 2^16, a loop count or a time-high are never truncated here, and the only mask
beyond the field extraction is the one the ABI states, xy = (x & 0xFFFF) | y << 16.

EVT 3.0 (16-bit words, type = w >> 12):
  0x0 ADDR_Y       y = w & 0x7FF
  0x2 ADDR_X       one event at x = w & 0x7FF, p = bit 11
  0x3 VECT_BASE_X  base = w & 0x7FF, vector polarity = bit 11
  0x4 VECT_12      one event per set bit b of w & 0xFFF at x = base + b; then base += 12
  0x5 VECT_8       one event per set bit b of w & 0xFF at x = base + b; then base += 8
  0x6 TIME_LOW     tl = w & 0xFFF
  0x8 TIME_HIGH    th = w & 0xFFF; a value below the previous TIME_HIGH is one more loop
  anything else    no CD event, no state
  t = loops << 24 | th << 12 | tl; everything is 0 before the first word that sets it.

EVT 2.0 (32-bit words, type = w >> 28):
  0x0 CD_OFF / 0x1 CD_ON  one event: x = w >> 11 & 0x7FF, y = w & 0x7FF, p = type,
                          t = th << 6 | (w >> 22 & 0x3F)
  0x8 TIME_HIGH           th = w & 0x0FFFFFFF
  anything else           no CD event, no state

Only run on streams of at most 50 000 words."""
import numpy as np

MAX_WORDS = 50_000


def _arrays(xy, t, p):
    return np.array(xy, np.uint32), np.array(t, np.int64), np.array(p, np.uint8)


def decode_evt2(words):
    assert len(words) <= MAX_WORDS
    xy, t, p = [], [], []
    th = 0
    for w in (int(v) for v in words):
        ty = w >> 28
        if ty in (0x0, 0x1):
            x, y = (w >> 11) & 0x7FF, w & 0x7FF
            xy.append((x & 0xFFFF) | (y << 16))
            t.append((th << 6) | ((w >> 22) & 0x3F))
            p.append(ty)
        elif ty == 0x8:
            th = w & 0x0FFFFFFF
    return _arrays(xy, t, p)


def decode_evt3(words):
    assert len(words) <= MAX_WORDS
    xy, t, p = [], [], []
    y = tl = th = loops = base = pol = 0
    seen_th = False

    def emit(x, pp):
        xy.append((x & 0xFFFF) | (y << 16))
        t.append((loops << 24) | (th << 12) | tl)
        p.append(pp)

    for w in (int(v) for v in words):
        ty = w >> 12
        if ty == 0x0:
            y = w & 0x7FF
        elif ty == 0x2:
            emit(w & 0x7FF, (w >> 11) & 1)
        elif ty == 0x3:
            base, pol = w & 0x7FF, (w >> 11) & 1
        elif ty in (0x4, 0x5):
            width = 12 if ty == 0x4 else 8
            for b in range(width):
                if (w >> b) & 1:
                    emit(base + b, pol)
            base += width
        elif ty == 0x6:
            tl = w & 0xFFF
        elif ty == 0x8:
            v = w & 0xFFF
            if seen_th and v < th:
                loops += 1
            th, seen_th = v, True
    return _arrays(xy, t, p)


def decode(fmt, words):
    return decode_evt2(words) if fmt == 2 else decode_evt3(words)
