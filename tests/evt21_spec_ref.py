"""A plain EVT 2.1 decoder written from the word table of include/ecc.h §8, the comparator of the
HIP decoder (the oracle has no EVT 2.1).  Parity against OpenEB, and the half order of the legacy
layout, are unpinned: this is the project's restatement of the published format.

EVT 2.1 (64-bit little-endian words, type = w >> 60):
  0x0 EVT_NEG / 0x1 EVT_POS  ts6 = w >> 54 & 0x3F, x = w >> 43 & 0x7FF, y = w >> 32 & 0x7FF,
                             valid = w & 0xFFFFFFFF; one event per set bit b, in ascending b:
                             xy = ((x + b) & 0xFFFF) | y << 16, t = th << 6 | ts6, p = type
  0x8 EVT_TIME_HIGH          th = w >> 32 & 0x0FFFFFFF (0 before the first one)
  anything else              no CD event, no state
legacy=True: the two 32-bit halves of every stored word are exchanged, w = lo << 32 | hi.

decode_evt21 is one Python loop per word on Python integers, for at most 50 000 words;
decode_evt21_np is the vectorised form for large streams, held equal to the loop by
tests/test_evt21.py."""
import numpy as np

MAX_WORDS = 50_000
LANE, WAVE, CHUNK, GROUP = 8, 512, 2048, 512 * 2048  # the HIP decoder's scan boundaries, in words


def _arrays(xy, t, p):
    return np.array(xy, np.uint32), np.array(t, np.int64), np.array(p, np.uint8)


def decode_evt21(words, legacy=False):
    assert len(words) <= MAX_WORDS
    xy, t, p = [], [], []
    th = 0
    for w in (int(v) for v in words):
        if legacy:
            w = ((w & 0xFFFFFFFF) << 32) | (w >> 32)
        ty = w >> 60
        if ty in (0x0, 0x1):
            ts6, x, y, valid = (w >> 54) & 0x3F, (w >> 43) & 0x7FF, (w >> 32) & 0x7FF, w & 0xFFFFFFFF
            for b in range(32):
                if (valid >> b) & 1:
                    xy.append(((x + b) & 0xFFFF) | (y << 16))
                    t.append((th << 6) | ts6)
                    p.append(ty)
        elif ty == 0x8:
            th = (w >> 32) & 0x0FFFFFFF
    return _arrays(xy, t, p)


def decode_evt21_np(words, legacy=False):
    w = np.ascontiguousarray(words, np.uint64)
    if legacy:
        w = (w << np.uint64(32)) | (w >> np.uint64(32))
    ty = (w >> np.uint64(60)).astype(np.int64)
    hi = (w >> np.uint64(32)).astype(np.int64)
    # running TIME_HIGH by forward fill: the index of the last type-8 word at or before each word
    idx = np.where(ty == 8, np.arange(len(w)), -1)
    last = np.maximum.accumulate(idx) if len(w) else idx
    th = np.where(last >= 0, hi[np.maximum(last, 0)] & 0x0FFFFFFF, 0)
    cd = ty <= 1
    wc, hc, thc = w[cd], hi[cd], th[cd]
    masks = (wc & np.uint64(0xFFFFFFFF)).astype("<u4")
    bits = np.unpackbits(masks.view(np.uint8).reshape(-1, 4), axis=1, bitorder="little")  # [word, b]
    cnt = bits.sum(axis=1).astype(np.int64)
    b = np.nonzero(bits)[1].astype(np.int64)
    rep = lambda a: np.repeat(a, cnt)
    x, y = rep((hc >> 11) & 0x7FF), rep(hc & 0x7FF)
    xy = (((x + b) & 0xFFFF) | (y << 16)).astype(np.uint32)
    t = ((rep(thc) << 6) | rep((hc >> 22) & 0x3F)).astype(np.int64)
    return xy, t, rep(hc >> 28).astype(np.uint8)


def decode(fmt, words):
    """fmt 21 or 22 (legacy); the loop form up to MAX_WORDS, the numpy form beyond."""
    f = decode_evt21 if len(words) <= MAX_WORDS else decode_evt21_np
    return f(words, legacy=fmt == 22)


# ---- word builders ----------------------------------------------------------------------------
def cd(p, ts6, x, y, mask):
    return (p << 60) | (ts6 << 54) | (x << 43) | (y << 32) | mask


def time_high(th):
    return (0x8 << 60) | (th << 32)


def swap_halves(words):
    w = np.asarray(words, np.uint64)
    return (w << np.uint64(32)) | (w >> np.uint64(32))


def junk(n, seed):
    """n uniform random 64-bit words (about 1 in 8 a CD word, 16 events each on average)."""
    return np.random.default_rng(seed).integers(0, 1 << 64, n, dtype=np.uint64)


def sparse(n, seed, p_cd=0.85, p_th=0.1, max_bits=3):
    """A file-like stream: CD words with 1 .. max_bits events, rising TIME_HIGHs, a few others."""
    rng = np.random.default_rng(seed)
    u = lambda lo, hi: rng.integers(lo, hi, n, dtype=np.uint64)
    sh = lambda a, k: a << np.uint64(k)
    kind = rng.random(n)
    th = np.cumsum(u(0, 3)) & np.uint64(0x0FFFFFFF)
    mask = sh(np.uint64(1), 0) << u(0, 32)
    for _ in range(max_bits - 1):
        mask |= (np.uint64(1) << u(0, 32)) * (rng.random(n) < 0.6).astype(np.uint64)
    cdw = sh(u(0, 2), 60) | sh(u(0, 64), 54) | sh(u(0, 40) * np.uint64(32), 43) | sh(u(0, 720), 32) | mask
    other = sh(rng.choice(np.array([0xA, 0xE, 0xF, 0x3], np.uint64), n), 60) | u(0, 1 << 60)
    return np.where(kind < p_cd, cdw, np.where(kind < p_cd + p_th, sh(np.uint64(8), 60) | sh(th, 32), other))
