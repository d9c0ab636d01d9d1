"""A guarded device view for the extent tests (tests/test_gpu_extents.py).

One device allocation laid out as

    [ front guard | skew | payload | tail | back guard ]

and duck-typed for the eccpy wrappers (.ptr, .nbytes, .dtype, .shape, .numpy(), int()).  Both
guards hold GUARD_ELEMS elements of the buffer's type filled with FILL: 16384 is the largest
window, slice or segment any entry point accepts, so an index that is off by a whole window still
lands in a guard instead of in another allocation.

placement "aligned": the payload starts on a 256-B boundary (what hipMalloc hands out);
placement "bare":    the payload starts at exactly its element type's natural alignment and no
                     more: 4 mod 16 for 4-byte elements (and ecc_corner), 8 mod 16 for 8-byte
                     elements, 1 mod 4 for bytes.  `skew` overrides the byte offset from the
                     256-B boundary (the float k-means documents 8 mod 16 and 0 mod 16).

Outputs: the payload is FILL as well and there is no tail, so entries the entry point leaves
unwritten stay recognisable.  Inputs: the caller gives the payload and a hostile tail; check()
compares the whole input with what was uploaded (a `const` input that gets written is caught by
that comparison).  In/out buffers (sae, centroids) are made with check_data=False.
"""
import numpy as np

GUARD_ELEMS = 16384
FILL = 0xA5
_ALIGN = 256


def bare_skew(dtype) -> int:
    """Byte offset from a 256-B boundary that leaves exactly the type's natural alignment."""
    dtype = np.dtype(dtype)
    if dtype.fields is not None:  # ecc_corner: three int32
        return 4
    return {1: 1, 2: 2, 4: 4, 8: 8}[dtype.itemsize]


class Guarded:
    def __init__(self, ecc, dtype, n, placement="aligned", data=None, tail=None, skew=None, check_data=True):
        self._ecc = ecc
        self.dtype = np.dtype(dtype)
        self.shape = (int(n),)
        it = self.dtype.itemsize
        self.nbytes = int(n) * it
        tail_b = b"" if tail is None else np.ascontiguousarray(tail, self.dtype).tobytes()
        if skew is None:
            skew = 0 if placement == "aligned" else bare_skew(self.dtype)
        self.placement, self.skew = placement, int(skew)
        self._guard = GUARD_ELEMS * it
        self._span = self.nbytes + len(tail_b)  # payload + tail
        self._total = self._guard + 2 * _ALIGN + self._span + self._guard + 16
        self._base = ecc.DeviceArray(self._total, np.uint8)
        first = self._base.ptr + self._guard
        self.ptr = (first + _ALIGN - 1) // _ALIGN * _ALIGN + self.skew
        self._off = self.ptr - self._base.ptr  # everything before the payload is front guard
        img = np.full(self._total, FILL, np.uint8)
        if data is not None:
            d = np.ascontiguousarray(data, self.dtype)
            assert d.size == n, (d.size, n)
            img[self._off:self._off + self.nbytes] = np.frombuffer(d.tobytes(), np.uint8)
        if tail_b:
            img[self._off + self.nbytes:self._off + self._span] = np.frombuffer(tail_b, np.uint8)
        self._image = img
        self._is_input = data is not None and check_data
        ecc.check(ecc.lib.ecc_memcpy_h2d(self._base.ptr, img.ctypes.data, self._total, None), "h2d")
        ecc.check(ecc.lib.ecc_stream_sync(None))

    def __int__(self):
        return self.ptr

    def _download(self):
        return self._base.numpy()  # waits for all device work first

    def numpy(self, stream=None):
        raw = self._download()[self._off:self._off + self.nbytes]
        return np.frombuffer(raw.tobytes(), self.dtype).copy()

    def damage(self):
        """First damaged byte offset relative to the payload start (negative: front guard; from
        nbytes on: tail or back guard), or None.  The payload of an output is not looked at."""
        got = self._download()
        lo, hi = self._off, self._off + self._span
        bad = np.nonzero(got[:lo] != FILL)[0]
        if len(bad):
            return int(bad[-1]) - lo  # the damaged byte nearest the payload
        if self._is_input:
            bad = np.nonzero(got[lo:hi] != self._image[lo:hi])[0]
            if len(bad):
                return int(bad[0])
        else:  # a tail of an in/out buffer is input all the same
            bad = np.nonzero(got[lo + self.nbytes:hi] != self._image[lo + self.nbytes:hi])[0]
            if len(bad):
                return self.nbytes + int(bad[0])
        bad = np.nonzero(got[hi:] != FILL)[0]
        if len(bad):
            return self._span + int(bad[0])
        return None

    def check(self, name="buffer"):
        d = self.damage()
        assert d is None, (f"{name} ({self.dtype}, {self.shape[0]} elements, {self.placement}): byte at payload offset "
                           f"{d} was written outside the documented extent" if (d < 0 or d >= self.nbytes) else
                           f"{name}: const input changed at payload byte offset {d}")

    def untouched(self):
        """Output payload as bytes == FILL mask (True where the entry point wrote nothing)."""
        raw = self._download()[self._off:self._off + self.nbytes]
        return raw == FILL


def guarded_in(ecc, data, placement, tail=None, skew=None, dtype=None):
    data = np.ascontiguousarray(data, dtype)
    return Guarded(ecc, data.dtype, data.size, placement, data=data.ravel(), tail=tail, skew=skew)


def guarded_inout(ecc, data, placement, tail=None, skew=None):
    data = np.ascontiguousarray(data)
    return Guarded(ecc, data.dtype, data.size, placement, data=data.ravel(), tail=tail, skew=skew, check_data=False)


def guarded_out(ecc, dtype, n, placement, skew=None):
    return Guarded(ecc, dtype, n, placement, skew=skew)


def check_all(**bufs):
    for name, b in bufs.items():
        if b is not None:
            b.check(name)
