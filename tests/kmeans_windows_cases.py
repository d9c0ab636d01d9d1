"""Inputs and oracle results shared by the ecc_kmeans_windows_xy16 tests: windows of Gaussian blobs
on a 346x260 frame in the downsample layout, the regular-grid starting centres, and the expected
values, which are orc.kmeans_run_xy16 on each window's points alone."""
import numpy as np

W, H = 346, 260
RAGGED_COUNTS = [0, 1, 63, 64, 65, 255, 256, 257, 1000, 1023, 1024, 1025, 2048, -7]  # the last: clamped to empty
RAGGED_STRIDE = 2048
RAGGED = dict(k=16, thr=20.0, tol=0.01, max_iters=25)
SEED = 20261020
PAD_XY = 0xDEADBEEF  # slots past a window's count


def grid_init(k, w=W, h=H):
    """k centres on a g x g grid over the frame, g = ceil(sqrt(k)): float32[2k]."""
    g = int(np.ceil(np.sqrt(k)))
    i = np.arange(k)
    return np.stack([(i % g + 0.5) * w / g, (i // g + 0.5) * h / g], 1).astype(np.float32).ravel()


def blob_window(rng, n):
    """n packed points: 3-7 blobs of sigma 9 plus about 3 % uniform noise."""
    nb = int(rng.integers(3, 8))
    cx, cy = rng.uniform(15, W - 15, nb), rng.uniform(15, H - 15, nb)
    b = rng.integers(0, nb, n)
    x, y = rng.normal(cx[b], 9.0), rng.normal(cy[b], 9.0)
    noise = rng.random(n) < 0.03
    x = np.where(noise, rng.uniform(0, W, n), x)
    y = np.where(noise, rng.uniform(0, H, n), y)
    x = np.clip(np.rint(x), 0, W - 1).astype(np.uint32)
    y = np.clip(np.rint(y), 0, H - 1).astype(np.uint32)
    return x | (y << 16)


def layout(windows, stride, tail=0):
    """Windows (arrays of packed points) at w * stride, PAD_XY elsewhere; `tail` further slots."""
    xy = np.full(len(windows) * stride + tail, PAD_XY, np.uint32)
    for w, p in enumerate(windows):
        assert len(p) <= stride
        xy[w * stride: w * stride + len(p)] = p
    return xy


def ragged_windows():
    rng = np.random.default_rng(SEED)
    return [blob_window(rng, max(c, 0)) for c in RAGGED_COUNTS]


class Want:
    """The oracle per window: centroids float32[n, 2k], labels (one array per window), sizes
    int32[n, k] (bincount of the oracle's labels), iters int32[n]."""

    def __init__(self, orc, windows, starts, max_iters, thr, tol):
        starts = np.asarray(starts, np.float32)
        self.n = len(windows)
        if starts.ndim == 1:
            starts = np.broadcast_to(starts, (self.n, starts.size))
        self.k = starts.shape[1] // 2
        self.cent = np.zeros((self.n, 2 * self.k), np.float32)
        self.labels, self.sizes, self.iters = [], np.zeros((self.n, self.k), np.int32), np.zeros(self.n, np.int32)
        for w, p in enumerate(windows):
            c, lab, it = orc.kmeans_run_xy16(p, starts[w], max_iters, thr, tol)
            self.cent[w], self.iters[w] = c, it
            self.labels.append(lab)
            self.sizes[w] = np.bincount(lab[lab != 255], minlength=self.k)[:self.k]
