"""bench.py's plain run, `--full` and `--dump-outputs`.

CPU: the options parse, `--dist-parity` is refused without `--full`, and `dump_outputs` writes
float32 / float64 arrays under 64 MB, identical from call to call (fixed seeded sample).
GPU: a plain run prints only the headline keys and its dumped outputs equal the oracle's over the
same seeded events (the whole arrays, and the sampled ones at the sampled indices).
"""
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
SLICE, WINDOW, CAP = 16384, 8192, 4096
FULL_ONLY = ("roofline", "stages", "stages_ms_per_step", "tracker", "track_merge", "per_gpu_rate_n1",
             "dist_parity", "ingest", "eps", "kmeans_c3", "cpu_baseline", "parity")


def _bench():
    sys.path.insert(0, str(ROOT))
    import bench
    return bench


def test_full_and_dump_options_parse():
    bench = _bench()
    a = bench.parse(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert (a.full, a.dump_outputs, a.steps, a.warmup) == (False, None, 7, 2)
    a = bench.parse(["--full", "--dump-outputs", "d", "--dist-parity"])
    assert a.full and a.dump_outputs == "d" and a.dist_parity
    for bad in (["--dist-parity"], ["--steps", "0"], ["--warmup", "-1"]):
        with pytest.raises(SystemExit):
            bench.parse(bad)


class _Host:
    def __init__(self, a):
        self.a = a

    def numpy(self):
        return self.a


def test_dump_outputs_format_and_determinism(ecc, tmp_path):
    """At the benchmark's own size (20 M events): every file float32 / float64, under 64 MB in all,
    the same bytes from two calls, and slots past a window's count masked to -1."""
    bench = _bench()
    n = 1221 * SLICE
    nw, ns = n // WINDOW, n // SLICE
    rng = np.random.default_rng(3)
    u = rng.integers(0, WINDOW + 1, nw).astype(np.int32)
    cnt = rng.integers(0, CAP + 1, ns).astype(np.int32)  # more rows than the sample holds
    nms = np.zeros(ns * CAP, ecc.CORNER_DTYPE)
    nms["x"] = np.arange(ns * CAP) % 346
    g = dict(rep_xy=_Host(ecc.pack_xy(rng.integers(0, 346, nw * WINDOW), rng.integers(0, 260, nw * WINDOW))),
             uniq=_Host(u), rep=_Host(WINDOW - u), c=_Host(rng.random(32).astype(np.float32)),
             labels=_Host(rng.integers(0, 16, nw * WINDOW).astype(np.uint8)),
             flags=_Host((rng.random(n) < 0.03).astype(np.uint8)), sae=_Host(rng.integers(0, 2 ** 40, 346 * 260)),
             nms_out=_Host(nms), nms_cnt=_Host(cnt), cap=CAP)
    for d in ("a", "b"):
        bench.dump_outputs(ecc, tmp_path / d, 0, g)
    files = sorted((tmp_path / "a").glob("*.npy"))
    assert len(files) == 10 and sum(f.stat().st_size for f in files) <= 64 * 2 ** 20
    for f in files:
        a = np.load(f)
        assert a.dtype in (np.float32, np.float64), f.name
        assert f.read_bytes() == (tmp_path / "b" / f.name).read_bytes(), f.name
    assert np.array_equal(np.load(tmp_path / "a" / "sae.npy"), g["sae"].a.astype(np.float64))
    lab = np.load(tmp_path / "a" / "kmeans_labels_sample.npy")
    xy = np.load(tmp_path / "a" / "downsample_rep_xy_sample.npy")
    assert lab.shape == (1_500_000,) and xy.shape == (1_500_000, 2)
    assert ((lab == -1) == (xy[:, 0] == -1)).all() and 0 < (lab == -1).sum() < lab.size
    assert len(np.load(tmp_path / "a" / "nms_corners.npy")) == 1_500_000
    assert np.load(tmp_path / "a" / "corner_flags_per_slice.npy").sum() == g["flags"].a.sum()


@pytest.mark.gpu
def test_plain_run_headline_and_dumped_outputs_match_oracle(ecc, orc, tmp_path):
    n, W, H, K = SLICE * 12, 346, 260, 16
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "3", "--warmup", "1", "--events", str(n),
                        "--dump-outputs", str(tmp_path)], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
    line = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert line["metric"] == "Mevents/s (downsample+cluster+corner)" and line["unit"] == "Mevents/s"
    assert line["higher_is_better"] is True and line["steps"] == 3 and line["full"] is False
    assert line["ms_per_step"] > 0 and line["value"] == pytest.approx(n / line["ms_per_step"] / 1e3, rel=0.02)
    assert not [k for k in FULL_ONLY if k in line]

    xy, t, _ = ecc.gen_events(n, seed=1, width=W, height=H)
    o_rx, _, o_u, o_r = orc.downsample_hash(xy)
    dense = np.concatenate([o_rx[w * WINDOW: w * WINDOW + o_u[w]] for w in range(len(o_u))])
    c0 = np.stack([np.linspace(20, W - 20, K), np.linspace(20, H - 20, K)[::-1]], 1).astype(np.float32).ravel()
    o_c, o_lab, _ = orc.kmeans_run_xy16(dense, c0, 10)
    o_flags, o_sae = orc.fast_detect(xy, t, W, H)
    o_out, o_cnt, _ = orc.corner_nms(xy, o_flags, W, H, cap=CAP)
    ld = lambda name: np.load(tmp_path / f"{name}.npy")
    assert np.array_equal(ld("downsample_unique_per_window"), o_u) and np.array_equal(ld("downsample_rep_per_window"), o_r)
    assert np.array_equal(ld("kmeans_centroids").view(np.uint32), o_c.view(np.uint32))
    assert np.array_equal(ld("sae"), o_sae.astype(np.float64))
    assert np.array_equal(ld("nms_count_per_slice"), o_cnt)
    # below the sample size the per-event and per-slot arrays are written whole
    assert np.array_equal(ld("corner_flags_sample"), o_flags)
    assert np.array_equal(ld("corner_flags_per_slice"), o_flags.reshape(-1, SLICE).sum(1))
    lab = ld("kmeans_labels_sample").reshape(-1, WINDOW)
    assert np.array_equal(np.concatenate([lab[w, :o_u[w]] for w in range(len(o_u))]), o_lab)
    assert all((lab[w, o_u[w]:] == -1).all() for w in range(len(o_u)))
    rxy = ld("downsample_rep_xy_sample").reshape(-1, WINDOW, 2)
    ox, oy = ecc.unpack_xy(dense)
    g_dense = np.concatenate([rxy[w, :o_u[w]] for w in range(len(o_u))])
    assert np.array_equal(g_dense, np.stack([ox, oy], 1))
    oo = np.asarray(o_out).view(np.int32).reshape(-1, CAP, 3)
    assert np.array_equal(ld("nms_corners"), np.concatenate([oo[s, :o_cnt[s]] for s in range(len(o_cnt))]))
