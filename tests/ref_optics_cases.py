"""Shared by tests/test_ref_optics.py and tests/test_gpu_ref_optics.py: the point sets of the OPTICS
pins and the reference's own answers to them.

The answers come from oracle/_ref/ref_optics — the reference's OPTICS code (ordering, threshold and
xi extraction, cluster tree, kd-tree, the event driver's statistics loop) compiled from the
reference tree by oracle/ref/Makefile — when that binary is built, and from
tests/golden/ref_cpu/optics_<case>.npz where it is not; the plumbing (input digest, recording with
ECC_RECORD_REF_GOLDEN=1, "with neither present a test fails") is that of tests/ref_cpu_cases.py.

A fixture keeps reach as the int32 SQUARE of each value (-1 for undefined): every point here is an
integer pixel, so a reach is the double square root of an integer.  The loader takes the square
roots and accepts them only if their bytes hash to the recorded digest of the reference's reach.
The statistics and the forests of the 8192-point cases are kept as their digests alone."""
import json
from pathlib import Path

import numpy as np

import ref_cpu_cases as rc

REF_OPTICS = rc.ROOT / "oracle" / "_ref" / "ref_optics"
GOLDEN = Path(__file__).resolve().parent / "golden"
XI_PARAMS = ((0.1, 4, 0.0), (0.02, 5, 0.15), (0.25, 2, 0.0))
BLOBS_MIN_PTS = (8, 9, 16, 17, 32, 33, 64)
W, H = 346, 260

# name -> (point set, eps, min_pts, threshold, what the expansion loop is fed)
CASES = {
    "kat1": ("kat1", 10.0, 2, 10.0, "ball"),
    "kat2": ("kat2", None, 2, 2.0, "ball"),       # eps -1 in the reference's test: estimated, see case()
    "event_csv": ("event_csv", 10.0, 2, 10.0, "ball"),
    "event_csv_e2": ("event_csv", 2.0, 2, 2.0, "ball"),
    "ties": ("ties", 10.0, 2, 10.0, "ball"),
    "ties_e2": ("ties", 2.0, 3, 2.0, "ball"),
    "kdtree": ("kdtree", 10.5, 2, 10.0, "kdtree"),
    **{f"blobs_mp{m}": ("blobs", 3.7, m, 2.5, "kdtree") for m in BLOBS_MIN_PTS},
    "full": ("full", 10.0, 2, 10.0, "ball"),
    "full_e2": ("full", 2.0, 2, 2.0, "ball"),
    "noise": ("noise", 2.0, 2, 2.0, "ball"),
    "noise_e10": ("noise", 10.0, 2, 10.0, "ball"),
}
SMALL = [c for c in CASES if CASES[c][0] not in ("full", "noise")]
_points, _answers = {}, {}


def points(ecc, name):
    """The point set `name` as int32 (n, 2).  Only the two KAT sets hold negative coordinates."""
    if name in _points:
        return _points[name]
    if name in ("kat1", "kat2"):
        kat = json.loads((GOLDEN / "optics_kat.json").read_text())[f"clustering_test_{name[-1]}"]
        p = np.asarray(kat["points"])
        assert (p == np.rint(p)).all()
    elif name == "event_csv":
        xy, _, _ = ecc.read_csv(str(GOLDEN / "event_raw_data8.csv"))
        p = np.stack(ecc.unpack_xy(xy), 1)
        assert len(p) == 320
    elif name == "ties":       # 600 draws from 900 pixels: duplicates and equal distances everywhere
        p = np.random.default_rng(67).integers(0, 30, (600, 2))
    elif name == "kdtree":
        rng = np.random.default_rng(492)
        p = np.stack([rng.integers(0, 120, 600), rng.integers(0, 90, 600)], 1)
    elif name == "blobs":      # three rounded Gaussian blobs (750 points) under 274 uniform ones, shuffled
        rng = np.random.default_rng(37)
        bx = np.concatenate([rng.normal(60, 4, 300), rng.normal(90, 6, 300), rng.normal(200, 3, 150), rng.uniform(0, W, 274)])
        by = np.concatenate([rng.normal(60, 4, 300), rng.normal(70, 6, 300), rng.normal(30, 3, 150), rng.uniform(0, H, 274)])
        p = np.stack([np.clip(np.rint(bx), 0, W - 1), np.clip(np.rint(by), 0, H - 1)], 1)[rng.permutation(1024)]
    elif name == "full":       # one window at capacity: 8192 distinct pixels of the frame
        q = np.random.default_rng(8192).choice(W * H, 8192, replace=False)
        p = np.stack([q % W, q // W], 1)
    elif name == "noise":      # a 128 x 64 lattice of spacing 3: at eps 2 no point has a neighbour
        q = np.random.default_rng(3).permutation(8192)
        p = np.stack([3 * (q % 128), 3 * (q // 128)], 1)
    else:
        raise KeyError(name)
    _points[name] = np.ascontiguousarray(p, np.int32)
    return _points[name]


def case(ecc, orc, name):
    """-> (points int32 (n, 2), eps, min_pts, threshold, feed)."""
    pts_name, eps, min_pts, thr, feed = CASES[name]
    p = points(ecc, pts_name)
    if eps is None:  # the estimate (optics.hpp:340-387) is outside the compiled spans: the oracle's value is passed
        eps = orc.epsilon_estimation(p.astype(np.float64), min_pts)
    return p, float(eps), min_pts, float(thr), feed


def shift(p):
    """Points moved to non-negative coordinates (packed u16 inputs); OPTICS sees differences only."""
    return p - np.minimum(p.min(0), 0)


def _squares(reach):
    r2 = np.rint(reach * reach).astype(np.int64)
    r2[reach < 0] = -1
    return r2


def _roots(r2):
    reach = np.sqrt(np.maximum(r2, 0).astype(np.float64))
    reach[r2 < 0] = -1.0
    return reach


def _store(res):
    out = dict(res)
    reach = out.pop("reach.f64")
    r2 = _squares(reach)
    assert _roots(r2).tobytes() == reach.tobytes() and r2.max() < 2 ** 31, "a reach is no square root of an int32"
    out["reach2.i32"] = r2.astype(np.int32)
    out["reach_sha"] = np.array(rc.sha(reach))
    return out


def _restore(kept):
    out = dict(kept)
    reach = _roots(out.pop("reach2.i32").astype(np.int64))
    assert rc.sha(reach) == str(out.pop("reach_sha")), "the stored squares do not reproduce the recorded reach"
    out["reach.f64"] = reach
    return out


def reference(ecc, orc, tmp_path, name):
    """The reference's answers to case `name`: dict(order int32[n], reach float64[n], differing (kd-tree
    sets that are not the exact ball), sizes (of the threshold clusters, in plot order), xi (per XI_PARAMS
    an int32 (k, 2) array), forest / forest_sha (per XI_PARAMS an int32 (k, 3) array of depth-first (level,
    first, second)), stats / stats_sha (uint64 (m, 5): size and the bits of two centroids and two variances, for
    the threshold clusters and then every xi list's pairs))."""
    if name in _answers:
        return _answers[name]
    p, eps, min_pts, thr, feed = case(ecc, orc, name)
    outputs = {"order.i32": np.int32, "reach.f64": np.float64, "meta.i32": np.int32, "sizes.i32": np.int32,
               "xi.i32": np.int32, "forest.i32": np.int32, "stats.u64": np.uint64}
    xi = ";".join(f"{c!r},{m},{s!r}" for c, m, s in XI_PARAMS)
    r = rc._ref(f"optics_{name}", tmp_path, "run", {"pts.i32": p},
                ["pts.i32", len(p), repr(eps), min_pts, repr(thr), feed, xi] + list(outputs), outputs,
                digest_only=("stats.u64", "forest.i32") if len(p) == 8192 else (), exe=REF_OPTICS, store=_store,
                restore=_restore)
    ans = dict(order=r["order.i32"], reach=r["reach.f64"], differing=int(r["meta.i32"][0]), sizes=r["sizes.i32"],
               xi=rc.unpack_lists(r["xi.i32"], 2))
    assert int(r["meta.i32"][1]) == len(ans["sizes"]) and int(ans["sizes"].sum()) == len(p)
    if "stats.u64" in r:
        ans["stats"] = r["stats.u64"].reshape(-1, 5)
    ans["stats_sha"] = str(r["stats.u64_sha"]) if "stats.u64_sha" in r else rc.sha(r["stats.u64"])
    if "forest.i32" in r:
        ans["forest"] = rc.unpack_lists(r["forest.i32"], 3)
        assert len(ans["forest"]) == len(XI_PARAMS)
    ans["forest_sha"] = str(r["forest.i32_sha"]) if "forest.i32_sha" in r else rc.sha(r["forest.i32"])
    assert len(ans["xi"]) == len(XI_PARAMS)
    _answers[name] = ans
    return ans


def same_stats(ref, got):
    """The reference's statistics against `got` (uint64 (m, 5)), whichever form is at hand."""
    got = np.ascontiguousarray(got, np.uint64).reshape(-1)
    if "stats" in ref and not np.array_equal(ref["stats"].reshape(-1), got):
        return False
    return ref["stats_sha"] == rc.sha(got)


def same_forest(ref, lists):
    """The reference's forests against `lists` (per XI_PARAMS the depth-first (level, first, second) rows)."""
    lists = [np.asarray(l, np.int32).reshape(-1, 3) for l in lists]
    if "forest" in ref and not rc.same_lists(ref["forest"], lists):
        return False
    return ref["forest_sha"] == rc.sha(rc.pack_lists(lists, 3))


def intervals(ref):
    """Every interval whose statistics the reference lists, in its order: the threshold clusters' runs,
    then each xi list's pairs."""
    starts = np.concatenate([[0], np.cumsum(ref["sizes"])]).astype(np.int64)
    out = [(int(b), int(e) - 1) for b, e in zip(starts[:-1], starts[1:])]
    for pairs in ref["xi"]:
        out += [(int(b), int(e)) for b, e in pairs]
    return out


def stat_words(recs):
    """CLUSTER_STAT_DTYPE / cluster_stats_ref.STAT_DTYPE records -> uint64 (m, 5) as the reference run writes them."""
    return np.stack([recs["size"].astype(np.uint64), recs["cx"].view(np.uint64), recs["cy"].view(np.uint64),
                     recs["vx"].view(np.uint64), recs["vy"].view(np.uint64)], 1).reshape(-1, 5)


def cluster_ids(sizes):
    return np.repeat(np.arange(len(sizes), dtype=np.int32), sizes)
