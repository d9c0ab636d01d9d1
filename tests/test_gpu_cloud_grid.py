"""The cloud cell grid (csrc/radius_grid.hpp over csrc/grid_geometry.hpp) on geometry that is not a
friendly box: every any-size point-cloud entry point — ecc_radius_counts / ecc_radius_lists (f32
and f64), ecc_dbscan_cloud (f32 and f64), ecc_optics_f64 — against a brute-force reference in the
reference's operation order, at 1, 2 and 3 dimensions.  Every comparison is exact: counts and
indices as integers, distances and core distances bit for bit.

References: orc.radius_f32 (float differences, widened), a numpy brute force for f64 (as
_brute_ball of test_gpu_parity.py), orc.dbscan_cloud, orc.optics.

`expected_doublings` restates the sizing rule of the grid in plain Python; the cases meant to
make the cell double (or not) assert that about their own INPUT with it.
"""
import functools
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
TYPES = [F32, F64]
TD = [(t, d) for t in TYPES for d in (1, 2, 3)]
TD_IDS = [f"{'f32' if t is F32 else 'f64'}-{d}d" for t, d in TD]


def dev(ecc, a):
    return ecc.DeviceArray.from_numpy(np.ascontiguousarray(a).ravel())


def expected_doublings(mn, mx, eps, n):
    """Cells of eps * (1 + 1e-6) (1.0 for eps 0), doubled until floor(span / cs) + 1 cells per axis
    make at most max(4 n, 4096) cells in all (2^31 - 2 at the most): the number of doublings."""
    max_cells = min(max(4 * n, 4096), 2 ** 31 - 2)
    cs = eps * (1.0 + 1e-6) if eps > 0 else 1.0
    span = [max(float(b) - float(a), 0.0) for a, b in zip(mn, mx)]
    for k in range(2200):
        q = [s / cs for s in span]
        if all(math.isfinite(x) for x in q) and math.prod(math.floor(x) + 1 for x in q) <= max_cells:
            return k
        cs *= 2.0
    raise AssertionError("no grid fits")


def doublings_of(pts, eps):
    fin = pts[np.isfinite(pts).all(1)].astype(F64)
    return expected_doublings(fin.min(0), fin.max(0), eps, len(pts))


# ------------------------------------------------------------------------------------ references
def brute_f64(pts, eps, min_pts):
    """(counts, core distances, offsets, ascending lists, their distances) of an fp64 cloud:
    square_distance (kdTree.hpp:180-192) in the same operation order, `<= eps * eps`."""
    n, dim = pts.shape
    eps2 = eps * eps
    cnt, core = np.zeros(n, np.int32), np.full(n, -1.0)
    rows, dists = [], []
    with np.errstate(all="ignore"):
        for a in range(0, n, 512):
            blk = pts[a:a + 512]
            s = np.zeros((len(blk), n))
            for d in range(dim):
                dd = pts[None, :, d] - blk[:, None, d]
                s = s + dd * dd
            ball = s <= eps2
            for r in range(len(blk)):
                idx = np.nonzero(ball[r])[0]
                d2 = s[r, idx]
                cnt[a + r] = len(idx)
                rows.append(idx.astype(np.int32))
                dists.append(np.sqrt(d2))
                if len(idx) >= min_pts:
                    core[a + r] = np.sqrt(np.sort(d2)[min_pts - 1])
    off = np.concatenate([[0], np.cumsum(cnt, dtype=np.int64)])
    return cnt, core, off, np.concatenate(rows), np.concatenate(dists)


def brute_f32(orc, pts, eps, min_pts):
    cnt, core, off, nbr = orc.radius_f32(pts, eps, min_pts)
    total = int(off[-1])
    nbr = nbr[:total]
    i_of = np.repeat(np.arange(len(pts)), np.diff(off))
    diff = (pts[nbr] - pts[i_of]).astype(F64)  # float differences, widened
    d2 = np.zeros(total)
    for d in range(pts.shape[1]):
        d2 = d2 + diff[:, d] * diff[:, d]
    return cnt, core, off, nbr, np.sqrt(d2)


def check_radius(ecc, orc, gpu, pts, eps, min_pts):
    """Counts with core distances, the size query, lists with distances, the ascending sort: all
    five outputs against the brute force.  Returns the reference."""
    pts = np.ascontiguousarray(pts)
    n, dim = pts.shape
    f32 = pts.dtype == F32
    assert f32 or pts.dtype == F64
    ref = brute_f32(orc, pts, eps, min_pts) if f32 else brute_f64(pts, eps, min_pts)
    o_cnt, o_core, o_off, o_nbr, o_nd = ref
    counts_fn = gpu.radius_counts_f32 if f32 else gpu.radius_counts_f64
    lists_fn = gpu.radius_lists_f32 if f32 else gpu.radius_lists_f64
    d_p = dev(ecc, pts)
    d_cnt, d_core = ecc.DeviceArray(n, np.int32), ecc.DeviceArray(n, F64)
    counts_fn(d_p, n, dim, eps, min_pts, d_cnt, d_core)
    d_off = ecc.DeviceArray(n + 1, np.int64)
    lists_fn(d_p, n, dim, eps, d_cnt, d_off, None, 0)
    gpu.sync()
    assert gpu.radius_status() == 0
    g_cnt = d_cnt.numpy()
    assert np.array_equal(g_cnt, o_cnt), np.nonzero(g_cnt != o_cnt)[0][:8]
    assert np.array_equal(d_core.numpy().view(np.int64), o_core.view(np.int64))
    assert np.array_equal(d_off.numpy(), o_off)
    total = int(o_off[-1])
    d_nbr, d_nd = ecc.DeviceArray(total, np.int32), ecc.DeviceArray(total, F64)
    lists_fn(d_p, n, dim, eps, d_cnt, d_off, d_nbr, total, d_nd)
    gpu.lists_sort_ascending(n, d_off, total, d_nbr, d_nd)
    gpu.sync()
    assert gpu.radius_status() == 0
    assert np.array_equal(d_off.numpy(), o_off)
    assert np.array_equal(d_nbr.numpy(), o_nbr)
    assert np.array_equal(d_nd.numpy().view(np.int64), o_nd.view(np.int64))
    return ref


# ------------------------------------------------------------------------------------ geometries
@functools.lru_cache(maxsize=None)
def cloud(geo, T, dim):
    """(points, eps, min_pts) of a numbered geometry; the same arrays for every test that uses it."""
    rng = np.random.default_rng(1000 * geo + 10 * dim + (T is F32))
    if geo == 1:  # 30 blobs of 50 over [0, 1000)^D: far more cells wanted than 4 n
        c = rng.uniform(0, 1000, (30, dim))
        pts, eps, min_pts = (c[:, None, :] + rng.normal(0, 0.5, (30, 50, dim))).reshape(-1, dim), 1.0, 5
    elif geo == 2:  # one far outlier: the grid collapses to one hot cell
        far = 1e6 if T is F32 else 1e12
        pts, eps, min_pts = np.concatenate([rng.uniform(0, 10, (2000, dim)), np.full((1, dim), far)]), 0.5, 8
    elif geo == 4:  # integer-valued, far from 0: 3-4-5 pairs sit on the `<=` boundary of eps 5
        shift = -2.0 ** 22 if T is F32 else 1e15
        pts, eps, min_pts = rng.integers(0, 60, (1500, dim)).astype(F64) + shift, 1.5, 4
    elif geo == 7:  # a cluster near 0 and points whose span overflows a double (fp64 only)
        assert T is F64
        ends = [s * v * e for v in (1e308, 1.7e308) for s in (-1.0, 1.0)
                for e in ([np.eye(dim)[0], np.ones(dim)] if dim > 1 else [np.ones(1)])]
        pts, eps, min_pts = np.concatenate([rng.normal(0, 1.0, (300, dim)), np.array(ends)]), 0.5, 5
    else:
        raise KeyError(geo)
    pts = np.ascontiguousarray(pts.astype(T))
    pts.setflags(write=False)
    return pts, eps, min_pts


# 1 ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,dim", TD, ids=TD_IDS)
def test_radius_forced_doubling(ecc, orc, gpu, T, dim):
    pts, eps, min_pts = cloud(1, T, dim)
    assert len(pts) == 1500
    k = doublings_of(pts, eps)
    if dim == 1:
        assert k == 0  # about 1000 cells of the 6000 allowed: one axis of this input needs no doubling
    else:
        assert k >= 4  # 2-D: 10^6 wanted cells against 6000 is 4 doublings; 3-D needs more
    cnt, core, *_ = check_radius(ecc, orc, gpu, pts, eps, min_pts)
    assert (core >= 0).any() and (core < 0).any()


# 2 ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,dim", TD, ids=TD_IDS)
def test_radius_one_far_outlier(ecc, orc, gpu, T, dim):
    pts, eps, min_pts = cloud(2, T, dim)
    assert doublings_of(pts, eps) >= 8
    cnt, core, *_ = check_radius(ecc, orc, gpu, pts, eps, min_pts)
    assert cnt[-1] == 1 and ((core >= 0).any() or dim == 3)  # 3-D: 2 points per unit volume, no ball of 8
    # ... and the same balls as without the outlier
    cnt0, *_ = check_radius(ecc, orc, gpu, pts[:-1], eps, min_pts)
    assert np.array_equal(cnt[:-1], cnt0)


# 3 ------------------------------------------------------------------------------------------------
def degenerate_boxes(T):
    rng = np.random.default_rng(33)
    xy = rng.uniform(0, 20, (800, 2))
    out = {
        "z_constant": (np.concatenate([xy, np.full((800, 1), 3.5)], 1), 1.0, 4),
        "y_z_constant": (np.concatenate([rng.uniform(0, 50, (800, 1)), np.full((800, 1), -2.25), np.full((800, 1), 7.0)], 1), 0.3, 4),
        "identical_500": (np.full((500, 2), 7.25), 0.5, 5),
        "exactly_eps_apart": (np.array([[0.0], [0.75]]), 0.75, 2),
        "exactly_eps_apart_3d": (np.array([[1.0, 2.0, 3.0], [1.0, 2.75, 3.0]]), 0.75, 2),
    }
    for d in (1, 2, 3):
        out[f"single_point_{d}d"] = (np.full((1, d), -3.0), 2.0, 1)
    z = rng.integers(-2, 3, (400, 2)).astype(F64)
    z[(z == 0) & (rng.random(z.shape) < 0.5)] = -0.0
    assert (np.signbit(z) & (z == 0)).any() and (~np.signbit(z) & (z == 0)).any()
    out["signed_zeros"] = (z, 1.0, 3)
    zz = np.zeros((64, 1))
    zz[::2] = -0.0  # every coordinate a zero: min and max of the box differ only in sign
    out["only_signed_zeros"] = (zz, 1.0, 3)
    return {k: (np.ascontiguousarray(p.astype(T)), e, m) for k, (p, e, m) in out.items()}


@pytest.mark.parametrize("T", TYPES, ids=["f32", "f64"])
def test_radius_degenerate_boxes(ecc, orc, gpu, T):
    for name, (pts, eps, min_pts) in degenerate_boxes(T).items():
        cnt, *_ = check_radius(ecc, orc, gpu, pts, eps, min_pts)
        if name.startswith("exactly_eps_apart"):
            assert cnt.tolist() == [2, 2], name  # d^2 == eps^2 passes `<=`
        if name == "identical_500":
            assert (cnt == 500).all()


# 4 ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,dim", TD, ids=TD_IDS)
def test_radius_offsets_and_signs(ecc, orc, gpu, T, dim):
    shifted, _, min_pts = cloud(4, T, dim)
    base = (shifted.astype(F64) - (-2.0 ** 22 if T is F32 else 1e15))
    assert np.array_equal(base, np.round(base)) and base.min() == 0 and base.max() == 59  # the shift lost nothing
    symmetric = np.ascontiguousarray((base[:600] % 41 - 20).astype(T))
    assert symmetric.min() == -20 and symmetric.max() == 20
    for pts in (shifted, symmetric):
        for eps in (1.5, 5.0):
            cnt, _, off, nbr, nd = check_radius(ecc, orc, gpu, pts, eps, min_pts)
            if eps == 5.0:  # pairs at distance exactly eps are in (3-4-5 ones from 2-D on)
                assert (nd == 5.0).any()
                if dim >= 2:
                    i_of = np.repeat(np.arange(len(pts)), cnt)
                    d = np.abs(pts[nbr].astype(F64) - pts[i_of].astype(F64))
                    assert ((nd == 5.0) & (np.sort(d, 1)[:, -2:] == [3, 4]).all(1)).any()


# 5 ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shift", [0.0, 2.0 ** 20], ids=["plain", "shifted"])
@pytest.mark.parametrize("T,shape", [(t, s) for t in TYPES for s in ("chain", "lattice")],
                         ids=[f"{t}-{s}" for t in ("f32", "f64") for s in ("chain", "lattice")])
def test_radius_exact_eps_spacing(ecc, orc, gpu, T, shape, shift):
    """Neighbours in a chain or lattice are exactly eps apart as written; in f64 the spacing
    k * 0.1 rounds some of those pairs inside eps and some outside."""
    eps = 0.25 if T is F32 else 0.1
    if shape == "chain":
        pts = (np.arange(4000, dtype=F64) * eps)[:, None]
    else:
        k = np.arange(60, dtype=F64) * eps
        pts = np.stack(np.meshgrid(k, k, indexing="ij"), -1).reshape(-1, 2)
    pts = np.ascontiguousarray((pts + shift).astype(T))
    assert doublings_of(pts, eps) == 0
    cnt, *_ = check_radius(ecc, orc, gpu, pts, eps, 3)
    full = 3 if shape == "chain" else 5
    if T is F32:  # exact arithmetic: every neighbour at distance eps is in
        assert cnt.max() == full and (cnt == full).sum() >= len(pts) - 240
    else:
        # rounding put some of the pairs inside and some (more than the border's) outside
        assert 1 < cnt.max() <= full and (cnt < full).sum() > 240


# 6 ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [1, 2])
def test_radius_f32_subnormal_scale(ecc, orc, gpu, dim):
    """Coordinates k * 2^-140 (subnormal floats), eps 3 * 2^-140: a flushed float difference would
    make every point everybody's neighbour."""
    u = 2.0 ** -140
    rng = np.random.default_rng(6 + dim)
    k = rng.integers(0, 400 if dim == 1 else 40, (600, dim))
    pts = np.ascontiguousarray((k * u).astype(F32))
    assert np.array_equal(pts.astype(F64) / u, k) and 0 < pts.max() < np.finfo(F32).tiny
    cnt, *_ = check_radius(ecc, orc, gpu, pts, 3 * u, 4)
    # the integer problem has the same balls
    ref_cnt, *_ = brute_f64(k.astype(F64), 3.0, 4)
    assert np.array_equal(cnt, ref_cnt) and cnt.max() < 300


@pytest.mark.parametrize("dim", [1, 2, 3])
def test_radius_f64_eps_whose_square_is_zero(ecc, orc, gpu, dim):
    eps = 5e-320
    assert eps > 0 and eps * eps == 0.0
    pts = np.random.default_rng(60 + dim).integers(0, [30, 12, 6][dim - 1], (1500, dim)).astype(F64)
    assert doublings_of(pts, eps) > 1000
    cnt, _, off, nbr, _ = check_radius(ecc, orc, gpu, pts, eps, 2)
    assert cnt.max() > 2 and (pts[nbr] == pts[np.repeat(np.arange(1500), cnt)]).all()  # the sets of equal points


# 7 ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [1, 2, 3])
def test_radius_f64_span_overflows_a_double(ecc, orc, gpu, dim):
    """max - min of an axis is +inf for finite input.  The brute force defines the result: a pair
    whose per-axis difference overflows has d^2 = inf and is no neighbour."""
    pts, eps, min_pts = cloud(7, F64, dim)
    with np.errstate(over="ignore"):
        assert np.isinf(pts.max(0) - pts.min(0)).all() and np.isfinite(pts).all()
    cnt, core, *_ = check_radius(ecc, orc, gpu, pts, eps, min_pts)
    assert (cnt[300:] == 1).all() and (core[:300] >= 0).any()
    cnt0, *_ = check_radius(ecc, orc, gpu, pts[:300], eps, min_pts)
    assert np.array_equal(cnt[:300], cnt0)


def test_radius_f64_eps_whose_square_overflows(ecc, orc, gpu):
    """eps * eps = +inf: `d^2 <= eps^2` holds for every pair of finite points, also where d^2 is
    +inf itself, so no two points may be kept apart by the grid."""
    rng = np.random.default_rng(77)
    pts = np.concatenate([rng.normal(0, 1e300, (40, 2)), [[1e308, -1e308], [-1e308, 1e308], [0, 0], [1.7e308, 1.7e308]]])
    cnt, _, _, _, nd = check_radius(ecc, orc, gpu, pts, 1e200, 3)
    assert (cnt == len(pts)).all() and np.isinf(nd).any()


# 8 ------------------------------------------------------------------------------------------------
def test_radius_f32_grid_stride_paths(ecc, gpu):
    """More points than the 4096 x 256 lanes of the box / count / scatter kernels and than the
    65536 x 4 waves of the core-distance select (min_pts above 64)."""
    n, eps, min_pts = 4096 * 256 + 300, 50.0, 80
    rng = np.random.default_rng(8)
    pts = rng.uniform(0, 1e6, n).astype(F32)
    order = np.argsort(pts, kind="stable")
    sample = np.unique(np.concatenate([rng.choice(n, 260, replace=False), order[:20], order[-20:]]))
    d_p = dev(ecc, pts)
    d_cnt, d_core = ecc.DeviceArray(n, np.int32), ecc.DeviceArray(n, F64)
    gpu.radius_counts_f32(d_p, n, 1, eps, min_pts, d_cnt, d_core)
    d_off = ecc.DeviceArray(n + 1, np.int64)
    gpu.radius_lists_f32(d_p, n, 1, eps, d_cnt, d_off, None, 0)
    gpu.sync()
    assert gpu.radius_status() == 0
    g_cnt, g_core = d_cnt.numpy(), d_core.numpy()
    assert int(d_off.numpy()[n]) == int(g_cnt.sum(dtype=np.int64))
    n_core = 0
    spts = pts[order]
    for i in sample:
        # brute force over everything within eps + 1 (a float difference at 1e6 is off by 1/16 at most)
        lo, hi = np.searchsorted(spts, [pts[i] - (eps + 1), pts[i] + (eps + 1)])
        dd = (spts[lo:hi] - pts[i]).astype(F64)  # the difference in float, widened
        s = dd * dd
        ball = s <= eps * eps
        c = int(ball.sum())
        want = math.sqrt(np.sort(s[ball])[min_pts - 1]) if c >= min_pts else -1.0
        assert g_cnt[i] == c and g_core[i] == want, (i, g_cnt[i], c, g_core[i], want)
        n_core += c >= min_pts
    assert 0 < n_core < len(sample)


# 9 ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", TYPES, ids=["f32", "f64"])
def test_radius_lists_capacity(ecc, orc, gpu, T):
    pts, eps, min_pts = cloud(1, T, 2)
    n = len(pts)
    f32 = T is F32
    counts_fn = gpu.radius_counts_f32 if f32 else gpu.radius_counts_f64
    lists_fn = gpu.radius_lists_f32 if f32 else gpu.radius_lists_f64
    o_cnt, _, o_off, o_nbr, _ = brute_f32(orc, pts, eps, 1) if f32 else brute_f64(pts, eps, 1)
    total = int(o_off[-1])
    d_p = dev(ecc, pts)
    d_cnt = ecc.DeviceArray(n, np.int32)
    counts_fn(d_p, n, 2, eps, 1, d_cnt)
    d_off = ecc.DeviceArray(n + 1, np.int64)

    # half the capacity: entries below nbr_cap only, the rest of the buffer untouched
    cap = total // 2
    d_nbr = dev(ecc, np.full(total, -7, np.int32))
    d_nd = dev(ecc, np.full(total, -3.0))
    lists_fn(d_p, n, 2, eps, d_cnt, d_off, d_nbr, cap, d_nd)
    gpu.sync()
    assert gpu.radius_status() == ecc.ERR_CAPACITY
    nbr, nd = d_nbr.numpy(), d_nd.numpy()
    assert (nbr[cap:] == -7).all() and (nd[cap:] == -3.0).all()
    assert np.array_equal(d_off.numpy(), o_off)
    for i in range(n):  # the rows below the capacity are whole and right
        if o_off[i + 1] <= cap:
            assert sorted(nbr[o_off[i]:o_off[i + 1]].tolist()) == o_nbr[o_off[i]:o_off[i + 1]].tolist(), i

    # counts of a smaller eps: every row is cut to its count, nothing written outside the rows
    counts_fn(d_p, n, 2, eps / 2, 1, d_cnt)
    s_cnt = d_cnt.numpy()
    s_total = int(s_cnt.sum())
    assert (s_cnt < o_cnt).any() and s_total < total
    d_nbr = dev(ecc, np.full(total, -7, np.int32))
    d_nd = dev(ecc, np.full(total, -3.0))
    lists_fn(d_p, n, 2, eps, d_cnt, d_off, d_nbr, total, d_nd)
    gpu.sync()
    assert gpu.radius_status() == ecc.ERR_CAPACITY
    nbr, nd, off = d_nbr.numpy(), d_nd.numpy(), d_off.numpy()
    assert np.array_equal(off, np.concatenate([[0], np.cumsum(s_cnt, dtype=np.int64)]))
    assert (nbr[s_total:] == -7).all() and (nd[s_total:] == -3.0).all()
    for i in range(n):
        row = nbr[off[i]:off[i + 1]].tolist()
        assert len(set(row)) == len(row) and set(row) <= set(o_nbr[o_off[i]:o_off[i + 1]].tolist()), i
    # a full-size call afterwards is clean again
    counts_fn(d_p, n, 2, eps, 1, d_cnt)
    lists_fn(d_p, n, 2, eps, d_cnt, d_off, d_nbr, total, d_nd)
    gpu.sync()
    assert gpu.radius_status() == 0


# 10 -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_radius_f64_reports_non_finite_coordinates(ecc, gpu, bad):
    pts = np.random.default_rng(10).uniform(0, 10, (500, 2))
    dirty = pts.copy()
    dirty[123, 1] = bad
    d_cnt = ecc.DeviceArray(500, np.int32)
    gpu.radius_counts_f64(dev(ecc, dirty), 500, 2, 0.5, 1, d_cnt)
    gpu.sync()
    assert gpu.radius_status() == ecc.ERR_INVALID
    gpu.radius_counts_f64(dev(ecc, pts), 500, 2, 0.5, 1, d_cnt)
    gpu.sync()
    assert gpu.radius_status() == ecc.OK
    assert np.array_equal(d_cnt.numpy(), brute_f64(pts, 0.5, 1)[0])


# 11 -----------------------------------------------------------------------------------------------
DBSCAN_CASES = [(g, t, d) for g in (1, 2, 4, 7) for t, d in ((F32, 1), (F32, 2), (F64, 1), (F64, 2), (F64, 3))
                if not (g == 7 and t is F32)]


@functools.lru_cache(maxsize=None)
def dbscan_reference(geo, T, dim):
    import orc
    pts, eps, _ = cloud(geo, T, dim)
    _, ref = orc.dbscan_cloud(pts, eps, 4, 1, 1 << 30)
    return ref


def gpu_dbscan_cloud(ecc, gpu, pts, eps, min_pts, min_size, max_size, dup_cap=1 << 16):
    n, dim = pts.shape
    d_lab, d_nc = ecc.DeviceArray(n, np.int32), ecc.DeviceArray(1, np.int32)
    d_dups, d_nd = ecc.DeviceArray(2 * dup_cap, np.int64), ecc.DeviceArray(1, np.int64)
    gpu.dbscan_cloud(dev(ecc, pts), n, dim, eps, min_pts, min_size, max_size, d_lab, d_nc, d_dups, dup_cap, d_nd)
    assert gpu.dbscan_cloud_status() == 0, gpu.last_error()
    lab, nc, nd = d_lab.numpy(), int(d_nc.numpy()[0]), int(d_nd.numpy()[0])
    members = [[] for _ in range(nc)]
    for i in np.nonzero(lab >= 0)[0]:
        members[lab[i]].append(int(i))
    for p, c in d_dups.numpy()[:2 * nd].reshape(-1, 2):
        members[c].append(int(p))
    return [sorted(m) for m in members]


@pytest.mark.parametrize("geo,T,dim", DBSCAN_CASES,
                         ids=[f"geo{g}-{'f32' if t is F32 else 'f64'}-{d}d" for g, t, d in DBSCAN_CASES])
def test_dbscan_cloud_on_hostile_geometry(ecc, orc, gpu, geo, T, dim):
    pts, eps, _ = cloud(geo, T, dim)
    ref = dbscan_reference(geo, T, dim)
    got = gpu_dbscan_cloud(ecc, gpu, pts, eps, 4, 1, 1 << 30)
    assert len(got) == len(ref)
    assert len(ref) > 0 or (geo, dim) == (4, 3)  # 1500 integer points in 60^3: all noise at eps 1.5
    for a, b in zip(got, ref):  # member lists with duplicate memberships
        assert a == sorted(b.tolist())


def test_dbscan_cloud_cases_include_duplicate_memberships(orc):
    dups = 0
    for case in DBSCAN_CASES:
        ref = dbscan_reference(*case)
        dups += sum(len(c) for c in ref) - len({int(i) for c in ref for i in c})
    assert dups > 0


# 12 -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geo,dim", [(1, 2), (2, 2), (4, 2), (7, 1)], ids=["geo1-2d", "geo2-2d", "geo4-2d", "geo7-1d"])
def test_optics_f64_on_hostile_geometry(ecc, orc, gpu, geo, dim):
    pts, eps, min_pts = cloud(geo, F64, dim)
    order, reach = gpu.optics_f64(pts, min_pts, eps)
    o_order, o_reach = orc.optics(pts, min_pts, eps)
    assert np.array_equal(order, o_order)
    assert np.array_equal(reach.view(np.int64), o_reach.view(np.int64))
    assert (o_reach > 0).sum() > 100
