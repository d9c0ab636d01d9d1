"""A literal Python restatement of what ecc_dbscan_lists / ecc_dbscan_lists_host produce: the loop
of ref_cpu_cases.clusters_from_labels (a push per label and per dup pair, sorted per cluster:
PCC/DBSCAN_simple.h:27-90, :82) extended to the members / pairs / n_members layout, with the
all-or-nothing capacity rule and the ignore rule for hostile entries.  Arrays are compared as bytes;
there are no tolerances.  Outputs start from sentinels, so everything outside the contract is part
of the comparison."""
import numpy as np

OK, ERR_INVALID, ERR_CAPACITY = 0, -1, -4
MEM_FILL, PAIR_FILL, NM_FILL = -77777, -88888, -99
TAIL = 5  # sentinel entries past the last segment's row
BAD_LABEL = 0x7FFFFFF0  # padding labels: outside every [-1, C)


def segment_lists(labels, count, n_clusters, dups):
    """One segment: labels[:count], dups = (segment-local slot, cluster) pairs ->
    (list of sorted member lists, anything ignored)."""
    nc = max(int(n_clusters), 0)
    invalid = int(n_clusters) < 0
    members = [[] for _ in range(nc)]
    for i in range(count):
        lab = int(labels[i])
        if 0 <= lab < nc:
            members[lab].append(i)
        elif lab != -1:
            invalid = True
    for j, c in dups:
        if 0 <= j < count and 0 <= c < nc:
            members[int(c)].append(int(j))
        else:
            invalid = True
    return [sorted(m) for m in members], invalid


def layout(lists):
    """Sorted member lists -> (members row, [(begin, end)]): an empty cluster is (begin, begin - 1)."""
    row, pairs = [], []
    for m in lists:
        pairs.append((len(row), len(row) + len(m) - 1))
        row.extend(m)
    return row, pairs


def expected(labels, n_clusters, dups, n_dups, dup_cap, n_segs, stride, counts, member_stride, pair_cap):
    """The whole device result over sentinel-filled outputs:
    (members int32[n_segs * member_stride + TAIL], n_members int64[n_segs + TAIL],
     pairs int32[(n_segs * pair_cap + TAIL) * 2], status, per-segment (row, pairs) or None)."""
    labels = np.asarray(labels, np.int32)
    dups = np.asarray(dups, np.int64).reshape(-1, 2)
    members = np.full(n_segs * member_stride + TAIL, MEM_FILL, np.int32)
    n_members = np.full(n_segs + TAIL, NM_FILL, np.int64)
    pairs = np.full((n_segs * pair_cap + TAIL) * 2, PAIR_FILL, np.int32)
    invalid, capacity = False, n_dups > dup_cap
    per_seg = [[] for _ in range(n_segs)]
    for p, c in dups[:max(min(n_dups, dup_cap), 0)]:
        if 0 <= p < n_segs * stride:
            per_seg[int(p) // stride].append((int(p) % stride, int(c)))
        else:
            invalid = True
    segs = []
    for s in range(n_segs):
        count = stride if counts is None else min(max(int(counts[s]), 0), stride)
        lists, bad = segment_lists(labels[s * stride:(s + 1) * stride], count, n_clusters[s], per_seg[s])
        invalid |= bad
        row, iv = layout(lists)
        n_members[s] = len(row)
        if len(row) > member_stride or len(iv) > pair_cap:
            capacity = True
            segs.append(None)
            continue
        members[s * member_stride: s * member_stride + len(row)] = row
        pairs[s * pair_cap * 2: (s * pair_cap + len(iv)) * 2] = np.asarray(iv, np.int32).reshape(-1)
        segs.append((row, iv))
    return members, n_members, pairs, (ERR_INVALID if invalid else ERR_CAPACITY if capacity else OK), segs


def dups_of_clusters(labels, clusters):
    """The memberships of `clusters` (index arrays in output order) other than each point's label, as
    (point, cluster) pairs: what a DBSCAN entry leaves in dups."""
    return [(int(p), c) for c, m in enumerate(clusters) for p in m if labels[p] != c]


def fabricated_segment(rng, count, kind):
    """(labels[count], C, dups [(slot, cluster)]) for one segment: labels random in [-1, C), 0 to
    3 x count dup pairs unique per (slot, cluster) and different from the slot's label.
    kind 0: all -1 (C random), 1: one cluster, 2: every point its own cluster, else random C in
    [0, count]."""
    if kind == 0:
        nc = int(rng.integers(0, count + 1))
        labels = np.full(count, -1, np.int32)
    elif kind == 1:
        nc = 1 if count else 0
        labels = np.zeros(count, np.int32)
    elif kind == 2:
        nc = count
        labels = rng.permutation(count).astype(np.int32)
    else:
        nc = int(rng.integers(0, count + 1))
        labels = rng.integers(-1, nc, count).astype(np.int32) if nc else np.full(count, -1, np.int32)
    free = [(j, c) for j in range(count) for c in range(nc) if labels[j] != c]
    k = min(int(rng.integers(0, 3 * count + 1)), len(free))
    pick = rng.choice(len(free), k, replace=False) if k else []
    return labels, nc, [free[i] for i in pick]


def fabricated(seed, n_segs, stride, full=False):
    """n_segs fabricated segments: (labels int32[n_segs * stride] with BAD_LABEL padding, counts,
    n_clusters, dups int64 (k, 2) with flattened points)."""
    rng = np.random.default_rng(seed)
    labels = np.full(n_segs * stride, BAD_LABEL, np.int32)
    counts, ncl, dups = np.zeros(n_segs, np.int32), np.zeros(n_segs, np.int32), []
    for s in range(n_segs):
        count = stride if full else (s % (stride + 1) if s < 3 * (stride + 1) else int(rng.integers(0, stride + 1)))
        lab, nc, d = fabricated_segment(rng, count, s % 7)
        labels[s * stride: s * stride + count] = lab
        counts[s], ncl[s] = count, nc
        dups += [(s * stride + j, c) for j, c in d]
    return labels, counts, ncl, np.asarray(dups, np.int64).reshape(-1, 2)
