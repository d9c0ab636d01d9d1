"""A literal Python restatement of optics::flat_clusters_to_tree (OPT/include/optics/optics.hpp:
948-995), the comparator of the xi-tree tests: the placement loop (:950-966, children before
parents) and the first-parent search (:974-992), on integer (first, second) pairs in
get_chi_clusters_flat's push order.  The forest the reference builds is determined by the placed
list and each position's parent: roots in ascending position are its result vector, a node's
children in ascending position its child list.  The restatement is pinned by the reference's
chi_cluster_tree_tests_1 / _2 (tests/golden/optics_tree_kat.json).

Where the reference would write outside its list or onto a filled slot (its assert after the loop,
:966, would catch only part of that), the restatement raises PlacementError: a test that meets one
fails."""
import json
from pathlib import Path

import numpy as np

KAT = json.loads((Path(__file__).resolve().parent / "golden" / "optics_tree_kat.json").read_text())


class PlacementError(AssertionError):
    pass


def place(pairs):
    """:950-966, literally: the placed ("sorted") list."""
    c = [(int(a), int(b)) for a, b in pairs]
    n = len(c)
    slots = [None] * n
    next_free = 0
    for idx in range(n):
        while next_free < n and slots[next_free] is not None:
            next_free += 1
        pos = next_free
        following = idx + 1
        while following < n and c[following][1] <= c[idx][1]:
            following += 1
            pos += 1
        if pos >= n:
            raise PlacementError(f"entry {idx} placed at {pos}, outside the {n} slots")
        if slots[pos] is not None:
            raise PlacementError(f"entry {idx} placed onto the filled slot {pos}")
        slots[pos] = c[idx]
    if any(s is None for s in slots):
        raise PlacementError("a slot stayed empty")
    return slots


def parents(placed):
    """:974-992, literally: the first later position whose interval holds this one's, or -1."""
    n = len(placed)
    out = []
    for k in range(n):
        p = -1
        for j in range(k + 1, n):
            if placed[k][0] >= placed[j][0] and placed[k][1] <= placed[j][1]:
                p = j
                break
        out.append(p)
    return out


def tree(pairs):
    """(sorted int32 (n, 2), parent int32[n], level int32[n], n_roots) of one flat list."""
    placed = place(pairs)
    par = parents(placed)
    level = [0] * len(par)
    for k in range(len(par) - 1, -1, -1):
        assert par[k] == -1 or par[k] > k
        level[k] = 0 if par[k] < 0 else level[par[k]] + 1
    return (np.asarray(placed, np.int32).reshape(-1, 2), np.asarray(par, np.int32), np.asarray(level, np.int32),
            sum(p < 0 for p in par))


def forest(placed, par):
    """The reference's result as nested lists [first, second, [children ...]], built as :984-992 does."""
    nodes = [[int(a), int(b), []] for a, b in placed]
    roots = []
    for k, p in enumerate(par):
        (roots if p < 0 else nodes[p][2]).append(nodes[k])
    return roots


def dfs(roots, level=0):
    """(level, first, second) of every node, depth first: a tree's root, then each child's subtree."""
    out = []
    for a, b, kids in roots:
        out.append((level, a, b))
        out += dfs(kids, level + 1)
    return out


def second_is_sorted(placed):
    s = [int(p[1]) for p in placed]
    return all(a <= b for a, b in zip(s, s[1:]))


# ------------------------------------------------------------------------------ flat-list generators
def nested_chain(n):
    """n intervals each inside the one before (outermost first, as the xi walk pushes them): level n - 1."""
    return [(i, 2 * n - i) for i in range(n)]


def disjoint(n):
    return [(3 * i, 3 * i + 1) for i in range(n)]


def synthetic_lists(rng, sizes):
    """Lists no reachability plot need ever give: equal seconds, identical pairs, overlapping intervals
    that do not nest, descending seconds, and a plain random mix — one of each kind per size."""
    out = []
    for n in sizes:
        first = rng.integers(0, 40, n)
        out.append(np.stack([first, np.full(n, 50)], 1))                               # equal seconds
        out.append(np.stack([rng.integers(0, 3, n), 5 + rng.integers(0, 2, n)], 1))    # many identical pairs
        b = np.sort(rng.integers(0, 4 * n + 1, n))
        out.append(np.stack([b, b + rng.integers(1, 12, n)], 1))                       # overlapping, not nested
        out.append(np.stack([first, 1000 - np.arange(n) // 2], 1))                     # descending seconds
        a = rng.integers(0, 60, n)
        out.append(np.stack([a, a + rng.integers(0, 60, n)], 1))                       # random intervals
        out.append(np.stack([rng.integers(-9, 9, n), rng.integers(-9, 9, n)], 1))      # begin > end, negatives
    return [np.asarray(p, np.int32).reshape(-1, 2) for p in out]


def xi_lists(rng, sizes, params):
    """Real xi outputs: optics_xi_ref.chi_clusters of random plots that meet exact equality."""
    import optics_xi_ref as xi
    return [xi.pairs_array(xi.chi_clusters(xi.random_plot(rng, n), *params)) for n in sizes]
