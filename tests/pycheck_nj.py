"""A second reading of neighbour joining as include/pagan_host.h defines it ("neighbour joining"), in numpy fp64 (test
infrastructure).  joins() follows the definition operation by operation -- the 64 partial row sums and their tree, Q in the
written bracketing, the tie rule, the update of the distances and of R in the written order -- vectorised over a row, so that the
device's join records can be compared with it byte for byte.  root_tree() is the rooting and the child order, literally;
brute_midpoint() finds the longest leaf-to-leaf path by trying all pairs, for inputs on which every sum is exact.
random_tree() makes unrooted binary trees with dyadic lengths, their additive matrices and their splits."""
import numpy as np


def row_sums(d):
    """R_i: x[l] = sum_q d(i, 64 q + l) from +0, q ascending, then x[l] += x[l + s] for s = 32 .. 1."""
    n = len(d)
    blocks = (n + 63) // 64
    p = np.zeros((n, blocks * 64), np.float64)
    p[:, :n] = d
    p[np.arange(n), np.arange(n)] = 0.0
    x = np.zeros((n, 64), np.float64)
    for q in range(blocks):
        x = x + p[:, 64 * q:64 * q + 64]
    s = 32
    while s >= 1:
        x[:, :s] = x[:, :s] + x[:, s:2 * s]
        s //= 2
    return x[:, 0].copy()


def joins(dist):
    """(join_ids [n-3, 2] int32, join_len [n-3, 2] float64, star_ids [3] int32, star_len [3] float64): the header's records, the
    lengths raw.  The upper triangle of dist is read."""
    dist = np.asarray(dist, np.float64)
    n = len(dist)
    if n == 2:
        h = dist[0, 1] / 2
        return (np.zeros((0, 2), np.int32), np.zeros((0, 2), np.float64), np.array([0, 1, -1], np.int32), np.array([h, h, 0.0]))
    up = np.triu(dist, 1)
    total = 2 * n - 3
    d = np.zeros((total, total), np.float64)                # by cluster id
    d[:n, :n] = up + up.T
    R = np.zeros(total, np.float64)
    R[:n] = row_sums(d[:n, :n])
    act = list(range(n))                                    # ascending ids
    ids, lens = [], []
    for t in range(n - 3):
        r = len(act)
        a = np.array(act)
        sub = d[np.ix_(a, a)]
        q = (np.float64(r - 2) * sub - R[a][:, None]) - R[a][None, :]      # row: the lower id
        q[np.tril_indices(r)] = np.inf
        best = q.min()
        at = int(np.flatnonzero(q.ravel() == best)[0])      # row-major: the lowest first id, then the lowest second id
        i, j = act[at // r], act[at % r]
        u = n + t
        dij = d[i, j]
        len_i = dij / 2 + (R[i] - R[j]) / (2 * np.float64(r - 2))
        len_j = dij - len_i
        k = np.array([c for c in act if c != i and c != j])
        duk = ((d[i, k] + d[j, k]) - dij) / 2
        R[k] = ((R[k] - d[i, k]) - d[j, k]) + duk
        d[u, k] = duk
        d[k, u] = duk
        R[u] = ((R[i] + R[j]) - np.float64(r) * dij) / 2
        act = [c for c in act if c != i and c != j] + [u]
        ids.append((i, j))
        lens.append((len_i, len_j))
    a, b, c = act
    star_len = [((d[a, b] + d[a, c]) - d[b, c]) / 2, ((d[a, b] + d[b, c]) - d[a, c]) / 2, ((d[a, c] + d[b, c]) - d[a, b]) / 2]
    return (np.array(ids, np.int32).reshape(-1, 2), np.array(lens, np.float64).reshape(-1, 2), np.array(act, np.int32),
            np.array(star_len, np.float64))


def clusters(n, join_ids, star_ids):
    """{cluster id: frozenset of its leaves} for the leaves and every join's cluster."""
    leaves = {k: frozenset([k]) for k in range(n)}
    for t, (i, j) in enumerate(np.asarray(join_ids).reshape(-1, 2)):
        leaves[n + t] = leaves[int(i)] | leaves[int(j)]
    return leaves


def splits_of_joins(n, join_ids, star_ids):
    """The tree's non-trivial splits, each as the side without leaf 0."""
    everything = frozenset(range(n))
    out = set()
    for v, s in clusters(n, join_ids, star_ids).items():
        if v >= n and 1 < len(s) < n - 1:
            out.add(everything - s if 0 in s else s)
    return out


def unrooted_edges(n, join_ids, join_len, star_ids, star_len):
    """[(child, parent, clamped length)] of the tree as the joins hang it from the star node 2 n - 3."""
    edges = []
    for t, ((i, j), (li, lj)) in enumerate(zip(np.asarray(join_ids).reshape(-1, 2), np.asarray(join_len).reshape(-1, 2))):
        edges.append((int(i), n + t, max(0.0, float(li))))
        edges.append((int(j), n + t, max(0.0, float(lj))))
    for c, l in zip(star_ids, star_len):
        edges.append((int(c), 2 * n - 3, max(0.0, float(l))))
    return edges


def root_tree(names, join_ids, join_len, star_ids, star_len):
    """(tree, facts): the rooted binary tree in synth.parse_newick's form (the root's length 0.0) and the rooting's own numbers
    (span, half, top, the node c whose upper edge carries the root, below, above)."""
    n = len(names)
    if n == 2:
        return ("internal", ("leaf", names[0], max(0.0, float(star_len[0]))), ("leaf", names[1], max(0.0, float(star_len[1]))), 0.0), {}
    star = 2 * n - 3
    kids = {v: [] for v in range(n, star + 1)}
    length, parent = {}, {}
    for c, p, l in unrooted_edges(n, join_ids, join_len, star_ids, star_len):
        kids[p].append(c)
        length[c] = l
        parent[c] = p
    low, far, toward, span = {k: k for k in range(n)}, {k: 0.0 for k in range(n)}, {}, {}
    top = None
    for v in range(n, star + 1):                            # ids grow towards the star: children come first
        low[v] = min(low[c] for c in kids[v])
        kids[v].sort(key=lambda c: low[c])
        first = None
        for c in kids[v]:
            if first is None or far[c] + length[c] > far[first] + length[first]:
                first = c
        second = None
        for c in kids[v]:
            if c != first and (second is None or far[c] + length[c] > far[second] + length[second]):
                second = c
        far[v], toward[v] = far[first] + length[first], first
        span[v] = (far[first] + length[first]) + (far[second] + length[second])
        if top is None or span[v] > span[top]:
            top = v
    half = span[top] / 2
    c = toward[top]
    while far[c] > half:
        c = toward[c]
    below = min(max(half - far[c], 0.0), length[c])
    above = length[c] - below
    # the unrooted tree with the root put on the edge above c, hung again from the root
    nbr = {v: {} for v in range(2 * n - 1)}
    for x, p in parent.items():
        if x != c:
            nbr[x][p] = nbr[p][x] = length[x]
    root = 2 * n - 2
    nbr[root][c] = nbr[c][root] = below
    nbr[root][parent[c]] = nbr[parent[c]][root] = above

    def hang(x, come_from, l):
        if x < n:
            return ("leaf", names[x], l), x
        below_x = sorted((hang(w, x, wl) for w, wl in nbr[x].items() if w != come_from), key=lambda tl: tl[1])
        assert len(below_x) == 2
        return ("internal", below_x[0][0], below_x[1][0], l), below_x[0][1]
    tree, _ = hang(root, None, 0.0)
    return tree, {"span": span[top], "half": half, "top": top, "c": c, "below": below, "above": above}


def tree_newick(tree):
    """The tree as pagan_nj_newick prints it."""
    def text(t, is_root):
        tail = "" if is_root else ":%.17g" % t[-1]
        if t[0] == "leaf":
            return t[1] + tail
        return "(%s,%s)%s" % (text(t[1], False), text(t[2], False), tail)
    return text(tree, True) + ";"


def deepest(tree):
    """The largest sum of lengths from a node down to a leaf (the node's own length not counted)."""
    if tree[0] == "leaf":
        return 0.0
    return max(deepest(tree[1]) + tree[1][-1], deepest(tree[2]) + tree[2][-1])


def brute_midpoint(n, edges):
    """The longest leaf-to-leaf path of an unrooted tree [(a, b, length)] by the path sums of all pairs: (its length, the pair)."""
    nbr = {}
    for a, b, l in edges:
        nbr.setdefault(a, []).append((b, l))
        nbr.setdefault(b, []).append((a, l))
    best, pair = -1.0, None
    for s in range(n):
        seen, stack = {s: 0.0}, [s]
        while stack:
            x = stack.pop()
            for w, l in nbr[x]:
                if w not in seen:
                    seen[w] = seen[x] + l
                    stack.append(w)
        for e in range(s + 1, n):
            if seen[e] > best:
                best, pair = seen[e], (s, e)
    return best, pair


def random_tree(n, seed, max_eighths=8):
    """An unrooted binary tree over leaves 0 .. n-1 (n >= 3) with every length a multiple of 1/8 in [1/8, max_eighths / 8]:
    (edges [(a, b, length)] with the internal nodes n .. 2n-3, the additive matrix [n, n], the non-trivial splits as
    splits_of_joins gives them, the leaves' edge lengths [n])."""
    rng = np.random.default_rng(seed)
    edges = [[0, n], [1, n], [2, n]]
    for leaf in range(3, n):
        e = int(rng.integers(len(edges)))
        a, b = edges[e]
        mid = n + leaf - 2
        edges[e] = [a, mid]
        edges.append([mid, b])
        edges.append([leaf, mid])
    edges = [(a, b, float(rng.integers(1, max_eighths + 1)) / 8) for a, b in edges]
    nbr = {}
    for a, b, l in edges:
        nbr.setdefault(a, []).append((b, l))
        nbr.setdefault(b, []).append((a, l))
    d = np.zeros((n, n), np.float64)
    for s in range(n):
        seen, stack = {s: 0.0}, [s]
        while stack:
            x = stack.pop()
            for w, l in nbr[x]:
                if w not in seen:
                    seen[w] = seen[x] + l
                    stack.append(w)
        d[s] = [seen[e] for e in range(n)]
    everything = frozenset(range(n))
    splits = set()

    def side(x, come_from):
        if x < n:
            return frozenset([x])
        s = frozenset()
        for w, _ in nbr[x]:
            if w != come_from:
                s |= side(w, x)
        return s
    for a, b, _ in edges:
        if a >= n and b >= n:
            s = side(a, b)
            splits.add(everything - s if 0 in s else s)
    leaf_len = np.zeros(n)
    for a, b, l in edges:
        if a < n:
            leaf_len[a] = l
        if b < n:
            leaf_len[b] = l
    return edges, d, splits, leaf_len
