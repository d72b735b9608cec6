"""A second, independent reading of the guide tree's definition (include/pagan_host.h, "guide tree") in plain Python.

Literal: cleaning as the walk cleans, k-mers as strings in a collections.Counter, S by dictionary look-up, the distance with
the math module, UPGMA over a plain matrix with a full scan per step.  Fast (for larger inputs): np.unique over packed codes,
or a dense spectrum and np.minimum for small k.  Nothing here calls the library."""
import collections
import math

import numpy as np

DNA_FULL = "ACGTRYMKWSBDHVN"
PROTEIN = "ARNDCQEGHILKMFPSTWYV"


def guess_type(upper):
    """The walk's guess over the upper-cased, gap-free strings: 1 DNA, 2 protein."""
    dna = sum(s.count(c) for s in upper for c in "ACGTUN")
    protein = sum(s.count(c) for s in upper for c in PROTEIN)
    if protein == 0:
        return 1 if dna > 0 else 2           # (x / 0 in floats: inf > 0.9, and 0 / 0 is no number, which is not > 0.9)
    return 1 if float(np.float32(dna) / np.float32(protein)) > 0.9 else 2      # (a float quotient, compared as a double)


def clean(seqs, data_type=0):
    """(type 1 / 2 / 3, cleaned strings)."""
    upper = ["".join(c for c in s.upper() if c not in "-\r\n") for s in seqs]
    t = data_type if data_type in (1, 2, 3) else guess_type(upper)
    if t == 2:
        keep = {c: c for c in PROTEIN}
        keep["U"] = keep["X"] = "X"
    else:
        keep = {c: c for c in DNA_FULL}
        keep["U"] = "T"
    return t, ["".join(keep[c] for c in s if c in keep) for s in upper]


def core_letters(t):
    return PROTEIN if t == 2 else "ACGT"


def default_k(t, longest):
    A, lo, hi = (20, 3, 12) if t == 2 else (4, 8, 31)
    k = 0
    while A ** k < 16 * longest:
        k += 1
    return max(lo, min(hi, k))


def kmer_counter(s, k, t):
    core = set(core_letters(t))
    c = collections.Counter()
    for i in range(len(s) - k + 1):
        w = s[i:i + k]
        if all(ch in core for ch in w):
            c[w] += 1
    return c


def distance_of(S, m, k, t):
    F = S / m if m > 0 else 0.0
    p = 1.0 - F ** (1.0 / k) if F > 0 else 1.0
    if p <= 0:
        return 0.0
    if t == 2:
        p = min(p, 0.85)
        return -math.log(1.0 - p - 0.2 * p * p)
    p = min(p, 0.7)
    return -0.75 * math.log(1.0 - p / 0.75)


def _finish(shared, kmers, k, t):
    n = len(kmers)
    dist = np.zeros((n, n), np.float64)
    for x in range(n):
        for y in range(x + 1, n):
            dist[x, y] = dist[y, x] = distance_of(int(shared[x, y]), int(min(kmers[x], kmers[y])), k, t)
    return dist


def distances_literal(seqs, data_type=0, k=0):
    """(shared [n, n] int64 with |n_x| on the diagonal, kmers [n], dist [n, n], k, type)."""
    t, cl = clean(seqs, data_type)
    if k == 0:
        k = default_k(t, max(len(s) for s in cl))
    counters = [kmer_counter(s, k, t) for s in cl]
    n = len(cl)
    kmers = np.array([sum(c.values()) for c in counters], np.int64)
    shared = np.zeros((n, n), np.int64)
    for x in range(n):
        shared[x, x] = kmers[x]
        for y in range(x + 1, n):
            a, b = counters[x], counters[y]
            shared[x, y] = shared[y, x] = sum(min(v, b[w]) for w, v in a.items() if w in b)
    return shared, kmers, _finish(shared, kmers, k, t), k, t


def packed_codes(s, k, t):
    """The valid windows' codes as integers (base A), by numpy."""
    core = core_letters(t)
    A = len(core)
    lut = np.full(256, -1, np.int64)
    for i, c in enumerate(core):
        lut[ord(c)] = i
    v = lut[np.frombuffer(s.encode(), np.uint8)] if s else np.zeros(0, np.int64)
    n = len(v) - k + 1
    if n <= 0:
        return np.zeros(0, np.uint64 if A ** k > 2 ** 62 else np.int64)
    bad = np.concatenate([[0], np.cumsum(v < 0)])
    ok = (bad[k:] - bad[:-k]) == 0
    if A ** k > 2 ** 62:                       # (4^31, 20^12 < 2^64: unsigned arithmetic)
        code = np.zeros(n, np.uint64)
        for j in range(k):
            code = code * np.uint64(A) + np.where(v[j:j + n] < 0, 0, v[j:j + n]).astype(np.uint64)
        return code[ok]
    code = np.zeros(n, np.int64)
    for j in range(k):
        code = code * A + np.where(v[j:j + n] < 0, 0, v[j:j + n])
    return code[ok]


def distances_unique(seqs, data_type=0, k=0):
    """The same through np.unique over packed codes and a merge of the sorted lists."""
    t, cl = clean(seqs, data_type)
    if k == 0:
        k = default_k(t, max(len(s) for s in cl))
    lists = [np.unique(packed_codes(s, k, t), return_counts=True) for s in cl]
    n = len(cl)
    kmers = np.array([int(c.sum()) for _, c in lists], np.int64)
    shared = np.zeros((n, n), np.int64)
    for x in range(n):
        shared[x, x] = kmers[x]
        for y in range(x + 1, n):
            (ca, na), (cb, nb) = lists[x], lists[y]
            _, ia, ib = np.intersect1d(ca, cb, assume_unique=True, return_indices=True)
            shared[x, y] = shared[y, x] = int(np.minimum(na[ia], nb[ib]).sum())
    return shared, kmers, _finish(shared, kmers, k, t), k, t


def shared_dense(seqs, data_type, k):
    """(shared, kmers) for small A^k: one dense spectrum a sequence, np.minimum a row."""
    t, cl = clean(seqs, data_type)
    A = len(core_letters(t))
    assert A ** k <= 1 << 16
    n = len(cl)
    spec = np.zeros((n, A ** k), np.int32)
    for x, s in enumerate(cl):
        spec[x] = np.bincount(packed_codes(s, k, t), minlength=A ** k)
    kmers = spec.sum(axis=1).astype(np.int64)
    shared = np.zeros((n, n), np.int64)
    for x in range(n):
        shared[x] = np.minimum(spec[x][None, :], spec).sum(axis=1)
    return shared, kmers


def upgma(dist):
    """UPGMA with the header's rules over a plain matrix: (children {id: (left, right)}, height {id: h}); ids as the header
    numbers them."""
    n = len(dist)
    d = {(i, j): float(dist[i][j]) for i in range(n) for j in range(i + 1, n)}
    size = {i: 1 for i in range(n)}
    height = {i: 0.0 for i in range(n)}
    children = {}
    active = list(range(n))
    for t in range(n - 1):
        best = None
        for ai, a in enumerate(active):              # (active is ascending by id: the first strictly smaller distance wins)
            for b in active[ai + 1:]:
                if best is None or d[(a, b)] < best[0]:
                    best = (d[(a, b)], a, b)
        v, a, b = best
        u = n + t
        children[u] = (a, b)
        height[u] = v / 2
        na, nb = float(size[a]), float(size[b])
        for c in active:
            if c != a and c != b:
                dac = d[(min(a, c), max(a, c))]
                dbc = d[(min(b, c), max(b, c))]
                d[(c, u)] = (na * dac + nb * dbc) / (na + nb)
        size[u] = size[a] + size[b]
        active = [c for c in active if c != a and c != b] + [u]
    return children, height


def upgma_tree(names, dist):
    """The tree in synth.parse_newick's shape: ("internal", left, right, branch) / ("leaf", name, branch)."""
    n = len(names)
    children, height = upgma(dist)

    def build(v, parent_h):
        b = 0.0 if parent_h is None else parent_h - height[v]
        b = b if b > 0 else 0.0
        if v < n:
            return ("leaf", names[v], b)
        return ("internal", build(children[v][0], height[v]), build(children[v][1], height[v]), b)
    return build(2 * n - 2, None)


def clades(tree):
    """The leaf sets under the internal nodes of a parse_newick tree."""
    out = set()

    def walk(t):
        if t[0] == "leaf":
            return frozenset([t[1]])
        s = walk(t[1]) | walk(t[2])
        out.add(s)
        return s
    walk(tree)
    return out
