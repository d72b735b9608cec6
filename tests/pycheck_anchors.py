"""Two readings of Find_anchors::find_long_substrings up to its sort by length (find_anchors.cpp:35-85) that share no code with
the product (csrc/host_anchors.cpp, csrc/dp_anchors.hip) or the oracle: the list of adjacent cross-string suffix pairs with a
common prefix >= min_length, in the order of the sorted suffix list, as (start in a, start in b, length).

naive()     the text read literally: the suffixes of a, then the suffixes of b, as byte strings; Python's stable sort by the
            byte string (bytes compare as unsigned chars and a proper prefix sorts first, as strcmp has it; of two equal
            suffixes the one of `a` stays first, as the stable sort of that list has it); a plain loop for the common prefix.
            Quadratic on repeats: up to a few thousand symbols.
doubling()  for larger inputs: ranks over  a + \\0 + b + \\1  by prefix doubling (np.lexsort round by round, every round's rank
            array kept), common prefixes read off the kept arrays, longest round first.  It is the algorithm of the device's
            finder restated in numpy, so it counts only as far as tests/test_pycheck_anchors_cpu.py holds it to naive().

a, b: bytes without NUL.  Both return a list of (pos1, pos2, length) tuples."""
import numpy as np


def naive(a, b, m):
    a, b = bytes(a), bytes(b)
    suffixes = [(a[i:], 0, i) for i in range(len(a))] + [(b[j:], 1, j) for j in range(len(b))]
    suffixes.sort(key=lambda s: s[0])                                   # (stable)
    out = []
    for (x, sx, px), (y, sy, py) in zip(suffixes, suffixes[1:]):
        if sx == sy:
            continue
        k, end = 0, min(len(x), len(y))
        while k < end and x[k] == y[k]:
            k += 1
        if k >= m:
            out.append((px, py, k) if sx == 0 else (py, px, k))
    return out


def _text(a, b, swap_sentinels=False):
    """a + \\0 + b + \\1 over integers: both sentinels below every byte"""
    t = np.empty(len(a) + len(b) + 2, np.int64)
    t[:len(a)] = np.frombuffer(a, np.uint8).astype(np.int64) + 2
    t[len(a) + 1:-1] = np.frombuffer(b, np.uint8).astype(np.int64) + 2
    t[len(a)], t[-1] = (1, 0) if swap_sentinels else (0, 1)
    return t


def _rounds(t):
    """[rank by the first 2^r symbols for r = 0, 1, ...] until every suffix has a rank of its own, and the suffix array"""
    n = t.shape[0]
    ranks, k = [t], 1
    while True:
        first = ranks[-1]
        second = np.zeros(n, np.int64)                                   # (nothing behind the text: below every rank)
        if k < n:
            second[:n - k] = first[k:] + 1
        order = np.lexsort((second, first))
        f, s = first[order], second[order]
        new_class = (f[1:] != f[:-1]) | (s[1:] != s[:-1])
        r = np.concatenate(([0], np.cumsum(new_class)))
        rk = np.empty(n, np.int64)
        rk[order] = r
        ranks.append(rk)
        if r[-1] == n - 1:
            return ranks, order
        assert k < n, "every suffix is a different string: the doubling ends"
        k *= 2


def doubling(a, b, m, swap_sentinels=False, lowest_round=0, end_slack=0):
    """The three keyword arguments make the deliberately wrong variants the tests keep (sentinels in the wrong order, the
    walk over the rounds stopping above round `lowest_round`, the end of the text taken `end_slack` symbols early)."""
    a, b = bytes(a), bytes(b)
    len1 = len(a)
    t = _text(a, b, swap_sentinels)
    n = t.shape[0]
    ranks, sa = _rounds(t)
    p, q = sa[:-1], sa[1:]
    real = (p != len1) & (p != n - 1) & (q != len1) & (q != n - 1)
    keep = real & ((p < len1) != (q < len1))
    p, q = p[keep], q[keep]
    i, j, length = p.copy(), q.copy(), np.zeros(p.shape[0], np.int64)
    last = n - 1 - end_slack                                             # (a common prefix ends in front of the last sentinel)
    for r in range(len(ranks) - 1, lowest_round - 1, -1):
        step = 1 << r
        fits = (i + step <= last) & (j + step <= last)
        same = fits & (ranks[r][np.minimum(i, n - 1)] == ranks[r][np.minimum(j, n - 1)])
        i, j, length = i + same * step, j + same * step, length + same * step
    from_a = p < len1
    pos1 = np.where(from_a, p, q)
    pos2 = np.where(from_a, q, p) - (len1 + 1)
    hit = length >= m
    return [(int(x), int(y), int(z)) for x, y, z in zip(pos1[hit], pos2[hit], length[hit])]


def drop_overlapping(hits, len1, len2):
    """find_anchors.cpp:89-126: walk the hits in order, drop one that touches a site of either string that a kept hit covers"""
    used1, used2 = [False] * len1, [False] * len2
    kept = []
    for h in hits:
        s1, s2, length = h[0], h[1], h[2]
        if any(used1[s1:s1 + length]) or any(used2[s2:s2 + length]):
            continue
        used1[s1:s1 + length] = [True] * length
        used2[s2:s2 + length] = [True] * length
        kept.append(h)
    return kept
