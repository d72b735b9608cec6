"""A second, independent reading of the guide tree made from an alignment (include/pagan_host.h, "guide tree from an
alignment") in plain Python.

Two readings of the counts: a literal one -- a double loop over the columns of every pair of rows -- and a numpy one (a
validity matrix and one indicator matrix per letter, multiplied) for larger inputs.  The distance comes through
pycheck_guide.distance_of(match, both, 1, t), the tree and its clades from pycheck_guide.  Nothing here calls the library.
evolve_aligned makes aligned rows along a balanced tree whose clades are known."""
import numpy as np

import pycheck_guide as G


def resolve_type(rows, data_type=0):
    """1 / 2 / 3: as the guide's cleaning resolves it, over the rows with their gap characters dropped."""
    return G.clean(rows, data_type)[0]


def letter_code(c, t):
    """The code of one character, or -1 for no letter."""
    c = c.upper()
    if t != 2 and c == "U":
        c = "T"
    return G.core_letters(t).find(c) if len(c) == 1 else -1


def counts_literal(rows, data_type=0):
    """(both [n, n], match [n, n], type): column by column, pair by pair."""
    t = resolve_type(rows, data_type)
    n = len(rows)
    assert all(len(r) == len(rows[0]) for r in rows)
    both = np.zeros((n, n), np.int64)
    match = np.zeros((n, n), np.int64)
    for x in range(n):
        for y in range(n):
            for cx, cy in zip(rows[x], rows[y]):
                a, b = letter_code(cx, t), letter_code(cy, t)
                if a >= 0 and b >= 0:
                    both[x, y] += 1
                    if a == b:
                        match[x, y] += 1
    return both, match, t


def codes(rows, t):
    """[n, L] int8: the letters' codes, -1 for no letter."""
    core = G.core_letters(t)
    lut = np.full(256, -1, np.int8)
    for i, c in enumerate(core):
        lut[ord(c)] = lut[ord(c.lower())] = i
    if t != 2:
        lut[ord("U")] = lut[ord("u")] = core.index("T")
    L = len(rows[0]) if rows else 0
    assert all(len(r) == L for r in rows)
    raw = np.frombuffer("".join(rows).encode("latin-1"), np.uint8).reshape(len(rows), L)
    return lut[raw]


def counts_numpy(rows, data_type=0):
    """The same counts as integer matrix products (exact: float64 holds every count below 2^53)."""
    t = resolve_type(rows, data_type)
    a = codes(rows, t)
    v = (a >= 0).astype(np.float64)
    both = v @ v.T
    match = np.zeros_like(both)
    for c in range(len(G.core_letters(t))):
        e = (a == c).astype(np.float64)
        match += e @ e.T
    return both.astype(np.int64), match.astype(np.int64), t


def distances(both, match, t):
    """pycheck_guide.distance_of(match, both, 1, t) off the diagonal, once per distinct (match, both)."""
    n = both.shape[0]
    key, inv = np.unique(match.astype(np.int64) * (1 << 32) + both, return_inverse=True)
    val = np.array([G.distance_of(int(k >> 32), int(k & 0xFFFFFFFF), 1, t) for k in key], np.float64)
    d = val[inv.reshape(-1)].reshape(n, n)
    d[np.arange(n), np.arange(n)] = 0.0
    return d


def reading(rows, data_type=0, literal=False):
    """(both, match, dist, type)."""
    both, match, t = (counts_literal if literal else counts_numpy)(rows, data_type)
    return both, match, distances(both, match, t), t


def tree(names, rows, data_type=0):
    """The UPGMA tree of the reading, in synth.parse_newick's shape."""
    _, _, d, _ = reading(rows, data_type)
    return G.upgma_tree(names, d)


def evolve_aligned(n_leaves, columns, sub, gap_start, mean_len, seed, letters="ACGT"):
    """(names s0.., rows): a root of uniform codes, log2(n_leaves) doublings, every parent of a level in order giving two
    children by `mutate`: substitutions at rate `sub` (another letter, uniformly), then gaps that start at rate gap_start and
    cover 1 + geometric(1 / mean_len) columns.  Columns never move, so the rows are aligned; gaps are inherited."""
    rng = np.random.default_rng(seed)
    A = len(letters)

    def mutate(row):
        r = row.copy()
        hit = (rng.random(columns) < sub) & (r >= 0)
        r[hit] = (r[hit] + rng.integers(1, A, int(hit.sum()))) % A
        starts = np.nonzero(rng.random(columns) < gap_start)[0]
        for s in starts:
            r[s:s + 1 + int(rng.geometric(1.0 / mean_len))] = -1
        return r
    level = [rng.integers(0, A, columns)]
    while len(level) < n_leaves:
        level = [mutate(p) for p in level for _ in (0, 1)]
    assert len(level) == n_leaves
    names = ["s%d" % i for i in range(n_leaves)]
    show = np.frombuffer((letters + "-").encode(), np.uint8)                   # (code -1 is the last entry: a gap)
    return names, [bytes(show[r]).decode() for r in level]


def true_clades(n_leaves):
    """The clades of evolve_aligned's tree: the aligned blocks of 2, 4, ... leaves."""
    out, size = set(), 2
    while size <= n_leaves:
        for lo in range(0, n_leaves, size):
            out.add(frozenset("s%d" % i for i in range(lo, lo + size)))
        size *= 2
    return out
