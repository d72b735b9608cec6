"""CPU: the raw list of the prefix-anchor finder -- the adjacent cross-string pairs of the suffix array, in its order, before
the sort by length and the overlap filter (host.prefix_hits_raw, the host's builder in csrc/host_anchors.cpp) -- against two
readings that share no code with it (tests/pycheck_anchors.py): find_anchors.cpp:35-85 read literally (naive) on small and
degenerate inputs, prefix doubling in numpy (doubling) where the literal reading is quadratic.  doubling is held to naive on
every family first, and three deliberately wrong variants of it show that the families tell such errors apart.  Then the
filter step of host.prefix_hits from the raw list, and the oracle's own finder (stable_sort + strcmp, reached through
define_tunnel) on the repetitive families.  Every comparison is exact and in order.

tests/test_anchors_gpu.py runs the same families, and the same references, through the device's finder."""
import functools

import numpy as np
import pytest

import pycheck_anchors as pa
from pagan2_msa_amd import host


def letters(rng, n, alphabet="ACGT"):
    return "".join(rng.choice(list(alphabet), n)).encode() if n else b""


def substituted(rng, s, k):
    """a copy of s with k sites changed to another letter"""
    t = bytearray(s)
    for i in rng.choice(len(t), k, replace=False):
        t[i] = rng.choice([c for c in b"ACGT" if c != t[i]])
    return bytes(t)


@functools.lru_cache(maxsize=None)
def families():
    """name -> [(a, b, min_length), ...]"""
    rng = np.random.default_rng(20260)
    f = {}
    f["one"] = [(b"A", b"A", 1)]
    f["empty"] = [(b"", b"ACGT", 1), (b"A", b"", 1)]
    f["runs"] = [(b"A" * 50, b"A" * 33, 5), (b"A" * 50, b"A" * 33, 1)]
    u = letters(rng, 37)
    f["period"] = [(u * 9, u * 7 + u[:20], 12)]
    f["ac"] = [(b"AC" * 100, b"CA" * 90, 7)]
    f["two"] = [(letters(rng, 300, "AC"), letters(rng, 280, "AC"), 4)]
    f["tail"] = [(letters(rng, 200) + b"ACGTACGT", letters(rng, 100) + b"ACGTACGT", 4)]
    s = letters(rng, 3000)
    f["same"] = [(s, s, 1)]
    f["bytes"] = [(b"\x01\xff" * 20 + b"A", b"\xff\x01" * 15 + b"A", 2)]
    h = letters(rng, 400)
    f["homol"] = [(h, substituted(rng, h, 12), 8)]
    f["none"] = [(letters(rng, 500), letters(rng, 500), 30)]
    edges = []
    for n in (255, 256, 257, 511, 512, 513, 1023, 1024, 1025):           # n = len1 + len2 + 2: the launch blocks hold 256
        len1 = (n - 2) // 2
        a = letters(rng, len1)
        edges.append((a, substituted(rng, a, len1 // 40) + letters(rng, n - 2 - 2 * len1), 8))
    f["edges"] = edges
    return f


def cases():
    return [(name, k) for name, group in families().items() for k in range(len(group))]


@functools.lru_cache(maxsize=None)
def naive_of(name, k):
    """the literal reading of a family's case, computed once for every test that needs it (the device's tests as well)"""
    return as_rows(pa.naive(*families()[name][k]))


@functools.lru_cache(maxsize=None)
def larger():
    """name -> (a, b, min_length): inputs on which the literal reading is too slow"""
    rng = np.random.default_rng(20261)
    u = letters(rng, 41)
    x = letters(rng, 20000)
    return {"long_runs": (b"A" * 9000, b"A" * 8000, 1000),
            "long_period": (u * 300, letters(rng, 3000) + u * 250, 12),
            "pair_20k": (x, substituted(rng, x, 300), 30)}


@functools.lru_cache(maxsize=None)
def doubling_of(name):
    return as_rows(pa.doubling(*larger()[name]))


def as_rows(hits):
    return np.array(hits, np.int32).reshape(-1, 3)


def same_rows(got, want):
    return got.shape == want.shape and np.array_equal(got, want)


@pytest.mark.parametrize("name,k", cases())
def test_host_raw_list_and_doubling_equal_the_literal_reading(pg, name, k):
    a, b, m = families()[name][k]
    want = naive_of(name, k)
    assert same_rows(host.prefix_hits_raw(a, b, m), want), "the host's raw list"
    assert same_rows(as_rows(pa.doubling(a, b, m)), want), "the doubling reading"
    # every reported pair is a common substring of that length which cannot be extended to the right
    for s1, s2, length in want.tolist():
        assert length >= m and a[s1:s1 + length] == b[s2:s2 + length]
        assert s1 + length == len(a) or s2 + length == len(b) or a[s1 + length] != b[s2 + length]


def test_the_families_have_the_hits_they_are_there_for():
    n_hits = {name: [naive_of(name, k).shape[0] for k in range(len(group))] for name, group in families().items()}
    assert n_hits["one"] == [1] and n_hits["empty"] == [0, 0] and n_hits["none"] == [0]
    assert n_hits["same"][0] >= 2990, "identical strings, min_length 1: nearly every adjacent pair is a hit"
    assert n_hits["runs"][1] == 2 * 33, "one-letter runs: the suffixes of either string alternate"
    for name in ("runs", "period", "ac", "two", "tail", "bytes", "homol", "edges"):
        assert all(c > 0 for c in n_hits[name]), name


WRONG = {"sentinels swapped": dict(swap_sentinels=True),
         "lowest round left out": dict(lowest_round=1),
         "end of text one early": dict(end_slack=1)}


@pytest.mark.parametrize("variant", sorted(WRONG))
def test_a_wrong_doubling_is_caught_by_some_family(variant):
    caught = [name for name, k in cases()
              if not same_rows(as_rows(pa.doubling(*families()[name][k], **WRONG[variant])), naive_of(name, k))]
    print(variant, "differs on", sorted(set(caught)))
    assert caught, "no family tells this variant from the literal reading"


@pytest.mark.parametrize("name", ["long_runs", "long_period", "pair_20k"])
def test_host_raw_list_equals_doubling_on_larger_inputs(pg, name):
    a, b, m = larger()[name]
    want = doubling_of(name)
    assert want.shape[0] > 0
    assert same_rows(host.prefix_hits_raw(a, b, m), want)


def filtered_from_raw(raw, filtered, len1, len2):
    """The overlap filter (stated in pycheck_anchors) over a length-sorted permutation of the raw list.  std::sort is not stable,
    so the order among hits of one length is the product's: the survivors in the order the product lists them, the others
    behind them (a hit that was dropped touches a kept hit that is at least as long, which stands in front of it here too)."""
    place = {tuple(h[:3]): i for i, h in enumerate(filtered.tolist())}
    rows = [tuple(h) for h in raw.tolist()]
    rows.sort(key=lambda h: (-h[2], place.get(h, len(place))))
    return as_rows(pa.drop_overlapping(rows, len1, len2))


@pytest.mark.parametrize("name,k", [c for c in cases() if c[0] != "bytes"] + [(n, None) for n in ("long_runs", "long_period", "pair_20k")])
def test_filtered_list_is_the_overlap_filter_of_the_sorted_raw_list(pg, name, k):
    a, b, m = larger()[name] if k is None else families()[name][k]
    raw = host.prefix_hits_raw(a, b, m)
    got = host.prefix_hits(a.decode(), b.decode(), m)
    assert np.array_equal(got[:, 2], got[:, 3]), "a prefix hit's score is its length"
    assert np.all(got[:-1, 2] >= got[1:, 2]), "sorted by length"
    assert len({tuple(h) for h in got[:, :3].tolist()}) == got.shape[0] and {tuple(h) for h in got[:, :3].tolist()} <= {tuple(h) for h in raw.tolist()}
    assert same_rows(filtered_from_raw(raw, got, len(a), len(b)), got[:, :3])


@pytest.mark.parametrize("name,k", [("runs", 0), ("runs", 1), ("period", 0), ("tail", 0), ("homol", 0)])
def test_tunnel_equals_the_oracles_on_repetitive_leaves(oracle, pg, name, k):
    """the oracle finds its hits with stable_sort + strcmp (quadratic on repeats: under 2,000 symbols)"""
    a, b, m = families()[name][k]
    a, b = a.decode(), b.decode()
    assert len(a) + len(b) < 2000
    band, n = host.define_tunnel(a, b, a, b, prefix_hit_length=m)
    oband, on = oracle.define_tunnel(oracle.OGraph.leaf(a), oracle.OGraph.leaf(b), min_length=m)
    assert n == on and n > 0
    assert np.array_equal(band.upper, oband.upper) and np.array_equal(band.lower, oband.lower)
