"""GPU: the prefix-anchor finder on the device (dp_anchors.hip: suffix array by prefix doubling with library sorts, common
prefixes from the rounds' rank arrays).  Which list is compared where:

* the RAW list -- the adjacent cross-string pairs in suffix-array order, as the device produces them, before the sort by
  length and the overlap filter (host.prefix_hits_raw(device=True): no length threshold, no cap on finders in flight) -- is
  compared, exactly and in order, with find_anchors.cpp:35-85 read literally in Python (tests/pycheck_anchors.py) on the
  small and degenerate families of tests/test_pycheck_anchors_cpu.py, with that file's numpy doubling on its larger inputs,
  and with the host's raw list (pinned by the same readings in that file) on homologous pairs up to the largest accepted
  text, 2^20 - 2 symbols;
* the FILTERED list (host.prefix_hits: what the walk uses) of device and host on the homologous pairs, under eight threads,
  and where the device declines a text;
* the tunnels made of it: against the oracle's restatement of find_long_substrings (through define_tunnel), and every
  internal node's band of a tree walk against the same walk with the finder kept on the host."""
import functools
import threading

import numpy as np
import pytest

from pagan2_msa_amd import host, synth
from test_pycheck_anchors_cpu import cases, doubling_of, families, larger, naive_of, same_rows

pytestmark = pytest.mark.gpu

PAGAN_E_NODEVICE = -5
N_MAX = (1 << 20) - 2                    # the largest text (len1 + len2 + 2) the device's finder accepts: 20-bit ranks


@functools.lru_cache(maxsize=None)
def pair(length, seed, sub=0.02, indel=0.004):
    names, seqs, _ = synth.evolve_balanced(2, length, branch=0.02, sub=sub, indel_start=indel, mean_len=4, seed=seed)
    return seqs[0], seqs[1]


@functools.lru_cache(maxsize=None)
def host_raw(a, b, m):
    """the host's raw list, computed once for every test that needs it"""
    return host.prefix_hits_raw(a, b, m)


@functools.lru_cache(maxsize=None)
def largest(kind, n=N_MAX):
    """(a, b, min_length) with len(a) + len(b) + 2 == n"""
    len1 = (n - 2) // 2
    len2 = n - 2 - len1
    if kind == "runs":
        return b"A" * len1, b"A" * len2, 200000
    rng = np.random.default_rng(77)
    x = rng.integers(0, 4, len1 + 1)
    y = x[:len2].copy()
    where = rng.random(len2) < 0.02
    y[where] = (y[where] + rng.integers(1, 4, int(where.sum()))) % 4
    code = np.frombuffer(b"ACGT", np.uint8)
    return code[x[:len1]].tobytes(), code[y].tobytes(), 30


@pytest.mark.parametrize("name,k", cases())
def test_device_raw_list_equals_the_literal_reading(pg, name, k):
    """the kernels on texts far below the walk's 16,384 threshold: block boundaries, empty strings, no hit at all, one-letter
    runs, identical strings (more hits than the sort's key array holds records), bytes >= 0x80"""
    a, b, m = families()[name][k]
    assert same_rows(host.prefix_hits_raw(a, b, m, device=True), naive_of(name, k))


@pytest.mark.parametrize("name", ["long_runs", "long_period", "pair_20k"])
def test_device_raw_list_equals_doubling_on_larger_inputs(pg, name):
    a, b, m = larger()[name]
    assert same_rows(host.prefix_hits_raw(a, b, m, device=True), doubling_of(name))


@pytest.mark.parametrize("length,seed", [(9000, 2), (20000, 3), (100000, 4)])
def test_device_hits_equal_host_hits(pg, monkeypatch, length, seed):
    a, b = pair(length, seed)
    monkeypatch.setenv("PAGAN_ANCHORS", "host")
    want = host.prefix_hits(a, b, 30)
    monkeypatch.delenv("PAGAN_ANCHORS")
    before = host.anchors_device_calls()
    got = host.prefix_hits(a, b, 30)
    assert host.anchors_device_calls() == before + 1, "the device's finder is meant to have run"
    assert len(want) > 0, "the pair is meant to share long substrings"
    assert np.array_equal(got, want)
    # the list as the device produces it, before a longer hit can hide a wrong one
    raw = host.prefix_hits_raw(a, b, 30, device=True)
    assert host.anchors_device_calls() == before + 1, "the raw seam is not counted"
    assert raw.shape[0] >= want.shape[0] and same_rows(raw, host_raw(a, b, 30))


@pytest.mark.parametrize("kind", ["pair", "runs"])
def test_largest_accepted_text(pg, kind):
    a, b, m = largest(kind)
    assert len(a) + len(b) + 2 == N_MAX
    want = host_raw(a, b, m)
    assert want.shape[0] > 1000
    assert same_rows(host.prefix_hits_raw(a, b, m, device=True), want)


def test_one_symbol_more_is_refused_and_the_host_answers(pg, monkeypatch):
    a, b, m = largest("pair", N_MAX + 1)
    assert len(a) + len(b) + 2 == N_MAX + 1
    with pytest.raises(RuntimeError, match="error %d$" % PAGAN_E_NODEVICE):
        host.prefix_hits_raw(a, b, m, device=True)
    before = host.anchors_device_calls()
    got = host.prefix_hits(a.decode(), b.decode(), m)
    assert host.anchors_device_calls() == before
    monkeypatch.setenv("PAGAN_ANCHORS", "host")
    want = host.prefix_hits(a.decode(), b.decode(), m)
    assert want.shape[0] > 1000 and np.array_equal(got, want)


def test_scratch_is_reused_across_sizes(pg):
    """one finder's scratch grows, is reused by smaller texts, grows again, and is rebuilt after the cache is released"""
    def device_raw(case):
        return host.prefix_hits_raw(*case, device=True)
    a, b = pair(100000, 4)
    assert same_rows(device_raw((a, b, 30)), host_raw(a, b, 30))
    assert same_rows(device_raw(families()["one"][0]), naive_of("one", 0))
    assert same_rows(device_raw(families()["same"][0]), naive_of("same", 0))
    assert same_rows(device_raw(largest("pair")), host_raw(*largest("pair")))
    for k in range(len(families()["edges"])):
        assert same_rows(device_raw(families()["edges"][k]), naive_of("edges", k)), "edges %d" % k
    pg.lib().pagan_dp_release_cache()
    assert same_rows(device_raw(families()["period"][0]), naive_of("period", 0))


def test_eight_threads_share_the_finders(pg, monkeypatch):
    """the walk's situation: more preparing threads than the four finders the device is shared between"""
    pairs = [pair(length, 30 + t) for t, length in enumerate((17000, 20000, 23000, 26000, 29000, 32000, 36000, 40000))]
    monkeypatch.setenv("PAGAN_ANCHORS", "host")
    want = [host.prefix_hits(a, b, 30) for a, b in pairs]
    monkeypatch.delenv("PAGAN_ANCHORS")
    assert all(w.shape[0] > 0 for w in want)
    before = host.anchors_device_calls()
    for _round in range(2):
        got = [None] * len(pairs)

        def work(t):
            got[t] = host.prefix_hits(pairs[t][0], pairs[t][1], 30)
        threads = [threading.Thread(target=work, args=(t,)) for t in range(len(pairs))]
        for th in threads:
            th.start()
        for th in threads:
            th.join()
        for t in range(len(pairs)):
            assert got[t] is not None and np.array_equal(got[t], want[t]), "thread %d" % t
    assert before + 1 <= host.anchors_device_calls() <= before + 16


def test_repeats_and_short_strings(pg, oracle):
    """low-complexity strings: long repeats make the doubling run many rounds; many equal common prefixes"""
    rng = np.random.default_rng(5)
    unit = "".join(rng.choice(list("ACGT"), 37))
    a = unit * 40 + "".join(rng.choice(list("ACGT"), 9000)) + "A" * 300
    b = "".join(rng.choice(list("ACGT"), 8000)) + unit * 35 + "A" * 250 + unit[:20]
    from pycheck_anchors import doubling
    want = np.array(doubling(a.encode(), b.encode(), 12), np.int32).reshape(-1, 3)
    assert want.shape[0] > 1000
    assert same_rows(host.prefix_hits_raw(a, b, 12), want), "the host's raw list"
    assert same_rows(host.prefix_hits_raw(a, b, 12, device=True), want), "the device's raw list"
    # (the oracle's finder is reached through define_tunnel)
    band, n = host.define_tunnel(a, b, a, b, prefix_hit_length=12)
    oband, on = oracle.define_tunnel(oracle.OGraph.leaf(a), oracle.OGraph.leaf(b), min_length=12)
    assert n == on and np.array_equal(band.upper, oband.upper) and np.array_equal(band.lower, oband.lower)


def test_tunnels_of_a_tree_walk_use_the_device_finder(pg, oracle, monkeypatch):
    names, seqs, nwk = synth.evolve_balanced(8, 9000, branch=0.01, sub=0.008, indel_start=0.0008, mean_len=4.0, seed=7)
    before = host.anchors_device_calls()
    msa = host.Msa(names, seqs, nwk, use_anchors=1).align()
    assert host.anchors_device_calls() >= before + 3          # (the upper levels at least: a wide level shares the device four ways at most)
    for k in range(msa.n_internal):
        l, r, m, b = msa.node_job(k)
        want = oracle.dp_align(l, r, m, b)
        assert msa.node_result(k).same_alignment(want), "node %d" % k
    # the oracle above is handed the band the walk made: the band itself against the same walk with the host's finder
    monkeypatch.setenv("PAGAN_ANCHORS", "host")
    before = host.anchors_device_calls()
    on_host = host.Msa(names, seqs, nwk, use_anchors=1).align()
    assert host.anchors_device_calls() == before
    assert on_host.n_internal == msa.n_internal
    for k in range(msa.n_internal):
        band, hband = msa.node_job(k)[3], on_host.node_job(k)[3]
        assert band is not None and hband is not None, "node %d is meant to be banded" % k
        assert np.array_equal(band.upper, hband.upper) and np.array_equal(band.lower, hband.lower), "node %d" % k
