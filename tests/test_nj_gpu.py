"""Neighbour joining on the device: the join records of nj_scan / nj_pick / nj_merge (csrc/dp_nj.hip) against the second reading
(tests/pycheck_nj.py) -- the ids equal, the lengths equal as bytes, no tolerance: the definition in include/pagan_host.h fixes
every operation -- at the edges of a lane, a wave and the 64-wide row-sum tree, with active-row counts that cross a workgroup of
the scan (4 rows), of the pick (256 records) and of the merge (256 slots); exact ties; and the entries above it, up to the walk."""
import numpy as np
import pytest

from pagan2_msa_amd import host, synth

import pycheck_nj as N

pytestmark = pytest.mark.gpu

SIZES = (4, 5, 63, 64, 65, 130, 257)


def _names(n):
    return ["t%d" % i for i in range(n)]


def _random_matrix(n, seed):
    a = np.random.default_rng(seed).random((n, n))
    return np.triu(a, 1) + np.triu(a, 1).T


def check(dist):
    """One device call against the reading, byte for byte; returns the device's records and its info."""
    n = len(dist)
    ids, lens, sid, slen, info = host.nj_joins(dist)
    ids0, lens0, sid0, slen0 = N.joins(dist)
    assert np.array_equal(ids, ids0) and np.array_equal(sid, sid0)
    assert lens.tobytes() == lens0.tobytes() and slen.tobytes() == slen0.tobytes()
    joins = max(n - 3, 0)
    assert (info["n"], info["joins"]) == (n, joins)
    assert info["launches"] == (3 * joins + 2 if n >= 3 else 0)
    assert info["device_bytes"] == host.nj_predict_bytes(n)
    assert info["scan_entries"] == sum(r * (r - 1) // 2 for r in range(4, n + 1))
    return ids, lens, sid, slen, info


@pytest.mark.parametrize("n", (2, 3) + SIZES)
def test_random_matrices(n):
    check(_random_matrix(n, 700 + n))


@pytest.mark.parametrize("n", SIZES)
def test_additive_dyadic_trees_and_their_splits(n):
    _, dist, splits, leaf_len = N.random_tree(n, 800 + n)
    ids, lens, sid, slen, _ = check(dist)
    assert N.splits_of_joins(n, ids, sid) == splits
    got = np.zeros(n)
    for c, l in list(zip(ids.ravel(), lens.ravel())) + list(zip(sid, slen)):
        if c < n:
            got[c] = l
    assert np.array_equal(got, leaf_len)


@pytest.mark.parametrize("n", (4, 5, 64, 65, 130))
def test_exact_ties(n):
    """Few distinct integer values: many pairs share the smallest Q, in one row and across rows, waves and workgroups."""
    t = np.random.default_rng(900 + n).integers(0, 3, (n, n)).astype(np.float64)
    check(np.triu(t, 1) + np.triu(t, 1).T)
    check(np.full((n, n), 0.25))                          # (the diagonal is not read)
    check(np.zeros((n, n)))


def test_six_hundred(monkeypatch):
    """More active rows than one pass of anything: 150 workgroups of the scan, three strides of the pick, three blocks of the merge.
    The stage times are measured on request only, and the events between the launches change no byte."""
    dist = _random_matrix(600, 6)
    ids, lens, _, _, info = check(dist)
    assert info["scan_ms"] == 0 and info["pick_ms"] == 0 and info["merge_ms"] == 0 and info["loop_ms"] > 0
    monkeypatch.setenv("PAGAN_NJ_EVENTS", "1")
    ids1, lens1, _, _, info = host.nj_joins(dist)
    assert info["scan_ms"] > 0 and info["pick_ms"] > 0 and info["merge_ms"] > 0 and info["loop_ms"] > 0
    assert ids1.tobytes() == ids.tobytes() and lens1.tobytes() == lens.tobytes()


def test_repeatable_and_the_tree_is_the_joins_tree():
    dist = _random_matrix(130, 11)
    a, b = host.nj_joins(dist), host.nj_joins(dist)
    for x, y in zip(a[:4], b[:4]):
        assert x.tobytes() == y.tobytes()
    names = _names(130)
    newick, info = host.nj_tree(names, dist, with_info=True)
    assert newick == host.nj_newick(names, *a[:4]) and host.nj_tree(names, dist) == newick
    assert info["root_ms"] > 0 and info["joins"] == 127
    for n in (2, 3, 4):
        d = _random_matrix(n, n)
        assert host.nj_tree(_names(n), d) == host.nj_newick(_names(n), *N.joins(d))


def test_the_upper_triangle_alone_is_read():
    dist = _random_matrix(9, 3)
    want = host.nj_tree(_names(9), dist)
    lower = dist.copy()
    lower[np.tril_indices(9)] = -7.0
    assert host.nj_tree(_names(9), lower) == want


@pytest.fixture(scope="module")
def family():
    return synth.evolve_balanced(8, 300, branch=0.05, sub=0.05, indel_start=0.01, seed=21)


def test_guide_tree_and_aln_tree_by_nj(family):
    names, seqs, _ = family
    _, _, dist, _ = host.guide_distances(seqs)
    newick, info = host.guide_tree(names, seqs, method="nj", with_info=True)
    assert newick == host.nj_tree(names, dist) and info["nj"]["joins"] == 5 and info["pairs"] == 28
    width = max(len(s) for s in seqs)
    rows = [s.ljust(width, "-") for s in seqs]
    _, _, adist, _ = host.aln_distances(rows)
    newick, info = host.aln_tree(names, rows, method="nj", with_info=True)
    assert newick == host.nj_tree(names, adist) and info["nj"]["joins"] == 5 and info["columns"] == width
    # the default is what it was
    assert host.guide_tree(names, seqs, method="upgma") == host.guide_tree(names, seqs) == host.guide_upgma(names, dist)
    assert host.aln_tree(names, rows, method="upgma") == host.aln_tree(names, rows) == host.guide_upgma(names, adist)
    assert host.guide_tree(names, seqs, with_info=True, method="upgma")[1].keys() == host.guide_tree(names, seqs, with_info=True)[1].keys()


def test_the_walk_on_a_neighbour_joining_tree(family):
    names, seqs, _ = family
    msa = host.Msa(names, seqs, tree_method="nj")
    assert msa.newick == host.guide_tree(names, seqs, method="nj")
    assert sorted(synth_leaves(msa.newick)) == sorted(names)
    msa.align()
    rows = msa.alignment()
    assert [r.replace("-", "") for r in rows] == seqs
    assert msa.alignment_tree(method="nj") == host.aln_tree(names, rows, data_type=msa.data_type, method="nj")
    assert msa.alignment_tree(method="upgma") == msa.alignment_tree()
    default = host.Msa(names, seqs)
    assert default.newick == host.Msa(names, seqs, tree_method="upgma").newick == host.guide_tree(names, seqs)


def synth_leaves(newick):
    def walk(t):
        return [t[1]] if t[0] == "leaf" else walk(t[1]) + walk(t[2])
    return walk(synth.parse_newick(newick))


def test_align_refined_by_nj(family):
    names, seqs, _ = family
    msa = host.align_refined(names, seqs, rounds=1, tree_method="nj")
    assert [r.replace("-", "") for r in msa.alignment()] == seqs
    assert msa.history[0]["newick"] == host.guide_tree(names, seqs, method="nj")
    if len(msa.history) > 1:
        first = host.Msa(names, seqs, msa.history[0]["newick"]).align()
        assert msa.history[1]["newick"] == first.alignment_tree(method="nj")
    fitted = host.align_refined(names, seqs, rounds=1, tree_method="nj", branch_lengths="ml")
    assert [r.replace("-", "") for r in fitted.alignment()] == seqs and "loglik" in fitted.history[0]
    a, b = host.align_refined(names, seqs, rounds=1), host.align_refined(names, seqs, rounds=1, tree_method="upgma")
    assert a.alignment() == b.alignment() and [h["newick"] for h in a.history] == [h["newick"] for h in b.history]
