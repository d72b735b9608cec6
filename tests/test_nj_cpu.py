"""Neighbour joining, the host side (no GPU): pagan_nj_newick -- the clamp, the midpoint rooting, the child order and the printed
lengths -- on the joins of the second reading (tests/pycheck_nj.py; the definition is in include/pagan_host.h), the reading
itself on trees whose answer is known, the refusals, the byte count, and what the device entries say without a device."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

from pagan2_msa_amd import abi, host, synth

import pycheck_nj as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _names(n):
    return ["t%d" % i for i in range(n)]


def _random_matrix(n, seed):
    a = np.random.default_rng(seed).random((n, n))
    return np.triu(a, 1) + np.triu(a, 1).T


def _code(fn, *args, **kw):
    from pagan2_msa_amd import PaganError
    with pytest.raises(PaganError) as e:
        fn(*args, **kw)
    return e.value.code


SIZES = (2, 3, 4, 5, 8, 65)


def _cases():
    out = []
    for n in SIZES:
        out.append(("random %d" % n, _random_matrix(n, 300 + n)))
        if n >= 3:
            out.append(("additive %d" % n, N.random_tree(n, 400 + n)[1]))
        out.append(("all equal %d" % n, np.full((n, n), 0.25) - 0.25 * np.eye(n)))
        out.append(("all zero %d" % n, np.zeros((n, n))))
        t = np.random.default_rng(500 + n).integers(0, 4, (n, n)).astype(np.float64)
        out.append(("integers %d" % n, np.triu(t, 1) + np.triu(t, 1).T))
    return out


@pytest.mark.parametrize("case", _cases(), ids=lambda c: c[0])
def test_newick_equals_the_reading_exactly(case):
    """Topology, child order and every printed length as a double."""
    _, dist = case
    names = _names(len(dist))
    rec = N.joins(dist)
    newick = host.nj_newick(names, *rec)
    tree, _ = N.root_tree(names, *rec)
    assert synth.parse_newick(newick) == tree
    assert newick == N.tree_newick(tree)
    assert sorted(re.findall(r"t\d+", newick)) == sorted(names)


def test_random_matrices_give_negative_raw_lengths_and_they_are_clamped():
    seen = 0
    for n in (5, 8, 65):
        dist = _random_matrix(n, 300 + n)
        ids, lens, sid, slen = N.joins(dist)
        seen += int((lens < 0).sum() + (slen < 0).sum())
        newick = host.nj_newick(_names(n), ids, lens, sid, slen)
        assert ":-" not in newick
    assert seen > 0
    # by hand: a negative raw length prints as 0, the other side keeps its own
    assert host.nj_newick(list("abc"), [], [], [0, 1, 2], [-1.0, 2.0, 4.0]) == "((a:0,b:2):1,c:3);"


@pytest.mark.parametrize("n", (3, 4, 5, 8, 17, 64, 65, 130))
def test_rooting_on_additive_dyadic_trees(n):
    """On an additive matrix with dyadic lengths every sum is exact: the reading recovers every split and every leaf edge, span is
    the matrix's largest entry (the brute force over all leaf pairs agrees), and the root is exactly half of it from the deepest
    leaf on either side."""
    names = _names(n)
    for seed in (1, 2, 3):
        edges, dist, splits, leaf_len = N.random_tree(n, 1000 * n + seed)
        ids, lens, sid, slen = N.joins(dist)
        assert N.splits_of_joins(n, ids, sid) == splits
        got = np.zeros(n)
        for (i, j), (li, lj) in zip(ids, lens):
            for c, l in ((i, li), (j, lj)):
                if c < n:
                    got[c] = l
        for c, l in zip(sid, slen):
            if c < n:
                got[c] = l
        assert np.array_equal(got, leaf_len)
        tree, facts = N.root_tree(names, ids, lens, sid, slen)
        assert facts["span"] == dist.max()
        longest, _ = N.brute_midpoint(n, [(a, b, l) for a, b, l in N.unrooted_edges(n, ids, lens, sid, slen)])
        assert longest == dist.max() == N.brute_midpoint(n, edges)[0]
        got_tree = synth.parse_newick(host.nj_newick(names, ids, lens, sid, slen))
        assert got_tree == tree
        half = dist.max() / 2
        assert N.deepest(got_tree[1]) + got_tree[1][-1] == half and N.deepest(got_tree[2]) + got_tree[2][-1] == half


def test_planted_ties():
    # n = 3, the star's offers (2, 2, 1): the first of the two largest carries the root, below = 2, above = 0 -- the root is ON the
    # star node, which stays in the tree as an ordinary binary node under an edge of length 0
    assert host.nj_newick(list("abc"), [], [], [0, 1, 2], [2.0, 2.0, 1.0]) == "(a:2,(b:2,c:1):0);"
    # the same with the root inside the star's edge: the star keeps two children and the edge above it
    assert host.nj_newick(list("abc"), [], [], [0, 1, 2], [1.0, 4.0, 2.0]) == "((a:1,c:2):1,b:3);"
    # a symmetric tree, two cherries of span 4 and a star of span 4: the first node in id order (5) is the top node, its first
    # child carries the root; the star ends up two levels down with one cherry and the odd leaf as its children
    ids, lens = [[0, 1], [2, 3]], [[2.0, 2.0], [2.0, 2.0]]
    newick = host.nj_newick(_names(5), ids, lens, [4, 5, 6], [0.0, 0.0, 0.0])
    assert newick == "(t0:2,(t1:2,((t2:2,t3:2):0,t4:0):0):0);"
    tree, facts = N.root_tree(_names(5), np.array(ids), np.array(lens), [4, 5, 6], [0.0, 0.0, 0.0])
    assert facts["top"] == 5 and facts["c"] == 0 and facts["span"] == 4.0 and N.tree_newick(tree) == newick
    # a later node wins only when strictly larger: make the second cherry longer
    newick = host.nj_newick(_names(5), ids, [[2.0, 2.0], [2.0, 2.5]], [4, 5, 6], [0.0, 0.0, 0.0])
    # node 6 (span 4.5) beats node 5, the star ties with it and does not replace it: the root is 2.25 above t3
    assert newick == "((((t0:2,t1:2):0,t4:0):0,t2:2):0.25,t3:2.25);"
    # the all-equal matrix: every Q ties, the pairs are taken in id order
    n = 6
    ids, lens, sid, slen = N.joins(np.full((n, n), 1.0) - np.eye(n))
    assert ids.tolist() == [[0, 1], [2, 3], [4, 5]] and sid.tolist() == [6, 7, 8]
    # the all-zero matrix: every length is 0 and the root sits above leaf 0
    ids, lens, sid, slen = N.joins(np.zeros((5, 5)))
    assert not lens.any() and not slen.any()
    newick = host.nj_newick(_names(5), ids, lens, sid, slen)
    assert synth.parse_newick(newick)[1] == ("leaf", "t0", 0.0) and newick.count(":0") == 8


def test_four_taxa_where_upgma_joins_the_wrong_pair():
    """A:1 and B:4 on one side of an inner edge of 1, C:1 and D:4 on the other: the long branches B and D are far from everything,
    UPGMA pairs the two short ones, neighbour joining recovers {A, B} | {C, D}."""
    names = list("ABCD")
    leaf = [1.0, 4.0, 1.0, 4.0]
    d = np.zeros((4, 4))
    for i in range(4):
        for j in range(4):
            if i != j:
                d[i, j] = leaf[i] + leaf[j] + (0.0 if i // 2 == j // 2 else 1.0)
    ids, lens, sid, slen = N.joins(d)
    assert N.splits_of_joins(4, ids, sid) == {frozenset([2, 3])}
    assert ids.tolist() == [[0, 1]] and lens.tolist() == [[1.0, 4.0]] and sid.tolist() == [2, 3, 4] and slen.tolist() == [1.0, 4.0, 1.0]

    def clades(t):
        if t[0] == "leaf":
            return frozenset([t[1]]), set()
        (a, ca), (b, cb) = clades(t[1]), clades(t[2])
        return a | b, ca | cb | {a | b}
    assert frozenset("AC") in clades(synth.parse_newick(host.guide_upgma(names, d)))[1]
    nj = clades(synth.parse_newick(host.nj_newick(names, ids, lens, sid, slen)))[1]
    assert frozenset("AC") not in nj and (frozenset("AB") in nj or frozenset("CD") in nj)
    assert host.nj_newick(names, ids, lens, sid, slen) == "((A:1,B:4):0.5,(C:1,D:4):0.5);"


def test_refusals():
    ids, lens, sid, slen = N.joins(_random_matrix(5, 1))
    good = _names(5)
    for bad in ("a(b", "a:b", "a b", "a,b", "a;b", "a)b", "a\tb", ""):
        assert _code(host.nj_newick, good[:4] + [bad], ids, lens, sid, slen) == abi.PAGAN_E_ARG
        assert _code(host.nj_tree, ["x", bad], np.ones((2, 2))) == abi.PAGAN_E_ARG
    # n
    assert _code(host.nj_tree, ["x"], np.zeros((1, 1))) == abi.PAGAN_E_ARG
    assert _code(host.nj_joins, np.zeros((1, 1))) == abi.PAGAN_E_ARG
    assert _code(host.nj_newick, ["x"], [], [], [0, 1, -1], [0.0, 0.0, 0.0]) == abi.PAGAN_E_ARG
    assert _code(host.nj_predict_bytes, 1) == abi.PAGAN_E_ARG
    assert _code(host.nj_predict_bytes, host.NJ_MAX_SEQS + 1) == abi.PAGAN_E_ARG
    L = host._lib()                                        # one cluster too many: refused before the matrix is looked at
    one = np.zeros(1)
    assert L.pagan_nj_joins(host.NJ_MAX_SEQS + 1, abi._dp(one), None, None, None, None, None) == abi.PAGAN_E_ARG
    assert L.pagan_nj_tree(host.NJ_MAX_SEQS + 1, None, abi._dp(one), None, 0, None) == abi.PAGAN_E_ARG
    # entries above the diagonal: not finite, negative (before any device is asked for)
    for v in (-1.0, np.nan, np.inf):
        d = _random_matrix(4, 2)
        d[1, 3] = v
        assert _code(host.nj_joins, d) == abi.PAGAN_E_ARG
        assert _code(host.nj_tree, _names(4), d) == abi.PAGAN_E_ARG
    # joins that are no tree
    assert _code(host.nj_newick, good, [[1, 0], [2, 5]], lens, sid, slen) == abi.PAGAN_E_ARG          # i >= j
    assert _code(host.nj_newick, good, [[0, 1], [0, 2]], lens, [3, 4, 6], slen) == abi.PAGAN_E_ARG      # 0 is gone by then
    assert _code(host.nj_newick, good, [[0, 1], [2, 6]], lens, [3, 4, 5], slen) == abi.PAGAN_E_ARG      # 6 is made by this join
    assert _code(host.nj_newick, good, ids, lens, [sid[1], sid[0], sid[2]], slen) == abi.PAGAN_E_ARG    # the star out of order
    assert _code(host.nj_newick, good, ids, np.full((2, 2), np.nan), sid, slen) == abi.PAGAN_E_ARG
    assert _code(host.nj_newick, good, ids, lens, sid, [0.0, np.inf, 0.0]) == abi.PAGAN_E_ARG
    with pytest.raises(ValueError):
        host.nj_newick(good, ids[:1], lens[:1], sid, slen)
    with pytest.raises(ValueError):
        host.nj_tree(good, np.zeros((4, 4)))
    for fn, args in ((host.guide_tree, (["a", "b"], ["ACGT", "ACGT"])), (host.aln_tree, (["a", "b"], ["ACGT", "ACGT"]))):
        with pytest.raises(ValueError):
            fn(*args, method="bionj")
    with pytest.raises(ValueError):
        host.Msa(["a", "b"], ["ACGT", "ACGT"], "(a:1,b:1);", tree_method="ml")
    with pytest.raises(ValueError):
        host.align_refined(["a", "b"], ["ACGT", "ACGT"], newick="(a:1,b:1);", tree_method="")


def test_predict_bytes():
    up = lambda x: (x + 255) // 256 * 256                 # noqa: E731
    assert host.nj_predict_bytes(2) == 0
    for n in (3, 4, 65, 600, host.NJ_MAX_SEQS):
        want = up(8 * n * n) + up(8 * n) + up(4 * n) + up(24 * n) + up(16) + up(24 * (n - 3) + 40)
        assert host.nj_predict_bytes(n) == want
    assert host.nj_predict_bytes(host.NJ_MAX_SEQS) >= 2 << 30


def test_new_symbols_are_exported(pg):
    lib = pg.lib()
    for sym in ("pagan_nj_joins", "pagan_nj_newick", "pagan_nj_tree", "pagan_nj_predict_bytes"):
        assert sym in host.HOST_EXPORTED and sym in host.PROTOTYPES and getattr(lib, sym) is not None
    assert C.sizeof(host.CNjInfo) == 4 * 4 + 2 * 8 + 5 * 8
    with open(os.path.join(ROOT, "include", "pagan_host.h")) as f:
        assert "#define PAGAN_NJ_MAX_SEQS %d\n" % host.NJ_MAX_SEQS in f.read()


def test_without_a_device_the_device_entries_say_so(pg):
    names, seqs, newick = synth.evolve_balanced(4, 200, seed=3)
    if pg.device_count() > 0:                            # (on a GPU machine: the same calls work)
        d = _random_matrix(4, 4)
        assert host.nj_tree(_names(4), d) == host.nj_newick(_names(4), *host.nj_joins(d)[:4])
        return
    for n in (2, 3, 4, 9):
        d = _random_matrix(n, n)
        assert _code(host.nj_joins, d) == abi.PAGAN_E_NODEVICE
        assert _code(host.nj_tree, _names(n), d) == abi.PAGAN_E_NODEVICE
    rows = [s[:150].ljust(150, "-") for s in seqs]
    assert _code(host.guide_tree, names, seqs, method="nj") == abi.PAGAN_E_NODEVICE
    assert _code(host.aln_tree, names, rows, method="nj") == abi.PAGAN_E_NODEVICE
    assert _code(host.Msa, names, seqs, tree_method="nj") == abi.PAGAN_E_NODEVICE
    assert _code(host.align_refined, names, seqs, tree_method="nj") == abi.PAGAN_E_NODEVICE
    msa = host.Msa(names, seqs, newick, tree_method="nj")          # with a tree: as before
    assert msa.newick == newick and msa.n_internal == 3
    assert _code(msa.alignment_tree, method="nj") == abi.PAGAN_E_ARG      # (not aligned yet: the rows do not exist)


def test_join_kernels_have_no_scratch():
    """dp_nj.hip compiled afresh to gfx950 assembly (no GPU needed): from the kernel metadata, the scan, the pick and the merge
    have no private segment and spill nothing."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import check_scratch
    finally:
        sys.path.pop(0)
    funcs, meta = check_scratch.analyse(check_scratch.assemble("dp_nj.hip"))
    for kernel in ("nj_scan", "nj_pick", "nj_merge"):
        found = {k: v for k, v in meta.items() if kernel in k and v}
        assert len(found) == 1, sorted(meta)
        for k, v in found.items():
            assert v["private_segment_fixed_size"] == 0 and v["vgpr_spill_count"] == 0 and v["sgpr_spill_count"] == 0, (k, v)
    assert not [k for k in funcs if "nj_" in k], funcs               # (a function is listed only if it touches scratch)
