"""Guide tree from the sequences, the host side (no GPU): the Python readings agree among themselves, and the library's
host-only entries -- UPGMA, the distance formula, the default k, the refusals -- agree with the reading
(tests/pycheck_guide.py; the definition is in include/pagan_host.h)."""
import ctypes as C
import math

import numpy as np
import pytest

from pagan2_msa_amd import abi, host, synth

import pycheck_guide as G


def small_families():
    """(label, sequences, data_type, k): what the fast readings must agree with the literal one on."""
    fam = []
    _, seqs, _ = synth.evolve_balanced(4, 120, branch=0.05, sub=0.05, indel_start=0.01, seed=1)
    fam.append(("dna4", seqs, 1, 6))
    fam.append(("dna4 default k", seqs, 0, 0))
    _, prot, _ = synth.evolve_balanced(4, 90, sub=0.05, indel_start=0.01, seed=2, alphabet=G.PROTEIN)
    fam.append(("protein4", prot, 2, 2))
    fam.append(("protein4 guessed", prot, 0, 3))
    fam.append(("degenerate", ["A" * 100, "A" * 37, "", "ACG", "acgu-ac\nGTNNACGTACGT", "ACGTACGTAC"], 1, 3))
    fam.append(("codon as dna", ["ATGGCCAAATTT", "ATGGCAAAATTT", "ATGNNNAAATTT"], 3, 3))
    fam.append(("protein x", ["ARNDXCQEUGHILK", "ARNDCQEGHILKBZ", "VVVVVVVV"], 2, 2))
    return fam


@pytest.mark.parametrize("fam", small_families(), ids=lambda f: f[0])
def test_fast_readings_equal_the_literal_one(fam):
    _, seqs, data_type, k = fam
    s0, m0, d0, k0, t0 = G.distances_literal(seqs, data_type, k)
    s1, m1, d1, k1, t1 = G.distances_unique(seqs, data_type, k)
    assert (k0, t0) == (k1, t1)
    assert np.array_equal(s0, s1) and np.array_equal(m0, m1) and np.array_equal(d0, d1)
    A = 20 if t0 == 2 else 4
    if A ** k0 <= 1 << 16:
        s2, m2 = G.shared_dense(seqs, data_type, k0)
        assert np.array_equal(s0, s2) and np.array_equal(m0, m2)


def test_literal_reading_on_cases_worked_by_hand():
    s, m, d, k, t = G.distances_literal(["A" * 100, "A" * 37, "acgu-ac\nGTNNACGTACGT"], 1, 3)
    assert t == 1 and list(m) == [98, 35, 6 + 6]                    # ACGTACGT (U -> T) | NN | ACGTACGT
    assert s[0, 1] == 35 and s[0, 2] == 0 and d[0, 1] == 0.0
    assert d[0, 2] == -0.75 * math.log(1.0 - 0.7 / 0.75)
    assert G.clean(["ACDEFGHIKLMNPQRSTVWYUXBZ"], 2) == (2, ["ACDEFGHIKLMNPQRSTVWYXX"])
    assert G.clean(["acgu-acgtnx"], 0) == (1, ["ACGTACGTN"])          # 9 of ACGTUN over 8 amino-acid letters: DNA
    assert G.clean(["acgu-nRYx"], 0) == (2, ["ACGXNRYX"])             # 5 over 6 (N, R, Y are residues too): protein


def _matrices():
    out = []
    for n in (2, 3, 4, 7, 40):
        rng = np.random.default_rng(100 + n)
        a = rng.random((n, n))
        out.append(("random %d" % n, a + a.T))
        out.append(("all equal %d" % n, np.full((n, n), 0.25)))
        out.append(("all zero %d" % n, np.zeros((n, n))))
        # planted exact ties: few distinct values, dyadic so that the averages tie exactly as well
        t = rng.integers(1, 4, (n, n)).astype(np.float64) / 8
        out.append(("ties %d" % n, np.triu(t, 1) + np.triu(t, 1).T))
        z = rng.integers(0, 3, (n, n)).astype(np.float64) / 4
        out.append(("zeros and ties %d" % n, np.triu(z, 1) + np.triu(z, 1).T))
    return out


@pytest.mark.parametrize("case", _matrices(), ids=lambda c: c[0])
def test_upgma_equals_the_reading_exactly(case):
    _, dist = case
    n = len(dist)
    names = ["t%d" % i for i in range(n)]
    newick = host.guide_upgma(names, dist)
    assert newick.endswith(";")
    # topology, child order and every branch length as a double: the arithmetic is +, *, / in a fixed order
    assert synth.parse_newick(newick) == G.upgma_tree(names, dist)


def test_upgma_tie_rule_by_hand():
    # d(0,1) = d(2,3) = 1: (0,1) first (lowest first id), then (2,3), then the two clusters
    d = np.full((4, 4), 3.0)
    d[0, 1] = d[1, 0] = d[2, 3] = d[3, 2] = 1.0
    assert host.guide_upgma(list("abcd"), d) == "((a:0.5,b:0.5):1,(c:0.5,d:0.5):1);"
    # the new cluster (id 3) ties with leaf 2 against nothing else; the left child is the lower id
    d = np.array([[0, 2, 2], [2, 0, 2], [2, 2, 0]], np.float64)
    assert host.guide_upgma(list("abc"), d) == "(c:1,(a:1,b:1):0);"


def test_upgma_is_not_cubic():
    n = 2048
    rng = np.random.default_rng(5)
    pts = rng.random((n, 3))
    dist = np.sqrt(((pts[:, None, :] - pts[None, :, :]) ** 2).sum(axis=2))
    newick = host.guide_upgma(["s%d" % i for i in range(n)], dist)
    assert newick.count(",") == n - 1 and len(G.clades(synth.parse_newick(newick))) == n - 1


def test_distance_of_equals_the_reading():
    worst = 0.0
    for t in (1, 2, 3):
        for k in (1, 2, 3, 8, 12) + ((17, 31) if t != 2 else ()):
            for m in (0, 1, 2, 7, 100, 99991, 2 ** 31 - 1):
                for S in sorted({0, 1, m // 1000, m // 3, m // 2, m - 1, m}):
                    if S < 0 or S > m:
                        continue
                    want = G.distance_of(S, m, k, t)
                    got = host.guide_distance_of(S, m, k, t)
                    if want == 0.0:
                        assert got == 0.0
                    else:
                        worst = max(worst, abs(got - want) / want)
    assert worst <= 1e-12
    # S = m, S = 0, m = 0 and both clamps
    assert host.guide_distance_of(50, 50, 8, 1) == 0.0
    for S, m in ((0, 50), (0, 0)):
        assert host.guide_distance_of(S, m, 8, 1) == pytest.approx(-0.75 * math.log(1 - 0.7 / 0.75), rel=1e-12)
        assert host.guide_distance_of(S, m, 3, 2) == pytest.approx(-math.log(1 - 0.85 - 0.2 * 0.85 ** 2), rel=1e-12)
    assert host.guide_distance_of(1, 10 ** 6, 2, 1) == host.guide_distance_of(0, 5, 2, 1)       # p = 0.999 -> 0.7
    for bad in ((5, 4, 8, 1), (-1, 4, 8, 1), (1, 4, 0, 1), (1, 4, 32, 1), (1, 4, 13, 2), (1, 4, 8, 0), (1, 4, 8, 4)):
        assert math.isnan(host.guide_distance_of(*bad))


def test_kmer_length_at_clamps_and_switch_points():
    assert host.guide_kmer_length(1, 0) == 8 and host.guide_kmer_length(3, 100) == 8 and host.guide_kmer_length(2, 0) == 3
    assert host.guide_kmer_length(1, 2 ** 62) == 31 and host.guide_kmer_length(2, 2 ** 62) == 12
    for t, A, lo, hi in ((1, 4, 8, 31), (3, 4, 8, 31), (2, 20, 3, 12)):
        for k in range(lo, hi):
            if A ** k % 16:
                continue
            L = A ** k // 16                                        # A^k = 16 L exactly
            assert host.guide_kmer_length(t, L) == k
            assert host.guide_kmer_length(t, L - 1) == max(lo, k if A ** (k - 1) < 16 * (L - 1) else k - 1)
            assert host.guide_kmer_length(t, L + 1) == k + 1
        for L in (1, 17, 4095, 4096, 4097, 100000, 10 ** 9, 10 ** 15):
            assert host.guide_kmer_length(t, L) == G.default_k(t, L)
    # protein by hand: 20^3 = 16 * 500, 20^4 = 16 * 10000
    assert host.guide_kmer_length(2, 500) == 3 and host.guide_kmer_length(2, 501) == 4
    assert host.guide_kmer_length(2, 10000) == 4 and host.guide_kmer_length(2, 10001) == 5
    for bad in ((0, 10), (4, 10), (1, -1)):
        assert _code(host.guide_kmer_length, *bad) == abi.PAGAN_E_ARG


def _code(fn, *args, **kw):
    from pagan2_msa_amd import PaganError
    with pytest.raises(PaganError) as e:
        fn(*args, **kw)
    return e.value.code


def test_refusals():
    d = np.ones((2, 2))
    for bad in ("a(b", "a:b", "a b", "a,b", "a;b", "a)b", "a\tb", ""):
        assert _code(host.guide_upgma, ["x", bad], d) == abi.PAGAN_E_ARG
        assert _code(host.guide_tree, ["x", bad], ["ACGT", "ACGT"]) == abi.PAGAN_E_ARG
    seqs = ["ACGTACGTACGTACGT", "ACGTACGTACGAACGT"]
    assert _code(host.guide_distances, seqs, 1, 32) == abi.PAGAN_E_ARG
    assert _code(host.guide_distances, seqs, 3, 32) == abi.PAGAN_E_ARG
    assert _code(host.guide_distances, ["ARNDCQEGHILKMFPSTWYV"] * 2, 2, 13) == abi.PAGAN_E_ARG
    assert _code(host.guide_distances, ["ARNDCQEGHILKMFPSTWYV"] * 2, 0, 13) == abi.PAGAN_E_ARG     # guessed protein
    assert _code(host.guide_distances, seqs, 1, -1) == abi.PAGAN_E_ARG
    assert _code(host.guide_distances, seqs, 4, 8) == abi.PAGAN_E_ARG
    assert _code(host.guide_distances, seqs[:1], 1, 8) == abi.PAGAN_E_ARG                          # n < 2
    assert _code(host.guide_distances, [], 1, 8) == abi.PAGAN_E_ARG
    assert _code(host.guide_tree, ["x"], seqs[:1]) == abi.PAGAN_E_ARG
    assert _code(host.guide_upgma, ["x"], np.zeros((1, 1))) == abi.PAGAN_E_ARG
    assert _code(host.guide_upgma, ["x", "y"], np.array([[0, -1.0], [-1.0, 0]])) == abi.PAGAN_E_ARG
    assert _code(host.guide_upgma, ["x", "y"], np.array([[0, np.nan], [np.nan, 0]])) == abi.PAGAN_E_ARG
    assert _code(host.guide_predict_bytes, 1, 100) == abi.PAGAN_E_ARG
    assert _code(host.guide_predict_bytes, host.GUIDE_MAX_SEQS + 1, 100) == abi.PAGAN_E_ARG
    # the limit itself is taken (2^31 - 32,768 pairs, four bytes each); one sequence more is refused by every entry,
    # before the sequences are looked at
    assert host.guide_predict_bytes(host.GUIDE_MAX_SEQS, 100) >= 4 * (host.GUIDE_MAX_SEQS * (host.GUIDE_MAX_SEQS - 1) // 2)
    too_many = ["A"] * (host.GUIDE_MAX_SEQS + 1)
    assert _code(host.guide_distances, too_many, 1, 8) == abi.PAGAN_E_ARG
    assert _code(host.guide_tree, too_many, too_many) == abi.PAGAN_E_ARG
    assert _code(host.guide_predict_bytes, 2, 2 ** 31) == abi.PAGAN_E_ARG


def test_predict_bytes_grows_with_the_input():
    a, b, c = host.guide_predict_bytes(2, 1000), host.guide_predict_bytes(2, 100000), host.guide_predict_bytes(2000, 100000)
    assert 0 < a < b < c
    assert b >= 100000 * (1 + 8 + 8 + 8)                 # letters, keys, sorted keys, the sort's second buffer
    assert c - b >= 4 * (2000 * 1999 // 2 - 1)           # a sum per pair


def test_new_symbols_are_exported(pg):
    lib = pg.lib()
    new = ["pagan_guide_distances", "pagan_guide_tree", "pagan_guide_kmer_length", "pagan_guide_distance_of", "pagan_guide_upgma",
           "pagan_guide_predict_bytes"]
    for sym in new:
        assert sym in host.HOST_EXPORTED and getattr(lib, sym) is not None
    assert C.sizeof(host.CGuideInfo) == 4 * 4 + 4 * 8 + 5 * 8


def test_without_a_device_the_device_entries_say_so(pg):
    names, seqs, newick = synth.evolve_balanced(4, 200, seed=3)
    if pg.device_count() > 0:                            # (on a GPU machine: the same calls work)
        assert host.Msa(names, seqs).newick == host.guide_tree(names, seqs)
        return
    assert _code(host.guide_distances, seqs) == abi.PAGAN_E_NODEVICE
    assert _code(host.guide_tree, names, seqs) == abi.PAGAN_E_NODEVICE
    assert _code(host.Msa, names, seqs) == abi.PAGAN_E_NODEVICE
    assert _code(host.Msa, names, seqs, None, data_type=1) == abi.PAGAN_E_NODEVICE
    assert _code(host.guide_distances, ["", ""], 1, 8) == abi.PAGAN_E_NODEVICE     # nothing to count is still no host path
    msa = host.Msa(names, seqs, newick)                  # with a tree: as before
    assert msa.newick == newick and msa.n_internal == 3
