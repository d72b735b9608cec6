"""Guide tree from the sequences, on the device: the k-mers every pair shares (pgd_pairs and the stages before it,
csrc/dp_guide.hip) against the Python reading (tests/pycheck_guide.py) exactly as integers, the distances to 1e-12 relative, the
tree against guide_upgma of the returned matrix exactly -- on the smallest shapes that can still go wrong -- and the tree in
the walk."""
import numpy as np
import pytest

from pagan2_msa_amd import host, synth

import pycheck_guide as G

pytestmark = pytest.mark.gpu

CHUNK = host.GUIDE_PAIR_CHUNK


def check(seqs, data_type=0, k=0, reading=None):
    """One device call against the reading; returns (shared, kmers, dist, info)."""
    shared, kmers, dist, info = host.guide_distances(seqs, data_type, k)
    s0, m0, d0, k0, t0 = reading if reading is not None else G.distances_unique(seqs, data_type, k)
    assert (info["k"], info["data_type"]) == (k0, t0)
    assert info["pair_chunk"] == CHUNK and info["pairs"] == len(seqs) * (len(seqs) - 1) // 2
    assert np.array_equal(kmers, m0)
    assert np.array_equal(shared, s0)
    assert np.array_equal(dist == 0, d0 == 0)
    nz = d0 != 0
    assert np.all(np.abs(dist[nz] - d0[nz]) <= 1e-12 * d0[nz])
    assert 0 <= info["device_bytes"] <= host.guide_predict_bytes(len(seqs), info["positions"])
    return shared, kmers, dist, info


def rand_dna(rng, n):
    return "".join("ACGT"[c] for c in rng.integers(0, 4, n))


def mutate(rng, s, every, letters="ACGT"):
    out = list(s)
    for i in range(int(rng.integers(0, every)), len(out), every):
        out[i] = letters[(letters.index(out[i]) + 1) % len(letters)]
    return "".join(out)


# ---- degenerate inputs -------------------------------------------------------------------------------------------

def test_two_and_three_sequences():
    rng = np.random.default_rng(1)
    a = rand_dna(rng, 80)
    b = mutate(rng, a, 9)
    for seqs in ([a, b], [a, b, a[10:60]]):
        for fn in (G.distances_literal, G.distances_unique):
            check(seqs, 1, 8, reading=fn(seqs, 1, 8))


def test_short_exact_empty_and_identical():
    rng = np.random.default_rng(2)
    a = rand_dna(rng, 50)
    seqs = [a, a[:7], a[:8], "", a, "A" * 100, "A" * 37]
    shared, kmers, dist, _ = check(seqs, 1, 8, reading=G.distances_literal(seqs, 1, 8))
    assert list(kmers) == [43, 0, 1, 0, 43, 93, 30]
    assert shared[0, 4] == 50 - 8 + 1 and dist[0, 4] == 0.0                 # identical
    assert shared[5, 6] == 37 - 8 + 1 and dist[5, 6] == 0.0                 # one code, counts 93 and 30
    assert shared[0, 2] == 1 and shared[0, 1] == 0 and shared[1, 3] == 0
    assert dist[1, 3] == dist[0, 3] == host.guide_distance_of(0, 0, 8, 1)   # nothing to share: the clamp


def test_the_largest_codes_are_not_the_sentinel():
    seqs = ["T" * 40, "T" * 35, "G" + "T" * 33]
    shared, kmers, _, _ = check(seqs, 1, 31, reading=G.distances_literal(seqs, 1, 31))
    assert list(kmers) == [10, 5, 4] and shared[0, 1] == 5 and shared[0, 2] == 3
    prot = ["V" * 20, "V" * 14, "A" + "V" * 15]
    shared, kmers, _, _ = check(prot, 2, 12, reading=G.distances_literal(prot, 2, 12))
    assert list(kmers) == [9, 3, 5] and shared[0, 1] == 3 and shared[0, 2] == 4


def test_letters_outside_the_core_and_cleaning():
    dna = ["ACGTNACGTACGTRACGTAC", "acgu-acgu\nACGUAC\r", "ACGTYYACGTAC", "NNNNNNNN", "AC-GT-ACGTACGT"]
    check(dna, 1, 4, reading=G.distances_literal(dna, 1, 4))
    check(dna, 0, 4, reading=G.distances_literal(dna, 0, 4))
    prot = ["ARNDXCQEGHILKMF", "arndcqeUghilkmf", "ARNDCQEGHILKBZJO", "XXXXXX", "WYV-WYV"]
    check(prot, 2, 3, reading=G.distances_literal(prot, 2, 3))
    check(prot, 0, 3, reading=G.distances_literal(prot, 0, 3))


def test_codon_input_is_dna_over_its_nucleotides():
    rng = np.random.default_rng(3)
    a = rand_dna(rng, 90)
    seqs = [a, mutate(rng, a, 7), mutate(rng, a, 5) + "NNN"]
    as_codon = check(seqs, 3, 6, reading=G.distances_literal(seqs, 3, 6))
    as_dna = host.guide_distances(seqs, 1, 6)
    for x, y in zip(as_codon[:3], as_dna[:3]):
        assert np.array_equal(x, y)
    assert as_codon[3]["data_type"] == 3 and as_dna[3]["data_type"] == 1


@pytest.mark.parametrize("data_type,k", [(1, 1), (1, 8), (1, 31), (2, 1), (2, 3), (2, 12)])
def test_k(data_type, k):
    alphabet = G.PROTEIN if data_type == 2 else "ACGT"
    _, seqs, _ = synth.evolve_balanced(4, 150, sub=0.01, indel_start=0.002, seed=10 + k, alphabet=alphabet)
    seqs = seqs + [seqs[0][:k], seqs[1][:max(k - 1, 0)]]
    shared, _, _, _ = check(seqs, data_type, k, reading=G.distances_literal(seqs, data_type, k))
    assert shared[0, 1] > 0


# ---- list lengths around the kernels' boundaries --------------------------------------------------------------------

def _all_unique_base(length, k):
    for seed in range(100):
        s = rand_dna(np.random.default_rng(1000 + seed), length)
        if len({s[i:i + k] for i in range(length - k + 1)}) == length - k + 1:
            return s
    raise AssertionError("no base sequence with all windows different")


def _boundary_lists(waves, k):
    sizes = sorted({1, CHUNK - 1, CHUNK, CHUNK + 1, 255, 256, 257, waves * CHUNK - 1, waves * CHUNK, waves * CHUNK + 1})
    base = _all_unique_base(max(sizes) + 200 + k, k)
    rng = np.random.default_rng(4)
    seqs = [base[:u + k - 1] for u in sizes]                      # u entries each, a prefix of the next
    seqs += [base[100:100 + u + k - 1] for u in (CHUNK, 257)]     # windows inside the longer lists
    seqs += [mutate(rng, base, 40), base[::-1]]                   # a long list that shares runs, one that shares next to nothing
    return sizes, seqs


def test_list_lengths_around_a_chunk_and_around_a_workgroup():
    k = 12
    # the waves a pair's workgroup has depend on the number of pairs alone: ask with as many sequences as the case will have
    waves = 16
    for _ in range(2):
        sizes, seqs = _boundary_lists(waves, k)
        waves = host.guide_distances(["A" * k] * len(seqs), 1, k)[3]["waves_per_pair"]
    sizes, seqs = _boundary_lists(waves, k)
    for order in (seqs, seqs[::-1]):                              # shorter first, longer first
        shared, kmers, _, info = check(order, 1, k)
        assert info["waves_per_pair"] == waves
        assert info["entries"] == sum(len(set(s[i:i + k] for i in range(len(s) - k + 1))) for s in order)
    assert sorted(kmers[-len(sizes):]) == sizes


def test_one_wave_a_pair_over_many_chunks():
    """With more than 4,096 pairs a pair has one wave, which walks a list of several chunks alone, every chunk's gallop going on
    from where the last chunk's window began: the shape of 512 x 10 kb, at the smallest size that takes it."""
    k = 12
    base = _all_unique_base(700 + k, k)
    rng = np.random.default_rng(6)
    sizes = [1, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK - 1, 2 * CHUNK, 2 * CHUNK + 1, 255, 256, 257, 400, 10 * CHUNK]
    seqs = []
    for i in range(92):
        u = sizes[i % len(sizes)]
        start = int(rng.integers(0, 700 - u)) if i % 3 else 0           # windows of one base: long shared stretches, shifted
        s = base[start:start + u + k - 1]
        seqs.append(mutate(rng, s, 30) if i % 4 == 3 else s)
    shared, kmers, _, info = check(seqs, 1, k)
    assert info["pairs"] == 92 * 91 // 2 == 4186 and info["waves_per_pair"] == 1
    assert max(kmers) == 10 * CHUNK and int(shared[np.triu_indices(92, 1)].max()) >= 400


def test_repeated_codes_with_counts():
    rng = np.random.default_rng(5)
    unit = rand_dna(rng, 70)
    seqs = [unit * 5, unit * 3 + rand_dna(rng, 50), unit[::-1] + unit, "AC" * 200, "ACG" * 100]
    shared, _, _, _ = check(seqs, 1, 8, reading=G.distances_literal(seqs, 1, 8))
    assert shared[0, 1] > 3 * 60


# ---- pair indexing ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [64, 65, 130])
def test_pair_indexing(n):
    rng = np.random.default_rng(n)
    root = rand_dna(rng, 40)
    seqs = [mutate(rng, root, int(rng.integers(3, 12))) for _ in range(n)]
    shared, _, _, _ = check(seqs, 1, 5)
    assert len({int(v) for v in shared[np.triu_indices(n, 1)]}) > 5              # (the pairs do differ)


def test_a_million_pairs_against_the_dense_reading():
    n, k = 1500, 4
    rng = np.random.default_rng(7)
    root = rand_dna(rng, 20)
    seqs = [mutate(rng, root, int(rng.integers(2, 9)))[:int(rng.integers(12, 21))] for _ in range(n)]
    want_shared, want_kmers = G.shared_dense(seqs, 1, k)
    shared, kmers, dist, info = host.guide_distances(seqs, 1, k)
    assert info["pairs"] == n * (n - 1) // 2 == 1124250
    assert np.array_equal(kmers, want_kmers)
    assert np.array_equal(shared, want_shared)
    x, y = 1499, 3
    assert dist[x, y] == dist[y, x] == host.guide_distance_of(shared[x, y], min(kmers[x], kmers[y]), k, 1)


# ---- size ------------------------------------------------------------------------------------------------------------

def test_one_long_pair_at_the_default_k():
    _, seqs, _ = synth.evolve_balanced(2, 20000, branch=0.05, sub=0.02, indel_start=0.002, seed=11)
    shared, kmers, dist, info = check(seqs)
    assert info["k"] == G.default_k(1, max(len(s) for s in seqs)) == 10
    assert 0 < shared[0, 1] < min(kmers) and 0 < dist[0, 1] < 0.2


def test_64_by_1000():
    _, seqs, _ = synth.evolve_balanced(64, 1000, branch=0.02, sub=0.01, indel_start=0.001, seed=12)
    check(seqs)


def test_protein_8_by_300():
    _, seqs, _ = synth.evolve_balanced(8, 300, sub=0.03, indel_start=0.003, seed=13, alphabet=G.PROTEIN)
    _, _, _, info = check(seqs)
    assert info["data_type"] == 2 and info["k"] == 3


def test_the_same_call_twice_gives_the_same_bytes():
    _, seqs, _ = synth.evolve_balanced(16, 700, sub=0.03, indel_start=0.003, seed=14)
    names = ["n%d" % i for i in range(16)]
    a, b = host.guide_distances(seqs), host.guide_distances(seqs)
    for u, v in zip(a[:3], b[:3]):
        assert u.tobytes() == v.tobytes()
    assert host.guide_tree(names, seqs) == host.guide_tree(names, seqs)


# ---- the tree is the right tree --------------------------------------------------------------------------------------

RIGHT_TREE = [("8 x 2000", dict(n_leaves=8, length=2000, branch=0.05, sub=0.02, indel_start=0.002)),
              ("8 x 2000, twice the change", dict(n_leaves=8, length=2000, branch=0.05, sub=0.04, indel_start=0.004)),
              ("16 x 3000", dict(n_leaves=16, length=3000, branch=0.05, sub=0.008, indel_start=0.0008)),
              ("8 x 400 protein", dict(n_leaves=8, length=400, branch=0.05, sub=0.03, alphabet=G.PROTEIN))]


@pytest.mark.parametrize("case", RIGHT_TREE, ids=lambda c: c[0])
@pytest.mark.parametrize("seed", range(5))
def test_the_balanced_tree_is_recovered(case, seed):
    names, seqs, truth = synth.evolve_balanced(seed=seed, **case[1])
    newick, info = host.guide_tree(names, seqs, with_info=True)
    _, _, dist, _ = host.guide_distances(seqs)
    assert newick == host.guide_upgma(names, dist)                               # the tree of the returned matrix, exactly
    assert G.clades(synth.parse_newick(newick)) == G.clades(synth.parse_newick(truth))
    assert info["upgma_ms"] >= 0 and info["k"] == G.default_k(2 if "alphabet" in case[1] else 1, max(len(s) for s in seqs))


# ---- in the walk -----------------------------------------------------------------------------------------------------

def _newick_of(tree):
    """A parse_newick tree written out again by other code than the library's: same topology, child order and lengths."""
    def w(t, top):
        tail = "" if top else ":" + repr(t[-1])
        if t[0] == "leaf":
            return t[1] + tail
        return "(" + w(t[1], False) + "," + w(t[2], False) + ")" + tail
    return w(tree, True) + ";"


def test_the_walk_aligns_from_sequences_alone():
    names, seqs, truth = synth.evolve_balanced(8, 600, branch=0.05, sub=0.02, indel_start=0.002, seed=0)
    msa = host.Msa(names, seqs).align()
    assert msa.newick == host.guide_tree(names, seqs)
    rows = msa.alignment()
    assert [r.replace("-", "") for r in rows] == seqs
    assert host.Msa(names, seqs, msa.newick).align().alignment() == rows
    # the balanced data: a tree of the same topology with the guide tree's lengths, written by the test
    tree = synth.parse_newick(msa.newick)
    assert G.clades(tree) == G.clades(synth.parse_newick(truth))
    again = _newick_of(tree)
    assert synth.parse_newick(again) == tree
    assert host.Msa(names, seqs, again).align().alignment() == rows
    # the walk's data_type is the guide tree's
    assert host.Msa(names, seqs, data_type=1).newick == host.guide_tree(names, seqs, data_type=1)
