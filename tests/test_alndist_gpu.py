"""Guide tree from the alignment, on the device: the row pair counts of pad_pack / pad_pairs / pad_fold (csrc/dp_alndist.hip)
against the Python reading (tests/pycheck_alndist.py) exactly as integers, the distances to 1e-12 relative (the tolerance
tests/test_guide_gpu.py uses for the same formula), the tree against guide_upgma of the returned matrix exactly -- on the
smallest shapes that can still go wrong: the edges of a 64-column word, of the split granule and of a 64-row tile, every bit
plane on its own, every kind of non-letter, the split path and the path without it -- and the tree in the walk."""
import math

import numpy as np
import pytest

from pagan2_msa_amd import host, synth

import pycheck_alndist as A
import pycheck_guide as G

pytestmark = pytest.mark.gpu

SPLIT_COLS = host.ALN_SPLIT_WORDS * 64
DNA_CLAMP = -0.75 * math.log(1.0 - 0.7 / 0.75)
PROTEIN_CLAMP = -math.log(1.0 - 0.85 - 0.2 * 0.85 * 0.85)


def check(rows, data_type=0, literal=False):
    """One device call against the reading; returns (both, match, dist, info)."""
    both, match, dist, info = host.aln_distances(rows, data_type)
    b0, m0, d0, t0 = A.reading(rows, data_type, literal=literal)
    n, L = len(rows), len(rows[0])
    assert info["data_type"] == t0 and info["planes"] == (6 if t0 == 2 else 3) and info["tile"] == host.ALN_TILE
    assert (info["columns"], info["words"], info["pairs"]) == (L, (L + 63) // 64, n * (n - 1) // 2)
    assert info["col_splits"] >= 1
    assert np.array_equal(both, b0)
    assert np.array_equal(match, m0)
    assert np.array_equal(dist == 0, d0 == 0)
    nz = d0 != 0
    assert np.all(np.abs(dist[nz] - d0[nz]) <= 1e-12 * d0[nz])
    assert 0 < info["device_bytes"] <= host.aln_predict_bytes(n, L)
    return both, match, dist, info


def random_rows(n, L, letters, seed, share=0.15, other="-.NX"):
    """n rows of L characters: `letters` uniformly, and 15 % characters that are no letters."""
    rng = np.random.default_rng(seed)
    pool = np.frombuffer((letters + other).encode(), np.uint8)
    p = np.concatenate([np.full(len(letters), (1 - share) / len(letters)), np.full(len(other), share / len(other))])
    raw = rng.choice(pool, (n, L), p=p)
    return [bytes(r).decode() for r in raw]


# ---- edges of the word, the granule and the tile -----------------------------------------------------------------

@pytest.mark.parametrize("L", [0, 1, 63, 64, 65, 127, 128, 129, SPLIT_COLS - 1, SPLIT_COLS, SPLIT_COLS + 1])
def test_word_edges(L):
    for letters, t in (("ACGT", 1), (G.PROTEIN, 2)):
        rows = random_rows(5, L, letters, 100 + L)
        both, _, _, info = check(rows, t)
        assert info["col_splits"] == (2 if L > SPLIT_COLS else 1)         # one tile: a split a granule
        if L >= 63:
            assert both[0, 1] > 0


@pytest.mark.parametrize("n", [2, 3, 63, 64, 65, 130])
def test_tile_edges(n):
    """A diagonal tile alone, one off-diagonal tile, three tile rows, padded rows in the last tile."""
    check(random_rows(n, 150, "ACGT", n), 1)
    check(random_rows(n, 70, G.PROTEIN, 1000 + n), 2)


def test_literal_reading_on_the_device_too():
    check(random_rows(4, 131, "ACGT", 7, other="-.NRYUu"), 1, literal=True)
    check(random_rows(3, 70, G.PROTEIN, 8, other="-.XBZU"), 2, literal=True)


# ---- every plane counts --------------------------------------------------------------------------------------------

def test_every_dna_plane_counts():
    base = "A" * 40 + "C" * 30 + "G" * 30 + "T" * 30                         # 130 columns, three words
    at = {"A": 0, "C": 40, "G": 70, "T": 100}
    for a, b in (("A", "C"), ("A", "G"), ("C", "T"), ("G", "T")):           # codes 0/1, 0/2, 1/3, 2/3: one bit each
        other = base[:at[a]] + b * 7 + base[at[a] + 7:]
        both, match, dist, _ = check([base, other, base], 1)
        assert both[0, 1] == 130 and match[0, 1] == 130 - 7 and match[1, 2] == 123 and match[0, 2] == 130
        assert dist[0, 2] == 0.0 and dist[0, 1] == pytest.approx(-0.75 * math.log(1.0 - (7 / 130) / 0.75), rel=1e-12)


def test_every_protein_plane_counts():
    P = G.PROTEIN
    base = "".join(c * 7 for c in P)                                         # 140 columns: 7 of every residue
    for a, b in ((0, 1), (0, 2), (0, 4), (0, 8), (0, 16), (19, 3)):         # one code bit each (19 = 10011, 3 = 00011)
        other = base[:7 * a] + P[b] * 5 + base[7 * a + 5:]
        both, match, dist, _ = check([base, other], 2)
        assert both[0, 1] == 140 and match[0, 1] == 135
        assert match[0, 0] == match[1, 1] == 140


# ---- non-letters --------------------------------------------------------------------------------------------------

def test_non_letters():
    L = 100
    a = random_rows(1, L, "ACGT", 3, share=0.0)[0]
    rows = [a, "-" * L, a, a.lower(), a.replace("T", "U"), a.replace("T", "u"),
            a[:50] + "-" * 50, "." * 50 + a[50:], a[:20] + "N" * 10 + "R" * 10 + "X" * 10 + ".-" * 5 + a[60:]]
    rows = [r[:33] + "-" + r[34:] for r in rows]                             # an all-gap column
    both, match, dist, _ = check(rows, 1, literal=True)
    letters = L - 1
    assert both[0, 0] == letters and both[1, 1] == 0 and not both[1].any()   # the all-gap row
    assert dist[0, 2] == 0.0 and match[0, 2] == letters                      # identical rows
    assert dist[0, 3] == dist[0, 4] == dist[0, 5] == 0.0 and match[0, 5] == letters    # lower case, U
    assert both[6, 7] == 0 and dist[6, 7] == DNA_CLAMP and dist[0, 1] == DNA_CLAMP      # no shared column: the clamp
    assert both[0, 8] == L - 40 and match[0, 8] == L - 40               # (N, R, X, '.', '-': the all-gap column is among them)
    # protein: U and X are no letters there
    p = random_rows(1, 80, G.PROTEIN, 4, share=0.0)[0]
    prot = [p, p[:40] + "X" * 20 + "U" * 20, "-" * 40 + p[40:], p[:40] + "-" * 40]
    both, match, dist, _ = check(prot, 2, literal=True)
    assert both[0, 1] == 40 and match[0, 1] == 40 and both[2, 3] == 0 and dist[2, 3] == PROTEIN_CLAMP


def test_guessed_type_and_codon_rows():
    dna = random_rows(6, 200, "ACGT", 5)
    prot = random_rows(6, 200, G.PROTEIN, 6)
    for rows, t in ((dna, 1), (prot, 2)):
        b0, m0, d0, i0 = check(rows, 0)
        b1, m1, d1, i1 = check(rows, t)
        assert i0["data_type"] == i1["data_type"] == t
        assert np.array_equal(b0, b1) and np.array_equal(m0, m1) and np.array_equal(d0, d1)
    b3, m3, d3, i3 = check(dna, 3)                                            # a codon alignment is read as DNA
    b1, m1, d1, _ = check(dna, 1)
    assert i3["data_type"] == 3 and i3["planes"] == 3
    assert np.array_equal(b3, b1) and np.array_equal(m3, m1) and np.array_equal(d3, d1)


# ---- the split path and the path without it --------------------------------------------------------------------------

def test_the_split_path():
    L = 5 * SPLIT_COLS + 77                                                  # six granules, the last one partly filled
    for letters, t in (("ACGT", 1), (G.PROTEIN, 2)):
        _, _, _, info = check(random_rows(4, L, letters, 11 + t), t)
        assert info["col_splits"] == 6
    # more granules than splits are taken: a split of several granules, the last split shorter (1,024 splits at most)
    rows = random_rows(2, 1030 * SPLIT_COLS + 1, "ACGT", 13)
    _, _, _, info = check(rows, 1)
    assert 1 < info["col_splits"] <= 1024 and info["words"] == 1030 * host.ALN_SPLIT_WORDS + 1
    # three tiles share the target: 341 splits at most
    _, _, _, info = check(random_rows(70, 4 * SPLIT_COLS, "ACGT", 14), 1)
    assert info["col_splits"] == 4


def test_many_rows_take_no_split():
    """32 tile rows, 528 tiles: every tile is one workgroup over all its words (two granules), rows padded in the last tile."""
    n, L = 1990, SPLIT_COLS + 90
    rows = random_rows(n, L, "ACGT", 15)
    both, match, dist, info = check(rows, 1)
    assert info["col_splits"] == 1 and info["words"] > host.ALN_SPLIT_WORDS
    assert both[0, n - 1] > 0 and match[5, 1234] < both[5, 1234]


def test_repeatability():
    rows = random_rows(70, 3 * SPLIT_COLS + 5, "ACGT", 16)
    names = ["r%d" % i for i in range(len(rows))]
    a, b = host.aln_distances(rows, 1), host.aln_distances(rows, 1)
    for x, y in zip(a[:3], b[:3]):
        assert x.tobytes() == y.tobytes()
    assert a[3]["col_splits"] == b[3]["col_splits"] > 1
    assert host.aln_tree(names, rows, 1) == host.aln_tree(names, rows, 1)


# ---- the tree ------------------------------------------------------------------------------------------------------

def test_aln_tree_is_upgma_of_the_returned_matrix():
    for n, L, letters, t, seed in ((2, 50, "ACGT", 1, 1), (9, 300, "ACGT", 1, 2), (70, 200, G.PROTEIN, 2, 3)):
        rows = random_rows(n, L, letters, seed)
        names = ["r%d" % i for i in range(n)]
        _, _, dist, _ = host.aln_distances(rows, t)
        newick, info = host.aln_tree(names, rows, t, with_info=True)
        assert newick == host.guide_upgma(names, dist)
        assert info["upgma_ms"] >= 0 and info["data_type"] == t and info["pairs"] == n * (n - 1) // 2


def test_the_device_recovers_the_generators_tree():
    names, rows = A.evolve_aligned(16, 600, 0.03, 0.01, 4.0, 0)
    check(rows, 1)
    newick = host.aln_tree(names, rows, 1)
    assert G.clades(synth.parse_newick(newick)) == A.true_clades(16)
    assert synth.parse_newick(newick) == A.tree(names, rows, 1)


# ---- in the walk ---------------------------------------------------------------------------------------------------

def ungapped(rows):
    return [r.replace("-", "") for r in rows]


def walk_checks(names, seqs, data_type):
    plain = host.Msa(names, seqs, data_type=data_type).align()
    rows = plain.alignment()
    tree = plain.alignment_tree()
    assert tree == host.aln_tree(names, rows, data_type)
    assert synth.parse_newick(tree) == A.tree(names, rows, data_type)
    tree2, info = plain.alignment_tree(with_info=True)
    assert tree2 == tree and info["columns"] == len(rows[0]) and info["data_type"] == data_type

    r0 = host.align_refined(names, seqs, rounds=0, data_type=data_type)
    assert r0.alignment() == rows and len(r0.history) == 1 and r0.history[0]["newick"] == plain.newick

    r1 = host.align_refined(names, seqs, rounds=1, data_type=data_type)
    h = r1.history
    assert h[0]["newick"] == plain.newick and h[0]["alignment_length"] == len(rows[0]) and h[0]["changed_clades"] == 0
    assert h[0]["score"] == sum(plain.node_info(k).score for k in range(plain.n_internal))
    assert len(h) in (1, 2) and r1.newick == h[-1]["newick"]
    if len(h) == 2:
        assert h[1]["newick"] == tree and tree != plain.newick
        assert h[1]["changed_clades"] == len(G.clades(synth.parse_newick(tree)) - G.clades(synth.parse_newick(plain.newick)))
        again = host.Msa(names, seqs, tree, data_type=data_type).align()
        assert r1.alignment() == again.alignment() and h[1]["alignment_length"] == len(again.alignment()[0])
    else:
        assert tree == plain.newick and r1.alignment() == rows
    assert ungapped(r1.alignment()) == seqs

    r4 = host.align_refined(names, seqs, rounds=4, data_type=data_type)
    h = r4.history
    assert 1 <= len(h) <= 5 and h[0]["newick"] == plain.newick and ungapped(r4.alignment()) == seqs
    # every walk's tree is the tree of the alignment before it
    prev = plain
    for step in h[1:]:
        assert step["newick"] == prev.alignment_tree() != prev.newick
        prev = host.Msa(names, seqs, step["newick"], data_type=data_type).align()
        assert step["alignment_length"] == len(prev.alignment()[0])
    assert r4.alignment() == prev.alignment()
    if len(h) < 5:                                                           # stopped early: a fixpoint
        assert r4.alignment_tree() == r4.newick


def test_in_the_walk_dna():
    names, seqs, _ = synth.evolve_balanced(8, 600, branch=0.05, sub=0.02, indel_start=0.002, seed=0)
    walk_checks(names, seqs, 1)


def test_in_the_walk_protein():
    names, seqs, _ = synth.evolve_balanced(8, 200, branch=0.05, sub=0.03, indel_start=0.004, seed=1, alphabet=G.PROTEIN)
    walk_checks(names, seqs, 2)
