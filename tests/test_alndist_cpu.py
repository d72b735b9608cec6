"""Guide tree from the alignment, the host side (no GPU): the two Python readings of the row pair counts agree, the reading
alone recovers the tree the rows were made on, the library refuses what the header says it refuses before it asks for a
device, and the pair kernel's code object has no scratch (tests/pycheck_alndist.py; the definition is in
include/pagan_host.h, "guide tree from an alignment")."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

from pagan2_msa_amd import abi, host, synth

import pycheck_alndist as A
import pycheck_guide as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _code(fn, *args, **kw):
    from pagan2_msa_amd import PaganError
    with pytest.raises(PaganError) as e:
        fn(*args, **kw)
    return e.value.code


def random_rows(n, L, letters, seed, other="-.NX", share=0.15):
    """n rows of L characters: `letters` uniformly, and a share of characters that are no letters."""
    rng = np.random.default_rng(seed)
    pool = np.array(list(letters + letters.lower()[:2] + other))
    p = np.concatenate([np.full(len(letters), (1 - share) * 0.9 / len(letters)), np.full(2, (1 - share) * 0.05),
                        np.full(len(other), share / len(other))])
    return ["".join(rng.choice(pool, L, p=p)) for _ in range(n)]


@pytest.mark.parametrize("case", [("dna", "ACGT", 1, "-.NRU"), ("dna guessed", "ACGT", 0, "-.N"), ("codon", "ACGT", 3, "-N"),
                                  ("protein", G.PROTEIN, 2, "-.XBZU"), ("protein guessed", G.PROTEIN, 0, "-X")], ids=lambda c: c[0])
def test_numpy_reading_equals_the_literal_one(case):
    _, letters, data_type, other = case
    for n, L, seed in ((2, 1, 0), (3, 70, 1), (7, 131, 2)):
        rows = random_rows(n, L, letters, seed, other)
        b0, m0, d0, t0 = A.reading(rows, data_type, literal=True)
        b1, m1, d1, t1 = A.reading(rows, data_type)
        assert t0 == t1 and (L < 70 or t0 == (data_type or (2 if letters == G.PROTEIN else 1)))    # (a single residue may guess as DNA)
        assert np.array_equal(b0, b1) and np.array_equal(m0, m1) and np.array_equal(d0, d1)
        assert np.array_equal(b0, b0.T) and np.array_equal(np.diag(b0), np.diag(m0))
        assert np.all(m0 <= b0) and np.all(b0 <= L)
        if L >= 70:                                                    # (the rows do hold letters and non-letters, matches and mismatches)
            assert 0 < m0.sum() < b0.sum() < n * n * L


def test_literal_reading_on_cases_worked_by_hand():
    rows = ["ACGT-ACGT.", "acgu-ACNTA", "TTTTTTTTTT", "----------"]
    b, m, d, t = A.reading(rows, 1, literal=True)
    assert t == 1
    assert b.tolist() == [[8, 7, 8, 0], [7, 8, 8, 0], [8, 8, 10, 0], [0, 0, 0, 0]]
    assert m.tolist() == [[8, 7, 2, 0], [7, 8, 2, 0], [2, 2, 10, 0], [0, 0, 0, 0]]       # U counts as T: column 3 matches
    assert d[0, 1] == 0.0 and d[0, 0] == 0.0
    clamp = -0.75 * math.log(1.0 - 0.7 / 0.75)
    assert d[0, 3] == clamp and d[0, 2] == clamp                                          # both = 0; p = 0.75 > 0.7
    # protein: U and X are no letters, the order of the codes is pycheck_guide.PROTEIN's
    b, m, d, t = A.reading(["ARNDU", "ARNEX", "arnd-"], 2, literal=True)
    assert b.tolist() == [[4, 4, 4], [4, 4, 4], [4, 4, 4]] and m.tolist() == [[4, 3, 4], [3, 4, 3], [4, 3, 4]]
    assert d[0, 1] == -math.log(1.0 - 0.25 - 0.2 * 0.25 * 0.25)
    assert [A.letter_code(c, 2) for c in "ARNDCQEGHILKMFPSTWYV"] == list(range(20))
    assert [A.letter_code(c, 1) for c in "ACGTUacgtu"] == [0, 1, 2, 3, 3, 0, 1, 2, 3, 3]
    assert all(A.letter_code(c, 1) < 0 for c in "-.NRYXB*? ") and all(A.letter_code(c, 2) < 0 for c in "-.XBZUJO*")


# four families x seeds 0..4: all 20 recover the tree (also with pycheck_guide.upgma_tree)
TREE_CASES = [("8x300", 8, 300, 0.04, 0.01, 4.0, "ACGT", 1), ("16x600", 16, 600, 0.03, 0.01, 4.0, "ACGT", 1),
              ("64x1000", 64, 1000, 0.03, 0.005, 4.0, "ACGT", 1), ("protein 8x200", 8, 200, 0.05, 0.01, 3.0, G.PROTEIN, 2)]


@pytest.mark.parametrize("case", TREE_CASES, ids=lambda c: c[0])
def test_the_reading_alone_recovers_the_tree(pg, case):
    _, n, L, sub, gap_start, mean_len, letters, t = case
    for seed in range(5):
        names, rows = A.evolve_aligned(n, L, sub, gap_start, mean_len, seed, letters)
        both, match, dist, rt = A.reading(rows, t)
        assert rt == t and len(rows) == n and all(len(r) == L for r in rows)
        newick = host.guide_upgma(names, dist)
        assert G.clades(synth.parse_newick(newick)) == A.true_clades(n), (case[0], seed)
        assert synth.parse_newick(newick) == G.upgma_tree(names, dist)
        gaps = np.mean([r.count("-") / L for r in rows])
        assert 0.05 < gaps < 0.3 and 0.2 < dist.max() < 0.6, (gaps, dist.max())    # (10-22 % gaps, largest distance 0.25-0.48)


def test_refusals_come_before_any_device_is_asked_for(pg):
    """All PAGAN_E_ARG, with or without a device: without one a call that got as far as the device would say PAGAN_E_NODEVICE."""
    ok = ["ACGT-ACGT", "ACGTAAC-T", "AC-TAACGT"]
    names = ["a", "b", "c"]
    ragged = ["ACGT-ACGT", "ACGTAACT", "AC-TAACGT"]
    assert _code(host.aln_distances, ragged, 1) == abi.PAGAN_E_ARG
    assert _code(host.aln_distances, ragged, 0) == abi.PAGAN_E_ARG
    assert _code(host.aln_tree, names, ragged) == abi.PAGAN_E_ARG
    assert _code(host.aln_distances, ok[:1]) == abi.PAGAN_E_ARG                                    # n = 1
    assert _code(host.aln_distances, []) == abi.PAGAN_E_ARG
    assert _code(host.aln_tree, names[:1], ok[:1]) == abi.PAGAN_E_ARG
    too_many = ["A"] * (host.GUIDE_MAX_SEQS + 1)
    assert _code(host.aln_distances, too_many, 1) == abi.PAGAN_E_ARG
    assert _code(host.aln_tree, too_many, too_many, 1) == abi.PAGAN_E_ARG
    for bad in (-1, 4, 7):
        assert _code(host.aln_distances, ok, bad) == abi.PAGAN_E_ARG
        assert _code(host.aln_tree, names, ok, bad) == abi.PAGAN_E_ARG
    for bad in ("a(b", "a b", ""):
        assert _code(host.aln_tree, ["x", "y", bad], ok) == abi.PAGAN_E_ARG
    L = host._lib()
    assert L.pagan_aln_distances(3, None, 1, None, None, None, None) == abi.PAGAN_E_ARG
    rows = host._c_strings(ok)
    rows[1] = None
    assert L.pagan_aln_distances(3, rows, 1, None, None, None, None) == abi.PAGAN_E_ARG
    # a walk whose rows do not exist yet
    tn, ts, nwk = synth.evolve_balanced(4, 60, seed=3)
    assert _code(host.Msa(tn, ts, nwk).alignment_tree) == abi.PAGAN_E_ARG
    assert L.pagan_msa_alignment_tree(None, None, 0, None) == abi.PAGAN_E_ARG


def test_predict_bytes_grows_with_the_input():
    assert _code(host.aln_predict_bytes, 1, 100) == abi.PAGAN_E_ARG
    assert _code(host.aln_predict_bytes, host.GUIDE_MAX_SEQS + 1, 100) == abi.PAGAN_E_ARG
    assert _code(host.aln_predict_bytes, 2, -1) == abi.PAGAN_E_ARG
    assert _code(host.aln_predict_bytes, 2, 2 ** 31) == abi.PAGAN_E_ARG
    assert host.aln_predict_bytes(2, 0) > 0
    tile = 2 * host.ALN_TILE * host.ALN_TILE * 4
    # the limits themselves are taken: 524,800 tiles of counts; 2^31 - 1 columns of two rows
    T = host.GUIDE_MAX_SEQS // host.ALN_TILE
    assert host.aln_predict_bytes(host.GUIDE_MAX_SEQS, 100) >= (T * (T + 1) // 2) * tile + host.GUIDE_MAX_SEQS * 100
    assert host.aln_predict_bytes(2, 2 ** 31 - 1) >= 2 * (2 ** 31 - 1)
    # monotone in n at every length, across the sizes where the number of tiles and the split change ...
    ns = [2, 3, 63, 64, 65, 128, 129, 640, 1000, 2047, 2048, 2880, 2881, 2900, 4096, 65536]
    Ls = [0, 1, 63, 64, 65, 511, 512, 513, 1024, 1025, 4096, 10000, 150000, 2 ** 20 + 1]
    for L in Ls:
        sizes = [host.aln_predict_bytes(n, L) for n in ns]
        assert all(a <= b for a, b in zip(sizes, sizes[1:])), (L, sizes)
    # ... and in the columns for every n
    for n in ns:
        sizes = [host.aln_predict_bytes(n, L) for L in Ls]
        assert all(a <= b for a, b in zip(sizes, sizes[1:])), (n, sizes)
    # the rows as bytes, six planes of bits, a tile of counts
    assert host.aln_predict_bytes(64, 64 * 8 * 100) >= 64 * 51200 + 6 * 64 * 51200 // 8 + tile


def test_new_symbols_are_exported(pg):
    lib = pg.lib()
    for sym in ("pagan_aln_distances", "pagan_aln_tree", "pagan_aln_predict_bytes", "pagan_msa_alignment_tree"):
        assert sym in host.HOST_EXPORTED and getattr(lib, sym) is not None
    assert C.sizeof(host.CAlnInfo) == 4 * 4 + 4 * 8 + 3 * 8
    with open(os.path.join(ROOT, "include", "pagan_host.h")) as f:
        text = f.read()
    assert "#define PAGAN_ALN_TILE         %d " % host.ALN_TILE in text
    assert "#define PAGAN_ALN_SPLIT_WORDS  %d " % host.ALN_SPLIT_WORDS in text
    for fn in (host.aln_distances, host.aln_tree, host.aln_predict_bytes, host.align_refined, host.Msa.alignment_tree):
        assert callable(fn)


def _oracle_backend(oracle):
    L = oracle.lib()

    def fn(n, jobs, opts, out, user):
        for k in range(n):
            j = jobs[k]
            rc = L.oracle_dp_align(j.left, j.right, j.model, j.band if j.band else None, opts, C.byref(out[k]))
            if rc != 0:
                return rc
        return 0
    return fn


def test_without_a_device_the_device_entries_say_so(pg, oracle):
    names, rows = A.evolve_aligned(4, 100, 0.04, 0.01, 4.0, 0)
    tn, ts, nwk = synth.evolve_balanced(4, 60, branch=0.03, sub=0.03, indel_start=0.01, mean_len=3, seed=12)
    msa = host.Msa(tn, ts, nwk, use_anchors=0)                 # aligned through the test seam: its rows exist without a device
    msa.set_batch_backend(_oracle_backend(oracle))
    msa.align()
    assert [r.replace("-", "") for r in msa.alignment()] == ts
    if pg.device_count() > 0:                                  # (on a GPU machine: the same calls work)
        assert host.aln_tree(names, rows) == host.guide_upgma(names, host.aln_distances(rows)[2])
        assert msa.alignment_tree() == host.aln_tree(tn, msa.alignment())
        assert host.align_refined(tn, ts, rounds=0).history[0]["newick"] == host.guide_tree(tn, ts)
        return
    assert _code(host.aln_distances, rows) == abi.PAGAN_E_NODEVICE
    assert _code(host.aln_distances, ["", ""], 1) == abi.PAGAN_E_NODEVICE          # nothing to count is still no host path
    assert _code(host.aln_tree, names, rows) == abi.PAGAN_E_NODEVICE
    assert _code(msa.alignment_tree) == abi.PAGAN_E_NODEVICE
    assert _code(host.align_refined, tn, ts) == abi.PAGAN_E_NODEVICE
    assert _code(host.align_refined, tn, ts, 1, nwk) == abi.PAGAN_E_NODEVICE


def test_pair_kernel_code_object_has_no_scratch():
    """dp_alndist.hip compiled afresh to gfx950 assembly (no GPU needed): from the kernel metadata, pad_pairs (both alphabets)
    and the fold kernel have no private segment and spill no VGPR -- the 32 accumulators and the planes of a word stay in
    registers."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import check_scratch
    finally:
        sys.path.pop(0)
    funcs, meta = check_scratch.analyse(check_scratch.assemble("dp_alndist.hip"))
    pairs = {k: v for k, v in meta.items() if "pad_pairs" in k and v}
    fold = {k: v for k, v in meta.items() if "pad_fold" in k and v}
    assert len(pairs) == 2 and len(fold) == 1, sorted(meta)
    for k, v in list(pairs.items()) + list(fold.items()):
        assert v["private_segment_fixed_size"] == 0 and v["vgpr_spill_count"] == 0 and v["sgpr_spill_count"] == 0, (k, v)
    assert not [k for k in funcs if "pad_" in k], funcs              # (a function is listed only if it touches scratch)
