"""Ancestral states in the tree walk (pagan_msa_ancestral and its readers) against the pruning reading of
tests/pycheck_anc.py over the walk's own leaf rows, its tree in the walk's ids and the branch lengths it aligned under: the
corrected, truncated ones (<= 0 becomes 0.001, anything above the float 0.2 is cut to it), restated here.  The tolerance and the tie
condition are tests/test_anc_gpu.py's."""
import numpy as np
import pytest

from pagan2_msa_amd import abi, host, synth

import pycheck_anc as A

pytestmark = pytest.mark.gpu


def balanced_newick(names, lengths):
    """A balanced tree over the names in order, the branch lengths taken from `lengths` one after the other."""
    it = iter(lengths)
    level = ["%s:%g" % (name, next(it)) for name in names]
    while len(level) > 2:
        level = ["(%s,%s):%g" % (level[k], level[k + 1], next(it)) for k in range(0, len(level), 2)]
    return "(%s,%s);" % tuple(level)


def walk_tree(names, newick):
    """(left, right, branch) in the walk's ids -- leaves in input order, internal nodes in the order their brackets close -- with
    the branch lengths corrected as the walk corrects them."""
    n = len(names)
    left, right, branch = [], [], [0.0] * (2 * n - 1)

    def corrected(d):
        return 0.001 if d <= 0 else min(d, float(np.float32(0.2)))     # (truncate_branches is a float option)

    def visit(t):
        if t[0] == "leaf":
            v = names.index(t[1])
        else:
            a, b = visit(t[1]), visit(t[2])
            v = n + len(left)
            left.append(a)
            right.append(b)
        branch[v] = corrected(t[-1])
        return v
    assert visit(synth.parse_newick(newick)) == 2 * n - 2
    return left, right, branch


def base_frequencies(seqs):
    """The walk's empirical base frequencies: float counts of A, C, G, T over all sequences, each over their float sum."""
    counts = [np.float32(sum(s.count(c) for s in seqs)) for c in "ACGT"]
    total = counts[0] + counts[1] + counts[2] + counts[3]
    return [c / total for c in counts]


def dna_walk():
    names, seqs, _ = synth.evolve_balanced(8, 300, branch=0.06, sub=0.05, indel_start=0.01, mean_len=3, seed=21)
    lengths = [0.03, 0.08, 0.05, 0.11, 0.02, 0.3, 0.07, 0.0, 0.04, 0.09, 0.06, 0.13, 0.05, 0.1]      # 0.3 is cut to 0.2, 0 becomes 0.001
    return names, seqs, balanced_newick(names, lengths), {"use_anchors": 0}, 1


def codon_walk():
    names, proteins, _ = synth.evolve_balanced(4, 70, branch=0.08, sub=0.06, indel_start=0.02, mean_len=2, seed=22, alphabet=A.PROTEIN)
    seqs = ["".join(A.CODONS[3 * A.PROTEIN.index(c) + 1] for c in p) for p in proteins]            # whole codons: indels keep the frame
    return names, seqs, balanced_newick(names, [0.05, 0.12, 0.07, 0.15, 0.04, 0.09]), {"use_anchors": 0, "data_type": 3}, 3


_walks = {}


def walked(kind):
    """The walk, its ancestral states and their reading, made once a kind."""
    if kind not in _walks:
        _walks[kind] = make_walk(kind)
    return _walks[kind]


@pytest.fixture(scope="module", params=["dna", "codon"])
def walk(request):
    return walked(request.param)


def make_walk(kind):
    names, seqs, newick, opts, data_type = dna_walk() if kind == "dna" else codon_walk()
    msa = host.Msa(names, seqs, newick, **opts).align()
    before = msa.alignment_all()
    anc = msa.ancestral()
    left, right, branch = walk_tree(names, newick)
    n = len(names)
    for k in range(n - 1):
        info = msa.node_info(k)
        assert (info.left, info.right) == (left[k], right[k])
        assert abs(info.dist - (branch[left[k]] + branch[right[k]])) < 1e-12
    bf = base_frequencies(seqs) if data_type == 1 else None
    reading = A.pruning(left, right, branch, before[:n], data_type, bf)
    tol = A.tolerance(left, right, A.STATES[data_type])
    return {"msa": msa, "anc": anc, "before": before, "reading": reading, "tol": tol, "data_type": data_type, "n": n,
            "width": 3 if data_type == 3 else 1}


def test_rows(walk):
    msa, anc, before, n, w = walk["msa"], walk["anc"], walk["before"], walk["n"], walk["width"]
    L = len(before[0]) // w
    assert anc.info["columns"] == L and anc.info["data_type"] == walk["data_type"] and anc.best.shape == (n - 1, L)
    assert msa.alignment_all() == before                               # alignment_row returns the same bytes before and after
    for leaf in range(n):
        assert anc.row(leaf) == before[leaf]
    left_out = shown = 0
    for k in range(n - 1):
        row, old = anc.row(n + k), before[n + k]
        assert len(row) == len(old)
        for col in range(L):
            got, was = row[col * w:(col + 1) * w], old[col * w:(col + 1) * w]
            assert (got == "-" * w) == (was == "-" * w), (k, col)      # gaps exactly where alignment_row has them
            if was == "-" * w:
                continue
            shown += 1
            want = walk["reading"]["post"][k][col]
            assert got == A.state_text(int(anc.best[k, col]), walk["data_type"])
            if A.decided(want, walk["tol"]):
                assert got == A.state_text(A.best_of(want)[0], walk["data_type"]), (k, col)
            else:
                left_out += 1
    assert shown > 0.5 * (n - 1) * L and left_out <= 0.01 * shown
    if walk["data_type"] == 1:                                         # (a parsimony placeholder, an IUPAC set, became a base)
        assert any(anc.row(n + k) != before[n + k] for k in range(n - 1))


def test_support(walk):
    anc, before, n, w, tol = walk["anc"], walk["before"], walk["n"], walk["width"], walk["tol"]
    L = len(before[0]) // w
    for k in range(n - 1):
        sup = anc.support(n + k)
        assert sup.dtype == np.float32 and sup.shape == (L,)
        for col in range(L):
            if before[n + k][col * w] == "-":
                assert sup[col] == -1.0
                continue
            want = walk["reading"]["post"][k][col]
            assert sup[col] == anc.best_p[k, col]
            p = float(want[int(anc.best[k, col])])                     # the posterior of the shown state
            assert abs(float(sup[col]) - p) <= 2 * tol + 2.0 ** -24 * p
    with pytest.raises(host_error()) as e:
        anc.support(0)                                                 # a leaf has no support row
    assert e.value.code == abi.PAGAN_E_ARG


def test_loglik(walk):
    anc, reading, tol = walk["anc"], walk["reading"], walk["tol"]
    total = 0.0
    for col, x in enumerate(anc.col_loglik):
        ll = float(reading["lik"][col].ln())
        assert abs(float(x) - ll) <= tol + 2.0 ** -52 * abs(ll)
        total += float(x)
    assert anc.loglik == total and total < 0


def test_fasta(walk, tmp_path):
    msa, anc, n = walk["msa"], walk["anc"], walk["n"]
    msa.write_fasta(tmp_path / "nodes.fas", include_internal=True)
    anc.write_fasta(tmp_path / "anc.fas")

    def entries(path):
        out = []
        for line in open(path).read().split("\n"):
            if line.startswith(">"):
                out.append([line[1:], ""])
            elif line:
                out[-1][1] += line
        return out
    a, b = entries(tmp_path / "nodes.fas"), entries(tmp_path / "anc.fas")
    assert [e[0] for e in a] == [e[0] for e in b] and len(b) == 2 * n - 1             # write_fasta_nodes' names and order
    rows = {("#%d#" % (k + 1)): anc.row(n + k) for k in range(n - 1)}
    rows.update({name: anc.row(k) for k, name in enumerate(msa.names)})
    assert all(rows[name] == row for name, row in b)
    anc.write_fasta(tmp_path / "anc7.fas", chars_by_line=7)
    assert entries(tmp_path / "anc7.fas") == b and max(len(x) for x in open(tmp_path / "anc7.fas").read().split("\n")) <= 7


def test_chunks_in_the_walk_change_no_byte(monkeypatch):
    """The DNA walk once more, its ancestral states in chunks of 64 columns: rows, best, best_p and the log likelihoods are the
    bytes of the walk that ran in one chunk."""
    one = walked("dna")
    assert one["anc"].info["chunks"] == 1
    names, seqs, newick, opts, _ = dna_walk()
    msa = host.Msa(names, seqs, newick, **opts).align()
    assert msa.alignment_all() == one["before"]
    monkeypatch.setenv("PAGAN_ANC_CHUNK_COLS", "64")
    anc = msa.ancestral()
    assert anc.info["chunk_cols"] == 64 and anc.info["chunks"] == (anc.info["columns"] + 63) // 64 > 1
    assert [anc.row(v) for v in range(2 * one["n"] - 1)] == [one["anc"].row(v) for v in range(2 * one["n"] - 1)]
    for a, b in ((anc.best, one["anc"].best), (anc.best_p, one["anc"].best_p), (anc.col_loglik, one["anc"].col_loglik)):
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
    assert np.float64(anc.loglik).tobytes() == np.float64(one["anc"].loglik).tobytes()


def host_error():
    from pagan2_msa_amd import PaganError
    return PaganError


def test_before_aligning_it_is_refused():
    names, seqs, newick, opts, _ = dna_walk()
    msa = host.Msa(names, seqs, newick, **opts)
    with pytest.raises(host_error()) as e:
        msa.ancestral()
    assert e.value.code == abi.PAGAN_E_ARG
    assert msa._L.pagan_msa_ancestral(msa._h, 0, None, None, None) == abi.PAGAN_E_ARG
