"""Branch lengths by maximum likelihood over a finished walk (pagan_msa_fit_branches) and in align_refined: the walk's fit is
anc_fit_branches over its own rows, its tree in the walk's ids and the lengths it aligned under (tests/test_anc_walk_gpu.py
restates those), the Newick it returns reads back to the same tree, align_refined(branch_lengths="ml") is the same steps made by
hand, and without the keyword align_refined is what it was."""
import numpy as np
import pytest

from pagan2_msa_amd import host

import test_anc_walk_gpu as W

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", params=["dna", "codon"])
def fitted_walk(request):
    names, seqs, newick, opts, data_type = W.dna_walk() if request.param == "dna" else W.codon_walk()
    msa = host.Msa(names, seqs, newick, **opts).align()
    before = msa.alignment_all()
    fit = msa.fit_branches()
    return {"names": names, "seqs": seqs, "newick": newick, "data_type": data_type, "msa": msa, "before": before, "fit": fit}


def test_the_walks_fit_is_the_fit_over_its_rows_tree_and_lengths(fitted_walk):
    w = fitted_walk
    names, msa, fit = w["names"], w["msa"], w["fit"]
    n = len(names)
    left, right, branch = W.walk_tree(names, w["newick"])
    bf = W.base_frequencies(w["seqs"]) if w["data_type"] == 1 else None
    want = host.anc_fit_branches(left, right, branch, w["before"][:n], w["data_type"], bf)
    assert fit["branch"].tobytes() == want["branch"].tobytes()
    for k in ("status", "rounds", "up_passes", "loglik_start", "loglik_end", "columns", "states", "data_type"):
        assert fit["info"][k] == want["info"][k], k
    assert fit["info"]["loglik_end"] >= fit["info"]["loglik_start"] == msa.ancestral().loglik
    assert fit["info"]["loglik_end"] > fit["info"]["loglik_start"]                  # guessed lengths are not the maximum
    assert msa.alignment_all() == w["before"] and msa.newick == w["newick"]         # the walk is not changed
    print(w["data_type"], fit["info"])


def test_the_newick_reads_back_to_the_same_tree(fitted_walk):
    w = fitted_walk
    names, fit = w["names"], w["fit"]
    left, right, _ = W.walk_tree(names, w["newick"])
    got_left, got_right, got_branch = host.newick_arrays(names, fit["newick"])
    assert (got_left, got_right) == (left, right)
    assert np.asarray(got_branch, np.float64).tobytes() == fit["branch"].tobytes()  # %.17g reads back to the same double
    assert host.arrays_newick(names, left, right, fit["branch"]) == fit["newick"]
    assert host.differing_clades(fit["newick"], w["newick"]) == 0


def test_the_options_reach_the_fit(fitted_walk):
    msa = fitted_walk["msa"]
    one = msa.fit_branches(max_rounds=1)
    assert one["info"]["rounds"] == 1 and one["info"]["status"] in ("max_rounds", "converged")
    capped = msa.fit_branches(t_max=0.05, t_min=0.01)
    assert np.all(capped["branch"][:-1] <= 0.05) and capped["branch"][-1] == 0
    with pytest.raises(W.host_error()) as e:
        msa.fit_branches(t_min=0.0)
    assert e.value.code == host.abi.PAGAN_E_ARG


def refined_by_hand(names, seqs, opts, ml):
    first = host.Msa(names, seqs, None, **opts).align()
    tree = first.alignment_tree()
    fit = None
    if ml:
        left, right, branch = host.newick_arrays(names, tree)
        fit = host.anc_fit_branches(left, right, branch, first.alignment(), first.data_type, W.base_frequencies(seqs))
        tree = host.arrays_newick(names, left, right, fit["branch"])
    second = host.Msa(names, seqs, tree, **opts).align()
    return first, second, tree, fit


def test_align_refined_with_fitted_lengths_is_the_same_steps_by_hand():
    names, seqs, _, opts, _ = W.dna_walk()
    first, second, tree, fit = refined_by_hand(names, seqs, opts, ml=True)
    msa = host.align_refined(names, seqs, rounds=1, branch_lengths="ml", **opts)
    assert len(msa.history) == 2 and msa.newick == tree == msa.history[1]["newick"] and msa.history[0]["newick"] == first.newick
    assert msa.alignment() == second.alignment()
    assert msa.history[0]["fit"] is None and msa.history[0]["loglik"] == first.ancestral().loglik
    assert msa.history[1]["loglik"] == second.ancestral().loglik
    assert msa.history[1]["fit"] == {k: fit["info"][k] for k in ("status", "rounds", "loglik_start", "loglik_end")}
    assert fit["info"]["loglik_end"] >= fit["info"]["loglik_start"]
    assert set(msa.history[1]) == {"newick", "alignment_length", "score", "changed_clades", "loglik", "fit"}
    assert msa.history[1]["score"] == float(sum(second.node_info(k).score for k in range(second.n_internal)))


def test_align_refined_without_the_keyword_is_what_it_was():
    names, seqs, _, opts, _ = W.dna_walk()
    first, second, tree, _ = refined_by_hand(names, seqs, opts, ml=False)
    msa = host.align_refined(names, seqs, rounds=1, **opts)
    assert tree != first.newick                                                      # (no fixpoint at the first round: two walks)
    assert [set(h) for h in msa.history] == [{"newick", "alignment_length", "score", "changed_clades"}] * 2
    assert msa.newick == tree and msa.alignment_all() == second.alignment_all()
    assert [h["newick"] for h in msa.history] == [first.newick, tree]
    assert msa.history[1]["score"] == float(sum(second.node_info(k).score for k in range(second.n_internal)))
    assert msa.history[1]["alignment_length"] == len(second.alignment()[0])
    assert msa.history[1]["changed_clades"] == host.differing_clades(tree, first.newick)
