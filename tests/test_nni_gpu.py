"""pa_nni and pa_nni_fold (csrc/dp_anc_nni.inc) and the search on top of them, on the device.

Bytes: M, E and degenerate of every candidate byte for byte against the float64 reading in the header's order
(tests/pycheck_nni_fp64.py, which tests/test_nni_cpu.py holds to the 50-digit reading first) -- include/pagan_host.h fixes the order
of every sum, the quotient and the column product, so nothing there has a tolerance.  `gain` passes through the host's log and is
held to log(M) + E log 2 recomputed here.  The invariant: a gain is the log likelihood anc_reconstruct gives the rearranged tree
minus the tree's own, within the derived bounds of the three.  The search: swap by swap and round by round the replay of
pycheck_nni.search on the fp64 reading, every accepted log likelihood anc_reconstruct's own bytes."""
import math

import numpy as np
import pytest

from pagan2_msa_amd import host

import pycheck_anc as A
import pycheck_nni as N
import pycheck_nni_fp64 as NF
import test_anc_walk_gpu as W

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
_readings = {}


def args_of(c):
    return (c["left"], c["right"], c["branch"], c["rows"], c["data_type"], c["base_freq"])


def reading_of(name):
    if name not in _readings:
        _readings[name] = NF.of_case(N.case(name))
    return _readings[name]


def compare(name):
    c, want = N.case(name), reading_of(name)
    got = host.anc_nni_gains(*args_of(c))
    n = len(c["rows"])
    assert got["kind"].tolist() == want["kind"].tolist() and got["info"]["candidates"] == int(np.count_nonzero(want["kind"]))
    for q in range(n - 1):
        for k in (0, 1):
            where = "%s: node %d, arrangement %d" % (name, n + q, k + 1)
            assert int(got["degenerate"][q, k]) == int(want["degenerate"][q, k]), where
            assert int(got["E"][q, k]) == int(want["E"][q, k]), where
            assert got["M"][q, k].tobytes() == want["M"][q, k].tobytes(), "%s: device %r, reading %r" % (where, got["M"][q, k], want["M"][q, k])
            # the host's log: within 4 u (|log M| + |E| log 2) of the same expression taken here
            M, E = float(got["M"][q, k]), int(got["E"][q, k])
            if M > 0:
                again = math.log(M) + E * math.log(2.0)
                assert abs(float(got["gain"][q, k]) - again) <= 4 * U * (abs(math.log(M)) + abs(E) * math.log(2.0)), where
    assert got["loglik"] == host.anc_reconstruct(*args_of(c))["loglik"]               # (-inf with an impossible column, in both)
    return got


@pytest.mark.parametrize("name", N.BYTE_CASES)
def test_the_gains_are_the_headers_operations(name):
    got = compare(name)
    if name.startswith("impossible"):
        assert got["degenerate"][got["kind"] > 0].min() > 0          # the impossible columns are counted, not multiplied in
    if name == "deep":
        assert got["info"]["candidates"] == 597 and got["info"]["chunks"] == 1
        assert np.isfinite(got["gain"]).all() and np.abs(got["gain"]).max() < 100   # the outside vectors' powers of two cancelled


def test_one_chunk_and_four_give_the_same_bytes(monkeypatch):
    one = compare("chunks")
    assert one["info"]["chunks"] == 1
    monkeypatch.setenv("PAGAN_ANC_CHUNK_COLS", "64")
    four = compare("chunks")
    assert four["info"]["chunks"] == 4 and four["info"]["chunk_cols"] == 64
    for k in ("M", "E", "degenerate", "gain", "kind"):
        assert one[k].tobytes() == four[k].tobytes(), k
    assert one["loglik"] == four["loglik"]


def test_a_gain_is_the_log_likelihood_of_the_rearranged_tree_minus_the_trees_own():
    """eight:dna, every candidate and both arrangements: ten short reconstructions.  The bound: pycheck_nni.loglik_tolerance of
    each of the two log likelihoods, pycheck_nni.gain_tolerance of the gain, and for the root edge the Chapman-Kolmogorov defect
    times 2 L ("Test bounds")."""
    c = N.case("eight:dna")
    n, S = len(c["rows"]), 4
    got = host.anc_nni_gains(*args_of(c))
    start = host.anc_reconstruct(*args_of(c))
    L = len(start["col_loglik"])
    assert got["loglik"] == start["loglik"]
    defect = N.ck_defect(c["left"], c["right"], c["branch"], c["data_type"], c["base_freq"])
    worst = 0.0
    for cand in N.candidates(c["left"], c["right"]):
        q = cand["c"] - n
        for k in (1, 2):
            assert got["degenerate"][q, k - 1] == 0
            l, r, b, _ = host.anc_nni_apply(c["left"], c["right"], c["branch"], cand["c"], k)
            after = host.anc_reconstruct(l, r, b, c["rows"], c["data_type"], c["base_freq"])
            M, E = float(got["M"][q, k - 1]), int(got["E"][q, k - 1])
            bound = (N.loglik_tolerance(c["left"], c["right"], S, start["col_loglik"]) + N.loglik_tolerance(l, r, S, after["col_loglik"])
                     + N.gain_tolerance(c["left"], c["right"], S, L, abs(math.log(M)) + abs(E) * math.log(2.0))
                     + (2 * L * defect if cand["kind"] == 2 else 0.0))
            err = abs((after["loglik"] - start["loglik"]) - float(got["gain"][q, k - 1]))
            print("node %d k %d: gain %.6f, difference of logliks off by %.3g, bound %.3g" % (cand["c"], k, got["gain"][q, k - 1], err, bound))
            assert err <= bound, (cand, k, err, bound)
            worst = max(worst, err / bound)
    print("largest error over its bound %.3g" % worst)


# ---- the search ---------------------------------------------------------------------------------------------------------------

def follow(start, rows, replay, found, names):
    """The device's search against the reading's replay, round by round."""
    assert found["info"]["status"] == replay["status"]
    assert [(s["round"], s["node"], s["k"], s["joint"]) for s in found["swaps"]] == [s[:4] for s in replay["swaps"]]
    for s, r in zip(found["swaps"], replay["swaps"]):
        assert abs(s["gain"] - r[4]) <= 8 * U * max(1.0, abs(r[4]))
    assert (found["left"], found["right"]) == (replay["left"], replay["right"])
    assert np.asarray(found["branch"]).tobytes() == np.asarray(replay["branch"], np.float64).tobytes()
    assert len(found["loglik"]) == len(replay["loglik"])
    if replay["status"] != "max_rounds":                             # the last evaluation selected nothing, or what it selected was refused
        assert found["info"]["rounds"] == len(found["loglik"])
    assert all(b >= a for a, b in zip(found["loglik"], found["loglik"][1:]))
    trees = [start] + list(replay["trees"])
    for ll, want, tree in zip(found["loglik"], replay["loglik"], trees):
        assert ll == host.anc_reconstruct(*tree, rows, 1, A.BASE_FREQ)["loglik"]      # fit_rounds = 0: anc_reconstruct's bytes
        assert abs(ll - want) <= 8 * U * abs(want)
    assert found["info"]["swaps"] == len(found["swaps"]) and found["info"]["loglik_end"] == found["loglik"][-1]


@pytest.mark.parametrize("n", sorted(N.SEARCH_CASES))
def test_the_search_is_the_readings_replay_and_finds_the_planted_tree(n):
    s = N.search_case(n)
    names = ["s%d" % k for k in range(n)]
    replay = NF.search(*s["start"], s["rows"], 1, A.BASE_FREQ)
    found = host.anc_nni_search(*s["start"], s["rows"], 1, A.BASE_FREQ)
    follow(s["start"], s["rows"], replay, found, names)
    assert found["info"]["status"] == "converged"
    true_newick = host.arrays_newick(names, *s["true"])
    assert host.differing_clades(host.arrays_newick(names, *s["start"]), true_newick) >= 2
    assert host.differing_clades(host.arrays_newick(names, found["left"], found["right"], found["branch"]), true_newick) == 0
    assert N.clades(found["left"], found["right"]) == N.clades(s["true"][0], s["true"][1])
    print(n, found["info"])


def test_the_search_falls_back_to_the_first_swap_alone():
    f = N.fallback_case()
    replay = NF.search(*f["start"], f["rows"], 1, A.BASE_FREQ, min_gain=f["min_gain"])
    found = host.anc_nni_search(*f["start"], f["rows"], 1, A.BASE_FREQ, min_gain=f["min_gain"])
    follow(f["start"], f["rows"], replay, found, None)
    first = [s for s in found["swaps"] if s["round"] == 0]
    assert len(first) == 1 and first[0]["joint"] == 0


def test_the_round_limit_and_the_fit_between_rounds():
    s = N.search_case(12)
    none = host.anc_nni_search(*s["start"], s["rows"], 1, A.BASE_FREQ, max_rounds=0)
    assert none["info"]["status"] == "max_rounds" and none["swaps"] == [] and (none["left"], none["right"]) == (list(s["start"][0]), list(s["start"][1]))
    assert none["loglik"].tolist() == [host.anc_reconstruct(*s["start"], s["rows"], 1, A.BASE_FREQ)["loglik"]]
    one = host.anc_nni_search(*s["start"], s["rows"], 1, A.BASE_FREQ, max_rounds=1)
    assert one["info"]["status"] == "max_rounds" and one["info"]["rounds"] == 1 and len(one["loglik"]) == 2
    plain = host.anc_nni_search(*s["start"], s["rows"], 1, A.BASE_FREQ)
    fitted = host.anc_nni_search(*s["start"], s["rows"], 1, A.BASE_FREQ, fit_rounds=4, t_min=1e-4, t_max=2.0)
    assert all(b >= a for a, b in zip(fitted["loglik"], fitted["loglik"][1:]))
    # round 0 sees the same gains and applies the same swaps; the fit starts from that tree's loglik and never lowers it.  (What
    # comes after need not be the plain search's: a fitted wrong edge shrinks, and the swap across it gains less -- DESIGN.md 14.)
    assert fitted["loglik"][0] == plain["loglik"][0] and fitted["loglik"][1] > plain["loglik"][1]
    assert [(s_["node"], s_["k"]) for s_ in fitted["swaps"] if s_["round"] == 0] == [(s_["node"], s_["k"]) for s_ in plain["swaps"] if s_["round"] == 0]
    assert all(1e-4 <= t <= 2.0 for t in fitted["branch"][:-1]) and fitted["branch"][-1] == 0
    assert fitted["loglik"][-1] == host.anc_reconstruct(fitted["left"], fitted["right"], fitted["branch"], s["rows"], 1, A.BASE_FREQ)["loglik"]
    assert fitted["info"]["loglik_end"] == fitted["loglik"][-1] and fitted["info"]["up_passes"] > plain["info"]["up_passes"]
    print("plain", plain["loglik"], "fitted", fitted["loglik"], fitted["info"]["status"], fitted["swaps"])


def test_the_fit_between_rounds_never_lowers_an_accepted_loglik_from_lengths_outside_its_bounds():
    """The 8-leaf search case with lengths the fit's start has to move: two leaf branches of 0 (a UPGMA tree has them) and
    t_min = 0.05 above several true lengths.  Every accepted log likelihood is still no lower than the one before, the first
    accepted one no lower than the plain search's (the same swaps, then a fit that may only raise it or be dropped), and the
    last one is anc_reconstruct's bytes at the lengths returned."""
    s = N.search_case(8)
    left, right, branch = s["start"]
    branch = list(branch)
    branch[0] = branch[3] = 0.0
    plain = host.anc_nni_search(left, right, branch, s["rows"], 1, A.BASE_FREQ, max_rounds=1)
    for t_min, t_max in ((0.05, 10.0), (0.2, 0.25), (1e-6, 0.06)):
        fitted = host.anc_nni_search(left, right, branch, s["rows"], 1, A.BASE_FREQ, fit_rounds=2, t_min=t_min, t_max=t_max)
        lls = fitted["loglik"]
        assert all(b >= a for a, b in zip(lls, lls[1:])), (t_min, t_max, lls)
        assert lls[0] == plain["loglik"][0] and lls[1] >= plain["loglik"][1]
        assert lls[-1] == host.anc_reconstruct(fitted["left"], fitted["right"], fitted["branch"], s["rows"], 1, A.BASE_FREQ)["loglik"]
        print(t_min, t_max, lls, fitted["info"]["status"])


# ---- over a walk ---------------------------------------------------------------------------------------------------------------

def test_the_walks_search_is_the_search_over_its_rows_tree_and_lengths():
    names, seqs, newick, opts, data_type = W.dna_walk()
    msa = host.Msa(names, seqs, newick, **opts).align()
    before = msa.alignment_all()
    n = len(names)
    left, right, branch = W.walk_tree(names, newick)
    want = host.anc_nni_search(left, right, branch, before[:n], data_type, W.base_frequencies(seqs))
    got = msa.search_tree()
    assert got["newick"] == host.arrays_newick(names, want["left"], want["right"], want["branch"])
    for k in ("status", "rounds", "swaps", "up_passes", "loglik_start", "loglik_end", "columns", "states"):
        assert got["info"][k] == want["info"][k], k
    assert got["info"]["loglik_start"] == msa.ancestral().loglik
    assert msa.alignment_all() == before and msa.newick == newick
    assert msa.search_tree(max_rounds=0)["info"]["rounds"] == 0
    with pytest.raises(W.host_error()) as e:
        msa.search_tree(min_gain=-1.0)
    assert e.value.code == host.abi.PAGAN_E_ARG


def test_align_refined_with_the_search_is_the_same_steps_by_hand():
    names, seqs, _, opts, _ = W.dna_walk()
    first = host.Msa(names, seqs, None, **opts).align()
    left, right, branch = host.newick_arrays(names, first.alignment_tree())
    search = host.anc_nni_search(left, right, branch, first.alignment(), first.data_type, W.base_frequencies(seqs))
    tree = host.arrays_newick(names, search["left"], search["right"], search["branch"])
    second = host.Msa(names, seqs, tree, **opts).align()
    msa = host.align_refined(names, seqs, rounds=1, tree_search="nni", **opts)
    assert len(msa.history) == 2 and msa.newick == tree and msa.alignment() == second.alignment()
    assert [set(h) for h in msa.history] == [{"newick", "alignment_length", "score", "changed_clades", "search"}] * 2
    assert msa.history[0]["search"] is None
    assert msa.history[1]["search"] == {k: search["info"][k] for k in ("status", "rounds", "swaps", "loglik_start", "loglik_end")}
    assert search["info"]["loglik_end"] >= search["info"]["loglik_start"]
    plain = host.align_refined(names, seqs, rounds=1, **opts)          # the default: today's history, key for key
    assert [set(h) for h in plain.history] == [{"newick", "alignment_length", "score", "changed_clades"}] * len(plain.history)
    both = host.align_refined(names, seqs, rounds=1, tree_search="nni", branch_lengths="ml", **opts)
    assert set(both.history[-1]) == {"newick", "alignment_length", "score", "changed_clades", "loglik", "fit", "search"}
    assert both.history[-1]["search"]["loglik_end"] >= both.history[-1]["search"]["loglik_start"]
