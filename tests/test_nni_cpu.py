"""Tree search by nearest-neighbour interchange (include/pagan_host.h), no GPU: the two readings against each other and against
full pruning, the host-only entry points (apply, select, predict_bytes) against the reading and on hand-worked trees, the search
loop of the reading on the cases tests/test_nni_gpu.py relies on, and the refusals.

  (i) == (ii): the header's formula equals full pruning of the rearranged tree -- to 1e-30 for ordinary candidates (50 digits), for
  the root edge within the Chapman-Kolmogorov defect of anc_pmatrix, measured here from the matrices themselves.
  The fp64 reading (pycheck_nni_fp64.py, what the device is held to byte for byte) against the 50-digit one within
  pycheck_nni.gain_tolerance ("Test bounds")."""
import ctypes as C
from decimal import Decimal

import numpy as np
import pytest

from pagan2_msa_amd import abi, host, synth

import pycheck_anc as A
import pycheck_nni as N
import pycheck_nni_fp64 as NF


def _code(fn, *args, **kw):
    from pagan2_msa_amd import PaganError
    with pytest.raises(PaganError) as e:
        fn(*args, **kw)
    return e.value.code


def args_of(c):
    return (c["left"], c["right"], c["branch"], c["rows"], c["data_type"], c["base_freq"])


_exact = {}


def exact(name):
    if name not in _exact:
        _exact[name] = N.gains_by_formula(*args_of(N.case(name)))
    return _exact[name]


# ---- the readings ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", N.EXACT_CASES)
def test_the_formula_is_full_pruning_of_the_rearranged_tree(name):
    c = N.case(name)
    n, S, L = len(c["rows"]), A.STATES[c["data_type"]], len(A.leaf_sets(c["rows"][0], c["data_type"]))
    kind, _ = N.kinds(c["left"], c["right"])
    start = N.loglik_by_pruning(*args_of(c))
    for node, w in exact(name).items():
        for k in (1, 2):
            if w["degenerate"][k - 1] or not start.is_finite():
                continue                                             # (an impossible column: no log likelihood to compare)
            d = abs(N.gain_by_pruning(*args_of(c), node, k, start) - w["gain"][k - 1])
            if kind[node - n] == 1:
                assert d <= Decimal("1e-30"), (node, k, d)
            else:
                bound = N.ck_defect(c["left"], c["right"], c["branch"], c["data_type"], c["base_freq"]) * L * S
                print("%s: root edge k = %d: |formula - pruning| = %.3g, bound %.3g" % (name, k, float(d), bound))
                assert float(d) <= bound, (node, k, float(d), bound)


@pytest.mark.parametrize("name", N.EXACT_CASES)
def test_the_fp64_reading_against_the_fifty_digit_reading(name):
    c = N.case(name)
    got = NF.of_case(c)
    n, S, L = len(c["rows"]), A.STATES[c["data_type"]], len(got["col_lik"])
    kind, _ = N.kinds(c["left"], c["right"])
    assert [int(x) for x in got["kind"]] == kind
    worst = 0.0
    for node, w in exact(name).items():
        q = node - n
        for k in (0, 1):
            assert int(got["degenerate"][q, k]) == w["degenerate"][k], (node, k)
            size = abs(np.log(got["M"][q, k])) + abs(int(got["E"][q, k])) * np.log(2.0)
            tol = N.gain_tolerance(c["left"], c["right"], S, L, size)
            err = float(abs(Decimal(float(got["gain"][q, k])) - w["gain"][k]))
            assert err <= tol, (node, k, err, tol)
            worst = max(worst, err / tol)
    for q in range(n - 1):
        if not kind[q]:
            assert got["M"][q].tolist() == [0.5, 0.5] and got["E"][q].tolist() == [1, 1] and not got["gain"][q].any() and not got["degenerate"][q].any()
    print("%s: largest error over its bound %.3g" % (name, worst))


def test_the_column_product_is_the_headers_tree():
    """By hand: 64 ones are (0.5, 1); a 3.0 in column 0 and a 0.75 in column 32 meet in the tree's first step; a second block is
    multiplied onto the running pair; the pair is the product whatever the length."""
    assert NF.column_product(np.ones(64)) == (0.5, 1) and NF.column_product(np.ones(1)) == (0.5, 1)
    x = np.ones(130)
    x[0], x[32], x[64], x[129] = 3.0, 0.75, 2.0 ** -40, 5.0
    M, E = NF.column_product(x)
    assert M * 2.0 ** E == 3.0 * 0.75 * 2.0 ** -40 * 5.0
    assert NF.column_product(np.array([0.0, 1.0]))[0] == 0.0         # frexp(0) = (0, 0): an underflown ratio zeroes the product


def test_an_impossible_column_counts_as_degenerate():
    for name in ("impossible", "impossible:protein"):
        w = exact(name)
        assert len(w) == 1 and all(d > 0 for x in w.values() for d in x["degenerate"]), w


def test_the_spot_cases_put_a_leaf_and_an_internal_node_in_every_position():
    seen = set()
    for name in N.SPOT_CASES:
        c = N.case(name)
        seen |= N.positions(c["left"], c["right"])
    assert seen == {(p, i) for p in "adbe" for i in (False, True)}


# ---- apply ---------------------------------------------------------------------------------------------------------------------

def test_apply_on_hand_worked_trees():
    # (((0, 1), 2), 3): nodes 4 = (0, 1), 5 = (4, 2), 6 = (5, 3).  The one candidate is 4: a = 0, d = 1, b = 2.
    left, right, branch = [0, 4, 5], [1, 2, 3], [0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.0]
    assert N.kinds(left, right)[0] == [1, 0, 0]
    # k = 1: 2 into 4's left slot, 0 where 2 was: 4 = (2, 1), 5 = (4, 0): already in post-order
    assert host.anc_nni_apply(left, right, branch, 4, 1) == ([2, 4, 5], [1, 0, 3], branch, list(range(7)))
    # k = 2: 4 = (0, 2), 5 = (4, 1)
    assert host.anc_nni_apply(left, right, branch, 4, 2) == ([0, 4, 5], [2, 1, 3], branch, list(range(7)))
    # ((0, 1), (2, 3)): the root edge only, at 4: a = 0, d = 1, e = 2, b = 3
    left, right = [0, 2, 4], [1, 3, 5]
    assert N.kinds(left, right)[0] == [2, 0, 0]
    assert host.anc_nni_apply(left, right, branch, 4, 1) == ([3, 2, 4], [1, 0, 5], branch, list(range(7)))       # ((3, 1), (2, 0))
    assert host.anc_nni_apply(left, right, branch, 4, 2) == ([0, 2, 4], [3, 1, 5], branch, list(range(7)))       # ((0, 3), (2, 1))
    for node, k in ((5, 1), (6, 1), (4, 0), (4, 3), (3, 1), (7, 1)):
        assert _code(host.anc_nni_apply, left, right, branch, node, k) == abi.PAGAN_E_ARG, (node, k)
    assert _code(host.anc_nni_apply, [0, 2, 4], [1, 3, 4], branch, 4, 1) == host.PAGAN_E_TREE


def test_apply_moves_an_internal_sibling_with_a_higher_id():
    # 6 leaves: 6 = (0, 1), 7 = (2, 3), 8 = (6, 7), 9 = (8, 4), 10 = (9, 5).  Candidate 6: a = 0, d = 1, b = 7 > 6.
    left, right = [0, 2, 6, 8, 9], [1, 3, 7, 4, 5]
    branch = [0.01 * (v + 1) for v in range(10)] + [0.0]
    assert N.kinds(left, right)[0] == [1, 1, 1, 0, 0]
    l, r, b, perm = host.anc_nni_apply(left, right, branch, 6, 1)
    # 6 = (7, 1), 8 = (6, 0) on the old ids; post-order: (2, 3) first, then ((2, 3), 1), then (.., 0)
    assert (l, r) == ([2, 6, 7, 8, 9], [3, 1, 0, 4, 5])
    assert perm == [0, 1, 2, 3, 4, 5, 7, 6, 8, 9, 10]
    assert b == [branch[perm.index(v)] for v in range(11)] and b[6] == branch[7] and b[7] == branch[6]
    assert (l, r, b, perm) == tuple(N.apply(left, right, branch, 6, 1))


@pytest.mark.parametrize("name", ["cat4:1", "bal4:1", "eight:dna", "small:protein"] + N.SPOT_CASES)
def test_apply_is_the_readings_and_the_same_swap_again_restores_the_clades(name):
    c = N.case(name)
    n = len(c["rows"])
    before = N.clades(c["left"], c["right"])
    for cand in N.candidates(c["left"], c["right"]):
        for k in (1, 2):
            want = N.apply(c["left"], c["right"], c["branch"], cand["c"], k)
            got = host.anc_nni_apply(c["left"], c["right"], c["branch"], cand["c"], k)
            assert got == tuple(want), (cand, k)
            l, r, b, perm = got
            host.anc_check_tree(l, r, b)
            assert sorted(perm) == list(range(2 * n - 1)) and perm[:n] == list(range(n)) and perm[-1] == 2 * n - 2
            assert N.clades(l, r) != before
            # the node that was c holds b and the child that stayed; the same k there exchanges them back
            back = host.anc_nni_apply(l, r, b, perm[cand["c"]], k)
            assert N.clades(back[0], back[1]) == before, (cand, k)
            assert sorted(back[2]) == sorted(c["branch"])


# ---- select --------------------------------------------------------------------------------------------------------------------

def _planted(n, gains, degenerate=()):
    g, d = np.zeros((n - 1, 2)), np.zeros((n - 1, 2), np.int64)
    for (node, k), x in gains.items():
        g[node - n, k - 1] = x
    for node, k in degenerate:
        d[node - n, k - 1] = 1
    return g, d


def test_select_on_planted_gains():
    # the 6-leaf tree above: candidates 6 (v = 8), 7 (v = 8), 8 (v = 9)
    left, right = [0, 2, 6, 8, 9], [1, 3, 7, 4, 5]
    both = lambda g, d, m=1e-3: (host.anc_nni_select(left, right, g, d, m), N.select(left, right, g, d, m))
    got, want = both(*_planted(6, {(6, 1): 2.0, (7, 2): 3.0, (8, 1): 1.0}))
    assert got == want == [(7, 2)]                                   # 6 and 8 share node 8 with 7's edge
    got, want = both(*_planted(6, {(6, 1): 2.0, (7, 2): 2.0}))
    assert got == want == [(6, 1)]                                   # a tie: the lower c
    got, want = both(*_planted(6, {(6, 1): 2.0, (6, 2): 2.0}))
    assert got == want == [(6, 1)]                                   # k = 2 only when strictly better
    got, want = both(*_planted(6, {(6, 1): 2.0, (6, 2): 2.5}))
    assert got == want == [(6, 2)]
    got, want = both(*_planted(6, {(6, 1): 2.0, (6, 2): 2.5}, [(6, 2)]))
    assert got == want == []                                         # the better k is degenerate: the candidate does not qualify
    got, want = both(*_planted(6, {(6, 1): 2.0, (6, 2): 1.5}, [(6, 2)]))
    assert got == want == [(6, 1)]
    got, want = both(*_planted(6, {(6, 1): 1e-3}))
    assert got == want == []                                         # a gain equal to min_gain
    got, want = both(*_planted(6, {(6, 1): 1e-3}), 0.0)
    assert got == want == [(6, 1)]
    got, want = both(*_planted(6, {(9, 1): 5.0, (10, 2): 5.0, (6, 1): -1.0}))
    assert got == want == []                                         # nodes without a candidate are not read; a loss is no gain
    # 8 leaves, ((0,1),(2,3)) and ((4,5),(6,7)) under the root: 8..11 cherries, 12 = (8, 9), 13 = (10, 11), 14 = (12, 13)
    left, right = [0, 2, 4, 6, 8, 10, 12], [1, 3, 5, 7, 9, 11, 13]
    assert N.kinds(left, right)[0] == [1, 1, 1, 1, 2, 0, 0]
    both = lambda g, d, m=1e-3: (host.anc_nni_select(left, right, g, d, m), N.select(left, right, g, d, m))
    got, want = both(*_planted(8, {(12, 1): 4.0, (8, 1): 3.0, (10, 2): 2.0, (11, 1): 1.0}))
    assert got == want == [(12, 1)]                                  # the root edge takes 12, 13 and the root: 8 (v = 12), 10 and 11 (v = 13) go
    got, want = both(*_planted(8, {(12, 1): 1.0, (8, 1): 3.0, (10, 2): 2.0, (11, 1): 1.5}))
    assert got == want == [(8, 1), (10, 2)]                          # 11 shares 13 with 10; the root edge shares 12 with 8
    assert _code(host.anc_nni_select, left, right, np.zeros((7, 2)), np.zeros((7, 2), np.int64), -1.0) == abi.PAGAN_E_ARG
    assert _code(host.anc_nni_select, left, right, np.zeros((7, 2)), np.zeros((7, 2), np.int64), float("nan")) == abi.PAGAN_E_ARG
    assert _code(host.anc_nni_select, [0, 2, 4, 6, 8, 10, 12], [1, 3, 5, 7, 9, 11, 12], np.zeros((7, 2)), np.zeros((7, 2), np.int64)) == host.PAGAN_E_TREE


# ---- the search loop of the reading ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", sorted(N.SEARCH_CASES))
def test_the_reading_finds_the_planted_tree_again(n):
    s = N.search_case(n)
    true, start = s["true"], s["start"]
    assert len(N.clades(start[0], start[1]) - N.clades(true[0], true[1])) >= 2
    found = NF.search(*start, s["rows"], 1, A.BASE_FREQ)
    assert found["status"] == "converged" and len(found["swaps"]) >= 2
    assert N.clades(found["left"], found["right"]) == N.clades(true[0], true[1])
    assert all(b >= a for a, b in zip(found["loglik"], found["loglik"][1:]))


def test_the_fallback_to_a_single_swap_in_the_readings_loop():
    """On fallback_case the joint application of round 0's swaps lowers the log likelihood and the first alone is accepted; with
    planted functions: both lower it, and the search stalls at the round's start tree."""
    f = N.fallback_case()
    found = NF.search(*f["start"], f["rows"], 1, A.BASE_FREQ, min_gain=f["min_gain"])
    first = [s for s in found["swaps"] if s[0] == 0]
    assert len(first) == 1 and first[0][3] == 0, found["swaps"]
    assert all(b >= a for a, b in zip(found["loglik"], found["loglik"][1:]))
    left, right, branch = f["start"]
    gains = NF.reading(left, right, branch, f["rows"], 1, A.BASE_FREQ)
    assert len(N.select(left, right, gains["gain"], gains["degenerate"], 0.0)) > 1
    calls = []

    def falling(l, r, b):
        calls.append((l, r))
        return -float(len(calls))
    stalled = N.search(left, right, branch, 0.0, 4, lambda l, r, b: (gains["gain"], gains["degenerate"]), falling)
    assert stalled["status"] == "stalled" and len(calls) == 3 and stalled["swaps"] == [] and stalled["loglik"] == [-1.0]
    assert (stalled["left"], stalled["right"]) == (list(left), list(right))


# ---- bytes, refusals, no device -------------------------------------------------------------------------------------------------------

def test_nni_predict_bytes():
    base = host.anc_nni_predict_bytes(8, 1000, 1, 256)
    assert base > host.anc_fit_predict_bytes(8, 1000, 1, 256)
    sizes = [host.anc_nni_predict_bytes(n, 1000, 1, 256) for n in (2, 3, 8, 9, 16, 100)]
    assert sizes == sorted(set(sizes))
    cols = [host.anc_nni_predict_bytes(8, L, 1, 256) for L in (0, 1, 64, 256, 257, 1000, 100000)]
    assert cols == sorted(cols) and cols[0] == cols[1] == cols[2] < cols[3] < cols[4]
    assert host.anc_nni_predict_bytes(8, 1000, 1, 256) < host.anc_nni_predict_bytes(8, 1000, 2, 256) < host.anc_nni_predict_bytes(8, 1000, 3, 256)
    for bad in ((1, 10, 1), (8, -1, 1), (8, 1 << 31, 1), (8, 10, 0)):
        assert _code(host.anc_nni_predict_bytes, *bad) == abi.PAGAN_E_ARG


def test_refusals_come_before_any_device_is_asked_for():
    left, right, branch = [0, 2, 4], [1, 3, 5], [0.1] * 7
    rows = ["ACGT", "ACGA", "ACCT", "AGGT"]
    for fn in (host.anc_nni_gains, host.anc_nni_search):
        assert _code(fn, left, right, branch, ["ACGT", "ACG", "ACCT", "AGGT"], 1) == abi.PAGAN_E_ARG
        assert _code(fn, left, right, branch, rows, 3) == abi.PAGAN_E_ARG
        assert _code(fn, left, right, branch, rows, 7) == abi.PAGAN_E_ARG
        assert _code(fn, [0, 2, 4], [1, 3, 4], branch, rows, 1) == host.PAGAN_E_TREE
    for bad in (dict(min_gain=-1.0), dict(min_gain=float("nan")), dict(max_rounds=-1), dict(fit_rounds=-1), dict(t_min=0.0),
                dict(t_min=1.0, t_max=0.5), dict(tol=-1.0)):
        assert _code(host.anc_nni_search, left, right, branch, rows, 1, **bad) == abi.PAGAN_E_ARG, bad
    with pytest.raises(ValueError):
        host.align_refined(["a", "b"], ["ACGT", "ACGA"], tree_search="spr")


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
    c = N.case("cat4:65")
    tn, ts, nwk = synth.evolve_balanced(4, 60, branch=0.03, sub=0.03, indel_start=0.01, mean_len=3, seed=12)
    msa = host.Msa(tn, ts, nwk, use_anchors=0)
    assert _code(msa.search_tree) == abi.PAGAN_E_ARG                                # before the rows exist
    msa.set_batch_backend(_oracle_backend(oracle))
    msa.align()
    before = msa.alignment_all()
    if pg.device_count() > 0:                                                      # (on a GPU machine: the same calls work)
        assert host.anc_nni_gains(*args_of(c))["info"]["columns"] == 65
        assert host.anc_nni_search(*args_of(c))["info"]["columns"] == 65
        assert msa.search_tree()["newick"].endswith(";")
    else:
        assert _code(host.anc_nni_gains, *args_of(c)) == abi.PAGAN_E_NODEVICE
        assert _code(host.anc_nni_search, *args_of(c)) == abi.PAGAN_E_NODEVICE
        assert _code(msa.search_tree) == abi.PAGAN_E_NODEVICE
    assert msa.alignment_all() == before


def test_the_new_symbols_are_exported(pg):
    lib = pg.lib()
    for sym in ("pagan_anc_nni_gains", "pagan_anc_nni_apply", "pagan_anc_nni_select", "pagan_anc_nni_search", "pagan_anc_nni_predict_bytes",
                "pagan_msa_search_tree"):
        assert sym in host.HOST_EXPORTED
        getattr(lib, sym)
