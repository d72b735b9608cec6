"""Ancestral states by marginal likelihood, on the device: pa_encode / pa_up / pa_down (csrc/dp_anc.hip) against the Python
readings of tests/pycheck_anc.py.

Tolerance (derived, not measured): every sum is over non-negative terms, so a column likelihood's relative error is at most the
number of roundings on its deepest chain times 2^-53; tol = 8 h (S + 3) 2^-53 with h the tree's height in nodes.  It is taken
relative on col_lik 2^col_exp, absolute on col_loglik (plus 2^-52 |col_loglik| for the host's log) and doubled on posteriors.
`best` is compared where the reading's two largest posteriors differ by more than 4 tol; tests/test_anc_cpu.py checks with the
reading alone that this leaves out at most 1 % of any case.

The down pass has cases of its own ("Tests"): trees deep enough that the outside vectors underflow unless they are
rescaled, for all three alphabets and with internal siblings; balanced trees, zero lengths and impossible columns on the four-wave
kernels; posteriors listed as a shuffled subset, so that a slot is not the node's own index; the tie rule by an exact tie and by
the all-zero column; chunks against a reading."""
import math
from decimal import Decimal

import numpy as np
import pytest

from pagan2_msa_amd import host

import pycheck_anc as A

pytestmark = pytest.mark.gpu


def run(c, post_nodes=None):
    n = len(c["rows"])
    nodes = list(range(n, 2 * n - 1)) if post_nodes is None else post_nodes
    return host.anc_reconstruct(c["left"], c["right"], c["branch"], c["rows"], c["data_type"], c["base_freq"], nodes)


def check_likelihood(c, got):
    S = A.STATES[c["data_type"]]
    tol = A.tolerance(c["left"], c["right"], S)
    want = c["reading"]["lik"]
    L = len(want)
    assert got["info"]["columns"] == L and got["info"]["states"] == S and got["info"]["data_type"] == c["data_type"]
    assert len(got["col_lik"]) == L
    for col in range(L):
        lik = Decimal(float(got["col_lik"][col])) * Decimal(2) ** int(got["col_exp"][col])
        assert abs(lik - want[col]) <= Decimal(tol) * want[col], (col, lik, want[col])
        if want[col] == 0:
            assert got["col_loglik"][col] == -math.inf
        else:
            ll = float(want[col].ln())
            assert abs(got["col_loglik"][col] - ll) <= tol + 2.0 ** -52 * abs(ll), (col, got["col_loglik"][col], ll)
    total = 0.0
    for x in got["col_loglik"]:                                   # the left-to-right fp64 sum, bit for bit
        total += float(x)
    assert got["loglik"] == total or (math.isnan(total) and math.isnan(got["loglik"]))
    assert np.array_equal(got["has_data"], c["reading"]["has_data"])
    n = len(c["rows"])
    assert 0 < got["info"]["device_bytes"] <= host.anc_predict_bytes(n, L, c["data_type"])
    return tol


def check_best(c, got, tol):
    """best, best_p of every internal node against the reading, where the tie condition decides; returns the cells left out."""
    post = c["reading"]["post"]
    n, L = len(c["rows"]), len(post[0])
    assert got["best"].shape == (n - 1, L) and got["best_p"].shape == (n - 1, L)
    left_out = 0
    for k in range(n - 1):
        for col in range(L):
            want = post[k][col]
            s, p = A.best_of(want)
            if A.decided(want, tol):
                assert got["best"][k, col] == s, (k, col)
                assert abs(float(got["best_p"][k, col]) - float(p)) <= 2 * tol + 2.0 ** -24 * float(p), (k, col)      # (best_p is a float)
            else:
                left_out += 1
    assert left_out <= 0.01 * (n - 1) * L                            # a condition of the test, not a measurement
    return left_out


def check_post_rows(c, got_post, nodes, tol):
    """got_post[q] against the reading's posterior of internal node nodes[q], every column and state."""
    post = c["reading"]["post"]
    n, L = len(c["rows"]), len(post[0])
    assert got_post.shape == (len(nodes), L, A.STATES[c["data_type"]])
    for q, v in enumerate(nodes):
        for col in range(L):
            want = post[v - n][col]
            have = got_post[q, col]
            assert all(abs(Decimal(float(h)) - w) <= Decimal(2 * tol) for h, w in zip(have, want)), (v, col)


def check_posteriors(c, got, tol):
    """post, best, best_p of every internal node (got was run with all of them listed) against the reading."""
    n = len(c["rows"])
    check_post_rows(c, got["post"], list(range(n, 2 * n - 1)), tol)
    return check_best(c, got, tol)


def same_bytes(a, b, keys):
    for k in keys:
        assert np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes(), k


OUTPUTS = ("col_lik", "col_exp", "col_loglik", "loglik", "best", "best_p", "has_data", "post")
_full = {}


def full_run(name):
    """The case run once with every internal node's posterior asked for, shared by the tests that compare with it (read only)."""
    if name not in _full:
        _full[name] = run(A.case(name))
        for v in _full[name].values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
    return _full[name]


def post_subsets(n):
    """Two strict subsets of the internal nodes n .. 2 n - 2: in descending order, and shuffled with the root second."""
    ids = list(range(n, 2 * n - 1))
    descending = [v for v in reversed(ids) if v != ids[1]]
    rest = ids[1:-1]
    shuffled = [rest[0], ids[-1]] + rest[:0:-1]
    assert len(set(shuffled)) == len(shuffled) < len(ids) and ids[-1] not in (shuffled[0], shuffled[-1])
    assert shuffled != sorted(shuffled) and shuffled != sorted(shuffled, reverse=True)
    return descending, shuffled


# ---- worked by hand ---------------------------------------------------------------------------------------------------------

def test_two_leaves_one_column_by_hand():
    Pl, pi = host.anc_pmatrix(1, 0.1, A.BASE_FREQ)
    Pr, _ = host.anc_pmatrix(1, 0.3, A.BASE_FREQ)
    tol = 8 * 2 * 7 * 2.0 ** -53
    got = host.anc_reconstruct([0], [1], [0.1, 0.3, 0.0], ["A", "G"], 1, A.BASE_FREQ, [2])
    terms = pi * Pl[:, 0] * Pr[:, 2]                                # pi[s] P_l[s][A] P_r[s][G]
    lik = got["col_lik"][0] * 2.0 ** int(got["col_exp"][0])
    assert abs(lik - terms.sum()) <= 2 * tol * terms.sum()
    assert np.all(np.abs(got["post"][0, 0] - terms / terms.sum()) <= 4 * tol)
    assert got["best"][0, 0] == int(np.argmax(terms)) and abs(got["best_p"][0, 0] - terms.max() / terms.sum()) < 1e-6
    assert got["has_data"].tolist() == [[1], [1], [1]]
    # one leaf missing: the other's message alone; both missing: the likelihood is exactly 1 and the posterior the prior
    got = host.anc_reconstruct([0], [1], [0.1, 0.3, 0.0], ["-A", "C-"], 1, A.BASE_FREQ, [2])
    for col, terms in ((0, pi * Pr[:, 1]), (1, pi * Pl[:, 0])):
        lik = got["col_lik"][col] * 2.0 ** int(got["col_exp"][col])
        assert abs(lik - terms.sum()) <= 2 * tol * terms.sum()
        assert np.all(np.abs(got["post"][0, col] - terms / terms.sum()) <= 4 * tol)
    assert got["has_data"].tolist() == [[0, 1], [1, 0], [1, 1]]
    got = host.anc_reconstruct([0], [1], [0.1, 0.3, 0.0], ["-", "?"], 1, A.BASE_FREQ, [2])
    assert got["col_lik"][0] == 1.0 and got["col_exp"][0] == 0 and got["col_loglik"][0] == 0.0 and got["loglik"] == 0.0
    assert np.all(np.abs(got["post"][0, 0] - pi / pi.sum()) <= 4 * tol) and got["best"][0, 0] == 3
    assert got["has_data"].tolist() == [[0], [0], [0]]


def test_one_letter_in_every_leaf_is_every_ancestors_letter():
    left, right, branch = A.balanced4([0.2, 0.15, 0.1, 0.05, 0.12, 0.07])
    got = host.anc_reconstruct(left, right, branch, ["ACGT"] * 4, 1, A.BASE_FREQ)
    assert got["best"].tolist() == [[0, 1, 2, 3]] * 3
    assert np.all(got["best_p"] > 0.9)


# ---- lane and wave edges, against the reading by definition ---------------------------------------------------------------

@pytest.mark.parametrize("L", A.EDGE_COLUMNS)
def test_column_edges_against_the_definition(L):
    c = A.case("edge:%d" % L)
    got = run(c)
    tol = check_likelihood(c, got)
    check_posteriors(c, got, tol)
    if L > 2:
        assert got["col_lik"][1] == 1.0 and not got["has_data"][:, 1].any()         # the all-gap column
        assert got["has_data"][:5, 2].sum() == 1                                    # the column with a single letter


# ---- scaling ---------------------------------------------------------------------------------------------------------------------

def test_caterpillar_of_600_leaves_keeps_its_exponent():
    c = A.case("caterpillar")
    got = run(c, [])
    check_likelihood(c, got)
    assert np.any(got["col_exp"] != 0) and got["col_exp"].min() < -1100              # below fp64's range without the bookkeeping
    assert np.all((got["col_lik"] > 0) & np.isfinite(got["col_loglik"]))


@pytest.mark.parametrize("name", A.DEEP_CASES)
def test_deep_trees_keep_their_posteriors(name):
    """Trees on which the outside vectors leave fp64's range unless pa_down rescales them (tests/test_anc_cpu.py asserts that they
    do), every posterior asked for; in deep:cherries the sibling of every internal spine child is an internal node."""
    c = A.case(name)
    got = full_run(name)
    tol = check_likelihood(c, got)
    check_posteriors(c, got, tol)
    n, S = len(c["rows"]), A.STATES[c["data_type"]]
    for v in A.deepest(c["left"], c["right"], 10):
        p = got["post"][v - n]
        assert np.all(np.isfinite(p)) and np.all(np.abs(p.sum(axis=1) - 1.0) <= 2 * S * tol), v


def test_best_without_any_posterior_asked_for():
    """The walk's path: post_nodes empty, so every slot is -1; best and best_p still come from the rescaled outside vectors."""
    c = A.case("deep:dna")
    got = run(c, [])
    assert got["post"].size == 0
    tol = check_likelihood(c, got)
    check_best(c, got, tol)
    same_bytes(got, full_run("deep:dna"), [k for k in OUTPUTS if k != "post"])


# ---- branch lengths at the ends -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["zero", "long"])
def test_zero_length_and_very_long_branches(name):
    c = A.case(name)
    got = run(c)
    check_posteriors(c, got, check_likelihood(c, got))


def test_a_column_that_cannot_happen():
    """Two leaves at length 0 under one parent with different letters: likelihood 0, log -inf, no posterior."""
    c = A.case("impossible")
    got = run(c)
    check_likelihood(c, got)
    assert got["col_lik"].tolist()[1:] == [0.0, 0.0] and got["col_lik"][0] > 0
    assert got["loglik"] == -math.inf
    assert np.all(got["post"][:, 1:, :] == 0) and np.all(got["best_p"][:, 1:] == 0) and np.all(np.isfinite(got["post"]))
    assert np.all(got["best"][:, 1:] == 0)                            # the first state of an all-zero vector, by the tie rule


@pytest.mark.parametrize("name", ["impossible:protein", "impossible:codon"])
def test_a_column_that_cannot_happen_on_the_four_wave_kernels(name):
    c = A.case(name)
    got = run(c)
    check_likelihood(c, got)
    never = [col for col, x in enumerate(c["reading"]["lik"]) if x == 0]
    assert never == [1, 2]
    assert np.all(got["col_lik"][never] == 0) and np.all(got["col_loglik"][never] == -math.inf) and got["loglik"] == -math.inf
    assert np.all(got["post"][:, never, :] == 0) and np.all(got["best_p"][:, never] == 0)
    assert np.all(got["best"][:, never] == 0)                         # not the last state: the tie rule is the first largest
    assert np.all(np.isfinite(got["post"])) and np.all(np.isfinite(got["best_p"])) and np.all(np.isfinite(got["col_lik"]))
    can = [0, 3, 4]                                                   # the columns beside them are ordinary ones
    assert np.all(got["col_lik"][can] > 0)
    post = c["reading"]["post"]
    tol = A.tolerance(c["left"], c["right"], A.STATES[c["data_type"]])
    for k in range(3):
        for col in can:
            assert all(abs(Decimal(float(h)) - w) <= Decimal(2 * tol) for h, w in zip(got["post"][k, col], post[k][col])), (k, col)


def test_an_exact_tie_goes_to_the_first_state():
    """Equal base frequencies and a column without data: the root's q is 1 * 0.25 in every state, exactly.  Only the root is pinned:
    below it the outside vectors carry P's rounding and the tie is no longer exact."""
    bf = (0.25,) * 4
    assert host.anc_pmatrix(1, 0.1, bf)[1].tolist() == [0.25] * 4
    left, right, branch = A.balanced4([0.2, 0.15, 0.1, 0.05, 0.12, 0.07])
    got = host.anc_reconstruct(left, right, branch, ["A-C", "A-G", "C-G", "T-G"], 1, bf, [4, 5, 6])
    assert not got["has_data"][:, 1].any() and got["col_lik"][1] == 1.0
    assert got["best"][2, 1] == 0 and got["best_p"][2, 1] == 0.25
    assert got["post"][2, 1].tolist() == [0.25] * 4
    assert got["best"][2, 2] == 2 and got["best_p"][2, 2] > 0.9       # (the column beside it, C G G G, is decided by its data)


# ---- protein and codons ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["protein", "codon"])
def test_protein_and_codons_against_the_pruning_reading(name):
    c = A.case(name)
    got = run(c)
    assert got["info"]["columns"] == 65
    check_posteriors(c, got, check_likelihood(c, got))
    missing = np.array([[s is None for s in A.leaf_sets(r, c["data_type"])] for r in c["rows"]])
    assert missing.sum() > 10 and np.array_equal(got["has_data"][:len(c["rows"])], ~missing)       # X, non-sense triplets, gaps


@pytest.mark.parametrize("name", A.BALANCED_CASES + ["zero:protein", "zero:codon"])
def test_balanced_trees_and_zero_lengths_on_the_four_wave_kernels(name):
    """Balanced trees: half the internal nodes have two internal children, so pa_down goes twice through its loop over the sides
    and uses its LDS vector again.  zero:*: identity matrices under the four waves."""
    c = A.case(name)
    got = run(c)
    check_posteriors(c, got, check_likelihood(c, got))


# ---- the slot of a posterior ------------------------------------------------------------------------------------------------------

def check_subset(c, name, nodes):
    """post[q] is node nodes[q]'s posterior -- by the reading, and the bytes of the run that listed every node -- and nothing else
    of the outputs depends on what was listed."""
    n = len(c["rows"])
    everything = full_run(name)
    got = run(c, nodes)
    tol = check_likelihood(c, got)
    check_post_rows(c, got["post"], nodes, tol)
    for q, v in enumerate(nodes):
        assert got["post"][q].tobytes() == everything["post"][v - n].tobytes(), (q, v)
    same_bytes(got, everything, [k for k in OUTPUTS if k != "post"])
    return got


@pytest.mark.parametrize("name", ["protein", "edge:130"])
def test_posteriors_land_in_the_slot_they_were_listed_at(name):
    c = A.case(name)
    for nodes in post_subsets(len(c["rows"])):
        check_subset(c, name, nodes)


# ---- bit stability ---------------------------------------------------------------------------------------------------------------

def test_outputs_are_the_same_bytes_from_run_to_run_and_for_every_chunk_size(monkeypatch):
    c = A.case("chunks")
    a, b = run(c), run(c)
    assert a["info"]["chunks"] == 1 and a["info"]["chunk_cols"] == 256
    keys = [k for k in a if k != "info"]
    for k in keys:
        assert np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes(), k
    monkeypatch.setenv("PAGAN_ANC_CHUNK_COLS", "64")               # (read from the environment at every call)
    z = run(c)
    assert z["info"]["chunk_cols"] == 64 and z["info"]["chunks"] == 4
    assert z["info"]["device_bytes"] < a["info"]["device_bytes"] and z["info"]["device_bytes"] <= host.anc_predict_bytes(6, 200, 1)
    for k in keys:
        assert np.asarray(a[k]).tobytes() == np.asarray(z[k]).tobytes(), k


def test_chunks_against_the_reading_on_the_four_wave_kernel(monkeypatch):
    """130 protein columns: one chunk by default, three under PAGAN_ANC_CHUNK_COLS=64, the last of them two columns wide.  Both
    against the reading and the same bytes; then a shuffled subset of the posteriors, so that a chunk that does not start at
    column 0 is put into `post` through slots that are not the nodes' own order."""
    c = A.case("chunks:protein")
    n = len(c["rows"])
    whole = full_run("chunks:protein")
    assert whole["info"]["chunks"] == 1 and whole["info"]["columns"] == 130
    check_posteriors(c, whole, check_likelihood(c, whole))
    monkeypatch.setenv("PAGAN_ANC_CHUNK_COLS", "64")
    cut = run(c)
    assert cut["info"]["chunk_cols"] == 64 and cut["info"]["chunks"] == 3
    check_posteriors(c, cut, check_likelihood(c, cut))
    same_bytes(cut, whole, OUTPUTS)
    for nodes in post_subsets(n):
        got = check_subset(c, "chunks:protein", nodes)
        assert got["info"]["chunks"] == 3
