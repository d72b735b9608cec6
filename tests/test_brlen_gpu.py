"""Branch lengths by maximum likelihood on the device (csrc/dp_anc_brlen.inc) against the reading of tests/pycheck_brlen.py:
g1, g2 and the informative counts of every branch within a bound derived by counting roundings (pycheck_brlen.tolerances: not
fitted to the device), the same bytes from run to run and for every chunk size, and the fit's contract -- log likelihoods that
never fall and are pagan_anc_reconstruct's own, lengths the reading's step rule leaves where they are, bounds kept, the root's
sum split in the old proportion, the old passes untouched.  The fit itself is followed round by round: every accepted candidate is
byte for byte the header's t + alpha (t' - t) over the device's own sums, at the alpha the 50-digit reading decides for as well;
and the start keeps every parameter within its bounds, byte for byte.  (The sums themselves are held to the header's order of
operations in tests/test_anc_bytes_gpu.py.)"""
import numpy as np
import pytest

from pagan2_msa_amd import host

import pycheck_anc as A
import pycheck_brlen as B

pytestmark = pytest.mark.gpu


def args_of(c, branch=None):
    return (c["left"], c["right"], c["branch"] if branch is None else branch, c["rows"], c["data_type"], c["base_freq"])


def same_bytes(a, b):
    return all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in ("g1", "g2", "informative")) and \
        np.float64(a["loglik"]).tobytes() == np.float64(b["loglik"]).tobytes()


# ---- g1, g2, informative ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", B.DERIV_CASES)
def test_derivatives_against_the_reading(name):
    c = B.case(name)
    r, n = c["brlen"], len(c["rows"])
    L = len(r["lik"])
    d = host.anc_branch_derivs(*args_of(c))
    assert d["info"]["columns"] == L and d["info"]["rounds"] == 1 and d["info"]["up_passes"] == 1
    assert d["g1"].shape == d["g2"].shape == d["informative"].shape == (2 * n - 1,)
    assert d["g1"][-1] == 0 and d["g2"][-1] == 0 and d["informative"][-1] == 0
    assert np.all(np.isfinite(d["g1"])) and np.all(np.isfinite(d["g2"]))
    assert [int(x) for x in d["informative"]] == r["informative"]
    t1, t2 = B.tolerances(r, L)
    worst = [0.0, 0.0]
    for v in range(2 * n - 2):
        e1, e2 = abs(float(d["g1"][v]) - float(r["g1"][v])), abs(float(d["g2"][v]) - float(r["g2"][v]))
        worst = [max(worst[0], e1 / t1[v] if t1[v] else 0.0), max(worst[1], e2 / t2[v] if t2[v] else 0.0)]
        assert e1 <= t1[v] and e2 <= t2[v], (name, v, e1, t1[v], e2, t2[v])
        if r["informative"][v] == 0:
            assert d["g1"][v] == 0 and d["g2"][v] == 0                             # the exact 0
    print("%s: largest error over its bound: g1 %.3g, g2 %.3g" % (name, worst[0], worst[1]))
    rec = host.anc_reconstruct(*args_of(c))
    assert np.float64(d["loglik"]).tobytes() == np.float64(rec["loglik"]).tobytes()


def test_the_cases_cover_what_they_are_for():
    """With the readings alone: every kind of branch occurs (leaf and internal child, each under leaf and internal sibling), some
    columns are informative for one branch and not for another, an impossible column counts nothing, and the deep case's
    partials and outside vectors leave fp64's range without the rescaling the quotients never see."""
    c = B.case("eight:65")
    n = 8
    kinds = set()
    for k in range(n - 1):
        for a, b in ((c["left"][k], c["right"][k]), (c["right"][k], c["left"][k])):
            kinds.add((a >= n, b >= n))
    assert len(kinds) == 4
    # the four-wave kernels (S = 20, S = 61): over the cases of each all four (child, sibling) kinds, and an internal child both
    # under the root and under an inner node
    for t, names in B.FOUR_WAVE_CASES.items():
        assert all(name in B.DERIV_CASES and B.case(name)["data_type"] == t for name in names)
        seen = set().union(*(B.kinds(B.case(name)["left"], B.case(name)["right"]) for name in names))
        assert {k[:2] for k in seen} == {(False, False), (False, True), (True, False), (True, True)}, t
        assert {k[2] for k in seen if k[0]} == {False, True}, t
    for name in ("onesided", "onesided:protein", "onesided:codon"):
        inf = B.case(name)["brlen"]["informative"]
        assert len(set(inf[:6])) > 1 and 0 < min(inf[:6]), name
    assert B.case("impossible")["brlen"]["informative"][0] == 1                    # of three columns
    deep = B.case("deep:dna")
    assert max(deep["brlen"]["rounds"]) > 5000 and min(x for x in A.case("deep:dna")["reading"]["lik"] if x > 0) < 1e-300


# ---- bit stability -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["eight:130", "chunks:protein", "balanced:codon"])
def test_the_same_bytes_from_run_to_run_and_for_every_chunk_size(name, monkeypatch):
    c = B._named(name) or A.case(name)
    one = host.anc_branch_derivs(*args_of(c))
    assert same_bytes(one, host.anc_branch_derivs(*args_of(c)))
    monkeypatch.setenv("PAGAN_ANC_CHUNK_COLS", "64")
    small = host.anc_branch_derivs(*args_of(c))
    assert small["info"]["chunk_cols"] == 64 and small["info"]["chunks"] == (small["info"]["columns"] + 63) // 64 > one["info"]["chunks"] == 1
    assert same_bytes(one, small)
    if name == "eight:130":                              # the fit in three chunks: the same lengths and log likelihoods
        monkeypatch.delenv("PAGAN_ANC_CHUNK_COLS")
        a = host.anc_fit_branches(*args_of(c), max_rounds=4)
        monkeypatch.setenv("PAGAN_ANC_CHUNK_COLS", "64")
        b = host.anc_fit_branches(*args_of(c), max_rounds=4)
        assert a["branch"].tobytes() == b["branch"].tobytes() and a["loglik"].tobytes() == b["loglik"].tobytes()
        assert b["info"]["chunks"] == 3 and a["info"]["rounds"] == b["info"]["rounds"] == 4
        assert b["info"]["up_passes"] > a["info"]["up_passes"]                     # a round repeats the up pass chunk by chunk


# ---- the fit -----------------------------------------------------------------------------------------------------------------------

_fits = {}


def fit_of(name):
    if name not in _fits:
        c = B.case(name)
        before = host.anc_reconstruct(*args_of(c))
        f = host.anc_fit_branches(*args_of(c))
        _fits[name] = (c, f, before)
    return _fits[name]


@pytest.mark.parametrize("name", B.FIT_CASES + B.UNRELATED_CASES)
def test_the_fit_keeps_its_contract(name):
    c, f, before = fit_of(name)
    n, info, hist = len(c["rows"]), f["info"], f["loglik"]
    print(name, info["status"], info["rounds"], info["up_passes"], float(hist[0]), float(hist[-1]))
    assert len(hist) >= 2 and np.all(np.diff(hist) >= 0)
    assert info["loglik_start"] == hist[0] == before["loglik"] and info["loglik_end"] == hist[-1]
    assert info["up_passes"] >= len(hist) and info["rounds"] >= len(hist) - 1
    # the accepted log likelihood is the old up pass's own, and the old passes are untouched by a fit in between
    at = host.anc_reconstruct(*args_of(c, f["branch"]))
    assert np.float64(at["loglik"]).tobytes() == np.float64(hist[-1]).tobytes()
    again = host.anc_reconstruct(*args_of(c))
    for k in ("col_lik", "col_exp", "col_loglik", "best", "best_p", "has_data"):
        assert again[k].tobytes() == before[k].tobytes(), k
    # bounds, the root's proportion
    free, rl, rr = B.parameters(c["left"], c["right"], c["branch"])
    t = f["branch"]
    assert t[-1] == 0 and all(B.T_MIN <= t[v] <= B.T_MAX for v in free)
    tau_in, tau = c["branch"][rl] + c["branch"][rr], t[rl] + t[rr]
    assert B.T_MIN * (1 - 1e-15) <= tau <= B.T_MAX * (1 + 1e-15)
    assert abs(t[rl] / tau - c["branch"][rl] / tau_in) <= 4 * 2.0 ** -53
    if name in B.FIT_CASES:
        assert info["status"] == "converged"
    else:
        assert info["status"] in ("converged", "max_rounds", "stalled")
    if name in B.SIM_CASES:                               # the lengths the rows were simulated on cannot be better than the maximum
        assert hist[-1] >= before["loglik"] and hist[-1] > hist[0]
    if name == "twins":
        assert t[0] == B.T_MIN and t[1] == B.T_MIN


@pytest.mark.parametrize("name", B.FIT_CASES)
def test_the_readings_step_leaves_the_fitted_lengths_where_they_are(name):
    """At the returned lengths the device's own step moved nothing by more than tol; the reading's g1, g2 there differ from the
    device's by at most their bounds t1, t2, so its Newton step g1 / g2 is within tol max(t, t_min) plus
    (t1 + |g1 / g2| t2) / (|g2| - t2) of zero.  A parameter at a bound is pushed outward by the reading as well."""
    c, f, _ = fit_of(name)
    t = [float(x) for x in f["branch"]]
    r = B.evaluate(c["left"], c["right"], t, c["rows"], c["data_type"], c["base_freq"])
    t1, t2 = B.tolerances(r, len(r["lik"]))
    free, rl, rr = B.parameters(c["left"], c["right"], t)
    interior = 0
    for length, v in [(t[v], v) for v in free] + [(t[rl] + t[rr], rl)]:
        g1, g2 = float(r["g1"][v]), float(r["g2"][v])
        if length <= B.T_MIN * (1 + 1e-15) or length >= B.T_MAX * (1 - 1e-15):
            assert B.step(length, g1, g2) == min(max(length, B.T_MIN), B.T_MAX), (name, v)
            continue
        interior += 1
        assert g2 + t2[v] < 0, (name, v, g2)                                        # a maximum in the interior is concave
        bound = (t1[v] + abs(g1 / g2) * t2[v]) / (abs(g2) - t2[v])
        assert abs(g1 / g2) <= B.TOL * max(length, B.T_MIN) + bound + 4 * 2.0 ** -53 * length, (name, v, g1 / g2, bound)
    assert interior or name == "twins"


def test_the_protein_fit_in_two_chunks_is_the_one_chunk_fit(monkeypatch):
    """One chunk: a round is DOWN_ONLY on the partials the accepted up pass left.  Two chunks of 64 columns: every round repeats
    the up pass chunk by chunk (FULL).  The same lengths and log likelihoods, byte for byte."""
    c = B.case("sim:protein")
    a = host.anc_fit_branches(*args_of(c))
    monkeypatch.setenv("PAGAN_ANC_CHUNK_COLS", "64")
    b = host.anc_fit_branches(*args_of(c))
    assert a["info"]["chunks"] == 1 and b["info"]["chunks"] == 2 and b["info"]["chunk_cols"] == 64
    assert a["branch"].tobytes() == b["branch"].tobytes() and a["loglik"].tobytes() == b["loglik"].tobytes()
    assert a["info"]["status"] == b["info"]["status"] == "converged" and a["info"]["rounds"] == b["info"]["rounds"]
    assert b["info"]["up_passes"] == a["info"]["up_passes"] + b["info"]["rounds"]


def the_round(c, r, before, after, trace):
    """Round r + 1 of the fit, from the fits that stopped after r and after r + 1 rounds: the lengths after it are byte for byte
    the header's candidate of alpha = 2^-h over the device's own g1, g2 at the lengths before it (h: the up passes the round took
    beyond its first), on Python floats; the 50-digit reading finds every earlier candidate lower than the accepted log
    likelihood and this one not; its log likelihood is pagan_anc_reconstruct's at those lengths.  Returns False once the fit
    has converged."""
    left, right = c["left"], c["right"]
    t = [float(x) for x in before["branch"]]
    d = host.anc_branch_derivs(*args_of(c, t))
    assert np.float64(d["loglik"]).tobytes() == np.float64(before["loglik"][-1]).tobytes()
    stepped, tau, tau_step, moved = B.full_step(left, right, t, d["g1"], d["g2"])
    rl, rr = left[-1], right[-1]
    assert tau_step == host.anc_branch_step(t[rl] + t[rr], d["g1"][rl], d["g2"][rl])            # the left child's sums
    trace["right differs"] += tau_step != host.anc_branch_step(t[rl] + t[rr], d["g1"][rr], d["g2"][rr])
    for v, s in stepped.items():
        assert s == host.anc_branch_step(t[v], d["g1"][v], d["g2"][v])
    h = after["info"]["up_passes"] - before["info"]["up_passes"] - 1
    if moved <= B.TOL:
        assert after["info"]["status"] == "converged" and after["info"]["rounds"] == r + 1 and h == -1
        assert after["branch"].tobytes() == before["branch"].tobytes() and after["loglik"].tobytes() == before["loglik"].tobytes()
        return False
    assert after["info"]["rounds"] == r + 1 and len(after["loglik"]) == r + 2 and 0 <= h <= 5
    assert after["loglik"][:r + 1].tobytes() == before["loglik"].tobytes()
    p = B.proportion(left, right, c["branch"])
    cands = [B.candidate(left, right, t, stepped, tau, tau_step, 2.0 ** -i, p) for i in range(h + 1)]
    assert after["branch"].tobytes() == np.asarray(cands[h], np.float64).tobytes(), (r, h)
    accepted = B.evaluate(left, right, t, c["rows"], c["data_type"], c["base_freq"], derivs=False)["loglik"]
    for i, cand in enumerate(cands):
        ll = B.evaluate(left, right, cand, c["rows"], c["data_type"], c["base_freq"], derivs=False)["loglik"]
        assert (ll < accepted) == (i < h), (r, i, h, float(ll - accepted))
    rec = host.anc_reconstruct(*args_of(c, after["branch"]))
    assert np.float64(rec["loglik"]).tobytes() == np.float64(after["loglik"][r + 1]).tobytes()
    trace["halvings"].append(h)
    return True


@pytest.mark.parametrize("name", ["unrelated", "sim:protein", "unrelated:protein"])
def test_every_round_of_the_fit_is_the_step_rule_over_its_own_sums(name):
    """The fit is deterministic, so the fits of max_rounds = 0 .. 16 are its trajectory.  `unrelated` halves its steps (the
    reading: in at least four rounds, twice in one; tests/test_brlen_cpu.py holds the margins of those decisions); sim:protein
    shows that a DOWN_ONLY round on the four-wave kernels reads the partials of the accepted candidate; it never halves, so
    unrelated:protein (12 rounds, a step halved) shows the same behind a rejected retry, whose up pass was the last before the
    accepted one's."""
    c = B.case(name)
    fits = [host.anc_fit_branches(*args_of(c), max_rounds=0)]
    assert fits[0]["info"]["chunks"] == 1
    trace = {"halvings": [], "right differs": 0}
    for r in range(B.LINE_SEARCH_CASES.get(name, 16)):
        fits.append(host.anc_fit_branches(*args_of(c), max_rounds=r + 1))
        if not the_round(c, r, fits[r], fits[r + 1], trace):
            break
    print(name, "halvings by round:", trace["halvings"])
    assert trace["right differs"] > 0                                 # the root's two children's sums are not the same bytes
    if name == "unrelated":
        assert len(trace["halvings"]) == 16 and sum(1 for h in trace["halvings"] if h) >= 4 and max(trace["halvings"]) >= 2
    elif name == "unrelated:protein":
        assert len(trace["halvings"]) == 12 and max(trace["halvings"]) >= 1 and trace["halvings"][-1] == 0    # a round follows the retry
    else:
        assert fits[-1]["info"]["status"] == "converged" and len(trace["halvings"]) >= 8


def test_a_fit_that_may_not_move_returns_where_it_started():
    c = B.case("sim:3")
    f = host.anc_fit_branches(*args_of(c), max_rounds=0)
    assert f["info"]["status"] == "max_rounds" and f["info"]["rounds"] == 0 and len(f["loglik"]) == 1
    assert f["branch"].tobytes() == np.asarray(c["branch"], np.float64).tobytes()
    one = host.anc_fit_branches(*args_of(c), max_rounds=1)
    assert one["info"]["rounds"] == 1 and len(one["loglik"]) == 2 and one["loglik"][1] >= one["loglik"][0]
    # the first round's candidate is the step rule over the device's own g1, g2, whatever alpha it was accepted at
    assert the_round(c, 0, f, one, {"halvings": [], "right differs": 0})


# ---- the start: every parameter within its bounds ---------------------------------------------------------------------------------

def started(c, branch_in, **opts):
    """The fit that may not move, from branch_in: its lengths are the header's start, byte for byte, and loglik_start is
    pagan_anc_reconstruct's at those lengths."""
    f = host.anc_fit_branches(*args_of(c, branch_in), max_rounds=0, **opts)
    want = B.start(c["left"], c["right"], branch_in, opts.get("t_min", B.T_MIN), opts.get("t_max", B.T_MAX))
    assert f["branch"].tobytes() == np.asarray(want, np.float64).tobytes(), (list(f["branch"]), want)
    assert f["info"]["status"] == "max_rounds" and f["info"]["rounds"] == 0 and f["info"]["up_passes"] == 1
    rec = host.anc_reconstruct(*args_of(c, want))
    assert np.float64(f["info"]["loglik_start"]).tobytes() == np.float64(rec["loglik"]).tobytes() == np.float64(f["loglik"][0]).tobytes()
    return f["branch"]


def test_the_fit_starts_within_its_bounds():
    c = B.case("lengths")                                # free branches of length 0 and 50; the root's left branch 0: p = 0
    free, rl, rr = B.parameters(c["left"], c["right"], c["branch"])
    assert {c["branch"][v] for v in free} >= {0.0, 50.0} and c["branch"][rl] == 0.0 < c["branch"][rr]
    t = started(c, c["branch"])
    assert sorted(t[v] for v in free) == sorted(min(max(c["branch"][v], B.T_MIN), B.T_MAX) for v in free)
    assert B.T_MIN in [t[v] for v in free] and B.T_MAX in [t[v] for v in free]
    assert t[rl] == 0.0 and t[rr] == c["branch"][rr] and t[-1] == 0.0
    pair = B.case("pair:65")
    t = started(pair, [0.0, 0.0, 0.0])                   # tau -> t_min, split 1/2
    assert t[0] == B.T_MIN * 0.5 and t[1] == B.T_MIN - t[0] and t[0] + t[1] == B.T_MIN
    t = started(pair, [10.0, 20.0, 0.0])                 # tau_in = 30 -> t_max, the proportion kept
    assert t[0] == B.T_MAX * (10.0 / 30.0) and t[1] == B.T_MAX - t[0]
    assert abs(t[0] / (t[0] + t[1]) - 10.0 / 30.0) <= 4 * 2.0 ** -53


@pytest.mark.parametrize("name", ["lengths", "sim:3"])
def test_bounds_that_leave_one_point_converge_there(name):
    c = B.case(name)
    f = host.anc_fit_branches(*args_of(c), t_min=0.1, t_max=0.1)
    free, rl, rr = B.parameters(c["left"], c["right"], c["branch"])
    assert f["info"]["status"] == "converged" and f["info"]["rounds"] == 1 and len(f["loglik"]) == 1 and f["info"]["up_passes"] == 1
    assert f["branch"].tobytes() == np.asarray(B.start(c["left"], c["right"], c["branch"], 0.1, 0.1), np.float64).tobytes()
    assert all(f["branch"][v] == 0.1 for v in free)
    # tau: t_r = 0.1 - t_l carries one rounding and the sum t_l + t_r here another, each at most 2^-53 of 0.1
    assert abs(f["branch"][rl] + f["branch"][rr] - 0.1) <= 2 * 2.0 ** -53 * 0.1
    rec = host.anc_reconstruct(*args_of(c, f["branch"]))
    assert np.float64(rec["loglik"]).tobytes() == np.float64(f["loglik"][0]).tobytes()
