"""Branch lengths by maximum likelihood, the host side (no GPU): the derivative matrices against the rate matrix, the reading of
tests/pycheck_brlen.py against itself (its g1 against a difference quotient of its own log likelihood, the root's two children,
its fit on every case the GPU tests fit), the step rule on a table written by hand, the refusals, the byte prediction, and what
the compiler made of pa_branch (the definition is in include/pagan_host.h, "branch lengths by maximum likelihood")."""
import ctypes as C
import os
import sys
from decimal import Decimal

import numpy as np
import pytest

from pagan2_msa_amd import abi, host, synth

import pycheck_anc as A
import pycheck_brlen as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _code(fn, *args, **kw):
    from pagan2_msa_amd import PaganError
    with pytest.raises(PaganError) as e:
        fn(*args, **kw)
    return e.value.code


# ---- the derivative matrices -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("data_type,bf", [(1, None), (1, A.BASE_FREQ), (2, None), (3, None)])
def test_derivative_matrices_are_q_p_and_q_q_p(data_type, bf):
    """D_1 = Q P and D_2 = Q Q P in numpy, to the 1e-12 tests/test_anc_cpu.py holds P(s) P(t) = P(s + t) to, relative to the largest
    entry of Q resp. Q Q (the entries of P are at most 1; those of the codon model's Q are not)."""
    Q, _ = host.anc_rate_matrix(data_type, bf)
    for t in (0.0, 0.05, 0.2, 0.9, 50.0):
        P = host.anc_pmatrix(data_type, t, bf)[0]
        D1, D2 = host.anc_pmatrix_deriv(data_type, t, 1, bf), host.anc_pmatrix_deriv(data_type, t, 2, bf)
        assert D1.shape == P.shape == D2.shape
        assert np.abs(D1 - Q @ P).max() <= 1e-12 * max(1.0, np.abs(Q).max()), t
        assert np.abs(D2 - Q @ Q @ P).max() <= 1e-12 * max(1.0, np.abs(Q @ Q).max()), t
    assert np.any(host.anc_pmatrix_deriv(data_type, 0.2, 1, bf) < 0)               # not clamped
    assert _code(host.anc_pmatrix_deriv, data_type, 0.1, 0, bf) == abi.PAGAN_E_ARG
    assert _code(host.anc_pmatrix_deriv, data_type, 0.1, 3, bf) == abi.PAGAN_E_ARG
    assert _code(host.anc_pmatrix_deriv, data_type, -0.1, 1, bf) == abi.PAGAN_E_ARG
    assert _code(host.anc_pmatrix_deriv, 0, 0.1, 1) == abi.PAGAN_E_ARG


# ---- the reading against itself ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["three:65", "eight:63", "onesided", "pair:64"])
def test_g1_is_the_slope_of_the_readings_own_loglik(name):
    """A central difference of the reading's exact log likelihood over t_c -+ h, h = 1e-4.  Its truncation error is h^2 / 6 times
    the third derivative, which like g1 is a sum over the informative columns of quotients bounded by powers of the largest rate
    (< 4 for DNA) times abs1: below 1e-6 abs1.  The matrices are the library's doubles, so P(t + h) - P(t - h) carries 2^-53 / 2h =
    6e-13 of noise an entry: 1e-9 covers it."""
    c = B.case(name)
    r, h = c["brlen"], 1e-4
    n = len(c["rows"])
    checked = 0
    for node in range(2 * n - 2):
        if r["informative"][node] == 0 or c["branch"][node] < 10 * h:
            continue
        ll = []
        for d in (-h, h):
            br = list(c["branch"])
            br[node] += d
            ll.append(B.evaluate(c["left"], c["right"], br, c["rows"], c["data_type"], c["base_freq"], derivs=False)["loglik"])
        slope = float((ll[1] - ll[0]) / (Decimal(br[node]) - Decimal(c["branch"][node] - h)))
        assert abs(slope - float(r["g1"][node])) <= 1e-6 * float(r["abs1"][node]) + 1e-9, (name, node)
        checked += 1
    assert checked >= min(2, 2 * n - 2)


@pytest.mark.parametrize("name", ["pair:130", "three:65", "eight:130", "onesided", "sim:5"])
def test_the_roots_two_children_have_one_slope(name):
    """The pulley principle: g1 and g2 of the root's two children agree to the model's reversibility error, a few 1e-15 an entry
    of P (tests/test_anc_cpu.py holds detailed balance to 1e-12), times the sums of absolute values behind them."""
    c = B.case(name)
    r = c["brlen"]
    a, b = c["left"][-1], c["right"][-1]
    assert r["informative"][a] == r["informative"][b] > 0
    assert abs(float(r["g1"][a] - r["g1"][b])) <= 1e-12 * float(r["abs1"][a] + r["abs1"][b])
    assert abs(float(r["g2"][a] - r["g2"][b])) <= 1e-12 * float(r["abs2"][a] + r["abs2"][b])


def test_what_is_not_informative_counts_nothing():
    c = B.case("onesided")
    r, has = c["brlen"], c["brlen"]["has_data"]
    rows = c["rows"]
    L = len(rows[0])
    # branch 0 (leaf 0): informative where it holds data and another leaf does too
    want = sum(1 for col in range(L) if has[0, col] and (has[1, col] or has[2, col] or has[3, col]))
    assert r["informative"][0] == want < L
    # branch 5 (the node over leaves 2, 3): the other side of the root must hold data
    assert r["informative"][5] == sum(1 for col in range(L) if has[5, col] and has[4, col]) < L
    imp = B.case("impossible")["brlen"]
    assert imp["loglik"] == Decimal("-Infinity") and all(x.is_finite() for x in imp["g1"] + imp["g2"])
    assert max(imp["informative"]) <= 1                                            # columns 1 and 2 cannot happen: f_0 = 0


# ---- the step rule -------------------------------------------------------------------------------------------------------------------

STEP_TABLE = [
    # t, g1, g2, t_min, t_max, want
    (0.1, 2.0, -40.0, 1e-6, 10.0, 0.1 + 2.0 / 40.0),         # Newton
    (0.1, -1.0, -40.0, 1e-6, 10.0, 0.1 - 1.0 / 40.0),
    (0.1, 3.0, 5.0, 1e-6, 10.0, 0.2),                        # not concave, uphill: doubled
    (0.1, -3.0, 5.0, 1e-6, 10.0, 0.05),                      # not concave, downhill: halved
    (0.1, 3.0, 0.0, 1e-6, 10.0, 0.2),
    (0.1, 0.0, 2.0, 1e-6, 10.0, 0.05),
    (0.1, 100.0, -1.0, 1e-6, 10.0, 0.4),                     # Newton beyond 4 t
    (0.1, -100.0, -1.0, 1e-6, 10.0, 0.025),                  # Newton below t / 4 (and below 0)
    (4.0, 100.0, -1.0, 1e-6, 10.0, 10.0),                    # t_max
    (2e-6, -100.0, -1.0, 1e-6, 10.0, 1e-6),                  # t_min
    (0.0, 5.0, -1.0, 1e-6, 10.0, 1e-6),                      # [t / 4, 4 t] is [0, 0]; then t_min
    (0.1, 0.0, 0.0, 1e-6, 10.0, 0.1),                        # no information
    (20.0, 0.0, 0.0, 1e-6, 10.0, 20.0),                      # ... not even the clamp
    (0.1, float("nan"), -1.0, 1e-6, 10.0, 0.1),
    (0.1, 1.0, float("inf"), 1e-6, 10.0, 0.1),
    (0.1, float("-inf"), -1.0, 1e-6, 10.0, 0.1),
]


def test_the_step_rule_on_a_table_written_by_hand():
    for t, g1, g2, lo, hi, want in STEP_TABLE:
        assert host.anc_branch_step(t, g1, g2, lo, hi) == want, (t, g1, g2)
        assert B.step(t, g1, g2, lo, hi) == want, (t, g1, g2)
    assert np.isnan(host.anc_branch_step(float("nan"), 1.0, -1.0))
    assert host.anc_branch_step(0.1, 2.0, -40.0) == 0.1 + 2.0 / 40.0               # the defaults


# ---- the reading's fit ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", B.FIT_CASES + B.UNRELATED_CASES)
def test_the_readings_fit(name):
    c, f = B.case(name), B.fitted(name)
    if name in B.FIT_CASES:
        assert f["status"] == "converged", (name, f["status"], f["rounds"])
    assert all(b >= a for a, b in zip(f["loglik"], f["loglik"][1:])) and len(f["loglik"]) >= 2
    free, rl, rr = B.parameters(c["left"], c["right"], c["branch"])
    assert all(B.T_MIN <= f["branch"][v] <= B.T_MAX for v in free) and B.T_MIN <= f["branch"][rl] + f["branch"][rr] <= B.T_MAX * (1 + 1e-15)
    if name in B.SIM_CASES:                               # what a maximum must satisfy
        assert f["loglik"][-1] >= c["brlen"]["loglik"]
    if name == "twins":
        assert f["branch"][0] == B.T_MIN and f["branch"][1] == B.T_MIN
    tau_in, tau = c["branch"][rl] + c["branch"][rr], f["branch"][rl] + f["branch"][rr]
    assert abs(f["branch"][rl] / tau - c["branch"][rl] / tau_in) <= 1e-15


def test_the_cases_reach_the_line_search():
    """A condition on the input of tests/test_brlen_gpu.py's round-by-round test, checked with the reading alone: within 16 rounds
    `unrelated` (4 leaves, 64 columns, DNA) halves a step in at least four rounds and twice in at least one, and no candidate,
    rejected or accepted, comes within 1e-6 of the log likelihood it is held against -- at least 1000 times columns *
    pycheck_anc.tolerance, the bound on the device's log likelihood error, so the device decides as the reading does.  None of the
    other fitted cases ever halves (which is why this one is there)."""
    c = B.case("unrelated")
    assert len(c["rows"]) == 4 and len(c["rows"][0]) == 64 and c["data_type"] == 1
    assert 1e-6 >= 1000 * 64 * A.tolerance(c["left"], c["right"], 4)
    f = B.fit(c["left"], c["right"], c["branch"], c["rows"], c["data_type"], c["base_freq"], max_rounds=16)
    tried = f["decisions"]
    assert f["rounds"] == 16 == len(tried) and f["status"] == "max_rounds"
    assert sum(1 for d in tried if len(d) > 1) >= 4 and max(len(d) for d in tried) >= 3
    for r, d in enumerate(tried):
        assert [a for a, _ in d] == [2.0 ** -i for i in range(len(d))]
        assert all(diff <= -1e-6 for _, diff in d[:-1]) and d[-1][1] >= 1e-6, (r, d)
    print("halvings by round:", [len(d) - 1 for d in tried], "smallest margin: %.3g" % min(abs(x) for d in tried for _, x in d))
    # the same on the four-wave kernels: 4 leaves, 64 random protein columns, a step halved within 12 rounds
    c = B.case("unrelated:protein")
    assert len(c["rows"]) == 4 and len(c["rows"][0]) == 64 and c["data_type"] == 2 and B.LINE_SEARCH_CASES == {"unrelated": 16, "unrelated:protein": 12}
    assert 1e-6 >= 1000 * 64 * A.tolerance(c["left"], c["right"], 20)
    tried = B.fit(c["left"], c["right"], c["branch"], c["rows"], c["data_type"], c["base_freq"], max_rounds=12)["decisions"]
    assert len(tried) == 12 and sum(1 for d in tried if len(d) > 1) >= 1
    for r, d in enumerate(tried):
        assert all(diff <= -1e-6 for _, diff in d[:-1]) and d[-1][1] >= 1e-6, (r, d)
    print("protein, halvings by round:", [len(d) - 1 for d in tried], "smallest margin: %.3g" % min(abs(x) for d in tried for _, x in d))
    for name in B.FIT_CASES:
        assert all(len(d) <= 1 for d in B.fitted(name)["decisions"]), name


def test_the_four_wave_cases_cover_every_kind_of_branch():
    """Trees alone (no reading): over the S = 20 cases together and over the S = 61 cases together a leaf and an internal child each
    occur beside a leaf and beside an internal sibling, and an internal child both under the root and under an inner node."""
    for t, names in B.FOUR_WAVE_CASES.items():
        seen = set()
        for name in names:
            c = B._named(name) or A.case(name)
            assert c["data_type"] == t and name in B.DERIV_CASES
            seen |= B.kinds(c["left"], c["right"])
        assert {k[:2] for k in seen} == {(False, False), (False, True), (True, False), (True, True)}, t
        assert {k[2] for k in seen if k[0]} == {False, True}, t
    c = B._named("codon:tree")                           # a random tree: what the balanced ones lack
    assert len(c["rows"]) == 5 and len(c["rows"][0]) == 3 * 65 and {(False, True), (True, False)} <= {k[:2] for k in B.kinds(c["left"], c["right"])}
    for name in ("sim:protein", "sim:codon"):            # a gap in every ninth column
        c = B._named(name)
        w = 3 if c["data_type"] == 3 else 1
        assert len(c["rows"]) == {2: 4, 3: 3}[c["data_type"]] and len(c["rows"][0]) == 65 * w and c["base_freq"] is None
        assert all(sum(r[col * w:(col + 1) * w] == "-" * w for r in c["rows"]) == (col % 9 == 0) for col in range(65))


def test_the_start_by_hand():
    """pycheck_brlen.start against the header's sentence on numbers written out: every free branch within [t_min, t_max], tau
    within them and split in branch_in's proportion (1/2 where both are 0), lengths inside the bounds untouched."""
    left, right = [0, 2, 4], [1, 3, 5]
    assert B.start(left, right, [0.0, 50.0, 0.3, 2e-7, 0.0, 0.13, 7.0]) == [1e-6, 10.0, 0.3, 1e-6, 0.0, 0.13, 0.0]
    assert B.start(left, right, [0.1, 0.2, 0.3, 0.4, 5.0, 15.0, 0.0]) == [0.1, 0.2, 0.3, 0.4, 10.0 * 0.25, 10.0 - 10.0 * 0.25, 0.0]
    assert B.start([0], [1], [0.0, 0.0, 0.0]) == [5e-7, 1e-6 - 5e-7, 0.0]
    assert B.start([0], [1], [0.0, 3e-7, 0.0]) == [0.0, 1e-6, 0.0]
    assert B.start([0], [1], [10.0, 20.0, 0.0]) == [10.0 * (10.0 / 30.0), 10.0 - 10.0 * (10.0 / 30.0), 0.0]
    assert B.start([0], [1], [0.3, 0.4, 0.0], 0.1, 0.1) == [0.1 * (0.3 / 0.7), 0.1 - 0.1 * (0.3 / 0.7), 0.0]
    # the fit of the reading starts there
    f = B.fit([0], [1], [10.0, 20.0, 0.0], ["ACGT", "ACGA"], 1, None, max_rounds=0)
    assert f["branch"] == B.start([0], [1], [10.0, 20.0, 0.0]) and f["rounds"] == 0 and f["decisions"] == []


# ---- refusals, no device --------------------------------------------------------------------------------------------------------

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


def test_refusals_come_before_any_device_is_asked_for():
    left, right, branch = [0, 2, 4], [1, 3, 5], [0.1] * 7
    rows = ["ACGT", "ACGA", "ACCT", "AGGT"]
    for fn in (host.anc_branch_derivs, host.anc_fit_branches):
        assert _code(fn, left, right, branch, ["ACGT", "ACG", "ACCT", "AGGT"], 1) == abi.PAGAN_E_ARG
        assert _code(fn, left, right, branch, rows, 3) == abi.PAGAN_E_ARG
        assert _code(fn, left, right, branch, rows, 7) == abi.PAGAN_E_ARG
        assert _code(fn, [0, 2, 4], [1, 3, 4], branch, rows, 1) == host.PAGAN_E_TREE
        assert _code(fn, left, right, [0.1, -0.1, 0.1, 0.1, 0.1, 0.1, 0.0], rows, 1) == host.PAGAN_E_TREE
    for bad in (dict(t_min=0.0), dict(t_min=-1.0), dict(t_min=1.0, t_max=0.5), dict(t_max=float("inf")), dict(tol=-1e-3),
                dict(tol=float("nan")), dict(max_rounds=-1)):
        assert _code(host.anc_fit_branches, left, right, branch, rows, 1, **bad) == abi.PAGAN_E_ARG, bad


def test_without_a_device_the_device_entries_say_so(pg, oracle):
    c = B.case("three:65")
    args = (c["left"], c["right"], c["branch"], c["rows"], 1, c["base_freq"])
    tn, ts, nwk = synth.evolve_balanced(4, 60, branch=0.03, sub=0.03, indel_start=0.01, mean_len=3, seed=12)
    msa = host.Msa(tn, ts, nwk, use_anchors=0)
    assert _code(msa.fit_branches) == abi.PAGAN_E_ARG                              # before the rows exist
    msa.set_batch_backend(_oracle_backend(oracle))
    msa.align()
    before = msa.alignment_all()
    if pg.device_count() > 0:                                                      # (on a GPU machine: the same calls work)
        assert host.anc_branch_derivs(*args)["info"]["columns"] == 65
        assert host.anc_fit_branches(*args)["info"]["columns"] == 65
        assert msa.fit_branches()["newick"].endswith(";")
    else:
        assert _code(host.anc_branch_derivs, *args) == abi.PAGAN_E_NODEVICE
        assert _code(host.anc_fit_branches, *args) == abi.PAGAN_E_NODEVICE
        assert _code(msa.fit_branches) == abi.PAGAN_E_NODEVICE
        # align_refined: the first walk needs a device itself, so its refusal is reached through the test seam's walk
        real = host.Msa

        class SeamMsa(real):
            def align(self):
                self.set_batch_backend(_oracle_backend(oracle))
                return super().align()
        host.Msa = SeamMsa
        try:
            assert _code(host.align_refined, tn, ts, 1, nwk, branch_lengths="ml", use_anchors=0) == abi.PAGAN_E_NODEVICE
        finally:
            host.Msa = real
    with pytest.raises(ValueError):
        host.align_refined(tn, ts, 1, nwk, branch_lengths="nj")
    assert msa.alignment_all() == before


def test_fit_predict_bytes_is_monotone():
    base = host.anc_fit_predict_bytes(8, 1000, 1, 256)
    assert base > host.anc_predict_bytes(8, 1000, 1, 256) - 7 * 4 * 8 * 1000       # no posterior slots; the rest and more
    sizes = [host.anc_fit_predict_bytes(n, 1000, 1, 256) for n in (2, 3, 8, 9, 16, 100)]
    assert sizes == sorted(set(sizes))
    cols = [host.anc_fit_predict_bytes(8, L, 1, 256) for L in (0, 1, 64, 256, 257, 1000, 100000)]
    assert cols == sorted(cols) and cols[0] == cols[1] == cols[2] < cols[3] < cols[4] < cols[5] < cols[6]      # the codes of every chunk stay
    assert host.anc_fit_predict_bytes(8, 1000, 1, 256) < host.anc_fit_predict_bytes(8, 1000, 2, 256) < host.anc_fit_predict_bytes(8, 1000, 3, 256)
    assert _code(host.anc_fit_predict_bytes, 1, 10, 1) == abi.PAGAN_E_ARG
    assert _code(host.anc_fit_predict_bytes, 8, -1, 1) == abi.PAGAN_E_ARG
    assert _code(host.anc_fit_predict_bytes, 8, 1 << 31, 1) == abi.PAGAN_E_ARG
    assert _code(host.anc_fit_predict_bytes, 8, 10, 0) == abi.PAGAN_E_ARG


def test_the_new_symbols_are_exported(pg):
    lib = pg.lib()
    for sym in ("pagan_anc_pmatrix_deriv", "pagan_anc_branch_step", "pagan_anc_branch_derivs", "pagan_anc_fit_branches",
                "pagan_anc_fit_predict_bytes", "pagan_msa_fit_branches"):
        assert sym in host.HOST_EXPORTED
        getattr(lib, sym)


# ---- the code object ---------------------------------------------------------------------------------------------------------------

def test_pa_branch_of_dna_keeps_to_its_registers():
    """dp_anc.hip compiled afresh to gfx950 assembly (no GPU needed): from the kernel metadata pa_branch<4, 1> has no private
    segment and spills nothing; the four-wave instantiations are there (their registers are recorded in DESIGN.md)."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import check_scratch
    finally:
        sys.path.pop(0)
    funcs, meta = check_scratch.analyse(check_scratch.assemble("dp_anc.hip"))
    kernels = {k: v for k, v in meta.items() if "pa_branchILi" in k and v}
    dna = [v for k, v in kernels.items() if "pa_branchILi4ELi1E" in k]
    assert len(dna) == 1 and len(kernels) == 3, sorted(meta)
    assert dna[0]["private_segment_fixed_size"] == 0 and dna[0]["sgpr_spill_count"] == 0 and dna[0]["vgpr_spill_count"] == 0, dna
    assert not [k for k in funcs if "pa_branchILi4ELi1E" in k], funcs              # (a function is listed only if it touches scratch)
    # pa_up, pa_down and pa_encode are in the same file: still without a private segment
    for k, v in meta.items():
        if v and any(x in k for x in ("pa_up", "pa_down", "pa_encode")):
            assert v["private_segment_fixed_size"] == 0, (k, v)
