"""Ancestral states by marginal likelihood, the host side (no GPU): the two Python readings agree, the transition matrices are
what a reversible substitution process has, the tree check and the byte prediction do what the header says, and without a
device the device entries say so (tests/pycheck_anc.py; the definition is in include/pagan_host.h, "ancestral states by
marginal likelihood")."""
import ctypes as C
from decimal import Decimal

import numpy as np
import pytest

from pagan2_msa_amd import abi, host, synth

import pycheck_anc as A


def _code(fn, *args, **kw):
    from pagan2_msa_amd import PaganError
    with pytest.raises(PaganError) as e:
        fn(*args, **kw)
    return e.value.code


# ---- the two readings ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [3, 4, 5])
def test_the_two_readings_agree(n):
    for seed in (0, 1):
        rng = np.random.default_rng(100 * n + seed)
        left, right, branch = A.random_tree(n, rng)
        rows = A.random_rows(n, 24, 1, 10 * n + seed, share=0.3)
        a = A.by_definition(left, right, branch, rows, A.BASE_FREQ)
        b = A.pruning(left, right, branch, rows, 1, A.BASE_FREQ)
        assert np.array_equal(a["has_data"], b["has_data"])
        assert not a["has_data"][:, 1].any() and a["lik"][1] == 1 and a["has_data"][:, 2].sum() >= 2
        for x, y in zip(a["lik"], b["lik"]):
            assert abs(x - y) <= Decimal("1e-30") * y
        for k in range(n - 1):
            for col in range(24):
                assert abs(sum(a["post"][k][col]) - 1) < Decimal("1e-40")
                for x, y in zip(a["post"][k][col], b["post"][k][col]):
                    assert abs(x - y) <= Decimal("1e-30")


def test_a_reading_worked_by_hand():
    """n = 2, one column: the likelihood is sum_s pi[s] P_l[s][a] P_r[s][b], the root's posterior its terms over it."""
    Pl, pi = host.anc_pmatrix(1, 0.1, A.BASE_FREQ)
    Pr, _ = host.anc_pmatrix(1, 0.3, A.BASE_FREQ)
    r = A.pruning([0], [1], [0.1, 0.3, 0.0], ["A", "G"], 1, A.BASE_FREQ)
    terms = pi * Pl[:, 0] * Pr[:, 2]
    assert abs(float(r["lik"][0]) - terms.sum()) <= 1e-15 * terms.sum()
    assert np.allclose([float(x) for x in r["post"][0][0]], terms / terms.sum(), rtol=0, atol=1e-15)
    r = A.pruning([0], [1], [0.1, 0.3, 0.0], ["R", "-"], 1, A.BASE_FREQ)            # R = A or G; the gap counts 1
    terms = pi * (Pl[:, 0] + Pl[:, 2])
    assert abs(float(r["lik"][0]) - terms.sum()) <= 1e-15 * terms.sum()


def test_leaf_encoding_of_the_reading():
    assert A.leaf_sets("acgun-.?x", 1) == [(0,), (1,), (2,), (3,), (0, 1, 2, 3), None, None, None, None]
    assert A.leaf_sets("ARVXBZU-", 2) == [(0,), (1,), (19,), None, None, None, None, None]
    assert A.leaf_sets("AAAAACTAANNN---A-CTTTatg", 3) == [(0,), (1,), None, None, None, None, (60,), (A.CODONS.index("ATG"),)]
    assert len(A.CODONS) == 61 and "".join(A.CODONS) == host.codon_alphabet()[0][:183]


def test_every_shared_case_keeps_the_tie_condition():
    """With the reading alone: in every case the GPU tests compare `best` on, at most 1 % of the cells are left out because the
    two largest posteriors lie within 4 tol of each other."""
    for name in A.POSTERIOR_CASES:
        assert A.undecided_share(A.case(name)) <= 0.01, name


@pytest.mark.parametrize("name", A.DEEP_CASES)
def test_deep_cases_underflow_without_rescaling(name):
    """What the deep:* cases are for: with the outside vectors left unscaled (plain fp64, the partials rescaled as the header
    says), the vector at the deepest internal node lies below the normal range, 2^-1022, in a column that holds data.  A
    change of seed or size that makes the case shallow fails here, not silently on the device."""
    c = A.case(name)
    n = len(c["rows"])
    host.anc_check_tree(c["left"], c["right"], c["branch"])
    outs, has = A.outside_without_rescaling(c["left"], c["right"], c["branch"], c["rows"], c["data_type"], c["base_freq"])
    node = A.deepest(c["left"], c["right"])[0]
    top = outs[node].max(axis=0)
    under = [col for col in range(len(top)) if has[2 * n - 2, col] and top[col] < 2.0 ** -1022]
    assert under, (name, top)
    assert np.array_equal(has, c["reading"]["has_data"])


def test_balanced_and_cherry_cases_have_nodes_with_two_internal_children():
    for name in A.BALANCED_CASES:
        c = A.case(name)
        host.anc_check_tree(c["left"], c["right"], c["branch"])
        kids = A.internal_children(c["left"], c["right"])
        assert 3 * kids.count(2) >= len(kids), (name, kids)
    c = A.case("deep:cherries")
    host.anc_check_tree(c["left"], c["right"], c["branch"])                       # the walk's ids: children first, the root 2 n - 2
    n, kids = len(c["rows"]), A.internal_children(c["left"], c["right"])
    assert kids.count(0) == n // 2 and kids.count(1) == 0 and kids.count(2) == n // 2 - 1     # cherries, and spine nodes over two internal nodes
    spine, v = 0, 2 * n - 2                                                        # down the spine: the left child, while it has children of its own
    while kids[v - n] == 2:
        spine, v = spine + 1, c["left"][v - n]
    assert spine == n // 2 - 1 and v == n
    assert len(set(c["branch"][:-1])) >= 3                                         # several matrices in play


def test_impossible_cases_on_the_wider_alphabets():
    for name in ("impossible:protein", "impossible:codon"):
        c = A.case(name)
        lik = c["reading"]["lik"]
        assert [x == 0 for x in lik] == [False, True, True, False, False], name
        assert all(x == 0 for k in range(3) for col in (1, 2) for x in c["reading"]["post"][k][col])


# ---- the transition matrices -------------------------------------------------------------------------------------------

TIMES = (0.05, 0.2, 0.25, 0.7, 0.9, 50.0)


@pytest.mark.parametrize("data_type", [1, 2, 3])
def test_pmatrix_rows_sum_to_one(data_type):
    """Within 1e-12, for all three data types.  The alignment model's own matrices would miss this (DNA with unequal frequencies
    by 1.2e-8, codons by 6.6e-5: their rate matrices are float products resp. decimal literals); pagan_anc_pmatrix takes the eigen
    solution of the rate matrix made proper (include/pagan_host.h) and does not renormalise P."""
    for t in TIMES:
        P = host.anc_pmatrix(data_type, t)[0]
        assert np.all(P >= 0)
        assert np.abs(P.sum(axis=1) - 1.0).max() <= 1e-12, (t, np.abs(P.sum(axis=1) - 1.0).max())


@pytest.mark.parametrize("data_type", [1, 2, 3])
def test_pmatrix_identity_semigroup_and_detailed_balance(data_type):
    S = A.STATES[data_type]
    P0, pi = host.anc_pmatrix(data_type, 0.0)
    assert P0.shape == (S, S) and np.array_equal(P0, np.eye(S))                    # the exact identity
    assert np.all(pi > 0)
    mats = {t: host.anc_pmatrix(data_type, t)[0] for t in TIMES}
    for t, P in mats.items():
        flow = pi[:, None] * P
        assert np.all(np.abs(flow - flow.T) <= 1e-12), t                           # pi_i P_ij = pi_j P_ji
    assert np.all(np.abs(mats[0.05] @ mats[0.2] - mats[0.25]) <= 1e-12)            # P(s) P(t) = P(s + t)
    assert np.all(np.abs(mats[0.2] @ mats[0.7] - mats[0.9]) <= 1e-12)


def test_pmatrix_with_unequal_base_frequencies():
    """The frequencies the device tests use: the same properties to the same 1e-12.  pi is the four floats as doubles."""
    P0, pi = host.anc_pmatrix(1, 0.0, A.BASE_FREQ)
    assert np.array_equal(P0, np.eye(4))
    assert np.array_equal(pi, np.asarray(A.BASE_FREQ, np.float32).astype(np.float64))
    mats = {t: host.anc_pmatrix(1, t, A.BASE_FREQ)[0] for t in TIMES}
    for t, P in mats.items():
        assert np.all(P >= 0) and np.abs(P.sum(axis=1) - 1.0).max() <= 1e-12
        flow = pi[:, None] * P
        assert np.all(np.abs(flow - flow.T) <= 1e-12), t
    assert np.all(np.abs(mats[0.05] @ mats[0.2] - mats[0.25]) <= 1e-12)
    assert not np.array_equal(mats[0.2], host.anc_pmatrix(1, 0.2)[0])


# The model's rate matrices, from outside the ancestral code: the DNA matrix restated here the way Model_factory::dna_model builds
# it (float arithmetic, kappa 2, rho 1), the WAG and the codon matrix read from the data tables the alignment model is made of.

def model_rates_dna(base_freq):
    f = np.float32
    bf = [f(x) for x in base_freq]
    ka = f(2.0 / 2.0)
    piR, piY = bf[0] + bf[2], bf[1] + bf[3]
    beta = f(1) / (f(2) * piR * piY * (f(1) + ka))
    alfaY = (piR * piY * ka - bf[0] * bf[2] - bf[1] * bf[3]) / ((f(2) + f(2) * ka) * (piY * bf[0] * bf[2] * f(1) + piR * bf[1] * bf[3]))
    alfaR = f(1) * alfaY
    Q = np.zeros((4, 4), np.float64)
    Q[0, 1], Q[0, 2], Q[0, 3] = beta * bf[1], alfaR * bf[2] / piR + beta * bf[2], beta * bf[3]
    Q[1, 0], Q[1, 2], Q[1, 3] = beta * bf[0], beta * bf[2], alfaY * bf[3] / piY + beta * bf[3]
    Q[2, 0], Q[2, 1], Q[2, 3] = alfaR * bf[0] / piR + beta * bf[0], beta * bf[1], beta * bf[3]
    Q[3, 0], Q[3, 1], Q[3, 2] = beta * bf[0], alfaY * bf[1] / piY + beta * bf[1], beta * bf[2]
    assert all(type(x) is np.float32 for x in (beta, alfaY, alfaR, piR, piY))
    return Q, np.array([float(x) for x in bf])


def table_of(header, name, count):
    """The `count` decimal literals of the array `name` in a data header of csrc/ (data only: there is no code in those files)."""
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "pagan2-msa_amd", "csrc", header)).read()
    body = text[text.index("%s[%d]" % (name, count)):]
    body = body[body.index("{") + 1:body.index("};")]
    body = re.sub(r"/\*.*?\*/|//[^\n]*", " ", body, flags=re.S)
    values = [float(x) for x in body.replace("\n", " ").split(",") if x.strip()]
    assert len(values) == count, (name, len(values))
    return np.array(values)


def model_rates(data_type, base_freq=None):
    if data_type == 1:
        return model_rates_dna(base_freq or (0.25, 0.25, 0.25, 0.25))
    if data_type == 2:
        return table_of("wag_data.h", "kWagQ", 400).reshape(20, 20), table_of("wag_data.h", "kWagPi", 20)
    return table_of("codon_data.h", "kCodonQ", 3721).reshape(61, 61), table_of("codon_data.h", "kCodonPi", 61)


def proper(Q, pi):
    """The header's rule: every exchange flow pi_i q_ij averaged with its mirror image, the diagonal minus the row's other entries."""
    flow = pi[:, None] * Q
    R = 0.5 * (flow + flow.T) / pi[:, None]
    np.fill_diagonal(R, 0.0)
    np.fill_diagonal(R, -R.sum(axis=1))
    return R


CASES_OF_RATES = [(1, None), (1, A.BASE_FREQ), (2, None), (3, None)]


@pytest.mark.parametrize("data_type,bf", CASES_OF_RATES)
def test_pmatrix_against_scipy_expm(data_type, bf):
    """scipy's expm of the model's rate matrix, made proper by the header's rule in numpy, against anc_pmatrix within 1e-9.  The
    rates come from outside the ancestral code (see above), so a rate scaled by 2, a dropped kappa or a wrong table fails here."""
    linalg = pytest.importorskip("scipy.linalg")
    Q, pi = model_rates(data_type, bf)
    R = proper(Q, pi)
    assert np.array_equal(host.anc_pmatrix(data_type, 0.1, bf)[1], pi)
    for t in (0.01, 0.2, 1.3):
        assert np.abs(linalg.expm(R * t) - host.anc_pmatrix(data_type, t, bf)[0]).max() <= 1e-9, t


@pytest.mark.parametrize("data_type,bf", CASES_OF_RATES)
def test_rate_matrix_is_the_models_made_proper(data_type, bf):
    """pagan_anc_rate_matrix against the same restatement, to rounding (six operations an entry, S entries a diagonal sum); it is a
    rate matrix, reversible under pi; and it moves no rate of the model by more than the model's own asymmetry
    |pi_i q_ij - pi_j q_ji| / (2 pi_i), which is what averaging a flow with its mirror image does."""
    Q, pi = model_rates(data_type, bf)
    R = proper(Q, pi)
    got, got_pi = host.anc_rate_matrix(data_type, bf)
    S = A.STATES[data_type]
    assert got.shape == (S, S) and np.array_equal(got_pi, pi)
    assert np.abs(got - R).max() <= 8 * S * 2.0 ** -53 * np.abs(R).max()
    off = got - np.diag(np.diag(got))
    assert np.all(off >= 0) and np.all(np.abs(got.sum(axis=1)) <= 4 * S * 2.0 ** -53 * np.abs(np.diag(got)))
    flow = pi[:, None] * got
    assert np.abs(flow - flow.T).max() <= 4 * 2.0 ** -53 * np.abs(flow).max()
    asym = np.abs(pi[:, None] * Q - (pi[:, None] * Q).T) / (2 * pi[:, None])
    moved = np.abs(off - (Q - np.diag(np.diag(Q))))
    assert np.all(moved <= asym + 4 * 2.0 ** -53 * np.abs(Q).max())
    assert _code(host.anc_rate_matrix, 0) == abi.PAGAN_E_ARG


def test_the_librarys_leaf_tables_are_the_readings():
    """pagan_anc_encode_row (the tables pa_encode reads on the device) against leaf_sets for every byte value a row can hold, both
    cases, and for every triplet over a ten-letter alphabet."""
    one = "".join(chr(c) for c in range(1, 128))
    for data_type in (1, 2):
        codes = host.anc_encode_row(data_type, one)
        sets = A.leaf_sets(one, data_type)
        assert len(codes) == 127
        for c, s in zip(codes, sets):
            if data_type == 1:
                assert int(c) == sum(1 << t for t in (s or ()))
            else:
                assert int(c) == (s[0] if s else 255)
    assert np.all(host.anc_encode_row(2, bytes(range(128, 256))) == 255) and np.all(host.anc_encode_row(1, bytes(range(128, 256))) == 0)
    letters = "ACGTUacgu-N"
    row = "".join(a + b + c for a in letters for b in letters for c in letters)
    codes = host.anc_encode_row(3, row)
    assert [int(c) for c in codes] == [s[0] if s else 255 for s in A.leaf_sets(row, 3)]
    assert len(set(int(c) for c in codes)) == 62                                    # all 61 sense codons, and missing
    assert _code(host.anc_encode_row, 3, "ACGT") == abi.PAGAN_E_ARG and _code(host.anc_encode_row, 0, "A") == abi.PAGAN_E_ARG


def test_pmatrix_refusals():
    assert _code(host.anc_pmatrix, 0, 0.1) == abi.PAGAN_E_ARG
    assert _code(host.anc_pmatrix, 4, 0.1) == abi.PAGAN_E_ARG
    assert _code(host.anc_pmatrix, 1, -0.1) == abi.PAGAN_E_ARG
    assert _code(host.anc_pmatrix, 2, float("inf")) == abi.PAGAN_E_ARG
    assert _code(host.anc_pmatrix, 3, float("nan")) == abi.PAGAN_E_ARG
    P, pi = host.anc_pmatrix(1, 0.1)                                               # no base_freq: a quarter each
    assert np.array_equal(pi, np.full(4, 0.25))


# ---- tree check, byte prediction ---------------------------------------------------------------------------------------------

def test_tree_validation():
    good = ([0, 2, 4], [1, 3, 5], [0.1, 0.0, 0.3, 0.2, 0.05, 0.5, 99.0])
    host.anc_check_tree(*good)
    host.anc_check_tree([0], [1], [0.1, 0.2, float("nan")])                        # the root's entry is ignored
    host.anc_check_tree(*A.caterpillar(50, 0.2))
    host.anc_check_tree([0, 2, 5], [1, 3, 4], good[2])                             # (4 and 5 in either order under the root)
    bad = [([0, 2, 6], [1, 3, 5], good[2]),                                        # the root as its own child
           ([0, 2, 4], [1, 3, 4], good[2]),                                        # a node used twice, node 5 never
           ([0, 0, 4], [1, 3, 5], good[2]),                                        # leaf 0 twice, leaf 2 never
           ([0, 2, -1], [1, 3, 5], good[2]),
           ([0, 4, 2], [1, 5, 3], good[2]),                                        # parents before children
           (good[0], good[1], [0.1, -0.01, 0.3, 0.2, 0.05, 0.5, 0.0]),
           (good[0], good[1], [0.1, 0.1, float("inf"), 0.2, 0.05, 0.5, 0.0]),
           (good[0], good[1], [0.1, 0.1, 0.3, 0.2, float("nan"), 0.5, 0.0])]
    for left, right, branch in bad:
        assert _code(host.anc_check_tree, left, right, branch) == host.PAGAN_E_TREE, (left, right, branch)
    rows = ["ACGT", "ACGA", "ACCT", "AGGT"]
    for left, right, branch in bad:                                                # the device entry refuses them before it asks for a device
        assert _code(host.anc_reconstruct, left, right, branch, rows, 1) == host.PAGAN_E_TREE


def test_reconstruct_refusals_come_before_any_device_is_asked_for():
    left, right, branch = [0, 2, 4], [1, 3, 5], [0.1] * 7
    rows = ["ACGT", "ACGA", "ACCT", "AGGT"]
    assert _code(host.anc_reconstruct, left, right, branch, ["ACGT", "ACG", "ACCT", "AGGT"], 1) == abi.PAGAN_E_ARG     # ragged
    assert _code(host.anc_reconstruct, left, right, branch, rows, 3) == abi.PAGAN_E_ARG       # codons: 4 is no multiple of 3
    assert _code(host.anc_reconstruct, left, right, branch, rows, 7) == abi.PAGAN_E_ARG
    assert _code(host.anc_reconstruct, left, right, branch, rows, 1, None, [3]) == abi.PAGAN_E_ARG      # a leaf's posterior
    assert _code(host.anc_reconstruct, left, right, branch, rows, 1, None, [7]) == abi.PAGAN_E_ARG
    assert _code(host.anc_reconstruct, left, right, branch, rows, 1, None, [4, 4]) == abi.PAGAN_E_ARG   # listed twice


def test_predict_bytes_is_monotone_in_every_argument():
    base = host.anc_predict_bytes(8, 1000, 1, 256)
    assert base > 0
    for n in (9, 16, 100):
        assert host.anc_predict_bytes(n, 1000, 1, 256) > base
    assert host.anc_predict_bytes(8, 1000, 1, 256) < host.anc_predict_bytes(8, 1000, 2, 256) < host.anc_predict_bytes(8, 1000, 3, 256)
    sizes = [host.anc_predict_bytes(8, 1000, 1, c) for c in (1, 64, 65, 128, 512, 960, 1024, 4096)]
    assert sizes == sorted(sizes) and sizes[0] == sizes[1] < sizes[2] == sizes[3] and sizes[-1] == sizes[-2]    # chunks are whole waves, at most the alignment
    cols = [host.anc_predict_bytes(8, L, 1, 1 << 20) for L in (0, 1, 64, 65, 1000, 100000)]
    assert cols == sorted(cols) and cols[0] == cols[1] == cols[2] < cols[3]
    # the partials and the outside vectors are most of it: 2 (n - 1) S doubles a column
    assert host.anc_predict_bytes(8, 1024, 3, 1024) >= 2 * 7 * 61 * 8 * 1024
    assert _code(host.anc_predict_bytes, 1, 10, 1) == abi.PAGAN_E_ARG
    assert _code(host.anc_predict_bytes, 8, -1, 1) == abi.PAGAN_E_ARG
    assert _code(host.anc_predict_bytes, 8, 1 << 31, 1) == abi.PAGAN_E_ARG
    assert _code(host.anc_predict_bytes, 8, 10, 0) == abi.PAGAN_E_ARG


# ---- exports, no device ------------------------------------------------------------------------------------------------------

def test_the_new_symbols_are_exported(pg):
    lib = pg.lib()
    for sym in ("pagan_anc_pmatrix", "pagan_anc_rate_matrix", "pagan_anc_encode_row", "pagan_anc_check_tree", "pagan_anc_predict_bytes", "pagan_anc_reconstruct", "pagan_msa_ancestral",
                "pagan_msa_ancestral_row", "pagan_msa_ancestral_support", "pagan_msa_write_fasta_ancestral", "pagan_msa_ancestral_best"):
        assert sym in host.HOST_EXPORTED
        getattr(lib, sym)


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


def test_without_a_device_the_device_entries_say_so(pg, oracle, tmp_path):
    tn, ts, nwk = synth.evolve_balanced(4, 60, branch=0.03, sub=0.03, indel_start=0.01, mean_len=3, seed=12)
    msa = host.Msa(tn, ts, nwk, use_anchors=0)
    assert _code(msa.ancestral) == abi.PAGAN_E_ARG                                 # before the rows exist
    msa.set_batch_backend(_oracle_backend(oracle))                                 # aligned through the test seam: its rows exist without a device
    msa.align()
    before = msa.alignment_all()
    c = A.case("edge:65")
    if pg.device_count() > 0:                                                      # (on a GPU machine: the same calls work)
        assert host.anc_reconstruct(c["left"], c["right"], c["branch"], c["rows"], 1, c["base_freq"])["info"]["columns"] == 65
        assert msa.ancestral().row(0) == before[0]
    else:
        assert _code(host.anc_reconstruct, c["left"], c["right"], c["branch"], c["rows"], 1, c["base_freq"]) == abi.PAGAN_E_NODEVICE
        assert _code(host.anc_reconstruct, [0], [1], [0.1, 0.1, 0.0], ["", ""], 1) == abi.PAGAN_E_NODEVICE    # nothing to do is still no host path
        assert _code(msa.ancestral) == abi.PAGAN_E_NODEVICE
        L = msa._L                                                                 # nothing was kept: the readers refuse
        assert L.pagan_msa_ancestral_row(msa._h, 4, C.create_string_buffer(1000)) == abi.PAGAN_E_ARG
        assert L.pagan_msa_write_fasta_ancestral(msa._h, str(tmp_path / "a.fas").encode(), 60) == abi.PAGAN_E_ARG
    assert msa.alignment_all() == before
