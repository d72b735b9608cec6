"""pa_up, pa_down, pa_branch and pa_branch_fold (csrc/dp_anc.hip, csrc/dp_anc_brlen.inc) byte for byte against the float64 reading
in the header's order (tests/pycheck_anc_fp64.py, which tests/test_anc_fp64_cpu.py holds to the 50-digit readings first):
include/pagan_host.h fixes the order of every sum, the rescaling and the quotients, so the device's outputs are one sequence of
fp64 operations and nothing here has a tolerance.  No cell, column or case is left out.  loglik and col_loglik are: they pass
through the host's log, and tests/test_anc_gpu.py and tests/test_brlen_gpu.py pin them to one another.

Where bytes differ the assertion names the first place in the passes' own order -- col_exp, col_lik, the root's posterior, the
posteriors node by node downward, then g1 / g2 branch by branch -- and the first column and state there: that says which sum is
at fault ("Tests")."""
import numpy as np
import pytest

from pagan2_msa_amd import host

import pycheck_anc as A
import pycheck_anc_fp64 as F
import pycheck_brlen as B

pytestmark = pytest.mark.gpu

CASES = list(A.POSTERIOR_CASES) + [name for name in B.DERIV_CASES if name not in A.POSTERIOR_CASES]
_cases = {}


def case_of(name):
    """(the case without its 50-digit readings, which nothing here needs; the fp64 reading), made once."""
    if name not in _cases:
        c = B._named(name) or A.case(name)
        _cases[name] = (c, F.of_case(c))
    return _cases[name]


def first_difference(c, want, rec, der):
    """None, or a description of the first place where the device's bytes are not the reading's, in the passes' order."""
    n = len(c["rows"])

    def where(a, b):
        a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
        if a.shape != b.shape or a.dtype != b.dtype:
            return "shape or type: %s %s against %s %s" % (a.shape, a.dtype, b.shape, b.dtype)
        if a.tobytes() == b.tobytes():
            return None
        words = {8: np.uint64, 4: np.uint32, 1: np.uint8}[a.dtype.itemsize]
        at = np.argwhere(a.view(words) != b.view(words))[0]
        return "at %s: device %r, reading %r" % (tuple(int(i) for i in at), a[tuple(at)], b[tuple(at)])

    steps = [("has_data", rec["has_data"], want["has_data"]), ("col_exp", rec["col_exp"], want["col_exp"]),
             ("col_lik", rec["col_lik"], want["col_lik"])]
    for k in range(n - 2, -1, -1):                                   # the down pass: the root first
        steps += [("post of node %d (column, state)" % (n + k), rec["post"][k], want["post"][k]),
                  ("best of node %d" % (n + k), rec["best"][k], want["best"][k]),
                  ("best_p of node %d" % (n + k), rec["best_p"][k], want["best_p"][k])]
    if der is not None:
        steps.append(("informative (branch)", der["informative"], want["informative"]))
        for v in range(2 * n - 1):
            steps += [("g1 of branch %d" % v, der["g1"][v:v + 1], want["g1"][v:v + 1]),
                      ("g2 of branch %d" % v, der["g2"][v:v + 1], want["g2"][v:v + 1])]
    for what, a, b in steps:
        d = where(a, b)
        if d:
            return "%s %s" % (what, d)
    return None


def compare(name):
    c, want = case_of(name)
    n = len(c["rows"])
    args = (c["left"], c["right"], c["branch"], c["rows"], c["data_type"], c["base_freq"])
    rec = host.anc_reconstruct(*args, list(range(n, 2 * n - 1)))
    der = host.anc_branch_derivs(*args)
    assert rec["post"].shape == want["post"].shape and der["g1"].shape == want["g1"].shape
    first = first_difference(c, want, rec, der)
    assert first is None, "%s: %s" % (name, first)
    return rec, der


@pytest.mark.parametrize("name", CASES)
def test_the_passes_and_the_branch_sums_are_the_headers_operations(name):
    compare(name)


@pytest.mark.parametrize("name", ["eight:130", "chunks:protein", "codon:tree"])
def test_in_chunks_of_64_columns_as_well(name, monkeypatch):
    monkeypatch.setenv("PAGAN_ANC_CHUNK_COLS", "64")
    rec, der = compare(name)
    assert rec["info"]["chunk_cols"] == 64 == der["info"]["chunk_cols"]
    assert rec["info"]["chunks"] == der["info"]["chunks"] == (rec["info"]["columns"] + 63) // 64 > 1
