"""The float64 reading in the header's order (tests/pycheck_anc_fp64.py) against the 50-digit readings (tests/pycheck_anc.py,
tests/pycheck_brlen.py), no GPU: on every case tests/test_anc_bytes_gpu.py compares as bytes, within the bounds those readings
already come with -- pycheck_anc.tolerance for likelihoods and posteriors (taken as tests/test_anc_gpu.py takes it),
pycheck_brlen.tolerances for g1 and g2.  No tolerance is new.  has_data, informative and col_exp are equal; `best` is compared
where pycheck_anc.decided says the column is decided.  This is what makes the byte comparison mean something: bytes equal to a
reading that is wrong would prove nothing.

col_exp has no counterpart among the 50-digit readings' outputs, but it follows from them (pycheck_anc.exponents): the rescaling
is by exact powers of two, so the exponents below a node add up to the binary exponent of its unscaled partial's largest entry."""
from decimal import Decimal

import numpy as np
import pytest

import pycheck_anc as A
import pycheck_anc_fp64 as F
import pycheck_brlen as B

CASES = list(A.POSTERIOR_CASES) + [name for name in B.DERIV_CASES if name not in A.POSTERIOR_CASES]


def check_passes(c, want, got):
    """col_lik 2^col_exp, col_exp, has_data, post, best, best_p against a pycheck_anc reading; returns the worst error over its bound."""
    S = A.STATES[c["data_type"]]
    tol = A.tolerance(c["left"], c["right"], S)
    n, L = len(c["rows"]), len(want["lik"])
    assert got["col_lik"].shape == (L,) and got["post"].shape == (n - 1, L, S)
    assert np.array_equal(got["has_data"], want["has_data"])
    worst = 0.0
    for col in range(L):
        lik = Decimal(float(got["col_lik"][col])) * Decimal(2) ** int(got["col_exp"][col])
        assert abs(lik - want["lik"][col]) <= Decimal(tol) * want["lik"][col], (col, lik, want["lik"][col])
        if want["lik"][col] > 0:
            worst = max(worst, float(abs(lik - want["lik"][col]) / want["lik"][col]) / tol)
    tops = want if "top" in want else A.pruning(c["left"], c["right"], c["branch"], c["rows"], c["data_type"], c["base_freq"], down=False)
    expo, safe = A.exponents(c["left"], c["right"], tops, tol)
    # where a largest entry lies within tol of a power of two (rows of P sum to 1 only to a few 1e-15, so the message of an N does),
    # the exponent is the rounding's to choose and col_lik 2^col_exp above is the check: a condition on the case, as `decided` is
    assert sum(safe) >= 0.9 * L or L < 10
    assert [int(e) for e, ok in zip(got["col_exp"], safe) if ok] == [e for e, ok in zip(expo, safe) if ok]
    if want["post"] is None:
        return worst
    for k in range(n - 1):
        for col in range(L):
            w = want["post"][k][col]
            for s in range(S):
                err = abs(Decimal(float(got["post"][k, col, s])) - w[s])
                assert err <= Decimal(2 * tol), (k, col, s)
                worst = max(worst, float(err) / (2 * tol))
            s, p = A.best_of(w)
            if A.decided(w, tol):
                assert got["best"][k, col] == s, (k, col)
                assert abs(float(got["best_p"][k, col]) - float(p)) <= 2 * tol + 2.0 ** -24 * float(p), (k, col)
            elif sum(w) == 0:                                        # a column that cannot happen: state 0 with best_p 0, and zeros
                assert got["best"][k, col] == 0 and got["best_p"][k, col] == 0 and not got["post"][k, col].any()
    return worst


def check_sums(c, want, got):
    """g1, g2, informative against pycheck_brlen.evaluate's; returns the worst errors over their bounds."""
    n = len(c["rows"])
    assert [int(x) for x in got["informative"]] == want["informative"]
    t1, t2 = B.tolerances(want, len(want["lik"]))
    worst = [0.0, 0.0]
    for v in range(2 * n - 1):
        e1, e2 = abs(float(got["g1"][v]) - float(want["g1"][v])), abs(float(got["g2"][v]) - float(want["g2"][v]))
        assert e1 <= t1[v] and e2 <= t2[v], (v, e1, t1[v], e2, t2[v])
        if want["informative"][v] == 0:
            assert got["g1"][v] == 0 and got["g2"][v] == 0           # the exact 0
        else:
            worst = [max(worst[0], e1 / t1[v]), max(worst[1], e2 / t2[v])]
    return worst


@pytest.mark.parametrize("name", CASES)
def test_the_fp64_reading_against_the_fifty_digit_readings(name):
    c = B.case(name)
    got = F.of_case(c)
    if name in A.POSTERIOR_CASES:
        want = A.case(name)["reading"]
    else:                                                            # the likelihoods come with the branch sums' reading
        want = dict(c["brlen"], post=None)
    worst = check_passes(c, want, got)
    line = "%s: largest error over its bound: passes %.3g" % (name, worst)
    if name in B.DERIV_CASES:
        line += ", g1 %.3g, g2 %.3g" % tuple(check_sums(c, c["brlen"], got))
    print(line)


def test_the_passes_alone_are_the_same_bytes():
    """derivs=False (what a case without branch sums is read with) leaves the passes' outputs as they are."""
    c = A.case("protein")
    a, b = F.of_case(c), F.of_case(c, derivs=False)
    assert all(a[k].tobytes() == b[k].tobytes() for k in b) and "g1" not in b


def test_the_column_sum_is_the_headers_tree():
    """On 130 columns by hand: 1e16 in column 0 swallows a 1.0 added to it directly, so the order shows.  The tree adds column 32
    to column 0 first; columns 64 .. 127 are block 1, 128 and 129 block 2, and the blocks join left to right."""
    x = np.zeros(130)
    x[0], x[1], x[32], x[33] = 1e16, 1.0, 1.0, 1.0
    # d = 32: x[0] = 1e16 + 1 = 1e16 (rounded), x[1] = 2; d = 1: 1e16 + 2
    assert F.column_sum(x) == 1e16 + 2.0 and (1e16 + 1.0) + 1.0 + 1.0 == 1e16
    x[64], x[129] = 1.0, 1.0                                         # block 1 adds 1.0 to 1e16 + 2: rounds to even, 1e16 + 4; block 2 likewise
    assert F.column_sum(x) == ((1e16 + 2.0) + 1.0) + 1.0
    assert F.column_sum(np.array([0.5])) == 0.5 and F.column_sum(np.zeros(0)) == 0.0
