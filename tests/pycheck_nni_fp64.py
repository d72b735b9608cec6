"""The float64 reading of "tree search by nearest-neighbour interchange" (include/pagan_host.h) in the header's own order of
operations, in the manner of tests/pycheck_anc_fp64.py and on that file's helpers, so that the device's M, E and degenerate can be
held to it byte for byte (tests/test_nni_gpu.py).  tests/test_nni_cpu.py holds it to the 50-digit reading of pycheck_nni.py first.

The up and the down loop are restated here, because pycheck_anc_fp64.reading does not return the partials and the outside vectors.
From the library it takes P and pi (host.anc_pmatrix: host only) and nothing else; the candidates, the swap, the selection and the
search loop are pycheck_nni's (plain Python, no arithmetic to round).

reading() returns a dict, row k for internal node n + k:
  kind [n - 1] int32; M, gain [n - 1, 2] float64; E, degenerate [n - 1, 2] int64     ((0.5, 1), 0 and 0 where there is no candidate)
  col_lik [L], col_exp [L], loglik                                                  the up pass's, loglik summed as the library sums it"""
import math

import numpy as np

from pagan2_msa_amd import host

import pycheck_anc as A
import pycheck_anc_fp64 as F
import pycheck_nni as N

LN2 = math.log(2.0)


def passes(left, right, branch, rows, data_type, base_freq=None, mid_t=None):
    """The two passes in the header's order.  Returns (msg, outs, pi, mats, col_lik, col_exp): msg(child) the child's message
    [S, L], outs {internal node: O [S, L]}, mats {length: P}."""
    n, S = len(rows), A.STATES[data_type]
    root = 2 * n - 2
    lengths = set(float(b) for b in branch[:-1])
    if mid_t is not None:
        lengths.add(float(mid_t))
    mats, pi = {}, None
    for t in lengths:
        P, pi = host.anc_pmatrix(data_type, t, base_freq)
        mats[t] = np.asarray(P, np.float64)
    pi = np.asarray(pi, np.float64)
    part, leaf_has = F._leaf_vectors(rows, data_type, S)
    L = part[0].shape[1]
    has = np.zeros((2 * n - 1, L), bool)
    has[:n] = leaf_has
    message = {}

    def msg(child):
        if child not in message:
            m = F._times(mats[float(branch[child])], part[child])
            m[:, ~has[child]] = 1.0
            message[child] = m
        return message[child]

    col_exp = np.zeros(L, np.int32)
    for k in range(n - 1):
        has[n + k] = has[left[k]] | has[right[k]]
        v, e = F._rescaled(msg(left[k]) * msg(right[k]), has[n + k])
        part.append(v)
        col_exp = col_exp + e
    col_lik = np.where(has[root], F._sum_over_states(pi[:, None] * part[root]), 1.0)
    outs = {root: np.repeat(pi[:, None], L, axis=1)}
    every = np.ones(L, bool)
    for k in range(n - 2, -1, -1):
        v = n + k
        for c, b in ((left[k], right[k]), (right[k], left[k])):
            if c >= n:
                outs[c], _ = F._rescaled(F._times_from_the_left(outs[v] * msg(b), mats[float(branch[c])]), every)
    msg.has = has
    return msg, outs, pi, mats, col_lik, col_exp.astype(np.int32)


def loglik_of(col_lik, col_exp):
    """log(col_lik) + col_exp * ln 2, column by column, added left to right: the library's sum on the host."""
    total = 0.0
    for x, e in zip(col_lik, col_exp):
        total += (math.log(x) if x > 0 else -math.inf) + int(e) * LN2
    return total


def column_product(r):
    """The header's column product of the ratios r [L]: (M, E)."""
    L = len(r)
    blocks = (L + 63) // 64
    x = np.ones(blocks * 64, np.float64)
    x[:L] = r
    m, e = np.frexp(x)
    m, e = m.reshape(blocks, 64), e.astype(np.int64).reshape(blocks, 64)
    d = 32
    while d >= 1:
        prod, de = np.frexp(m[:, :d] * m[:, d:2 * d])
        e[:, :d] = e[:, :d] + e[:, d:2 * d] + de
        m[:, :d] = prod
        d //= 2
    M, E = np.float64(0.5), 1
    for q in range(blocks):
        M, de = np.frexp(M * m[q, 0])
        E = E + int(e[q, 0]) + int(de)
    return float(M), int(E)


def candidate_sums(c, msg, outs, pi, mats, branch):
    """f_0, f_1, f_2 [L] of one candidate (pycheck_nni.candidates' dict), in the header's order."""
    ma, md, mb = msg(c["a"]), msg(c["d"]), msg(c["b"])
    if c["kind"] == 2:
        T = pi[:, None] * msg(c["e"])
        P_mid = mats[float(branch[c["c"]] + branch[c["rr"]])]
    else:
        T = outs[c["v"]]
        P_mid = mats[float(branch[c["c"]])]
    u = (ma * md, mb * md, ma * mb)
    X = (mb, ma, md)
    ha, hd, hb = msg.has[c["a"]], msg.has[c["d"]], msg.has[c["b"]]
    pair_has = (ha | hd, hb | hd, ha | hb)
    f = []
    for k in range(3):
        y = F._times(P_mid, u[k])
        y[:, ~pair_has[k]] = 1.0                         # a pair without data is a node without data: the exact 1
        f.append(F._sum_over_states((T * X[k]) * y))
    return f


def reading(left, right, branch, rows, data_type, base_freq=None):
    n = len(rows)
    kind, _ = N.kinds(left, right)
    cands = N.candidates(left, right)
    mid_t = None
    for c in cands:
        if c["kind"] == 2:
            mid_t = branch[c["c"]] + branch[c["rr"]]
    msg, outs, pi, mats, col_lik, col_exp = passes(left, right, branch, rows, data_type, base_freq, mid_t)
    M, gain = np.full((n - 1, 2), 0.5, np.float64), np.zeros((n - 1, 2), np.float64)
    E, deg = np.ones((n - 1, 2), np.int64), np.zeros((n - 1, 2), np.int64)
    for c in cands:
        f = candidate_sums(c, msg, outs, pi, mats, branch)
        for k in (1, 2):
            good = (f[0] > 0) & (f[k] > 0)
            with np.errstate(divide="ignore", invalid="ignore"):
                r = np.where(good, f[k] / f[0], 1.0)
            q = c["c"] - n
            M[q, k - 1], E[q, k - 1] = column_product(r)
            deg[q, k - 1] = int(np.count_nonzero(~good))
            gain[q, k - 1] = (math.log(M[q, k - 1]) if M[q, k - 1] > 0 else -math.inf) + int(E[q, k - 1]) * LN2
    return {"kind": np.asarray(kind, np.int32), "M": M, "E": E, "gain": gain, "degenerate": deg, "col_lik": col_lik, "col_exp": col_exp,
            "loglik": loglik_of(col_lik, col_exp)}


def of_case(c):
    return reading(c["left"], c["right"], c["branch"], c["rows"], c["data_type"], c["base_freq"])


def loglik(left, right, branch, rows, data_type, base_freq=None):
    """The up pass alone: the library's loglik of the tree."""
    _, _, _, _, col_lik, col_exp = passes(left, right, branch, rows, data_type, base_freq)
    return loglik_of(col_lik, col_exp)


def search(left, right, branch, rows, data_type, base_freq=None, min_gain=1e-3, max_rounds=32):
    """pycheck_nni.search (fit_rounds = 0) on this reading's gains and logliks: the replay the device's search is held to."""
    return N.search(left, right, branch, min_gain, max_rounds,
                    gains=lambda l, r, b: (lambda x: (x["gain"], x["degenerate"]))(reading(l, r, b, rows, data_type, base_freq)),
                    loglik=lambda l, r, b: loglik(l, r, b, rows, data_type, base_freq))
