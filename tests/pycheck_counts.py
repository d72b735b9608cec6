"""The exact expected transition, end and emission counts of one pair (test infrastructure), from pycheck_fb.Exact's path sums.

An interior arc pred -> cell of weight w (Exact.arcs_into: one term of the forward recurrence) is taken by the paths that reach
pred, take it and go on from cell to the end: its expected count is prefix(pred) * w * suffix(cell) / fwd_total, with the suffix
the backward pass's (every end transition once: what B holds).  The end transitions are the terms of the forward end corner
(Exact.end_forward), each as often as that corner lists it: prefix(cell) * w / fwd_total.  An emission count is the posterior
prefix * suffix / fwd_total of an M cell with i, j >= 1, added at (state_left[i], state_right[j]).  Sums are taken in 50-digit
decimals and rounded once.  A pair whose forward total is 0 has every count 0.

Nothing under pagan2-msa_amd/ may import this file.
"""
import numpy as np

import pycheck_fb
from pycheck_fb import M, ZERO, _ctx


def counts(ex, n_states=None):
    """ex: pycheck_fb.Exact.  Returns {"trans": [3, 3] float64 (from, to), "end": [3] (X-close, Y-close, M-end),
    "emit": [S, S] (left state, right state; None without n_states), "into": [Lx, Ly, 3] the arcs into every cell summed}."""
    trans = [[ZERO] * 3 for _ in range(3)]
    end = [ZERO] * 3
    emit = [[ZERO] * n_states for _ in range(n_states)] if n_states else None
    into = np.zeros((ex.Lx, ex.Ly, 3))
    tot = ex.fwd_total
    if tot:
        add, mul, div = _ctx.add, _ctx.multiply, _ctx.divide
        with ex._deep():
            for i in range(ex.Lx):
                for j in range(ex.lo[i], ex.hi[i] + 1):
                    for s in range(3):
                        cell = (i, j, s)
                        suf = ex.suffix(cell)
                        if not suf:
                            continue
                        here = ZERO
                        for pred, w in ex.arcs_into(cell):
                            pv = ex.prefix(pred)
                            if pv:
                                xi = div(mul(mul(pv, w), suf), tot)
                                trans[pred[2]][s] = add(trans[pred[2]][s], xi)
                                here = add(here, xi)
                        into[i, j, s] = float(here)
                        if emit is not None and s == M and i >= 1 and j >= 1:
                            a, b = ex.L.state[i], ex.R.state[j]
                            emit[a][b] = add(emit[a][b], div(mul(ex.prefix(cell), suf), tot))
            for cell, w in ex.end_forward:
                end[cell[2]] = add(end[cell[2]], div(mul(ex.prefix(cell), w), tot))
    f = lambda rows: np.array([[float(v) for v in r] for r in rows], np.float64)
    return {"trans": f(trans), "end": f([end])[0], "emit": f(emit) if emit is not None else None, "into": into}


def run(left, right, mp, band=None, emissions=True):
    """the counts of a pair and its Exact object"""
    ex = pycheck_fb.Exact(left, right, mp, band)
    out = counts(ex, mp.n_states if emissions else None)
    out["exact"] = ex
    return out


def gradient_sums(c):
    """the count sums that are the derivatives of log_fwd by log gap_ext, log gap_open, log non_gap"""
    t, e = c["trans"], c["end"]
    X, Y = pycheck_fb.X, pycheck_fb.Y
    return {"ext": t[X, X] + t[Y, Y],
            "open": t[Y, X] + t[M, X] + t[X, Y] + t[M, Y],
            "ng": t[M, X] + t[M, Y] + 2 * t[M, M] + t[X, M] + t[Y, M] + e[2]}
