"""A second reading of posterior decoding (maximum expected accuracy paths), in plain Python (test infrastructure).

The device fills a score matrix diagonal by diagonal over job records and edge lists (dp_fb_decode.inc).  This file takes the
definition from the other end: the cells and transitions are the arc lists of a pycheck_fb.Exact -- arcs_into() for a cell's
predecessors, end_forward for the end corner's terms, inside() for the band -- and the arithmetic is Python floats over a
posterior table the caller gives.

  * weight(s, i, j) = posterior * (1 for a match, g for a gap state);
  * A(M, 0, 0) = 0; elsewhere A(cell) = weight + max over the arcs into the cell whose own weight is above 0 and whose source has a
    finite A, in the arcs' order, strict > (the first maximum stays); -inf without such an arc or outside the band;
  * the optimum: the same maximum over the end terms; the path: the cells' own maxima repeated back to the start corner.

brute_force() does not fill anything: it lists every path from the start corner to an end term and takes the best sum.

Nothing under pagan2-msa_amd/ may import this file.
"""
import numpy as np

import pycheck_fb
from pycheck_fb import X, Y, M

NINF = float("-inf")


def exact_arcs(left, right, mp, band=None):
    """a pycheck_fb.Exact for its arc listings alone (arcs_into, end_forward, inside), without the path sums its constructor
    takes in 50-digit decimals: for pairs whose posteriors come from elsewhere"""
    ex = pycheck_fb.Exact.__new__(pycheck_fb.Exact)
    ex.L, ex.R = pycheck_fb._Side(left), pycheck_fb._Side(right)
    ex.Lx, ex.Ly = ex.L.n - 1, ex.R.n - 1
    ex.ext, ex.open, ex.ng = (pycheck_fb._promote(v) for v in (mp.gap_ext, mp.gap_open, mp.non_gap))
    ex.close = pycheck_fb.ONE
    ex._score, ex._emit = mp.score, {}
    if band is None:
        ex.lo, ex.hi = [0] * ex.Lx, [ex.Ly - 1] * ex.Lx
    else:
        ex.lo = [max(0, int(v)) for v in band.upper]
        ex.hi = [min(int(v), ex.Ly - 1) for v in band.lower]
    ex._mul = pycheck_fb._ctx.multiply
    ex._end_terms()
    return ex


def weights(post, g):
    w = np.array(post, np.float64, copy=True)
    w[:, :, X] *= g
    w[:, :, Y] *= g
    return w


def _arcs(ex, cell):
    """the arcs into `cell` that are transitions: weight above 0, source inside the band"""
    return [(pred, wt) for pred, wt in ex.arcs_into(cell) if wt > 0 and ex.inside(pred[0], pred[1])]


def _ends(ex):
    return [(cell, wt) for cell, wt in ex.end_forward if wt > 0 and ex.inside(cell[0], cell[1])]


class Mea:
    """A, the optimum and the path of one pair.  post: [Lx, Ly, 3] posteriors (X, Y, M); g: the gap weight.
    status 0 decoded / 1 no end term is reachable; objective; end = (state, i, j); visited: rows (i, j, state) end -> start
    without the start corner."""

    def __init__(self, ex, post, g):
        self.ex, self.g = ex, float(g)
        self.w = weights(post, g)
        Lx, Ly = ex.Lx, ex.Ly
        A = np.full((Lx, Ly, 3), NINF)
        back = {}
        for i in range(Lx):
            for j in range(ex.lo[i], ex.hi[i] + 1):             # (row by row: every arc comes from a smaller row or column)
                for s in (X, Y, M):
                    if i == 0 and j == 0:
                        if s == M:
                            A[0, 0, M] = 0.0
                        continue
                    best, arg = NINF, None
                    for pred, _wt in _arcs(ex, (i, j, s)):
                        a = A[pred[0], pred[1], pred[2]]
                        if a > best:
                            best, arg = a, pred
                    if arg is not None:
                        A[i, j, s] = self.w[i, j, s] + best
                        back[(i, j, s)] = arg
        self.A = A
        best, arg = NINF, None
        for cell, _wt in _ends(ex):
            a = A[cell[0], cell[1], cell[2]]
            if a > best:
                best, arg = a, cell
        self.visited = np.zeros((0, 3), np.int32)
        if arg is None:
            self.status, self.objective, self.end = 1, 0.0, None
            return
        self.status, self.objective, self.end = 0, float(best), (arg[2], arg[0], arg[1])
        rows, cell = [], arg
        while cell != (0, 0, M):
            rows.append(cell)
            cell = back[cell]
        self.visited = np.array(rows, np.int32).reshape(-1, 3)


def objective_of(w, visited):
    """the sum of the weights `w` ([Lx, Ly, 3], from weights()) along any path (rows (i, j, state))"""
    return float(sum(w[int(i), int(j), int(s)] for i, j, s in visited))


def is_path(ex, visited, end):
    """every step of `visited` (rows (i, j, state), end -> start, no start corner) is an arc of arcs_into, the first cell is the
    end pick `end` = (state, i, j), the pick is an end_forward term, and the last step leaves the start corner"""
    cells = [(int(i), int(j), int(s)) for i, j, s in visited]
    first = (int(end[1]), int(end[2]), int(end[0]))
    if first not in [c for c, _ in _ends(ex)]:
        return False
    if not cells:
        return first == (0, 0, M)
    if cells[0] != first:
        return False
    chain = cells + [(0, 0, M)]
    for t in range(len(chain) - 1):
        if chain[t + 1] not in [p for p, _ in _arcs(ex, chain[t])]:
            return False
    return True


def brute_force(ex, post, g, limit=2000000):
    """(best objective or None when no path exists, number of paths): every start -> end path listed one by one"""
    w = weights(post, g)
    best, count = [None], [0]

    def walk(cell, total):
        if cell == (0, 0, M):
            count[0] += 1
            if count[0] > limit:
                raise RuntimeError("more than %d paths: not a tiny pair" % limit)
            if best[0] is None or total > best[0]:
                best[0] = total
            return
        for pred, _wt in _arcs(ex, cell):
            walk(pred, total + w[cell[0], cell[1], cell[2]])

    for cell, _wt in _ends(ex):
        walk(cell, 0.0)
    return best[0], count[0]
