"""A second reading, in plain Python, of how the segmented traceback cuts a path (dp_kernels.hip: pg_trace_spec,
pg_trace_compose; dp_plan.cpp, validate_job: how many boundaries a job gets).  Restated from the code, never calling it:
given the cells a path visits and the width of every anti-diagonal, `plan` says which segments pg_trace_compose must
record, which cells one lane walks serially, and which exit every table entry on the path took.

    boundaries    diagonal pairs {k*SEG, k*SEG - 1}, k = 1 .. K, K = (nd - 1) // SEG with nd = Lx + Ly - 1; K = 0 when
                  Lx + Ly < SERIAL_MIN or (table entries / 3) * SEG > SPEC_FACTOR * (Lx + Ly)
    a table entry the chase from a (cell, state) of pair k: stops at the first cell on pair k - 1 (EXIT "entry"); a move
                  that lands below that pair is followed to the pair it lands on or above (narrow boundary: at most
                  FOLLOW_ENTRIES entries on pair k) or given up (EXIT "miss_wide"); after CAP_SEGS * SEG cells it is
                  given up (EXIT "miss_cap"); the start cell ends it (EXIT "done")
    compose       from the end cell: a node on a pair takes its entry (one segment), any other node is walked serially

The module-level constants are the kernels'; the hand-worked tests shrink SEG."""
import numpy as np

SEG = 256                   # PG_SEG
FOLLOW_ENTRIES = 3 * 512    # pg_trace_spec: follow = n_entries <= 3 * 512
CAP_SEGS = 2                # pg_trace_spec: steps >= 2 * PG_SEG
SERIAL_MIN = 2000           # validate_job: serial < 2000
SPEC_FACTOR = 20000         # validate_job: speculative > 20000 * serial

ENTRY, MISS_WIDE, MISS_CAP, DONE = "entry", "miss_wide", "miss_cap", "done"
X_MAT, Y_MAT, M_MAT = 0, 1, 2


def diagonal_widths(Lx, Ly, band=None):
    """Cells of every anti-diagonal d = 0 .. Lx + Ly - 2 (<= 0: none) of the full matrix or of a row band given as
    (upper, lower) column bounds per row, clamped as the library clamps them (dp_band.h)."""
    nd = Lx + Ly - 1
    lo = np.zeros(Lx, np.int64)
    hi = np.full(Lx, Ly - 1, np.int64)
    if band is not None:
        lo = np.maximum(np.asarray(band[0], np.int64)[:Lx], 0)
        hi = np.minimum(np.asarray(band[1], np.int64)[:Lx], Ly - 1)
    rows = np.arange(Lx)
    d = np.arange(nd)
    # imax[d] = max{i: lo[i] + i <= d}, imin[d] = min{i: hi[i] + i >= d}; both keys rise strictly with i
    imax = np.searchsorted(lo + rows, d, side="right") - 1
    imin = np.searchsorted(hi + rows, d, side="left")
    return (imax - imin + 1).astype(np.int64)


def table_entries(widths, K):
    return sum(3 * (max(int(widths[k * SEG]), 0) + max(int(widths[k * SEG - 1]), 0)) for k in range(1, K + 1))


def n_boundaries(Lx, Ly, widths):
    """validate_job's decision: the number of boundary pairs the job's traceback is cut at."""
    nd = Lx + Ly - 1
    K = (nd - 1) // SEG
    serial = Lx + Ly
    speculative = table_entries(widths, K) // 3 * SEG
    if serial < SERIAL_MIN or speculative > SPEC_FACTOR * serial:
        return 0
    return K


def boundary_of(d, K):
    if d <= 0:
        return 0
    k = d // SEG if d % SEG == 0 else ((d + 1) // SEG if (d + 1) % SEG == 0 else 0)
    return k if 1 <= k <= K else 0


def visited_cells(result):
    """The cells (i, j, state) a result's path visits, end -> start: its columns of kinds 2 (M), 3 (X), 4 (Y), each with
    the coordinate a gap column leaves out carried along from the columns before it (skip columns 5 / 6 move a
    coordinate and visit nothing)."""
    cells = []
    i = j = 0
    for left, right, kind in np.asarray(result.cols).tolist():
        if kind in (2, 3, 5):
            i = left
        if kind in (2, 4, 6):
            j = right
        if kind == 2:
            cells.append((i, j, M_MAT))
        elif kind == 3:
            cells.append((i, j, X_MAT))
        elif kind == 4:
            cells.append((i, j, Y_MAT))
    cells.reverse()
    out = np.array(cells, np.int32).reshape(-1, 3)
    if len(out):
        assert tuple(int(v) for v in out[0]) == (result.end[1], result.end[2], result.end[0]), "the first visited cell is the end cell"
    return out


def _chase(cells, t, K, widths):
    """pg_trace_spec's loop for the entry of visited cell t (on pair k): (cells walked, exit kind, pairs followed over)."""
    n = len(cells)
    k = boundary_of(int(cells[t][0] + cells[t][1]), K)
    D = k * SEG
    n_entries = 3 * (max(int(widths[D]), 0) + max(int(widths[D - 1]), 0))
    follow = n_entries <= FOLLOW_ENTRIES
    kb, low = k - 1, (k - 1) * SEG
    steps, u, followed = 0, t, 0
    while True:
        if u == n:                                      # the node is the start cell
            return steps, DONE, followed
        dd = int(cells[u][0] + cells[u][1])
        if steps > 0 and kb >= 1 and dd <= low:
            if dd >= low - 1:
                return steps, ENTRY, followed
            if not follow:
                return steps, MISS_WIDE, followed
            while kb >= 1 and dd < low - 1:
                kb -= 1
                low -= SEG
                followed += 1
            if kb >= 1 and dd <= low:
                return steps, ENTRY, followed
        if steps >= CAP_SEGS * SEG:
            return steps, MISS_CAP, followed
        u += 1
        steps += 1


def plan(cells, widths, K):
    """What pg_trace_compose records for a path: dict of
        segments  [(i, j, state, cells, offset)] in the order composed (the start cell of each lies on a boundary pair)
        serial    offsets of the cells walked one by one
        hops      per segment (boundary k, exit kind, pairs followed over)
        n_cells   cells of the path."""
    cells = np.asarray(cells).reshape(-1, 3)
    n = len(cells)
    t, segments, serial, hops = 0, [], [], []
    while t < n:
        i, j, s = (int(v) for v in cells[t])
        k = boundary_of(i + j, K)
        if k > 0:
            steps, kind, followed = _chase(cells, t, K, widths)
            assert steps > 0
            segments.append((i, j, s, steps, t))
            hops.append((k, kind, followed))
            t += steps
        else:
            serial.append(t)
            t += 1
    assert len(segments) <= 2 * K + 8, "pg_trace_compose's segment array"
    return {"segments": segments, "serial": serial, "hops": hops, "n_cells": n}


def pairs_passed_without_a_cell(cells, K):
    """Boundary pairs below the end cell that the path has no cell on: a long edge carried it over."""
    cells = np.asarray(cells).reshape(-1, 3)
    if not len(cells):
        return []
    d = set(int(v) for v in cells[:, 0] + cells[:, 1])
    top = int(cells[0][0] + cells[0][1])
    return [k for k in range(1, K + 1) if k * SEG - 1 <= top and k * SEG not in d and k * SEG - 1 not in d]
