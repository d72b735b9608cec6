"""The stored Viterbi matrices of a device job against oracle.dp_matrices, cell for cell (a plain module: no fixtures).

  diag_index(Lx, Ly, band)                  where the device keeps every in-band cell (diagonal-major), from the band alone
  decode_words(words, left, right, i, j)    the device's back-pointer words in the oracle's terms
  check_matrices(batch, k, job, want, flags, compact=None)
                                            every score as a bit pattern, every pointer as integers, every in-band cell
  quantised(job, seed) / tie_counts(...)    inputs whose candidates tie exactly, and the condition such a job must meet

Nothing here carries a tolerance or leaves a cell, a state or a class out."""
import numpy as np

import pagan2_msa_amd as pg
from pagan2_msa_amd import abi
from pagan2_msa_amd.abi import _dp, _u32p

NAMES = "XYM"


def row_band(Lx, Ly, band):
    """(lo[Lx], hi[Lx]) clamped as the library (dp_band.h: RowBand) and the reference's Tunnel_matrix clamp them."""
    if band is None:
        return np.zeros(Lx, np.int64), np.full(Lx, Ly - 1, np.int64)
    return np.maximum(band.upper[:Lx].astype(np.int64), 0), np.minimum(band.lower[:Lx].astype(np.int64), Ly - 1)


def band_cells(Lx, Ly, band):
    """(i, j) of every in-band cell in row-major order -- the order of the oracle's arrays."""
    lo, hi = row_band(Lx, Ly, band)
    width = np.maximum(hi - lo + 1, 0)
    i = np.repeat(np.arange(Lx, dtype=np.int64), width)
    start = np.concatenate([[0], np.cumsum(width)])[:-1]
    j = np.arange(int(width.sum()), dtype=np.int64) - np.repeat(start, width) + np.repeat(lo, width)
    return i, j


def diag_index(Lx, Ly, band):
    """(i, j, pos): every in-band cell in row-major order and its position doff[d] + (i - imin[d]), d = i + j, in the device's
    diagonal-major arrays.  Computed from the band alone: a diagonal's cells are the in-band cells with i + j == d, imin[d] is
    the smallest row among them and doff[d] the number of cells on the diagonals before it (dp_device.h; for a monotone band
    the rows of a diagonal form one interval, which the permutation check below holds the band to)."""
    i, j = band_cells(Lx, Ly, band)
    d = i + j
    nd = Lx + Ly - 1
    count = np.bincount(d, minlength=nd)
    doff = np.concatenate([[0], np.cumsum(count)])[:-1]
    imin = np.full(nd, Lx, np.int64)
    np.minimum.at(imin, d, i)
    pos = doff[d] + (i - imin[d])
    seen = np.zeros(i.size, bool)
    assert pos.size == 0 or (pos.min() >= 0 and pos.max() < i.size), "a diagonal's in-band rows are not one interval"
    seen[pos] = True
    assert seen.all(), "a diagonal's in-band rows are not one interval"
    return i, j, pos


def decode_words(words, left, right, i, j):
    """Back-pointer words [n, 3] (X, Y, M) of the cells (i[n], j[n]) -> dict of int64 arrays [n, 3]: matrix, x_ind, y_ind,
    x_edge_ind, y_edge_ind as oracle.dp_matrices gives them, adjl / adjr (the two flag bits), and ok (False where an edge slot
    lies outside its site's list; the other fields are then those of slot 0).

    The layout is pack_bp's and cell_any_t's in csrc/dp_kcommon.h: word = from | ADJL (4) | ADJR (8) | k1 << 4 | k2 << 18 with
    from = 0 X, 1 Y, 2 M, 3 none; k1 / k2 count along the bwd lists of left site i / right site j.  State X consumes a left site
    and uses k1 only (its y_ind is j), state Y uses k2 only (its x_ind is i), state M uses both.  A cell without predecessor
    (from == 3) decodes to the oracle's untouched pointer: matrix -1, every index -1 but the gap states' own column / row.
    left / right need bwd_off, bwd_src and bwd_eid only."""
    w = words.astype(np.int64)
    n = w.shape[0]
    frm = w & 3
    none = frm == 3
    k1 = (w >> 4) & 0x3fff
    k2 = (w >> 18) & 0x3fff
    out = {"matrix": np.where(none, -1, frm), "adjl": (w & 4) != 0, "adjr": (w & 8) != 0, "ok": np.ones((n, 3), bool)}
    x_ind = np.full((n, 3), -1, np.int64); y_ind = np.full((n, 3), -1, np.int64)
    x_edge = np.full((n, 3), -1, np.int64); y_edge = np.full((n, 3), -1, np.int64)

    def side(g, site, k, use):
        off = g.bwd_off.astype(np.int64)
        deg = off[site + 1] - off[site]
        inside = k < deg
        at = off[site] + np.where(use & inside, k, 0)
        at = np.where(use & inside, at, 0)
        src = np.where(use & inside, np.asarray(g.bwd_src, np.int64)[at] if g.bwd_src.size else -1, -1)
        eid = np.where(use & inside, np.asarray(g.bwd_eid, np.int64)[at] if g.bwd_eid.size else -1, -1)
        return src, eid, inside | ~use

    for m in (0, 2):                                     # X and M take an edge of the left site
        x_ind[:, m], x_edge[:, m], ok = side(left, i, k1[:, m], ~none[:, m])
        out["ok"][:, m] &= ok
    for m in (1, 2):                                     # Y and M take an edge of the right site
        y_ind[:, m], y_edge[:, m], ok = side(right, j, k2[:, m], ~none[:, m])
        out["ok"][:, m] &= ok
    y_ind[:, 0] = np.where(i > 0, j, -1)                 # compute_fwd_scores: max_x.y_ind = j for every row but the first,
    x_ind[:, 1] = np.where(j > 0, i, -1)                 # max_y.x_ind = i for every column but the first
    out.update(x_ind=x_ind, y_ind=y_ind, x_edge_ind=x_edge, y_edge_ind=y_edge)
    return out


class _Side:
    """One graph in the numbering the device arrays are in: bwd lists, and `site`: device site -> the caller's site."""

    def __init__(self, g, keep=None, slot=None):
        off = g.bwd_off.astype(np.int64)
        if keep is None:
            self.bwd_off, self.bwd_src, self.bwd_eid = off, g.bwd_src.astype(np.int64), g.bwd_eid.astype(np.int64)
            self.site = np.arange(g.n_sites, dtype=np.int64)
            return
        keep = keep.astype(np.int64)
        new = np.full(g.n_sites, -1, np.int64)
        new[keep] = np.arange(keep.size)
        deg = np.diff(off)
        owner = np.repeat(np.arange(g.n_sites, dtype=np.int64), deg)
        within = np.arange(int(off[-1]), dtype=np.int64) - np.repeat(off[:-1], deg)
        kept = (new[owner] >= 0) & (new[g.bwd_src.astype(np.int64)] >= 0) if owner.size else np.zeros(0, bool)
        assert np.array_equal(within[kept], slot), "debug_compact's edge slots are not the kept edges' positions"
        self.bwd_src = new[g.bwd_src.astype(np.int64)[kept]]
        self.bwd_eid = g.bwd_eid.astype(np.int64)[kept]
        cnt = np.bincount(new[owner[kept]], minlength=keep.size)
        self.bwd_off = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
        self.site = keep


def dead_sites(g):
    """Sites no path reaches: no bwd edge, or bwd edges from such sites only.  The start site, the end site and the last site
    before it are never counted (the terminal rules name them)."""
    off = g.bwd_off.astype(np.int64)
    alive = np.ones(g.n_sites, bool)
    for s in range(1, g.n_sites - 2):
        src = g.bwd_src[off[s]:off[s + 1]]
        alive[s] = bool(alive[src].any()) if src.size else False
    return np.nonzero(~alive)[0]


def device_arrays(batch, k, cells):
    """(scores [cells, 3] float64, words [cells, 3] uint32) of job k as they lie on the device."""
    sc = np.empty((cells, 3), np.float64)
    bp = np.empty((cells, 3), np.uint32)
    L = pg.lib()
    pg.check(L.pagan_batch_debug_scores(batch._h, k, _dp(sc), sc.size), "pagan_batch_debug_scores")
    pg.check(L.pagan_batch_debug_backptrs(batch._h, k, bp.ctypes.data_as(_u32p), bp.size), "pagan_batch_debug_backptrs")
    return sc, bp


def _bits(x):
    return int(np.float64(x).view(np.uint64))


def check_matrices(batch, k, job, want, flags=0, compact=None, arrays=None):
    """Job k of a batch that has run: every in-band cell's three scores and back-pointers against `want`, what
    oracle.dp_matrices gives for `job` under `flags`.  Asserts that the score equals the oracle's as a bit pattern (-inf
    included), that `from` is the oracle's matrix and is 3 exactly where the oracle has no predecessor, that the source cell
    and both edge ids are the oracle's, and that the two flag bits say whether the source is the site before.

    compact: pg.debug_compact(left, right, band) when the library runs the job with its dead sites taken out -- the device
    arrays are then in the compacted numbering, and are compared on the kept cells; the caller asserts what was dropped.

    arrays: (scores, words) in the device's layout instead of job k's (the helper's own test, without a device).

    A failure lists the first five differing (i, j, state) in the caller's numbering with both sides' values, the device
    diagonal and that diagonal's class (pg.debug_far), i.e. the step of the fill that produced the cell."""
    left, right, model, band = job
    Lx, Ly = left.n_sites - 1, right.n_sites - 1
    if compact is None:
        dl, dr, dband = _Side(left), _Side(right), band
    else:
        dl = _Side(left, compact["keep_left"], compact["slot_left"])
        dr = _Side(right, compact["keep_right"], compact["slot_right"])
        dband = abi.Band(compact["upper"], compact["lower"])
    dLx, dLy = dl.site.size - 1, dr.site.size - 1
    i, j, pos = diag_index(dLx, dLy, dband)
    if compact is None and arrays is None:
        assert i.size == batch.cells_of(k), "the band gives %d cells, the library counts %d" % (i.size, batch.cells_of(k))
    sc, bp = arrays if arrays is not None else device_arrays(batch, k, i.size)
    sc, bp = sc[pos], bp[pos]
    # the same cells in the oracle's arrays
    oi, oj = dl.site[i], dr.site[j]
    begin, end = want["begin"].astype(np.int64), want["end"].astype(np.int64)
    assert np.all((oj >= begin[oi]) & (oj <= end[oi])), "a device cell lies outside the oracle's band"
    ooff = np.concatenate([[0], np.cumsum(np.maximum(end - begin + 1, 0))])
    assert ooff[-1] == want["score"].shape[0]
    at = ooff[oi] + (oj - begin[oi])
    if compact is None:
        assert np.array_equal(at, np.arange(at.size)), "the band's cells are not the oracle's cells"
    w_score, w_ptr = want["score"][at], want["ptr"][at].astype(np.int64)

    got = decode_words(bp, dl, dr, i, j)
    # device numbering -> the caller's sites (a -1 stays -1)
    gx = np.where(got["x_ind"] >= 0, dl.site[np.maximum(got["x_ind"], 0)], -1)
    gy = np.where(got["y_ind"] >= 0, dr.site[np.maximum(got["y_ind"], 0)], -1)
    has = got["matrix"] >= 0
    adjl = has & (got["x_ind"] == (i - 1)[:, None])
    adjr = has & (got["y_ind"] == (j - 1)[:, None])
    bad = (sc.view(np.int64) != w_score.view(np.int64)) | ~got["ok"] | (got["matrix"] != w_ptr[:, :, 0])
    bad |= (gx != w_ptr[:, :, 1]) | (gy != w_ptr[:, :, 2])
    bad |= (got["x_edge_ind"] != w_ptr[:, :, 3]) | (got["y_edge_ind"] != w_ptr[:, :, 4])
    bad |= (got["adjl"] != adjl) | (got["adjr"] != adjr)
    if not bad.any():
        return
    cls = None
    if compact is None and band is not None:
        cls = pg.debug_far(left, right, band)[4] & 15
    lines = []
    for c, m in np.argwhere(bad)[:5]:
        d = int(i[c] + j[c])
        lines.append("(%d, %d, %s) device diagonal %d class %s: score %r (%#x) / oracle %r (%#x); word %#x = from %d, source (%d, %d), "
                     "edges (%d, %d), adjl %d adjr %d%s / oracle matrix %d, source (%d, %d), edges (%d, %d)"
                     % (oi[c], oj[c], NAMES[m], d, "-" if cls is None else int(cls[d]), float(sc[c, m]), _bits(sc[c, m]),
                        float(w_score[c, m]), _bits(w_score[c, m]), int(bp[c, m]), got["matrix"][c, m], gx[c, m], gy[c, m],
                        got["x_edge_ind"][c, m], got["y_edge_ind"][c, m], got["adjl"][c, m], got["adjr"][c, m],
                        "" if got["ok"][c, m] else " (edge slot outside the site's list)", *w_ptr[c, m]))
    raise AssertionError("flags %d: %d of %d (cell, state) entries differ from the oracle; the first:\n  %s"
                         % (flags, int(bad.sum()), bad.size, "\n  ".join(lines)))


# ---- inputs whose candidates tie ---------------------------------------------------------------------------------------------------

def quantised(job, seed=0):
    """The job with every number that enters a score on a grid of 0.25: the model's log_score becomes one of the eight values
    -1.0 .. 0.75 (its own value halved, rounded, clipped -- matches stay above mismatches), the four indel parameters become
    distinct multiples of 0.25 (so that an end-gap or terminal-open rule applied to the wrong cell still changes a score), and
    both graphs' edge weights are drawn from {0, -0.25, -0.5}.  All of it is exact in float32 and sums of a few thousand such
    terms are exact in float64, so candidates tie exactly and the first-maximum rule decides the stored word."""
    left, right, model, band = job
    rng = np.random.default_rng(7000 + seed)
    table = np.clip(np.round(model.log_score.astype(np.float64) * 2.0) / 4.0, -1.0, 0.75).astype(np.float32) + np.float32(0.0)      # (+ 0: no negative zero)
    m2 = abi.Model(table, *np.float32([-1.5, -0.75, -0.5, -0.25]))       # open, extension, end extension, non-gap: all apart

    def graph(g):
        lw = rng.choice(np.float32([0.0, -0.25, -0.5]), g.bwd_logw.shape[0]).astype(np.float32)
        return abi.Graph(g.state, g.bwd_off, g.bwd_src, lw, g.bwd_eid, n_edges=g.n_edges)
    return graph(left), graph(right), m2, band


def tie_counts(job, want):
    """(reachable (cell, state) entries, those of them with a tie, M entries with a tie whose two sites both have two or more
    bwd edges) of oracle.dp_matrices' result `want`."""
    left, right, _, band = job
    i, j = band_cells(left.n_sites - 1, right.n_sites - 1, band)
    reach = want["score"] > -np.inf
    tied = reach & (want["ties"] > 0)
    multi = (np.diff(left.bwd_off.astype(np.int64))[i] >= 2) & (np.diff(right.bwd_off.astype(np.int64))[j] >= 2)
    return int(reach.sum()), int(tied.sum()), int((tied[:, 2] & multi).sum())


def assert_tie_rich(job, want):
    """The condition a tie-rich input must meet, on the oracle alone: ties at 10 % of the reachable entries or more, at least
    100 of them in M cells with two or more edges on both sites."""
    reach, tied, multi = tie_counts(job, want)
    assert tied >= 0.10 * reach, "%d of %d reachable entries have a tie" % (tied, reach)
    assert multi >= 100, "%d tied M cells with two or more edges on both sites" % multi
