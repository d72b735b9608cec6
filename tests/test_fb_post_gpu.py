"""GPU: reading a finished forward/backward pass on the device (dp_fb_post.inc) -- pg_fb_gather (path support, posterior cells)
and pg_fb_marginals (the posterior matrix summed over rows and over columns, best partner per site) -- against the oracle's
dense posterior (oracle/oracle_fb.cpp) with the sums taken in numpy.  Tolerance: the project's posterior tolerance, 1e-7
relative, with an absolute part of 1e-12 per in-band cell of the row or column that was summed."""
import numpy as np
import pytest

import pagan2_msa_amd as pgm
from pagan2_msa_amd import abi, host, synth

pytestmark = pytest.mark.gpu
ROWS = 64                      # FB_PM_ROWS: rows (columns) of one workgroup of pg_fb_marginals


def _random_tunnel(rng, Lx, Ly, lo_half, hi_half):
    half = rng.integers(lo_half, hi_half, Lx)
    centre = np.arange(Lx) * (Ly - 1) // max(Lx - 1, 1)
    upper = np.maximum.accumulate(np.maximum(centre - half, 0))
    lower = np.maximum.accumulate(np.minimum(centre + half, Ly - 1))
    upper[0] = 0
    lower[-1] = Ly - 1
    return abi.Band(upper.astype(np.int32), lower.astype(np.int32))


def _boxed_tunnel(Lx, Ly, boxes, half=8):
    """a narrow band around the main diagonal with square boxes [(first row, side), ...] that hold every cell of their rows x columns"""
    centre = np.arange(Lx) * (Ly - 1) // max(Lx - 1, 1)
    upper, lower = np.maximum(centre - half, 0), np.minimum(centre + half, Ly - 1)
    for a, w in boxes:
        upper[a:a + w] = np.minimum(upper[a:a + w], max(centre[a] - half, 0))
        lower[a:a + w] = np.maximum(lower[a:a + w], min(centre[a + w - 1] + half, Ly - 1))
    upper, lower = np.maximum.accumulate(upper), np.maximum.accumulate(lower)
    upper[0] = 0
    lower[-1] = Ly - 1
    return abi.Band(upper.astype(np.int32), lower.astype(np.int32))


def _is_plain(g):
    n = g.n_sites
    return bool(np.all(np.diff(g.bwd_off)[1:] == 1) and np.array_equal(g.bwd_src[:n - 1], np.arange(n - 1)))


def _in_band(Lx, Ly, band):
    """[Lx, Ly] bool: the cells inside the tunnel as the library clamps it"""
    if band is None:
        return np.ones((Lx, Ly), bool)
    lo = np.maximum(np.asarray(band.upper[:Lx]), 0)
    hi = np.minimum(np.asarray(band.lower[:Lx]), Ly - 1)
    j = np.arange(Ly)[None, :]
    return (j >= lo[:, None]) & (j <= hi[:, None])


class Case:
    def __init__(self, kind, left, right, mp, band, model, oracle):
        self.kind, self.left, self.right, self.mp, self.band, self.model = kind, left, right, mp, band, model
        self.Lx, self.Ly = left.n_sites - 1, right.n_sites - 1
        _lf, _lb, self.post, self.logf = oracle.fb(left, right, mp, band=band)
        inb = _in_band(self.Lx, self.Ly, band)
        self.n_row, self.n_col = inb.sum(1), inb.sum(0)

    def pair(self):
        return (self.left, self.right, self.mp, self.band)


@pytest.fixture(scope="module")
def cases(pg, oracle):
    """Every pair of this file with the oracle's posterior, computed once."""
    out = []
    rng = np.random.default_rng(2031)
    bf4 = [0.3, 0.2, 0.2, 0.3]
    # 1: plain DNA pairs, full matrix: 3 row blocks and a remainder; a one-residue sequence (Lx = 2)
    _, seqs, _ = synth.evolve_balanced(2, 150, branch=0.05, sub=0.06, indel_start=0.02, mean_len=3, seed=41)
    gl, gr = (host.HGraph.leaf(s).flatten() for s in seqs)
    assert gl.n_sites - 1 > 2 * ROWS and (gl.n_sites - 1) % ROWS and (gr.n_sites - 1) % ROWS
    mp, model = host.model_prob(1, 0.1, base_freq=bf4), host.dna_model(bf4, 0.1)[0]
    out.append(Case("plain", gl, gr, mp, None, model, oracle))
    one = host.HGraph.leaf("G").flatten()
    assert one.n_sites - 1 == 2
    out.append(Case("plain", one, gr, mp, None, model, oracle))
    out.append(Case("plain", gr, one, mp, None, model, oracle))
    # 2: the graph pairs of a tree of 8 (multi-edge sites, skip edges): no band, narrow and wide random tunnels
    names, seqs8, nwk = synth.evolve_balanced(8, 700, branch=0.04, sub=0.04, indel_start=0.01, mean_len=4, seed=46)
    msa = host.Msa(names, seqs8, nwk, use_anchors=0).align()
    bf = np.array([sum(s.count(x) for s in seqs8) for x in "ACGT"], np.float32)
    bf /= bf.sum()
    leaf_pair = None
    for k in range(msa.n_internal):
        left, right, model_k, _band = msa.node_job(k)
        mp_k = host.model_prob(1, msa.node_info(k).dist, base_freq=bf)
        if _is_plain(left) and _is_plain(right):
            leaf_pair = leaf_pair or (left, right, mp_k, model_k)
            continue
        Lx, Ly = left.n_sites - 1, right.n_sites - 1
        out.append(Case("graph", left, right, mp_k, None, model_k, oracle))
        out.append(Case("graph", left, right, mp_k, _random_tunnel(rng, Lx, Ly, 5, 12), model_k, oracle))
        out.append(Case("graph", left, right, mp_k, _random_tunnel(rng, Lx, Ly, 100, 180), model_k, oracle))
    assert sum(c.kind == "graph" for c in out) == 9
    # 3: a protein pair (211 states)
    aa = "ARNDCQEGHILKMFPSTWYV"
    _, ps, _ = synth.evolve_balanced(2, 200, branch=0.05, sub=0.08, indel_start=0.01, mean_len=3, seed=42, alphabet=aa)
    leaf_alpha, _ = host.alphabets(2)
    pl, pr = (host.HGraph.leaf(s, leaf_alpha).flatten() for s in ps)
    out.append(Case("protein", pl, pr, host.model_prob(2, 0.2), None, host.protein_model(0.2)[0], oracle))
    # 4: a boxed tunnel: the diagonals' intervals jump where a box begins and ends
    left, right, mp_k, model_k = leaf_pair
    Lx, Ly = left.n_sites - 1, right.n_sites - 1
    out.append(Case("boxed", left, right, mp_k, _boxed_tunnel(Lx, Ly, [(100, 150), (400, 200)]), model_k, oracle))
    return out


def _close(got, want, n_cells):
    return np.all(np.abs(got - want) <= 1e-7 * np.abs(want) + 1e-12 * n_cells)


def _check_marginals(c, mg):
    post = c.post
    for side, (gap, match, best, best_p, state, n_cells) in enumerate((
            ("pX", "pM_left", "best_j", "best_p_left", 0, c.n_row), ("pY", "pM_right", "best_i", "best_p_right", 1, c.n_col))):
        axis = 1 - side
        want_gap, want_m = post[:, :, state].sum(axis), post[:, :, 2].sum(axis)
        assert _close(mg[gap], want_gap, n_cells), (c.kind, gap, np.abs(mg[gap] - want_gap).max())
        assert _close(mg[match], want_m, n_cells), (c.kind, match, np.abs(mg[match] - want_m).max())
        top = post[:, :, 2].max(axis)
        assert _close(mg[best_p], top, n_cells), (c.kind, best_p)
        b = mg[best]
        assert np.all((b >= -1) & (b < post.shape[axis]))
        has = b >= 0
        assert np.all(mg[best_p][~has] == 0.0)
        idx = np.arange(post.shape[side])
        at = post[idx[has], b[has], 2] if side == 0 else post[b[has], idx[has], 2]
        assert _close(at, top[has], n_cells[has]), (c.kind, best)
        assert np.all(top[~has] <= 1e-12 * n_cells[~has])
    return mg["pX"] + mg["pM_left"], mg["pY"] + mg["pM_right"]


def test_site_marginals_of_every_kind_of_pair(pg, cases):
    """Cases 1-4 one pair at a time: sums and best partners against the oracle; two plain sequences use every site
    (pX + pM = 1, pY + pM' = 1); a graph pair's sums stay <= 1 and some site of every such pair is skipped with real mass."""
    seen = set()
    for c in cases:
        fb = pgm.FullProbability(*c.pair())
        mg = fb.site_marginals()
        rows, cols = _check_marginals(c, mg)
        print("%s %d x %d%s: row sums %.6f .. %.6f, column sums %.6f .. %.6f" % (c.kind, c.Lx, c.Ly, " banded" if c.band is not None else "",
                                                                               rows.min(), rows.max(), cols.min(), cols.max()))
        if c.kind == "plain":
            assert np.all(np.abs(rows - 1) <= 1e-7) and np.all(np.abs(cols - 1) <= 1e-7)
        if c.kind == "graph":
            assert rows.max() <= 1 + 1e-9 and cols.max() <= 1 + 1e-9
            assert min(rows.min(), cols.min()) < 0.999
        seen.add(c.kind)
        # one side only: the other pass does not run, the values are the same bits
        only = fb.site_marginals(columns=False)
        assert set(only) == {"pX", "pM_left", "best_j", "best_p_left"}
        assert all(np.array_equal(only[k], mg[k]) for k in only)
        fb.close()
    assert seen == {"plain", "graph", "protein", "boxed"}
    assert any(c.Lx == 2 for c in cases) and any(c.Lx > 2 * ROWS and c.kind == "plain" for c in cases)


def test_site_marginals_batch_is_the_one_pair_call_bit_for_bit(pg, cases):
    """One launch per pass over a batch that mixes all kinds: every array equal to the one-pair call's, and to a second run's."""
    fbs = pgm.full_probability_batch([c.pair() for c in cases])
    a = pgm.site_marginals_batch(fbs)
    b = pgm.site_marginals_batch(fbs)
    for c, fb, ma, mb in zip(cases, fbs, a, b):
        one = pgm.FullProbability(*c.pair())
        assert one.log_fwd == fb.log_fwd
        mo = one.site_marginals()
        for k in mo:
            assert ma[k].tobytes() == mb[k].tobytes(), (c.kind, k)
            assert ma[k].tobytes() == mo[k].tobytes(), (c.kind, k)
        one.close()
    for fb in fbs:
        fb.close()


def _own_cells(cols):
    """the DP cell of every column, derived here (not by the library): (state, i, j), or None at skip columns"""
    ci = cj = 0
    out = []
    for left, right, ps in cols:
        if ps == 2:
            ci, cj = left, right
            out.append((2, ci, cj))
        elif ps == 3:
            ci = left
            out.append((0, ci, cj))
        elif ps == 4:
            cj = right
            out.append((1, ci, cj))
        else:
            out.append(None)
    return out


def test_path_support_along_viterbi_and_sampled_paths(pg, cases):
    n_skip = 0
    rng = np.random.default_rng(8)
    for c in cases:
        if c.kind == "protein":
            continue
        res = pgm.align(c.left, c.right, c.model, c.band)
        assert res.status == 0
        fb = pgm.FullProbability(*c.pair())
        sup = fb.path_support(res.cols)
        own = _own_cells(res.cols.tolist())
        real = [k for k, x in enumerate(own) if x is not None]
        skip = [k for k, x in enumerate(own) if x is None]
        n_skip += len(skip)
        assert np.all(sup[skip] == -1.0)
        want = np.array([c.post[own[k][1], own[k][2], own[k][0]] for k in real])
        assert np.allclose(sup[real], want, rtol=1e-7, atol=1e-12), c.kind
        lib_cells = pgm.path_cells(res.cols)
        assert [tuple(x) for x in lib_cells[real].tolist()] == [own[k] for k in real]
        assert np.all(lib_cells[skip] == -1)
        # the same numbers as posterior_cells on the same cells, bit for bit
        assert fb.posterior_cells(lib_cells[real]).tobytes() == sup[real].tobytes()
        # a sampled path: the columns' cells, reversed, are the cells the sampler visited
        u = rng.random(c.left.n_sites + c.right.n_sites)
        sres, visited = fb.sample_path(u)
        sc = pgm.path_cells(sres.cols)
        sc = sc[sc[:, 0] >= 0]
        assert np.array_equal(sc[::-1][:, [1, 2, 0]], visited)
        ssup = fb.path_support(sres.cols)
        assert np.all(ssup[sres.cols[:, 2] >= 5] == -1.0) and np.all(ssup[sres.cols[:, 2] <= 4] > 0)
        fb.close()
    assert n_skip > 0


def test_errors(pg, cases):
    c = cases[0]
    L = pgm.lib()
    import ctypes as C
    out = np.zeros(4)
    dp = out.ctypes.data_as(C.POINTER(C.c_double))
    cols = np.array([[1, 1, 2], [2, 2, 2]], np.int32)
    cp = cols.ctypes.data_as(C.POINTER(abi.CCol))
    assert L.pagan_fb_path_support(None, cp, 2, dp) == abi.PAGAN_E_ARG
    assert L.pagan_fb_site_marginals(None, dp, None, None, None, None, None, None, None) == abi.PAGAN_E_ARG
    fb = pgm.FullProbability(*c.pair())
    assert L.pagan_fb_path_support(fb._h, cp, -1, dp) == abi.PAGAN_E_ARG
    for bad in ([[c.Lx, 1, 2]], [[1, c.Ly, 2]], [[1, c.Ly + 5, 4]], [[-3, 1, 3]]):
        with pytest.raises(pgm.PaganError) as e:
            fb.path_support(np.array(bad, np.int32))
        assert e.value.code == abi.PAGAN_E_ARG
    with pytest.raises(pgm.PaganError) as e:
        fb.path_support(np.array([[1, 1, 9]], np.int32))
    assert e.value.code == abi.PAGAN_E_ARG
    assert fb.path_support(np.zeros((0, 3), np.int32)).shape == (0,)
    fb.close()
