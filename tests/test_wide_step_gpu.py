"""GPU parity of the seven-wave wide step (dp_pipe.hip, wide_run7; round 6): the site decode from the loader's normalised
records, the left site kept in registers while a lane keeps its row, the L2 operands requested in front of the lock step.

Every job is one run of class 4 diagonals of a known shape -- asserted from the plan before anything is compared -- and is
compared bit for bit with the oracle:

  * a box in a narrow band: entry from the hand-scheduled loop (the first steps take every operand from L2), served far sites
    whose cells lie inside the run, the exit; with the wide ring of 12 x 384 (geometry A) and of 9 x 512 positions (B);
  * a stripe wider than the lanes over the whole job: every lane hands its row over three times and decodes its next left
    site when that row comes into the band, and nearly every step has an operand older than the wide ring;
  * the same stripe with three-edge sites (the third pass and the PR_THREE decode inside a run), and once more with edges
    longer than the loader permutes (the one shape that keeps the order-agnostic decode);
  * the option bits, and the A/B switch that leaves every run to the four compute waves."""
import functools

import numpy as np
import pytest

from pagan2_msa_amd import abi, synth
from test_pipe_gpu import same

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def wide_job(shape, seed):
    """left, right, model, band of one of the shapes above"""
    n, half, box, graph = {
        "box_a": (1800, 25, (600, 900, 30), {}),
        "box_b": (1800, 25, (600, 990, 130), {}),
        "stripe": (1500, 270, None, {}),
        "stripe_b": (1500, 380, None, {}),
        "three": (1500, 270, None, dict(p_extra=0.05, max_deg=4, max_span=12)),
        "three_far": (1500, 270, None, dict(p_extra=0.05, max_deg=4, max_span=20)),
    }[shape]
    kw = dict(p_extra=0.03, max_deg=3, max_span=30)
    kw.update(graph)
    left = synth.random_graph(n, 15, 300 + seed, **kw)
    right = synth.random_graph(n, 15, 400 + seed, **kw)
    Lx, Ly = left.n_sites - 1, right.n_sites - 1
    centre = np.arange(Lx) * (Ly - 1) // max(Lx - 1, 1)
    upper = np.maximum(centre - half, 0); lower = np.minimum(centre + half, Ly - 1)
    if box:
        a, b, jump = box
        upper[a:b] = upper[a]; lower[a:b] = lower[b - 1] + jump
    upper = np.maximum.accumulate(upper); lower = np.maximum.accumulate(lower)
    upper[0] = 0; lower[-1] = Ly - 1
    return left, right, synth.random_model(15, seed), abi.Band(upper, lower)


@functools.lru_cache(maxsize=None)
def expected(oracle, shape, seed, flags=0):
    left, right, model, band = wide_job(shape, seed)
    return oracle.dp_align(left, right, model, band, flags=flags) if flags else oracle.dp_align(left, right, model, band)


def plan_of(pg, shape, seed):
    """(first diagonal, diagonals, widest diagonal, rows) of the job's class 4 run -- there is exactly one --, the number of served
    far sites and the number of their cells on the run's diagonals"""
    left, right, _, band = wide_job(shape, seed)
    n_far, hfl, hfr, _, cls = pg.debug_far(left, right, band)
    cls = cls & 15
    Lx, Ly = left.n_sites - 1, right.n_sites - 1
    lo = np.maximum(band.upper[:Lx].astype(np.int64), 0); hi = np.minimum(band.lower[:Lx].astype(np.int64), Ly - 1)
    d4 = np.nonzero(cls == 4)[0]
    assert len(d4) and d4[-1] - d4[0] + 1 == len(d4), "one run of class 4 diagonals"
    assert not (cls == 5).any()
    d0, d1 = int(d4[0]), int(d4[-1])
    edge = np.zeros(len(cls) + 2, np.int64)
    rows = np.arange(Lx)
    np.add.at(edge, rows + lo, 1); np.add.at(edge, rows + hi + 1, -1)
    width = np.cumsum(edge)[:len(cls)]
    in_run = np.maximum(np.minimum(rows + hi, d1) - np.maximum(rows + lo, d0) + 1, 0)        # cells of row i on the run's diagonals
    far_l = (hfl[:Lx] & 0x80) != 0
    far_cells = int(in_run[far_l].sum())
    for j in np.nonzero(hfr[:Ly] & 0x80)[0]:
        i = rows[(lo <= j) & (j <= hi) & (rows + j >= d0) & (rows + j <= d1)]
        far_cells += len(i)
    return d0, len(d4), int(width[d0:d1 + 1].max()), int((in_run > 0).sum()), int(n_far), far_cells


def check(pg, oracle, shape, seed, flags=0):
    left, right, model, band = wide_job(shape, seed)
    got = pg.align(left, right, model, band, flags=flags) if flags else pg.align(left, right, model, band)
    same(got, expected(oracle, shape, seed, flags), "%s seed %d flags %d" % (shape, seed, flags))


def assert_box_a(pg, seed):
    _, n4, widest, _, n_far, far_cells = plan_of(pg, "box_a", seed)
    assert n4 == 195 and widest == 300
    assert 23 <= n_far <= 33 and 313 <= far_cells <= 580


def assert_stripe(pg, shape, seed, width):
    _, n4, widest, rows, _, _ = plan_of(pg, shape, seed)
    assert n4 == 2517 and widest == width
    assert rows == wide_job(shape, seed)[0].n_sites - 1 and rows >= 1500, "the run covers every row: each lane takes several"


@pytest.mark.parametrize("seed", range(4))
def test_a_box_entered_from_the_narrow_loop(pg, oracle, seed):
    assert_box_a(pg, seed)
    check(pg, oracle, "box_a", seed)


@pytest.mark.parametrize("seed", range(2))
def test_a_box_in_the_wider_ring(pg, oracle, seed):
    _, n4, widest, _, _, _ = plan_of(pg, "box_b", seed)
    assert n4 == 475 and widest == 390 and widest > 352
    check(pg, oracle, "box_b", seed)


@pytest.mark.parametrize("seed", range(2))
def test_a_stripe_hands_every_row_over(pg, oracle, seed):
    assert_stripe(pg, "stripe", seed, 271)
    check(pg, oracle, "stripe", seed)


def test_a_stripe_in_the_wider_ring(pg, oracle):
    assert_stripe(pg, "stripe_b", 0, 381)
    check(pg, oracle, "stripe_b", 0)


@pytest.mark.parametrize("seed", range(2))
def test_three_edge_sites_inside_a_run(pg, oracle, seed):
    assert_stripe(pg, "three", seed, 271)
    left, right, _, _ = wide_job("three", seed)
    three = lambda g: sum(1 for s in range(1, g.n_sites - 1) if g.bwd_off[s + 1] - g.bwd_off[s] == 3)
    assert three(left) + three(right) > 0, "the job is meant to have three-edge sites"
    check(pg, oracle, "three", seed)


def test_three_edge_sites_the_loader_left_as_they_were(pg, oracle):
    """Three edges, one from the previous site, one of them more than PAGE - 2 = 12 sites long: no PR_THREE, and site7 sorts
    the edges out itself.  Every row of the stripe has cells in the run, so each such left site is decoded inside it."""
    assert_stripe(pg, "three_far", 0, 271)
    left, right, _, _ = wide_job("three_far", 0)

    def unpermuted(g):
        n = 0
        for s in range(1, g.n_sites - 1):
            dist = s - g.bwd_src[g.bwd_off[s]:g.bwd_off[s + 1]]
            n += len(dist) == 3 and (dist == 1).sum() == 1 and dist.max() > 12
        return n
    assert unpermuted(left) >= 10 and unpermuted(right) >= 10
    check(pg, oracle, "three_far", 0)


@pytest.mark.parametrize("flags", [abi.OPT_NO_TERMINAL_EDGES, abi.OPT_NO_REDUCED_TERMINAL_PEN])
def test_option_bits_in_a_wide_run(pg, oracle, flags):
    assert_box_a(pg, 0)
    check(pg, oracle, "box_a", 0, flags)


@pytest.mark.parametrize("shape,seed", [("box_a", 1), ("stripe", 0)])
def test_the_four_wave_run_behind_its_switch(pg, oracle, monkeypatch, shape, seed):
    """PAGAN_DP_WIDE7=0 routes every run to wide_run.  (The request in front of the lock step has a compile-time switch,
    -DPG_WIDE7_FETCH_BEHIND: an A/B library, not a run-time path.)"""
    if shape == "box_a":
        assert_box_a(pg, seed)
    else:
        assert_stripe(pg, shape, seed, 271)
    monkeypatch.setenv("PAGAN_DP_WIDE7", "0")
    check(pg, oracle, shape, seed)
