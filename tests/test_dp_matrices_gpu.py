"""Every stored score and back-pointer of the Viterbi fill against the oracle's own matrices (oracle.dp_matrices), on every
fill kernel and on each of the banded kernel's classes of step.

The other GPU tests compare a job's optimal path with the oracle (`same`), or whole matrices between two of the library's own
kernels and modes.  Here the whole matrix has a reference outside the library: for every in-band cell and the three states the
score as a bit pattern, the predecessor state, the source cell, both edge ids and the two adjacency bits
(tests/dp_matrix_check.py: check_matrices; no tolerance, no cell left out).  This is also where the kernels the other files
use as their reference -- pg_fill_ring, the one-workgroup wavefront -- are checked themselves.

Every case builds its job with the maker of the file that owns the shape, asserts from the host-only plan calls that the job
takes the route and classes it is meant to take (CASES[name].plan, run without a GPU by tests/test_oracle_matrices_cpu.py),
runs one poisoned batch, compares the matrices and then the path as well.

The CPU side of the largest cases, the 1500 x 541 stripe (738 871 cells) and the stripe segment (742 401), measured on one
core of the development machine, best of three: oracle.dp_matrices 0.11 s, check_matrices' decode and comparison 0.37 s (its
arrays encoded from the oracle's instead of read from a device).  On the MI355X host every case stays well under a second, device run and download included."""
import functools

import numpy as np
import pytest

from pagan2_msa_amd import abi, synth
import dp_matrix_check as mc
import test_far_plan_cpu
import test_pipe_gpu
import test_routes_cpu
import test_strips_gpu
import test_tiles_gpu
import test_wide_step_gpu
from test_pipe_gpu import banded_job, same

pytestmark = pytest.mark.gpu

NTE, NRT = abi.OPT_NO_TERMINAL_EDGES, abi.OPT_NO_REDUCED_TERMINAL_PEN
STRIPS = {"PAGAN_DP_WIDE": "strips", "PAGAN_DP_STRIP_SITES": "100000", "PAGAN_DP_STRIP_STATES": "100000"}
TILES = {"PAGAN_DP_WIDE": "tiles"}
PIPE, BIG, TILED, WAVEFRONT, STRIPED = ("pg_fill_pipe", "pg_fill_pipe (large table)", "pg_fill_tiles_flow", "pg_fill_wavefront",
                                        "pg_fill_pipe (row strips)")


class Case:
    """job: () -> (left, right, model, band); env on top of PAGAN_DP_COMPACT=0; route: what debug_route must say;
    plan: (pg, job) -> None, the further assertions on the host-only plan."""

    def __init__(self, job, route, env=None, flags=0, plan=None):
        self.make, self.route, self.env, self.flags, self.plan = job, route, dict(env or {}), flags, plan

    @functools.cached_property
    def job(self):
        return self.make()

    def assert_plan(self, pg):
        left, right, model, band = self.job
        assert pg.debug_route(left, right, model, band)[0] == self.route
        if self.plan:
            self.plan(pg, self.job)


# ---- plan assertions (each the one of the file that owns the shape) -----------------------------------------------------------

def classes(pg, job):
    return pg.debug_far(job[0], job[1], job[3])[4] & 15


def plan_classes(want):
    def check(pg, job):
        cls, waves = pg.debug_plan(job[0], job[1], job[3])
        assert set(np.unique(cls)) >= want, "the job is meant to reach these classes"
        assert sum(len(w) for w in waves) >= 4, "waves are meant to sleep and wake"
    return check


def plan_class5_box(pg, job):
    plan_classes({1, 3, 4})(pg, job)
    assert (classes(pg, job) == 5).sum() > 100, "the box is meant to be wider than the record windows"


def plan_4_behind_5(pg, job):
    cls = classes(pg, job)
    assert [d for d in range(1, len(cls)) if cls[d] == 4 and cls[d - 1] == 5], "a class 4 run directly behind a class 5 run"


def plan_history_lines(pg, job):
    n, hfl, hfr, hb, cls = pg.debug_far(job[0], job[1], job[3])
    assert n > 0 and ((hb & 1) & (cls == 1)).sum() > 200, "far sites on class 1 diagonals: the lanes' own far blocks run"


def plan_third_pass(pg, job):
    n, hfl, hfr, hb, cls = pg.debug_far(job[0], job[1], job[3])
    assert ((hb & 2) > 0).sum() > 200, "three-edge sites on class 1 diagonals: the third pass runs"


def plan_dead_sites(pg, job):
    cls, _ = pg.debug_plan(job[0], job[1], job[3])
    assert (cls == 3).sum() < 100 and ((cls == 1) | (cls == 2)).sum() > 800


def plan_wide(shape):
    def check(pg, job):
        if shape == "box_a":
            test_wide_step_gpu.assert_box_a(pg, 0)
        else:
            test_wide_step_gpu.assert_stripe(pg, shape, 0, 271)
    return check


def plan_stripe_segment(pg, job):
    """one run of class 4 diagonals, wider than the lanes, over more than a thousand rows: every lane takes several"""
    left, right, _, band = job
    cls = classes(pg, job)
    d4 = np.nonzero(cls == 4)[0]
    assert len(d4) > 1500 and d4[-1] - d4[0] + 1 == len(d4) and not (cls == 5).any(), "one run of class 4 diagonals"
    lo, hi = mc.row_band(left.n_sites - 1, right.n_sites - 1, band)
    rows = np.arange(lo.size)
    in_run = np.maximum(np.minimum(rows + hi, d4[-1]) - np.maximum(rows + lo, d4[0]) + 1, 0)
    assert (in_run > 0).sum() >= 1100
    i, j = mc.band_cells(lo.size, right.n_sites - 1, band)
    assert np.bincount(i + j)[d4].max() == 271


def plan_tiles(at_least):
    def check(pg, job):
        assert len(pg.debug_tiles(job[0], job[1], job[3])[1]) >= at_least
    return check


def plan_wide_band_tiles(pg, job):
    left, right, _, band = job
    side, tiles = pg.debug_tiles(left, right, band)
    full = ((left.n_sites + side - 2) // side) * ((right.n_sites + side - 2) // side)
    assert 0 < len(tiles) < full, "tiles outside the band are not launched"


def plan_strips(at_least):
    def check(pg, job):
        assert len(pg.debug_strips(job[0], job[1], job[3])) >= at_least
    return check


# ---- jobs ---------------------------------------------------------------------------------------------------------------------

def hist_job(seed):
    left, right, band = test_far_plan_cpu.job(seed, n=2000 + 150 * seed, max_span=int([14, 18, 25, 30, 40, 44, 60, 22][seed]))
    return left, right, synth.random_model(15, seed), band


def third_pass_job():
    left, right, band = test_far_plan_cpu.job(40, n=1800, p_extra=0.05, max_deg=4, max_span=5)
    return left, right, synth.random_model(15, 50), band


def big_table_job(S):
    left, right, _, band = banded_job(0, max_span=40)
    rng = np.random.default_rng(100)
    left.state[1:-1] = rng.integers(0, S, left.n_sites - 2)
    right.state[1:-1] = rng.integers(0, S, right.n_sites - 2)
    return left, right, synth.random_model(S, 0), band


def full_job(cases, name, states=15):
    nl, nr, p_extra, max_deg, max_span, p_dead = cases[name][:6]
    left = synth.random_graph(nl, states, 101, p_extra=p_extra, max_deg=max_deg, max_span=max_span, p_dead=p_dead)
    right = synth.random_graph(nr, states, 202, p_extra=p_extra, max_deg=max_deg, max_span=max_span, p_dead=p_dead)
    return left, right, synth.random_model(states, 7), None


def stripe_segment_job():
    """test_wide_step_gpu's stripe (541 columns a row) over rows 1200 .. 2300 of a band 51 columns wide: few enough cells per
    diagonal on average for the router to leave the job on the banded kernel, so that the stripe's class 4 run is executed"""
    kw = dict(p_extra=0.03, max_deg=3, max_span=30)
    left, right = synth.random_graph(4000, 15, 300, **kw), synth.random_graph(4000, 15, 400, **kw)
    Lx, Ly = left.n_sites - 1, right.n_sites - 1
    centre = np.arange(Lx) * (Ly - 1) // max(Lx - 1, 1)
    half = np.full(Lx, 25)
    half[1200:2300] = 270
    upper = np.maximum.accumulate(np.maximum(centre - half, 0)); lower = np.maximum.accumulate(np.minimum(centre + half, Ly - 1))
    upper[0] = 0; lower[-1] = Ly - 1
    return left, right, synth.random_model(15, 0), abi.Band(upper, lower)


def wide_band_job(seed=0):
    left = synth.random_graph(900, 15, 10 + seed, p_extra=0.08, max_deg=4, max_span=30)
    right = synth.random_graph(860, 15, 20 + seed, p_extra=0.08, max_deg=4, max_span=30)
    return left, right, synth.random_model(15, seed), test_tiles_gpu.wide_band(left.n_sites - 1, right.n_sites - 1, 400, seed)


def shape_job(nl, nr):
    left = synth.random_graph(nl, 15, 300 + nl, p_extra=0.2, max_deg=4, max_span=12, p_dead=0.02)
    right = synth.random_graph(nr, 15, 400 + nr, p_extra=0.2, max_deg=4, max_span=12, p_dead=0.02)
    return left, right, synth.random_model(15, nl + nr), None


def small_wide_job(nl, nr):
    left = synth.random_graph(nl, 15, 5, p_extra=0.1, max_deg=3, max_span=9)
    right = synth.random_graph(nr, 15, 6, p_extra=0.1, max_deg=3, max_span=9)
    return left, right, synth.random_model(15, 3), None


def dead_job(banded):
    """p_dead = 0.3 with two or three edges of up to 60 sites into every other site: the dead sites are stepped over (with the
    short edges of the other files' graphs the cascade leaves no path at all, and the job is unreachable)"""
    left = synth.random_graph(700, 15, 501, p_extra=1.0, max_deg=3, max_span=60, p_dead=0.3)
    right = synth.random_graph(660, 15, 502, p_extra=1.0, max_deg=3, max_span=60, p_dead=0.3)
    band = test_routes_cpu.narrow_band(left, right, 60) if banded else None
    return left, right, synth.random_model(15, 21), band


@functools.lru_cache(maxsize=None)
def sweep_5000_739():
    """(job, flags) of test_a_wide_run_whose_first_row_moved_on_its_first_diagonal"""
    case = test_pipe_gpu.sweep_case(5000, 739)
    return case[:4], case[4]


def most_multi_edge_strip_case():
    """the name of test_strips_gpu.CASES' entry whose graphs have the most sites with two or more bwd edges"""
    def multi(name):
        left, right, _, _ = full_job(test_strips_gpu.CASES, name)
        return sum(int((np.diff(g.bwd_off) >= 2).sum()) for g in (left, right))
    return max(sorted(test_strips_gpu.CASES), key=multi)


CASES = {
    # banded, small table: pg_fill_pipe
    "banded_0": Case(lambda: banded_job(0, max_span=40), PIPE, plan=plan_classes({2, 3, 4})),
    "banded_1": Case(lambda: banded_job(1, max_span=40), PIPE, plan=plan_classes({2, 3, 4})),
    "banded_2": Case(lambda: banded_job(2, max_span=8), PIPE, plan=plan_classes({1, 3, 4})),
    "banded_3_class5_box": Case(lambda: banded_job(3, max_span=8), PIPE, plan=plan_class5_box),
    "class4_behind_class5": Case(lambda: sweep_5000_739()[0], PIPE, flags=sweep_5000_739()[1], plan=plan_4_behind_5),
    "history_lines_0": Case(lambda: hist_job(0), PIPE, plan=plan_history_lines),
    "history_lines_6": Case(lambda: hist_job(6), PIPE, flags=NTE, plan=plan_history_lines),
    "third_pass_40": Case(third_pass_job, PIPE, plan=plan_third_pass),
    "wide7_box_a": Case(lambda: test_wide_step_gpu.wide_job("box_a", 0), PIPE, plan=plan_wide("box_a")),
    # (a stripe is wider than 242 cells on every diagonal, so it is a wide job to the router -- more than 128 cells per diagonal on
    # average -- and runs on the tiled kernel: its class 4 plan, which test_wide_step_gpu.py asserts, is never executed)
    "stripe": Case(lambda: test_wide_step_gpu.wide_job("stripe", 0), TILED, plan=plan_wide("stripe")),
    "stripe_three_far": Case(lambda: test_wide_step_gpu.wide_job("three_far", 0), TILED, plan=plan_wide("three_far")),
    "wide7_stripe_segment": Case(stripe_segment_job, PIPE, plan=plan_stripe_segment),
    "banded_dead_sites": Case(lambda: banded_job(12, n=500, max_span=6, box=False, p_dead=0.2), PIPE, plan=plan_dead_sites),
    # banded, large table
    "table_1892": Case(lambda: big_table_job(1892), BIG, plan=plan_classes({2, 3, 4})),
    "table_211": Case(lambda: big_table_job(211), BIG, plan=plan_classes({2, 3, 4})),
    # row strips
    "strips_plain": Case(lambda: full_job(test_strips_gpu.CASES, "plain"), STRIPED, STRIPS, plan=plan_strips(2)),
    "strips_most_multi_edge": Case(lambda: full_job(test_strips_gpu.CASES, most_multi_edge_strip_case()), STRIPED, STRIPS, plan=plan_strips(2)),
    "strips_wide_band": Case(wide_band_job, STRIPED, STRIPS, plan=plan_strips(2)),
    # tiles
    "tiles_three_and_more_edges": Case(lambda: full_job(test_tiles_gpu.CASES, "three_and_more_edges"), TILED, TILES, plan=plan_tiles(16)),
    "tiles_edges_across_tiles": Case(lambda: full_job(test_tiles_gpu.CASES, "edges_across_tiles"), TILED, TILES, plan=plan_tiles(16)),
    "tiles_dead_sites": Case(lambda: full_job(test_tiles_gpu.CASES, "dead_sites"), TILED, TILES, plan=plan_tiles(16)),
    "tiles_wide_band": Case(wide_band_job, TILED, TILES, plan=plan_wide_band_tiles),
    # test_shapes_around_the_tile_size's shapes: full matrices of at most 128 cells per diagonal on average, which the router
    # gives to the banded kernel whatever PAGAN_DP_WIDE says
    "shape_1x700": Case(lambda: shape_job(1, 700), PIPE, TILES),
    "shape_700x1": Case(lambda: shape_job(700, 1), PIPE, TILES),
    "shape_63x64": Case(lambda: shape_job(63, 64), PIPE, TILES),
    "shape_2x2": Case(lambda: shape_job(2, 2), PIPE, TILES),
    # the comparing kernels: the other files' references
    "wavefront": Case(lambda: full_job(test_tiles_gpu.CASES, "three_and_more_edges"), WAVEFRONT, {"PAGAN_DP_WIDE": "wavefront"}),
    "ring": Case(lambda: banded_job(5), PIPE, {"PAGAN_DP_FILL": "ring"}),
    "negative_zero": Case(lambda: test_routes_cpu.jobs()[WAVEFRONT], WAVEFRONT),
    # option bits
    "banded_no_terminal_edges": Case(lambda: banded_job(7, n=400, box=False), PIPE, flags=NTE),
    "banded_no_reduced_terminal": Case(lambda: banded_job(7, n=400, box=False), PIPE, flags=NRT),
    "strips_no_terminal_edges": Case(lambda: small_wide_job(400, 370), STRIPED, STRIPS, flags=NTE),
    "strips_no_reduced_terminal": Case(lambda: small_wide_job(400, 370), STRIPED, STRIPS, flags=NRT),
    "tiles_no_terminal_edges": Case(lambda: small_wide_job(300, 280), TILED, TILES, flags=NTE),
    "tiles_no_reduced_terminal": Case(lambda: small_wide_job(300, 280), TILED, TILES, flags=NRT),
    # who wrote the back-pointers (test_who_wrote_the_back_pointers adds the followers)
    "bp_fill_ring": Case(lambda: banded_job(0), PIPE, {"PAGAN_DP_BP": "fill", "PAGAN_DP_FILL": "ring"}),
    "bp_pass": Case(lambda: banded_job(0), PIPE, {"PAGAN_DP_BP": "pass"}),
    # ties: the quantised maker; mc.assert_tie_rich holds for each (asserted here and in tests/test_oracle_matrices_cpu.py)
    "ties_banded": Case(lambda: mc.quantised(banded_job(0), 0), PIPE, plan=plan_classes({2, 3, 4})),
    "ties_stripe_three": Case(lambda: mc.quantised(test_wide_step_gpu.wide_job("three", 0), 1), TILED, plan=plan_wide("three")),
    "ties_strips": Case(lambda: mc.quantised(full_job(test_strips_gpu.CASES, "three_and_more_edges"), 2), STRIPED, STRIPS, plan=plan_strips(2)),
    "ties_tiles": Case(lambda: mc.quantised(full_job(test_tiles_gpu.CASES, "three_and_more_edges"), 3), TILED, TILES, plan=plan_tiles(16)),
}
TIE_CASES = sorted(n for n in CASES if n.startswith("ties_"))
COMPACT_CASES = {
    "compact_banded": Case(lambda: dead_job(True), PIPE),
    "compact_tiles": Case(lambda: dead_job(False), TILED, TILES),
}


@functools.lru_cache(maxsize=None)
def reference(oracle, name, flags):
    """(oracle.dp_matrices, oracle.dp_align) of a case's job: computed once, shared, never written to"""
    case = CASES.get(name) or COMPACT_CASES[name]
    left, right, model, band = case.job
    want = oracle.dp_matrices(left, right, model, band, flags=flags)
    for a in want.values():
        a.setflags(write=False)
    return want, oracle.dp_align(left, right, model, band, flags=flags)


def set_env(monkeypatch, case, compact=False):
    if not compact:
        monkeypatch.setenv("PAGAN_DP_COMPACT", "0")      # the device arrays are read back as the caller's matrices
    for key, value in case.env.items():
        monkeypatch.setenv(key, value)


def run_and_check(pg, oracle, name, case, runs=1, compact=None):
    want, path = reference(oracle, name, case.flags)
    b = pg.Batch([case.job], flags=case.flags)
    for _ in range(runs):
        assert pg.lib().pagan_batch_debug_poison(b._h) == 0
        b.run(); b.sync()
    mc.check_matrices(b, 0, case.job, want, case.flags, compact=compact)
    same(b.fetch()[0], path, name)
    b.close()


@pytest.mark.parametrize("name", sorted(CASES))
def test_every_stored_cell_equals_the_oracles(pg, oracle, monkeypatch, name):
    case = CASES[name]
    set_env(monkeypatch, case)
    case.assert_plan(pg)
    if name in TIE_CASES:
        mc.assert_tie_rich(case.job, reference(oracle, name, case.flags)[0])
    run_and_check(pg, oracle, name, case)


@pytest.mark.parametrize("follow", ["0", "1"])
def test_who_wrote_the_back_pointers(pg, oracle, monkeypatch, follow):
    """pg_backptr alone (PAGAN_DP_FOLLOW=0) and the follower workgroups behind the fill (1), run twice on one batch: the second
    run finds the first one's flags and words in the arena."""
    case = CASES["bp_pass"]
    set_env(monkeypatch, case)
    monkeypatch.setenv("PAGAN_DP_FOLLOW", follow)
    case.assert_plan(pg)
    want, path = reference(oracle, "bp_pass", 0)
    b = pg.Batch([case.job])
    for _ in range(2):
        assert pg.lib().pagan_batch_debug_poison(b._h) == 0
        b.run(); b.sync()
    done, total = b.debug_followed(0)
    assert total > 50 and (done >= 0.9 * total if follow == "1" else done == 0)
    mc.check_matrices(b, 0, case.job, want, 0)
    same(b.fetch()[0], path)
    b.close()


@pytest.mark.parametrize("name", sorted(COMPACT_CASES))
def test_compacted_jobs_on_their_kept_cells(pg, oracle, monkeypatch, name):
    """The product's default: the library aligns the graphs with their dead sites taken out, and the device arrays are in the
    compacted numbering.  pg.debug_compact maps them back (keep_*: the sites, slot_*: the edge slots); every kept cell is
    compared, the dropped rows and columns are exactly the dead sites, and the oracle has nothing but -inf there."""
    case = COMPACT_CASES[name]
    set_env(monkeypatch, case, compact=True)
    left, right, model, band = case.job
    route, compacted, _ = pg.debug_route(left, right, model, band)
    assert route == case.route and compacted
    comp = pg.debug_compact(left, right, band)
    want, _ = reference(oracle, name, 0)
    for g, keep, axis in ((left, comp["keep_left"], 0), (right, comp["keep_right"], 1)):
        dropped = np.setdiff1d(np.arange(g.n_sites), keep)
        assert np.array_equal(dropped, mc.dead_sites(g)) and dropped.size > 0.2 * g.n_sites
        i, j = mc.band_cells(left.n_sites - 1, right.n_sites - 1, band)
        gone = np.isin((i, j)[axis], dropped)
        assert gone.any() and np.all(want["score"][gone] == -np.inf) and np.all(want["ptr"][gone][:, :, 0] == -1)
    run_and_check(pg, oracle, name, case, compact=comp)


def test_three_routes_in_one_batch(pg, oracle, monkeypatch):
    """A banded job, a striped one and a tiled one side by side in one pg.Batch, each compared under its own index."""
    monkeypatch.setenv("PAGAN_DP_COMPACT", "0")
    jobs = test_routes_cpu.jobs()
    routes = [PIPE, STRIPED, TILED]
    batch = [jobs[r] for r in routes]
    for r, (left, right, model, band) in zip(routes, batch):
        assert pg.debug_route(left, right, model, band)[0] == r
    b = pg.Batch(batch)
    assert pg.lib().pagan_batch_debug_poison(b._h) == 0
    b.run(); b.sync()
    for k, job in enumerate(batch):
        mc.check_matrices(b, k, job, oracle.dp_matrices(*job), 0)
    res = b.fetch()
    for k, job in enumerate(batch):
        same(res[k], oracle.dp_align(*job), routes[k])
    b.close()
