"""The segmented traceback (dp_kernels.hip: pg_trace_spec, pg_trace_compose, pg_trace_emit) on paths planted to leave through
every exit of its chase: tests/trace_scenarios.py builds the inputs, tests/test_trace_plan_cpu.py shows on the CPU that each
reaches the exit it is named for.  Every job is compared three ways: the alignment with the oracle's (bit-exact), the
device's trace with the oracle's visited cells, and the segments pg_trace_compose recorded with the predictor's
(tests/trace_plan.py) -- start cell, state, cells, offset and the number of boundaries."""
import numpy as np
import pytest

import trace_plan as tp
import trace_scenarios as ts

pytestmark = pytest.mark.gpu


def check_job(b, k, got, want, job, what):
    """job k of batch b after run + fetch against the oracle's result `want`"""
    left, right, _, band = job
    assert got.same_alignment(want), "%s: the alignment differs from the oracle's" % what
    n_bound, segs, n_cells, status = b.debug_segments(k)
    if want.status != 0:
        assert (status, len(segs), n_cells) == (1, 0, 0), what
        return
    cells, K, plan = ts.predict(want, left, right, band)
    assert status == 0 and n_bound == K, "%s: %d boundaries, predicted %d (status %d)" % (what, n_bound, K, status)
    assert n_cells == len(cells), "%s: %d cells on the path, the oracle visits %d" % (what, n_cells, len(cells))
    trace = b.debug_trace(k, n_cells)
    bad = np.nonzero((trace[:, 0] != cells[:, 0]) | (trace[:, 1] != cells[:, 1]) | ((trace[:, 2] & 3) != cells[:, 2]))[0]
    assert bad.size == 0, "%s: trace cell %d is %s, the oracle's %s" % (what, bad[0], trace[bad[0]].tolist(), cells[bad[0]].tolist())
    assert [tuple(r) for r in segs.tolist()] == plan["segments"], "%s: segments (hops %s)" % (what, plan["hops"])


def run_alone(pg, oracle, key, job):
    b = pg.Batch([job])
    try:
        b.run(); b.sync()
        got = b.fetch()[0]
        assert b.debug_reruns() == 0, "%s: the path check asked for a second run" % (key,)
        check_job(b, 0, got, ts.oracle_result(oracle, key, job), job, str(key))
    finally:
        b.close()


# (c) pure_diagonal: the band upper = lower = row, one cell per row -- the ABI and the oracle accept it; every odd diagonal,
# so one diagonal of every boundary pair, is empty.
@pytest.mark.parametrize("name", sorted(ts.SCENARIOS))
def test_a_planted_path_alone(pg, oracle, name):
    """(a) wide boundaries, (b) narrow ones, the comb and the gap runs, (c) the narrowest band, (d) the end of the path,
    (e) the switch at Lx + Ly = 2000: one job per batch."""
    run_alone(pg, oracle, name, ts.job(name))


def test_one_batch_of_mixed_jobs(pg, oracle):
    """(f) a job below the switch, a full matrix with many boundaries, narrow banded jobs and an unreachable one (status 1: the
    traceback kernels skip it) in one batch, in shuffled order: each comes out as it does alone."""
    names = ["switch_1999", "wide_left_land_rot0", "narrow_left_takeoff_rot1", "comb_narrow", "gap_run_y_narrow", "switch_2001",
             "unreachable", "stop_bypass_both_3_edges"]
    order = np.random.default_rng(5).permutation(len(names))
    names = [names[k] for k in order]
    jobs = [ts.unreachable_job() if n == "unreachable" else ts.job(n) for n in names]
    wants = [ts.oracle_result(oracle, n, j) for n, j in zip(names, jobs)]
    assert wants[names.index("unreachable")].status == 1
    b = pg.Batch(jobs)
    try:
        for rep in range(2):                             # (the second run finds the first one's tables and segments in the arena)
            b.run(); b.sync()
        got = b.fetch()
        assert b.debug_reruns() == 0
        for k, n in enumerate(names):
            check_job(b, k, got[k], wants[k], jobs[k], "job %d (%s)" % (k, n))
    finally:
        b.close()


@pytest.mark.parametrize("batch", range(ts.SWEEP_CASES // ts.SWEEP_BATCH))
def test_seeded_sweep(pg, oracle, batch):
    """(g) 0 .. 6 bypassed blocks of 1 .. 800 sites on either side or both, full matrices and bands of many widths; the
    CPU test shows that every case is reachable and that 24 of the 32 paths pass a pair without a cell on it."""
    cases = range(batch * ts.SWEEP_BATCH, (batch + 1) * ts.SWEEP_BATCH)
    jobs = [ts.sweep_job(c) for c in cases]
    b = pg.Batch(jobs)
    try:
        b.run(); b.sync()
        got = b.fetch()
        assert b.debug_reruns() == 0
        for k, c in enumerate(cases):
            check_job(b, k, got[k], ts.oracle_result(oracle, ("sweep", c), jobs[k]), jobs[k], "sweep case %d" % c)
    finally:
        b.close()


def test_a_back_pointer_that_names_the_other_edge_slot_is_seen(pg, oracle):
    """(h) On a planted full matrix, the back-pointer of every visited cell that leaves through a bypass is rewritten to name
    the site's other edge -- the chain edge into the junk block, a valid pointer to a valid cell -- between fill and
    traceback.  pg_trace_check must see each (one re-run), and the result must stay the oracle's."""
    name = "wide_left_land_rot0"
    job = ts.job(name)
    left = job[0]
    want = ts.oracle_result(oracle, name, job)
    cells = tp.visited_cells(want)
    b = pg.Batch([job])
    try:
        b.run(); b.sync()
        assert b.fetch()[0].same_alignment(want) and b.debug_reruns() == 0
        trace = b.debug_trace(0, len(cells))
        through = [t for t in range(len(cells) - 1) if cells[t][0] - cells[t + 1][0] > 1]
        assert len(through) >= 4, "the job has bypassed blocks of 3, 40, 300 and 700 sites"
        for t in through:
            i, j, w = (int(v) for v in trace[t])
            w &= 0xffffffff
            assert (i, j, w & 3) == tuple(int(v) for v in cells[t]) and (w & 3) == tp.M_MAT
            first = int(left.bwd_off[i])
            assert int(left.bwd_off[i + 1]) - first == 2
            k1 = (w >> 4) & 16383
            assert int(left.bwd_src[first + k1]) == int(cells[t + 1][0]) and not (w & 4), "the path takes the long edge"
            other = 1 - k1
            assert int(left.bwd_src[first + other]) == i - 1
            frm = int(trace[t + 1][2]) & 3                   # a cell's `from` label is the next visited cell's matrix
            word = frm | 4 | (w & 8) | (other << 4) | (w & 0xfffc0000)
            before = b.debug_reruns()
            b.debug_poke_bp(0, i, j, tp.M_MAT, word)
            b.run(); b.sync()
            got = b.fetch()[0]
            assert b.debug_reruns() == before + 1, "the other edge slot at visited cell %d (%d, %d) went unnoticed" % (t, i, j)
            check_job(b, 0, got, want, job, "after the re-run for cell %d" % t)
    finally:
        b.close()
