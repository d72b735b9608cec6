"""The traceback predictor (tests/trace_plan.py) on hand-worked paths, the planted-graph generator, and the preconditions
of tests/test_trace_gpu.py: every scenario of tests/trace_scenarios.py, run on the oracle and the predictor alone, reaches
the exit of pg_trace_spec / pg_trace_compose it is named for."""
import types

import numpy as np
import pytest

from pagan2_msa_amd import synth

import trace_plan as tp
import trace_scenarios as ts


# ---- hand-worked cases: segments of 8 diagonals, pairs {8, 7}, {16, 15}, {24, 23}, ... ------------------------------------------
@pytest.fixture
def seg8(monkeypatch):
    monkeypatch.setattr(tp, "SEG", 8)


def path(ds, state=tp.M_MAT):
    """a path given by the diagonals of its cells, end -> start (the predictor reads nothing but i + j of a cell)"""
    return np.array([((d + 1) // 2, d // 2, state) for d in ds], np.int32)


def cell(d, state=tp.M_MAT):
    return ((d + 1) // 2, d // 2, state)


WIDE, NARROW = np.full(64, 1000), np.full(64, 1)


def test_a_jump_that_lands_one_above_the_pair(seg8):
    ds = [30, 28, 26, 24, 22, 20, 17, 15, 13, 11, 9, 7, 5, 3, 1]
    p = tp.plan(path(ds), WIDE, 3)
    assert p["serial"] == [0, 1, 2]                                      # 30, 28, 26: above the top pair
    assert p["segments"] == [cell(24) + (4, 3), cell(15) + (4, 7), cell(7) + (4, 11)]
    assert p["hops"] == [(3, tp.ENTRY, 0), (2, tp.ENTRY, 0), (1, tp.DONE, 0)]
    assert p == tp.plan(path(ds), NARROW, 3)


def test_a_jump_that_lands_on_either_diagonal_of_the_pair(seg8):
    on_d = [30, 28, 26, 24, 22, 20, 16, 14, 12, 10, 8, 6, 4, 2]
    p = tp.plan(path(on_d), WIDE, 3)
    assert p["segments"] == [cell(24) + (3, 3), cell(16) + (4, 6), cell(8) + (4, 10)]
    assert p["hops"] == [(3, tp.ENTRY, 0), (2, tp.ENTRY, 0), (1, tp.DONE, 0)] and p["serial"] == [0, 1, 2]
    below = [30, 28, 26, 24, 22, 20, 15, 13, 11, 9, 7, 5, 3, 1]
    p = tp.plan(path(below), WIDE, 3)
    assert p["segments"] == [cell(24) + (3, 3), cell(15) + (4, 6), cell(7) + (4, 10)]
    assert p["hops"] == [(3, tp.ENTRY, 0), (2, tp.ENTRY, 0), (1, tp.DONE, 0)] and p["serial"] == [0, 1, 2]


def test_a_jump_that_lands_one_below_the_pair(seg8):
    ds = [30, 28, 26, 24, 22, 20, 14, 12, 10, 8, 6, 4, 2]
    p = tp.plan(path(ds), WIDE, 3)                                       # wide: the entry gives up, one lane walks 14, 12, 10
    assert p["segments"] == [cell(24) + (3, 3), cell(8) + (4, 9)]
    assert p["hops"] == [(3, tp.MISS_WIDE, 0), (1, tp.DONE, 0)] and p["serial"] == [0, 1, 2, 6, 7, 8]
    p = tp.plan(path(ds), NARROW, 3)                                     # narrow: the chase goes on to pair 1
    assert p["segments"] == [cell(24) + (6, 3), cell(8) + (4, 9)]
    assert p["hops"] == [(3, tp.ENTRY, 1), (1, tp.DONE, 0)] and p["serial"] == [0, 1, 2]
    assert tp.pairs_passed_without_a_cell(path(ds), 3) == [2]


def test_a_jump_over_two_pairs(seg8):
    ds = [38, 36, 34, 32, 30, 28, 10, 8, 6, 4, 2]
    p = tp.plan(path(ds), NARROW, 4)
    assert p["segments"] == [cell(32) + (4, 3), cell(8) + (4, 7)]
    assert p["hops"] == [(4, tp.ENTRY, 2), (1, tp.DONE, 0)] and p["serial"] == [0, 1, 2]
    p = tp.plan(path(ds), WIDE, 4)
    assert p["segments"] == [cell(32) + (3, 3), cell(8) + (4, 7)]
    assert p["hops"] == [(4, tp.MISS_WIDE, 0), (1, tp.DONE, 0)] and p["serial"] == [0, 1, 2, 6]
    assert tp.pairs_passed_without_a_cell(path(ds), 4) == [2, 3]
    onto = [38, 36, 34, 32, 30, 28, 8, 6, 4, 2]                          # ... and straight onto the third
    p = tp.plan(path(onto), NARROW, 4)
    assert p["segments"] == [cell(32) + (3, 3), cell(8) + (4, 6)] and p["hops"][0] == (4, tp.ENTRY, 2)
    past = [38, 36, 34, 32, 30, 28, 4, 2]                                # ... and past every pair: the chase runs to the start
    p = tp.plan(path(past), NARROW, 4)
    assert p["segments"] == [cell(32) + (5, 3)] and p["hops"] == [(4, tp.DONE, 3)]
    p = tp.plan(path(past), WIDE, 4)
    assert p["segments"] == [cell(32) + (3, 3)] and p["hops"] == [(4, tp.MISS_WIDE, 0)] and p["serial"] == [0, 1, 2, 6, 7]


def test_a_chain_that_meets_the_step_cap(seg8):
    """a gap run (one diagonal per cell) that leaves every pair out through a long edge: 16 cells after pair 5 the chase has
    followed over pairs 4 and 3 and is given up on diagonal 20; one lane walks 20 .. 17 and 14 .. 9, pair 1 ends the path"""
    ds = list(range(40, 32, -1)) + list(range(30, 24, -1)) + list(range(22, 16, -1)) + list(range(14, 0, -1))
    p = tp.plan(path(ds, tp.X_MAT), NARROW, 5)
    assert p["segments"] == [cell(40, tp.X_MAT) + (16, 0), cell(8, tp.X_MAT) + (8, 26)]
    assert p["hops"] == [(5, tp.MISS_CAP, 2), (1, tp.DONE, 0)]
    assert p["serial"] == list(range(16, 26)) and p["n_cells"] == 34
    p = tp.plan(path(ds, tp.X_MAT), WIDE, 5)                             # wide: given up at the first pair it misses
    assert p["segments"][0] == cell(40, tp.X_MAT) + (8, 0) and p["hops"][0] == (5, tp.MISS_WIDE, 0)
    assert p["serial"] == list(range(8, 26))


def test_boundaries_above_the_job_s_count_are_none(seg8):
    assert [tp.boundary_of(d, 2) for d in (0, 7, 8, 9, 15, 16, 23, 24)] == [0, 1, 1, 0, 2, 2, 0, 0]
    p = tp.plan(path([23, 21, 19, 17, 15, 13]), WIDE, 2)                # diagonal 23 would belong to pair 3
    assert p["serial"] == [0, 1, 2, 3] and p["segments"] == [cell(15) + (2, 4)]


# ---- the host's rule -----------------------------------------------------------------------------------------------------------
def test_the_switch_below_2000_and_for_very_wide_matrices():
    w = tp.diagonal_widths(1000, 999)
    assert tp.n_boundaries(1000, 999, w) == 0
    assert tp.n_boundaries(1000, 1000, tp.diagonal_widths(1000, 1000)) == 7            # nd - 1 = 1998 = 7 * 256 + 206
    assert tp.n_boundaries(1025, 1025, tp.diagonal_widths(1025, 1025)) == 8            # nd - 1 = 2048: diagonal 2048 exists
    assert tp.n_boundaries(1025, 1024, tp.diagonal_widths(1025, 1024)) == 7
    # Lx + Ly = 4000: K = 15, 30 W cells on the pairs, 7680 W chase steps against 20000 * 4000
    assert tp.n_boundaries(2000, 2000, np.full(3999, 10416)) == 15
    assert tp.n_boundaries(2000, 2000, np.full(3999, 10417)) == 0
    # full matrices n x n: a pair holds n cells on average, so (2 n K) * 256 chase steps with K = n / 128 stand against
    # 20000 * 2 n: the serial chase takes over from about n = 20000 -- "ten thousand cells wide on average"
    assert tp.n_boundaries(16000, 16000, tp.diagonal_widths(16000, 16000)) == 124
    assert tp.n_boundaries(24000, 24000, tp.diagonal_widths(24000, 24000)) == 0


def test_diagonal_widths_of_a_matrix_and_of_a_band():
    assert tp.diagonal_widths(3, 4).tolist() == [1, 2, 3, 3, 2, 1]
    rows = np.arange(4)
    assert tp.diagonal_widths(4, 4, (rows, rows)).tolist() == [1, 0, 1, 0, 1, 0, 1]
    # rows hold the columns 0-1, 0-2, 1-5, 4-5 (bounds clamped to the matrix)
    assert tp.diagonal_widths(4, 6, ([-3, 0, 1, 4], [1, 2, 9, 9])).tolist() == [1, 2, 1, 2, 1, 1, 1, 2, 1]


def test_visited_cells_of_a_result():
    cols = np.array([(1, 1, 2), (2, -1, 5), (3, -1, 5), (4, 2, 2), (5, -1, 3), (-1, 3, 6), (-1, 4, 4)], np.int32)
    res = types.SimpleNamespace(cols=cols, end=(tp.Y_MAT, 5, 4, -1, -1))
    assert tp.visited_cells(res).tolist() == [[5, 4, tp.Y_MAT], [5, 2, tp.X_MAT], [4, 2, tp.M_MAT], [1, 1, tp.M_MAT]]


# ---- the generator -------------------------------------------------------------------------------------------------------------
def test_planted_graph_is_a_chain_with_one_long_edge_per_block():
    core = np.arange(10) % 4
    slots = set()
    for seed in range(8):
        g = synth.planted_graph(core, [(3, 5), (10, 2)], seed)
        assert g.n_sites == 1 + 10 + 7 + 1 and g.state[0] == -1 and g.state[-1] == -1
        assert g.state[[1, 2, 3, 9, 10]].tolist() == [0, 1, 2, 3, 0] and np.all((g.state[4:9] >= 0) & (g.state[4:9] < 4))
        deg = np.diff(g.bwd_off)
        assert deg[0] == 0 and sorted(np.nonzero(deg == 2)[0].tolist()) == [9, 18] and set(deg[1:].tolist()) == {1, 2}
        for s, far in ((9, 3), (18, 15)):                                # site 9 = core 4; site 18 = the stop site
            srcs = g.bwd_src[g.bwd_off[s]:g.bwd_off[s + 1]].tolist()
            assert sorted(srcs) == [far, s - 1]
            slots.add((s, srcs.index(far)))
        assert sorted(g.bwd_eid.tolist()) == list(range(1, g.n_edges)) and np.all(g.bwd_logw == 0)
        for s in range(1, g.n_sites):
            assert np.all(g.bwd_src[g.bwd_off[s]:g.bwd_off[s + 1]] < s)
    assert slots == {(9, 0), (9, 1), (18, 0), (18, 1)}, "the long edge must come first and second"
    assert synth.planted_graph(core, [], 0).bwd_src.tolist() == synth.Graph.chain(core).bwd_src.tolist()


@pytest.mark.parametrize("blocks", [[(100, 3)], [(100, 40)], [(40, 6), (90, 6), (140, 6)], [(300, 7)]])
def test_the_oracle_takes_every_bypass(oracle, blocks):
    """the best path matches core to core; every block comes out as x-skipped columns (kind 5)"""
    core = ts.core_states(300, 5)
    left, right = synth.planted_graph(core, blocks, 1), synth.Graph.chain(core)
    res = oracle.dp_align(left, right, ts.model())
    kinds = np.bincount(res.cols[:, 2], minlength=7)
    assert res.status == 0 and kinds[2] == 300 and kinds[5] == sum(n for _, n in blocks) and kinds[[3, 4, 6]].sum() == 0
    res = oracle.dp_align(right, left, ts.model())
    kinds = np.bincount(res.cols[:, 2], minlength=7)
    assert res.status == 0 and kinds[2] == 300 and kinds[6] == sum(n for _, n in blocks) and kinds[[3, 4, 5]].sum() == 0


# ---- preconditions of the GPU scenarios --------------------------------------------------------------------------------------
def scenario_facts(oracle, name):
    left, right, _, band = ts.job(name)
    res = ts.oracle_result(oracle, name, ts.job(name))
    assert res.status == 0, name
    cells, K, plan = ts.predict(res, left, right, band)
    return cells, K, plan, ts.tags(cells, K, plan, left, right)


@pytest.mark.parametrize("name", sorted(ts.SCENARIOS))
def test_a_scenario_reaches_the_exit_it_is_named_for(oracle, name):
    _, expect, want_jumps = ts.SCENARIOS[name]
    cells, K, plan, tags = scenario_facts(oracle, name)
    assert expect <= tags, "%s: %s not reached (%s)" % (name, sorted(expect - tags), sorted(tags))
    got = ts.jump_residues(cells)
    assert all(j in got for j in want_jumps), "%s: jumps %s, wanted %s" % (name, sorted(got), want_jumps)
    left, right, _, band = ts.job(name)
    if name.startswith("wide_") or name.startswith("narrow_"):
        widths = tp.diagonal_widths(left.n_sites - 1, right.n_sites - 1, ts.band_arrays(band))
        on_pairs = [3 * (max(widths[k * 256], 0) + max(widths[k * 256 - 1], 0)) for k in range(1, K + 1)]
        if band is None:
            assert max(on_pairs) > tp.FOLLOW_ENTRIES and left.n_sites * right.n_sites <= 2.4e6
        else:
            assert max(on_pairs) <= tp.FOLLOW_ENTRIES
    if name.startswith("switch_"):
        assert K == (0 if name == "switch_1999" else 7) and left.n_sites + right.n_sites - 2 == int(name[7:])
        assert ts.jumps(cells) and ts.jumps(cells)[0][0] > 3 * 256 and ts.jumps(cells)[0][1] < 3 * 256 - 1
    if name.startswith("end_residue_"):
        assert (int(cells[0][0]) + int(cells[0][1])) % 256 == int(name.split("_")[2]) and not ts.jumps(cells)[1:]
    if name.startswith("stop_bypass_"):
        for g, on in ((left, "left" in name or "both" in name), (right, "right" in name or "both" in name)):
            assert g.bwd_off[-1] - g.bwd_off[-2] == (1 if not on else (3 if "3_edges" in name else 2))
    if name == "pure_diagonal":
        assert set(tp.diagonal_widths(left.n_sites - 1, right.n_sites - 1, ts.band_arrays(band)).tolist()) == {0, 1}


def test_the_scenarios_cover_every_exit(oracle):
    seen = set()
    for name in ts.SCENARIOS:
        seen |= scenario_facts(oracle, name)[3]
    assert seen >= {"entry", "follow1", "follow2", "miss_wide", "miss_cap", "done", "serial_mid_path", "gap_jump_over_pair",
                    "end_below_last"}, sorted(seen)


def test_the_sweep_s_seed_does_what_it_was_chosen_for(oracle):
    """32 cases, every one reachable, and in at least 24 the path passes a boundary pair without a cell on it"""
    passed = 0
    for case in range(ts.SWEEP_CASES):
        left, right, _, band = ts.sweep_job(case)
        assert left.n_sites + right.n_sites - 2 >= tp.SERIAL_MIN
        res = ts.oracle_result(oracle, ("sweep", case), ts.sweep_job(case))
        assert res.status == 0, case
        cells, K, plan = ts.predict(res, left, right, band)
        passed += bool(tp.pairs_passed_without_a_cell(cells, K))
    assert passed >= 24, passed
