"""The descriptor words of pg_fill_pipe (dp_plan.cpp: pack_pipe_descriptors), word for word against
tests/golden/pipe_descriptors.npz.  No GPU: pagan_dp_debug_descriptors is host code.

The words are the host-kernel contract of the banded fill's hot loop (word 4 of a diagonal: class in bits 0-3, bit 4, the
residency mask from bit 5 up with bit 5 for a far history, bit 19 for the lanes' third pass / a seven-wave wide run, a 12-bit
hop from bit 20; word 7: lead_req).  A lost bit 19 or history bit still gives bit-exact alignments, only slower, so nothing but
an equality test notices.  The fixture was recorded from the planner as it stood before the host side was split into
dp_plan.cpp (tests/golden/make_descriptor_golden.py has the provenance); the coverage test says what the set of jobs must
keep reaching if it is ever shortened."""
import os

import numpy as np
import pytest

from pagan2_msa_amd import abi, synth
from test_far_plan_cpu import job as far_job

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pipe_descriptors.npz")


def chain_job():
    rng = np.random.default_rng(2024)
    left = synth.chain_graph("".join(rng.choice(list("ACGT"), 600)))
    right = synth.chain_graph("".join(rng.choice(list("ACGT"), 620)))
    Lx, Ly = left.n_sites - 1, right.n_sites - 1
    centre = np.arange(Lx) * (Ly - 1) // (Lx - 1)
    upper = np.maximum.accumulate(np.maximum(centre - 20, 0)); lower = np.maximum.accumulate(np.minimum(centre + 20, Ly - 1))
    upper[0] = 0; lower[-1] = Ly - 1
    return left, right, abi.Band(upper, lower)


def box_job(n, seed_l, seed_r, r0, r1, widen):
    """test_far_plan_cpu's wide-box construction: a band of +-25 with rows r0:r1 widened into a box"""
    left = synth.random_graph(n, 15, seed_l, p_extra=0.03, max_deg=3, max_span=30)
    right = synth.random_graph(n, 15, seed_r, p_extra=0.03, max_deg=3, max_span=30)
    Lx, Ly = left.n_sites - 1, right.n_sites - 1
    centre = np.arange(Lx) * (Ly - 1) // max(Lx - 1, 1)
    upper = np.maximum(centre - 25, 0); lower = np.minimum(centre + 25, Ly - 1)
    upper[r0:r1] = upper[r0]; lower[r0:r1] = lower[r1 - 1] + widen
    upper = np.maximum.accumulate(upper); lower = np.maximum.accumulate(lower)
    upper[0] = 0; lower[-1] = Ly - 1
    return left, right, abi.Band(upper, lower)


def box_1800():
    return box_job(1800, 301, 401, 600, 900, 30)


# name: (job, states of the model, environment)
CASES = {
    "chain": (chain_job, 15, {}),
    "far": (lambda: far_job(0, n=600), 15, {}),
    "far_big_table": (lambda: far_job(0, n=600), 211, {}),
    "box_1800": (box_1800, 15, {}),
    "box_2400": (lambda: box_job(2400, 303, 403, 600, 1100, 300), 15, {}),
    "box_1800_wide7_off": (box_1800, 15, {"PAGAN_DP_WIDE7": "0"}),
    "box_1800_after_wide_reach": (box_1800, 15, {"PAGAN_DP_AFTER_WIDE": "reach"}),
    "box_1800_no_hist_no_three": (box_1800, 15, {"PAGAN_DP_HIST": "0", "PAGAN_DP_THREE": "0"}),
}


def words_of(pg, name, setenv):
    make, n_states, env = CASES[name]
    for k, v in env.items():
        setenv(k, v)
    left, right, band = make()
    return pg.debug_descriptors(left, right, band, n_states)


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


@pytest.mark.parametrize("name", sorted(CASES))
def test_descriptor_words_are_the_recorded_ones(pg, golden, monkeypatch, name):
    got = words_of(pg, name, monkeypatch.setenv)
    want = golden[name].T                     # stored [8, diagonals]
    assert got.shape == want.shape and got.shape[0] > 0, "the job is meant to be pg_fill_pipe's"
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert bad.size == 0, "%s: %d diagonals differ, the first is %d: %s != %s" % (name, bad.size, bad[0], got[bad[0]], want[bad[0]])


def test_the_fixture_covers_the_layout(golden):
    assert sorted(golden.files) == sorted(list(CASES) + ["n_states"])
    assert {15, 211} <= set(int(s) for s in golden["n_states"]), "both table sizes"
    w4 = np.concatenate([golden[name][4] for name in CASES]).view(np.uint32)
    assert set(int(c) for c in np.unique(w4 & 15)) == {0, 1, 2, 3, 4, 5}, "every class"
    for bit in (4, 5, 19):
        on = (w4 >> bit) & 1
        assert on.any() and not on.all(), "bit %d both set and clear" % bit
    hop = w4 >> 20
    assert (hop == 4095).any() and (hop < 4095).any(), "a saturated and an unsaturated hop"
