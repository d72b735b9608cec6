"""The device's parent-graph builder (csrc/dp_parent.hip) on the planted inputs of tests/parent_scenarios.py: the rules no
random walk reaches -- runs of skipped sites whose deletion decides a later run (the fixpoint of pp_bound), a run deleted
in part or not at all, the stop site's shortened edges landing in another site's list, the distance and count limits, a
used edge between unequal sites -- and the sizes at which its scans and strided loops take another path (1023 .. 3073
sites, more than 1024 runs).  Every build is held, field by field and floats as bits, against the oracle's and (the small
ones) the Python reading's, its build_info against the reading's runs and deletions, and built twice.

Two ways of handing in the children: "resident" chains the device's own outputs upward (their used marks are set by
pp_mark_used); "uploaded" hands in host-built children at every level (the upload brings the marks)."""
import numpy as np
import pytest

import parent_scenarios as ps
from pagan2_msa_amd import host
from test_host_cpu import same_graph
from test_pycheck_parent_cpu import same_dump

pytestmark = pytest.mark.gpu

UNIFORM = np.full(4, 0.25, np.float32)


def dump_bytes(g):
    f = g.flatten()
    parts = [f.state, f.bwd_off, f.bwd_src, f.bwd_logw, f.bwd_eid] + list(g.attrs()) + list(g.fwd())
    return b"|".join(np.ascontiguousarray(a).tobytes() for a in parts)


def device_chain(scn, oracle, mode):
    seqs, levels = ps.realise(scn, oracle, host)
    pars = host.dna_model(UNIFORM, 0.1)[1]
    pys = ps.python_chain(scn, levels, with_counts=False)[0] if scn.python else None
    twin = {}

    def build(hl, hr, lv, k):
        if mode == "uploaded" and k > 0:                                 # the host builder's graph of the level below instead
            hl, hr = (twin["p"] if lv.left_leaf is None else hl), (twin["p"] if lv.right_leaf is None else hr)
        if mode == "uploaded":
            twin["next"] = host.HGraph.parent(hl, hr, lv.path, lv.lbl, lv.rbl, pars, 4, lv.flags)
        hp = host.HGraph.parent_device(hl, hr, lv.path, lv.lbl, lv.rbl, pars, 4, lv.flags)
        again = host.HGraph.parent_device(hl, hr, lv.path, lv.lbl, lv.rbl, pars, 4, lv.flags)
        assert dump_bytes(hp) == dump_bytes(again), "%s level %d: two builds differ" % (scn, k + 1)
        assert hp.build_info[:1] + hp.build_info[2:] == again.build_info[:1] + again.build_info[2:]
        if mode == "uploaded":
            twin["p"] = twin["next"]
        return hp

    deleted = 0
    for k, lv, hp in ps.host_chain(scn, seqs, levels, host, build):
        what = "%s level %d (%s children)" % (scn, k + 1, mode)
        same_graph(hp, lv.parent, what + ", device against oracle")
        if pys is not None:
            same_dump(pys[k], hp, what + ", Python against device")
        runs, rounds, gone, outside, patched = hp.build_info
        assert (runs, gone) == ps.run_structure(lv.parent.attrs()), what
        assert outside == 0 and patched == 0 and rounds >= 1, what
        deleted += gone
    return levels, deleted


@pytest.mark.parametrize("mode", ["resident", "uploaded"])
@pytest.mark.parametrize("scn", ps.SCENARIOS, ids=repr)
def test_planted_scenario(oracle, pg, scn, mode):
    levels, deleted = device_chain(scn, oracle, mode)
    if any(r.startswith("pass2_delete") for r in scn.rules):
        assert deleted > 0


@pytest.mark.parametrize("mode", ["resident", "uploaded"])
@pytest.mark.parametrize("scn", ps.SIZES, ids=repr)
def test_tiled_sizes(oracle, pg, scn, mode):
    """k tiles of the coupled chain: at the deleting level every tile's second run goes only because its first did."""
    levels, deleted = device_chain(scn, oracle, mode)
    top = levels[ps.DELETING_LEVEL - 1].parent.attrs()
    assert top[0].shape[0] == scn.expect["n"] and ps.run_structure(top) == (scn.expect["runs"], scn.expect["deleted"])
    assert deleted == scn.expect["deleted"]
