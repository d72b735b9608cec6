"""CPU: the planted inputs of tests/parent_scenarios.py through the three CPU texts of the parent-graph builder -- the
product's host builder (HGraph.parent), the oracle (OGraph.parent) and the Python reading (pycheck_parent) -- field by field,
floats as bits; the rules each scenario is there for, counted on the Python reading; the validator and the hand-path
deriver that stand in front of every builder; and the claim that made all this necessary: the random walks of
tests/test_parent_gpu.py reach none of the rules below."""
import collections

import numpy as np
import pytest

import parent_scenarios as ps
import pycheck_parent as pp
from pagan2_msa_amd import host, synth
from test_host_cpu import base_freq, same_graph
from test_pycheck_parent_cpu import same_dump

UNIFORM = np.full(4, 0.25, np.float32)


def host_parsimony(oracle):
    pars = host.dna_model(UNIFORM, 0.1)[1]
    assert np.array_equal(np.asarray(pars, np.int32).ravel(), oracle.dna_parsimony().ravel())
    return pars


@pytest.mark.parametrize("scn", ps.SCENARIOS, ids=repr)
def test_scenario_through_host_oracle_and_python(oracle, pg, scn):
    seqs, levels = ps.realise(scn, oracle, host)
    pars = host_parsimony(oracle)
    pys, total, _per = ps.python_chain(scn, levels)
    def build(hl, hr, lv, k):
        return host.HGraph.parent(hl, hr, lv.path, lv.lbl, lv.rbl, pars, 4, lv.flags)
    for k, lv, hp in ps.host_chain(scn, seqs, levels, host, build):
        same_graph(hp, lv.parent, "%s level %d, host against oracle" % (scn, k + 1))
        same_dump(pys[k], lv.parent, "%s level %d, Python against oracle" % (scn, k + 1))
    for rule in scn.rules:
        assert total[rule] > 0, "%s does not reach %s: %s" % (scn, rule, dict(total))


@pytest.mark.parametrize("scn", ps.SIZES, ids=repr)
def test_tiled_sizes_host_against_oracle(oracle, pg, scn):
    seqs, levels = ps.realise(scn, oracle, host)
    pars = host_parsimony(oracle)
    def build(hl, hr, lv, k):
        return host.HGraph.parent(hl, hr, lv.path, lv.lbl, lv.rbl, pars, 4, lv.flags)
    for k, lv, hp in ps.host_chain(scn, seqs, levels, host, build):
        same_graph(hp, lv.parent, "%s level %d" % (scn, k + 1))
    top = levels[ps.DELETING_LEVEL - 1].parent.attrs()
    assert top[0].shape[0] == scn.expect["n"]
    assert ps.run_structure(top) == (scn.expect["runs"], scn.expect["deleted"])


def test_one_tile_is_the_coupled_chain(oracle, pg):
    """What the tiled builds repeat: per tile two runs at the deleting level, three deleted sites -- two from the run that
    goes on its own, one from the run that goes only because the first did (against the undeleted lists it stays: a
    builder that evaluated the runs side by side and stopped there would delete two sites per tile, not three)."""
    scn = ps.BY_NAME["coupled_matched_site_edge"]
    _seqs, levels = ps.realise(scn, oracle, host)
    _pys, _total, per = ps.python_chain(scn, levels)
    c = per[ps.DELETING_LEVEL - 1]
    assert c["pass2_runs"] == ps.TILE_RUNS and c["coupling_matched_site_edge_lost"] == 1 and c["pass2_delete_whole_run"] == 2
    top = levels[ps.DELETING_LEVEL - 1].parent.attrs()
    assert top[0].shape[0] == ps.TILE_SITES + 2 and ps.run_structure(top) == (ps.TILE_RUNS, ps.TILE_DELETED)
    big = ps.SIZES[-1]
    assert big.expect["runs"] > 1024 + 2 and big.expect["n"] > 3 * 1024          # coupled pairs behind the 1024th run


def test_three_runs_decide_each_other_in_turn(oracle, pg):
    """At its last level the chain has three runs and all three go; the second and the third each decide otherwise than
    against the undeleted lists, and the third's edge is lost to the SECOND run's deletion, which the first brought about."""
    scn = ps.BY_NAME["three_runs_in_a_chain"]
    _seqs, levels = ps.realise(scn, oracle, host)
    _pys, _total, per = ps.python_chain(scn, levels)
    assert [c["pass2_delete_whole_run"] for c in per[:-1]] == [0] * (len(per) - 1)
    last = per[-1]
    assert last["pass2_runs"] == 3 and last["pass2_delete_whole_run"] == 3 and last["coupling_matched_site_edge_lost"] == 2
    sa, _sd, ea, _ef = levels[-1].parent.attrs()
    gone = np.nonzero(sa[:, 1] == pp.non_real)[0].tolist()
    assert gone == [2, 3, 5, 6, 8]
    lost = [(int(e[0]), int(e[1])) for e in ea if e[5] == 0 and e[1] - e[0] > 1 and e[0] in gone]
    assert (2, 7) in lost and (5, 9) in lost                            # d -> n1 and e -> n3


def test_every_rule_is_reached_or_argued_unreachable():
    named = collections.Counter(r for s in ps.SCENARIOS for r in s.rules)
    missing = [r for r in pp.RULES if r != "pass2_runs" and not named[r] and r not in ps.UNREACHABLE]
    assert not missing, missing
    assert not [r for r in ps.UNREACHABLE if named[r]], "listed as unreachable and reached"
    for r in ("coupling_own_first_edge_lost", "coupling_matched_site_edge_lost", "pass2_delete_prefix_of_run",
              "stop_shorten_new_beside_others"):
        assert named[r], r


def test_a_parent_above_non_real_sites(oracle, pg):
    """The level above the deleting one: its child holds non_real sites, which no path visits and for which the device
    builder's child -> parent maps are never written.  The scenario's last level is that build and goes through every
    builder with the rest; here only that the input is what it is meant to be."""
    scn = ps.BY_NAME["coupled_matched_site_edge"]
    _seqs, levels = ps.realise(scn, oracle, host)
    assert len(levels) == ps.DELETING_LEVEL + 1
    child = levels[-1].left.attrs()[0]
    assert (child[:, 1] == 5).sum() == ps.TILE_DELETED and levels[-1].left_leaf is None
    cols = levels[-1].path.cols
    assert not set(np.nonzero(child[:, 1] == 5)[0].tolist()) & set(cols[np.isin(cols[:, 2], (2, 3)), 0].tolist())


# ---- the gate ----
def test_validator_refuses_what_no_builder_checks(oracle, pg):
    scn = ps.BY_NAME["coupled_matched_site_edge"]
    _seqs, levels = ps.realise(scn, oracle, host)
    lv = levels[6]                                                      # M x x M x M: skip columns on the left
    L, R, good = lv.left.flatten(), lv.right.flatten(), lv.path
    ps.validate(good, L, R)
    cols = good.cols.copy()
    assert cols[:, 2].tolist().count(ps.XSKIPPED) == 3
    def bad(c=None, lu=None, ru=None):
        p = ps.Path(cols if c is None else c, good.left_used if lu is None else lu, good.right_used if ru is None else ru)
        with pytest.raises(ValueError):
            ps.validate(p, L, R)
    c = cols.copy(); c[0, 2] = 7; bad(c)                                # a path state outside 2..6
    c = cols.copy(); c[0, 2] = ps.XGAPPED; bad(c)                       # a state that does not fit the column's children
    c = cols.copy(); c[[1, 2]] = c[[2, 1]]; bad(c)                      # not monotone
    bad(cols[:-1])                                                      # a child site left over
    k = cols[:, 2].tolist().index(ps.XSKIPPED)
    c = cols.copy(); c[k, 2] = ps.XGAPPED; bad(c)                       # visits a site no edge leads to from there
    bad(lu=good.left_used[:-1])                                         # a used edge missing
    bad(lu=np.append(good.left_used[:-1], [int(L.n_edges) - 1 if int(L.n_edges) - 1 not in good.left_used else 0]))
    bad(ru=good.right_used[1:])
    # (skip columns in the wrong order: test_hand_path_deriver_reproduces_the_aligner, where both children have some)


def test_hand_path_deriver_reproduces_the_aligner(oracle, pg):
    """From the visited cells alone, derive() gives the oracle DP's columns and used edges exactly -- at every node of the
    random walks the suite already has (a balanced tree with skip columns on both sides, a caterpillar)."""
    checked = {"nodes": 0, "xskips": 0, "yskips": 0, "swapped": 0}
    def walk(tree, by_name, bf):
        def rec(t):
            if t[0] == "leaf":
                return oracle.OGraph.leaf(by_name[t[1]], oracle.DNA_ALPHABET, 0), min(max(t[2], 0.001), 0.2)
            ol, dl = rec(t[1])
            orr, dr = rec(t[2])
            model, _ = host.dna_model(bf, dl + dr)
            L, R = ol.flatten(), orr.flatten()
            res = oracle.dp_align(L, R, model)
            want = ps.Path(res.cols, res.left_used, res.right_used)
            assert ps.derive(ps.visited_cells(res.cols), L, R).same(want)
            ps.validate(want, L, R)
            st = res.cols[:, 2].tolist()
            for k in range(len(st) - 1):                                # right child's skips, then left's: swapped is refused
                if st[k] == ps.YSKIPPED and st[k + 1] == ps.XSKIPPED:
                    c = res.cols.copy()
                    c[[k, k + 1]] = c[[k + 1, k]]
                    with pytest.raises(ValueError):
                        ps.validate(ps.Path(c, res.left_used, res.right_used), L, R)
                    checked["swapped"] += 1
            checked["nodes"] += 1
            checked["xskips"] += int((res.cols[:, 2] == ps.XSKIPPED).sum())
            checked["yskips"] += int((res.cols[:, 2] == ps.YSKIPPED).sum())
            return oracle.OGraph.parent(ol, orr, res, dl, dr, oracle.dna_parsimony(), 4, 0), min(max(t[3], 0.001), 0.2)
        rec(tree)
    names, seqs, nwk = synth.evolve_balanced(16, 160, branch=0.05, sub=0.05, indel_start=0.012, mean_len=6, seed=3)
    walk(synth.parse_newick(nwk), dict(zip(names, seqs)), base_freq(seqs))
    names, seqs, nwk = synth.evolve_caterpillar(14, 150, seed=2)
    walk(synth.parse_newick(nwk), dict(zip(names, seqs)), base_freq(seqs))
    assert checked["nodes"] == 28 and checked["xskips"] > 20 and checked["yskips"] > 5 and checked["swapped"] > 0, checked


# ---- why the planted inputs are needed ----
NOT_REACHED_BY_THE_WALKS = ("coupling_own_first_edge_lost", "coupling_matched_site_edge_lost", "pass2_delete_prefix_of_run",
                            "pass2_edge_starts_before_run", "pass2_over_limit_then_stop_site", "stop_shorten_new",
                            "stop_shorten_new_beside_others", "drop_distance", "history_ends_differ_used")


def test_the_random_walks_of_test_parent_gpu_reach_none_of_this(oracle, pg):
    """The inputs of tests/test_parent_gpu.py (DNA ones; the protein walk differs in its states only) through the counting
    Python reading, clamped branches and all: deletions happen, and each one takes a whole run, decided in the first round."""
    total = collections.Counter()
    def walk(tree, by_name, bf, flags=0, band=False, leaf_flags=0):
        anc_alpha = host.alphabets(1)[1]
        def rec(t):
            if t[0] == "leaf":
                return oracle.OGraph.leaf(by_name[t[1]], oracle.DNA_ALPHABET, leaf_flags), (min(max(t[2], 0.001), 0.2) if t[2] > 0 else 0.001)
            ol, dl = rec(t[1])
            orr, dr = rec(t[2])
            model, _ = host.dna_model(bf, dl + dr)
            b = oracle.define_tunnel(ol, orr, alphabet=anc_alpha)[0] if band else None
            res = oracle.dp_align(ol.flatten(), orr.flatten(), model, b)
            pl, pr = (pp.Sequence.from_dump(g.flatten(), g.attrs(), g.fwd()) for g in (ol, orr))
            pp.build_parent(pl, pr, res.cols, res.left_used, res.right_used, dl, dr, oracle.dna_parsimony(), 4, flags, counter=total)
            d = t[3]
            return oracle.OGraph.parent(ol, orr, res, dl, dr, oracle.dna_parsimony(), 4, flags), (0.001 if d <= 0 else min(d, 0.2))
        rec(tree)
    def go(evolved, **kw):
        names, seqs, nwk = evolved
        walk(synth.parse_newick(nwk), dict(zip(names, seqs)), base_freq(seqs), **kw)
    go(synth.evolve_balanced(16, 160, branch=0.05, sub=0.05, indel_start=0.012, mean_len=6, seed=3))
    go(synth.evolve_balanced(64, 150, branch=0.03, sub=0.03, indel_start=0.02, mean_len=3, seed=21))
    for flags in (0, 1, 2):
        go(synth.evolve_balanced(8, 400, branch=0.02, sub=0.015, indel_start=0.004, mean_len=5, seed=5), flags=flags, band=True)
    for n, seed in ((14, 2), (18, 6)):
        go(synth.evolve_caterpillar(n, 150, seed=seed))
    names, seqs, nwk = synth.evolve_balanced(8, 200, branch=0.03, sub=0.02, indel_start=0.01, mean_len=3, seed=8)
    seqs = [s.replace("AC", "AAAC", 3).replace("GT", "GGGGGT", 2) for s in seqs]
    for leaf_flags in (1, 2):
        go((names, seqs, nwk), leaf_flags=leaf_flags)
    assert total["pass2_delete_whole_run"] > 0 and total["stop_shorten_dup"] > 0
    reached = {r: total[r] for r in NOT_REACHED_BY_THE_WALKS if total[r]}
    assert not reached, reached
