"""GPU: pg_fb_counts (dp_fb_counts.inc) -- expected transition, end and emission counts -- against the exact reading
(tests/pycheck_counts.py: path sums in 50-digit decimals), at the smallest shapes where the kernel can go wrong, and the counts
inside the tree walk.

Pairs (the random-graph pairs are tests/test_fb_exact_gpu.py's own, built by its build_pairs): P1 / P2 70 x 66 random graphs --
more than 64 and no multiple of 64 a side, edges that span up to 20 sites (predecessors in another row block), p_dead 0 / 0.03 --
in full and behind a (8, 30) tunnel (predecessors outside the band); P3t p_dead 0.08, full probability 0; P4at rebuilt end sites,
2 x 10 end edges at distance 0.5 (log_fwd > log_bwd: the end counts follow the forward corner's multiplicities, the interior
counts use B); a one-residue sequence against 150 sites both ways round; a plain 150 x 150 DNA pair (three row blocks); a protein
pair (211 states: no emission table).

Tolerance, the project's: |got - want| <= 1e-7 |want| + 1e-12 (in-band cells) per entry.  The exact counts are computed once
(fixture `refs`)."""
import math

import numpy as np
import pytest

import pagan2_msa_amd as pgm
from pagan2_msa_amd import abi, host, synth

import fb_testlib
import pycheck_counts
from fb_testlib import random_tunnel
from test_fb_exact_gpu import BF, Pair, build_pairs

pytestmark = pytest.mark.gpu
ENVS = {"default": {}, "deep": {"PAGAN_FB_DEEP_MIN_ND": "0"}, "ring": {"PAGAN_FB_RING_MIN_ND": "0"}}
FROM_EXACT = ("P1", "P1t", "P2", "P2t", "P3t", "P4at")


def counts_pairs():
    """{name: Pair}, host only"""
    out = {name: p for name, p in build_pairs().items() if name in FROM_EXACT}
    mp = host.model_prob(1, 0.1, base_freq=BF)
    _, seqs, _ = synth.evolve_balanced(2, 150, branch=0.1, sub=0.1, indel_start=0.03, mean_len=3, seed=17)
    a, b = (host.HGraph.leaf(s).flatten() for s in seqs)
    one = host.HGraph.leaf("G").flatten()
    out["one_left"] = Pair("one_left", one, b, mp, None)
    out["one_right"] = Pair("one_right", a, one, mp, None)
    out["plain"] = Pair("plain", a, b, mp, None)
    out["plain_t"] = Pair("plain_t", a, b, mp, random_tunnel(np.random.default_rng(6), a.n_sites - 1, b.n_sites - 1, 8, 30))
    out["protein"] = Pair("protein", synth.random_graph(70, 20, 71, p_extra=0.4, max_deg=4, max_span=20),
                          synth.random_graph(40, 20, 72, p_extra=0.4, max_deg=4, max_span=20), host.model_prob(2, 0.2), None)
    return out


# (pair, environment, the schedule the pair's sweeps take under it)
CASES = [("P1", "default", 0), ("P1t", "default", 0), ("P1t", "deep", 3), ("P2", "default", 0), ("P2t", "default", 0), ("P3t", "default", 0),
         ("P4at", "default", 0), ("one_left", "default", 0), ("one_right", "default", 0), ("plain", "default", 2), ("plain_t", "ring", 2)]


@pytest.fixture(scope="module")
def pairs(pg):
    return counts_pairs()


@pytest.fixture(scope="module")
def refs(pairs):
    """{name: pycheck_counts.run(...)}: computed once and not modified"""
    return {name: pycheck_counts.run(*p.args(), emissions=p.mp.n_states <= 32) for name, p in pairs.items()}


def cells_of(p):
    return int(fb_testlib.in_band(p.Lx, p.Ly, p.band).sum())


def close(got, want, n_cells):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return (not np.isnan(got).any()) and bool(np.all(np.abs(got - want) <= 1e-7 * np.abs(want) + 1e-12 * n_cells))


def check_counts(c, ref, p, what):
    n = cells_of(p)
    for key in ("trans", "end") + (("emit",) if ref["emit"] is not None else ()):
        assert c[key].shape == ref[key].shape, (what, key)
        assert close(c[key], ref[key], n), (what, key, np.abs(c[key] - ref[key]).max(), c[key], ref[key])


def _bits(c):
    return tuple(c[k].tobytes() if c[k] is not None else None for k in ("trans", "end", "emit"))


@pytest.mark.parametrize("name, env, schedule", CASES, ids=["%s-%s-%d" % c for c in CASES])
def test_counts_against_the_exact_reading(pg, pairs, refs, monkeypatch, name, env, schedule):
    fb_testlib.set_env(monkeypatch, ENVS[env])
    p, ref = pairs[name], refs[name]
    what = (name, env)
    fb = pgm.FullProbability(*p.args())
    assert fb.schedule == schedule, (what, fb.schedule)
    c = fb.expected_counts()
    print("%s under %s: trans %s end %s | exact trans %s end %s" % (name, env, c["trans"].ravel(), c["end"], ref["trans"].ravel(), ref["end"]))
    check_counts(c, ref, p, what)
    n = cells_of(p)
    # on the device alone: the arcs into a state sum to the state's posterior, the table to the matches'
    mg = fb.site_marginals()
    into = c["trans"].sum(axis=0)
    assert close(into[0], mg["pX"].sum(), n) and close(into[1], mg["pY"].sum(), n), (what, into, mg["pX"].sum(), mg["pY"].sum())
    assert close(into[2], mg["pM_left"][1:].sum(), n), (what, into[2], mg["pM_left"][1:].sum())
    assert close(c["emit"].sum(), mg["pM_left"][1:].sum(), n), what
    if np.isfinite(ref["exact"].log_fwd):
        assert abs(c["end"].sum() - 1.0) <= 1e-7
    else:
        assert not c["trans"].any() and not c["end"].any() and not c["emit"].any(), what
    # two runs give the same bits; without the table the transitions keep theirs
    again = fb.expected_counts()
    assert _bits(again) == _bits(c), what
    lean = fb.expected_counts(emissions=False)
    assert lean["emit"] is None and _bits(lean)[:2] == _bits(c)[:2], what
    assert fb.counts_ms() > 0
    fb.close()


def test_the_inputs_are_what_the_cases_need(pg, pairs, refs):
    """Conditions on the inputs, not results."""
    for name in ("P1", "P1t", "P2", "P2t", "P3t", "P4at"):
        assert pairs[name].Lx > 64 and pairs[name].Lx % 64 and pairs[name].Ly > 64 and pairs[name].Ly % 64
    for name in ("P1", "P2", "P4at", "protein"):                      # an edge from another row block
        g = pairs[name].left
        site = np.repeat(np.arange(g.n_sites), np.diff(g.bwd_off))
        assert np.any((site // 64 != g.bwd_src // 64) & (site < g.n_sites - 1)), name
    assert refs["P3t"]["exact"].log_fwd == -np.inf and not refs["P3t"]["trans"].any()
    assert refs["P4at"]["exact"].log_fwd - refs["P4at"]["exact"].log_bwd > 1e-6
    assert pairs["one_left"].Lx == 2 and pairs["one_right"].Ly == 2 and pairs["plain"].Lx > 128
    assert pairs["protein"].mp.n_states > 32 and refs["protein"]["emit"] is None
    for name in ("P1", "P2", "P4at", "plain"):                        # every kind of transition is there to be counted
        assert np.all(refs[name]["trans"] > 1e-6) and np.all(refs[name]["end"] > 1e-6), (name, refs[name]["trans"], refs[name]["end"])


def test_batch_over_all_pairs_is_the_one_pair_call_bit_for_bit(pg, pairs, refs, monkeypatch):
    """one launch over pairs of 1 to 3 row blocks, with and without a table (the protein pair has none)"""
    fb_testlib.set_env(monkeypatch, {})
    names = sorted(pairs)
    fbs = pgm.full_probability_batch([pairs[n].args() for n in names])
    tables = [pairs[n].mp.n_states <= 32 for n in names]
    got = pgm.expected_counts_batch(fbs, tables)
    assert fbs[0].counts_ms() > 0 and all(fb.counts_ms() == 0 for fb in fbs[1:])
    for n, fb, c, table in zip(names, fbs, got, tables):
        check_counts(c, refs[n], pairs[n], (n, "batch"))
        assert _bits(fb.expected_counts(emissions=table)) == _bits(c), n
        fb.close()


def test_protein_pair_has_transitions_and_no_emission_table(pg, pairs, refs, monkeypatch):
    fb_testlib.set_env(monkeypatch, {})
    p, ref = pairs["protein"], refs["protein"]
    fb = pgm.FullProbability(*p.args())
    with pytest.raises(pgm.PaganError) as e:
        fb.expected_counts()
    assert e.value.code == abi.PAGAN_E_ARG
    c = fb.expected_counts(emissions=False)
    assert c["emit"] is None
    check_counts(c, ref, p, "protein")
    # in a batch with a DNA pair: the table for the one that has it
    dna = pgm.FullProbability(*pairs["P1"].args())
    with pytest.raises(pgm.PaganError) as e:
        pgm.expected_counts_batch([dna, fb])
    assert e.value.code == abi.PAGAN_E_ARG
    fb.close()
    dna.close()


# ---- the walk ----

@pytest.fixture(scope="module")
def tree():
    return synth.evolve_balanced(4, 300, branch=0.05, sub=0.05, indel_start=0.01, mean_len=4, seed=33)


def test_walk_keeps_every_nodes_counts_and_leaves_the_alignment_alone(pg, tree):
    names, seqs, nwk = tree
    off = host.Msa(names, seqs, nwk, full_probability=1).align()
    msa = host.Msa(names, seqs, nwk, full_probability=1, expected_counts=1).align()
    assert msa.alignment_all() == off.alignment_all()
    for k in range(msa.n_internal):
        assert msa.node_result(k).same_alignment(off.node_result(k)), k
        assert msa.node_fb(k)[:2] == off.node_fb(k)[:2] and msa.node_support(k).tobytes() == off.node_support(k).tobytes()
        left, right, _model, band = msa.node_job(k)
        fb = pgm.FullProbability(left, right, msa.node_model_prob(k), band)
        assert _bits(msa.node_counts(k)) == _bits(fb.expected_counts()), k
        assert _bits(msa.node_counts(k, emissions=False))[:2] == _bits(fb.expected_counts())[:2]
        fb.close()
        with pytest.raises(pgm.PaganError) as e:
            off.node_counts(k)
        assert e.value.code == abi.PAGAN_E_ARG
    total = msa.expected_counts()
    assert total["nodes"] == list(range(msa.n_internal)) and total["dists"] == [msa.node_info(k).dist for k in range(msa.n_internal)]
    assert np.array_equal(total["trans"], sum(c["trans"] for c in total["node_counts"]))
    assert abs(total["end"].sum() - msa.n_internal) <= 1e-6
    rate, ext = host.fit_indel(total["dists"], total["node_counts"])
    assert 0 < rate < 1 and 0 < ext < 1


def test_walk_counts_under_sample_path_and_the_decoder(pg, tree):
    names, seqs, nwk = tree
    for kw in ({"sample_path": 1, "sample_seed": 3, "sample_on_device": 1}, {"posterior_decode": 1}):
        msa = host.Msa(names, seqs, nwk, expected_counts=1, **kw).align()
        ref = host.Msa(names, seqs, nwk, **kw).align()
        assert msa.alignment_all() == ref.alignment_all(), kw
        for k in range(msa.n_internal):
            left, right, _model, band = msa.node_job(k)
            fb = pgm.FullProbability(left, right, msa.node_model_prob(k), band)
            assert _bits(msa.node_counts(k)) == _bits(fb.expected_counts()), (kw, k)
            fb.close()


def test_walk_with_an_indel_model_aligns_under_it(pg, tree):
    names, seqs, nwk = tree
    msa = host.Msa(names, seqs, nwk, full_probability=1, expected_counts=1, indel_model=(0.03, 0.03, 0.6, -1)).align()
    for k in range(msa.n_internal):
        dist = msa.node_info(k).dist
        rate = np.float32(0.03) + np.float32(0.03)
        t = 1.0 - math.exp(-0.5 * float(rate) * dist)
        mp = msa.node_model_prob(k)
        assert (np.float32(mp.gap_open), np.float32(mp.non_gap), np.float32(mp.gap_ext)) == (np.float32(t), np.float32(1.0 - 2 * t), np.float32(0.6)), k
        assert np.all(msa.node_counts(k)["trans"] >= 0)
    for r, s in zip(msa.alignment(), seqs):
        assert r.replace("-", "") == s
