"""GPU: the forward/backward pass inside the tree walk (host_tree.cpp: full_probability, sample_path, sample_seed) -- the
walk's per-node totals, column support and site marginals against the same calls made pair by pair on the node's job, the
alignment untouched by full_probability, sampled walks that depend on (seed, node) only, and the pass's sub-batches: a walk
whose memory budget admits one node at a time leaves what the uncut walk leaves."""
import ctypes as C

import numpy as np
import pytest

import pagan2_msa_amd as pgm
from pagan2_msa_amd import abi, host, synth

pytestmark = pytest.mark.gpu


def _trees():
    a = synth.evolve_balanced(8, 400, branch=0.04, sub=0.04, indel_start=0.01, mean_len=4, seed=46)
    b = synth.evolve_balanced(4, 3000, branch=0.01, sub=0.01, indel_start=0.008, mean_len=4, seed=61)
    return [(a, {"use_anchors": 0}), (b, {"use_anchors": 1})]


@pytest.fixture(scope="module")
def walks(pg):
    """[(off, with full_probability=2)] per tree, aligned once."""
    out = []
    for (names, seqs, nwk), opts in _trees():
        off = host.Msa(names, seqs, nwk, **opts).align()
        fp2 = host.Msa(names, seqs, nwk, full_probability=2, **opts).align()
        out.append((off, fp2, (names, seqs, nwk), opts))
    return out


def _same_walk(a, b):
    assert a.alignment_all() == b.alignment_all()
    for k in range(a.n_internal):
        ra, rb = a.node_result(k), b.node_result(k)
        assert ra.same_alignment(rb), k
        assert np.float64(a.node_info(k).score).tobytes() == np.float64(b.node_info(k).score).tobytes()


def test_full_probability_leaves_the_alignment_alone_and_reports_every_node(pg, walks):
    for off, fp2, (names, seqs, nwk), opts in walks:
        fp1 = host.Msa(names, seqs, nwk, full_probability=1, **opts).align()
        _same_walk(off, fp1)
        _same_walk(off, fp2)
        n = len(names)
        banded = 0
        for k in range(fp1.n_internal):
            left, right, _model, band = fp1.node_job(k)
            banded += band is not None
            res = fp1.node_result(k)
            fb = pgm.FullProbability(left, right, fp1.node_model_prob(k), band)
            lf, lb, sweep_ms, post_ms = fp1.node_fb(k)
            assert (lf, lb) == (fb.log_fwd, fb.log_bwd), k
            assert abs(lf - lb) <= 1e-7 * abs(lf)
            assert sweep_ms >= 0 and post_ms >= 0
            sup = fp1.node_support(k)
            assert sup.tobytes() == fb.path_support(res.cols).tobytes(), k
            assert np.all(sup[res.cols[:, 2] >= 5] == -1.0) and np.all(sup[res.cols[:, 2] <= 4] > 0)
            fb.close()
            row = fp1.support_row(n + k)
            assert row.shape == (len(fp1.alignment()[0]),) and row.dtype == np.float32
            assert np.array_equal(row[row >= 0], sup[sup >= 0].astype(np.float32)), k
            with pytest.raises(pgm.PaganError) as e:                   # marginals were not asked for
                fp1.node_marginals(k)
            assert e.value.code == abi.PAGAN_E_ARG
        assert banded == (fp1.n_internal if opts["use_anchors"] else 0)
        # the root's columns are the alignment's: its support covers every column that is not a skip column
        root = fp1.n_internal - 1
        rrow, rsup = fp1.support_row(n + root), fp1.node_support(root)
        assert np.array_equal(rrow, rsup.astype(np.float32))
        with pytest.raises(pgm.PaganError) as e:
            fp1.support_row(0)
        assert e.value.code == abi.PAGAN_E_ARG
        with pytest.raises(pgm.PaganError) as e:
            off.node_fb(0)
        assert e.value.code == abi.PAGAN_E_ARG


def test_full_probability_2_keeps_the_site_marginals(pg, walks):
    for _off, fp2, _tree, _opts in walks:
        for k in range(fp2.n_internal):
            left, right, _model, band = fp2.node_job(k)
            fb = pgm.FullProbability(left, right, fp2.node_model_prob(k), band)
            want, got = fb.site_marginals(), fp2.node_marginals(k)
            assert set(want) == set(got)
            for name in want:
                assert want[name].tobytes() == got[name].tobytes(), (k, name)
            assert fp2.node_support(k).tobytes() == fb.path_support(fp2.node_result(k).cols).tobytes()
            fb.close()


def _cols(msa):
    return [msa.node_result(k).cols.copy() for k in range(msa.n_internal)]


def test_sampled_walks_depend_on_seed_and_node_only(pg, walks):
    for _off, _fp2, (names, seqs, nwk), opts in walks:
        n = len(names)
        a = host.Msa(names, seqs, nwk, sample_path=1, sample_seed=1, **opts).align()
        b = host.Msa(names, seqs, nwk, sample_path=1, sample_seed=1, **opts).align()
        c = host.Msa(names, seqs, nwk, sample_path=1, sample_seed=2, **opts).align()
        assert a.alignment_all() == b.alignment_all()
        assert any(not np.array_equal(x, y) for x, y in zip(_cols(a), _cols(c)))
        # node by node instead of level by level: the same rows
        d = host.Msa(names, seqs, nwk, sample_path=1, sample_seed=1, **opts)
        while d.remaining > 0:
            d.align_nodes(d.ready()[-1:])
        d.finish()
        assert d.alignment_all() == a.alignment_all()
        for k in range(a.n_internal):
            left, right, _model, band = a.node_job(k)
            res = a.node_result(k)
            fb = pgm.FullProbability(left, right, a.node_model_prob(k), band)
            u = host.sample_uniforms(1, n + k, left.n_sites + right.n_sites - 1)
            want, _visited = fb.sample_path(u)
            assert np.array_equal(want.cols, res.cols), k
            assert np.array_equal(want.left_used, res.left_used) and np.array_equal(want.right_used, res.right_used)
            lf, lb, _, _ = a.node_fb(k)
            assert a.node_info(k).score == lf == fb.log_fwd and res.status == 0
            assert a.node_support(k).tobytes() == fb.path_support(res.cols).tobytes()
            fb.close()
            # every site of both children is used once, in order
            assert [x for x in res.cols[:, 0] if x >= 0] == list(range(1, left.n_sites - 1))
            assert [x for x in res.cols[:, 1] if x >= 0] == list(range(1, right.n_sites - 1))


# ---- the sub-batch cut ----

CUT_MODES = {
    "marginals": {"full_probability": 2, "expected_counts": 1},
    "device_sampler": {"sample_path": 1, "sample_on_device": 1, "expected_counts": 1},
    "host_sampler": {"sample_path": 1},
    "decoder": {"posterior_decode": 1, "expected_counts": 1},
}


@pytest.fixture(scope="module")
def cut_tree():
    """4 leaves x 300 sites, balanced: two leaf-level nodes of near-equal size in one round, the smallest walk a cut can happen in.
    Few indels, so that the root (the largest node: it sets the budget) is not a tenth longer than its grandchildren -- then the
    budget for the root alone would admit both leaf-level nodes at once in every mode but the decoder's."""
    return synth.evolve_balanced(4, 300, branch=0.05, sub=0.05, indel_start=0.002, mean_len=4, seed=33)


def _pass_bytes(msa, k, kw):
    """(what the forward/backward pass of node k takes under the mode: the sum the walk cuts by, the node's Viterbi batch)"""
    left, right, _model, band = msa.node_job(k)
    l, r = left.n_sites, right.n_sites
    need = pgm.fb_predict_bytes(l, r, band, n_states=msa.node_model_prob(k).n_states)
    if kw.get("posterior_decode"):
        need += pgm.fb_decode_predict_bytes(l, r, band)
    elif kw.get("sample_on_device"):
        need += pgm.fb_sample_predict_bytes(l, r, 1)
    if kw.get("expected_counts"):
        need += pgm.fb_counts_predict_bytes(l, r, msa.node_model_prob(k).n_states)
    dp = pgm.lib().pagan_dp_predict_bytes(l, r, C.byref(band.c) if band is not None else None)
    assert need > 0 and dp > 0
    return need, dp


@pytest.mark.parametrize("mode", sorted(CUT_MODES))
def test_a_budget_for_one_node_at_a_time_changes_nothing(pg, cut_tree, mode):
    names, seqs, nwk = cut_tree
    # full matrices: behind a band a node of 300 sites takes little more than the predictors' constants, and two fit wherever one does
    kw = dict(CUT_MODES[mode], use_anchors=0)
    whole = host.Msa(names, seqs, nwk, **kw).align()
    assert whole.n_internal == 3
    leaf_level = [k for k in range(3) if whole.node_info(k).level == whole.node_info(0).level]
    assert leaf_level == [0, 1] and whole.node_info(2).level != whole.node_info(0).level
    needs = [_pass_bytes(whole, k, kw) for k in range(3)]
    budget = max(fb + dp for fb, dp in needs) + 1            # every node fits alone, its Viterbi batch included
    assert 2 * min(needs[k][0] for k in leaf_level) > budget                    # ... and the two leaf-level passes do not fit together
    tight = host.Msa(names, seqs, nwk, device_mem_budget=budget, **kw).align()
    assert tight.alignment_all() == whole.alignment_all()
    for k in range(3):
        a, b = whole.node_result(k), tight.node_result(k)
        assert a.same_alignment(b) and a.status == b.status, k
        assert np.array_equal(a.left_used, b.left_used) and np.array_equal(a.right_used, b.right_used), k
        assert np.float64(whole.node_info(k).score).tobytes() == np.float64(tight.node_info(k).score).tobytes(), k
        assert np.array(whole.node_fb(k)[:2]).tobytes() == np.array(tight.node_fb(k)[:2]).tobytes(), k
        assert whole.node_support(k).tobytes() == tight.node_support(k).tobytes(), k
        if kw.get("full_probability") == 2:
            want, got = whole.node_marginals(k), tight.node_marginals(k)
            assert set(want) == set(got) and all(want[name].tobytes() == got[name].tobytes() for name in want), k
        if kw.get("expected_counts"):
            want, got = whole.node_counts(k), tight.node_counts(k)
            assert all(want[name].tobytes() == got[name].tobytes() for name in ("trans", "end", "emit")), k
        if kw.get("posterior_decode"):
            assert np.array(whole.node_decode(k)[:2]).tobytes() == np.array(tight.node_decode(k)[:2]).tobytes(), k
    if kw.get("posterior_decode"):
        # the decoder's time is booked at a sub-batch's first node: the cut walk has a sub-batch per leaf-level node, the uncut one
        assert all(tight.node_decode(k)[2] > 0 for k in leaf_level)
        assert sorted(whole.node_decode(k)[2] > 0 for k in leaf_level) == [False, True]


def test_a_codon_walk_is_cut_by_its_tables(pg):
    """Four codon leaves of ~40 codons with full_probability=1: a pair's arena is its score table (8 * 1892^2 B = 28.6 MB of logs)
    and little else.  Under a budget that holds one leaf-level pass and not two the walk must take the two leaf-level nodes in a
    sub-batch each -- a one-workgroup pair's sweeps are timed only when it is its call's one pair, so the cut walk books a time at
    both and the uncut one at neither -- and give the uncut walk's bytes."""
    import fb_tables
    names, seqs, nwk = fb_tables.evolve_codons(4, 40, seed=96, branch=0.05, sub=0.08, indel_start=0.01, mean_len=2)
    kw = {"data_type": 3, "full_probability": 1, "use_anchors": 0}
    whole = host.Msa(names, seqs, nwk, **kw).align()
    assert whole.n_internal == 3 and whole.data_type == 3
    leaf_level = [k for k in range(3) if whole.node_info(k).level == whole.node_info(0).level]
    assert leaf_level == [0, 1]
    table = 8 * 1892 * 1892
    needs = [_pass_bytes(whole, k, kw) for k in range(3)]
    budget = max(fb + dp for fb, dp in needs) + 1
    assert all(fb >= table for fb, _dp in needs) and table < budget < 2 * table
    tight = host.Msa(names, seqs, nwk, device_mem_budget=budget, **kw).align()
    assert tight.alignment_all() == whole.alignment_all()
    for k in range(3):
        a, b = whole.node_result(k), tight.node_result(k)
        assert a.same_alignment(b) and a.status == b.status == 0, k
        assert np.float64(whole.node_info(k).score).tobytes() == np.float64(tight.node_info(k).score).tobytes(), k
        assert np.array(whole.node_fb(k)[:2]).tobytes() == np.array(tight.node_fb(k)[:2]).tobytes(), k
        assert whole.node_support(k).tobytes() == tight.node_support(k).tobytes(), k
    print("sweep ms booked: uncut %s, cut %s" % ([whole.node_fb(k)[2] for k in range(3)], [tight.node_fb(k)[2] for k in range(3)]))
    assert all(tight.node_fb(k)[2] > 0 for k in leaf_level) and not any(whole.node_fb(k)[2] > 0 for k in leaf_level)
