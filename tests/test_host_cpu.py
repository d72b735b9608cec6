"""CPU tests of the host-side pieces (graph builder, anchors, model) against the oracle's
restatement.  No GPU: the alignment paths fed to the builders come from the oracle DP."""
import ctypes as C

import numpy as np
import pytest

from pagan2_msa_amd import abi, host, synth


def same_graph(hg, og, what=""):
    a, b = hg.flatten(), og.flatten()
    for f in ("state", "bwd_off", "bwd_src", "bwd_eid"):
        assert np.array_equal(getattr(a, f), getattr(b, f)), "%s: %s differs" % (what, f)
    assert a.bwd_logw.tobytes() == b.bwd_logw.tobytes(), what + ": bwd_logw bits differ"
    assert a.n_edges == b.n_edges
    (sa, sd, ea, ef), (sb, sdb, eb, efb) = hg.attrs(), og.attrs()
    assert np.array_equal(sa, sb), what + ": site attributes differ"
    assert sd.tobytes() == sdb.tobytes(), what + ": site distances differ"
    assert np.array_equal(ea, eb), what + ": edge attributes differ"
    assert ef.tobytes() == efb.tobytes(), what + ": edge weights differ"
    (fo, fe), (fob, feb) = hg.fwd(), og.fwd()
    assert np.array_equal(fo, fob) and np.array_equal(fe, feb), what + ": fwd lists differ"


@pytest.mark.parametrize("flags", [0, 1, 2])
def test_leaf_graphs(oracle, pg, flags):
    for s in ["ACGT", "A", "AAAAAAAACCCCCGTTTGGGGGGGGGGGGAC", "ACGTTTTTTACGGGGACCCCCCCCATTTAGGAN" * 3]:
        same_graph(host.HGraph.leaf(s, flags=flags), oracle.OGraph.leaf(s, flags=flags), "leaf %s/%d" % (s[:8], flags))


def walk(tree, seqs_by_name, oracle, bf, flags=0, check=None, band=False, protein=False):
    """Post-order progressive alignment with the oracle DP; both graph builders in lockstep."""
    stats = {"nodes": 0, "skips": 0, "nonreal": 0, "multi": 0, "states": set()}
    leaf_alpha, anc_alpha = host.alphabets(2 if protein else 1)
    o_leaf_alpha = oracle.protein_leaf_alphabet() if protein else oracle.DNA_ALPHABET
    char_as = 20 if protein else 4

    def rec(t):
        if t[0] == "leaf":
            s = seqs_by_name[t[1]]
            return (host.HGraph.leaf(s, leaf_alpha), oracle.OGraph.leaf(s, o_leaf_alpha),
                    min(max(t[2], 0.001), 0.2) if t[2] > 0 else 0.001)
        hl, ol, dl = rec(t[1])
        hr, orr, dr = rec(t[2])
        if protein:
            model, pars = host.protein_model(dl + dr)
            opars = oracle.protein_model(dl + dr)[1]
        else:
            model, pars = host.dna_model(bf, dl + dr)
            opars = oracle.dna_parsimony()
        gl, gr = hl.flatten(), hr.flatten()
        b = None
        if band:
            b, _ = host.define_tunnel(hl.string(False, anc_alpha), hr.string(False, anc_alpha),
                                      hl.string(True, anc_alpha), hr.string(True, anc_alpha))
            ob, _ = oracle.define_tunnel(ol, orr, alphabet=anc_alpha)
            assert np.array_equal(b.upper, ob.upper) and np.array_equal(b.lower, ob.lower)
        res = oracle.dp_align(gl, gr, model, b)
        assert res.status == 0
        hp = host.HGraph.parent(hl, hr, res, dl, dr, pars, char_as, flags)
        op = oracle.OGraph.parent(ol, orr, res, dl, dr, opars, char_as, flags)
        stats["states"].update(hp.flatten().state.tolist())
        same_graph(hp, op, "node %d" % stats["nodes"])
        stats["nodes"] += 1
        sa = hp.attrs()[0]
        stats["skips"] += int(np.isin(sa[:, 2], (5, 6)).sum())
        stats["nonreal"] += int((sa[:, 1] == 5).sum())
        stats["multi"] += int((np.diff(hp.flatten().bwd_off) > 1).sum())
        if check:
            check(hp, res)
        d = t[3]
        return hp, op, (0.001 if d <= 0 else min(d, 0.2))
    rec(tree)
    return stats


def base_freq(seqs):
    c = np.array([sum(s.count(x) for s in seqs) for x in "ACGT"], np.float32)
    return c / c.sum()


def test_progressive_graphs_balanced(oracle, pg):
    names, seqs, nwk = synth.evolve_balanced(16, 160, branch=0.05, sub=0.05, indel_start=0.012, mean_len=6, seed=3)
    st = walk(synth.parse_newick(nwk), dict(zip(names, seqs)), oracle, base_freq(seqs))
    assert st["nodes"] == 15 and st["skips"] > 20 and st["multi"] > 20


def test_progressive_graphs_banded_and_flags(oracle, pg):
    names, seqs, nwk = synth.evolve_balanced(8, 400, branch=0.02, sub=0.015, indel_start=0.004, mean_len=5, seed=5)
    for flags in (0, 1, 2):
        st = walk(synth.parse_newick(nwk), dict(zip(names, seqs)), oracle, base_freq(seqs), flags=flags, band=True)
        assert st["nodes"] == 7


def test_progressive_graphs_caterpillar_deletes_ranges(oracle, pg):
    """Deep caterpillar: skipped-edge limits drop edges and the deletion pass leaves non_real sites."""
    names, seqs, nwk = synth.evolve_caterpillar(14, 150, seed=2)
    st = walk(synth.parse_newick(nwk), dict(zip(names, seqs)), oracle, base_freq(seqs))
    assert st["nodes"] == 13 and st["nonreal"] > 0


def test_progressive_graphs_protein(oracle, pg):
    """WAG / 211-letter alphabet: upper nodes carry X and pair codes from the parsimony table."""
    aa = "ARNDCQEGHILKMFPSTWYV"
    names, seqs, nwk = synth.evolve_balanced(16, 120, branch=0.05, sub=0.08, indel_start=0.012, mean_len=4, seed=9,
                                             alphabet=aa)
    seqs[3] = seqs[3][:40] + "X" + seqs[3][41:]
    st = walk(synth.parse_newick(nwk), dict(zip(names, seqs)), oracle, None, protein=True)
    assert st["nodes"] == 15 and st["skips"] > 5
    assert max(st["states"]) > 20                                # pair codes reached internal nodes (X yields to a residue)
    st = walk(synth.parse_newick(nwk), dict(zip(names, seqs)), oracle, None, protein=True, band=True)
    assert st["nodes"] == 15


def test_define_tunnel_matches_oracle_on_leaves(oracle, pg):
    for seed in range(4):
        _, seqs, _ = synth.evolve_balanced(2, 2500, branch=0.01, sub=0.01 + 0.01 * seed, indel_start=0.003, seed=seed)
        ol, orr = oracle.OGraph.leaf(seqs[0]), oracle.OGraph.leaf(seqs[1])
        want, nw = oracle.define_tunnel(ol, orr)
        got, ng = host.define_tunnel(seqs[0], seqs[1], seqs[0], seqs[1])
        assert ng == nw and np.array_equal(got.upper, want.upper) and np.array_equal(got.lower, want.lower)
        assert np.all(np.diff(got.upper) >= 0) and np.all(np.diff(got.lower) >= 0)
    # repeats and identical tails: equal suffixes across the two strings, many equal-length hits
    a = "ACGTACGTAGCTAGCTAGGATCGATCGATTTAGCGCGATATCGCGAT" * 9 + "GGGTTTCACAC"
    b = a[:150] + "TT" + a[150:300] + a[310:]
    want, nw = oracle.define_tunnel(oracle.OGraph.leaf(a), oracle.OGraph.leaf(b), min_length=12)
    got, ng = host.define_tunnel(a, b, a, b, prefix_hit_length=12)
    assert ng == nw and np.array_equal(got.upper, want.upper) and np.array_equal(got.lower, want.lower)


def test_dna_model_against_numpy(pg):
    bf = np.array([0.31, 0.19, 0.22, 0.28], np.float32)
    for dist in (0.002, 0.1, 0.4):
        model, pars = host.dna_model(bf, dist)
        pi = bf.astype(np.float64)
        ka, piR, piY = 1.0, pi[0] + pi[2], pi[1] + pi[3]
        beta = 1 / (2 * piR * piY * (1 + ka))
        aY = (piR * piY * ka - pi[0] * pi[2] - pi[1] * pi[3]) / ((2 + 2 * ka) * (piY * pi[0] * pi[2] + piR * pi[1] * pi[3]))
        aR = aY
        Q = np.array([[0, beta * pi[1], aR * pi[2] / piR + beta * pi[2], beta * pi[3]],
                      [beta * pi[0], 0, beta * pi[2], aY * pi[3] / piY + beta * pi[3]],
                      [aR * pi[0] / piR + beta * pi[0], beta * pi[1], 0, beta * pi[3]],
                      [beta * pi[0], aY * pi[1] / piY + beta * pi[1], beta * pi[2], 0]])
        Q -= np.diag(Q.sum(1))
        w, v = np.linalg.eig(Q)
        P = (v @ np.diag(np.exp(w * dist)) @ np.linalg.inv(v)).real
        lo = 0.5 * (pi[:, None] + pi[None, :]) * P / (pi[:, None] * pi[None, :])
        assert np.allclose(model.log_score[:4, :4], np.log(lo), rtol=0, atol=2e-6)
        t = 1 - np.exp(-0.5 * 0.02 * dist)
        assert np.allclose(model.params, [np.log(t), np.log(0.8), np.log(0.95), np.log(1 - 2 * t)], atol=1e-6)
        # ambiguity rows are the max over member bases; N-N is the overall max
        assert model.log_score[14, 14] == model.log_score[:4, :4].max()
        assert model.log_score[4, 0] == max(model.log_score[0, 0], model.log_score[2, 0])   # R vs A
    assert np.array_equal(pars, __import__("oracle").dna_parsimony())


# ---- the walk's entry points under the oracle's DP behind the batch seam: what one entry check, one switch read and one guard for
# the per-node accessors must leave as it was

def _seam(oracle):
    L = oracle.lib()

    def fn(n, jobs, opts, out, user):
        for k in range(n):
            j = jobs[k]
            rc = L.oracle_dp_align(j.left, j.right, j.model, j.band if j.band else None, opts, C.byref(out[k]))
            if rc != 0:
                return rc
        return 0
    return fn


def _seam_walk(oracle, names, seqs, nwk, **opts):
    msa = host.Msa(names, seqs, nwk, **opts)
    msa.set_batch_backend(_seam(oracle))
    return msa


@pytest.mark.parametrize("opts, code", [
    (dict(posterior_decode=1, sample_path=1), abi.PAGAN_E_ARG),          # a decoder together with sample_path
    (dict(expected_counts=1), abi.PAGAN_E_ARG),                          # counts without a pass
    (dict(indel_model=(8.0, 8.0, -1, -1)), abi.PAGAN_E_ARG),             # no room for a match at the root's distance
    (dict(full_probability=1), abi.PAGAN_E_NODEVICE),                    # the seam has no forward/backward pass
])
def test_refusals_are_the_same_through_align_and_align_nodes(oracle, pg, opts, code):
    names, seqs, nwk = synth.evolve_balanced(4, 60, branch=0.05, sub=0.05, indel_start=0.01, mean_len=3, seed=31)
    H = host._lib()
    msa = _seam_walk(oracle, names, seqs, nwk, use_anchors=0, **opts)
    ids = np.array(msa.ready(), np.int32)
    assert len(ids) == 2
    assert H.pagan_msa_align(msa._h) == code
    assert H.pagan_msa_align_nodes(msa._h, len(ids), ids.ctypes.data_as(C.POINTER(C.c_int32))) == code
    assert H.pagan_msa_align_nodes(msa._h, 0, None) == code              # (before the list of nodes is looked at)
    assert msa.remaining == 3 and msa.ready() == list(ids)               # nothing ran


def test_host_threads_switch_changes_no_output(oracle, pg, tmp_path, monkeypatch):
    names, seqs, nwk = synth.evolve_caterpillar(6, 150, seed=17)

    def outputs(tag):
        msa = _seam_walk(oracle, names, seqs, nwk, use_anchors=1).align()
        path = str(tmp_path / (tag + ".fas"))
        msa.write_fasta(path, include_internal=True)
        with open(path, "rb") as f:
            fasta = f.read()
        return msa.alignment_all(), [msa.export_result(msa.n + k).tobytes() for k in range(msa.n_internal)], fasta

    monkeypatch.delenv("PAGAN_HOST_THREADS", raising=False)
    unset = outputs("unset")
    monkeypatch.setenv("PAGAN_HOST_THREADS", "1")
    one = outputs("one")
    assert len(unset[0]) == 11 and len(unset[1]) == 5 and unset[2].count(b">") == 11
    assert one == unset


def test_node_accessors_on_the_edges(oracle, pg):
    """Every pagan_msa_node_* entry: PAGAN_E_ARG below and above the internal nodes and for a node not aligned yet, success once it
    is.  Two keep what they always returned for a node that exists but is not aligned: node_info is PAGAN_OK with an empty
    result part, node_device is -1.  The five readers of a forward/backward pass stay PAGAN_E_ARG behind the seam, which has no
    pass (their success is the GPU suite's: tests/test_msa_fb_gpu.py, test_fb_decode_gpu.py, test_fb_counts_gpu.py)."""
    names, seqs, nwk = synth.evolve_balanced(4, 60, branch=0.05, sub=0.05, indel_start=0.01, mean_len=3, seed=31)
    H = host._lib()
    msa = _seam_walk(oracle, names, seqs, nwk, use_anchors=1)
    h = msa._h
    d = (C.c_double * 64)()
    i = (C.c_int32 * 64)()
    f64p, i32p = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    dp, ip = C.cast(d, f64p), C.cast(i, i32p)
    info, job, res, prob = host.CNodeInfo(), abi.CJob(), abi.CResult(), abi.CModelProb()
    plain = {"info": lambda k: H.pagan_msa_node_info(h, k, C.byref(info)),
             "job": lambda k: H.pagan_msa_node_job(h, k, C.byref(job)),
             "result": lambda k: H.pagan_msa_node_result(h, k, C.byref(res)),
             "model_prob": lambda k: H.pagan_msa_node_model_prob(h, k, C.byref(prob)),
             "device": lambda k: H.pagan_msa_node_device(h, k)}
    of_a_pass = {"fb": lambda k: H.pagan_msa_node_fb(h, k, dp),
                 "decode": lambda k: H.pagan_msa_node_decode(h, k, dp),
                 "counts": lambda k: H.pagan_msa_node_counts(h, k, dp, None),
                 "support": lambda k: H.pagan_msa_node_support(h, k, dp),
                 "marginals": lambda k: H.pagan_msa_node_marginals(h, k, dp, dp, ip, dp, dp, dp, ip, dp)}
    n_internal = msa.n_internal
    assert n_internal == 3
    for name, call in list(plain.items()) + list(of_a_pass.items()):
        for k in (-1, n_internal):
            assert call(k) == abi.PAGAN_E_ARG, (name, k)
    first = msa.ready()[0] - msa.n                                   # not aligned yet
    for name, call in list(plain.items()) + list(of_a_pass.items()):
        if name == "info":
            assert call(first) == abi.PAGAN_OK and info.node == msa.n + first and info.cells == 0 and info.left_sites == 0
        else:
            assert call(first) == abi.PAGAN_E_ARG, name              # (node_device: -1 is also "no device")
    msa.align_nodes([msa.n + first])
    assert plain["info"](first) == abi.PAGAN_OK and info.cells > 0 and info.left_sites > 2
    assert plain["job"](first) == abi.PAGAN_OK and job.left.contents.n_sites == info.left_sites and bool(job.band)
    assert plain["result"](first) == abi.PAGAN_OK and res.n_cols > 0 and res.cells == info.cells
    assert plain["model_prob"](first) == abi.PAGAN_OK and prob.n_states == 15
    assert plain["device"](first) >= 0
    for name, call in of_a_pass.items():
        assert call(first) == abi.PAGAN_E_ARG, name
    # null outputs are refused as before, on an aligned node too
    assert H.pagan_msa_node_info(h, first, None) == abi.PAGAN_E_ARG and H.pagan_msa_node_job(h, first, None) == abi.PAGAN_E_ARG
    assert H.pagan_msa_node_result(h, first, None) == abi.PAGAN_E_ARG and H.pagan_msa_node_model_prob(h, first, None) == abi.PAGAN_E_ARG
    other = [k for k in range(n_internal) if k != first and msa.n + k in msa.ready()][0]
    assert plain["result"](other) == abi.PAGAN_E_ARG                 # its sibling is still to come
