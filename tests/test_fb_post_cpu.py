"""CPU: the host-only pieces around the forward/backward pass in the tree walk -- pagan_path_cells (the DP cell a column sits
on), pagan_sample_uniforms (the keyed generator the walk samples paths with), the new walk options' defaults, and the test seam
refusing the pass instead of skipping it."""
import ctypes as C

import numpy as np
import pytest

import pagan2_msa_amd as pgm
from pagan2_msa_amd import abi, host, synth

M64 = (1 << 64) - 1


def path_cells_py(cols):
    """The rule of include/pagan_dp.h restated."""
    ci = cj = 0
    out = []
    for left, right, ps in cols:
        if ps == 2:
            ci, cj = left, right
            out.append((2, ci, cj))
        elif ps == 3:
            ci = left
            out.append((0, ci, cj))
        elif ps == 4:
            cj = right
            out.append((1, ci, cj))
        else:
            assert ps in (5, 6)
            out.append((-1, -1, -1))
    return np.array(out, np.int32).reshape(-1, 3)


def test_path_cells_on_hand_made_columns(pg):
    cols = [[1, 1, 2], [2, -1, 3], [3, -1, 5], [4, -1, 3], [-1, 2, 4], [-1, 3, 6], [-1, 4, 6], [5, 5, 2], [-1, 6, 4], [6, -1, 3]]
    got = pgm.path_cells(cols)
    assert np.array_equal(got, path_cells_py(cols))
    assert got.tolist() == [[2, 1, 1], [0, 2, 1], [-1, -1, -1], [0, 4, 1], [1, 4, 2], [-1, -1, -1], [-1, -1, -1], [2, 5, 5], [1, 5, 6], [0, 6, 6]]
    # a gap before any match sits in row / column 0
    assert pgm.path_cells([[-1, 1, 4], [1, -1, 3]]).tolist() == [[1, 0, 1], [0, 1, 1]]
    assert pgm.path_cells(np.zeros((0, 3), np.int32)).shape == (0, 3)
    with pytest.raises(pgm.PaganError) as e:
        pgm.path_cells([[1, 1, 7]])
    assert e.value.code == abi.PAGAN_E_ARG
    assert pgm.lib().pagan_path_cells(None, 3, None) == abi.PAGAN_E_ARG


def test_path_cells_along_an_oracle_path_with_skip_columns(pg, oracle):
    """A homopolymer-graph pair (multi-edge sites, skip edges) inside a band of +-25: the cells derived from the oracle's
    Viterbi columns all lie on a path -- none has posterior 0 under the oracle's forward/backward."""
    _, seqs, _ = synth.evolve_balanced(2, 300, branch=0.05, sub=0.06, indel_start=0.01, mean_len=3, seed=5)
    gl, gr = (oracle.OGraph.leaf(s, oracle.DNA_ALPHABET, flags=2).flatten() for s in seqs)
    Lx, Ly = gl.n_sites - 1, gr.n_sites - 1
    centre = np.arange(Lx) * (Ly - 1) // (Lx - 1)                 # (the two graphs differ by more than 25 sites: the band follows the diagonal)
    up = np.maximum(centre - 25, 0).astype(np.int32)
    lo = np.minimum(centre + 25, Ly - 1).astype(np.int32)
    band = abi.Band(up, lo)
    bf = [0.25] * 4
    res = oracle.dp_align(gl, gr, oracle.dna_model(bf, 0.1), band)
    assert res.status == 0
    cells = pgm.path_cells(res.cols)
    assert np.array_equal(cells, path_cells_py(res.cols.tolist()))
    skip = res.cols[:, 2] >= 5
    assert skip.sum() > 0 and np.all(cells[skip] == -1) and np.all(cells[~skip, 0] >= 0)
    _, _, post, _ = oracle.fb(gl, gr, oracle.model_prob(1, 0.1, base_freq=bf), band=band)
    real = cells[~skip]
    p = post[real[:, 1], real[:, 2], real[:, 0]]
    assert p.min() > 0, p.min()
    print("skip columns %d, posterior along the path: min %.3g median %.3f" % (skip.sum(), p.min(), np.median(p)))


def _mix(x):
    x = (x + 0x9E3779B97F4A7C15) & M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


def uniforms_py(seed, node, n):
    key = _mix(_mix(seed & M64) ^ (node & M64))
    return np.array([(_mix(key ^ s) >> 11) / 9007199254740992.0 for s in range(n)])


def test_sample_uniforms_are_a_pure_function_of_their_key(pg):
    for seed, node in ((0, 0), (1, 8), (2, 8), (1, 9), (M64, 31), (123456789012345, 2 ** 31 - 1)):
        u = host.sample_uniforms(seed, node, 257)
        assert u.shape == (257,) and u.min() >= 0.0 and u.max() < 1.0
        assert np.array_equal(u, uniforms_py(seed, node, 257))
        assert np.array_equal(u, host.sample_uniforms(seed, node, 257))
        assert np.array_equal(u[:40], host.sample_uniforms(seed, node, 40))           # u[s] does not depend on n
    a, b, c = host.sample_uniforms(1, 8, 64), host.sample_uniforms(2, 8, 64), host.sample_uniforms(1, 9, 64)
    assert not np.any(a == b) and not np.any(a == c) and not np.any(b == c)
    big = host.sample_uniforms(7, 3, 20000)
    assert abs(big.mean() - 0.5) < 0.01 and len(np.unique(big)) == big.size
    assert pgm.lib().pagan_sample_uniforms(1, 1, -1, None) == abi.PAGAN_E_ARG


def test_default_opts_leave_the_new_fields_off(pg):
    o = host.CMsaOpts()
    C.memset(C.byref(o), 0xFF, C.sizeof(o))
    host._lib().pagan_msa_default_opts(C.byref(o))
    assert (o.full_probability, o.sample_path, o.sample_seed) == (0, 0, 0)
    assert (o.use_anchors, o.anchors_offset, o.mostcommon) == (1, 15, 0)
    # the new fields are the struct's last: what came before them has not moved
    names = [f[0] for f in host.CMsaOpts._fields_]
    assert names[-3:] == ["full_probability", "sample_path", "sample_seed"] and names[-4] == "mostcommon"


def _oracle_backend(oracle):
    L = oracle.lib()

    def fn(n, jobs, opts, out, user):
        for k in range(n):
            j = jobs[k]
            rc = L.oracle_dp_align(j.left, j.right, j.model, j.band if j.band else None, opts, C.byref(out[k]))
            if rc != 0:
                return rc
        return 0
    return fn


@pytest.mark.parametrize("opts", [{"full_probability": 1}, {"full_probability": 2}, {"sample_path": 1, "sample_seed": 3}])
def test_the_test_seam_refuses_the_pass_instead_of_skipping_it(pg, oracle, opts):
    names, seqs, nwk = synth.evolve_balanced(4, 60, branch=0.03, sub=0.03, indel_start=0.01, mean_len=3, seed=12)
    msa = host.Msa(names, seqs, nwk, use_anchors=0, **opts)
    msa.set_batch_backend(_oracle_backend(oracle))
    with pytest.raises(pgm.PaganError) as e:
        msa.align()
    assert e.value.code == abi.PAGAN_E_NODEVICE
    with pytest.raises(pgm.PaganError) as e:
        msa.align_nodes(msa.ready()[:1])
    assert e.value.code == abi.PAGAN_E_NODEVICE
    # the same walk with the options off goes through, and has nothing to report for a node
    plain = host.Msa(names, seqs, nwk, use_anchors=0)
    plain.set_batch_backend(_oracle_backend(oracle))
    plain.align()
    with pytest.raises(pgm.PaganError) as e:
        plain.node_fb(0)
    assert e.value.code == abi.PAGAN_E_ARG
    with pytest.raises(pgm.PaganError) as e:
        plain.support_row(0)
    assert e.value.code == abi.PAGAN_E_ARG


def test_fb_predict_bytes_covers_the_matrices(pg):
    cells = pgm.lib().pagan_dp_count_cells(301, 281, None)
    assert cells == 300 * 280
    assert pgm.fb_predict_bytes(301, 281) >= 48 * cells
    up = np.maximum(np.arange(300) - 10, 0).astype(np.int32)
    lo = np.minimum(np.arange(300) + 10, 279).astype(np.int32)
    band = abi.Band(up, lo)
    inb = pgm.lib().pagan_dp_count_cells(301, 281, C.byref(band.c))
    assert 48 * inb <= pgm.fb_predict_bytes(301, 281, band) < pgm.fb_predict_bytes(301, 281)
