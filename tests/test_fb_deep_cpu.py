"""The deep-ring forward/backward sweeps (dp_fb_deep.inc: pg_fb_forward_deep / pg_fb_backward_deep), what needs no GPU:

  * the routing: pagan_fb_debug_route is the function pagan_fb_run decides with (fb_route in dp_fb_plan.cpp), so what it answers here
    is what the product does -- plain pairs keep the ring sweeps, graph pairs of 4,096 cell diagonals or more inside a tunnel take
    the deep ring, PAGAN_FB_DEEP=0 gives them back to the block schedule, short pairs stay on the one-workgroup kernels, and one
    edge that reaches further back than any ring does not disqualify a pair (it marks a few diagonals far);
  * the disassembly, in the manner of test_fb_asm_cpu.py: no scratch, and for the ALL_LDS instantiations no load from memory and no
    vmcnt wait on the step of a diagonal that is not marked far."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import pagan2_msa_amd as pgm
from pagan2_msa_amd import abi, host, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pagan2-msa_amd", "csrc")


def walk_on_cpu(oracle, names, seqs, nwk, **opts):
    """The tree walk with the oracle's DP behind the batch seam (as test_workqueue_cpu.py)."""
    L = oracle.lib()

    def backend(n, jobs, o, out, user):
        for k in range(n):
            j = jobs[k]
            rc = L.oracle_dp_align(j.left, j.right, j.model, j.band if j.band else None, o, C.byref(out[k]))
            if rc != 0:
                return rc
        return 0
    msa = host.Msa(names, seqs, nwk, **opts)
    msa.set_batch_backend(backend)
    msa._keep_backend = backend
    return msa.align()


def reach(g):
    """longest i - src over the bwd lists of the sites 1 .. n_sites - 2 (numpy recomputation)"""
    n = g.n_sites - 1
    off = g.bwd_off.astype(np.int64)
    idx = np.repeat(np.arange(g.n_sites), np.diff(off))
    keep = (idx >= 1) & (idx < n)
    return int((idx[keep] - g.bwd_src[:off[-1]][keep]).max())


@pytest.fixture(scope="module")
def long_graph_pair(oracle, pg):
    """the root pair of 4 x 2.5 kb inside its define_tunnel band: two graphs with multi-edge sites, ~5,000 cell diagonals"""
    names, seqs, nwk = synth.evolve_balanced(4, 2500, branch=0.01, sub=0.01, indel_start=0.008, mean_len=4, seed=61)
    msa = walk_on_cpu(oracle, names, seqs, nwk, use_anchors=1)
    left, right, _model, band = msa.node_job(msa.n_internal - 1)
    assert band is not None
    assert int((np.diff(left.bwd_off) > 1).sum()) > 0 and int((np.diff(right.bwd_off) > 1).sum()) > 0
    return left, right, band


def _random_tunnel(rng, Lx, Ly, lo_half, hi_half):
    half = rng.integers(lo_half, hi_half, Lx)
    centre = np.arange(Lx) * (Ly - 1) // max(Lx - 1, 1)
    upper = np.maximum.accumulate(np.maximum(centre - half, 0))
    lower = np.maximum.accumulate(np.minimum(centre + half, Ly - 1))
    upper[0] = 0
    lower[-1] = Ly - 1
    return abi.Band(upper.astype(np.int32), lower.astype(np.int32))


def clean_env(monkeypatch):
    for v in ("PAGAN_FB_DEEP", "PAGAN_FB_DEEP_MIN_ND", "PAGAN_FB_RING", "PAGAN_FB_RING_MIN_ND", "PAGAN_FB_BAND_MIN_ND", "PAGAN_FB_GROUPS"):
        monkeypatch.delenv(v, raising=False)


def test_plain_leaf_pair_in_a_tunnel_keeps_the_ring(pg, monkeypatch):
    clean_env(monkeypatch)
    _, seqs, _ = synth.evolve_balanced(2, 6000, branch=0.02, sub=0.02, indel_start=0.003, mean_len=4, seed=47)
    gl, gr = (host.HGraph.leaf(s).flatten() for s in seqs)
    band, _ = host.define_tunnel(seqs[0], seqs[1], seqs[0], seqs[1])
    code, info = pgm.fb_route(gl, gr, band)
    assert code == 2, (code, info)
    assert info["diagonals"] == gl.n_sites + gr.n_sites - 3 and info["reach_left"] == 1 and info["reach_right"] == 1
    assert info["segments"] == 0


def test_long_graph_pair_in_its_tunnel_takes_the_deep_ring(pg, long_graph_pair, monkeypatch):
    clean_env(monkeypatch)
    left, right, band = long_graph_pair
    code, info = pgm.fb_route(left, right, band)
    assert info["diagonals"] >= 4096, info
    assert code == 3, (code, info)
    assert info["segments"] >= 1 and info["min_D"] >= 4 and info["widest"] <= 1024
    assert info["reach_left"] == reach(left) and info["reach_right"] == reach(right)
    assert info["reach_left"] > 1 or info["reach_right"] > 1
    # the switch: back on the block schedule; without its band: a full matrix keeps the blocks
    monkeypatch.setenv("PAGAN_FB_DEEP", "0")
    assert pgm.fb_route(left, right, band)[0] == 1
    monkeypatch.delenv("PAGAN_FB_DEEP")
    assert pgm.fb_route(left, right, None)[0] == 1
    # PAGAN_FB_GROUPS overrides everything
    monkeypatch.setenv("PAGAN_FB_GROUPS", "1")
    assert pgm.fb_route(left, right, band)[0] == 0
    monkeypatch.setenv("PAGAN_FB_GROUPS", "4")
    assert pgm.fb_route(left, right, band)[0] == 1


def test_pair_under_the_threshold_stays_on_the_one_workgroup_kernels(oracle, pg, monkeypatch):
    clean_env(monkeypatch)
    names, seqs, nwk = synth.evolve_balanced(4, 700, branch=0.04, sub=0.04, indel_start=0.01, mean_len=4, seed=46)
    msa = walk_on_cpu(oracle, names, seqs, nwk, use_anchors=0)
    left, right, _model, _band = msa.node_job(msa.n_internal - 1)
    band = _random_tunnel(np.random.default_rng(3), left.n_sites - 1, right.n_sites - 1, 20, 70)
    code, info = pgm.fb_route(left, right, band)
    assert info["diagonals"] < 4096 and info["widest"] <= 256 and code == 0, (code, info)
    # ... and the existing tests' switches do not send it to the deep ring: PAGAN_FB_BAND_MIN_ND=0 is the block schedule
    monkeypatch.setenv("PAGAN_FB_BAND_MIN_ND", "0")
    monkeypatch.setenv("PAGAN_FB_RING_MIN_ND", "0")
    assert pgm.fb_route(left, right, band)[0] == 1
    # its own threshold does
    monkeypatch.setenv("PAGAN_FB_DEEP_MIN_ND", "0")
    assert pgm.fb_route(left, right, band)[0] == 3


def test_one_edge_beyond_any_ring_does_not_disqualify_the_pair(pg, monkeypatch):
    clean_env(monkeypatch)
    rng = np.random.default_rng(5)
    n = 3000
    gr = abi.Graph.chain(rng.integers(0, 4, n))
    base = abi.Graph.chain(rng.integers(0, 4, n))
    # site 1500 gets a second edge, from site 1400: reach 100, beyond the deepest ring (64 diagonals)
    at = 1500
    off = base.bwd_off.copy()
    k = int(off[at + 1])
    src = np.insert(base.bwd_src, k, at - 100)
    lw = np.insert(base.bwd_logw, k, np.float32(np.log(0.3)))
    eid = np.insert(base.bwd_eid, k, base.n_edges)
    off[at + 1:] += 1
    gl = abi.Graph(base.state, off, src, lw, eid, n_edges=base.n_edges + 1)
    half = 10
    centre = np.arange(n + 1)
    band = abi.Band(np.maximum(centre - half, 0).astype(np.int32), np.minimum(centre + half, n).astype(np.int32))
    code, info = pgm.fb_route(gl, gr, band)
    assert code == 3, (code, info)
    assert info["reach_left"] == 100 and info["reach_right"] == 1
    assert info["far_cells"] > 0 and 0 < info["far_diagonals"] < info["diagonals"] // 20, info
    assert info["far_cells"] <= 2 * half + 1 and info["far_diagonals"] <= 2 * half + 1, info      # the cells of row 1,500, no others


# ---- disassembly ----

@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    out = str(tmp_path_factory.mktemp("fbdeepasm") / "dp_fb.s")
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "--offload-device-only", "-S", "-o", out, "dp_fb.hip"],
                   check=True, cwd=CSRC, stderr=subprocess.DEVNULL)
    return open(out).read()


def test_deep_kernels_have_no_scratch_and_fit_the_lds(asm):
    found = re.findall(r"\.group_segment_fixed_size:\s+(\d+)(?:(?!\.group_segment_fixed_size).)*?\.name:\s+(\S*pg_fb_\w+_deep\S*)\s+\.private_segment_fixed_size:\s+(\d+)", asm, re.S)
    assert len(found) == 4, found                                  # forward / backward x ALL_LDS
    for lds, name, scratch in found:
        assert int(scratch) == 0, (name, scratch)
        assert 24 * 4096 <= int(lds) <= 160 * 1024, (name, lds)    # the ring of D * B = 4,096 cells and the windows, inside what a workgroup may declare


def test_no_memory_load_on_a_step_without_far_cells(asm):
    """How the two sections of a step are told apart: the kernels bracket the call of the cell function compiled WITHOUT the far
    path (the branch taken when the diagonal's far bit is clear) with two marker instructions that nothing else in the file
    emits, `s_nop 13` before and `s_nop 14` behind (inline asm with a memory clobber: no load or store moves across them).  The
    lines between them are that section; it must not branch to a label outside itself, so it is all of the section.  There:
    no load from memory and no wait on vmcnt (the periodic drain sits behind the second marker, before the step's barrier).
    The far section, by contrast, must hold the sc1 loads."""
    load = re.compile(r"\b(global_load|flat_load|buffer_load|scratch_load)")
    checked = 0
    for m in re.finditer(r"^(_ZN[^\n:]*pg_fb_(forward|backward)_deepILb([01])E[^\n:]*):", asm, re.M):
        name, all_lds = m.group(1), m.group(3) == "1"
        lines = asm[m.end():asm.index("s_endpgm", m.end())].splitlines()
        begin = [k for k, ln in enumerate(lines) if ln.strip().startswith("s_nop 13")]
        end = [k for k, ln in enumerate(lines) if ln.strip().startswith("s_nop 14")]
        assert len(begin) == 1 and len(end) == 1 and begin[0] < end[0], (name, begin, end)
        assert any("sc1" in ln and load.search(ln) for ln in lines[:begin[0]] + lines[end[0]:]), name     # the far loads go to the L2
        if not all_lds:
            continue
        assert not any("src_shared_base" in ln for ln in lines), name
        near = lines[begin[0]:end[0]]
        assert len(near) > 300, (name, len(near))                   # (the arithmetic of a cell is in there)
        labels = {ln.split(":")[0] for ln in near if ln.startswith(".LBB")}
        for ln in near:
            if re.search(r"\bs_c?branch", ln):
                assert ln.split()[1] in labels, (name, ln)
        assert not any(load.search(ln) for ln in near), (name, [ln for ln in near if load.search(ln)][:3])
        assert not any("vmcnt" in ln for ln in near), (name, [ln for ln in near if "vmcnt" in ln][:3])
        # from the second marker to the step's barrier (or the jump to it): the periodic drain is the only vmcnt wait, and no load
        step_end = next(k for k in range(end[0], len(lines)) if lines[k].strip() == "s_barrier" or lines[k].split()[:1] == ["s_branch"])
        tail = lines[end[0]:step_end]
        assert not any(load.search(ln) for ln in tail), name
        assert sum("vmcnt" in ln for ln in tail) <= 1, (name, [ln for ln in tail if "vmcnt" in ln])
        checked += 1
    assert checked == 2
