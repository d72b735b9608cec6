"""CPU: the host-only pieces around the device path sampler (dp_fb_sample.inc, pg_fb_sample) -- the per-path streams of uniform
numbers, the new entry points, the size prediction, the tree walk's sampler switch behind the test seam, and the kernel's
disassembly: no scratch and no spill in pg_fb_sample (a step of a path is a chain of dependent loads; a spilled register would
put a memory round trip of its own on it)."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import pagan2_msa_amd as pgm
from pagan2_msa_amd import abi, host, synth

M64 = (1 << 64) - 1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pagan2-msa_amd", "csrc")


def _mix(x):
    x = (x + 0x9E3779B97F4A7C15) & M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


def uniforms_path_py(seed, node, path, n):
    """The three mixes of include/pagan_dp.h restated."""
    key = _mix(_mix(seed & M64) ^ (node & M64))
    return np.array([(_mix(key ^ ((s + (path << 32)) & M64)) >> 11) / 9007199254740992.0 for s in range(n)])


def test_path_streams(pg):
    for seed, node in ((0, 0), (1, 8), (M64, 31), (123456789012345, 2 ** 31 - 1), (7, -3)):
        u0 = host.sample_uniforms_path(seed, node, 0, 300)
        assert np.array_equal(u0, host.sample_uniforms(seed, node, 300))              # path 0 is the existing stream, bit for bit
        for path in (1, 70000):
            u = host.sample_uniforms_path(seed, node, path, 300)
            assert u.min() >= 0.0 and u.max() < 1.0
            assert np.array_equal(u, uniforms_path_py(seed, node, path, 300))
            assert np.array_equal(u[:40], host.sample_uniforms_path(seed, node, path, 40))
            assert not np.any(u == u0)
        assert not np.any(host.sample_uniforms_path(seed, node, 1, 300) == host.sample_uniforms_path(seed, node, 70000, 300))
    # neighbouring paths and neighbouring nodes do not share numbers
    a, b, c = (pgm.sample_uniforms_path(1, 8, p, 4096) for p in (0, 1, 2))
    assert len(np.unique(np.concatenate([a, b, c, pgm.sample_uniforms_path(1, 9, 1, 4096)]))) == 4 * 4096
    u = np.zeros(4)
    up = u.ctypes.data_as(C.POINTER(C.c_double))
    assert pgm.lib().pagan_sample_uniforms_path(1, 1, -1, 4, up) == abi.PAGAN_E_ARG
    assert pgm.lib().pagan_sample_uniforms_path(1, 1, 0, -1, up) == abi.PAGAN_E_ARG
    assert pgm.lib().pagan_sample_uniforms_path(1, 1, 0, 4, None) == abi.PAGAN_E_ARG


NEW_DP = ["pagan_sample_uniforms_path", "pagan_fb_sample_paths_batch", "pagan_fb_sample_paths", "pagan_fb_samples_summary",
          "pagan_fb_samples_visited", "pagan_fb_samples_visited_all", "pagan_fb_samples_result", "pagan_fb_samples_ms",
          "pagan_fb_sample_predict_bytes", "pagan_fb_samples_destroy"]


def test_new_symbols_are_exported_and_resolve(pg):
    lib = C.CDLL(pgm.LIB_PATH)
    for sym in NEW_DP:
        assert sym in abi.EXPORTED and getattr(lib, sym) is not None
    assert "pagan_msa_set_sampler" in host.HOST_EXPORTED and lib.pagan_msa_set_sampler is not None
    # the calls that need no device refuse bad arguments before they look for one
    L = pgm.lib()
    out = C.c_void_p()
    assert L.pagan_fb_sample_paths(None, 1, 1, 4, 0, C.byref(out)) == abi.PAGAN_E_ARG
    assert L.pagan_fb_sample_paths_batch(1, None, 1, None, 4, 0, C.byref(out)) == abi.PAGAN_E_ARG
    assert L.pagan_fb_sample_paths_batch(0, None, 1, None, 0, 0, None) == abi.PAGAN_E_ARG            # n_paths < 1
    assert L.pagan_fb_samples_summary(None, None, None, None, None, None, None) == abi.PAGAN_E_ARG
    assert L.pagan_fb_samples_visited(None, 0, None, None) == abi.PAGAN_E_ARG
    assert L.pagan_fb_samples_result(None, 0, None) == abi.PAGAN_E_ARG
    assert L.pagan_fb_samples_ms(None, None) == abi.PAGAN_E_ARG
    L.pagan_fb_samples_destroy(None)
    assert host._lib().pagan_msa_set_sampler(None, 1) == abi.PAGAN_E_ARG


def test_predict_bytes_grows_with_the_path_steps_not_the_matrix(pg):
    for lx, ly in ((301, 281), (100001, 100001), (2, 2)):
        steps = (lx - 1) + (ly - 1)
        for k in (1, 64, 65, 1024):
            with_traces = pgm.fb_sample_predict_bytes(lx, ly, k)
            assert with_traces >= 12 * k * steps
            assert with_traces <= 12 * (k + 1) * steps + 64 * k + 8192                # (one path's pack buffer, the records)
            assert 64 * k <= pgm.fb_sample_predict_bytes(lx, ly, k, traces=False) <= 64 * k + 8192
    # the lengths' sum decides, not their product
    assert pgm.fb_sample_predict_bytes(1001, 11, 64) == pgm.fb_sample_predict_bytes(506, 506, 64)
    assert pgm.fb_sample_predict_bytes(100001, 100001, 64) < 1 << 28                 # (the matrix would be 240 GB)
    assert pgm.fb_sample_predict_bytes(301, 281, 0) == abi.PAGAN_E_ARG
    assert pgm.lib().pagan_fb_sample_predict_bytes(301, 281, 4, 2) == abi.PAGAN_E_ARG


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


def test_the_seam_still_refuses_a_sampled_walk_with_the_sampler_on_the_device(pg, oracle):
    names, seqs, nwk = synth.evolve_balanced(4, 60, branch=0.03, sub=0.03, indel_start=0.01, mean_len=3, seed=12)
    msa = host.Msa(names, seqs, nwk, use_anchors=0, sample_path=1, sample_seed=3, sample_on_device=1)
    msa.set_batch_backend(_oracle_backend(oracle))
    with pytest.raises(pgm.PaganError) as e:
        msa.align()
    assert e.value.code == abi.PAGAN_E_NODEVICE
    with pytest.raises(pgm.PaganError) as e:
        msa.align_nodes(msa.ready()[:1])
    assert e.value.code == abi.PAGAN_E_NODEVICE
    # the switch alone changes nothing about a walk that does not sample
    plain = host.Msa(names, seqs, nwk, use_anchors=0, sample_on_device=1)
    plain.set_batch_backend(_oracle_backend(oracle))
    ref = host.Msa(names, seqs, nwk, use_anchors=0)
    ref.set_batch_backend(_oracle_backend(oracle))
    assert plain.align().alignment_all() == ref.align().alignment_all()
    assert host._lib().pagan_msa_set_sampler(plain._h, 2) == abi.PAGAN_E_ARG
    # the options struct has not grown: the switch is a setter
    assert [f[0] for f in host.CMsaOpts._fields_][-3:] == ["full_probability", "sample_path", "sample_seed"]


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    out = str(tmp_path_factory.mktemp("fbsample") / "dp_fb.s")
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "--offload-device-only", "-S", "-o", out, "dp_fb.hip"],
                   check=True, cwd=CSRC, stderr=subprocess.DEVNULL)
    return open(out).read()


def test_the_sampler_kernel_has_no_scratch_and_no_spill(asm):
    """pg_fb_sample as the build compiles it: no private segment, no spilled register (the metadata's counts), and no
    instruction that touches scratch memory anywhere in its body."""
    meta = re.findall(r"\.name:\s+(\S*pg_fb_sampleE\S*)\s+\.private_segment_fixed_size:\s+(\d+)", asm)
    assert len(meta) == 1 and int(meta[0][1]) == 0, meta
    name = meta[0][0]
    at = re.search(r"\.name:\s+" + re.escape(name) + r"\s", asm).start()
    block = asm[at:asm.index(".wavefront_size", at)]
    spills = dict(re.findall(r"\.(sgpr_spill_count|vgpr_spill_count):\s+(\d+)", block))
    assert spills == {"sgpr_spill_count": "0", "vgpr_spill_count": "0"}, spills
    m = re.search(r"^%s:" % re.escape(name), asm, re.M)
    body = asm[m.end():asm.index("s_endpgm", m.end())].splitlines()
    assert len(body) > 1000                                          # (the corner, the three passes and their exps are in there)
    assert not [ln for ln in body if re.search(r"\b(scratch_|buffer_(load|store))", ln)][:3]
    assert sum("global_load" in ln for ln in body) > 10 and not any("flat_load" in ln for ln in body)
