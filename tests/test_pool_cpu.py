"""The bookkeeping of device resources (pagan2-msa_amd/csrc/dp_pool.h), no GPU: tests/native/slab_pool_main.cpp -- literal readings
of the three pools of idle device memory and of the per-device object pool the library had before, driven beside SlabPool and
IdlePerDevice with the same seeded sequences, and a check of Carve -- compiled with a host compiler under AddressSanitizer and
UBSan and run as a child process: exit status 0, every rule of every old pool exercised, and the three policies the program runs
are the ones the library's translation units write out."""
import os
import re
import subprocess

import pytest

from test_fb_plan_cpu import _sanitizing_compiler

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pagan2-msa_amd", "csrc")
MAIN = os.path.join(ROOT, "tests", "native", "slab_pool_main.cpp")


def _policy(path, name):
    """the initialiser of `const SlabPolicy <name>` in a source file, without comments and white space"""
    with open(path) as f:
        src = f.read()
    body = re.search(r"const SlabPolicy %s = \{(.*?)\};" % name, src, re.S).group(1)
    body = re.sub(r"/\*.*?\*/|//[^\n]*", "", body, flags=re.S)
    return re.sub(r"\s+", "", body).rstrip(",")


def test_the_program_runs_the_librarys_policies():
    for name, source in (("kArenaPolicy", "dp_abi.hip"), ("kFbArenaPolicy", "dp_fb.hip"), ("kParentPolicy", "dp_parent.hip")):
        assert _policy(MAIN, name) == _policy(os.path.join(CSRC, source), name), name


def test_no_source_but_the_two_headers_defines_what_they_replaced():
    """one rounding helper, one carver with its name, no pool or owner of the old names, one getenv on a HIP error path"""
    old = ("struct ArenaPool", "struct FbArenaPool", "struct MemPool", "struct StreamPool", "struct ScratchPool", "struct GpuObjPool",
           "struct FbOwned", "struct FbDeviceScope", "size_t align_up(", "size_t fb_round256(")
    for name in sorted(os.listdir(CSRC)):
        with open(os.path.join(CSRC, name)) as f:
            text = f.read()
        assert len(re.findall(r"\bup256\s*(?:=|\(size_t)", text)) == (1 if name == "dp_pool.h" else 0), name
        assert len(re.findall(r"struct Carve\b", text)) == (1 if name == "dp_pool.h" else 0), name
        for word in old:
            assert word not in text, (name, word)
        if name.endswith(".hip"):
            assert "hipGetErrorString" not in text, name
    with open(os.path.join(CSRC, "dp_pool.h")) as f:
        text = f.read()
    assert "#include <hip" not in text and '#include "dp_hip.h"' not in text and "getenv" not in text


def test_the_pools_agree_with_the_old_ones_under_sanitizers(tmp_path):
    cxx = _sanitizing_compiler(str(tmp_path))
    if cxx is None:
        pytest.skip("no host compiler with the AddressSanitizer and UBSan runtimes")
    exe = str(tmp_path / "slab_pool_main")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe, MAIN],
                   check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, (run.stdout + run.stderr)[-4000:]
    lines = run.stdout.splitlines()
    assert [l.split(":")[0] for l in lines] == ["batch arenas", "fb arenas", "builder slabs", "objects cap 0", "objects cap 4", "carve"]
    counts = {l.split(":")[0]: dict(zip(l.split(":")[1].split()[0::2], map(int, l.split(":")[1].split()[1::2]))) for l in lines[:5]}
    assert set(counts["batch arenas"]) == {"reuse", "evicted_by_count", "smallest_while_others_stay"}
    assert set(counts["fb arenas"]) == {"reuse", "refused_for_slack", "evicted_by_count", "evicted_by_bytes"}
    assert set(counts["builder slabs"]) == {"reuse", "refused_for_slack", "evicted_by_count"}
    for pool in ("batch arenas", "fb arenas", "builder slabs"):
        assert all(v > 0 for v in counts[pool].values()), (pool, counts[pool])
    assert counts["objects cap 0"]["reuse"] > 0 and counts["objects cap 0"]["not_kept"] == 0
    assert counts["objects cap 4"]["reuse"] > 0 and counts["objects cap 4"]["not_kept"] > 0
    assert lines[5] == "carve: ok"
