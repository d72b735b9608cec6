"""The owner of a node's result and the job struct the tree walk and the pileup chain share (pagan2-msa_amd/csrc/host_job.h), no
GPU: tests/native/host_job_main.cpp -- OwnedResult and NodeJob driven through the cases host_tree.cpp and host_pileup.cpp go through,
against a pagan_result_free of the program's own that counts its calls and knows what is live -- compiled with a host compiler
under AddressSanitizer and UBSan and run as a child process.  And: the two sources free no result by hand any more."""
import os
import subprocess

import pytest

from test_fb_plan_cpu import _sanitizing_compiler

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pagan2-msa_amd", "csrc")
MAIN = os.path.join(ROOT, "tests", "native", "host_job_main.cpp")

CASES = ["adopt, destroy", "adopt over a held result", "reset, adopt", "moved by a vector that reallocates",
         "move-assign onto a held result", "an empty result", "a NodeJob moved with its band"]
FREES = [1, 2, 2, 40, 2, 1, 40]


def test_the_walk_and_the_pileup_free_no_result_by_hand():
    def text(name):
        with open(os.path.join(CSRC, name)) as f:
            return f.read()
    tree, pileup, job = text("host_tree.cpp"), text("host_pileup.cpp"), text("host_job.h")
    for word in ("getenv", "pagan_result_free", "has_res"):
        assert word not in tree, word
    assert "pagan_result_free" not in pileup and "has_res" not in pileup
    assert "#include <hip" not in job
    # the aligner is called in one place, behind the test seam or not
    assert sum(text(n).count("pagan_dp_align_batch(") for n in os.listdir(CSRC) if n.startswith("host_")) == 1


def test_owned_result_and_node_job_under_sanitizers(tmp_path):
    cxx = _sanitizing_compiler(str(tmp_path))
    if cxx is None:
        pytest.skip("no host compiler with the AddressSanitizer and UBSan runtimes")
    exe = str(tmp_path / "host_job_main")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe, MAIN],
                   check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, (run.stdout + run.stderr)[-4000:]
    assert run.stdout.splitlines() == ["%s: ok frees %d" % (c, n) for c, n in zip(CASES, FREES)]
