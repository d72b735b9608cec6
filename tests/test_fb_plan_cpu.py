"""The forward/backward plan (dp_fb_plan.cpp), no GPU:

  * what the host-only exports answer for the pairs and environments of fb_plan_cases.py equals tests/golden/fb_plans.json, which
    was recorded before the plan moved out of dp_fb.hip (tests/golden/make_fb_plan_golden.py says how) -- and the file covers
    every schedule, both decode routes, a deep-ring plan of segments with different B and far diagonals, and for every routing
    variable a pair it moves;
  * INTEGRATION.md's list of PAGAN_FB_* switches is what FbSwitches::read parses, and nothing else in dp_fb_plan.cpp reads the
    environment;
  * the planner alone, compiled with a host compiler under AddressSanitizer and UBSan (tests/native/fb_plan_main.cpp), run as a
    child process on the same pairs and environments: exit status 0 and the library's plans."""
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import fb_plan_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pagan2-msa_amd", "csrc")


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(ROOT, "tests", "golden", "fb_plans.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def all_pairs():
    return cases.pairs()


@pytest.fixture(scope="module")
def answers(pg, all_pairs):
    """{pair: {environment: (tier 1, tier 2)}} from the library, computed once"""
    out = {}
    for name, left, right, band in all_pairs:
        out[name] = {}
        for env in cases.ENVIRONMENTS:
            with cases.Environment(env):
                out[name][cases.env_name(env)] = (cases.tier1(pg, left, right, band), cases.tier2(pg, left, right, band))
    return out


def test_the_golden_file_covers_what_it_is_there_for(golden, all_pairs):
    t1, t2 = golden["tier1"]["plans"], golden["tier2"]["plans"]
    names = [name for name, _, _, _ in all_pairs]
    assert list(t1) == names and list(t2) == names
    envs = [cases.env_name(e) for e in cases.ENVIRONMENTS]
    for name in names:
        assert list(t1[name]) == envs and list(t2[name]) == envs
    plans1 = [p for name in names for p in t1[name].values()]
    plans2 = [p for name in names for p in t2[name].values()]
    assert {p["schedule"] for p in plans1} == {0, 1, 2, 3}
    assert {p["decode_route"] for p in plans1} == {0, 1}
    assert any(len({b & 0xffff for b in p["seg_B"]}) >= 2 for p in plans2)
    assert any(any(v & 1 for v, _ in p["dfar"]) and any(b >> 16 for b in p["seg_B"]) for p in plans2)
    assert any(p["n_init"] > 32 for p in plans2)
    assert any(p["nsplit"] == 3 for p in plans2) and any(f != p["groups"] for p in plans2 for f, _ in p["groups_within"])
    for var in cases.ROUTING_VARIABLES:
        moved = [name for name in names for env, p in t1[name].items()
                 if env.split("=")[0] == var and p["schedule"] != t1[name]["default"]["schedule"]]
        assert moved, var
    assert any(t1[name]["PAGAN_FB_DECODE_RING=0"]["decode_route"] != t1[name]["default"]["decode_route"] for name in names)
    assert any(t2[name]["PAGAN_FB_RING_SPLIT=0"]["nsplit"] != t2[name]["default"]["nsplit"] for name in names)


def test_the_long_standing_exports_answer_as_before_the_plan_moved(pg, golden, all_pairs, answers):
    for name, left, right, band in all_pairs:
        assert cases.predicted_bytes(pg, left, right, band) == golden["tier1"]["predict_bytes"][name], name
        for env, (t1, _) in answers[name].items():
            assert t1 == golden["tier1"]["plans"][name][env], (name, env)
    assert sorted(golden["tier1"]["predict_bytes"]) == sorted(answers)


def test_the_whole_plan_is_the_one_from_before_it_moved(golden, answers):
    for name, by_env in answers.items():
        for env, (t1, t2) in by_env.items():
            assert t2 == golden["tier2"]["plans"][name][env], (name, env)
            assert t2["schedule"] == t1["schedule"] and t2["decode_route"] == t1["decode_route"], (name, env)
    assert sorted(golden["tier2"]["plans"]) == sorted(answers)


def test_integration_md_lists_the_switch_table():
    """INTEGRATION.md's list of the forward/backward switches names exactly the PAGAN_FB_* variables FbSwitches::read parses: the
    eleven there are, which with PAGAN_DP_VERBOSE make the twelve string literals of read()."""
    with open(os.path.join(CSRC, "dp_fb_plan.cpp")) as f:
        src = f.read()
    read = src[src.index("FbSwitches FbSwitches::read()"):]
    read = read[:read.index("\n}\n")]
    literals = set(re.findall(r'"([^"]*)"', read)) - {"0", "off"}
    assert len(literals) == 12 and "getenv" in read and "getenv" not in src.replace(read, "")
    parsed = {v for v in literals if v.startswith("PAGAN_FB_")}
    assert literals - parsed == {"PAGAN_DP_VERBOSE"} and parsed == set(cases.FB_VARIABLES)
    # (FB_TRY's error branch is dp_hip.h's hip_code: the one getenv on a HIP error path, and it reads PAGAN_DP_VERBOSE)
    fb_files = sorted(f for f in os.listdir(CSRC) if re.fullmatch(r"dp_fb_.*\.inc", f))
    assert {"dp_fb_deep.inc", "dp_fb_post.inc", "dp_fb_counts.inc", "dp_fb_sample.inc", "dp_fb_decode.inc"} <= set(fb_files)
    for name in ["dp_fb.hip", "dp_pool.h"] + fb_files:
        with open(os.path.join(CSRC, name)) as f:
            assert f.read().count("getenv") == 0, name
    with open(os.path.join(CSRC, "dp_hip.h")) as f:
        text = f.read()
    assert text.count("getenv") == 1 and re.findall(r"getenv\(([^)]*)\)", text) == ['"PAGAN_DP_VERBOSE"']
    with open(os.path.join(ROOT, "INTEGRATION.md")) as f:
        doc = f.read()
    doc = doc[doc.index("The forward/backward side's `PAGAN_FB_*` switches"):doc.index("A process that runs many forward/backward sweeps")]
    assert set(re.findall(r"PAGAN_FB_[A-Z0-9_]+", doc)) == parsed


# ---- the planner on its own, under sanitizers ----

def _sanitizing_compiler(tmp):
    """a host compiler that links and runs an AddressSanitizer + UBSan program, or None (also where a library is preloaded into
    every process: the sanitizer's runtime has to come first)"""
    if os.environ.get("LD_PRELOAD"):
        return None
    probe = os.path.join(tmp, "probe.cpp")
    with open(probe, "w") as f:
        f.write("int main() { return 0; }\n")
    for cxx in ("g++", "clang++", "/opt/rocm/llvm/bin/clang++"):
        path = shutil.which(cxx)
        if not path:
            continue
        exe = os.path.join(tmp, "probe")
        if subprocess.run([path, "-fsanitize=address,undefined", "-o", exe, probe], capture_output=True).returncode == 0 and \
                subprocess.run([exe], capture_output=True).returncode == 0:
            return path
    return None


def _write_input(path, all_pairs):
    def graph(g):
        nb = int(g.bwd_off[-1])
        bits = np.ascontiguousarray(g.bwd_logw[:nb]).view(np.uint32)
        return " ".join(str(v) for part in ([g.n_sites, g.n_edges, nb], g.state, g.bwd_off, g.bwd_src[:nb], g.bwd_eid[:nb], bits) for v in part)
    with open(path, "w") as f:
        f.write("%d %s\n" % (len(cases.CAPS), " ".join("%d %d" % c for c in cases.CAPS)))
        f.write("%d\n" % len(cases.ENVIRONMENTS))
        for env in cases.ENVIRONMENTS:
            f.write("%d %s\n" % (len(env), " ".join("%s %s" % kv for kv in sorted(env.items()))))
        f.write("%d\n" % len(all_pairs))
        for name, left, right, band in all_pairs:
            f.write("%s\n%s\n%s\n" % (name, graph(left), graph(right)))
            f.write("0\n" if band is None else "%d %s %s\n" % (len(band.upper), " ".join(map(str, band.upper)), " ".join(map(str, band.lower))))


def _plan_line(e, name, t1, t2):
    """the program's line for a plan, from the library's answers"""
    join = lambda v: "".join(" %d" % x for x in v)
    return "plan %d %s 0 %d |%s | %d %d %d %d %d %d %d %d %d |%s |%s |%s |%s |%s" % (
        e, name, t2["schedule"], join(t1["info"]), t2["groups"], t2["block"], t2["nsplit"], t2["n_init"], t2["init_dmin"], t2["segments"],
        t2["n_dfar"], t2["decode_route"], t2["decode_block"], join(g for fb in t2["groups_within"] for g in fb), join(t2["init_at"]),
        join(t2["seg_start"]), join(t2["seg_B"]), "".join(" %d:%d" % (v, n) for v, n in t2["dfar"]))


def _switches_line(e, env):
    """FbSwitches' fields for an environment, from the rules INTEGRATION.md states (defaults, "=0", set at all, clamps)"""
    num = lambda k, dflt: int(env.get("PAGAN_FB_" + k, dflt))
    on = lambda k: 0 if env.get("PAGAN_FB_" + k) == "0" else 1
    band_min = 0x7fffffff if env.get("PAGAN_FB_BAND_MIN_ND") == "off" else num("BAND_MIN_ND", 4096)
    fields = [on("RING"), num("RING_MIN_ND", 256), on("RING_SPLIT"), on("DEEP"), num("DEEP_MIN_ND", 4096), band_min,
              int("PAGAN_FB_GROUPS" in env), max(1, min(64, num("GROUPS", 1))), max(8, min(48, num("SLOTS_X16", 46))),
              max(20, min(80, num("SPLIT", 40))), int("PAGAN_FB_BWD_FIRST" in env), on("DECODE_RING")]
    return "switches %d %s" % (e, " ".join(map(str, fields)))


def test_the_planner_alone_runs_clean_under_sanitizers_and_plans_the_same(all_pairs, answers, tmp_path):
    cxx = _sanitizing_compiler(str(tmp_path))
    if cxx is None:
        pytest.skip("no host compiler with the AddressSanitizer and UBSan runtimes")
    exe = str(tmp_path / "fb_plan_main")
    subprocess.run([cxx, "-std=c++17", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                    os.path.join(ROOT, "tests", "native", "fb_plan_main.cpp"), os.path.join(CSRC, "dp_fb_plan.cpp")], check=True)
    data = str(tmp_path / "pairs.txt")
    _write_input(data, all_pairs)
    env = {k: v for k, v in os.environ.items() if k not in cases.FB_VARIABLES and k != "PAGAN_DP_VERBOSE"}
    run = subprocess.run([exe, data], capture_output=True, text=True, env=env)
    assert run.returncode == 0, run.stderr[-4000:]
    # the four ladders as dp_fb.hip wrote them out before there was one
    rows = lambda w: 1024 if w > 512 else 512 if w > 256 else 256 if w > 128 else 128 if w > 64 else 64
    threads = lambda w: 1024 if w >= 768 else 512 if w >= 384 else 256 if w >= 192 else 128 if w >= 96 else 64
    expected = ["ladder %d %d %d" % (w, rows(w), threads(w)) for rung in (64, 96, 128, 192, 256, 384, 512, 768, 1024) for w in (rung - 1, rung, rung + 1)]
    for e, environment in enumerate(cases.ENVIRONMENTS):
        expected.append(_switches_line(e, environment))
        expected += [_plan_line(e, name, *answers[name][cases.env_name(environment)]) for name, _, _, _ in all_pairs]
    lines = run.stdout.splitlines()
    assert len(lines) == len(expected)
    for got, want in zip(lines, expected):
        assert got == want
