"""Writes tests/golden/fb_plans.json: for every pair of tests/fb_plan_cases.py under every environment there, what the library's
host-only forward/backward exports answer.  No GPU.

    python tests/golden/make_fb_plan_golden.py [--tier 1|2|all] [--out FILE]

Tier 1 is the long-standing exports (pagan_fb_debug_route with its eight info words, pagan_fb_debug_decode_route, the four
*_predict_bytes), tier 2 pagan_fb_debug_plan.  The committed file was recorded from the commit BEFORE the plan moved to
dp_fb_plan.cpp: tier 1 from that commit's unmodified library (its package on PYTHONPATH, which wins over this tree's), tier 2
from a build of it that carried pagan_fb_debug_plan as a patch over its own routing functions (PAGAN_DP_LIB); --tier 1 / --tier 2
replace that tier in FILE and keep the other.  Run with neither against the library of this tree it must reproduce the
committed file byte for byte (tests/test_fb_plan_cpu.py checks the contents)."""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.append(os.path.dirname(os.path.dirname(HERE)))
sys.path.append(os.path.dirname(HERE))

import pagan2_msa_amd as pgm  # noqa: E402
import fb_plan_cases as cases  # noqa: E402


def record(tier):
    out = {}
    all_pairs = cases.pairs()
    if tier == 1:
        out["predict_bytes"] = {name: cases.predicted_bytes(pgm, left, right, band) for name, left, right, band in all_pairs}
    collect = cases.tier1 if tier == 1 else cases.tier2
    out["plans"] = {}
    for name, left, right, band in all_pairs:
        out["plans"][name] = {}
        for env in cases.ENVIRONMENTS:
            with cases.Environment(env):
                out["plans"][name][cases.env_name(env)] = collect(pgm, left, right, band)
    return out


def dumps(doc):
    """one plan a line"""
    lines = ["{"]
    for t, tier in enumerate(sorted(doc)):
        lines.append(' "%s": {' % tier)
        keys = sorted(doc[tier])
        for k, key in enumerate(keys):
            if key != "plans":
                lines.append('  "%s": %s%s' % (key, json.dumps(doc[tier][key], sort_keys=True), "," if k + 1 < len(keys) else ""))
                continue
            lines.append('  "plans": {')
            names = list(doc[tier]["plans"])
            for p, name in enumerate(names):
                lines.append('   "%s": {' % name)
                envs = list(doc[tier]["plans"][name])
                for e, env in enumerate(envs):
                    lines.append('    "%s": %s%s' % (env, json.dumps(doc[tier]["plans"][name][env], sort_keys=True), "," if e + 1 < len(envs) else ""))
                lines.append("   }" + ("," if p + 1 < len(names) else ""))
            lines.append("  }" + ("," if k + 1 < len(keys) else ""))
        lines.append(" }" + ("," if t + 1 < len(doc) else ""))
    lines.append("}")
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tier", default="all", choices=["1", "2", "all"])
    ap.add_argument("--out", default=os.path.join(HERE, "fb_plans.json"))
    args = ap.parse_args()
    doc = {}
    if args.tier != "all" and os.path.exists(args.out):
        with open(args.out) as f:
            doc = json.load(f)
    for tier in (1, 2):
        if args.tier in (str(tier), "all"):
            doc["tier%d" % tier] = record(tier)
    with open(args.out, "w") as f:
        f.write(dumps(doc))
    print("%s: %d bytes, library %s" % (args.out, os.path.getsize(args.out), pgm.LIB_PATH))


if __name__ == "__main__":
    main()
