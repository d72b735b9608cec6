#!/usr/bin/env python3
"""Which rules of the parent-graph builder does an input reach?  CPU only (the oracle and the Python reading with its
counters, tests/pycheck_parent.py); prints one line per input: its parameters and the rules beyond the common ones.

  --mode walks     random caterpillars (synth.evolve_caterpillar), aligned by the oracle's DP, branches not clamped
  --mode planted   random planted chains (tests/parent_scenarios.py): a few kinds of leaves over a small set of labels,
                   assigned to the levels at random, with random branch lengths

This is how the pinned seeds and the planted chains of tests/parent_scenarios.py were found; `--want RULE` stops at the
first input that reaches RULE and prints it in full."""
import argparse
import collections
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

COMMON = {"history_between_used_sites_unused", "history_fresh_used", "pass1_bwd_increment", "pass1_fwd_increment", "pass2_runs",
          "pass2_at_or_below_limit", "plain_x_after_y", "plain_y_after_x", "history_between_skipped_sites_unused",
          "history_ends_differ_unused", "pass1_bwd_refused", "pass1_fwd_refused", "dup_reset", "start_shorten", "stop_shorten_dup"}


def random_walk(rng):
    from pagan2_msa_amd import synth
    n, L = int(rng.integers(10, 21)), int(rng.integers(30, 101))
    branch = float(rng.choice([0.03, 0.1, 0.2, 0.3]))
    indel, mean_len = float(rng.choice([0.02, 0.04, 0.08])), float(rng.choice([1.5, 3.0, 6.0]))
    seed = int(rng.integers(0, 1000000))
    _names, seqs, _nwk = synth.evolve_caterpillar(n, L, branch=branch, indel_start=indel, mean_len=mean_len, seed=seed)
    import parent_scenarios as ps
    return ps.Scenario("walk", "dp", seqs, branch, ()), (n, L, branch, indel, mean_len, seed)


def random_planted(rng):
    import parent_scenarios as ps
    U, kinds, n = int(rng.integers(5, 13)), int(rng.integers(2, 5)), int(rng.integers(8, 21))
    masks = [[u for u in range(U) if rng.random() < 0.6] or [0] for _ in range(kinds)]
    masks[0] = list(range(U)) if rng.random() < 0.5 else masks[0]
    order, stay = [0], float(rng.choice([0.0, 0.5, 0.8]))                 # (deletion wants the same kind of leaf level after level)
    for _ in range(n - 1):
        order.append(order[-1] if len(order) > 2 and rng.random() < stay else int(rng.integers(0, kinds)))
    branch = [(float(rng.choice([0.03, 0.06, 0.1, 0.2, 0.3])), float(rng.choice([0.03, 0.06, 0.1, 0.2, 0.3]))) for _ in range(n - 1)]
    if rng.random() < 0.5:
        branch = [branch[0]] * (n - 1)
    take, y_first = str(rng.choice(["far", "near"])), bool(rng.random() < 0.5)
    leaves = [masks[k] for k in order]
    return ps.Scenario("planted", "planted", leaves, branch, (), take=take, y_first=y_first), (leaves, branch, take, y_first)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--mode", choices=("walks", "planted"), default="walks")
    ap.add_argument("--n", type=int, default=100)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--want", action="append", default=[])
    args = ap.parse_args()
    import oracle
    import parent_scenarios as ps
    from pagan2_msa_amd import host
    oracle.build()
    rng = np.random.default_rng(args.seed)
    t0, reached, unlaid = time.time(), collections.Counter(), 0
    for k in range(args.n):
        scn, params = (random_walk if args.mode == "walks" else random_planted)(rng)
        got = ps.realise(scn, oracle, host, keep=False)
        if got is None:
            unlaid += 1
            continue
        _parents, total, _per = ps.python_chain(scn, got[1])
        rules = sorted(r for r in total if r not in COMMON)
        for r in total:
            reached[r] += 1
        hit = [w for w in args.want if total[w]]
        if hit or (not args.want and args.mode == "walks"):
            print(k, params if (hit or args.mode == "walks") else "", {r: total[r] for r in rules}, flush=True)
        if hit:
            break
    print("%d inputs (%d without a path) in %.0f s; inputs reaching each rule:" % (args.n, unlaid, time.time() - t0))
    import pycheck_parent as pp
    for r in pp.RULES:
        print("  %-40s %d" % (r, reached[r]))


if __name__ == "__main__":
    main()
