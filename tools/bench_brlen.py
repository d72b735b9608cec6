"""Measurement: branch lengths by maximum likelihood (csrc/dp_anc_brlen.inc) on the shapes tools/bench_anc.py uses -- the walk
over bench.make_inputs' sequences and tree, then Msa.fit_branches() from the lengths the walk aligned under -- and on the
600-leaf caterpillar of random DNA rows (one derivative evaluation: there is nothing to fit in random rows).  A tool, not a test.

One process; per workload one warm-up call, then `repeats` timed calls (3 by default), one JSON line:
  * per round the medians of up, down, branch and fold device ms (pagan_anc_fit_info's sums over the call divided by the up
    passes resp. the rounds) and the host's share: the call's wall time less every device stage, over the wall time;
  * pa_branch beside pa_up + pa_down of the same shape, as a ratio, so that a reader can place it;
  * rounds, up passes, status, loglik start -> end, chunks, device bytes.
With `refine`: align_refined(rounds=2) on the two bench families (DNA cfg4-like and protein cfg3-like, cut down to 16 x 2 kb and
16 x 300 aa so that four walks each stay short) with and without branch_lengths="ml": score, length, clades, loglik per walk.
Reported, not asserted.  Results go to stdout and, appended, to profiles/brlen_bench.jsonl.
    python tools/bench_brlen.py [repeats] [workload ... | refine]"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import bench
from pagan2_msa_amd import host, synth
import pycheck_anc as A

args = sys.argv[1:]
repeats = int(args[0]) if args and args[0].isdigit() else 3
names_given = [a for a in args if not a.isdigit()]
ALL = ["cfg4_32x100kb_dna_anchored", "cfg5_512x10kb_dna_anchored", "cfg3_64x500aa_protein_full", "codon_16x1500_anchored",
       "caterpillar_600x4096_dna"]
chosen = names_given or ALL
OUT = os.path.join(ROOT, "profiles", "brlen_bench.jsonl")


def emit(record):
    line = json.dumps(record)
    print(line, flush=True)
    with open(OUT, "a") as f:
        f.write(line + "\n")


def report(label, call, extra):
    call()
    infos, walls = [], []
    for _ in range(repeats):
        t0 = time.perf_counter()
        infos.append(call())
        walls.append((time.perf_counter() - t0) * 1e3)
    i = infos[0]
    ups, rounds = max(i["up_passes"], 1), max(i["rounds"], 1)
    med = {k: float(np.median([x[k] for x in infos])) for k in ("encode_ms", "up_ms", "down_ms", "branch_ms", "fold_ms", "total_ms")}
    device = med["encode_ms"] + med["up_ms"] + med["down_ms"] + med["branch_ms"] + med["fold_ms"]
    out = {"workload": label, "columns": i["columns"], "states": i["states"], "chunks": i["chunks"], "device_bytes": i["device_bytes"],
           "status": i["status"], "rounds": i["rounds"], "up_passes": i["up_passes"], "loglik_start": i["loglik_start"], "loglik_end": i["loglik_end"],
           "per_round_ms": {"up": med["up_ms"] / ups, "down": med["down_ms"] / rounds, "branch": med["branch_ms"] / rounds, "fold": med["fold_ms"] / rounds},
           "branch_over_up_plus_down": (med["branch_ms"] / rounds) / (med["up_ms"] / ups + med["down_ms"] / rounds),
           "call_ms": med["total_ms"], "wall_ms": float(np.median(walls)), "host_share": 1.0 - device / med["total_ms"], "repeats": repeats}
    out.update(extra)
    emit(out)


def refine():
    families = {"dna_16x2kb": (synth.evolve_balanced(16, 2000, branch=0.05, sub=0.05, indel_start=0.005, mean_len=3, seed=31), {"use_anchors": 1}),
                "protein_16x300aa": (synth.evolve_balanced(16, 300, branch=0.08, sub=0.08, indel_start=0.01, mean_len=2, seed=32, alphabet=A.PROTEIN),
                                     {"use_anchors": 0, "data_type": 2})}
    for label, ((names, seqs, _), opts) in families.items():
        for mode in (None, "ml"):
            t0 = time.perf_counter()
            msa = host.align_refined(names, seqs, rounds=2, branch_lengths=mode, **opts)
            walks = []
            for h in msa.history:
                w = {k: h[k] for k in ("alignment_length", "score", "changed_clades")}
                if mode:
                    w.update(loglik=h["loglik"], fit=h["fit"])
                walks.append(w)
            if not mode:
                walks[-1]["loglik"] = msa.ancestral().loglik
            emit({"refine": label, "branch_lengths": mode, "walks": walks, "wall_s": time.perf_counter() - t0})
            msa.close()


for workload in chosen:
    if workload == "refine":
        refine()
        continue
    if workload.startswith("caterpillar"):
        n, L = 600, 4096
        left, right, branch = A.caterpillar(n, 0.2)
        rows = A.random_rows(n, L, 1, 7, share=0.1)
        report(workload, lambda: host.anc_branch_derivs(left, right, branch, rows, 1, A.BASE_FREQ)["info"], {"n": n, "what": "one evaluation"})
        continue
    cfg, leaves, length, branch, sub, indel, mean_len, anchors, alphabet = bench.WORKLOADS[workload]
    names, seqs, newick = bench.make_inputs(workload)
    data_type = 3 if alphabet == "CODON" else 2 if len(alphabet) == 20 else 1
    t0 = time.perf_counter()
    msa = host.Msa(names, seqs, newick, use_anchors=anchors, data_type=data_type).align()
    walk_s = time.perf_counter() - t0
    report(workload, lambda: msa.fit_branches()["info"], {"n": msa.n, "walk_wall_s": walk_s, "what": "fit from the walk's lengths"})
    msa.close()
