"""Measurement: the ancestral reconstruction (csrc/dp_anc.hip) on the alignments of cfg4 (32 x 100 kb DNA), cfg5 (512 x 10 kb
DNA), cfg3 (64 x 500 aa) and the anchored codon workload (16 x 1,500 codons) -- the walk over bench.make_inputs' sequences and
tree, then pagan_msa_ancestral -- and on a 600-leaf caterpillar of random DNA rows.  A tool, not a test.

One process; per workload two warm-up calls, then `repeats` timed calls (20 by default), one JSON line:
  * encode / up / down device ms (HIP events around the launches, summed over the chunks: pagan_anc_info): medians, and the
    smallest and the largest of the calls as the spread;
  * the partials' traffic against HBM: the up pass stores one partial (S doubles) per internal node and column and loads one per
    internal child, the down pass loads partial and outside vector of every internal node, the sibling's partial per internal
    child with an internal sibling, and stores one outside vector per internal child; bytes over the pass's time beside the
    8 TB/s peak of the part.  What a cache absorbs is not subtracted: it is an upper bound on what HBM saw.
  * FMA/s: S * S multiply-adds per internal child's message in the up pass (a leaf's message is a gather, not counted), in the
    down pass the sibling's message where it is internal and S * S per outside vector; beside the fp64 vector peak
    (256 CUs x 4 SIMDs x 16 FMA lanes x 2.4 GHz = 3.93e13 FMA/s);
  * the call's wall time and the walk's, chunk size and count, device bytes.
    python tools/bench_anc.py [repeats] [workload ...]"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import bench
from pagan2_msa_amd import host
import pycheck_anc as A

HBM_BYTES_PER_S = 8.0e12
FP64_VECTOR_FMA_PER_S = 256 * 4 * 16 * 2.4e9

args = sys.argv[1:]
repeats = int(args[0]) if args else 20
ALL = ["cfg4_32x100kb_dna_anchored", "cfg5_512x10kb_dna_anchored", "cfg3_64x500aa_protein_full", "codon_16x1500_anchored",
       "caterpillar_600x4096_dna"]
chosen = args[1:] or ALL


def counts(left, right, n, S, L):
    """(bytes up, bytes down, FMAs up, FMAs down) of the whole alignment."""
    inner_children = sum((l >= n) + (r >= n) for l, r in zip(left, right))
    inner_siblings = sum((l >= n and r >= n) * 2 for l, r in zip(left, right))
    vec = S * 8 * L
    up_b = (n - 1) * vec + inner_children * vec
    down_b = 2 * (n - 1) * vec + inner_siblings * vec + inner_children * vec
    up_f = inner_children * S * S * L
    down_f = (inner_siblings + inner_children) * S * S * L
    return up_b, down_b, up_f, down_f


def report(label, call, left, right, n, extra):
    call()
    call()
    infos, walls = [], []
    for _ in range(repeats):
        t0 = time.perf_counter()
        infos.append(call())
        walls.append(time.perf_counter() - t0)
    info = infos[0]
    med = {k: float(np.median([i[k] for i in infos])) for k in ("encode_ms", "up_ms", "down_ms")}
    spread = {k: [float(min(i[k] for i in infos)), float(max(i[k] for i in infos))] for k in ("encode_ms", "up_ms", "down_ms")}
    S, L = info["states"], info["columns"]
    up_b, down_b, up_f, down_f = counts(left, right, n, S, L)
    out = {"workload": label, "n": n, "columns": L, "states": S, "chunk_cols": info["chunk_cols"], "chunks": info["chunks"],
           "matrices": info["matrices"], "device_bytes": info["device_bytes"], "median_ms": med, "min_max_ms": spread,
           "up_bytes_per_s": up_b / (med["up_ms"] / 1e3), "down_bytes_per_s": down_b / (med["down_ms"] / 1e3),
           "up_share_of_hbm_peak": up_b / (med["up_ms"] / 1e3) / HBM_BYTES_PER_S,
           "down_share_of_hbm_peak": down_b / (med["down_ms"] / 1e3) / HBM_BYTES_PER_S,
           "up_fma_per_s": up_f / (med["up_ms"] / 1e3), "down_fma_per_s": down_f / (med["down_ms"] / 1e3),
           "up_share_of_fp64_vector_peak": up_f / (med["up_ms"] / 1e3) / FP64_VECTOR_FMA_PER_S,
           "down_share_of_fp64_vector_peak": down_f / (med["down_ms"] / 1e3) / FP64_VECTOR_FMA_PER_S,
           "call_wall_s": float(np.median(walls)), "call_wall_min_max_s": [float(min(walls)), float(max(walls))],
           "repeats": repeats}
    out.update(extra)
    print(json.dumps(out), flush=True)


for workload in chosen:
    if workload.startswith("caterpillar"):
        n, L = 600, 4096
        left, right, branch = A.caterpillar(n, 0.2)
        rows = A.random_rows(n, L, 1, 7, share=0.1)
        report(workload, lambda: host.anc_reconstruct(left, right, branch, rows, 1, A.BASE_FREQ)["info"], left, right, n, {})
        continue
    cfg, leaves, length, branch, sub, indel, mean_len, anchors, alphabet = bench.WORKLOADS[workload]
    names, seqs, newick = bench.make_inputs(workload)
    data_type = 3 if alphabet == "CODON" else 2 if len(alphabet) == 20 else 1
    t0 = time.perf_counter()
    msa = host.Msa(names, seqs, newick, use_anchors=anchors, data_type=data_type).align()
    walk_s = time.perf_counter() - t0
    n = msa.n
    tree = [msa.node_info(k) for k in range(n - 1)]
    anc = [None]

    def call():
        anc[0] = msa.ancestral()
        return anc[0].info
    report(workload, call, [t.left for t in tree], [t.right for t in tree], n, {"walk_wall_s": walk_s})
    print(json.dumps({"workload": workload, "loglik": anc[0].loglik,
                      "mean_support_of_shown_states": float(np.mean([s[s >= 0].mean() for s in (anc[0].support(n + k) for k in range(n - 1))]))}),
          flush=True)
    msa.close()
