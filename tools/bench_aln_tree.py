"""Measurement: the guide tree from the alignment (csrc/dp_alndist.hip, csrc/host_guide.cpp) on the alignments of cfg4
(32 x 100 kb) and cfg5 (512 x 10 kb) -- the leaf rows of the walk over bench.make_inputs' sequences and tree -- and on two
synthetic sets of rows from pycheck_alndist.evolve_aligned (4,096 x 10,000 and 16,384 x 2,000).  A tool, not a test.

One process; per workload one warm-up call, then `repeats` timed calls, JSON lines:
  * pack / pairs device ms (HIP events, pagan_aln_info; pairs includes the fold) and UPGMA host ms, medians; col_splits;
  * pair-words per second (a pair-word: one pair of rows over one 64-column word; the kernel computes whole tiles, so the
    tiles' pair-words are counted) beside the instruction-rate bound of the inner loop: the compiled loop issues
    VALU_PER_PAIR_WORD vector instructions a lane per pair-word (counted in the gfx950 assembly; DNA: 4 XOR, 2 OR, 2 AND, 2
    bit-select, 4 popcount-add, 1 merged add, and the address arithmetic of the x loads: 15.2; protein 24.4), a SIMD issues a
    wave's vector instruction over two cycles (32 lanes a cycle), 256 CUs x 4 SIMDs at 2.4 GHz: 7.86e13 lane-instructions a
    second;
  * the call's wall time (the walk's sets: aln_tree, tree included; the synthetic sets: pagan_aln_distances without output
    matrices -- at n = 16,384 the three n x n matrices and the tree are seconds of host work that is not what is measured here);
  * the same counts by numpy on one thread, timed on `sample` pairs, checked against the device's integers (not at
    n = 16,384), scaled to all pairs;
  * for the walk's sets: the call's share of the walk's wall time, measured here.
Then align_refined(rounds=2) on the two families: per walk the clades that differ from the true tree, the sum of the node
scores and the alignment length.  Reported, not asserted.
    python tools/bench_aln_tree.py [repeats] [sample]"""
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
os.environ.setdefault("OMP_NUM_THREADS", "1")
import numpy as np
import bench
from pagan2_msa_amd import host
import pycheck_alndist as A

repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 5
sample = int(sys.argv[2]) if len(sys.argv) > 2 else 200

# per lane: vector instructions in the loops of pad_pairs<3> (32 pair-words a pass) and pad_pairs<6> (16)
VALU_PER_PAIR_WORD = {3: 486 / 32, 6: 390 / 16}
LANE_INSTRUCTIONS_PER_S = 256 * 4 * 32 * 2.4e9


def device_only(rows, t):
    """pagan_aln_distances with no output matrix: upload, pack, pairs, download of the tiles."""
    ra = host._c_strings(rows)
    ci = host.CAlnInfo()
    L = host._lib()

    def call():
        rc = L.pagan_aln_distances(len(rows), ra, t, None, None, None, C.byref(ci))
        assert rc == 0, rc
        return host.struct_dict(ci)
    return call


def measure(label, call, n, rows, t, extra):
    call()
    infos, walls = [], []
    for _ in range(repeats):
        t0 = time.perf_counter()
        infos.append(call())
        walls.append(time.perf_counter() - t0)
    info = infos[0]
    med = {k: float(np.median([i[k] for i in infos])) for k in ("pack_ms", "pairs_ms", "upgma_ms")}
    tiles_side = (n + host.ALN_TILE - 1) // host.ALN_TILE
    words_pad = (info["words"] + host.ALN_SPLIT_WORDS - 1) // host.ALN_SPLIT_WORDS * host.ALN_SPLIT_WORDS
    pair_words = tiles_side * (tiles_side + 1) // 2 * host.ALN_TILE ** 2 * words_pad
    bound = LANE_INSTRUCTIONS_PER_S / VALU_PER_PAIR_WORD[info["planes"]]
    # numpy, one thread, a sample of pairs
    a = A.codes(rows, info["data_type"])
    v = a >= 0
    rng = np.random.default_rng(0)
    pairs = [sorted(rng.choice(n, 2, replace=False)) for _ in range(sample)]
    t0 = time.perf_counter()
    got = []
    for x, y in pairs:
        m = v[x] & v[y]
        got.append((int(m.sum()), int((m & (a[x] == a[y])).sum())))
    numpy_s = (time.perf_counter() - t0) / sample * info["pairs"]
    out = {"workload": label, "n": n, "columns": info["columns"], "words": info["words"], "planes": info["planes"],
           "pairs": info["pairs"], "col_splits": info["col_splits"], "device_bytes": info["device_bytes"], "median_ms": med,
           "tile_pair_words": pair_words, "pair_words_per_s": pair_words / (med["pairs_ms"] / 1e3),
           "bound_pair_words_per_s": bound, "share_of_bound": pair_words / (med["pairs_ms"] / 1e3) / bound,
           "call_wall_s": float(np.median(walls)), "numpy_one_thread_s_scaled_from_sample": numpy_s, "sample": sample,
           "repeats": repeats}
    out.update(extra)
    return out, pairs, got


def true_distance(newick_a, newick_true):
    return host.differing_clades(newick_a, newick_true)


for workload in ("cfg4_32x100kb_dna_anchored", "cfg5_512x10kb_dna_anchored"):
    names, seqs, newick = bench.make_inputs(workload)
    t0 = time.perf_counter()
    msa = host.Msa(names, seqs, newick).align()
    rows = msa.alignment()
    walk_s = time.perf_counter() - t0
    msa.close()
    out, pairs, got = measure(workload, lambda: host.aln_tree(names, rows, 1, with_info=True)[1], len(rows), rows, 1,
                              {"walk_wall_s": walk_s})
    both, match, _, _ = host.aln_distances(rows, 1)
    assert all((both[x, y], match[x, y]) == g for (x, y), g in zip(pairs, got))
    out["share_of_walk"] = out["call_wall_s"] / walk_s
    print(json.dumps(out), flush=True)

for n, L in ((4096, 10000), (16384, 2000)):
    _, rows = A.evolve_aligned(n, L, 0.03, 0.005, 4.0, 0)
    out, pairs, got = measure("evolve_aligned_%dx%d" % (n, L), device_only(rows, 1), n, rows, 1, {})
    if n <= 4096:
        both, match, _, _ = host.aln_distances(rows, 1)
        assert all((both[x, y], match[x, y]) == g for (x, y), g in zip(pairs, got))
    print(json.dumps(out), flush=True)

for workload in ("cfg4_32x100kb_dna_anchored", "cfg5_512x10kb_dna_anchored"):
    names, seqs, true_newick = bench.make_inputs(workload)
    t0 = time.perf_counter()
    msa = host.align_refined(names, seqs, rounds=2)
    wall = time.perf_counter() - t0
    walks = [{"clades_not_in_true_tree": true_distance(h["newick"], true_newick), "score": h["score"],
              "alignment_length": h["alignment_length"], "changed_clades": h["changed_clades"]} for h in msa.history]
    final = msa.alignment_tree()
    print(json.dumps({"refined": workload, "rounds": 2, "walks": walks, "first_tree": "k-mer guide tree",
                      "tree_of_last_alignment_clades_not_in_true_tree": true_distance(final, true_newick),
                      "fixpoint": final == msa.newick, "wall_s": wall}), flush=True)
    msa.close()
