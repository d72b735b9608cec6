"""Diagnostic: one 2 x 100 kb banded alignment (python probe_pair.py [leaves [sites per leaf]]); kernel times, and with PG_STAMPS=1
and the statistics build of the library (tools/build_stamps.sh, PAGAN_DP_LIB) the fill kernel's counters (tools/pipe_stats.py)."""
import ctypes as C
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np
import pagan2_msa_amd as pg
from pagan2_msa_amd import synth, host, abi

leaves = int(sys.argv[1]) if len(sys.argv) > 1 else 2
length = int(sys.argv[2]) if len(sys.argv) > 2 else 100000     # sites per leaf (a short pair for a quick look: 3000)
names, seqs, nwk = synth.evolve_balanced(leaves, length, branch=0.01, sub=0.008, indel_start=0.0008, mean_len=4.0, seed=5)
if os.environ.get("PG_ALIGN_RING"):
    os.environ["PAGAN_DP_FILL"] = "ring"      # tree walk on the reference kernel; only the timed batch uses the experiment
msa = host.Msa(names, seqs, nwk, use_anchors=1).align()
if os.environ.get("PG_ALIGN_RING"):
    os.environ["PAGAN_DP_FILL"] = "pipe"
if os.environ.get("PG_NOSTORE"):
    os.environ["PAGAN_DP_DEBUG_FLAGS"] = "0x100"
print("timing", msa.timing())
k = msa.n_internal - 1
l, r, m, b = msa.node_job(k)
batch = pg.Batch([(l, r, m, b)])
for rep in range(3):
    batch.run(); batch.sync()
    print("node", k, "cells", batch.cells, "ms", batch.last_ms(), "nd", l.n_sites + r.n_sites - 3)
if os.environ.get("PG_STAMPS"):
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))), "tools"))
    import pipe_stats
    n_int = 3 * (l.n_sites + r.n_sites - 2)
    raw = np.zeros(n_int, np.int32)
    pg.lib().pagan_batch_debug_trace(batch._h, 0, raw.ctypes.data_as(C.c_void_p), raw.nbytes)
    st = pipe_stats.decode(raw)
    for w in range(4):
        n = max(int(st["phase_steps"][w]), 1)
        print("wave %d: %d class-0 steps with cells; cycles/step: " % (w, n) +
              ", ".join("%s %.0f" % (pipe_stats.PHASES[k], st["phase_cycles"][w][k] / n) for k in range(7)))
    for w in range(4):
        n, t = st["class_steps"][w], st["class_cycles"][w]
        print("wave %d steps with cells by class (n, Mcycles, cycles/step): " % w +
              "  ".join("c%d %d %.0fM %.0f" % (c, n[c], t[c] / 1e6, t[c] / max(n[c], 1)) for c in range(5)))
    for w in range(4):
        print("wave %d wide steps, Mcycles: " % w + ", ".join("%s %.0f" % (pipe_stats.WIDE_BUCKETS[k], st["wide_cycles"][w][k] / 1e6) for k in range(4)))
    kinds = pipe_stats.WAIT_KINDS
    for w in range(4):
        n, t = st["wait_count"][w], st["wait_cycles"][w]
        print("wave %d waits (count, Mcycles): " % w + "; ".join("%s %d %.0fM" % (kinds[k], n[k], t[k] / 1e6) for k in sorted(kinds)))
    for a_ in range(3):
        n = max(int(st["assist_diagonals"][a_]), 1)
        t = st["assist_cycles"][a_] / n
        print("assist %d: %d diagonals; cycles/diagonal: prepare (descriptors, loader) %.0f, wait for compute waves %.0f, compute %.0f, publish %.0f; "
              "inside prepare: scan %.0f, batch %.0f, decode %.0f, far: pool writes %.0f, polls for landed cells %.0f, addresses %.0f, L2 loads %.0f, poll for the descriptor window %.0f" %
              ((a_, n) + tuple(t[:12])))
        print("assist %d: %d of its diagonals went to the general code whole, %d had cells staged by it; %d passes held two diagonals; passes sent there for: " %
              (a_, int(st["assist_general_whole"][a_]), int(st["assist_general_cells"][a_]), int(st["assist_pairs"][a_])) +
              ", ".join("%s %d" % (pipe_stats.ASSIST_WHY[k], int(st["assist_why"][a_][k])) for k in range(6)))
    print("waves 0-3 compute, 4-6 assist, 7 loader: (wave slot, SIMD, CU) =", [(int(x & 15), int((x >> 4) & 3), int((x >> 8) & 15)) for x in st["hwid"]])
    if os.environ.get("PG_RUNS_OUT"):
        cnt, cap = st["run_count"], st["run_cap"]
        cls_, _w = pg.debug_plan(l, r, b)
        np.savez_compressed(os.environ["PG_RUNS_OUT"], cnt=cnt, recs=st["runs"][: int(min(cap, cnt.max()))], cls=cls_)
        print("runs of the asm loop per wave:", cnt.tolist(), "capacity", cap)
if os.environ.get("PG_CHECK"):
    import oracle
    bad = 0
    for kk in range(msa.n_internal):
        a, b2, m2, bb = msa.node_job(kk)
        want = oracle.dp_align(a, b2, m2, bb)
        ok = msa.node_result(kk).same_alignment(want)
        bad += not ok
        print("node", kk, "level", msa.node_info(kk).level, "cells", want.cells, "OK" if ok else "MISMATCH", flush=True)
    print("mismatches:", bad)
