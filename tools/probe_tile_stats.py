"""Diagnostic (stats build: tools/build_stamps.sh, PAGAN_DP_LIB=.../libpagan_dp_stats.so): where a tiled job's time goes.
One full-matrix pair; prints tiles, prologue cycles per tile, steps and cycles per step by kind (simple / near / loops), the
flow waits.  The counters, and where in the trace buffer's tail they lie, are stated once, in pagan2-msa_amd/csrc/dp_tiles_stats.h:
layout() reads its PG_TS_* constants (tools/pipe_stats.py's reader), decode() names a downloaded buffer's counters."""
import os, sys
import numpy as np
import pipe_stats

HEADER = os.path.join(pipe_stats.HERE, "..", "pagan2-msa_amd", "csrc", "dp_tiles_stats.h")
KINDS = ("SIMPLE", "NEAR", "LOOPS")
# one per counter, in the words decode() returns them under
COUNTERS = (["TILES", "PROLOGUE", "TILE_CYCLES"] + ["STEPS_" + k for k in KINDS] + ["CYCLES_" + k for k in KINDS] +
            ["WAIT_DIAGONALS", "WAIT_NEIGHBOURS", "ACQUIRE_TILE", "RELEASE", "LAG_WAIT", "LAG_HALO", "FAR_STEPS", "FAR_FETCHES", "PAIRS"])
# every constant decode() needs: a header that loses one is an error here, not a wrong number in the table
NAMES = ["PG_TS_MIN_INTS", "PG_TS_BACK", "PG_TS_ALIGN", "PG_TS_COUNTERS", "PG_TS_KINDS"] + ["PG_TS_" + c for c in COUNTERS]


def layout(path=HEADER):
    """{name: value} of the header's PG_TS_* constants"""
    return pipe_stats.read_header(path, "PG_TS_", NAMES, ("PG_TS_FIRST",))


def first(n3, L):
    """the int of a buffer of n3 ints at which the 64-bit counters begin (the header's PG_TS_FIRST)"""
    return pipe_stats.formula("PG_TS_FIRST", n3, L)


def decode(raw, L=None):
    """{counter: value} of a trace buffer `raw` (int32, all 3 * (Lx + Ly) ints of it), as Python ints"""
    L = L or layout()
    raw = np.ascontiguousarray(raw, dtype=np.int32)
    if len(raw) < L["PG_TS_MIN_INTS"]:
        raise ValueError("a job with fewer than %d trace ints records nothing" % L["PG_TS_MIN_INTS"])
    at = first(len(raw), L)
    c = raw[at: at + 2 * L["PG_TS_COUNTERS"]].view(np.uint64)
    return {name: int(c[L["PG_TS_" + name]]) for name in COUNTERS}


def main():
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import ctypes as C
    import bench
    import pagan2_msa_amd as pg
    from pagan2_msa_amd import host
    w = sys.argv[1] if len(sys.argv) > 1 else "cfg2_16x2kb_dna_full"
    names, seqs, newick = bench.make_inputs(w)
    cfg, leaves, length, branch, sub, indel, mean_len, anchors, alphabet = bench.WORKLOADS[w]
    msa = host.Msa(names, seqs, newick, use_anchors=anchors).align()
    for k in ([int(x) for x in sys.argv[2].split(",")] if len(sys.argv) > 2 else (0, msa.n_internal - 1)):
        left, right, model, band = msa.node_job(k)
        b = pg.Batch([(left, right, model, band)])
        b.run(); b.sync()
        pg.lib().pagan_batch_debug_poison(b._h)       # counters (tail of the trace buffer) to all ones: they come back as x - 1
        b.run(); b.sync()
        nl_, nr_ = left.n_sites, right.n_sites
        if pg.debug_route(left, right, model, band)[1]:               # aligned on compacted graphs: the device's job has their sizes
            cp = pg.debug_compact(left, right, band)
            nl_, nr_ = len(cp["keep_left"]), len(cp["keep_right"])
        n = 3 * (nl_ - 1 + nr_ - 1)
        # multi-edge / dead site statistics of what the device aligns
        deg_l = np.diff(left.bwd_off); deg_r = np.diff(right.bwd_off)
        print("  graphs: sites %d %d (device %d %d), bwd degree 0/1/2/3+ left %s right %s" % (
            left.n_sites, right.n_sites, nl_, nr_, [int((deg_l == q).sum()) for q in (0, 1, 2)] + [int((deg_l >= 3).sum())],
            [int((deg_r == q).sum()) for q in (0, 1, 2)] + [int((deg_r >= 3).sum())]))
        raw = np.zeros(n, np.int32)
        pg.lib().pagan_batch_debug_trace(b._h, 0, raw.ctypes.data_as(C.c_void_p), raw.nbytes)
        c = {name: (v + 1) % (1 << 64) for name, v in decode(raw).items()}
        ms = b.last_ms()
        tiles = max(c["TILES"], 1)
        print("node", k, "sites", left.n_sites, right.n_sites, "fill %.2f ms" % ms[0])
        print("  tiles", tiles, "prologue cycles/tile %.0f" % (c["PROLOGUE"] / tiles), "whole tile cycles/tile %.0f" % (c["TILE_CYCLES"] / tiles))
        for kind in KINDS:
            if c["STEPS_" + kind]:
                print("  %-6s steps %9d  cycles/step %.0f" % (kind.lower(), c["STEPS_" + kind], c["CYCLES_" + kind] / c["STEPS_" + kind]))
        if c["STEPS_LOOPS"]:
            print("  loops steps with a fetch from beyond the LDS window: %d (%.0f %%), such fetches one after the other per step (largest lane): %.2f; (left, right) pairs per loops step (largest lane): %.1f" %
                  (c["FAR_STEPS"], 100.0 * c["FAR_STEPS"] / c["STEPS_LOOPS"], c["FAR_FETCHES"] / max(c["FAR_STEPS"], 1), c["PAIRS"] / c["STEPS_LOOPS"]))
        print("  waits per tile: diagonals %.0f, neighbours %.0f, acquire+tile %.0f, release %.0f, lag wait %.0f, lag halo %.0f" %
              tuple(c[q] / tiles for q in ("WAIT_DIAGONALS", "WAIT_NEIGHBOURS", "ACQUIRE_TILE", "RELEASE", "LAG_WAIT", "LAG_HALO")))
        b.close()


if __name__ == "__main__":
    main()
