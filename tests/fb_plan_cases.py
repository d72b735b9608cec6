"""The fixed pairs and environments the forward/backward plan is recorded and checked under (tests/golden/fb_plans.json, written by
tests/golden/make_fb_plan_golden.py, read by tests/test_fb_plan_cpu.py), and what both collect from the library's host-only exports."""
import os

import numpy as np

from pagan2_msa_amd import abi, host, synth

FB_VARIABLES = ("PAGAN_FB_RING", "PAGAN_FB_RING_MIN_ND", "PAGAN_FB_RING_SPLIT", "PAGAN_FB_DEEP", "PAGAN_FB_DEEP_MIN_ND", "PAGAN_FB_BAND_MIN_ND",
                "PAGAN_FB_GROUPS", "PAGAN_FB_SLOTS_X16", "PAGAN_FB_SPLIT", "PAGAN_FB_BWD_FIRST", "PAGAN_FB_DECODE_RING")
# the variables that move a pair's sweeps from one schedule to another
ROUTING_VARIABLES = ("PAGAN_FB_RING", "PAGAN_FB_RING_MIN_ND", "PAGAN_FB_DEEP", "PAGAN_FB_DEEP_MIN_ND", "PAGAN_FB_BAND_MIN_ND", "PAGAN_FB_GROUPS")

# default; each switch off (the set-at-all one: on), alone; each threshold at 0; no block schedule for narrow pairs; the workgroup
# override; the slot budget and its split at and beyond their clamps (8 ... 48, 20 ... 80)
ENVIRONMENTS = [{}] + [{"PAGAN_FB_" + k: "0"} for k in ("RING", "DEEP", "RING_SPLIT", "DECODE_RING")] + [{"PAGAN_FB_BWD_FIRST": "1"}] + \
    [{"PAGAN_FB_" + k: "0"} for k in ("RING_MIN_ND", "DEEP_MIN_ND", "BAND_MIN_ND")] + [{"PAGAN_FB_BAND_MIN_ND": "off"}] + \
    [{"PAGAN_FB_GROUPS": v} for v in ("1", "4", "1000")] + [{"PAGAN_FB_SLOTS_X16": v} for v in ("8", "48", "4", "100")] + \
    [{"PAGAN_FB_SPLIT": v} for v in ("20", "80", "5", "95")]
# what a launch leaves a pair's forward / backward tiled sweep: no cut, a cut, and below the two a sweep always gets
CAPS = [(64, 64), (3, 5), (1, 1)]
N_STATES = 4


def env_name(env):
    return ",".join("%s=%s" % kv for kv in sorted(env.items())) or "default"


def tunnel(Lx, Ly, half):
    """the band of half-width half[i] about the diagonal, made monotone"""
    centre = np.arange(Lx) * (Ly - 1) // max(Lx - 1, 1)
    upper = np.maximum.accumulate(np.maximum(centre - half, 0))
    lower = np.maximum.accumulate(np.minimum(centre + half, Ly - 1))
    upper[0] = 0
    lower[-1] = Ly - 1
    return abi.Band(upper.astype(np.int32), lower.astype(np.int32))


def with_edges(g, extra):
    """g with more bwd edges, extra = [(site, source, weight), ...] by rising site, each behind its site's own"""
    off, src, lw, eid, n_edges = g.bwd_off.copy(), g.bwd_src, g.bwd_logw, g.bwd_eid, g.n_edges
    for site, source, w in extra:
        k = int(off[site + 1])
        src = np.insert(src, k, source); lw = np.insert(lw, k, np.float32(np.log(w))); eid = np.insert(eid, k, n_edges)
        off[site + 1:] += 1
        n_edges += 1
    return abi.Graph(g.state, off, src, lw, eid, n_edges=n_edges)


def pairs():
    """[(name, left, right, band or None), ...]"""
    out = []
    rng = np.random.default_rng(20)
    chain = lambda n: abi.Graph.chain(rng.integers(0, 4, n))
    graph = lambda n, seed: synth.random_graph(n, 4, seed, p_extra=0.05, max_deg=3, max_span=8)
    # two leaves inside their define_tunnel band, 12,000 cell diagonals: the LDS ring (2)
    _, seqs, _ = synth.evolve_balanced(2, 6000, branch=0.02, sub=0.02, indel_start=0.003, mean_len=4, seed=47)
    gl, gr = (host.HGraph.leaf(s).flatten() for s in seqs)
    out.append(("leaves_in_tunnel", gl, gr, host.define_tunnel(seqs[0], seqs[1], seqs[0], seqs[1])[0]))
    # two graphs with multi-edge sites inside a tunnel, 5,000 cell diagonals: the deep ring (3)
    gl, gr = graph(2500, 61), graph(2560, 62)
    out.append(("graphs_in_tunnel", gl, gr, tunnel(2501, 2561, np.random.default_rng(3).integers(20, 70, 2501))))
    # the same kind under every threshold: the one-workgroup kernels (0)
    gl, gr = graph(700, 46), graph(720, 45)
    out.append(("short_graphs_in_tunnel", gl, gr, tunnel(701, 721, np.random.default_rng(3).integers(20, 70, 701))))
    # a full matrix whose widest diagonal has more than 256 cells: the block schedule (1)
    out.append(("graphs_full_matrix", graph(300, 71), graph(280, 72), None))
    # two short leaves, full matrix: below the ring's shortest pair
    out.append(("short_leaves", chain(100), chain(90), None))
    # more corner assignments than a ring sweep holds (6 x 6 edge pairs into the end sites), long and narrow: the block schedule
    n = 2100
    ends = lambda g: with_edges(g, [(n + 1, n - d, 0.5) for d in range(1, 6)])
    out.append(("many_corner_assignments", ends(chain(n)), ends(chain(n)), tunnel(n + 1, n + 1, np.full(n + 1, 12))))
    # a band that jumps: rows below 150 end at column 160, rows from 150 on begin at column 162 -- cell diagonal 311 is empty
    upper = np.where(np.arange(301) < 150, 0, 162)
    lower = np.where(np.arange(301) < 150, 160, 300)
    out.append(("empty_diagonal", chain(300), chain(300), abi.Band(upper.astype(np.int32), lower.astype(np.int32))))
    # one row
    out.append(("one_row", chain(0), chain(50), None))
    # a tunnel whose half-width steps from 20 to 150 half way, a leaf against a leaf with one more edge of reach 100 in the wide half:
    # segments of B = 64 and B = 256, and the cells of row 4,500 beyond the wide segment's ring of 16 diagonals
    n = 6000
    out.append(("stepped_tunnel", with_edges(chain(n), [(4500, 4400, 0.3)]), chain(n),
                tunnel(n + 1, n + 1, np.where(np.arange(n + 1) < 3000, 20, 150))))
    return out


class Environment:
    """the process's PAGAN_FB_* variables set to `env` (and no other), put back on exit"""

    def __init__(self, env):
        self.env = env

    def __enter__(self):
        self.saved = {k: os.environ.pop(k, None) for k in FB_VARIABLES}
        os.environ.update(self.env)

    def __exit__(self, *exc):
        for k, v in self.saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def rle(a):
    """[[value, run length], ...]"""
    out = []
    for v in (int(x) for x in a):
        if out and out[-1][0] == v:
            out[-1][1] += 1
        else:
            out.append([v, 1])
    return out


def tier1(pgm, left, right, band):
    """what the long-standing exports say under the current environment"""
    code, info = pgm.fb_route(left, right, band)
    return {"schedule": code, "info": [info[k] for k in pgm.FB_ROUTE_INFO], "decode_route": pgm.fb_decode_route(left, right, band)}


def predicted_bytes(pgm, left, right, band):
    L = pgm.lib()
    b = band.c if band is not None else None
    return [int(L.pagan_fb_predict_bytes(left.n_sites, right.n_sites, b)), int(L.pagan_fb_decode_predict_bytes(left.n_sites, right.n_sites, b)),
            int(L.pagan_fb_sample_predict_bytes(left.n_sites, right.n_sites, 3, 0)), int(L.pagan_fb_counts_predict_bytes(left.n_sites, right.n_sites, N_STATES))]


def tier2(pgm, left, right, band):
    """pagan_fb_debug_plan under the current environment, the capped workgroups for every entry of CAPS"""
    plans = [pgm.fb_plan(left, right, band, N_STATES, *caps) for caps in CAPS]
    p = plans[0]
    out = {k: p[k] for k in pgm.FB_PLAN_HEAD if k not in ("groups_fwd", "groups_bwd")}
    out["groups_within"] = [[q["groups_fwd"], q["groups_bwd"]] for q in plans]
    out["init_at"] = [int(v) for v in p["init_at"]]
    out["seg_start"] = [int(v) for v in p["seg_start"]]
    out["seg_B"] = [int(v) for v in p["seg_B"]]
    out["dfar"] = rle(p["dfar"])
    return out
