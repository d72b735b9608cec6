"""One job per fill kernel (dp_plan.cpp: route_of), and the route pagan_dp_debug_route reports for each in the default
environment.  No GPU: the route is host code.  tests/test_routes_gpu.py runs the same jobs in one batch."""
import os
import re

import numpy as np

from pagan2_msa_amd import abi, synth


def narrow_band(left, right, half=20):
    Lx, Ly = left.n_sites - 1, right.n_sites - 1
    centre = np.arange(Lx) * (Ly - 1) // (Lx - 1)
    upper = np.maximum.accumulate(np.maximum(centre - half, 0)); lower = np.maximum.accumulate(np.minimum(centre + half, Ly - 1))
    upper[0] = 0; lower[-1] = Ly - 1
    return abi.Band(upper, lower)


def unweighted(g):       # (random_graph gives half of its edges a weight, and a weighted edge makes a site a multi-edge one)
    return abi.Graph(g.state, g.bwd_off, g.bwd_src, np.zeros_like(g.bwd_logw), g.bwd_eid, n_edges=g.n_edges)


def jobs():
    """{route: (left, right, model, band)}"""
    out = {}
    a = synth.random_graph(500, 15, 51, p_extra=0.05, max_deg=3, max_span=8)
    b = synth.random_graph(520, 15, 52, p_extra=0.05, max_deg=3, max_span=8)
    out["pg_fill_pipe"] = (a, b, synth.random_model(15, 5), narrow_band(a, b))
    a = synth.random_graph(500, 211, 61, p_extra=0.05, max_deg=3, max_span=8)
    b = synth.random_graph(520, 211, 62, p_extra=0.05, max_deg=3, max_span=8)
    out["pg_fill_pipe (large table)"] = (a, b, synth.random_model(211, 5), narrow_band(a, b))
    a = unweighted(synth.random_graph(400, 15, 8, p_extra=0.02, max_deg=3, max_span=8))
    b = unweighted(synth.random_graph(260, 15, 9, p_extra=0.02, max_deg=3, max_span=8))
    out["pg_fill_pipe (row strips)"] = (a, b, synth.random_model(15, 1), None)
    a = synth.random_graph(260, 15, 101, p_extra=0.15, max_deg=5, max_span=7)
    b = synth.random_graph(300, 15, 202, p_extra=0.15, max_deg=5, max_span=7)
    out["pg_fill_tiles_flow"] = (a, b, synth.random_model(15, 7), None)
    a = synth.random_graph(150, 15, 41, p_extra=0.1, max_deg=3, max_span=9)
    b = synth.random_graph(140, 15, 42, p_extra=0.1, max_deg=3, max_span=9)
    model = synth.random_model(15, 4)
    t = model.log_score.copy()
    t[2, 5] = t[5, 2] = np.float32(-0.0)
    out["pg_fill_wavefront"] = (a, b, abi.Model(t, *model.params), None)
    return out


def test_every_route_has_its_job(pg):
    all_jobs = jobs()
    assert sorted(all_jobs) == sorted(pg.ROUTES)
    for route, (left, right, model, band) in all_jobs.items():
        assert pg.debug_route(left, right, model, band)[0] == route
    left, right, _, _ = all_jobs["pg_fill_pipe (row strips)"]
    assert len(pg.debug_strips(left, right)) == 3


def test_integration_md_lists_the_switch_table():
    """INTEGRATION.md's list of the aligner's environment switches names exactly the variables DpSwitches::read parses."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "pagan2-msa_amd", "csrc", "dp_plan.cpp")) as f:
        src = f.read()
    read = src[src.index("DpSwitches DpSwitches::read()"):]
    read = read[:read.index("\n}\n")]
    parsed = set(re.findall(r'"(PAGAN_DP_[A-Z0-9_]+)"', read))
    assert len(parsed) >= 22 and "getenv" not in src.replace(read, "")
    with open(os.path.join(root, "INTEGRATION.md")) as f:
        doc = f.read()
    doc = doc[doc.index("switches read by the library"):doc.index("PAGAN_STORE_TIMEOUT_S")]
    assert set(re.findall(r"PAGAN_DP_[A-Z0-9_]+", doc)) == parsed
