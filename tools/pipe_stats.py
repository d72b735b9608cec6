"""The banded fill kernel's statistics (a -DPG_PIPE_STATS build: tools/build_stamps.sh), read back.

The kernel writes its counters to the tail of the job's trace buffer; where, and what each field means, is stated once, in
pagan2-msa_amd/csrc/dp_pipe_stats.h.  layout() reads the PG_ST_* constants out of that header, decode() turns a downloaded trace
buffer (pagan_batch_debug_trace) into named arrays, and the lists below name the fields for the probes' print-outs
(tools/probe_strips.py, tests/diagnostics/probe_pair.py).  Cycle counts come back in cycles: decode() undoes the kernel's shifts."""
import os
import re

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = os.path.join(HERE, "..", "pagan2-msa_amd", "csrc", "dp_pipe_stats.h")

# the regions of the trace tail: (name, waves that own a stride of it)
REGIONS = (("PHASE", "PG_ST_WAVES"), ("CLASS", "PG_ST_WAVES"), ("WIDE", "PG_ST_WAVES"), ("WAIT", "PG_ST_WAVES"),
           ("ASSIST", "PG_ST_ASSIST_WAVES"), ("HWID", None))
# every constant decode() needs: a header that loses one is an error here, not a wrong number in a table
NAMES = (["PG_ST_MIN_INTS", "PG_ST_RESERVE", "PG_ST_WAVES", "PG_ST_ASSIST_WAVES", "PG_ST_PHASE_SHIFT", "PG_ST_CYCLE_SHIFT", "PG_ST_ASSIST_WHY", "PG_ST_ASSIST_WHYS",
          "PG_ST_RUN_NUM", "PG_ST_RUN_DEN", "PG_ST_RUN_ALIGN", "PG_ST_RUN_HEAD", "PG_ST_RUN_INTS"] +
         ["PG_ST_%s_%s" % (r, k) for r, _ in REGIONS for k in ("BACK", "STRIDE", "FIELDS") if (r, k) != ("HWID", "STRIDE")])

PHASES = ("flow control", "lds wait + dpp", "descriptor request + hand-over", "compute", "commit", "carry + prefetch", "loop edge")
WIDE_BUCKETS = ("loader and neighbour flags", "shift + records + operands off the wide ring", "L2 operands", "arithmetic + stores + flag")
WAIT_KINDS = {0: "asm loop entries / diagonals run in it (M)", 1: "loader rows", 2: "loader cols", 3: "downstream (ring row reuse)", 4: "upstream (row above)",
              5: "descriptor window / asm: exits after 48 looks at the upstream flag (count), ... downstream (M)",
              6: "far: all waves 8 steps behind / asm: looks at the upstream flag (count)", 7: "rendezvous / asm: exits with no row near the band (count)",
              8: "assist wave (staged multi-edge candidates)", 9: "asm: upstream waits (count) / downstream waits (M = count / 1e6)"}
ASSIST_WHY = ("slots", "a site's shape", "the other side", "the cell's shape or an edge from site 0", "a recent operand off the ring", "the pool")


def read_header(path, prefix, names, formulas):
    """{name: value} of a statistics header's `prefix`* constants (the plain `#define NAME integer` lines); `names` and the
    function-like macros `formulas` have to be among them (the tiled fill's recorder, dp_tiles_stats.h, is read with this too:
    tools/probe_tile_stats.py)"""
    with open(path) as f:
        text = f.read()
    found = {m.group(1): int(m.group(2)) for m in re.finditer(r"^#define\s+(%s[A-Z0-9_]+)\s+(\d+)\b" % prefix, text, re.M)}
    # ... and its function-like macros of n3, as text (formula() evaluates them)
    found["formulas"] = {m.group(1): m.group(2) for m in re.finditer(r"^#define\s+(%s[A-Z_]+)\(n3\)\s+(.+)$" % prefix, text, re.M)}
    missing = [n for n in names if n not in found] + [n for n in formulas if n not in found["formulas"]]
    if missing:
        raise KeyError(os.path.basename(path) + " does not define " + ", ".join(missing))
    return found


def layout(path=HEADER):
    """{name: value} of the header's PG_ST_* constants"""
    return read_header(path, "PG_ST_", NAMES, ("PG_ST_RUN_BASE", "PG_ST_RUN_CAP"))


def formula(name, n3, L):
    """the header's function-like macro `name(n3)`, evaluated: its text with the constants put in (C's int division is Python's //
    for the non-negative operands here; a macro that another uses is expanded first)"""
    body = L["formulas"][name]
    for other, text in L["formulas"].items():
        body = body.replace("%s(n3)" % other, "(%s)" % text)
    body = re.sub(r"PG_[A-Z0-9_]+", lambda m: str(L[m.group(0)]), body).replace("/", "//")
    return eval(body, {"__builtins__": {}}, {"n3": n3})


def run_base(n3, L):
    """first int of the per-run records' region (the header's PG_ST_RUN_BASE)"""
    return formula("PG_ST_RUN_BASE", n3, L)


def run_cap(n3, L):
    """records per wave that fit in front of the reserve (the header's PG_ST_RUN_CAP; <= 0: none)"""
    # (C truncates a negative quotient towards zero, Python floors it: only the sign matters below zero, and it is the same)
    return formula("PG_ST_RUN_CAP", n3, L)


def regions(n3, L):
    """[(name, first int, one past the last)] of everything the kernel writes in a buffer of n3 ints"""
    out = []
    for r, waves in REGIONS:
        first = n3 - L["PG_ST_%s_BACK" % r]
        n = L["PG_ST_%s_FIELDS" % r] if waves is None else L["PG_ST_%s_STRIDE" % r] * (L[waves] - 1) + L["PG_ST_%s_FIELDS" % r]
        out.append((r, first, first + n))
    r0, cap = run_base(n3, L), max(run_cap(n3, L), 0)
    if cap:                                                      # (no room for a record: the kernel leaves the slot counters alone too)
        out.append(("RUN_SLOTS", r0, r0 + L["PG_ST_WAVES"]))
        out.append(("RUN_RECORDS", r0 + L["PG_ST_RUN_HEAD"], r0 + L["PG_ST_RUN_HEAD"] + L["PG_ST_RUN_INTS"] * L["PG_ST_WAVES"] * cap))
    return out


def decode(raw, L=None):
    """The counters of a trace buffer `raw` (int32, all 3 * (Lx + Ly) ints of it) by name; first index: the wave."""
    L = L or layout()
    raw = np.asarray(raw)
    n3 = len(raw)
    if n3 < L["PG_ST_MIN_INTS"]:
        raise ValueError("a job with fewer than %d trace ints records nothing" % L["PG_ST_MIN_INTS"])

    def region(r, waves):
        first, stride, fields = n3 - L["PG_ST_%s_BACK" % r], L["PG_ST_%s_STRIDE" % r], L["PG_ST_%s_FIELDS" % r]
        return np.stack([raw[first + stride * w: first + stride * w + fields] for w in range(L[waves])]).astype(np.int64)

    ph, cl, wd, wt, a = (region(r, w) for r, w in REGIONS[:5])
    cyc, why = 1 << L["PG_ST_CYCLE_SHIFT"], L["PG_ST_ASSIST_WHY"]
    nc, nk, nb = L["PG_ST_CLASS_FIELDS"] // 2, L["PG_ST_WAIT_FIELDS"] // 2, L["PG_ST_ASSIST_FIELDS"] - 4      # classes, wait kinds, assist buckets
    hw = n3 - L["PG_ST_HWID_BACK"]
    r0, cap = run_base(n3, L), max(run_cap(n3, L), 0)
    recs = r0 + L["PG_ST_RUN_HEAD"]
    return {
        "phase_steps": ph[:, 0], "phase_cycles": ph[:, 1:] << L["PG_ST_PHASE_SHIFT"],
        "class_steps": cl[:, :nc], "class_cycles": cl[:, nc:] * cyc,
        "wide_cycles": wd * cyc,
        "wait_count": wt[:, :nk], "wait_cycles": wt[:, nk:] * cyc,
        "assist_diagonals": a[:, 0], "assist_cycles": a[:, 1:1 + nb] * cyc,
        "assist_general_whole": a[:, nb + 1], "assist_pairs": a[:, nb + 2], "assist_general_cells": a[:, nb + 3],
        "assist_why": a[:, why: why + L["PG_ST_ASSIST_WHYS"]],         # (not a PG_AS_BUCKETS build: in the place of the cycle buckets 2..7)
        "hwid": raw[hw: hw + L["PG_ST_HWID_FIELDS"]].astype(np.int64),
        "run_count": raw[r0: r0 + L["PG_ST_WAVES"]].copy(), "run_cap": cap,
        "runs": raw[recs: recs + L["PG_ST_RUN_INTS"] * L["PG_ST_WAVES"] * cap].reshape(cap, L["PG_ST_WAVES"], L["PG_ST_RUN_INTS"]),
    }
