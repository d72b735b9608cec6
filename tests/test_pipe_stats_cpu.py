"""The statistics recorder of the banded fill kernel (csrc/dp_pipe_stats.h) and its reader (tools/pipe_stats.py).

The statistics build is the project's measuring instrument (DESIGN's per-class cycle tables come from it) and never ships, so
nothing else notices when it stops compiling or when the kernel and the Python side disagree about where a counter lies:

  * dp_pipe.hip compiles device-only with -DPG_PIPE_STATS and with -DPG_PIPE_STATS -DPG_AS_BUCKETS (no GPU needed; the
    product's flags otherwise: tools/check_scratch.py);
  * tools/pipe_stats.py finds every layout constant it needs in the header;
  * the regions of the trace tail do not overlap, and at the smallest buffer that records anything they all lie inside the
    reserve the kernel keeps clear of the per-run records;
  * a buffer filled with 0, 1, 2, ... decodes to the offsets the header's constants say."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import check_scratch  # noqa: E402
import pipe_stats  # noqa: E402


@pytest.mark.parametrize("defines", [("-DPG_PIPE_STATS",), ("-DPG_PIPE_STATS", "-DPG_AS_BUCKETS")], ids=["stats", "stats_buckets"])
def test_statistics_build_compiles(defines):
    out = check_scratch.assemble(extra=defines)                # (raises if hipcc fails)
    with open(out) as f:
        text = f.read()
    assert text.count(".amdhsa_kernel ") == 4 and "pg_fill_pipe" in text
    # the recorder reads the cycle counter; the product never does
    assert "s_memtime" in text


@pytest.fixture(scope="module")
def L():
    return pipe_stats.layout()


def test_every_layout_name_is_in_the_header(L):
    assert all(n in L for n in pipe_stats.NAMES)
    with open(pipe_stats.HEADER) as f:
        text = f.read()
    for n in pipe_stats.NAMES:                                  # ... once each: a second definition would be a second truth
        assert text.count("#define %s " % n) == 1, n


def test_regions_do_not_overlap(L):
    # every buffer size from the threshold to well past the first one that holds a run record, and a few long jobs'
    for n3 in list(range(L["PG_ST_MIN_INTS"], 8192)) + [18000, 65536, 600006, 1200000]:
        regs = sorted(pipe_stats.regions(n3, L), key=lambda r: r[1])
        for (na, a0, a1), (nb, b0, b1) in zip(regs, regs[1:]):
            assert a0 < a1 <= b0, (n3, na, a0, a1, nb, b0, b1)
        assert regs[0][1] >= 0 and regs[-1][2] <= n3
        # the per-run records and their slot counters end in front of the reserve, the tail's regions lie inside it
        for name, first, end in regs:
            if name.startswith("RUN_"):
                assert end <= n3 - L["PG_ST_RESERVE"], (n3, name, first, end)
            else:
                assert first >= n3 - L["PG_ST_RESERVE"], (n3, name, first, end)
    assert any(n == "RUN_RECORDS" for n, _, _ in pipe_stats.regions(8191, L))


def test_all_regions_inside_the_reserve_at_the_threshold(L):
    n3 = L["PG_ST_MIN_INTS"]
    assert pipe_stats.run_cap(n3, L) <= 0                       # no room for a run record yet: nothing is written in front of the reserve
    regs = pipe_stats.regions(n3, L)
    assert sorted(n for n, _, _ in regs) == sorted(r for r, _ in pipe_stats.REGIONS)
    for name, first, end in regs:
        assert n3 - L["PG_ST_RESERVE"] <= first < end <= n3, (name, first, end)


@pytest.mark.parametrize("n3", [4096, 18000])
def test_decoding_arange_gives_the_offsets_back(L, n3):
    st = pipe_stats.decode(np.arange(n3, dtype=np.int32), L)
    ps, cs = L["PG_ST_PHASE_SHIFT"], L["PG_ST_CYCLE_SHIFT"]
    for w in range(L["PG_ST_WAVES"]):
        at = n3 - L["PG_ST_PHASE_BACK"] + L["PG_ST_PHASE_STRIDE"] * w
        assert st["phase_steps"][w] == at and list(st["phase_cycles"][w]) == [(at + 1 + k) << ps for k in range(7)]
        at = n3 - L["PG_ST_CLASS_BACK"] + L["PG_ST_CLASS_STRIDE"] * w
        assert list(st["class_steps"][w]) == [at + c for c in range(5)] and list(st["class_cycles"][w]) == [(at + 5 + c) << cs for c in range(5)]
        at = n3 - L["PG_ST_WIDE_BACK"] + L["PG_ST_WIDE_STRIDE"] * w
        assert list(st["wide_cycles"][w]) == [(at + c) << cs for c in range(4)]
        at = n3 - L["PG_ST_WAIT_BACK"] + L["PG_ST_WAIT_STRIDE"] * w
        assert list(st["wait_count"][w]) == [at + c for c in range(10)] and list(st["wait_cycles"][w]) == [(at + 10 + c) << cs for c in range(10)]
    for a in range(L["PG_ST_ASSIST_WAVES"]):
        at = n3 - L["PG_ST_ASSIST_BACK"] + L["PG_ST_ASSIST_STRIDE"] * a
        assert st["assist_diagonals"][a] == at and list(st["assist_cycles"][a]) == [(at + 1 + k) << cs for k in range(12)]
        assert (st["assist_general_whole"][a], st["assist_pairs"][a], st["assist_general_cells"][a]) == (at + 13, at + 14, at + 15)
        assert list(st["assist_why"][a]) == [at + L["PG_ST_ASSIST_WHY"] + k for k in range(6)]
    at = n3 - L["PG_ST_HWID_BACK"]
    assert list(st["hwid"]) == [at + k for k in range(L["PG_ST_HWID_FIELDS"])]
    r0 = pipe_stats.run_base(n3, L)
    assert r0 % L["PG_ST_RUN_ALIGN"] == 0 and list(st["run_count"]) == [r0 + w for w in range(L["PG_ST_WAVES"])]
    cap = st["run_cap"]
    assert st["runs"].shape == (cap, L["PG_ST_WAVES"], L["PG_ST_RUN_INTS"])
    if cap:
        slot, w = cap - 1, L["PG_ST_WAVES"] - 1
        first = r0 + L["PG_ST_RUN_HEAD"] + L["PG_ST_RUN_INTS"] * (slot * L["PG_ST_WAVES"] + w)
        assert list(st["runs"][slot][w]) == [first + k for k in range(L["PG_ST_RUN_INTS"])]
        assert first + L["PG_ST_RUN_INTS"] <= n3 - L["PG_ST_RESERVE"]
