"""The statistics recorder of the tiled fill (csrc/dp_tiles_stats.h) and its reader (tools/probe_tile_stats.py).

Like the banded kernel's (tests/test_pipe_stats_cpu.py) this build is a measuring instrument that never ships, so nothing else
notices when it stops compiling or when the kernel and the Python side disagree about where a counter lies:

  * dp_tiles.hip compiles device-only with -DPG_TILE_STATS (no GPU needed; the product's flags otherwise) and reads the clock,
    the product does not;
  * the reader finds every layout constant it needs in the header, once;
  * for every buffer size the counters lie in the buffer's last PG_TS_BACK ints (an odd buffer's begin one int earlier: the
    counters are 64-bit), 8-byte aligned, clear of the banded recorder's regions -- a statistics library carries both recorders;
  * a buffer with known counters decodes to the names the header gives them;
  * the switch is named in the header alone."""
import glob
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import check_scratch  # noqa: E402
import pipe_stats  # noqa: E402
import probe_tile_stats as tile_stats  # noqa: E402


def assembly(*defines):
    with open(check_scratch.assemble("dp_tiles.hip", extra=defines)) as f:       # (raises if hipcc fails)
        return f.read()


def test_statistics_build_compiles_and_reads_the_clock():
    text = assembly("-DPG_TILE_STATS")
    assert text.count(".amdhsa_kernel ") == 2 and "pg_fill_tiles_flow" in text
    assert "s_memtime" in text


def test_product_build_never_reads_the_clock():
    text = assembly()
    assert text.count(".amdhsa_kernel ") == 2 and "s_memtime" not in text


@pytest.fixture(scope="module")
def L():
    return tile_stats.layout()


def test_every_layout_name_is_in_the_header_once(L):
    assert all(n in L for n in tile_stats.NAMES)
    with open(tile_stats.HEADER) as f:
        text = f.read()
    for n in tile_stats.NAMES:
        assert text.count("#define %s " % n) == 1, n
    assert text.count("#define PG_TS_FIRST(n3) ") == 1
    # one index per counter
    assert sorted(L["PG_TS_" + c] for c in tile_stats.COUNTERS) == list(range(L["PG_TS_COUNTERS"]))
    assert [L["PG_TS_%s_%s" % (w, k)] - L["PG_TS_%s_SIMPLE" % w] for w in ("STEPS", "CYCLES") for k in tile_stats.KINDS] == 2 * list(range(L["PG_TS_KINDS"]))


def test_counters_lie_in_the_tail_clear_of_the_banded_recorder(L):
    P = pipe_stats.layout()
    for n3 in range(L["PG_TS_MIN_INTS"], 8193):
        at = tile_stats.first(n3, L)
        end = at + 2 * L["PG_TS_COUNTERS"]
        assert at % 2 == 0, (n3, at)                            # ints: an 8-byte boundary of the 8-byte aligned buffer
        # the last PG_TS_BACK ints; where that is an odd int (n3 odd: 3 * (Lx + Ly) can be) the even one in front of it
        assert n3 - L["PG_TS_BACK"] - n3 % 2 == at < end <= n3, (n3, at, end)
        for name, r0, r1 in pipe_stats.regions(n3, P):
            assert r1 <= at or r0 >= end, (n3, name, r0, r1, at, end)


@pytest.mark.parametrize("n3", [4096, 4097, 18001])
def test_known_counters_decode_to_their_names(L, n3):
    raw = np.full(n3, -1, np.int32)
    raw[tile_stats.first(n3, L):][:2 * L["PG_TS_COUNTERS"]] = (np.arange(L["PG_TS_COUNTERS"], dtype=np.uint64) + np.uint64(100)).view(np.int32)
    c = tile_stats.decode(raw, L)
    assert c == {"TILES": 100, "PROLOGUE": 101, "STEPS_SIMPLE": 102, "STEPS_NEAR": 103, "STEPS_LOOPS": 104,
                 "CYCLES_SIMPLE": 105, "CYCLES_NEAR": 106, "CYCLES_LOOPS": 107, "TILE_CYCLES": 108,
                 "WAIT_DIAGONALS": 109, "WAIT_NEIGHBOURS": 110, "ACQUIRE_TILE": 111, "RELEASE": 112, "LAG_WAIT": 113, "LAG_HALO": 114,
                 "FAR_STEPS": 115, "FAR_FETCHES": 116, "PAIRS": 117}
    # ... at the place the kernels have always written them
    at = (n3 - 64) & ~1
    assert list(raw[at: at + 36].view(np.uint64)) == list(range(100, 118))
    with pytest.raises(ValueError):
        tile_stats.decode(raw[:L["PG_TS_MIN_INTS"] - 1], L)


def test_the_switch_is_named_in_the_header_alone():
    named = []
    for path in sorted(glob.glob(os.path.join(check_scratch.CSRC, "*"))):
        if os.path.isfile(path):
            with open(path, errors="replace") as f:
                if "PG_TILE_STATS" in f.read():
                    named.append(os.path.basename(path))
    assert named == ["dp_tiles_stats.h"]
