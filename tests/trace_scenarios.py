"""Planted inputs that steer the Viterbi path over chosen boundary pairs of the segmented traceback (dp_kernels.hip,
pg_trace_*), shared by tests/test_trace_plan_cpu.py (oracle + predictor: does each scenario reach the exit it is named
for?) and tests/test_trace_gpu.py (device against oracle and predictor).

A planted pair is a core sequence on both sides plus bypassed junk blocks (synth.planted_graph): without a band, or in
a band around the path the construction aims for, the best path matches core to core and leaves every block through
its one long edge.  On that path core site c sits on diagonal 2c + (junk before c on both sides), which is what `place`
solves for when a scenario wants a jump to take off from, or land on, a given diagonal."""
import functools

import numpy as np

from pagan2_msa_amd import abi, synth

import trace_plan as tp

SEG = 256


def model():
    return synth.jc_like_dna_model(0.1)


def core_states(n, seed):
    return np.random.default_rng(seed).integers(0, 4, n).astype(np.int32)


def site_of(c, blocks):
    """site of core site c (0: the start site) in planted_graph(core, blocks)"""
    return c + sum(length for pos, length in blocks if pos < c)


def place(specs, first_parity_pos=12):
    """specs: [(left length, right length, k, residue, 'land' | 'takeoff')] in rising order of diagonal.  Returns
    (left blocks, right blocks) such that the jump over spec b's block(s) lands on / takes off from diagonal k*SEG + residue;
    a bypassed one-site block on the left is put in front of a spec where the parity of the diagonals has to flip."""
    bl, br, S, last = [], [], 0, first_parity_pos - 30
    for ll, lr, k, res, mode in specs:
        T = k * SEG + res - (0 if mode == "land" else ll + lr + 2)        # the diagonal of core site pos
        if (T - S) % 2:
            bl.append((last + 30, 1))
            S += 1
        pos = (T - S) // 2
        assert pos > last + 40, "blocks too close: %r" % (specs,)
        if ll:
            bl.append((pos, ll))
        if lr:
            br.append((pos, lr))
        S += ll + lr
        last = pos
    return bl, br


def path_band(n_core_left, blocks_left, col_of_core, Ly, half):
    """Row band of +-half columns around the aimed-for path: col_of_core[c] is the right site opposite left core site c
    (c = 0: the start site); the rows of a junk block keep the interval of the core site before it (flat)."""
    centre = []
    at = dict(blocks_left)
    for c in range(n_core_left + 1):
        centre.append(col_of_core[c])
        centre.extend([col_of_core[c]] * at.get(c, 0))
    centre = np.array(centre, np.int64)
    upper = np.maximum.accumulate(np.maximum(centre - half, 0))
    lower = np.maximum.accumulate(np.minimum(centre + half, Ly - 1))
    upper[0] = 0
    lower[-1] = Ly - 1
    return abi.Band(upper, lower)


def planted_pair(n_core, blocks_left, blocks_right, seed, half=None, swap=False):
    """(left, right, model, band): the same core on both sides; half: None = the full matrix.  swap: sides exchanged."""
    if swap:
        blocks_left, blocks_right = blocks_right, blocks_left
    core = core_states(n_core, seed)
    left = synth.planted_graph(core, blocks_left, seed + 1)
    right = synth.planted_graph(core, blocks_right, seed + 2)
    band = None
    if half is not None:
        cols = [site_of(c, blocks_right) for c in range(n_core + 1)]
        band = path_band(n_core, blocks_left, cols, right.n_sites - 1, half)
    return left, right, model(), band


def with_extra_edge(g, site, src, logw, slot):
    """g with one more bwd edge src -> site at position `slot` of the site's list"""
    off = g.bwd_off.copy()
    at = int(off[site]) + slot
    off[site + 1:] += 1
    return abi.Graph(g.state, off, np.insert(g.bwd_src, at, src), np.insert(g.bwd_logw, at, np.float32(logw)),
                     np.insert(g.bwd_eid, at, g.n_edges), n_edges=g.n_edges + 1)


# ---- the scenario list --------------------------------------------------------------------------------------------------------
# name -> (builder, tags the predictor must report for it, [(land | takeoff, residue)] jumps it must contain)
SCENARIOS = {}
RESIDUES = (1, 0, -1, -2)


def scenario(name, expect=(), jumps=()):
    def reg(fn):
        SCENARIOS[name] = (fn, frozenset(expect), tuple(jumps))
        return fn
    return reg


def _lengths_specs(rot, mode, side):
    """blocks of 3, 40, 300 and 700 sites near pairs 1, 2, 4 and 7 (land) / 2, 3, 6, 10 (takeoff); block b's residue is
    RESIDUES[(rot + b) % 4], so the four rotations give every length every residue"""
    ks = (1, 2, 4, 7) if mode == "land" else ((2, 3, 6, 12) if side == "both" else (2, 3, 6, 10))
    specs = []
    for b, (length, k) in enumerate(zip((3, 40, 300, 700), ks)):
        specs.append((length, length // 2 + 1 if side == "both" else 0, k, RESIDUES[(rot + b) % 4], mode))
    return specs


def _register_lengths():
    for mode in ("land", "takeoff"):
        for rot in range(4):
            for half, width in ((None, "wide"), ((20, 40, 60, 30)[rot], "narrow")):
                for side in ("left", "right", "both"):
                    if side != "left" and rot != (1 if side == "right" else 2):
                        continue
                    name = "%s_%s_%s_rot%d" % (width, side, mode, rot)
                    specs = _lengths_specs(rot, mode, side)
                    want_jumps = [(mode, s[3]) for s in specs]
                    expect = {"miss_wide"} if half is None else {"follow2"}       # (the 700-site block spans two pairs wherever it lies)

                    def build(specs=specs, half=half, side=side, rot=rot):
                        bl, br = place(specs)
                        n_core = 1000 if side != "both" else 770
                        return planted_pair(n_core, bl, br, 100 + rot, half, swap=(side == "right"))
                    SCENARIOS[name] = (build, frozenset(expect), tuple(want_jumps))


_register_lengths()


def _comb_blocks():
    # one block of 4 junk sites at each of the pairs 6 .. 2: take off from k*SEG + 2, land on k*SEG - 4
    return place([(4, 0, k, 2, "takeoff") for k in (2, 3, 4, 5, 6)])


@scenario("comb_narrow", expect={"miss_cap", "serial_mid_path"})
def comb_narrow():
    bl, br = _comb_blocks()
    return planted_pair(1000, bl, br, 200, 25)


@scenario("comb_wide", expect={"miss_wide", "serial_mid_path"})
def comb_wide():
    # (1150 core sites: pair 7 of a 1000 x 1000 matrix lies so near the end corner that it is a narrow boundary)
    bl, br = _comb_blocks()
    return planted_pair(1150, bl, br, 200, None)


def _gap_run(swap, half, seed=300):
    """the left graph has a stretch of 40 sites the right lacks, behind core site a = 128 * 3 - 7; two bypassed blocks of 12
    junk sites inside it, the first such that the X cell behind it flies over pair 3"""
    n, a, G = 1000, 128 * 3 - 7, 40
    rng = np.random.default_rng(seed)
    core = core_states(n, seed)
    extra = rng.integers(0, 4, G).astype(np.int32)
    long_core = np.concatenate([core[:a], extra, core[a:]])
    blocks = [(a + 4, 12), (a + 22, 12)]
    g_long = synth.planted_graph(long_core, blocks, seed + 1)
    g_short = synth.planted_graph(core, [], seed + 2)
    band = None
    if half is not None:
        if not swap:
            cols = [c if c <= a else (a if c <= a + G else c - G) for c in range(n + G + 1)]
            band = path_band(n + G, blocks, cols, g_short.n_sites - 1, half)
        else:
            # rows: the short graph's sites; row a holds the whole Y run
            first = np.array([site_of(c if c <= a else c + G, blocks) for c in range(n + 1)], np.int64)
            upper = np.maximum(first - half, 0)
            lower = np.minimum(first + half, g_long.n_sites - 2)
            lower[a] = first[a + 1] + half
            upper[0] = 0
            lower[-1] = g_long.n_sites - 2
            band = abi.Band(upper, np.maximum.accumulate(lower))
    return (g_short, g_long, model(), band) if swap else (g_long, g_short, model(), band)


@scenario("gap_run_x_narrow", expect={"follow1", "gap_jump_over_pair"})
def gap_run_x_narrow():
    return _gap_run(False, 30)


@scenario("gap_run_y_narrow", expect={"follow1", "gap_jump_over_pair"})
def gap_run_y_narrow():
    return _gap_run(True, 30)


@scenario("gap_run_x_wide", expect={"miss_wide", "gap_jump_over_pair"})
def gap_run_x_wide():
    return _gap_run(False, None)


@scenario("pure_diagonal", expect={"entry"})
def pure_diagonal():
    """(c) one cell per row and per even diagonal: upper = lower = the row; every odd diagonal is empty"""
    core = core_states(1000, 400)
    g = abi.Graph.chain(core)
    rows = np.arange(g.n_sites - 1, dtype=np.int32)
    return g, abi.Graph.chain(core), model(), abi.Band(rows, rows)


def _end_pair(n_core, parity_block, half=None):
    return planted_pair(n_core, [(500, 1)] if parity_block else [], [], 500 + n_core % 7, half)


for _res, (_n, _p) in {254: (1151, False), 255: (1151, True), 0: (1024, False), 1: (1024, True)}.items():
    SCENARIOS["end_residue_%d" % _res] = (functools.partial(_end_pair, _n, _p), frozenset(), ())
    SCENARIOS["end_residue_%d_narrow" % _res] = (functools.partial(_end_pair, _n, _p, 20), frozenset(), ())


def _stop_bypass(side, three, half=None, seed=600):
    """a bypassed block of 5 junk sites behind the last core site (the stop site carries the long edge), on the left, the
    right or both; three: a third, worse edge into the stop site from two sites before the block, in front of the others"""
    n = 1020
    bl = [(n, 5)] if side in ("left", "both") else []
    br = [(n, 5)] if side in ("right", "both") else []
    left, right, m, band = planted_pair(n, bl, br, seed + 7 * three, half)
    if three:
        if bl:
            left = with_extra_edge(left, left.n_sites - 1, n - 2, -3.0, 0)
        if br:
            right = with_extra_edge(right, right.n_sites - 1, n - 2, -3.0, 0)
    return left, right, m, band


for _side in ("left", "right", "both"):
    for _three in (0, 1):
        SCENARIOS["stop_bypass_%s_%d_edges" % (_side, 2 + _three)] = (functools.partial(_stop_bypass, _side, _three), frozenset({"end_below_last"}), ())
SCENARIOS["stop_bypass_both_3_edges_narrow"] = (functools.partial(_stop_bypass, "both", 1, 20), frozenset({"end_below_last"}), ())


def _switch(total):
    """(e) Lx + Ly = total: core of 998 sites and one bypassed block of total - 1998 sites that flies over pair 3"""
    length = total - 1998
    bl, br = place([(length, 0, 3, -2, "land")])
    return planted_pair(998, bl, br, 700 + length, None)


for _total in (1999, 2000, 2001):
    SCENARIOS["switch_%d" % _total] = (functools.partial(_switch, _total), frozenset(), (("land", -2),))


def unreachable_job():
    """built like tests/golden/unreachable.npz: the band never reaches the last columns"""
    g = synth.chain_graph("ACGTACGTACGTACGTACGT")
    return g, synth.chain_graph("ACGTACGTACGTACGTACGT"), model(), abi.Band(np.zeros(21, np.int32), np.full(21, 3, np.int32))


@functools.lru_cache(maxsize=None)
def job(name):
    return SCENARIOS[name][0]()


# ---- (g) the seeded sweep ---------------------------------------------------------------------------------------------------
SWEEP_SEED = 9100           # chosen on the CPU (tests/test_trace_plan_cpu.py asserts what it was chosen for)
SWEEP_CASES, SWEEP_BATCH = 32, 8


@functools.lru_cache(maxsize=None)
def sweep_job(case):
    """0 .. 6 bypassed blocks of 1 .. 800 sites (uniform, or log-uniform for more short ones) on the left, the right or both at one position,
    in the full matrix or a band of random half-width around the aimed-for path"""
    rng = np.random.default_rng(SWEEP_SEED + case)
    n_core = int(rng.integers(1000, 1100))
    n_blocks = int(rng.integers(0, 7))
    bl, br = [], []
    for p in np.sort(rng.choice(np.arange(5, n_core + 1), n_blocks, replace=False)):
        length = int(rng.integers(1, 801)) if rng.random() < 0.6 else max(1, min(800, int(np.exp(rng.uniform(0, np.log(800.0))).round())))
        side = int(rng.integers(0, 3))
        if side in (0, 2):
            bl.append((int(p), length))
        if side in (1, 2):
            br.append((int(p), int(rng.integers(1, length + 1))))
    half = [None, 12, 25, 60, 150, 300][int(rng.integers(0, 6))]
    if half is None and (n_core + sum(l for _, l in bl)) * (n_core + sum(l for _, l in br)) > 2500000:
        half = 300                                                      # (the oracle's time: no full matrix above 2.5 M cells)
    return planted_pair(n_core, bl, br, SWEEP_SEED + 1000 + case, half)


# ---- what the oracle and the predictor say about a job ----------------------------------------------------------------------
def band_arrays(band):
    return None if band is None else (band.upper, band.lower)


def predict(result, left, right, band):
    """(visited cells, n_bound, plan) of an oracle result"""
    Lx, Ly = left.n_sites - 1, right.n_sites - 1
    widths = tp.diagonal_widths(Lx, Ly, band_arrays(band))
    K = tp.n_boundaries(Lx, Ly, widths)
    cells = tp.visited_cells(result)
    return cells, K, tp.plan(cells, widths, K)


def jumps(cells):
    """[(diagonal it takes off from, diagonal it lands on, state of the cell that takes off)] of the moves through a long edge"""
    d = cells[:, 0].astype(np.int64) + cells[:, 1]
    out = []
    for t in range(len(cells) - 1):
        if cells[t][0] - cells[t + 1][0] > 1 or cells[t][1] - cells[t + 1][1] > 1:
            out.append((int(d[t]), int(d[t + 1]), int(cells[t][2])))
    return out


def tags(cells, K, plan, left, right):
    """the names this module's scenarios use for what a path exercises"""
    out = set()
    for k, kind, followed in plan["hops"]:
        if kind == tp.ENTRY:
            out.add("entry" if followed == 0 else ("follow1" if followed == 1 else "follow2"))
        else:
            out.add(kind)
    for a, b, state in jumps(cells):
        over = [k for k in range(1, K + 1) if b < k * SEG - 1 and k * SEG < a]
        if over and state != tp.M_MAT:
            out.add("gap_jump_over_pair")
    if len(cells) and (cells[0][0] < left.n_sites - 2 or cells[0][1] < right.n_sites - 2):
        out.add("end_below_last")
    if plan["serial"] and plan["segments"] and any(t > plan["segments"][0][4] for t in plan["serial"]):
        out.add("serial_mid_path")
    return out


def jump_residues(cells):
    """{('takeoff', r), ('land', r)} with r in -2 .. 1 relative to the nearest multiple of SEG"""
    out = set()
    for a, b, _ in jumps(cells):
        for what, d in (("takeoff", a), ("land", b)):
            r = (d + 2) % SEG - 2
            if -2 <= r <= 1:
                out.add((what, r))
    return out


_ORACLE = {}


def oracle_result(oracle, key, job_):
    """the oracle's result of a scenario / sweep case, computed once per session"""
    if key not in _ORACLE:
        left, right, m, band = job_
        _ORACLE[key] = oracle.dp_align(left, right, m, band)
    return _ORACLE[key]
