"""CPU: oracle.dp_matrices -- the matrices oracle.dp_align fills -- pinned from three sides before anything on a GPU is held
against it: cell for cell against the second reading's matrices (tests/pycheck.py), against dp_align's own path, and against
hand-worked cell values; then the comparison helper itself (tests/dp_matrix_check.py) on arrays laid out as the device lays
them out, the tie condition of the tie-rich inputs, and every plan assertion of tests/test_dp_matrices_gpu.py (host-only calls)."""
import numpy as np
import pytest

import pagan2_msa_amd as pg_mod
from pagan2_msa_amd import abi, synth
import dp_matrix_check as mc
import pycheck
import test_dp_matrices_gpu as gpu_cases

FLAGS = [0, abi.OPT_NO_TERMINAL_EDGES, abi.OPT_NO_REDUCED_TERMINAL_PEN]


def small_job(seed, banded, p_dead=0.0, quantise=False):
    """random graphs of 20 to 60 sites, full matrix or a band a few cells wide"""
    rng = np.random.default_rng(500 + seed)
    nl, nr = (int(x) for x in rng.integers(20, 61, 2))
    left = synth.random_graph(nl, 15, 2 * seed, p_extra=0.35, max_deg=4, max_span=9, p_dead=p_dead)
    right = synth.random_graph(nr, 15, 2 * seed + 1, p_extra=0.35, max_deg=4, max_span=9, p_dead=p_dead)
    band = None
    if banded:
        Lx, Ly = left.n_sites - 1, right.n_sites - 1
        centre = np.arange(Lx) * (Ly - 1) // max(Lx - 1, 1)
        half = rng.integers(2, 9, Lx)
        upper = np.maximum.accumulate(np.maximum(centre - half, 0)); lower = np.maximum.accumulate(np.minimum(centre + half, Ly - 1))
        upper[0] = 0; lower[-1] = Ly - 1
        band = abi.Band(upper, lower)
    job = (left, right, synth.random_model(15, seed), band)
    return mc.quantised(job, seed) if quantise else job


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


@pytest.mark.parametrize("flags", FLAGS)
@pytest.mark.parametrize("kind", ["plain", "dead_sites", "ties", "ties_dead_sites"])
@pytest.mark.parametrize("banded", [False, True])
@pytest.mark.parametrize("seed", range(3))
def test_cell_for_cell_against_the_second_reading(oracle, seed, banded, kind, flags):
    left, right, model, band = small_job(seed, banded, p_dead=0.12 if "dead" in kind else 0.0, quantise="ties" in kind)
    va = pycheck.ViterbiAlignment(left, right, model, band, flags)
    va.align()
    score, ptr = va.matrices()
    want = oracle.dp_matrices(left, right, model, band, flags=flags)
    assert np.array_equal(want["begin"], va.match.lo) and np.array_equal(want["end"], va.match.hi)
    assert want["score"].shape == score.shape
    assert np.array_equal(bits(want["score"]), bits(score)), "scores differ as bit patterns"
    bad = np.argwhere(want["ptr"] != ptr)
    assert bad.size == 0, "first differing pointers (cell, state, field): %s" % bad[:5].tolist()
    assert (want["ties"][want["score"] == -np.inf] == 0).all(), "an unreachable entry has no finite candidate to tie"
    if "dead" in kind:
        i, j = mc.band_cells(left.n_sites - 1, right.n_sites - 1, band)
        assert ((want["ptr"][:, 2, 0] == -1) & (i > 0) & (j > 0)).sum() >= 10, "the inputs are meant to leave M cells unreachable"


def walk(want, end):
    """the cells (state, i, j) a traceback visits from the end corner's pointer, following oracle.dp_matrices' pointers"""
    begin = want["begin"].astype(np.int64)
    off = np.concatenate([[0], np.cumsum(np.maximum(want["end"].astype(np.int64) - begin + 1, 0))])
    state, i, j = end[0], end[1], end[2]
    cells = []
    while i >= 1 or j >= 1:
        cells.append((state, i, j))
        assert want["begin"][i] <= j <= want["end"][i]
        state, i, j = (int(v) for v in want["ptr"][off[i] + j - begin[i], state, :3])
        assert state >= 0, "the walk reached a cell without predecessor"
    assert (state, i, j) == (abi.M_MAT, 0, 0)
    return cells


@pytest.mark.parametrize("flags", FLAGS)
@pytest.mark.parametrize("seed,banded,p_dead,quantise", [(0, False, 0.0, False), (1, True, 0.0, False), (2, False, 0.12, False),
                                                          (3, True, 0.12, True), (4, False, 0.0, True)])
def test_the_pointers_lead_along_dp_aligns_path(oracle, seed, banded, p_dead, quantise, flags):
    left, right, model, band = small_job(seed, banded, p_dead, quantise)
    res = oracle.dp_align(left, right, model, band, flags=flags)
    assert res.status == 0
    want = oracle.dp_matrices(left, right, model, band, flags=flags)
    cells = pg_mod.path_cells(res.cols)                      # (state, i, j) per column, start -> end; -1 at skip columns
    on_path = [tuple(int(v) for v in c) for c in cells if c[0] >= 0]
    assert walk(want, res.end)[::-1] == on_path


def test_identical_sequences_cell_values(oracle):
    """test_oracle_cpu.test_identical_sequences_closed_form's vector, read off the matrix: M(k, k) is the k-th partial sum,
    reached from M(k - 1, k - 1) over the chain's k-th edges."""
    m = synth.jc_like_dna_model(0.1)
    s = "ACGTACGGTCATTGCA"
    g = synth.chain_graph(s)
    want = oracle.dp_matrices(g, g, m)
    n = len(s) + 1
    assert want["score"].shape == (n * n, 3) and np.array_equal(want["begin"], np.zeros(n)) and np.array_equal(want["end"], np.full(n, n - 1))
    ng = m.params[3]
    acc = 0.0
    assert want["score"][0].tolist() == [-np.inf, -np.inf, 0.0] and (want["ptr"][0] == -1).all()
    for k, c in enumerate(s, 1):
        a = synth.DNA_FULL.index(c)
        acc = acc + (float(np.float32(2) * ng) + float(m.log_score[a, a]))
        assert want["score"][k * n + k, 2] == acc
        assert want["ptr"][k * n + k, 2].tolist() == [abi.M_MAT, k - 1, k - 1, k, k]
    go, ge, gE = (float(x) for x in m.params[:3])
    # first column: X(1, 0) opens from M(0, 0) without the open penalty (reduced terminal penalties), then end-gap extensions
    assert want["score"][n, 0] == 0.0 + float(ng) + 0.0 and want["ptr"][n, 0].tolist() == [abi.M_MAT, 0, 0, 1, -1]
    assert want["score"][2 * n, 0] == want["score"][n, 0] + gE and want["ptr"][2 * n, 0].tolist() == [abi.X_MAT, 1, 0, 2, -1]
    assert want["score"][n, 1] == -np.inf and want["ptr"][n, 1].tolist() == [-1, -1, -1, -1, -1]
    assert want["ptr"][1, 1].tolist() == [abi.M_MAT, 0, 0, -1, 1] and want["ptr"][1, 0].tolist() == [-1, -1, -1, -1, -1]
    flat = oracle.dp_matrices(g, g, m, flags=abi.OPT_NO_REDUCED_TERMINAL_PEN | abi.OPT_NO_TERMINAL_EDGES)
    assert flat["score"][n, 0] == (0.0 + float(ng)) + go and flat["score"][2 * n, 0] == flat["score"][n, 0] + ge


def test_skip_edge_cell_values(oracle):
    """test_oracle_cpu.test_skip_columns_and_used_edges' vector: M(5, 3) (T against T) is reached over the long edge 8 from
    M(2, 2), and a single list position decides nothing here -- the edge from site 4 comes first and loses."""
    st = np.array([-1, 0, 1, 2, 2, 3, 0, -1], np.int32)
    off = np.array([0, 0, 1, 2, 3, 4, 6, 7, 8], np.int32)
    src = np.array([0, 1, 2, 3, 4, 2, 5, 6], np.int32)
    eid = np.array([1, 2, 3, 4, 5, 8, 6, 7], np.int32)
    left = abi.Graph(st, off, src, np.zeros(8, np.float32), eid, n_edges=9)
    right = synth.chain_graph("ACTA")
    want = oracle.dp_matrices(left, right, synth.jc_like_dna_model(0.1))
    Ly = right.n_sites - 1
    assert want["ptr"][5 * Ly + 3, 2].tolist() == [abi.M_MAT, 2, 2, 8, 3]
    assert want["ptr"][2 * Ly + 2, 2].tolist() == [abi.M_MAT, 1, 1, 2, 2]


def test_ties_count_later_equal_candidates_only(oracle):
    """Two equal edges into one left site: the second's candidates equal the first's and are turned away -- a tie in X and in M
    of that row; a chain has none anywhere."""
    m = synth.jc_like_dna_model(0.1)
    g = synth.chain_graph("ACGT")
    assert (oracle.dp_matrices(g, g, m)["ties"][:, 2] == 0).all()
    st = np.array([-1, 0, 1, 2, -1], np.int32)                    # A C G
    off = np.array([0, 0, 1, 2, 4, 5], np.int32)
    src = np.array([0, 1, 2, 2, 3], np.int32)                     # site 3 has the edge from site 2 twice
    left = abi.Graph(st, off, src, np.zeros(5, np.float32), np.array([1, 2, 3, 4, 5], np.int32), n_edges=6)
    want = oracle.dp_matrices(left, synth.chain_graph("ACG"), m)
    Ly = 4
    assert want["ties"][3 * Ly + 3, 2] == 1 and want["ptr"][3 * Ly + 3, 2].tolist() == [abi.M_MAT, 2, 2, 3, 3]
    assert want["ties"][3 * Ly + 0, 0] == 1 and want["ptr"][3 * Ly + 0, 0, 3] == 3
    assert (want["ties"][:3 * Ly] == 0).all()


# ---- the comparison helper, without a device ----------------------------------------------------------------------------------

def device_layout(job, want):
    """oracle.dp_matrices' arrays as a device would hold them: diagonal-major, pointers packed into words (written here from
    the word's definition in dp_device.h / pack_bp, independently of decode_words)."""
    left, right, _, band = job
    i, j, pos = mc.diag_index(left.n_sites - 1, right.n_sites - 1, band)
    ptr = want["ptr"].astype(np.int64)
    words = np.zeros((i.size, 3), np.uint32)
    for c in range(i.size):
        for m in range(3):
            matrix, x_ind, y_ind, xe, ye = ptr[c, m]
            if matrix < 0:
                words[c, m] = 3
                continue
            k1 = k2 = 0
            if m != 1:
                k1 = list(left.bwd_eid[left.bwd_off[i[c]]:left.bwd_off[i[c] + 1]]).index(xe)
            if m != 0:
                k2 = list(right.bwd_eid[right.bwd_off[j[c]]:right.bwd_off[j[c] + 1]]).index(ye)
            words[c, m] = matrix | (4 if m != 1 and x_ind == i[c] - 1 else 0) | (8 if m != 0 and y_ind == j[c] - 1 else 0) | k1 << 4 | k2 << 18
    sc = np.empty_like(want["score"]); bp = np.empty_like(words)
    sc[pos] = want["score"]; bp[pos] = words
    return sc, bp


@pytest.mark.parametrize("seed,banded,p_dead", [(0, False, 0.0), (1, True, 0.1), (2, True, 0.0)])
def test_the_helper_accepts_the_oracle_and_sees_every_kind_of_difference(oracle, pg, seed, banded, p_dead):
    job = small_job(seed, banded, p_dead)
    left, right, model, band = job
    want = oracle.dp_matrices(*job)
    i, j, pos = mc.diag_index(left.n_sites - 1, right.n_sites - 1, band)
    assert i.size == pg.lib().pagan_dp_count_cells(left.n_sites, right.n_sites, band.c if band else None)
    sc, bp = device_layout(job, want)
    mc.check_matrices(None, 0, job, want, arrays=(sc, bp))
    rng = np.random.default_rng(seed)
    reach = np.argwhere(want["ptr"][:, :, 0] >= 0)
    multi = [(c, m) for c, m in reach if m == 2 and left.bwd_off[i[c] + 1] - left.bwd_off[i[c]] >= 2]
    c, m = reach[rng.integers(len(reach))]
    c2, _ = multi[rng.integers(len(multi))]
    dead = np.argwhere(want["ptr"][:, :, 0] < 0)
    cd, md = dead[rng.integers(len(dead))]
    changes = {
        "one ulp in a score": lambda s, b: s.__setitem__((pos[c], m), np.nextafter(s[pos[c], m], 0.0)),
        "a NaN score": lambda s, b: s.__setitem__((pos[c], m), np.nan),
        "another from label": lambda s, b: b.__setitem__((pos[c], m), (b[pos[c], m] & ~np.uint32(3)) | np.uint32((int(b[pos[c], m] & 3) + 1) % 3)),
        "another left edge": lambda s, b: b.__setitem__((pos[c2], 2), b[pos[c2], 2] ^ np.uint32(1 << 4)),
        "a flipped ADJL bit": lambda s, b: b.__setitem__((pos[c], m), b[pos[c], m] ^ np.uint32(4)),
        "a flipped ADJR bit": lambda s, b: b.__setitem__((pos[c], m), b[pos[c], m] ^ np.uint32(8)),
        "a predecessor where there is none": lambda s, b: b.__setitem__((pos[cd], md), np.uint32(2)),
        "none where there is a predecessor": lambda s, b: b.__setitem__((pos[c], m), np.uint32(3)),
        "two cells swapped": lambda s, b: s.__setitem__(([pos[c], pos[c] - 1],), s[[pos[c] - 1, pos[c]]]),
    }
    for what, change in changes.items():
        s2, b2 = sc.copy(), bp.copy()
        change(s2, b2)
        if what == "two cells swapped" and np.array_equal(bits(s2), bits(sc)):
            continue
        with pytest.raises(AssertionError, match="differ from the oracle"):
            mc.check_matrices(None, 0, job, want, arrays=(s2, b2))


def test_diag_index_counts_what_the_library_counts(pg):
    for name in ("banded_0", "banded_3_class5_box", "tiles_wide_band", "shape_1x700", "shape_2x2"):
        left, right, _, band = gpu_cases.CASES[name].job
        i, j, pos = mc.diag_index(left.n_sites - 1, right.n_sites - 1, band)
        assert i.size == pg.lib().pagan_dp_count_cells(left.n_sites, right.n_sites, band.c if band else None), name
        d = (i + j)[np.argsort(pos)]
        assert (np.diff(d) >= 0).all(), "positions run diagonal by diagonal"


# ---- the GPU file's inputs: tie condition and plans, on the CPU ----------------------------------------------------------------

@pytest.mark.parametrize("name", gpu_cases.TIE_CASES)
def test_tie_rich_inputs_meet_their_condition_by_the_oracle_alone(oracle, name):
    case = gpu_cases.CASES[name]
    left, right, model, band = case.job
    for a in (model.table, model.params, left.bwd_logw, right.bwd_logw):
        v = np.asarray(a, np.float64)
        assert np.array_equal(v * 4, np.round(v * 4)) and not np.signbit(v[v == 0]).any(), "every parameter is a multiple of 0.25"
    assert np.unique(model.table).size <= 8 and len(set(model.params)) == 4
    assert set(np.unique(left.bwd_logw)) | set(np.unique(right.bwd_logw)) == {0.0, -0.25, -0.5}
    mc.assert_tie_rich(case.job, gpu_cases.reference(oracle, name, case.flags)[0])


@pytest.mark.parametrize("name", sorted(gpu_cases.CASES) + sorted(gpu_cases.COMPACT_CASES))
def test_the_gpu_cases_take_the_routes_and_classes_they_are_meant_to(pg, monkeypatch, name):
    """host-only plan calls: what tests/test_dp_matrices_gpu.py asserts in front of every run"""
    case = gpu_cases.CASES.get(name) or gpu_cases.COMPACT_CASES[name]
    gpu_cases.set_env(monkeypatch, case, compact=name in gpu_cases.COMPACT_CASES)
    case.assert_plan(pg)
    if name in gpu_cases.COMPACT_CASES:
        left, right, model, band = case.job
        assert pg.debug_route(left, right, model, band)[1], "the library is meant to take the dead sites out"
        comp = pg.debug_compact(left, right, band)
        assert np.array_equal(np.setdiff1d(np.arange(left.n_sites), comp["keep_left"]), mc.dead_sites(left))
        assert np.array_equal(np.setdiff1d(np.arange(right.n_sites), comp["keep_right"]), mc.dead_sites(right))
