"""Score tables and pairs for the readers of a finished forward/backward pass (test infrastructure; host only but for
walk_root_pair, which runs a walk on the device; the GPU files import it, test_mea_cpu.py holds the host-only builders to their
conditions).

Every model the project builds gives a symmetric, or nearly symmetric, joint-probability table without a zero entry, and on such
a table a transposed lookup, a skipped lookup and a stale LDS window of a kernel all pass.  Here:

  * asymmetric(mp, seed): every entry times a factor from [0.5, 1] drawn per (a, b) -- score[a, b] != score[b, a];
  * with_zeros(mp, states, seed): a random half of the off-diagonal entries among `states` set to 0, drawn per ORDERED pair, so
    that some (a, b) is 0 where (b, a) is not;
  * zeros_bite(...): the condition that makes a zero table worth its name on a pair -- a decode that skipped or transposed the
    lookup would leave another finite / -inf pattern in the score matrix, and a transposed walk back would find no step;
  * the plain leaf pairs whose widest diagonals reach the 512- and 1,024-thread instances of pg_fb_ring_decode (leaf_pairs), the
    71 x 67 graph pairs under the protein table (graph_pairs) and the codon leaf pair (codon_leaf_pair).

The path sums assume nothing of a table beyond entries >= 0: rows need not sum to anything."""
import numpy as np

from pagan2_msa_amd import abi, host, synth

import fb_testlib
from fb_testlib import random_tunnel

BF = [0.3, 0.2, 0.2, 0.3]
AA = "ARNDCQEGHILKMFPSTWYV"
CODONS = [a + b + c for a in "ACGT" for b in "ACGT" for c in "ACGT" if a + b + c not in ("TAA", "TAG", "TGA")]


def asymmetric(mp, seed):
    """a copy of `mp` whose table is not symmetric: every entry times a float32 factor from [0.5, 1]; gap parameters untouched"""
    rng = np.random.default_rng(seed)
    factor = rng.uniform(0.5, 1.0, mp.score.shape).astype(np.float32)
    score = (mp.score * factor).astype(np.float32)
    assert not np.array_equal(score, score.T)
    assert np.array_equal(score > 0, mp.score > 0) and np.all(np.isfinite(score))
    return abi.ModelProb(score, mp.gap_open, mp.gap_ext, mp.non_gap)


def with_zeros(mp, states, seed):
    """a copy of `mp` with a seeded random half of the off-diagonal entries among `states` at 0, chosen per ordered pair"""
    rng = np.random.default_rng(seed)
    st = np.array(sorted(states), np.int64)
    a, b = np.meshgrid(st, st, indexing="ij")
    off = a != b
    pairs = np.stack([a[off], b[off]], axis=1)
    pick = rng.permutation(pairs.shape[0])[:pairs.shape[0] // 2]
    score = mp.score.copy()
    score[pairs[pick, 0], pairs[pick, 1]] = 0.0
    zero = score == 0
    assert (zero & ~zero.T).any()                               # some (a, b) is 0 where (b, a) is not
    assert np.all(np.diag(score)[st] > 0)
    return abi.ModelProb(score, mp.gap_open, mp.gap_ext, mp.non_gap)


class Pair:
    """test_fb_exact_gpu.Pair's fields, and `before`: the table a zero table was made from (None for a table without zeros)"""

    def __init__(self, name, left, right, mp, band=None, before=None, model=None):
        self.name, self.left, self.right, self.mp, self.band, self.before, self.model = name, left, right, mp, band, before, model
        self.Lx, self.Ly = left.n_sites - 1, right.n_sites - 1

    def args(self):
        return (self.left, self.right, self.mp, self.band)


def bound(ref, n):
    """the decode tests' bound (test_mea_gpu.py): 1e-7 relative + 1e-12 a summed weight"""
    return 1e-7 * np.abs(ref) + 1e-12 * n


def entries(p, transposed=False):
    """[Lx, Ly]: the table entry a match at (i, j) looks up, score[left state, right state] (transposed: the other way round)"""
    sl, sr = p.left.state[:p.Lx].astype(np.int64), p.right.state[:p.Ly].astype(np.int64)
    sl[0] = sr[0] = 0                                           # (the start sites carry no state: cell row / column 0 holds no match)
    t = p.mp.score.T if transposed else p.mp.score
    e = t[sl[:, None], sr[None, :]].astype(np.float64)
    e[0, :] = e[:, 0] = 1.0
    return e


def zeros_bite(p, ex_before, mea_z):
    """Asserts that the zeros of p.mp decide what p's decode must give.  mea_z: pycheck_mea.Mea at g = 0.5 over the zero table's
    arcs; ex_before: the arc listing under p.before (the table before the zeros).

    What is NOT asserted, because it cannot hold: that a fill ignoring the zeros ends at another objective.  A match into (i, j)
    from (i-1, j-1) can always be replaced by X into (i, j-1) and Y into (i, j) (all nine transitions between X, Y and M have a
    positive probability in every model the library accepts), which visits two more cells of weight >= 0: the optimum over the
    larger path set is the optimum over the smaller one (measured on Q64z and Q257z: the two objectives are equal to the bit, and
    the blind fill walks through no zero cell).  The zeros show in the matrix and in the walk back instead:

      * skipped lookup: at least one in-band match cell with entry 0 has a predecessor with a finite score -- the reading holds
        -inf there, a kernel that does not look holds a number (check_decode compares the finite / -inf patterns);
      * transposed lookup: at least one such cell has a transposed entry > 0 (-inf there, a number from the kernel), and at least
        one cell with entry > 0 and a finite score has a transposed entry of 0 (a number there, -inf from the kernel);
      * the walk back and the samplers: the decoded path holds a match cell whose transposed entry is 0 (a transposed walk finds
        no candidate there and ends with status 2; a path drawn there has probability 0).

    Returns the four counts."""
    assert p.before is not None and mea_z.status == 0 and mea_z.g == 0.5
    e, et = entries(p), entries(p, transposed=True)
    fin = np.isfinite(mea_z.A[:, :, 2])
    assert not fin[e == 0].any(), p.name                         # (the reading itself: no match on a zero entry)
    could = np.zeros((p.Lx, p.Ly), bool)                         # zero-entry cells some arc of the table before reaches
    for i, j in zip(*np.nonzero(e == 0)):
        if not ex_before.inside(int(i), int(j)):
            continue
        could[i, j] = any(wt > 0 and ex_before.inside(pr[0], pr[1]) and np.isfinite(mea_z.A[pr[0], pr[1], pr[2]])
                          for pr, wt in ex_before.arcs_into((int(i), int(j), 2)))
    skipped = int(could.sum())
    t_minus = int((could & (et > 0)).sum())
    t_plus = int((fin & (et == 0)).sum())
    v = mea_z.visited
    m = v[v[:, 2] == 2]
    on_path = int((et[m[:, 0], m[:, 1]] == 0).sum())
    assert (e[m[:, 0], m[:, 1]] > 0).all(), p.name
    assert skipped >= 1 and t_minus >= 1 and t_plus >= 1 and on_path >= 1, (p.name, skipped, t_minus, t_plus, on_path)
    return skipped, t_minus, t_plus, on_path


def widest_diagonal(p):
    """(cells of the widest diagonal inside the band, diagonals)"""
    inb = fb_testlib.in_band(p.Lx, p.Ly, p.band)
    i, j = np.nonzero(inb)
    return int(np.bincount(i + j).max()), p.Lx + p.Ly - 1


def block_for(width):
    """the workgroup ladder of test_fb_plan_cpu.py: 64 / 128 / 256 / 512, else 1,024"""
    for b in (64, 128, 256, 512):
        if width <= b:
            return b
    return 1024


# the tables' seeds; with the pairs' seeds below they were tried on the CPU: zeros_bite holds for every zero-table pair
DNA_TABLE_SEED, DNA_ZERO_SEED = 101, 102
PROTEIN_TABLE_SEED, PROTEIN_ZERO_SEED = 201, 202
CODON_TABLE_SEED = 301


def dna_tables():
    plain = asymmetric(host.model_prob(1, 0.2, base_freq=BF), DNA_TABLE_SEED)
    return plain, with_zeros(plain, range(4), DNA_ZERO_SEED)


def protein_tables():
    plain = asymmetric(host.model_prob(2, 0.2), PROTEIN_TABLE_SEED)
    return plain, with_zeros(plain, range(20), PROTEIN_ZERO_SEED)


def _leaves(seqs, alphabet=None):
    if alphabet is None:
        return [host.HGraph.leaf(s).flatten() for s in seqs]
    return [host.HGraph.leaf(s, alphabet).flatten() for s in seqs]


def _trim(seqs, n):
    """the first sequence cut to n residues (n + 1 matrix rows), the second left at least as long"""
    assert len(seqs[0]) >= n and len(seqs[1]) >= n
    return [seqs[0][:n], seqs[1]]


# (name, evolve length, evolve seed, residues the first sequence is cut to or None)
DNA_SHAPES = (("R257", 290, 81, 270), ("R512z", 540, 82, 511), ("R513", 540, 83, 512), ("R513z", 540, 84, 512))
PROTEIN_SHAPES = (("Q64z", 300, 91, None), ("Q257z", 290, 92, 270), ("Q513z", 540, 93, 512))
Q64_TUNNEL_SEED = 35


def leaf_pairs():
    """{name: Pair}: plain leaf pairs from synth.evolve_balanced(2, n, ...), DNA under dna_tables(), protein under
    protein_tables().  Unbanded, the widest diagonal is min(Lx, Ly): one sequence is cut to set it.

      R257   DNA, asymmetric, 257 .. 300 wide           R512z  DNA, zeros, exactly 512       R513  DNA, asymmetric, exactly 513
      R513z  DNA, zeros, exactly 513                    Q64z   protein, zeros, tunnel (8, 30): <= 64 wide, more than 512 diagonals
      Q257z  protein, zeros, 257 .. 300                 Q513z  protein, zeros, exactly 513"""
    out = {}
    dna, dna_z = dna_tables()
    for name, n, seed, cut in DNA_SHAPES:
        _, seqs, _ = synth.evolve_balanced(2, n, branch=0.2, sub=0.2, indel_start=0.03, mean_len=3, seed=seed)
        gl, gr = _leaves(_trim(seqs, cut))
        z = name.endswith("z")
        out[name] = Pair(name, gl, gr, dna_z if z else dna, None, dna if z else None)
    prot, prot_z = protein_tables()
    leaf_alpha, _ = host.alphabets(2)
    for name, n, seed, cut in PROTEIN_SHAPES:
        _, seqs, _ = synth.evolve_balanced(2, n, branch=0.2, sub=0.2, indel_start=0.03, mean_len=3, seed=seed, alphabet=AA)
        gl, gr = _leaves(_trim(seqs, cut) if cut else seqs, leaf_alpha)
        assert max(gl.state[1:-1].max(), gr.state[1:-1].max()) < 20          # (the zeros lie among the states the leaves carry)
        band = random_tunnel(np.random.default_rng(Q64_TUNNEL_SEED), gl.n_sites - 1, gr.n_sites - 1, 8, 30) if name == "Q64z" else None
        out[name] = Pair(name, gl, gr, prot_z, band, prot)
    return out


# what every leaf pair must be, asserted by check_shapes(): (lowest, highest widest diagonal, more than 512 diagonals?)
WIDTHS = {"R257": (257, 300), "R512z": (512, 512), "R513": (513, 513), "R513z": (513, 513),
          "Q64z": (1, 64), "Q257z": (257, 300), "Q513z": (513, 513)}


def check_shapes(pairs):
    """{name: (widest diagonal, diagonals, workgroup size of the ladder)} with the widths leaf_pairs() promises asserted"""
    out = {}
    for name, (lo, hi) in WIDTHS.items():
        mw, nd = widest_diagonal(pairs[name])
        assert lo <= mw <= hi, (name, mw)
        if name == "Q64z":
            assert nd > 512, (name, nd)                      # two window refills
        else:
            assert mw == min(pairs[name].Lx, pairs[name].Ly)
        out[name] = (mw, nd, block_for(mw))
    return out


G211_SEEDS = (71, 72)


def graph_pairs():
    """G211 / G211z: 70 x 66 random graphs over the 20 leaf states (degree up to 4, edges that span up to 20 sites) under the
    asymmetric protein table and under its zero table: pg_fb_decode_fill, fd_preds and fd_corner at S = 211"""
    prot, prot_z = protein_tables()
    gl = synth.random_graph(70, 20, G211_SEEDS[0], p_extra=0.4, max_deg=4, max_span=20)
    gr = synth.random_graph(66, 20, G211_SEEDS[1], p_extra=0.4, max_deg=4, max_span=20)
    return {"G211": Pair("G211", gl, gr, prot), "G211z": Pair("G211z", gl, gr, prot_z, None, prot)}


def evolve_codons(n, length, seed, **kw):
    letters = "".join(chr(64 + k) for k in range(61))
    names, seqs, nwk = synth.evolve_balanced(n, length, seed=seed, alphabet=letters, **kw)
    return names, ["".join(CODONS[ord(c) - 64] for c in s) for s in seqs], nwk


def codon_table(dist, oracle):
    """asymmetric(host.model_prob(3, dist)), the host's table first held to the oracle's byte for byte"""
    mp = host.model_prob(3, dist)
    want = oracle.model_prob(3, dist)
    assert mp.table.tobytes() == want.table.tobytes() and (mp.gap_open, mp.gap_ext, mp.non_gap) == (want.gap_open, want.gap_ext, want.non_gap)
    return asymmetric(mp, CODON_TABLE_SEED)


def codon_leaf_pair(oracle):
    """K1892: two leaves of about 40 codons, one with a planted stop codon, the other with a last partial triplet"""
    _, seqs, _ = evolve_codons(2, 40, seed=95, branch=0.1, sub=0.15, indel_start=0.03, mean_len=2)
    seqs[0] = seqs[0][:30] + "TAA" + seqs[0][33:]
    seqs[1] = seqs[1] + "AC"
    gl, gr = (host.HGraph.codon_leaf(s).flatten() for s in seqs)
    assert 61 in gl.state[1:-1] and gr.n_sites - 2 == len(seqs[1]) // 3 + 1          # (the stop codon and the partial triplet read NNN)
    return Pair("K1892", gl, gr, codon_table(0.2, oracle))


def walk_root_pair(data_type, oracle=None):
    """The root job of a four-leaf walk (the one builder here that needs a device: the walk aligns the leaf pairs), under the
    asymmetric table: G211w (protein, some site state >= 20) or K1892g (codon, some site state > 61) -- graph against graph,
    ancestral states in both."""
    if data_type == 2:
        names, seqs, nwk = synth.evolve_balanced(4, 60, branch=0.08, sub=0.1, indel_start=0.03, mean_len=3, seed=57, alphabet=AA)
        mp = protein_tables()[0]
    else:
        names, seqs, nwk = evolve_codons(4, 40, seed=58, branch=0.08, sub=0.1, indel_start=0.03, mean_len=2)
        mp = codon_table(0.2, oracle)
    msa = host.Msa(names, seqs, nwk, data_type=data_type, use_anchors=0).align()
    left, right, _model, band = msa.node_job(msa.n_internal - 1)
    assert band is None and max(left.state[1:-1].max(), right.state[1:-1].max()) > (19 if data_type == 2 else 61)
    return Pair("G211w" if data_type == 2 else "K1892g", left, right, mp)


def wide_zero_pair():
    """R1024z: a DNA leaf pair of 1,024 x 1,300 cells under the zero table -- the widest diagonal a ring decode takes, every one of
    its 1,024 threads with a row, and long enough for the windows to wrap (stale_window_cells)"""
    _, seqs, _ = synth.evolve_balanced(2, 1400, branch=0.2, sub=0.2, indel_start=0.02, mean_len=3, seed=85)
    assert len(seqs[0]) >= 1023 and len(seqs[1]) >= 1299
    gl, gr = _leaves([seqs[0][:1023], seqs[1][:1299]])
    dna, dna_z = dna_tables()
    return Pair("R1024z", gl, gr, dna_z, None, dna)


def stale_window_cells(Lx, Ly, cols, refill=256):
    """pg_fb_ring_decode's row and column windows on a full Lx x Ly matrix, replayed: at every multiple of `refill` the columns up
    to d - imin + refill and the rows up to imax + refill are written at index % cols.  Returns the match cells (i, j >= 1) that
    would read another row's or column's entry -- 0 when `cols` entries are enough for the pair."""
    col, row = np.full(cols, -1), np.full(cols, -1)
    cols_hi = rows_hi = -1
    bad = 0
    for d in range(Lx + Ly - 1):
        mn, mx = max(0, d - (Ly - 1)), min(d, Lx - 1)
        if d % refill == 0:
            wc, wr = min(Ly - 1, d - mn + refill), min(Lx - 1, mx + refill)
            j, i = np.arange(cols_hi + 1, wc + 1), np.arange(rows_hi + 1, wr + 1)
            col[j % cols], row[i % cols] = j, i                  # (a refill writes fewer than `cols` entries: no index twice)
            cols_hi, rows_hi = max(cols_hi, wc), max(rows_hi, wr)
        i = np.arange(max(mn, 1), min(mx, d - 1) + 1)
        bad += int(((col[(d - i) % cols] != d - i) | (row[i % cols] != i)).sum())
    return bad
