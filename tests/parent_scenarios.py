"""Planted inputs for the parent-graph builders (test infrastructure; no GPU, nothing of the HIP library beyond models and
alphabets).

The random walks of tests/test_parent_gpu.py reach the common rules of Basic_alignment::build_ancestral_sequence only.
A scenario here is a short caterpillar of builds -- ((leaf0, leaf1), leaf2), ... -- made to reach named rules
(pycheck_parent.RULES).  Its alignment paths come from one of two places:

  "dp"       the oracle's DP on sequences evolved from a pinned seed (tools/search_parent_rules.py found the seeds);
  "planted"  written down, not aligned.  Every leaf is a list of LABELS (one per site); a leaf site is matched with the
             site of the graph built so far that carries the same label, sites only the graph has are either visited as
             gaps or jumped over an edge of the graph (then they are skip columns), sites only the leaf has are gaps;
             `avoid` names, per level, labels whose sites the path must jump.
             Which edge is taken where several are admissible is the scenario's `take` ("far": the farthest, "near": the
             nearest); `y_first` puts the leaf's own sites before or behind the graph's own between two matches.  The
             visited cells go through derive(), which writes the columns in the aligner's order (between two visited
             cells the right child's skipped sites come before the left child's, test_pycheck_cpu.py) and collects the
             used edges.

No builder checks its path, so every path -- the oracle's too -- goes through validate() before a builder sees it.
realise() runs a scenario once on the oracle's graphs and keeps the result for every test of the session."""
import collections

import numpy as np

import pycheck_parent as pp

MATCHED, XGAPPED, YGAPPED, XSKIPPED, YSKIPPED = 2, 3, 4, 5, 6


class Path:
    """What a builder reads of an alignment result: (n, 3) columns (left, right, path state) and the children's used edges."""

    def __init__(self, cols, left_used, right_used):
        self.cols = np.asarray(cols, np.int32).reshape(-1, 3)
        self.left_used = np.asarray(sorted(left_used), np.int32)
        self.right_used = np.asarray(sorted(right_used), np.int32)

    def same(self, other):
        return (np.array_equal(self.cols, other.cols) and np.array_equal(self.left_used, other.left_used)
                and np.array_equal(self.right_used, other.right_used))


def _edge(g, start, end):
    """id of the first bwd edge of site `end` that starts at `start` (pairs are unique within a list), or -1"""
    for k in range(int(g.bwd_off[end]), int(g.bwd_off[end + 1])):
        if int(g.bwd_src[k]) == start:
            return int(g.bwd_eid[k])
    return -1


def derive(visited, left, right):
    """visited: the cells of the path in order, (l, r) for a match, (l, -1) / (-1, r) for a gap; left / right: the
    children flattened (abi.Graph).  -> Path.  ValueError if a step is no edge of its child."""
    nl, nr = left.state.shape[0], right.state.shape[0]
    cols, lu, ru = [], set(), set()
    lp = rp = 0
    for l, r in list(visited) + [(nl - 1, nr - 1)]:
        if r >= 0:
            if r <= rp:
                raise ValueError("right site %d after %d" % (r, rp))
            e = _edge(right, rp, r)
            if e < 0:
                raise ValueError("no right edge %d -> %d" % (rp, r))
            ru.add(e)
            cols.extend((-1, q, YSKIPPED) for q in range(rp + 1, r))
            rp = r
        if l >= 0:
            if l <= lp:
                raise ValueError("left site %d after %d" % (l, lp))
            e = _edge(left, lp, l)
            if e < 0:
                raise ValueError("no left edge %d -> %d" % (lp, l))
            lu.add(e)
            cols.extend((q, -1, XSKIPPED) for q in range(lp + 1, l))
            lp = l
        if l < 0 and r < 0:
            raise ValueError("empty cell")
        if (l, r) != (nl - 1, nr - 1):
            cols.append((l, r, MATCHED if l >= 0 and r >= 0 else XGAPPED if l >= 0 else YGAPPED))
    return Path(cols, lu, ru)


def visited_cells(cols):
    return [(int(l), int(r)) for l, r, s in cols if s in (MATCHED, XGAPPED, YGAPPED)]


def validate(path, left, right):
    """The one gate in front of every builder.  Path states in 2..6 and in keeping with which child the column has;
    monotone: the columns take each child's sites 1, 2, ... in order, all of them; every step between visited cells is an
    existing child edge; the skip columns are exactly the sites those edges jump, in the aligner's order; the used-edge
    ids are those edges.  ValueError otherwise."""
    cols = np.asarray(path.cols)
    nl, nr = left.state.shape[0], right.state.shape[0]
    if cols.ndim != 2 or cols.shape[1] != 3:
        raise ValueError("columns are not (n, 3)")
    want_l = want_r = 1
    for l, r, s in cols.tolist():
        if s not in (MATCHED, XGAPPED, YGAPPED, XSKIPPED, YSKIPPED):
            raise ValueError("path state %d" % s)
        has = (l >= 0, r >= 0)
        if has != {MATCHED: (True, True), XGAPPED: (True, False), XSKIPPED: (True, False), YGAPPED: (False, True),
                   YSKIPPED: (False, True)}[s] or (l < 0 and l != -1) or (r < 0 and r != -1):
            raise ValueError("column (%d, %d) in state %d" % (l, r, s))
        if l >= 0:
            if l != want_l:
                raise ValueError("left site %d where %d is due" % (l, want_l))
            want_l += 1
        if r >= 0:
            if r != want_r:
                raise ValueError("right site %d where %d is due" % (r, want_r))
            want_r += 1
    if want_l != nl - 1 or want_r != nr - 1:
        raise ValueError("the columns end at (%d, %d) of (%d, %d)" % (want_l, want_r, nl - 1, nr - 1))
    again = derive(visited_cells(cols), left, right)                    # (raises for a step that is no edge)
    if not np.array_equal(again.cols, cols):
        raise ValueError("skip columns are not the sites the edges jump, in the aligner's order")
    if not (np.array_equal(again.left_used, np.sort(np.asarray(path.left_used))) and
            np.array_equal(again.right_used, np.sort(np.asarray(path.right_used)))):
        raise ValueError("used edges are not the path's")
    return path


# ---- scenarios --------------------------------------------------------------------------------------------------------
class Scenario:
    """name; kind "planted" (leaves: lists of labels) or "dp" (leaves: sequences); branch: one length or one (left, right)
    pair per level; flags (one, or one per level) / leaf_flags as the builders take them; take, y_first (True, False or the
    set of levels where it holds), avoid, flip (levels at which the leaf is the LEFT child): see the module's text; rules:
    what it is there for; python: whether the Python reading follows (False for the big ones); expect: structural facts of
    the deleting build for the big ones."""

    def __init__(self, name, kind, leaves, branch, rules, flags=0, leaf_flags=0, take="far", y_first=False, flip=(),
                 avoid=None, python=True, expect=None):
        self.name, self.kind, self.leaves, self.rules = name, kind, leaves, tuple(rules)
        n = len(leaves) - 1
        b = branch if isinstance(branch, (list, tuple)) else [branch] * n
        self.branch = [(x, x) if not isinstance(x, (list, tuple)) else tuple(x) for x in b]
        assert len(self.branch) == n
        self.flags = flags if isinstance(flags, (list, tuple)) else [flags] * n
        self.leaf_flags, self.take, self.y_first, self.flip = leaf_flags, take, y_first, set(flip)
        self.python, self.expect = python, expect or {}
        self.avoid = avoid or {}                                        # level (1..) -> labels the path may not visit there
        for r in self.rules:
            assert r in pp.RULES, r

    def __repr__(self):
        return self.name


def label_sequence(labels, leaf):
    """the leaf's residues: by label, so that matched sites mostly agree, with a mismatch (an ambiguous parent) now and then"""
    return "".join("ACGT"[(u + (leaf if u % 5 == 0 else 0)) % 4] for u in labels)


def planted_cells(graph, graph_labels, real, leaf_labels, take, y_first, avoid=()):
    """The visited cells of (graph, leaf) under the rules in the module's text; graph on the left.  None: the leaf's matches
    cannot be reached over the graph's edges."""
    n = graph.state.shape[0]
    fwd = [[] for _ in range(n)]
    for e in range(1, n):
        for k in range(int(graph.bwd_off[e]), int(graph.bwd_off[e + 1])):
            fwd[int(graph.bwd_src[k])].append(e)
    where = {}
    for s in range(1, n - 1):
        if real[s]:
            where.setdefault(graph_labels[s], []).append(s)
    cells, a, last, own = [], 0, 0, []
    def walk_to(c):
        """graph sites visited from a to c (c included unless it is the stop site)"""
        reach = {c}
        for s in range(c - 1, a - 1, -1):
            if graph_labels[s] not in avoid and any(t in reach for t in fwd[s] if t <= c):
                reach.add(s)
        if a not in reach:
            return None
        out, s = [], a
        while s != c:
            cand = [t for t in fwd[s] if t <= c and t in reach]
            s = max(cand) if take == "far" else min(cand)
            out.append(s)
        return out
    for r, u in enumerate(leaf_labels, start=1):
        m = next((s for s in where.get(u, ()) if s > last), None)
        if m is None:
            own.append(r)
            continue
        steps = walk_to(m)
        if steps is None:
            own.append(r)
            continue
        gaps = [(s, -1) for s in steps[:-1]]
        ys = [(-1, q) for q in own]
        cells += (ys + gaps if y_first else gaps + ys) + [(m, r)]
        a = last = m
        own = []
    steps = walk_to(n - 1)
    if steps is None:
        return None
    gaps = [(s, -1) for s in steps[:-1]]
    ys = [(-1, q) for q in own]
    return cells + (ys + gaps if y_first else gaps + ys)


class Frozen:
    """An oracle graph as it was at one moment (the next level up marks its used edges in place): what same_graph,
    same_dump and the Python import read."""

    def __init__(self, og):
        self._f, self._a, self._w = og.flatten(), og.attrs(), og.fwd()

    def flatten(self):
        return self._f

    def attrs(self):
        return self._a

    def fwd(self):
        return self._w


class Level:
    """left / right: the children as handed in (Frozen, no used marks yet); path; parent: the oracle's (Frozen);
    left_leaf / right_leaf: index of the leaf sequence, or None for the parent of the level below"""
    __slots__ = ("left", "right", "path", "lbl", "rbl", "flags", "parent", "left_leaf", "right_leaf")


_realised = {}


def realise(scn, oracle, host, keep=True):
    """-> (leaf sequences, [Level]) with the oracle's graphs at every level; once per scenario and session.  None for a
    planted scenario whose path cannot be laid (the search's business; a listed scenario must not be one)."""
    if scn.name in _realised:
        return _realised[scn.name]
    pars = oracle.dna_parsimony()
    if scn.kind == "planted":
        seqs = [label_sequence(lab, k) for k, lab in enumerate(scn.leaves)]
    else:
        seqs = list(scn.leaves)
    g = oracle.OGraph.leaf(seqs[0], oracle.DNA_ALPHABET, scn.leaf_flags)
    labels = [None] + list(scn.leaves[0]) + [None] if scn.kind == "planted" else None
    levels = []
    bf = None
    if scn.kind == "dp":
        c = np.array([sum(s.count(x) for s in seqs) for x in "ACGT"], np.float32)
        bf = c / c.sum()
    for k in range(1, len(seqs)):
        leaf = oracle.OGraph.leaf(seqs[k], oracle.DNA_ALPHABET, scn.leaf_flags)
        (lbl, rbl), flags = scn.branch[k - 1], scn.flags[k - 1]
        flip = (k - 1) in scn.flip
        gf, lf = g.flatten(), leaf.flatten()
        if scn.kind == "planted":
            real = g.attrs()[0][:, 1] != pp.non_real
            y_first = scn.y_first if isinstance(scn.y_first, bool) else k in scn.y_first
            cells = planted_cells(gf, labels, real, scn.leaves[k], scn.take, y_first, scn.avoid.get(k, ()))
            if cells is None:
                return None
            if flip:
                cells = [(r, l) for l, r in cells]
            path = derive(cells, lf if flip else gf, gf if flip else lf)
        else:
            model, _ = host.dna_model(bf, lbl + rbl)
            res = oracle.dp_align(lf if flip else gf, gf if flip else lf, model)
            assert res.status == 0
            path = Path(res.cols, res.left_used, res.right_used)
        left, right = (leaf, g) if flip else (g, leaf)
        validate(path, left.flatten(), right.flatten())
        lv = Level()
        lv.left, lv.right, lv.path, lv.lbl, lv.rbl, lv.flags = Frozen(left), Frozen(right), path, lbl, rbl, flags
        below = 0 if k == 1 else None
        lv.left_leaf, lv.right_leaf = (k, below) if flip else (below, k)
        g = oracle.OGraph.parent(left, right, path, lbl, rbl, pars, 4, flags)
        lv.parent = Frozen(g)
        if scn.kind == "planted":
            leaf_labels = [None] + list(scn.leaves[k]) + [None]
            ll, rl = (leaf_labels, labels) if flip else (labels, leaf_labels)
            labels = [None] + [ll[l] if l >= 0 else rl[r] for l, r, _ in path.cols.tolist()] + [None]
        levels.append(lv)
    out = (seqs, levels)
    if keep:
        _realised[scn.name] = out
    return out


def python_chain(scn, levels, with_counts=True):
    """The Python reading over the levels of a realised scenario, its children imported from the oracle's dump.
    -> ([parent Sequence per level], Counter, [Counter per level])"""
    total, per, out = collections.Counter(), [], []
    import oracle
    pars = oracle.dna_parsimony()
    for lv in levels:
        def imp(og):
            return pp.Sequence.from_dump(og.flatten(), og.attrs(), og.fwd())
        c = collections.Counter()
        out.append(pp.build_parent(imp(lv.left), imp(lv.right), lv.path.cols, lv.path.left_used, lv.path.right_used, lv.lbl, lv.rbl,
                                   pars, 4, lv.flags, counter=c if with_counts else None))
        per.append(c)
        total.update(c)
    return out, total, per


def run_structure(parent_attrs):
    """(runs of skipped sites, deleted sites) of a built parent, from its site attributes alone"""
    sa = parent_attrs[0]
    sk = np.isin(sa[:, 2], (XSKIPPED, YSKIPPED))
    runs = int((sk[1:] & ~sk[:-1]).sum())
    return runs, int((sa[:, 1] == pp.non_real).sum())


# ---- the library -------------------------------------------------------------------------------------------------------
def tiled(motif_leaves, k, pad=0):
    """the motif's leaves with the labels of k copies side by side (copy t's labels offset by t * stride), then `pad` plain
    matched sites that every leaf has"""
    stride = 1 + max(max(l) for l in motif_leaves if l)
    out = []
    for lab in motif_leaves:
        out.append([u + t * stride for t in range(k) for u in lab] + [k * stride + p for p in range(pad)])
    return out

# Two chains carry the fixpoint of the device builder's boundary pass.  Both rest on one observation about the rules: a
# site d that is deleted in one run can only decide a LATER run through an edge whose counter grew while d itself was
# skipped or matched as that growth requires, at most one per level, and that is reset by any use -- so d must own an edge
# that jumps out of its run and (for the counter to grow on the edge as d's first fwd edge) no edge to anything nearer.
# Sites that sit side by side always get an edge when they first meet, so the nearer edge has to die by distance first:
# two levels at 0.2 with its end skipped, then a level that visits the end and not the start.
_a, _d, _b, _m1, _f2, _m2 = range(6)
_B, _D, _B2, _Q = [_a, _b, _m1, _f2, _m2], [_a, _d, _m2], [_a, _b, _m1, _m2], [_a, _m1, _m2]
# L1 puts d in front of b (plain edge d -> b), L2-L4 kill that edge, L5/L6 add m1 -> m2 and a -> m1, then the same leaf
# level after level: d's only fwd edge d -> m2 counts up with the rest.  L11: run {f2} finds d -> m2 as the last over-limit
# edge of m2's list, which starts before the run: nothing goes.  L12: run {d, b} goes, and with it d -> m2 -- so run {f2}
# now finds f2 -> m2 and goes too, which it would not against the undeleted lists.  L13 builds above the non_real sites.
COUPLED_MATCHED_LEAVES = [_B, _D, _D, _D, _B, _B2] + [_Q] * 8
COUPLED_MATCHED_BRANCH = [0.03, 0.2, 0.2, 0.15, 0.03, 0.03] + [0.03] * 7

_A, _o, _p, _dd, _n1, _g, _h2, _n2, _Z = range(9)
_K = [_A, _o, _p, _dd, _h2, _n2, _Z]
# the other way round: run {h2}'s own largest-start edge d -> h2 is over the limit, and against the undeleted lists the run
# would go; run {d} goes first, the edge with it, h2 has no bwd edge left and stays.
COUPLED_OWN_LEAVES = ([_K, [_A, _o, _dd, _g, _n2, _Z], _K, _K, [_A, _o, _p, _dd, _g, _n2, _Z], [_A, _o, _dd, _n1, _g, _n2, _Z],
                       [_A, _o, _p, _n1, _g, _n2, _Z], _K, [_A, _dd, _Z]] + [[_A, _dd, _n2, _Z]] * 5 + [[_A, _p, _n1, _n2, _Z]] * 2)
COUPLED_OWN_BRANCH = [0.03, 0.2, 0.2, 0.2] + [0.03] * 11
COUPLED_OWN_AVOID = dict([(k, {_p, _n1, _h2}) for k in range(8, 14)] + [(14, {_dd, _h2}), (15, {_dd, _h2})])

# Three runs, each deciding the next: the first chain twice over.  d's only fwd edge d -> n1 is the last over-limit edge of
# n1's list and e's only fwd edge e -> n3 that of n3's.  Level 14: run {d, b} goes; so run {e, c} finds c -> n1 and goes,
# which it would not have; so run {h} finds h -> n3 and goes, which it would not have either -- and not even against lists
# that have lost the first run alone.  A builder that evaluates the runs side by side needs three rounds that change
# something.  (Levels 3-6: both plain edges d -> b and e -> c die by distance, each while the site it starts from has been
# skipped twice at 0.2 and the path then takes that site's other edges.)
_ta, _td, _tb, _tm, _te, _tc, _tn1, _th, _tn3 = range(9)
_TB, _TD1, _TD2 = [_ta, _tb, _tm, _tc, _tn1, _th, _tn3], [_ta, _td, _tn1, _th, _tn3], [_ta, _tb, _tm, _te, _tn3]
_TQ = [_ta, _tm, _tn1, _tn3]
THREE_RUNS_LEAVES = [_TB, _TD1, _TD2, _TB, _TB, _TD1, _TD2, [_ta, _tb, _tm, _tn1, _tn3]] + [_TQ] * 7
THREE_RUNS_BRANCH = [0.03, 0.03, 0.2, 0.2, 0.08, 0.05] + [0.03] * 8


def _by_order(kinds, order):
    return [kinds[k] for k in order]


def _walk(n, length, branch, indel_start, mean_len, seed):
    from pagan2_msa_amd import synth
    return synth.evolve_caterpillar(n, length, branch=branch, indel_start=indel_start, mean_len=mean_len, seed=seed)[1]


SCENARIOS = [
    Scenario("coupled_matched_site_edge", "planted", COUPLED_MATCHED_LEAVES, COUPLED_MATCHED_BRANCH, y_first=True,
             rules=("coupling_matched_site_edge_lost", "pass2_edge_starts_before_run", "pass2_delete_whole_run",
                    "pass2_matched_without_over_limit_edge", "pass2_no_bwd_edge", "drop_distance", "plain_x_after_y")),
    Scenario("coupled_own_first_edge", "planted", COUPLED_OWN_LEAVES, COUPLED_OWN_BRANCH, y_first={1}, avoid=COUPLED_OWN_AVOID,
             rules=("coupling_own_first_edge_lost", "pass2_delete_whole_run", "pass2_no_bwd_edge", "pass1_bwd_refused",
                    "pass1_fwd_refused", "history_between_used_sites_unused")),
    Scenario("three_runs_in_a_chain", "planted", THREE_RUNS_LEAVES, THREE_RUNS_BRANCH, y_first=True,
             rules=("coupling_matched_site_edge_lost", "pass2_edge_starts_before_run", "pass2_delete_whole_run", "drop_distance")),
    Scenario("run_before_the_stop_site", "planted", [[0, 1]] + [[0]] * 8, 0.03, flags=2,
             rules=("pass2_over_limit_then_stop_site", "pass2_at_or_below_limit", "pass1_bwd_increment", "pass1_fwd_increment")),
    Scenario("prefix_of_a_run", "planted", _by_order([[0, 1, 2, 3, 4, 5], [1, 2, 4, 5], [0, 2, 5]], [0, 0] + [1] * 7 + [0] + [1] * 6 + [2, 1]), 0.06,
             rules=("pass2_delete_prefix_of_run", "pass2_over_limit_then_gapped", "pass2_delete_whole_run")),
    Scenario("stop_shortening_lands_beside_others", "planted",
             _by_order([[0, 1, 2, 3, 4, 5, 8], [1, 3, 7], [0, 2, 7, 8, 9], [0, 2, 3, 5, 6, 8]], [0, 1, 2, 3, 3, 0, 1]),
             [(0.03, 0.1), (0.03, 0.3), (0.2, 0.06), (0.03, 0.2), (0.2, 0.06), (0.1, 0.03)], y_first=True,
             rules=("stop_shorten_new", "stop_shorten_new_beside_others", "stop_shorten_dup", "start_shorten")),
    Scenario("branch_count_limit", "planted",
             _by_order([list(range(11)), [2, 3, 5, 6, 7, 8, 9, 10], [0, 2, 3, 5, 6, 9, 10]], [0] + [1] * 4 + [2] * 5 + [0] * 3),
             [(0.03, 0.06)] * 12, rules=("drop_count", "history_between_skipped_sites_unused")),
    Scenario("used_edge_between_unequal_sites", "planted", _by_order([[0, 1, 2, 3, 4, 5, 6], [2, 3, 6], [3]], [0, 1, 1, 1, 2]),
             [(0.2, 0.06), (0.1, 0.1), (0.3, 0.06), (0.2, 0.3)], y_first=True,
             rules=("history_ends_differ_used", "history_ends_differ_unused", "drop_distance")),
    Scenario("flipped_sides", "planted", COUPLED_MATCHED_LEAVES, COUPLED_MATCHED_BRANCH, y_first=True, flip=range(1, 13),
             rules=("coupling_matched_site_edge_lost", "pass2_edge_starts_before_run")),
    # pinned seeds of small random caterpillars (tools/search_parent_rules.py --mode walks), branches as evolved
    Scenario("walk_244406", "dp", _walk(20, 30, 0.3, 0.04, 6.0, 244406), 0.3,
             rules=("drop_distance", "drop_count", "history_ends_differ_used", "stop_shorten_dup", "dup_reset", "history_fresh_used")),
    Scenario("walk_964780", "dp", _walk(20, 30, 0.03, 0.02, 6.0, 964780), 0.03,
             rules=("pass2_delete_prefix_of_run", "pass2_delete_whole_run", "child_weight_not_one")),
    Scenario("walk_reads_settings", "dp", _walk(8, 40, 0.05, 0.04, 3.0, 5), 0.05, flags=1, leaf_flags=1,
             rules=("child_weight_not_one", "plain_y_after_x", "plain_x_after_y")),
    # the smallest builds: one column of each state, and none
    Scenario("one_matched", "planted", [[0], [0]], 0.05, rules=()),
    Scenario("one_xgapped", "planted", [[0], []], 0.05, rules=("start_shorten",)),
    Scenario("one_ygapped", "planted", [[], [0]], 0.05, rules=("start_shorten",)),
    Scenario("one_xskipped", "planted", [[0], [], []], 0.05, flags=2, rules=("pass2_at_or_below_limit",)),
    Scenario("one_yskipped", "planted", [[0], [], []], 0.05, flags=2, flip={1}, rules=("pass2_at_or_below_limit",)),
    Scenario("no_column", "planted", [[], []], 0.05, rules=()),
]

# Rules no scenario reaches, with the reason (tests assert nothing about them)
UNREACHABLE = {}

# ---- sizes: the coupled_matched_site_edge chain side by side, k times, then plain matched sites ----
TILE_SITES, TILE_RUNS, TILE_DELETED, DELETING_LEVEL = 6, 2, 3, 12


def size_scenario(n):
    """the chain tiled so that the deleting build (level 12) has n parent sites, start and stop included"""
    k, pad = divmod(n - 2, TILE_SITES)
    return Scenario("tiled_%d_sites" % n, "planted", tiled(COUPLED_MATCHED_LEAVES, k, pad), COUPLED_MATCHED_BRANCH, y_first=True,
                    python=False, rules=("coupling_matched_site_edge_lost", "pass2_delete_whole_run"),
                    expect={"n": n, "runs": TILE_RUNS * k, "deleted": TILE_DELETED * k, "tiles": k})


SIZES = [size_scenario(n) for n in (1023, 1024, 1025, 2047, 2049, 3 * 1024 + 1, 2 + TILE_SITES * 600)]   # the last: 1200 runs
BY_NAME = {s.name: s for s in SCENARIOS + SIZES}


def host_chain(scn, seqs, levels, host, build):
    """The product's graphs up a realised scenario: build(left HGraph, right HGraph, level, k) -> the parent HGraph of
    level k, which is the child of level k + 1 (the leaves come from the product's leaf builder).  Yields (k, level, parent)."""
    leaf_alpha = host.alphabets(1)[0]
    prev = None
    for k, lv in enumerate(levels):
        def child(leaf, prev=prev):
            return prev if leaf is None else host.HGraph.leaf(seqs[leaf], leaf_alpha, flags=scn.leaf_flags)
        prev = build(child(lv.left_leaf), child(lv.right_leaf), lv, k)
        yield k, lv, prev
