"""A second, independent reading of "tree search by nearest-neighbour interchange" (include/pagan_host.h) in plain Python, on top
of tests/pycheck_anc.py and like it in `decimal` at 50 digits.  From the library it takes P(t) and pi (host.anc_pmatrix: host only)
and nothing else.
  (i)   gains_by_formula: the header's f_k from partials, messages and outside vectors restated here (pycheck_anc.pruning keeps
        them to itself), nothing rescaled: a Decimal has the range.
  (ii)  gain_by_pruning: the log likelihood of the rearranged tree by full pruning (pycheck_brlen.evaluate) minus that of the tree
        as it is.  It takes nothing from the formula: the tree is rearranged by apply() and pruned from its leaves.
  (iii) kinds, candidates, apply, select and search: the host-only parts, which have no arithmetic to round."""
import functools
from decimal import Decimal

import numpy as np

from pagan2_msa_amd import host

import pycheck_anc as A
import pycheck_brlen as B

D0, D1 = A.D0, A.D1
U = 2.0 ** -53


# ---- (iii) the tree's side --------------------------------------------------------------------------------------------------

def parents(left, right):
    n = len(left) + 1
    parent = [-1] * (2 * n - 1)
    for k in range(n - 1):
        parent[left[k]] = parent[right[k]] = n + k
    return parent


def kinds(left, right):
    """(kind [n - 1]: 0 no candidate, 1 ordinary, 2 the root edge; parent [2 n - 1])."""
    n = len(left) + 1
    root, parent = 2 * n - 2, parents(left, right)
    kind = [1 if (n + k != root and parent[n + k] != root) else 0 for k in range(n - 1)]
    if n >= 3 and left[-1] >= n and right[-1] >= n:
        kind[left[-1] - n] = 2
    return kind, parent


def candidates(left, right):
    """One dict per candidate in node order: c, kind, a, d, b, and v (ordinary) or e, rr (the root edge)."""
    n = len(left) + 1
    kind, parent = kinds(left, right)
    out = []
    for k in range(n - 1):
        c = n + k
        if kind[k] == 1:
            v = parent[c]
            b = right[v - n] if left[v - n] == c else left[v - n]
            out.append({"c": c, "kind": 1, "a": left[k], "d": right[k], "b": b, "v": v})
        elif kind[k] == 2:
            rr = right[-1]
            out.append({"c": c, "kind": 2, "a": left[k], "d": right[k], "e": left[rr - n], "b": right[rr - n], "rr": rr})
    return out


def swap_in_place(left, right, node, k):
    """The swap on ids that stay: k = 1 puts b into c's left slot and a where b was; k = 2 the same with the right slot and d."""
    n = len(left) + 1
    c = next(x for x in candidates(left, right) if x["c"] == node)
    mine = left if k == 1 else right
    if c["kind"] == 2:
        holder, slot = right, c["rr"] - n
    else:
        v = c["v"]
        holder, slot = (right, v - n) if left[v - n] == node else (left, v - n)
    mine[node - n], holder[slot] = holder[slot], mine[node - n]


def renumber(left, right, branch):
    """The internal nodes in post-order (left subtree, right subtree, the node).  Returns (left, right, branch, perm)."""
    n = len(left) + 1
    perm = list(range(n)) + [-1] * (n - 1)
    order = []
    stack = [(2 * n - 2, 0)]
    while stack:
        v, stage = stack.pop()
        if v < n:
            continue
        if stage == 0:
            stack += [(v, 1), (left[v - n], 0)]
        elif stage == 1:
            stack += [(v, 2), (right[v - n], 0)]
        else:
            perm[v] = n + len(order)
            order.append(v)
    new_left = [perm[left[v - n]] for v in order]
    new_right = [perm[right[v - n]] for v in order]
    new_branch = [0.0] * (2 * n - 1)
    for v in range(2 * n - 1):
        new_branch[perm[v]] = float(branch[v])
    new_branch[-1] = 0.0
    return new_left, new_right, new_branch, perm


def apply_many(left, right, branch, swaps):
    """Swaps whose edges share no node, applied on the same ids in the order given, renumbered once."""
    l, r = list(left), list(right)
    for node, k in swaps:
        swap_in_place(l, r, node, k)
    return renumber(l, r, branch)


def apply(left, right, branch, node, k):
    return apply_many(left, right, branch, [(node, k)])


def clades(left, right):
    """The leaf sets under the internal nodes."""
    n = len(left) + 1
    below = [frozenset([k]) for k in range(n)]
    for k in range(n - 1):
        below.append(below[left[k]] | below[right[k]])
    return set(below[n:])


def select(left, right, gain, degenerate, min_gain=1e-3):
    """[(node, k)] in the order taken."""
    n = len(left) + 1
    picks = []
    for c in candidates(left, right):
        q = c["c"] - n
        k = 2 if gain[q][1] > gain[q][0] else 1
        if degenerate[q][k - 1] == 0 and gain[q][k - 1] > min_gain:
            ends = {c["c"], c["v"]} if c["kind"] == 1 else {c["c"], c["rr"], 2 * n - 2}
            picks.append((-float(gain[q][k - 1]), c["c"], k, ends))
    picks.sort(key=lambda p: (p[0], p[1]))
    taken, out = set(), []
    for _, c, k, ends in picks:
        if taken & ends:
            continue
        taken |= ends
        out.append((c, k))
    return out


def search(left, right, branch, min_gain, max_rounds, gains, loglik):
    """The header's search with fit_rounds = 0 on the caller's gains(left, right, branch) -> (gain, degenerate) [n - 1][2] and
    loglik(left, right, branch).  Returns dict(left, right, branch, loglik (the accepted ones), status, swaps: (round, node, k,
    joint, gain), trees: the accepted tree of every round)."""
    n = len(left) + 1
    left, right, branch = list(left), list(right), [float(x) for x in branch]
    ll = loglik(left, right, branch)
    hist, swaps, trees, status = [ll], [], [], "max_rounds"
    for rnd in range(max_rounds):
        gain, deg = gains(left, right, branch)
        sel = select(left, right, gain, deg, min_gain)
        if not sel:
            status = "converged"
            break
        cand = apply_many(left, right, branch, sel)[:3]
        llc, joint = loglik(*cand), 1
        if llc < ll and len(sel) > 1:
            sel, joint = sel[:1], 0
            cand = apply_many(left, right, branch, sel)[:3]
            llc = loglik(*cand)
        if llc < ll:
            status = "stalled"
            break
        swaps += [(rnd, c, k, joint, float(gain[c - n][k - 1])) for c, k in sel]
        (left, right, branch), ll = cand, llc
        hist.append(ll)
        trees.append(cand)
    return {"left": left, "right": right, "branch": branch, "loglik": hist, "status": status, "swaps": swaps, "trees": trees}


# ---- (i) the formula at 50 digits -------------------------------------------------------------------------------------------------

def _dec(M):
    return np.array([[Decimal(float(x)) for x in r] for r in M], dtype=object)


def vectors(left, right, branch, rows, data_type, base_freq=None):
    """(message(child) -> [S, L], outs {internal node: O}, pi, has): pruning and the outside pass, nothing rescaled."""
    n, S = len(rows), A.STATES[data_type]
    mats, pi = A._model(branch, data_type, base_freq)
    sets = [A.leaf_sets(r, data_type) for r in rows]
    L = len(sets[0])
    has = A._has_data(left, right, sets)
    part = {}
    for k in range(n):
        v = np.full((S, L), D0, dtype=object)
        for col, s in enumerate(sets[k]):
            for t in (s or ()):
                v[t, col] = D1
        part[k] = v
    memo = {}

    def message(child):
        if child not in memo:
            m = mats[float(branch[child])].dot(part[child])
            for col in range(L):
                if not has[child, col]:
                    m[:, col] = D1
            memo[child] = m
        return memo[child]

    for k in range(n - 1):
        part[n + k] = message(left[k]) * message(right[k])
    root = 2 * n - 2
    outs = {root: np.array([[pi[s]] * L for s in range(S)], dtype=object)}
    for k in range(n - 2, -1, -1):
        for c, b in ((left[k], right[k]), (right[k], left[k])):
            if c >= n:
                outs[c] = mats[float(branch[c])].T.dot(outs[n + k] * message(b))
    return message, outs, pi, has


def gains_by_formula(left, right, branch, rows, data_type, base_freq=None):
    """{c: dict(gain [2] Decimal, degenerate [2] int, ratios [2][L] Decimal (1 where degenerate))} by the header's formula."""
    message, outs, pi, has = vectors(left, right, branch, rows, data_type, base_freq)
    S = A.STATES[data_type]
    L = has.shape[1]
    out = {}
    for c in candidates(left, right):
        ma, md, mb = message(c["a"]), message(c["d"]), message(c["b"])
        if c["kind"] == 2:
            T = np.array([[pi[s]] * L for s in range(S)], dtype=object) * message(c["e"])
            P_mid = _dec(host.anc_pmatrix(data_type, branch[c["c"]] + branch[c["rr"]], base_freq)[0])
        else:
            T = outs[c["v"]]
            P_mid = _dec(host.anc_pmatrix(data_type, branch[c["c"]], base_freq)[0])
        u = (ma * md, mb * md, ma * mb)
        X = (mb, ma, md)
        pair = ((c["a"], c["d"]), (c["b"], c["d"]), (c["a"], c["b"]))
        f = []
        for k in range(3):
            y = P_mid.dot(u[k])
            for col in range(L):
                if not (has[pair[k][0], col] or has[pair[k][1], col]):
                    y[:, col] = D1                       # a pair without data is a node without data: the exact 1
            f.append(((T * X[k]) * y).sum(axis=0))
        gain, deg, ratios = [D0, D0], [0, 0], [[], []]
        for k in (1, 2):
            for col in range(L):
                if f[0][col] > 0 and f[k][col] > 0:
                    r = f[k][col] / f[0][col]
                    gain[k - 1] += r.ln()
                else:
                    r = D1
                    deg[k - 1] += 1
                ratios[k - 1].append(r)
        out[c["c"]] = {"gain": gain, "degenerate": deg, "ratios": ratios}
    return out


# ---- (ii) full pruning of the rearranged tree ----------------------------------------------------------------------------------------

def loglik_by_pruning(left, right, branch, rows, data_type, base_freq=None):
    return B.evaluate(left, right, branch, rows, data_type, base_freq, derivs=False)["loglik"]


def gain_by_pruning(left, right, branch, rows, data_type, base_freq, node, k, start=None):
    """The rearranged tree's log likelihood minus the tree's own, both by full pruning (Decimals; -Infinity with an impossible
    column)."""
    if start is None:
        start = loglik_by_pruning(left, right, branch, rows, data_type, base_freq)
    l, r, b, _ = apply(left, right, branch, node, k)
    return loglik_by_pruning(l, r, b, rows, data_type, base_freq) - start


# ---- the cases the CPU and the GPU tests share ---------------------------------------------------------------------------------

EDGE_COLUMNS = (1, 63, 64, 65, 130)
LENGTHS4 = [0.11, 0.07, 0.23, 0.31, 0.05, 0.17]


@functools.lru_cache(maxsize=None)
def case(name):
    """dict(left, right, branch, rows, data_type, base_freq) of a named shape."""
    kind, _, arg = name.partition(":")
    bf, t = A.BASE_FREQ, 1
    if kind == "cat4":                                   # (((0, 1), 2), 3): one ordinary candidate, node 4
        L = int(arg)
        left, right, _ = A.caterpillar(4, 0.1)
        branch = LENGTHS4 + [0.0]
        rows = A.random_rows(4, L, 1, 900 + L, share=0.1)
    elif kind == "bal4":                                 # ((0, 1), (2, 3)): the root edge only
        L = int(arg)
        left, right, branch = A.balanced4(LENGTHS4)
        rows = A.random_rows(4, L, 1, 910 + L, share=0.1)
    elif kind == "eight":                                # a random tree, a tenth of the cells missing; column 2 holds a single letter
        t = {"dna": 1, "protein": 2, "codon": 3}[arg]
        left, right, branch = A.random_tree(8, np.random.default_rng(920 + t))
        rows = A.random_rows(8, {1: 70, 2: 66, 3: 65}[t], t, 930 + t, share=0.1)
        bf = bf if t == 1 else None
    elif kind == "chunks":                               # 250 columns: one chunk, or four of 64
        left, right, branch = A.random_tree(8, np.random.default_rng(925))
        rows = A.random_rows(8, 250, 1, 935, share=0.1)
    elif kind == "small":                              # the four-wave kernels at sizes the 50-digit reading gets through
        t = {"protein": 2, "codon": 3}[arg]
        left, right, branch = A.random_tree({2: 6, 3: 5}[t], np.random.default_rng(960 + t))
        rows, bf = A.random_rows({2: 6, 3: 5}[t], {2: 12, 3: 4}[t], t, 970 + t, share=0.1), None
    elif kind == "spots":                                # random 7-leaf trees: between them a leaf and an internal node in every position
        left, right, branch = A.random_tree(7, np.random.default_rng(940 + int(arg)))
        rows = A.random_rows(7, 20, 1, 945 + int(arg), share=0.1)
    elif kind == "deep":                                 # the 600-leaf caterpillar: 597 candidates in one block, O far below fp64's range unscaled
        left, right, branch = A.caterpillar(600, 0.2)
        rows = A.random_rows(600, 8, 1, 950, share=0.1)
    elif kind == "impossible":                           # pycheck_anc's impossible columns: leaves 0 and 1 at length 0 with different letters
        c = A.case(name)
        return {k: c[k] for k in ("left", "right", "branch", "rows", "data_type", "base_freq")}
    else:
        raise KeyError(name)
    return {"left": left, "right": right, "branch": branch, "rows": rows, "data_type": t, "base_freq": bf}


SPOT_CASES = ["spots:%d" % s for s in range(4)]
BYTE_CASES = (["cat4:%d" % L for L in EDGE_COLUMNS] + ["bal4:%d" % L for L in EDGE_COLUMNS] + ["eight:dna", "eight:protein", "eight:codon"]
              + ["small:protein", "small:codon"] + SPOT_CASES + ["deep", "impossible", "impossible:protein", "impossible:codon"])
# the cases the 50-digit reading is taken on (eight:protein and eight:codon would take it minutes)
EXACT_CASES = (["cat4:%d" % L for L in (1, 65)] + ["bal4:%d" % L for L in (1, 65)] + ["eight:dna", "small:protein", "small:codon"]
               + SPOT_CASES + ["impossible", "impossible:protein"])


def positions(left, right):
    """{(position, is internal)} over the candidates: which of a, d, b, e is held by a leaf and which by an internal node."""
    n = len(left) + 1
    return {(p, c[p] >= n) for c in candidates(left, right) for p in "adbe" if p in c}


def planted(n, seed, swaps, lo=0.05, hi=0.3):
    """(true tree, start tree): a random n-leaf tree renumbered in post-order, and the same after `swaps` NNIs at ordinary
    candidates drawn with the seed (away from the root: the root edge is never drawn)."""
    rng = np.random.default_rng(seed)
    true = renumber(*A.random_tree(n, rng, lo, hi))[:3]
    left, right, branch = true
    for _ in range(swaps):
        cands = [c for c in candidates(left, right) if c["kind"] == 1]
        c = cands[int(rng.integers(len(cands)))]
        left, right, branch, _ = apply(left, right, branch, c["c"], int(rng.integers(1, 3)))
    return true, (left, right, branch)


# {leaves: (seed, planted swaps)}: the searches tests/test_nni_gpu.py follows round by round; tests/test_nni_cpu.py checks with
# the fp64 reading alone that the start tree differs from the true one and that the search finds it again
SEARCH_CASES = {8: (1009, 2), 12: (1015, 3)}
SEARCH_COLUMNS = 512


@functools.lru_cache(maxsize=None)
def search_case(n):
    """dict(true, start: (left, right, branch); rows) of SEARCH_CASES[n]: rows simulated on the true tree."""
    seed, swaps = SEARCH_CASES[n]
    true, start = planted(n, seed, swaps)
    return {"true": true, "start": start, "rows": B.simulate(*true, SEARCH_COLUMNS, 1, A.BASE_FREQ, seed + 50)}


@functools.lru_cache(maxsize=None)
def fallback_case():
    """7 leaves, 16 columns, min_gain 0: in round 0 the swaps selected lower the log likelihood when applied together, and the
    first alone is accepted.  Found by trying the seeds 2000 .. 2069 (6 to 10 leaves, 16 to 64 columns, three planted swaps) with
    the fp64 reading; 2023 and 2080 are two more."""
    true, start = planted(7, 2069, 3, lo=0.02, hi=0.5)
    return {"true": true, "start": start, "rows": B.simulate(*true, 16, 1, A.BASE_FREQ, 2069 + 50), "min_gain": 0.0}


# ---- bounds ----------------------------------------------------------------------------------------------------------------------

def ck_defect(left, right, branch, data_type, base_freq=None):
    """The Chapman-Kolmogorov defect of anc_pmatrix at the root's two lengths s, t, from the matrices themselves at 50 digits: the
    largest entry of |P(s) P(t) - P(s + t)| relative to P(s + t)'s.  Every f_k is a sum of non-negative terms with P_mid's entries
    as factors, so P(s) P(t) in P(s + t)'s place (what full pruning of the rooted tree multiplies by) moves f_k by at most this share
    of itself."""
    s, t = branch[left[-1]], branch[right[-1]]
    Ps, Pt, Pst = (_dec(host.anc_pmatrix(data_type, x, base_freq)[0]) for x in (s, t, s + t))
    return float((abs(Ps.dot(Pt) - Pst) / Pst).max())


def loglik_tolerance(left, right, S, col_loglik):
    """The bound of a device log likelihood against the exact one: pycheck_anc.tolerance relative on every column's likelihood (so
    absolute on its logarithm), 3 u of each term for the host's log, product and sum in log(col_lik) + col_exp log 2, and
    (L - 1) u of the terms' absolute sum for the running sum over the L columns."""
    L = len(col_loglik)
    return L * A.tolerance(left, right, S) + (3 + L) * U * float(np.abs(col_loglik).sum())


def gain_tolerance(left, right, S, columns, log_abs_sum=0.0):
    """The bound of the fp64 reading's (and so the device's) gain against the 50-digit one, by counting roundings as
    pycheck_anc.tolerance does ("Test bounds").  Every f_k is, like a column's likelihood, a sum of non-negative
    terms over the whole tree -- each leaf's vector, each branch's matrix and pi enter once -- so its relative error is bounded as
    the likelihood's is, by tol = pycheck_anc.tolerance.  Per column: the quotient f_k / f_0 errs relatively by at most 2 tol
    (numerator and denominator) + u (the division); its logarithm by the same to first order.  The product: frexp is exact, each
    of the 6 tree steps and each block's step multiplies two mantissas and rounds once, so a column's factor passes through at
    most 6 + blocks roundings of u.  Summed over the columns; the host's log(M) + E log 2 adds 4 u (|log M| + |E| log 2), which
    log_abs_sum carries."""
    tol = A.tolerance(left, right, S)
    blocks = (columns + 63) // 64
    return columns * (2 * tol + U + (6 + blocks) * U) + 4 * U * log_abs_sum
