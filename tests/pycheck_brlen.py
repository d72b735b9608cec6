"""A second, independent reading of "branch lengths by maximum likelihood" (include/pagan_host.h) in plain Python, on top of
tests/pycheck_anc.py and like it in `decimal` at 50 digits.  From the library it takes P(t), D_1(t), D_2(t) and pi (host.anc_pmatrix,
host.anc_pmatrix_deriv: host only) and nothing else: the partials, the outside vectors, f_r, the informative columns, g1, g2,
the step rule and the whole fit are restated here from the header's text.  Nothing is rescaled: a Decimal has the range.

evaluate() also returns, per branch, what a bound on the device's rounding error needs: the sums of absolute values the
derivatives are made of, and the number of roundings on the way (tolerances())."""
import functools
from decimal import Decimal

import numpy as np

from pagan2_msa_amd import host

import pycheck_anc as A

D0, D1 = A.D0, A.D1
U = 2.0 ** -53
T_MIN, T_MAX, TOL, MAX_ROUNDS = 1e-6, 10.0, 1e-6, 32


def _dec(M):
    return np.array([[Decimal(float(x)) for x in r] for r in M], dtype=object)


def _model(branch, data_type, base_freq):
    """({length: (P, D_1, D_2 as object arrays of Decimals, |D_1|, |D_2| as doubles)}, pi as Decimals)."""
    mats, pi = {}, None
    for t in set(float(b) for b in branch[:-1]):
        P, p = host.anc_pmatrix(data_type, t, base_freq)
        d1, d2 = _dec(host.anc_pmatrix_deriv(data_type, t, 1, base_freq)), _dec(host.anc_pmatrix_deriv(data_type, t, 2, base_freq))
        mats[t] = (_dec(P), d1, d2, np.abs(d1.astype(float)), np.abs(d2.astype(float)))
        pi = [Decimal(float(x)) for x in p]
    return mats, pi


def evaluate(left, right, branch, rows, data_type, base_freq=None, derivs=True):
    """The header's definitions at these lengths.  Returns a dict: lik [L], loglik (their logarithms' sum; -Infinity with an
    impossible column), has_data; with derivs also g1, g2 [2 n - 1] Decimals (the root's 0), informative [2 n - 1] ints,
    abs1, abs2 [2 n - 1] (the sums over the informative columns of A1 and of A2 + A1^2, see tolerances()) and rounds [2 n - 1]
    (the roundings behind one f_r of that branch)."""
    n, S = len(rows), A.STATES[data_type]
    mats, pi = _model(branch, data_type, base_freq)
    sets = [A.leaf_sets(r, data_type) for r in rows]
    L = len(sets[0])
    has = A._has_data(left, right, sets)
    root = 2 * n - 2

    def mat(v):
        return mats[float(branch[v])]

    def leaf_product(M, k):
        """M times the indicator of leaf k's state sets, column by column (all ones for missing data)."""
        out = np.full((S, L), D0, dtype=object)
        for col, s in enumerate(sets[k]):
            for t in (s if s is not None else range(S)):
                out[:, col] = out[:, col] + M[:, t]
        return out

    part = {}

    def times(M, v):
        return leaf_product(M, v) if v < n else M.dot(part[v])

    @functools.lru_cache(maxsize=None)
    def message(child):
        m = times(mat(child)[0], child)
        for col in range(L):
            if not has[child, col]:
                m[:, col] = D1
        return m

    for k in range(n - 1):
        part[n + k] = message(left[k]) * message(right[k])
    lik = []
    for col in range(L):
        total = D0
        for s in range(S):
            total += pi[s] * part[root][s, col]
        lik.append(total if has[root, col] else D1)
    loglik = D0
    for x in lik:
        loglik += x.ln() if x > 0 else Decimal("-Infinity")
    out = {"lik": lik, "loglik": loglik, "has_data": has}
    if not derivs:
        return out
    # roundings: kL of a partial's entry, kO of an outside vector's, kW of W's, all relative (every term is non-negative)
    kL = [0] * (2 * n - 1)
    for k in range(n - 1):
        kL[n + k] = kL[left[k]] + kL[right[k]] + 2 * S + 1
    kO, rounds = {root: 0}, [0] * (2 * n - 1)
    outs = {root: np.array([[pi[s]] * L for s in range(S)], dtype=object)}
    out_has = {root: np.zeros(L, bool)}
    g1, g2 = [D0] * (2 * n - 1), [D0] * (2 * n - 1)
    abs1, abs2, informative = [D0] * (2 * n - 1), [D0] * (2 * n - 1), [0] * (2 * n - 1)
    for k in range(n - 2, -1, -1):
        v = n + k
        for c, b in ((left[k], right[k]), (right[k], left[k])):
            W = outs[v] * message(b)
            kW = kO[v] + S + kL[b] + 1
            out_has[c] = out_has[v] | (has[b] != 0)
            _, d1, d2, a1, a2 = mat(c)
            f = [(W * times(M, c)).sum(axis=0) for M in (mat(c)[0], d1, d2)]
            # A_r = F_r^abs / f_0 only scales a tolerance: in doubles, every column scaled by its largest W and largest L_c first
            Lc = leaf_product(np.eye(S, dtype=object) * D1, c) if c < n else part[c]
            wtop, ltop = W.max(axis=0), Lc.max(axis=0)
            Wf = np.array([[float(W[s, col] / wtop[col]) if wtop[col] > 0 else 0.0 for col in range(L)] for s in range(S)])
            Lf = np.array([[float(Lc[s, col] / ltop[col]) if ltop[col] > 0 else 0.0 for col in range(L)] for s in range(S)])
            f0f = (Wf * (mat(c)[0].astype(float) @ Lf)).sum(axis=0)
            fa = [(Wf * (M @ Lf)).sum(axis=0) for M in (a1, a2)]
            rounds[c] = kW + kL[c] + 2 * S + 1
            for col in range(L):
                if not (has[c, col] and out_has[c][col] and f[0][col] > 0):
                    continue
                informative[c] += 1
                q = f[1][col] / f[0][col]
                g1[c] += q
                g2[c] += f[2][col] / f[0][col] - q * q
                A1, A2 = Decimal(fa[0][col] / f0f[col]), Decimal(fa[1][col] / f0f[col])
                abs1[c] += A1
                abs2[c] += A2 + A1 * A1
            if c >= n:
                outs[c] = mat(c)[0].T.dot(W)
                kO[c] = kW + S
    out.update(g1=g1, g2=g2, informative=informative, abs1=abs1, abs2=abs2, rounds=rounds)
    return out


def tolerances(reading, columns):
    """(tol_g1 [2 n - 1], tol_g2 [2 n - 1]) for the device's fp64 sums against the reading, by counting roundings (u = 2^-53).
    The device's f_r of a branch is a sum of products of W (K_W relative roundings, all terms non-negative), D_r (the same doubles
    on both sides) and L_c (K_L): with K = rounds[c] its error is at most K u F_r^abs, F_r^abs the same sum over |D_r|; f_0 has no
    negative term, so F_0^abs = f_0.  With A_r = F_r^abs / f_0 >= |f_r / f_0|:
      f_1 / f_0                 errs by at most (2 K + 1) u A_1          (numerator, denominator, the division)
      f_2 / f_0 - (f_1/f_0)^2   by (2 K + 1) u A_2 + (4 K + 3) u A_1^2 + u (A_2 + A_1^2) <= (4 K + 4) u (A_2 + A_1^2)
    and the column sum (six steps of the tree, then a block a step) adds (6 + blocks) u times the sum of the absolute values.
    Everything is first order in u; the factor 2 in front pays for the higher orders (K u < 1e-10 in every case here)."""
    blocks = (columns + 63) // 64
    t1, t2 = [], []
    for K, a1, a2 in zip(reading["rounds"], reading["abs1"], reading["abs2"]):
        t1.append(2 * (2 * K + 1 + 6 + blocks) * U * float(a1))
        t2.append(2 * (4 * K + 4 + 6 + blocks) * U * float(a2))
    return t1, t2


# ---- the step rule and the fit ------------------------------------------------------------------------------------------------

def step(t, g1, g2, t_min=T_MIN, t_max=T_MAX):
    """The header's step rule on Python floats."""
    if not all(np.isfinite(x) for x in (t, g1, g2)):
        return t
    if g1 == 0 and g2 == 0:
        return t
    s = t - g1 / g2 if g2 < 0 else (2 * t if g1 > 0 else t / 2)
    s = min(max(s, t / 4), 4 * t)
    return min(max(s, t_min), t_max)


def parameters(left, right, branch):
    """The fit's parameters: every branch but the root's two by node id, and ("tau", t_l + t_r) in their place."""
    n = len(left) + 1
    rl, rr = left[-1], right[-1]
    return [c for c in range(2 * n - 2) if c not in (rl, rr)], rl, rr


def full_step(left, right, branch, g1, g2, t_min=T_MIN, t_max=T_MAX):
    """({branch id: stepped length}, tau, stepped tau, the largest |t' - t| / max(t, t_min)) with g1, g2 as floats."""
    free, rl, rr = parameters(left, right, branch)
    stepped = {c: step(branch[c], float(g1[c]), float(g2[c]), t_min, t_max) for c in free}
    tau = branch[rl] + branch[rr]
    tau_step = step(tau, float(g1[rl]), float(g2[rl]), t_min, t_max)
    moved = max([abs(stepped[c] - branch[c]) / max(branch[c], t_min) for c in free] + [abs(tau_step - tau) / max(tau, t_min)])
    return stepped, tau, tau_step, moved


def proportion(left, right, branch_in):
    """p: the root's left branch over the sum of its two in branch_in, 1/2 where both are 0."""
    rl, rr = left[-1], right[-1]
    tau_in = branch_in[rl] + branch_in[rr]
    return branch_in[rl] / tau_in if tau_in > 0 else 0.5


def start(left, right, branch_in, t_min=T_MIN, t_max=T_MAX):
    """The lengths the fit starts from, on Python floats: every free branch kept within [t_min, t_max]; tau likewise, and where that
    moved it, split as t_l = tau p, t_r = tau - t_l; the root's own entry 0."""
    free, rl, rr = parameters(left, right, branch_in)
    t = [float(x) for x in branch_in]
    t[-1] = 0.0
    for c in free:
        t[c] = min(max(t[c], t_min), t_max)
    tau_in = branch_in[rl] + branch_in[rr]
    tau = min(max(tau_in, t_min), t_max)
    if tau != tau_in:
        t[rl] = tau * proportion(left, right, branch_in)
        t[rr] = tau - t[rl]
    return t


def candidate(left, right, t, stepped, tau, tau_step, alpha, p, t_min=T_MIN, t_max=T_MAX):
    """The header's candidate t + alpha (t' - t) on Python floats (alpha = 1: t' itself), every parameter kept within its bounds,
    tau split by p."""
    free, rl, rr = parameters(left, right, t)

    def bounded(x):
        return min(max(x, t_min), t_max)
    cand = list(t)
    for c in free:
        cand[c] = stepped[c] if alpha == 1.0 else bounded(t[c] + alpha * (stepped[c] - t[c]))
    new_tau = tau_step if alpha == 1.0 else bounded(tau + alpha * (tau_step - tau))
    cand[rl] = new_tau * p
    cand[rr] = new_tau - cand[rl]
    return cand


def fit(left, right, branch_in, rows, data_type, base_freq=None, t_min=T_MIN, t_max=T_MAX, tol=TOL, max_rounds=MAX_ROUNDS):
    """The header's fit with the reading's own g1, g2 and loglik.  Returns dict(branch, loglik (the accepted ones), status, rounds,
    decisions): decisions[r] lists round r's candidates in the order they were tried as (alpha, the candidate's log likelihood
    minus the accepted one it was held against); the last of a round is the accepted one unless the round stalled, and a round
    that converged has none."""
    p = proportion(left, right, branch_in)
    t = start(left, right, branch_in, t_min, t_max)
    ll = evaluate(left, right, t, rows, data_type, base_freq, derivs=False)["loglik"]
    hist, status, rounds, decisions = [ll], "max_rounds", 0, []
    for _ in range(max_rounds):
        r = evaluate(left, right, t, rows, data_type, base_freq)
        rounds += 1
        stepped, tau, tau_step, moved = full_step(left, right, t, r["g1"], r["g2"], t_min, t_max)
        decisions.append([])
        if moved <= tol:
            status = "converged"
            break
        alpha, accepted = 1.0, False
        for _ in range(6):
            cand = candidate(left, right, t, stepped, tau, tau_step, alpha, p, t_min, t_max)
            llc = evaluate(left, right, cand, rows, data_type, base_freq, derivs=False)["loglik"]
            decisions[-1].append((alpha, float(llc - ll)))
            if not llc < ll:
                accepted = True
                break
            alpha *= 0.5
        if not accepted:
            status = "stalled"
            break
        t, ll = cand, llc
        hist.append(ll)
    return {"branch": t, "loglik": hist, "status": status, "rounds": rounds, "decisions": decisions}


# ---- rows simulated on a tree, and the cases the CPU and the GPU tests share ---------------------------------------------------------

def simulate(left, right, branch, L, data_type, base_freq, seed):
    """n rows of L columns evolved down the tree under the library's own P(t): the root's state from pi, a child's from its
    parent's row of P."""
    n, rng = len(left) + 1, np.random.default_rng(seed)
    S = A.STATES[data_type]
    state = {}
    pi = host.anc_pmatrix(data_type, 0.1, base_freq)[1]
    state[2 * n - 2] = rng.choice(S, size=L, p=pi / pi.sum())
    for k in range(n - 2, -1, -1):
        for c in (left[k], right[k]):
            P = host.anc_pmatrix(data_type, branch[c], base_freq)[0]
            P = P / P.sum(axis=1, keepdims=True)
            state[c] = np.array([rng.choice(S, p=P[s]) for s in state[n + k]])
    return ["".join(A.state_text(int(s), data_type) for s in state[k]) for k in range(n)]


def _named(name):
    kind, _, arg = name.partition(":")
    bf, t = A.BASE_FREQ, 1
    if kind == "pair":                                   # n = 2: the root pair only
        L = int(arg)
        left, right, branch = [0], [1], [0.07, 0.19, 0.0]
        rows = A.random_rows(2, L, 1, 700 + L, share=0.2)
    elif kind == "three":                                # a leaf child with an internal sibling and the other way round
        L = int(arg)
        left, right, branch = A.random_tree(3, np.random.default_rng(710 + L))
        rows = A.random_rows(3, L, 1, 720 + L, share=0.2)
    elif kind == "eight":                                # random trees: internal children with leaf and with internal siblings
        L = int(arg)
        left, right, branch = A.random_tree(8, np.random.default_rng(730 + L))
        rows = A.random_rows(8, L, 1, 740 + L, share=0.2)
    elif kind == "codon" and arg == "tree":              # the four-wave kernel on a random tree: leaves beside internal siblings
        left, right, branch = A.random_tree(5, np.random.default_rng(752))
        rows, t, bf = A.random_rows(5, 65, 3, 753), 3, None
    elif kind == "onesided" and arg:                     # the construction below on the four-wave kernels, 20 columns
        t, bf = {"protein": 2, "codon": 3}[arg], None
        left, right, branch = A.balanced4([0.05, 0.12, 0.3, 0.08, 0.11, 0.21])
        gap = "---" if t == 3 else "-"
        width = len(gap)
        text = A.random_rows(4, 20, t, 754 + t, share=0.1)
        rows = [[r[i:i + width] for i in range(0, len(r), width)] for r in text]
        for col in range(0, 20, 5):
            rows[0][col] = rows[1][col] = gap            # nothing under node 4
        for col in range(3, 20, 7):
            rows[0][col] = rows[1][col] = rows[2][col] = gap         # a single leaf holds data
        for col in (10, 11):
            for r in range(4):
                rows[r][col] = gap
        rows = ["".join(r) for r in rows]
    elif kind == "sim" and arg in ("protein", "codon"):  # the fit on the four-wave kernels; a gap in every ninth column
        t, bf = {"protein": 2, "codon": 3}[arg], None
        n = {2: 4, 3: 3}[t]
        tree_seed, rows_seed = {2: (802, 812), 3: (833, 843)}[t]     # (803, 813 for codons converge as well, in 16 rounds)
        left, right, branch = A.random_tree(n, np.random.default_rng(tree_seed), lo=0.03, hi=0.4)
        width = 3 if t == 3 else 1
        rows = [list(r) for r in simulate(left, right, branch, 65, t, None, rows_seed)]
        for col in range(0, 65, 9):
            rows[(col // 9) % n][col * width:(col + 1) * width] = "-" * width
        rows = ["".join(r) for r in rows]
    elif kind == "onesided":                             # columns with data on one side of the root only, and all-missing columns
        left, right, branch = A.balanced4([0.05, 0.12, 0.3, 0.08, 0.11, 0.21])
        rows = [list(r) for r in A.random_rows(4, 70, 1, 750, share=0.1)]
        for col in range(0, 70, 5):
            rows[0][col] = rows[1][col] = "-"            # nothing under node 4
        for col in range(3, 70, 7):
            rows[0][col] = rows[1][col] = rows[2][col] = "-"         # a single leaf holds data
        for col in (10, 11):
            for r in range(4):
                rows[r][col] = "-"
        rows = ["".join(r) for r in rows]
    elif kind == "lengths":                              # zero-length and very long branches in one tree
        left, right, branch = A.balanced4([0.0, 0.3, 50.0, 0.07, 0.0, 0.13])
        rows = A.random_rows(4, 70, 1, 760)
    elif kind == "sim":                                  # rows simulated on a known tree: arg = leaves
        n = int(arg)
        left, right, branch = A.random_tree(n, np.random.default_rng(770 + n), lo=0.03, hi=0.4)
        rows = simulate(left, right, branch, 130, 1, bf, 780 + n)
    elif kind == "twins":                                # leaves 0 and 1 are one cherry and hold the same row
        left, right, branch = [0, 2, 4], [1, 3, 5], [0.1, 0.08, 0.15, 0.2, 0.12, 0.09, 0.0]
        rows = simulate(left, right, branch, 65, 1, bf, 790)
        rows[1] = rows[0]
    elif kind == "unrelated" and arg == "protein":       # the same on the four-wave kernels: the reading halves a step in round 9
        t, bf = 2, None
        left, right, branch = A.random_tree(4, np.random.default_rng(799))
        rows = A.random_rows(4, 64, 2, 800, share=0.0)
    elif kind == "unrelated":                            # random rows: no tree behind them
        left, right, branch = A.random_tree(4, np.random.default_rng(795))
        rows = A.random_rows(4, 64, 1, 796, share=0.0)
    else:
        return None
    return {"left": left, "right": right, "branch": branch, "rows": rows, "data_type": t, "base_freq": bf}


@functools.lru_cache(maxsize=None)
def case(name):
    """A named shape with its reading: pycheck_anc.case's dict (its own names as well) with "brlen" = evaluate() at its lengths."""
    c = _named(name)
    if c is None:
        c = {k: v for k, v in A.case(name).items() if k != "reading"}
    c["brlen"] = evaluate(c["left"], c["right"], c["branch"], c["rows"], c["data_type"], c["base_freq"])
    return c


@functools.lru_cache(maxsize=None)
def fitted(name):
    """The reading's fit of a named case."""
    c = case(name)
    return fit(c["left"], c["right"], c["branch"], c["rows"], c["data_type"], c["base_freq"])


def kinds(left, right):
    """The kinds of branch in a tree: {(the child is internal, its sibling is internal, its parent is the root)}."""
    n = len(left) + 1
    out = set()
    for k in range(n - 1):
        for a, b in ((left[k], right[k]), (right[k], left[k])):
            out.add((a >= n, b >= n, k == n - 2))
    return out


EDGE_COLUMNS = (1, 63, 64, 65, 130)
DERIV_CASES = (["pair:%d" % L for L in EDGE_COLUMNS] + ["three:%d" % L for L in EDGE_COLUMNS] + ["eight:%d" % L for L in EDGE_COLUMNS]
               + ["onesided", "lengths", "impossible", "zero", "long", "balanced:protein", "balanced:codon", "deep:dna"]
               # the four-wave pa_branch on every kind of branch, on the informative rule, zero lengths and impossible columns
               + ["protein", "codon", "chunks:protein", "zero:protein", "zero:codon", "impossible:protein", "impossible:codon",
                  "codon:tree", "onesided:protein", "onesided:codon"])
FOUR_WAVE_CASES = {2: ["balanced:protein", "protein", "chunks:protein", "zero:protein", "impossible:protein", "onesided:protein"],
                   3: ["balanced:codon", "codon", "zero:codon", "impossible:codon", "codon:tree", "onesided:codon"]}
# The fit is a Jacobi iteration: on a tree with a short internal branch between long ones the steps of neighbouring branches
# overshoot in turn and the error shrinks by about 0.9 a round, so that 32 rounds are too few from n = 6 on ("Branch
# lengths by maximum likelihood").  The DNA cases fitted here converge in 16 to 19 rounds; sim:protein (S = 20, 4 leaves) in 13 and
# sim:codon (S = 61, 3 leaves) in 10 of the reading's rounds, no step halved (2 s and 7 s of the reading on one core).
SIM_CASES = ["sim:3", "sim:5", "sim:protein", "sim:codon"]
FIT_CASES = SIM_CASES + ["pair:65", "pair:130", "twins"]
# Rows with no tree behind them: the surface is flat and far from concave at lengths above 1, branches run into t_max, and the
# iteration need not settle in 32 rounds.  What holds for them is the contract alone: bounds kept, log likelihoods never falling.
UNRELATED_CASES = ["unrelated", "three:130"]
# {case: rounds}: the fits followed round by round (tests/test_brlen_gpu.py); within these rounds the reading halves steps and
# decides every candidate by a margin of 1e-6 or more (tests/test_brlen_cpu.py)
LINE_SEARCH_CASES = {"unrelated": 16, "unrelated:protein": 12}
