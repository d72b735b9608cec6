"""A second, deliberately different reading of the reference's parent-graph builder, in plain Python (test infrastructure).

oracle/oracle_host.cpp (struct Builder) restates Basic_alignment::build_ancestral_sequence -- create_ancestral_sequence,
create_ancestral_edges, transfer_child_edge (both overloads), check_skipped_boundaries, delete_edge_range
(src/main/basic_alignment.cpp:36-653) -- over its own restatement of the Sequence / Site / Edge containers
(src/main/sequence.h:34-130, 216-640, 716-870); the product (pagan2-msa_amd/csrc/host_graph.cpp) is a third text over flat
CSR chains.  This file reads the same source once more, class by class and method by method with the reference's names --
Python objects, edge lists linked through next_*_edge_index with the sites' iteration cursors, numpy.float32 wherever the
reference holds a float -- so that the readings can be compared field by field on real progressive alignments (parity
is unpinned: the reference cannot be built here, and independent readings that agree narrow what that leaves open).

What is NOT read a second time: the children handed to the builder (they are imported from the oracle's dump of its
graphs, leaves included), the alignment path (the oracle's DP), the model's parsimony table.  Branches of the reference
that its defaults switch off are kept as comments: edges_for_skipped_flanked_by_gaps, weight_edges, pair_end_reads,
weighted_branch_skip_penalty (basic_alignment.h:544-571), use-consensus / build-contigs (reads options).
"""
import math

import numpy as np

f32 = np.float32

# sequence.h:226, 229
start_site, real_site, stop_site, break_start_site, break_stop_site, non_real = range(6)
ends_site, terminal, matched, xgapped, ygapped, xskipped, yskipped = range(7)


def logf(w):
    """log of a float, as a float (std::log(float); glibc evaluates it in double and rounds once)"""
    return f32(math.log(float(w))) if float(w) > 0.0 else f32(-np.inf)


class Edge:                                                           # sequence.h:34-130
    def __init__(self, s, e, w=None):
        self.index = -1
        self.start_site_index = s
        self.end_site_index = e
        if w is None:                                                 # Edge(int s, int e)                          :56-59
            self.posterior_weight = f32(1.0)
            self.log_posterior_weight = f32(0)
        else:                                                         # Edge(int s, int e, float w)                 :61-65
            self.posterior_weight = f32(w)
            self.log_posterior_weight = logf(f32(w))
        self.next_fwd_edge_index = -1
        self.next_bwd_edge_index = -1
        self.used_in_alignment = False
        self.branch_count_since_last_used = 0
        self.branch_distance_since_last_used = f32(0)
        self.branch_count_as_skipped_edge = 0

    def copy(self):
        c = Edge(self.start_site_index, self.end_site_index)
        c.__dict__.update(self.__dict__)
        return c

    def set_weight(self, w):                                          # :98
        self.posterior_weight = f32(w)
        self.log_posterior_weight = logf(f32(w))

    def multiply_weight(self, w):                                     # :99 (float parameter)
        self.posterior_weight = f32(self.posterior_weight * f32(w))
        self.log_posterior_weight = logf(self.posterior_weight)

    def __eq__(self, b):                                              # :101-104
        return self.start_site_index == b.start_site_index and self.end_site_index == b.end_site_index

    __hash__ = None


class Site:                                                           # sequence.h:216-640
    def __init__(self, edges, type_=real_site, p_state=terminal):     # :248-251
        self.index = -1
        self.character_state = -1
        self.site_type = type_
        self.path_state = p_state
        self.edges = edges
        self.first_fwd_edge_index = self.current_fwd_edge_index = -1
        self.first_bwd_edge_index = self.current_bwd_edge_index = -1
        self.branch_count_since_last_used = 0
        self.branch_distance_since_last_used = f32(0)
        self.ambiguous = False
        self.left_index = self.right_index = -1

    # ---- :343-365
    def add_new_fwd_edge_index(self, i):
        if self.first_fwd_edge_index < 0:
            self.first_fwd_edge_index = self.current_fwd_edge_index = i
            return
        prev = self.current_fwd_edge_index
        self.current_fwd_edge_index = i
        self.edges[prev].next_fwd_edge_index = self.current_fwd_edge_index

    def add_new_bwd_edge_index(self, i):
        if self.first_bwd_edge_index < 0:
            self.first_bwd_edge_index = self.current_bwd_edge_index = i
            return
        prev = self.current_bwd_edge_index
        self.current_bwd_edge_index = i
        self.edges[prev].next_bwd_edge_index = self.current_bwd_edge_index

    # ---- :369-417
    def has_fwd_edge(self):
        return self.first_fwd_edge_index >= 0

    def get_first_fwd_edge(self):
        self.current_fwd_edge_index = self.first_fwd_edge_index
        return self.edges[self.current_fwd_edge_index]

    def has_next_fwd_edge(self):
        return self.edges[self.current_fwd_edge_index].next_fwd_edge_index >= 0

    def get_next_fwd_edge(self):
        if self.edges[self.current_fwd_edge_index].next_fwd_edge_index < 0:
            return None
        self.current_fwd_edge_index = self.edges[self.current_fwd_edge_index].next_fwd_edge_index
        return self.edges[self.current_fwd_edge_index]

    def has_bwd_edge(self):
        return self.first_bwd_edge_index >= 0

    def get_first_bwd_edge(self):
        self.current_bwd_edge_index = self.first_bwd_edge_index
        return self.edges[self.current_bwd_edge_index]

    def has_next_bwd_edge(self):
        return self.edges[self.current_bwd_edge_index].next_bwd_edge_index >= 0

    def get_next_bwd_edge(self):
        if self.edges[self.current_bwd_edge_index].next_bwd_edge_index < 0:
            return None
        self.current_bwd_edge_index = self.edges[self.current_bwd_edge_index].next_bwd_edge_index
        return self.edges[self.current_bwd_edge_index]

    def contains_bwd_edge(self, copy):                                # :419-450 (thorough = false)
        if self.has_bwd_edge():
            edge = self.get_first_bwd_edge()
            if copy == edge:
                return True
            while self.has_next_bwd_edge():
                edge = self.get_next_bwd_edge()
                if copy == edge:
                    return True
        return False

    def update_bwd_edge_details(self, copy):                          # :452-502 (thorough = false)
        def take(edge):
            if copy == edge:
                edge.branch_count_as_skipped_edge = copy.branch_count_as_skipped_edge
                edge.branch_count_since_last_used = copy.branch_count_since_last_used
                edge.branch_distance_since_last_used = copy.branch_distance_since_last_used
                edge.set_weight(f32(float(copy.posterior_weight)))    # get_posterior_weight() is a double, set_weight takes a float
        if self.has_bwd_edge():
            take(self.get_first_bwd_edge())
            while self.has_next_bwd_edge():
                take(self.get_next_bwd_edge())

    def delete_bwd_edge(self, edge_ind):                              # :537-581
        if self.has_bwd_edge():
            edge = self.get_first_bwd_edge()
            if edge.index == edge_ind:
                if self.has_next_bwd_edge():
                    edge2 = self.get_next_bwd_edge()
                    self.current_bwd_edge_index = self.first_bwd_edge_index = edge2.index
                else:
                    self.current_bwd_edge_index = self.first_bwd_edge_index = -1
                return
            while self.has_next_bwd_edge():
                prev_ind = edge.index
                edge = self.get_next_bwd_edge()
                if edge.index == edge_ind:
                    if self.has_next_bwd_edge():
                        edge = self.get_next_bwd_edge()
                        self.edges[prev_ind].next_bwd_edge_index = edge.index
                    else:
                        self.edges[prev_ind].next_bwd_edge_index = -1

    def delete_fwd_edge(self, edge_ind):                              # :583-625
        if self.has_fwd_edge():
            edge = self.get_first_fwd_edge()
            if edge.index == edge_ind:
                if self.has_next_fwd_edge():
                    edge = self.get_next_fwd_edge()
                    self.current_fwd_edge_index = self.first_fwd_edge_index = edge.index
                else:
                    self.current_fwd_edge_index = self.first_fwd_edge_index = -1
                return
            while self.has_next_fwd_edge():
                prev_ind = edge.index
                edge = self.get_next_fwd_edge()
                if edge.index == edge_ind:
                    if self.has_next_fwd_edge():
                        edge = self.get_next_fwd_edge()
                        self.edges[prev_ind].next_fwd_edge_index = edge.index
                    else:
                        self.edges[prev_ind].next_fwd_edge_index = -1


class Sequence:                                                       # sequence.h:640-870
    def __init__(self):
        self.sites = []
        self.edges = []
        self.curr_edge_index = 0

    def push_back_site(self, site):                                   # :716-723
        site.index = len(self.sites)
        self.sites.append(site)

    def push_back_edge(self, edge):                                   # :727-733 (the vector holds a copy)
        edge = edge.copy()
        edge.index = len(self.edges)
        self.edges.append(edge)
        self.curr_edge_index = len(self.edges) - 1

    def get_current_edge_index(self):
        return self.curr_edge_index

    def get_site_at(self, i):
        return self.sites[i]

    def get_bwd_edge_index_at_site(self, site, copy):                 # :756-772
        if not self.sites[site].has_bwd_edge():
            return -1
        edge = self.sites[site].get_first_bwd_edge()
        if edge == copy:
            return edge.index
        while self.sites[site].has_next_bwd_edge():
            edge = self.sites[site].get_next_bwd_edge()
            if edge == copy:
                return edge.index
        return -1

    def contains_this_bwd_edge_at_site(self, site, copy):             # :774-780
        return self.get_bwd_edge_index_at_site(site, copy) >= 0

    def delete_all_bwd_edges_at_site(self, index):                    # :836-852
        site = self.get_site_at(index)
        if site.has_bwd_edge():
            edge = site.get_first_bwd_edge()
            self.get_site_at(edge.start_site_index).delete_fwd_edge(edge.index)
            while site.has_next_bwd_edge():
                edge = site.get_next_bwd_edge()
                self.get_site_at(edge.start_site_index).delete_fwd_edge(edge.index)
        site.first_bwd_edge_index = site.current_bwd_edge_index = -1  # set_first_bwd_edge_index(-1)                :331-334

    def delete_all_fwd_edges_at_site(self, index):                    # :854-870
        site = self.get_site_at(index)
        if site.has_fwd_edge():
            edge = site.get_first_fwd_edge()
            self.get_site_at(edge.end_site_index).delete_bwd_edge(edge.index)
            while site.has_next_fwd_edge():
                edge = site.get_next_fwd_edge()
                self.get_site_at(edge.end_site_index).delete_bwd_edge(edge.index)
        site.first_fwd_edge_index = site.current_fwd_edge_index = -1

    # ---- the test's side: in from / out to the oracle's dump format (oracle/__init__.py: OGraph.flatten, attrs, fwd) ----
    @classmethod
    def from_dump(cls, flat, attrs, fwd):
        sa, sd, ea, ef = attrs
        seq = cls()
        for k in range(ea.shape[0]):
            e = Edge(int(ea[k, 0]), int(ea[k, 1]))
            e.index = k
            e.used_in_alignment = bool(ea[k, 2])
            e.branch_count_since_last_used = int(ea[k, 3])
            e.branch_count_as_skipped_edge = int(ea[k, 4])
            e.posterior_weight = f32(ef[k, 0]); e.log_posterior_weight = f32(ef[k, 1]); e.branch_distance_since_last_used = f32(ef[k, 2])
            seq.edges.append(e)
        fo, fe = fwd
        for s in range(sa.shape[0]):
            t = Site(seq.edges, int(sa[s, 1]), int(sa[s, 2]))
            t.index = s
            t.character_state = int(sa[s, 0])
            t.left_index, t.right_index = int(sa[s, 3]), int(sa[s, 4])
            t.branch_count_since_last_used = int(sa[s, 5])
            t.branch_distance_since_last_used = f32(sd[s])
            t.ambiguous = bool(sa[s, 6])
            seq.sites.append(t)
            for k in range(int(flat.bwd_off[s]), int(flat.bwd_off[s + 1])):       # the lists in their iteration order
                t.add_new_bwd_edge_index(int(flat.bwd_eid[k]))
            for k in range(int(fo[s]), int(fo[s + 1])):
                t.add_new_fwd_edge_index(int(fe[k]))
        return seq

    def mark_used(self, eids):
        for e in eids:
            self.edges[int(e)].used_in_alignment = True

    def dump(self):
        """-> (state, bwd_off, bwd_src, bwd_logw, bwd_eid), (site_attr, site_dist, edge_attr, edge_f), (fwd_off, fwd_eid)"""
        ns, ne = len(self.sites), len(self.edges)
        state = np.zeros(ns, np.int32); off = np.zeros(ns + 1, np.int32)
        src, lw, eid = [], [], []
        sa = np.zeros((ns, 8), np.int32); sd = np.zeros(ns, np.float32)
        fo = np.zeros(ns + 1, np.int32); fe = []
        linked = np.zeros(ne, np.int32)
        for s, t in enumerate(self.sites):
            state[s] = t.character_state
            off[s] = len(src)
            if t.has_bwd_edge():
                e = t.get_first_bwd_edge()
                while True:
                    src.append(e.start_site_index); lw.append(e.log_posterior_weight); eid.append(e.index)
                    if not t.has_next_bwd_edge():
                        break
                    e = t.get_next_bwd_edge()
            fo[s] = len(fe)
            nf = 0
            if t.has_fwd_edge():
                e = t.get_first_fwd_edge()
                while True:
                    fe.append(e.index); linked[e.index] = 1; nf += 1
                    if not t.has_next_fwd_edge():
                        break
                    e = t.get_next_fwd_edge()
            sa[s] = (t.character_state, t.site_type, t.path_state, t.left_index, t.right_index, t.branch_count_since_last_used,
                     int(t.ambiguous), nf)
            sd[s] = t.branch_distance_since_last_used
        off[ns] = len(src); fo[ns] = len(fe)
        ea = np.zeros((ne, 6), np.int32); ef = np.zeros((ne, 3), np.float32)
        for k, e in enumerate(self.edges):
            ea[k] = (e.start_site_index, e.end_site_index, int(e.used_in_alignment), e.branch_count_since_last_used,
                     e.branch_count_as_skipped_edge, linked[k])
            ef[k] = (e.posterior_weight, e.log_posterior_weight, e.branch_distance_since_last_used)
        return ((state, off, np.array(src, np.int32), np.array(lw, np.float32), np.array(eid, np.int32)), (sa, sd, ea, ef),
                (fo, np.array(fe, np.int32)))


# the builder's branches by name, for Basic_alignment's optional counter (tests/parent_scenarios.py says which planted
# input is there for which).  "pass2_runs" is a total, not a branch.
RULES = (
    "start_shorten", "stop_shorten_dup", "stop_shorten_new", "stop_shorten_new_beside_others", "dup_reset",
    "drop_count", "drop_distance",
    # transfer_child_edge_2's if-chain (:604-637).  Its 2nd and 3rd arms ask for an unused child edge and its implicit
    # 4th (nothing changes) is what is left for a used one, so of the eight outcome x used pairs these five exist.
    "history_ends_differ_used", "history_ends_differ_unused", "history_between_used_sites_unused",
    "history_between_skipped_sites_unused", "history_fresh_used",
    "child_weight_not_one", "plain_x_after_y", "plain_y_after_x",
    "pass1_bwd_increment", "pass1_bwd_refused", "pass1_fwd_increment", "pass1_fwd_refused",
    "pass2_runs", "pass2_no_bwd_edge", "pass2_at_or_below_limit", "pass2_over_limit_then_gapped",
    "pass2_over_limit_then_stop_site", "pass2_matched_without_over_limit_edge", "pass2_delete_whole_run",
    "pass2_delete_prefix_of_run", "pass2_edge_starts_before_run",
    "coupling_own_first_edge_lost", "coupling_matched_site_edge_lost",
)


class Basic_alignment:
    def __init__(self, left, right, left_branch_length, right_branch_length, parsimony, S, char_as, flags=0, counter=None):
        """counter: None, or a mapping (collections.Counter) that takes one count per rule taken, by the names in RULES;
        counting changes nothing that is built."""
        self.counter = counter
        self.left, self.right = left, right
        self.left_branch_length, self.right_branch_length = f32(left_branch_length), f32(right_branch_length)
        self.parsimony, self.S, self.char_as = parsimony, S, char_as
        # set_basic_settings, basic_alignment.h:544-571
        self.max_allowed_skip_distance = f32(0.5)
        self.max_allowed_skip_branches = 10
        self.max_allowed_match_skip_branches = 5
        self.branch_skip_probability = f32(0.9)
        self.reduced_terminal_gap_penalties = True                    # set_additional_settings :626-627 (no --no-reduced-...)
        if flags & 1:                                                 # set_reads_alignment_settings :573-586
            self.max_allowed_skip_distance = f32(5)
            self.max_allowed_skip_branches = 50000
            self.max_allowed_match_skip_branches = 50000
            self.branch_skip_probability = f32(1)
        if flags & 2:
            self.reduced_terminal_gap_penalties = False

    def hit(self, rule):
        if self.counter is not None:
            assert rule in RULES, rule
            self.counter[rule] += 1

    def build_ancestral_sequence(self, sequence, path):               # basic_alignment.cpp:36-59
        self.create_ancestral_sequence(sequence, path)
        self.create_ancestral_edges(sequence)
        self.check_skipped_boundaries(sequence)

    def create_ancestral_sequence(self, sequence, path):              # :61-179
        left, right = self.left, self.right
        edges = sequence.edges
        first_site = Site(edges, start_site, ends_site)
        first_site.character_state = -1
        first_site.left_index, first_site.right_index = 0, 0
        sequence.push_back_site(first_site)
        l_pos = r_pos = 1
        for (_l, _r, ps) in path:
            site = Site(edges)
            # mp.matrix x_mat / y_mat / m_mat and real_site, folded into the column's path state by the aligner's replay
            if ps in (xgapped, xskipped):
                c = left.get_site_at(l_pos)
                site.character_state = c.character_state
                if c.ambiguous:
                    site.ambiguous = True
                if ps == xgapped:
                    site.path_state = xgapped
                else:
                    site.path_state = xskipped
                    site.branch_count_since_last_used = c.branch_count_since_last_used + 1
                    site.branch_distance_since_last_used = f32(c.branch_distance_since_last_used + self.left_branch_length)
                site.left_index, site.right_index = l_pos, -1
                l_pos += 1
            elif ps in (ygapped, yskipped):
                c = right.get_site_at(r_pos)
                site.character_state = c.character_state
                if c.ambiguous:
                    site.ambiguous = True
                if ps == ygapped:
                    site.path_state = ygapped
                else:
                    site.path_state = yskipped
                    site.branch_count_since_last_used = c.branch_count_since_last_used + 1
                    site.branch_distance_since_last_used = f32(c.branch_distance_since_last_used + self.right_branch_length)
                site.left_index, site.right_index = -1, r_pos
                r_pos += 1
            elif ps == matched:
                lc = left.get_site_at(l_pos).character_state
                rc = right.get_site_at(r_pos).character_state
                site.character_state = int(self.parsimony[lc + rc * self.S])        # Int_matrix::g(i, j) = data[i + j * x]
                if lc != rc or lc >= self.char_as:                                  # model->is_ambiguity_character(lc)
                    site.ambiguous = True
                site.path_state = matched
                site.left_index, site.right_index = l_pos, r_pos
                l_pos += 1
                r_pos += 1
            else:
                raise ValueError("path state %d" % ps)
            sequence.push_back_site(site)
        last_site = Site(edges, stop_site, ends_site)
        last_site.character_state = -1
        last_site.left_index, last_site.right_index = len(left.sites) - 1, len(right.sites) - 1
        sequence.push_back_site(last_site)

    def create_ancestral_edges(self, sequence):                       # :181-368
        sites = sequence.sites
        left_child_index, right_child_index = [], []
        for i in range(len(sites)):
            if sites[i].left_index >= 0:
                left_child_index.append(i)
            if sites[i].right_index >= 0:
                right_child_index.append(i)
        prev_path_state = -1                                          # Edge_history prev(-1,-1)
        for i in range(1, len(sites)):
            psite = sites[i]
            pstate = psite.path_state
            if psite.left_index >= 0:
                tsite = self.left.get_site_at(psite.left_index)
                if tsite.has_bwd_edge():
                    child = tsite.get_first_bwd_edge()
                    self.transfer_child_edge(sequence, child, left_child_index, self.left_branch_length)
                    while tsite.has_next_bwd_edge():
                        child = tsite.get_next_bwd_edge()
                        self.transfer_child_edge(sequence, child, left_child_index, self.left_branch_length)
                # (:250-284: edges_for_skipped_flanked_by_gaps is false)
                if pstate in (xgapped, xskipped) and prev_path_state in (ygapped, yskipped):      # :286-296
                    self.hit("plain_x_after_y")
                    edge = Edge(i - 1, i, 1.0)
                    sequence.push_back_edge(edge)
                    sequence.get_site_at(edge.start_site_index).add_new_fwd_edge_index(sequence.get_current_edge_index())
                    sequence.get_site_at(edge.end_site_index).add_new_bwd_edge_index(sequence.get_current_edge_index())
            if psite.right_index >= 0:
                tsite = self.right.get_site_at(psite.right_index)
                if tsite.has_bwd_edge():
                    child = tsite.get_first_bwd_edge()
                    self.transfer_child_edge(sequence, child, right_child_index, self.right_branch_length)
                    while tsite.has_next_bwd_edge():
                        child = tsite.get_next_bwd_edge()
                        self.transfer_child_edge(sequence, child, right_child_index, self.right_branch_length)
                if pstate in (ygapped, yskipped) and prev_path_state in (xgapped, xskipped):      # :350-358
                    self.hit("plain_y_after_x")
                    edge = Edge(i - 1, i, 1.0)
                    sequence.push_back_edge(edge)
                    sequence.get_site_at(edge.start_site_index).add_new_fwd_edge_index(sequence.get_current_edge_index())
                    sequence.get_site_at(edge.end_site_index).add_new_bwd_edge_index(sequence.get_current_edge_index())
            prev_path_state = pstate

    def transfer_child_edge(self, sequence, child, child_index, branch_length):     # :510-569
        edge = Edge(child_index[child.start_site_index], child_index[child.end_site_index], 1.0)    # (weight_edges is false)
        stop_shortened = False
        if self.reduced_terminal_gap_penalties:
            if sequence.get_site_at(edge.start_site_index).site_type == start_site and edge.end_site_index - edge.start_site_index > 1:
                if child.end_site_index - child.start_site_index == 1:
                    self.hit("start_shorten")
                    edge.start_site_index = edge.end_site_index - 1
            if sequence.get_site_at(edge.end_site_index).site_type == stop_site and edge.end_site_index - edge.start_site_index > 1:
                if child.end_site_index - child.start_site_index == 1:
                    edge.end_site_index = edge.start_site_index + 1
                    stop_shortened = True
        # (:540-563: pair_end_reads is false)
        self.transfer_child_edge_2(sequence, edge, child, branch_length, stop_shortened=stop_shortened)

    def transfer_child_edge_2(self, sequence, edge, child, branch_length, branch_weight=f32(1.0), stop_shortened=False):  # :572-653
        # (stop_shortened is the counters' alone: whether :535-539 moved this edge's end off the stop site)
        end = sequence.get_site_at(edge.end_site_index)
        if end.contains_bwd_edge(edge):                               # no identical copies
            self.hit("stop_shorten_dup" if stop_shortened else "dup_reset")
            end.update_bwd_edge_details(edge)
            return
        if not child.used_in_alignment and child.branch_count_since_last_used + 1 > self.max_allowed_skip_branches:
            self.hit("drop_count")
            return
        if not child.used_in_alignment and f32(child.branch_distance_since_last_used + f32(branch_length)) > self.max_allowed_skip_distance:
            self.hit("drop_distance")
            return
        used = "used" if child.used_in_alignment else "unused"
        if child.posterior_weight != f32(1.0):
            self.hit("child_weight_not_one")
        start = sequence.get_site_at(edge.start_site_index)
        dist_start, dist_end = start.branch_distance_since_last_used, end.branch_distance_since_last_used
        count_start, count_end = start.branch_count_since_last_used, end.branch_count_since_last_used

        def penalty():
            # branch_weight * child->get_posterior_weight() * this->branch_skip_probability: float * double * float, in double,
            # handed to multiply_weight(float)
            return f32(float(branch_weight) * float(child.posterior_weight) * float(self.branch_skip_probability))
        if dist_start != dist_end or count_start != count_end:
            self.hit("history_ends_differ_" + used)
            edge.branch_distance_since_last_used = max(dist_start, dist_end)
            edge.branch_count_since_last_used = max(count_start, count_end)
            edge.multiply_weight(penalty())
        elif not child.used_in_alignment and count_start == 0 and count_end == 0:
            self.hit("history_between_used_sites_unused")
            edge.branch_distance_since_last_used = f32(child.branch_distance_since_last_used + f32(branch_length))
            edge.branch_count_since_last_used = child.branch_count_since_last_used + 1
            edge.multiply_weight(penalty())
        elif not child.used_in_alignment:
            self.hit("history_between_skipped_sites_unused")
            edge.branch_distance_since_last_used = f32(child.branch_distance_since_last_used + f32(branch_length))
            edge.branch_count_since_last_used = child.branch_count_since_last_used + 1
        else:
            self.hit("history_fresh_used")
        if not sequence.contains_this_bwd_edge_at_site(edge.end_site_index, edge):
            if stop_shortened:
                self.hit("stop_shorten_new")
                if end.has_bwd_edge():
                    self.hit("stop_shorten_new_beside_others")
            if not child.used_in_alignment:
                edge.branch_count_as_skipped_edge = child.branch_count_as_skipped_edge
            else:
                edge.branch_count_as_skipped_edge = 0
            sequence.push_back_edge(edge)
            sequence.get_site_at(edge.start_site_index).add_new_fwd_edge_index(sequence.get_current_edge_index())
            sequence.get_site_at(edge.end_site_index).add_new_bwd_edge_index(sequence.get_current_edge_index())

    def check_skipped_boundaries(self, sequence):                     # :370-489
        sites = sequence.sites
        for i in range(len(sites)):
            tsite = sites[i]
            if tsite.has_bwd_edge():
                edge = tsite.get_first_bwd_edge()
                while tsite.has_next_bwd_edge():
                    another = tsite.get_next_bwd_edge()
                    if another.start_site_index > edge.start_site_index:
                        edge = another
                psite = sites[edge.start_site_index]
                # `psite->get_path_state()==Site::start_site`: a path state compared with a site type's number (0)
                if (psite.path_state == matched or psite.path_state == start_site) and tsite.path_state in (xskipped, yskipped):
                    self.hit("pass1_bwd_increment")
                    edge.branch_count_as_skipped_edge += 1
                elif tsite.path_state in (xskipped, yskipped):
                    self.hit("pass1_bwd_refused")
            if tsite.has_fwd_edge():
                edge = tsite.get_first_fwd_edge()
                while tsite.has_next_fwd_edge():
                    another = tsite.get_next_fwd_edge()
                    if another.start_site_index < edge.start_site_index:
                        edge = another
                nsite = sites[edge.end_site_index]
                if tsite.path_state in (xskipped, yskipped) and (nsite.path_state == matched or nsite.path_state == ends_site):
                    self.hit("pass1_fwd_increment")
                    edge.branch_count_as_skipped_edge += 1
                elif tsite.path_state in (xskipped, yskipped):
                    self.hit("pass1_fwd_refused")
        alone = self.decisions_against_undeleted_lists(sequence) if self.counter is not None else None
        non_skipped = True
        skip_start = -1
        for i in range(1, len(sites)):
            tsite = sites[i]
            tstate = tsite.path_state
            if non_skipped and tstate in (xskipped, yskipped):
                run_first, run_edge = i, -1
                if tsite.has_bwd_edge():
                    edge = tsite.get_first_bwd_edge()
                    while tsite.has_next_bwd_edge():
                        another = tsite.get_next_bwd_edge()
                        if another.start_site_index > edge.start_site_index:
                            edge = another
                    run_edge = edge.index
                    if edge.branch_count_as_skipped_edge > self.max_allowed_match_skip_branches:
                        skip_start = i
                non_skipped = False
                if alone is not None:
                    self.count_run(sequence, alone, run_first, run_edge, skip_start)
            if not non_skipped and skip_start >= 0 and tstate == matched:
                edge_ind = -1
                if tsite.has_bwd_edge():
                    edge = tsite.get_first_bwd_edge()
                    if edge.branch_count_as_skipped_edge > self.max_allowed_match_skip_branches:
                        edge_ind = edge.index
                    while tsite.has_next_bwd_edge():
                        edge = tsite.get_next_bwd_edge()
                        if edge.branch_count_as_skipped_edge > self.max_allowed_match_skip_branches:
                            edge_ind = edge.index
                if edge_ind >= 0:
                    self.delete_edge_range(sequence, edge_ind, skip_start)
                non_skipped = True
                skip_start = -1
            if tstate in (xgapped, ygapped, matched):
                non_skipped = True
                skip_start = -1

    # ---- the counters' side of pass 2: nothing below changes a graph ----
    def run_behind(self, sequence, f):
        m = f + 1
        while sequence.sites[m].path_state in (xskipped, yskipped):
            m += 1
        return m

    def decisions_against_undeleted_lists(self, sequence):
        """{first site of a run: (edge of its own list that decides, last over-limit edge of the matched site's list or -1,
        deleted interval)} with every list as pass 1 left it -- what each run would do if no other run deleted anything."""
        sites, lim, out = sequence.sites, self.max_allowed_match_skip_branches, {}
        def bwd(t):
            k, v = t.first_bwd_edge_index, []
            while k >= 0:
                v.append(sequence.edges[k]); k = sequence.edges[k].next_bwd_edge_index
            return v
        for f in range(1, len(sites) - 1):
            if sites[f].path_state not in (xskipped, yskipped) or sites[f - 1].path_state in (xskipped, yskipped):
                continue
            m = self.run_behind(sequence, f)
            e0, last, a, b = -1, -1, 0, -1
            for e in bwd(sites[f]):
                if e0 < 0 or e.start_site_index > sequence.edges[e0].start_site_index:
                    e0 = e.index
            if e0 >= 0 and sequence.edges[e0].branch_count_as_skipped_edge > lim and sites[m].path_state == matched:
                for e in bwd(sites[m]):
                    if e.branch_count_as_skipped_edge > lim:
                        last = e.index
                if last >= 0 and sequence.edges[last].start_site_index >= f:
                    a, b = f, sequence.edges[last].start_site_index
            out[f] = (e0, last, (a, b))
        return out

    def count_run(self, sequence, alone, f, e0, skip_start):
        """One run of skipped sites, at the moment the sequential scan has decided on its first site (the lists of the
        matched site behind it cannot change any more before the scan gets there: deletions only reach backwards)."""
        sites, lim = sequence.sites, self.max_allowed_match_skip_branches
        self.hit("pass2_runs")
        m = self.run_behind(sequence, f)
        last, a, b = -1, 0, -1
        if e0 < 0:
            self.hit("pass2_no_bwd_edge")
        elif skip_start < 0:
            self.hit("pass2_at_or_below_limit")
        elif sites[m].path_state != matched:
            self.hit("pass2_over_limit_then_stop_site" if sites[m].site_type == stop_site else "pass2_over_limit_then_gapped")
        else:
            t = sites[m]
            k = t.first_bwd_edge_index
            while k >= 0:
                if sequence.edges[k].branch_count_as_skipped_edge > lim:
                    last = k
                k = sequence.edges[k].next_bwd_edge_index
            if last < 0:
                self.hit("pass2_matched_without_over_limit_edge")
            elif sequence.edges[last].start_site_index < f:
                self.hit("pass2_edge_starts_before_run")
            else:
                a, b = f, sequence.edges[last].start_site_index
                self.hit("pass2_delete_whole_run" if b == m - 1 else "pass2_delete_prefix_of_run")
        if (a, b) != alone[f][2]:
            self.hit("coupling_own_first_edge_lost" if e0 != alone[f][0] else "coupling_matched_site_edge_lost")

    def delete_edge_range(self, sequence, edge_ind, skip_start_site):  # :491-508
        edge = sequence.edges[edge_ind]
        this_site_index = edge.start_site_index
        while this_site_index >= skip_start_site:
            sequence.get_site_at(this_site_index).site_type = non_real
            sequence.delete_all_bwd_edges_at_site(this_site_index)
            sequence.delete_all_fwd_edges_at_site(this_site_index)
            this_site_index -= 1


def build_parent(left, right, cols, left_used, right_used, lbl, rbl, parsimony, char_as, flags=0, counter=None):
    """left / right: Sequence; cols: (n, 3) array of (left, right, path state).  Marks the children's used edges, as
    OGraph.parent does, and returns the parent Sequence.  counter: see Basic_alignment."""
    left.mark_used(left_used)
    right.mark_used(right_used)
    S = int(round(len(parsimony) ** 0.5))
    seq = Sequence()
    Basic_alignment(left, right, lbl, rbl, parsimony, S, char_as, flags, counter).build_ancestral_sequence(seq, [tuple(int(x) for x in c) for c in cols])
    return seq
