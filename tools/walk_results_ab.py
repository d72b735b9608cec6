"""Check of a host-side refactor: the tree walk's and the pileup chain's results under two builds of the library, byte for byte.

    PAGAN_DP_LIB=<library A> python tools/walk_results_ab.py dump cpu a_cpu.json parent
    PAGAN_DP_LIB=<library B> python tools/walk_results_ab.py dump cpu b_cpu.json result
    python tools/walk_results_ab.py compare a_cpu.json b_cpu.json          (exit status 1 on any difference)

`dump cpu` needs no GPU: the walks go through the oracle's DP behind the batch seam -- DNA anchored balanced 8 leaves; DNA
caterpillar 6 leaves with anchor_mode=1 and force_gap under a memory budget; protein 6 leaves; codons 4 leaves; mostcommon on 6
leaves; a rank-mode walk whose upper half is imported and whose rows are asked for behind finish(lazy=True); a pileup chain of 6
reads of which one is rejected.  `dump gpu` runs the 8-leaf DNA walk on the current device with full_probability=2, with
sample_path=1 on the device's sampler, and with posterior_decode=1 and expected_counts=1.  A dump holds, per walk, the SHA-256 of
every internal node's exported result, of all rows, of the FASTA file with the ancestors, and of what the forward/backward pass
left at the nodes (device times excluded), beside a few plain figures."""
import ctypes as C
import hashlib
import json
import os
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pagan2_msa_amd as pg                                          # noqa: E402
from pagan2_msa_amd import host, synth                               # noqa: E402


def sha(*parts):
    h = hashlib.sha256()
    for p in parts:
        h.update(p if isinstance(p, bytes) else np.ascontiguousarray(p).tobytes() if isinstance(p, np.ndarray) else str(p).encode())
        h.update(b"|")
    return h.hexdigest()


def seam():
    import oracle
    oracle.build()
    L = oracle.lib()

    def fn(n, jobs, opts, out, user):
        for k in range(n):
            j = jobs[k]
            rc = L.oracle_dp_align(j.left, j.right, j.model, j.band if j.band else None, opts, C.byref(out[k]))
            if rc != 0:
                return rc
        return 0
    return fn


def walk_record(msa, passes=False):
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "all.fas")
        msa.write_fasta(path, include_internal=True)
        with open(path, "rb") as f:
            fasta = f.read()
    rows = msa.alignment_all()
    infos = [msa.node_info(k) for k in range(msa.n_internal)]
    rec = {"nodes": [sha(msa.export_result(msa.n + k).tobytes()) for k in range(msa.n_internal)],
           "rows": sha(*rows), "fasta": sha(fasta), "width": len(rows[0]), "parents_built": msa.parents_built,
           "scores": [i.score for i in infos], "hits": [i.n_hits for i in infos], "forced_gaps": [i.n_forced_gaps for i in infos]}
    if passes:
        rec["fb"] = [sha(np.array(msa.node_fb(k)[:2])) for k in range(msa.n_internal)]
        rec["log_fwd"] = [msa.node_fb(k)[0] for k in range(msa.n_internal)]
        rec["support"] = [sha(msa.node_support(k)) for k in range(msa.n_internal)]
        for what, call in (("marginals", msa.node_marginals), ("decode", lambda k: np.array(msa.node_decode(k)[:2])), ("counts", msa.node_counts)):
            try:
                vals = [call(k) for k in range(msa.n_internal)]
            except pg.PaganError as e:                               # (the walk keeps none: the same refusal from both builds)
                rec[what] = "refused %d" % e.code
                continue
            rec[what] = [sha(*[v[key] for key in sorted(v) if v[key] is not None]) if isinstance(v, dict) else sha(v) for v in vals]
    return rec


def dump_cpu():
    fn = seam()
    out = {}

    def run(name, names, seqs, nwk, **opts):
        msa = host.Msa(names, seqs, nwk, **opts)
        msa.set_batch_backend(fn)
        try:
            out[name] = walk_record(msa.align())
        except pg.PaganError as e:
            out[name] = {"error": e.code}
        return msa

    names, seqs, nwk = synth.evolve_balanced(8, 600, branch=0.02, sub=0.02, indel_start=0.004, mean_len=5, seed=41)
    run("dna_anchored_balanced_8", names, seqs, nwk, use_anchors=1)
    # a stretch nothing aligns to in the two deepest leaves: an empty tunnel block for --force-gap to replace
    names, seqs, nwk = synth.evolve_caterpillar(6, 1500, branch=0.02, sub=0.02, indel_start=0.003, mean_len=4, seed=42)
    rng = np.random.default_rng(9)
    junk = lambda n: "".join(np.array(list("ACGT"))[rng.integers(0, 4, n)])
    seqs = [s[:600] + junk(400) + s[1000:] if k < 2 else s for k, s in enumerate(seqs)]
    free = run("dna_caterpillar_6_overlapping_hits", names, seqs, nwk, anchor_mode=1, prefix_hit_length=20)
    need = 0
    for k in range(free.n_internal):
        left, right, _, band = free.node_job(k)
        need = max(need, pg.lib().pagan_dp_predict_bytes(left.n_sites, right.n_sites, C.byref(band.c)))
    run("dna_caterpillar_6_force_gap", names, seqs, nwk, anchor_mode=1, prefix_hit_length=20, force_gap=1, force_gap_threshold=200,
        device_mem_budget=int(need * 0.9))
    names, seqs, nwk = synth.evolve_caterpillar(6, 200, seed=43, alphabet="ARNDCQEGHILKMFPSTWYV")
    run("protein_6", names, seqs, nwk, use_anchors=1, data_type=2)
    names, seqs, nwk = synth.evolve_balanced(4, 300, branch=0.03, sub=0.03, indel_start=0.0, seed=44)
    run("codons_4", names, seqs, nwk, use_anchors=0, data_type=3)
    names, seqs, nwk = synth.evolve_caterpillar(6, 300, seed=45)
    seqs = [s[:50] + "RYN" + s[53:] for s in seqs]                    # ambiguous sites for fix_ambiguous_states
    run("mostcommon_6", names, seqs, nwk, use_anchors=1, mostcommon=1)
    # rank mode: this walk aligns the lower half itself, takes the upper half from the walk that aligned everything
    names, seqs, nwk = synth.evolve_balanced(8, 400, branch=0.02, sub=0.02, indel_start=0.004, mean_len=5, seed=46)
    owner = host.Msa(names, seqs, nwk, use_anchors=1)
    owner.set_batch_backend(fn)
    owner.align()
    rank = host.Msa(names, seqs, nwk, use_anchors=1)
    rank.set_batch_backend(fn)
    rank.align_nodes(rank.ready())
    while rank.remaining:
        for node in rank.ready():
            rank.import_result(owner.export_result(node))
    before = rank.parents_built
    out["rank_mode_upper_half_imported"] = dict(walk_record(rank.finish(lazy=True)), parents_built_before_rows=before)
    # the pileup chain: read 3 is unrelated to the others (it overlaps the reference all the same under the gap-happy pileup
    # model: the threshold of tests/test_pileup_cpu.py drops it)
    names, seqs, _ = synth.evolve_balanced(8, 500, branch=0.01, sub=0.01, indel_start=0.002, mean_len=3, seed=47)
    names, seqs = names[:6], seqs[:6]
    seqs[3] = junk(480)
    pile = host.Pileup(names, seqs, use_anchors=1, min_overlap=0.85)
    pile.set_batch_backend(fn)
    pile.align()
    steps = [pile.step(k) for k in range(pile.n_steps)]
    results = [pile.step_result(k) for k in range(pile.n_steps)]
    out["pileup_6_one_rejected"] = {
        "accepted": [s.accepted for s in steps], "scores": [s.score for s in steps], "rows": sha(*pile.alignment()),
        "steps": [sha(s.read, s.accepted, s.overlap, s.identity, s.aligned, s.matched, s.read_length, s.status, s.cells, s.n_cols) for s in steps],
        "results": [sha(r.status, np.float64(r.score), r.end, r.cols, r.left_used, r.right_used, r.cells) for r in results]}
    return out


def dump_gpu():
    if pg.device_count() < 1:
        raise SystemExit("dump gpu needs a GPU: there is no CPU path")
    names, seqs, nwk = synth.evolve_balanced(8, 300, branch=0.02, sub=0.02, indel_start=0.004, mean_len=5, seed=41)
    out = {}
    for name, opts in (("full_probability_2", dict(full_probability=2)),
                       ("sample_path_on_device", dict(sample_path=1, sample_seed=7, sample_on_device=1)),
                       ("decode_and_counts", dict(posterior_decode=1, expected_counts=1))):
        out[name] = walk_record(host.Msa(names, seqs, nwk, use_anchors=1, **opts).align(), passes=True)
    return out


def compare(path_a, path_b):
    with open(path_a) as f:
        a = json.load(f)
    with open(path_b) as f:
        b = json.load(f)
    bad = 0
    for name in sorted(set(a["walks"]) | set(b["walks"])):
        same = a["walks"].get(name) == b["walks"].get(name)
        fields = [k for k in sorted(a["walks"].get(name, {})) if a["walks"][name].get(k) != b["walks"].get(name, {}).get(k)]
        print("%-36s %s%s" % (name, "equal" if same else "DIFFERENT", "" if same else ": " + ", ".join(fields)))
        bad += not same
    print("%d walk(s), %d different; %s against %s" % (len(a["walks"]), bad, a["library"], b["library"]))
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    if len(sys.argv) != 5 or sys.argv[1] != "dump" or sys.argv[2] not in ("cpu", "gpu"):
        raise SystemExit(__doc__)
    walks = dump_cpu() if sys.argv[2] == "cpu" else dump_gpu()
    with open(sys.argv[3], "w") as f:
        json.dump({"library": sys.argv[4], "walks": walks}, f, indent=1)
    print("%d walk(s) written to %s" % (len(walks), sys.argv[3]))
