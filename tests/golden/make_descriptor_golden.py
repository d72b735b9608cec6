"""Generates tests/golden/pipe_descriptors.npz: the descriptor words of pg_fill_pipe for the jobs of
tests/test_descriptors_cpu.py.

PROVENANCE: recorded at commit 2b37f25 (the parent of the commit that split the aligner's host side into dp_plan.cpp) plus
one lift: the packing block inside pagan_batch_create's staging loop was moved verbatim into pack_pipe_descriptors() and
exported as pagan_dp_debug_descriptors, nothing else.  So the words are the ones that commit's pagan_batch_create uploaded.
Run on a later tree it must reproduce the committed file byte for byte:  python tests/golden/make_descriptor_golden.py
(PAGAN_DP_LIB selects the library, as everywhere).  The claims checked while recording are what each job was chosen for.
"""
import io
import os
import sys
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))
import pagan2_msa_amd as pg  # noqa: E402
import test_descriptors_cpu as t  # noqa: E402


def record(name):
    make, n_states, env = t.CASES[name]
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        left, right, band = make()
        return pg.debug_descriptors(left, right, band, n_states)
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def runs(mask):
    """lengths of the runs of True"""
    edges = np.flatnonzero(np.diff(np.concatenate([[0], mask.astype(np.int8), [0]])))
    return edges[1::2] - edges[::2]


def main():
    out = {name: record(name) for name in t.CASES}
    cls = {name: out[name][:, 4].view(np.uint32) & 15 for name in out}
    width = {name: out[name][:, 1] - out[name][:, 0] + 1 for name in out}
    bit = lambda name, b: (out[name][:, 4].view(np.uint32) >> b) & 1  # noqa: E731
    assert set(np.unique(cls["chain"])) == {0, 3}
    assert set(np.unique(cls["far"])) == {1, 2, 3} and bit("far", 5).any() and bit("far", 19).any()
    left, right, band = t.CASES["far"][0]()
    assert pg.debug_far(left, right, band)[0] == 10, "served far sites"
    assert not np.array_equal(out["far"][:, 4], out["far_big_table"][:, 4])
    assert list(runs(cls["box_1800"] == 4)) == [195] and width["box_1800"].max() == 300 and not (cls["box_1800"] == 5).any()
    assert width["box_2400"][cls["box_2400"] == 4].max() == 432 and int((cls["box_2400"] == 5).sum()) == 485
    for name in ("box_1800_wide7_off", "box_1800_after_wide_reach", "box_1800_no_hist_no_three"):
        assert not np.array_equal(out[name][:, 4], out["box_1800"][:, 4]), name
    out = {name: np.ascontiguousarray(w.T) for name, w in out.items()}       # [8, diagonals]: a word's column compresses far better
    out["n_states"] = np.array([t.CASES[name][1] for name in t.CASES], np.int32)
    path = os.path.join(HERE, "pipe_descriptors.npz")
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED, compresslevel=9) as z:       # (np.savez stamps every entry with the time)
        for name in sorted(out):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(out[name]), allow_pickle=False)
            z.writestr(zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0)), buf.getvalue(), zipfile.ZIP_DEFLATED, 9)
    print(path, os.path.getsize(path), "bytes;", {name: out[name].shape[1] for name in t.CASES})


if __name__ == "__main__":
    main()
