"""bench.py --dump-outputs, without a GPU: the arrays of the last step as float32 where exact and float64 otherwise, under
the size limit, the long arrays as a fixed, seeded sample of their rows (the same rows on every run) with the rows named."""
import os
import sys
from types import SimpleNamespace

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def results(n_nodes, n_cols, seed=1):
    rng = np.random.default_rng(seed)
    return [SimpleNamespace(score=-1000.25 - k, status=0, end=(0, n_cols - 1, n_cols - 2, 3, 4), cells=10 ** 7 + k,
                            cols=rng.integers(-1, 120000, (n_cols, 3)).astype(np.int32),
                            left_used=rng.integers(0, 2, n_cols - 5).astype(np.int32),
                            right_used=rng.integers(0, 2, n_cols - 7).astype(np.int32)) for k in range(n_nodes)]


def load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_small_output_is_written_whole(tmp_path):
    rs = results(3, 1000)
    bench.write_outputs(str(tmp_path), bench.alignment_outputs(rs))
    got = load(tmp_path)
    assert not any(k.endswith("_rows") for k in got)
    assert got["score"].dtype == np.float64 and list(got["score"]) == [r.score for r in rs]
    assert got["cols"].dtype == np.float32 and np.array_equal(got["cols"], np.concatenate([r.cols for r in rs]))
    assert np.array_equal(got["n_left_used"], [len(r.left_used) for r in rs])
    assert got["end"].shape == (3, 5)


def test_values_beyond_float32_stay_float64(tmp_path):
    bench.write_outputs(str(tmp_path), {"big": np.array([2 ** 24 + 1, 3], np.int64), "small": np.array([1, 2], np.int64)})
    got = load(tmp_path)
    assert got["big"].dtype == np.float64 and got["big"][0] == 2 ** 24 + 1
    assert got["small"].dtype == np.float32


def test_large_output_is_a_fixed_sample_under_the_limit(tmp_path):
    arrays = bench.alignment_outputs(results(31, 110000))
    a, b = tmp_path / "a", tmp_path / "b"
    bench.write_outputs(str(a), arrays)
    bench.write_outputs(str(b), arrays)
    assert sum(os.path.getsize(os.path.join(a, f)) for f in os.listdir(a)) < 64 * 10 ** 6
    ga, gb = load(a), load(b)
    assert sorted(ga) == sorted(gb) and all(np.array_equal(ga[k], gb[k]) for k in ga)
    rows = ga["cols_rows"].astype(np.int64)
    assert len(rows) < len(arrays["cols"]) and np.all(np.diff(rows) > 0)
    assert np.array_equal(ga["cols"], arrays["cols"][rows])
    assert len(ga["score"]) == 31                                  # the per-node arrays are never sampled
