"""One batch in the default environment that holds a job of every fill kernel, in shuffled order, run twice and fetched: what
pagan_batch_create groups by route and launch_fill launches per group (dp_abi.hip) -- the banded kernel with both table sizes,
the HBM wavefront, the row strips and the tiles beside them on the second stream, the two pg_backptr passes."""
import numpy as np
import pytest

from test_routes_cpu import jobs
from test_tiles_gpu import same

pytestmark = pytest.mark.gpu


def test_a_batch_with_a_job_of_every_route(pg, oracle):
    all_jobs = jobs()
    order = np.random.default_rng(3).permutation(len(all_jobs))
    routes = [sorted(all_jobs)[k] for k in order]
    assert routes != sorted(all_jobs)
    batch = pg.Batch([all_jobs[r] for r in routes])
    batch.run()
    batch.run()
    got = batch.fetch()
    assert batch.debug_reruns() == 0
    batch.close()
    for route, res in zip(routes, got):
        same(res, oracle.dp_align(*all_jobs[route]), route)
