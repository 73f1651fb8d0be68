"""The dense NN batch kernel's two block sizes: 128 threads (two waves, 16 queries; kernels.hpp kNNBlock), which the index build chooses
for a cloud whose records fit the Infinity Cache, and 256 threads (32 queries) for larger ones, here through PCT_NN_BLOCK=256, which the
build reads every time.

What a block size can get wrong is the slot arithmetic: which query a group of 8 lanes takes, in the cell-sorted batch (the XCD-contiguous
block order over a block count that is no multiple of 8) and in arrival order, and what the lanes behind the end of the batch do -- a last
block with one live group, with one whole wave idle, with a single query.  Every case compares the cell-pruned search with the all-fp64
brute force (ALGO_STREAM_EXACT) on one cloud of 20,000 points, indexed once per block size: indices and fp64 squared distances, bit
for bit, as in test_gpu_stage0_tails.py.

Not covered here: the kernel's wide instantiation (64-bit addresses), which needs arrays beyond 4 GB and has no switch.  A grid of 2^30
cells has such an array (2^30 + 1 run bounds), and test_gpu_grid_limits.py runs the wide form there at both block sizes; the other two
ways into it (more than 2^28 - 16 points, more than 2^28 queries) stay out of the tests' reach.  Its static figures are in
profiles/nn_persist_asm.txt.
"""
import os

import numpy as np
import pytest

from pointcloudtraj_amd import synth

pytestmark = pytest.mark.gpu

SORTED_Q = 16384          # batches of at least this many queries are counting-sorted by cell first
BLOCK_Q = {128: 16, 256: 32}     # queries per block of the kernel


@pytest.fixture(scope="module")
def E():
    from pointcloudtraj_amd import engine
    engine.init(0)
    return engine


@pytest.fixture(scope="module", params=[128, 256], ids=["block128", "block256"])
def cloud(E, request):
    pts = synth.uniform_points(5101, 20000, 0.0, 20.0)
    c = E.Cloud(len(pts))
    c.set_input(pts)
    before = os.environ.get("PCT_NN_BLOCK")
    if request.param == 256:                          # 128 is what the build chooses for a cloud of this size
        os.environ["PCT_NN_BLOCK"] = "256"
    try:
        c.build_grid()                                # the automatic cell size
    finally:
        if before is None:
            os.environ.pop("PCT_NN_BLOCK", None)
        else:
            os.environ["PCT_NN_BLOCK"] = before
    assert c.pyramid_info()["levels"] == 0, "the cloud must take the dense kernel, not the pyramid walk"
    c.block_q = BLOCK_Q[request.param]
    yield c
    c.close()


def nn_device(E, c, q):
    import torch
    tq = torch.from_numpy(np.ascontiguousarray(q, np.float32)).cuda()
    tidx = torch.empty(len(q), dtype=torch.int32, device="cuda")
    td2 = torch.empty(len(q), dtype=torch.float64, device="cuda")
    c.reserve_queries(len(q))
    c.nn_device(tq.data_ptr(), len(q), tidx.data_ptr(), td2.data_ptr(), torch.cuda.current_stream().cuda_stream, E.ALGO_GRID)
    torch.cuda.synchronize()
    return tidx.cpu().numpy().astype(np.int64), td2.cpu().numpy()


def check_against_exact(E, c, q, what):
    ri, rd = c.nn(q, E.ALGO_STREAM_EXACT)
    gi, gd = nn_device(E, c, q)
    assert np.array_equal(gd, rd), what
    assert np.array_equal(gi, ri.astype(np.int64)), what
    return gi, gd


# queries from a box wider than the cloud's, so border blocks and queries outside the grid occur
def queries(seed, Q):
    return synth.uniform_points(seed, Q, -1.0, 21.0)


@pytest.mark.parametrize("extra", [37, 0, 1], ids=["ragged_37", "whole_blocks", "one_query_in_the_last_block"])
def test_sorted_batch_ends(E, cloud, extra):
    """the cell-sorted path: 16,384 + 37 queries end in a block with five live queries and idle waves behind them and make 1,027 (514)
    blocks, no multiple of 8 (the XCD-contiguous order's remainder branch); one more block than 16,384 ends on a block boundary; + 1 leaves
    one query to the last block"""
    Q = SORTED_Q + (extra or cloud.block_q)
    assert (Q + cloud.block_q - 1) // cloud.block_q % 8 != 0
    check_against_exact(E, cloud, queries(5110 + Q % 97, Q), f"sorted batch of {Q}")


@pytest.mark.parametrize("Q", [5000, 1, 9, 17, 33, 64], ids=["5000", "1", "9", "17", "33", "64"])
def test_arrival_order_batch_ends(E, cloud, Q):
    """the arrival-order path (no sorted records): 5,000 queries end in a block with one live wave; 1 and 9 queries are a single group and
    two groups of one wave; 17 and 33 leave one query to a second block of 16 and of 32; 64 queries fill whole blocks"""
    check_against_exact(E, cloud, queries(5120 + Q % 89, Q), f"arrival-order batch of {Q}")


def test_large_sorted_batch(E, cloud):
    """262,149 queries: 16,385 (8,193) blocks, more than the card holds at once, the last with five queries"""
    check_against_exact(E, cloud, queries(5130, 262149), "sorted batch of 262,149")


def test_work_counters_twin(E, cloud):
    """the instrumented twin of the kernel (set_work_counters) has the same block size: exact answers on a ragged sorted batch, and a work
    count that is the sum of its parts -- a query's scanned points do not depend on the block it falls into, so the batch as a whole and
    the same queries in arrival-order pieces (each below the sort's threshold) report the same totals"""
    Q = SORTED_Q + 37
    q = queries(5140, Q)
    cloud.set_work_counters(True)
    try:
        check_against_exact(E, cloud, q, "instrumented kernel, sorted batch")
        nn_device(E, cloud, q)
        whole = cloud.last_work()
        parts = [0, 0]
        for a in range(0, Q, 5000):
            nn_device(E, cloud, q[a:a + 5000])
            w = cloud.last_work()
            parts[0] += w[0]
            parts[1] += w[1]
    finally:
        cloud.set_work_counters(False)
    print("work, whole batch:", whole, "in pieces:", tuple(parts))
    assert whole[0] > 0 and whole[1] > 0
    assert tuple(parts) == whole
