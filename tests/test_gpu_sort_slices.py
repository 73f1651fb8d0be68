"""The query sort's slice offsets (kernels.hpp qsort_hist_kernel / qsort_scatter1_kernel): a sort block's slice of each bucket is the
return value of the histogram pass's atomic on the bucket's total, kept in a table with one row of 1,024 offsets per block; the scatter
pass reads its row and issues no global atomic.

What that can get wrong: offsets of another block or another batch (a table row that is stale, too short a table), a bucket total that
is not complete or not zero when a batch starts (three batches on one stream without a synchronise between them, a small one after a
large one), one bucket that holds the whole batch (offsets up to Q, 113 blocks in one chain), and the captured form.

Every case runs the indexed search (PCT_ALGO_GRID, device buffers prefilled with a sentinel, so every row must be overwritten) against
the streaming search (PCT_ALGO_STREAM, which does not sort) on the same queries: indices and fp64 squared distances bit for bit -- a
query filed twice, lost, or written over by another block's shows.  The cloud is 20,000 uniform points in [0, 10)^3.

  a  925,696 queries = 113 full blocks of 8,192, the smallest batch that takes the all-live path with more than one block, and
     925,773 with a ragged last block; the query array aligned and 12 bytes past alignment
  b  every query identical (16,461 and 925,773 queries), and queries alternating between two opposite corners
  c  batches of 925,696, 20,001 and 925,696 (other queries) on one stream, no synchronise in between
  d  a captured graph of a sorted batch (engine.NNPlan, 20,001 queries, PCT_ALGO_GRID), replayed three times with new queries
"""
import numpy as np
import pytest

from pointcloudtraj_amd import synth

pytestmark = pytest.mark.gpu

S_IDX, S_D2 = -7, -1.0
FULL = 113 * 8192             # 925,696
RAGGED = FULL + 77            # 925,773


@pytest.fixture(scope="module")
def E():
    from pointcloudtraj_amd import engine
    engine.init(0)
    return engine


@pytest.fixture(scope="module")
def cloud(E):
    pts = synth.uniform_points(6201, 20_000, 0.0, 10.0)
    c = E.Cloud(len(pts))
    c.set_input(pts)
    c.build_grid()
    assert c.pyramid_info()["levels"] == 0
    c.reserve_queries(RAGGED)
    yield c
    c.close()


class Batch:
    """a query array on the card (skew_floats = 3: 12 bytes past a 16-byte boundary) and sentinel-filled outputs"""

    def __init__(self, q, skew_floats=0):
        import torch
        q = np.ascontiguousarray(q, np.float32)
        self.Q = len(q)
        self.buf = torch.zeros(3 * self.Q + 4 + skew_floats, dtype=torch.float32, device="cuda")
        self.buf[skew_floats:skew_floats + 3 * self.Q] = torch.from_numpy(q.reshape(-1).copy()).cuda()
        self.ptr = self.buf.data_ptr() + 4 * skew_floats
        assert self.buf.data_ptr() % 16 == 0 and self.ptr % 16 == (4 * skew_floats) % 16
        self.idx = torch.full((self.Q,), S_IDX, dtype=torch.int32, device="cuda")
        self.d2 = torch.full((self.Q,), S_D2, dtype=torch.float64, device="cuda")

    def launch(self, E, c):
        import torch
        c.nn_device(self.ptr, self.Q, self.idx.data_ptr(), self.d2.data_ptr(), torch.cuda.current_stream().cuda_stream, E.ALGO_GRID)

    def result(self):
        return self.idx.cpu().numpy().astype(np.int64), self.d2.cpu().numpy()


def grid_nn(E, c, q, skew_floats=0):
    import torch
    b = Batch(q, skew_floats)
    torch.cuda.synchronize()
    b.launch(E, c)
    torch.cuda.synchronize()
    return b.result()


def same(got, ref, what):
    gi, gd = got
    ri, rd = ref
    assert np.array_equal(gd, rd), what
    assert np.array_equal(gi, np.asarray(ri).astype(np.int64)), what


@pytest.fixture(scope="module")
def big(E, cloud):
    """925,773 uniform queries and their streaming answers; the batch of full blocks is a prefix"""
    q = synth.uniform_points(6202, RAGGED, -0.5, 10.5)
    return q, cloud.nn(q, E.ALGO_STREAM)


@pytest.fixture(scope="module")
def other(E, cloud):
    q = synth.uniform_points(6203, FULL, -0.5, 10.5)
    return q, cloud.nn(q, E.ALGO_STREAM)


@pytest.mark.parametrize("skew", [0, 3], ids=["aligned", "12_bytes_past"])
@pytest.mark.parametrize("Q", [FULL, RAGGED], ids=["full_blocks", "ragged_last_block"])
def test_a_full_blocks(E, cloud, big, Q, skew):
    q, (ri, rd) = big
    same(grid_nn(E, cloud, q[:Q], skew), (ri[:Q], rd[:Q]), (Q, skew))


@pytest.mark.parametrize("Q", [16_461, RAGGED])
def test_b_one_bucket(E, cloud, Q):
    p = np.float32([3.25, 7.5, 1.125])
    ri, rd = cloud.nn(p[None, :], E.ALGO_STREAM)
    q = np.repeat(p[None, :], Q, axis=0)
    same(grid_nn(E, cloud, q), (np.repeat(ri, Q), np.repeat(rd, Q)), Q)


def test_b_two_opposite_corners(E, cloud):
    corners = np.float32([[0.0, 0.0, 0.0], [10.0, 10.0, 10.0]])
    ri, rd = cloud.nn(corners, E.ALGO_STREAM)
    which = np.arange(RAGGED) & 1
    same(grid_nn(E, cloud, corners[which]), (ri[which], rd[which]), "corners")


def test_c_three_batches_no_synchronise(E, cloud, big, other):
    import torch
    q, (ri, rd) = big
    q3, ref3 = other
    batches = [Batch(q[:FULL]), Batch(q[:20_001]), Batch(q3)]
    torch.cuda.synchronize()
    for b in batches:
        b.launch(E, cloud)
    torch.cuda.synchronize()
    same(batches[0].result(), (ri[:FULL], rd[:FULL]), "first, 113 blocks")
    same(batches[1].result(), (ri[:20_001], rd[:20_001]), "second, 20 blocks after 113")
    same(batches[2].result(), ref3, "third, other queries")


def test_d_captured_graph(E, cloud, big):
    q, (ri, rd) = big
    Q = 20_001
    plan = E.NNPlan(cloud, Q, E.ALGO_GRID)
    try:
        for k in range(3):
            a = 1000 * k
            gi, gd = plan.run(q[a:a + Q])
            same((gi.astype(np.int64), gd), (ri[a:a + Q], rd[a:a + Q]), ("replay", k))
    finally:
        plan.close()
