"""Stage 0 of the dense NN batch kernel: 32-bit byte offsets for its reads, the wrapping clamp min(position, b - 1) of the slots beyond a
run, and the 8-lane folds and run-bound broadcasts as ds_swizzle (kernels.hpp coop_screen_rows, coop_stage0, coop_argmin8).

Every test compares the cell-pruned search with the all-fp64 brute force (ALGO_STREAM_EXACT) on the same cloud: indices and fp64 squared
distances, bit for bit.  The class of input a test is about is counted on the CPU with the kernel's own fp32 cell arithmetic, and the
count is asserted.  The sparse hand-made clouds are built with PCT_PYRAMID=0 (read at every build): left alone, the engine would give
them the pyramid walk, and these tests are about the dense kernel.

Not covered here: the kernel's wide instantiation (nn_grid_coop_kernel<., false>, 64-bit addresses), which the engine launches only for
clouds of more than 2^28 - 16 points, grids of 2^30 cells or batches beyond 2^28 queries.  The second needs no large cloud -- a bounding
box of [0, 1023]^3 with unit cells -- and test_gpu_grid_limits.py runs the wide form there, on queries whose run ends at cell_start[2^30],
and the narrow form on the largest table it is allowed; the other two sizes no test can afford, and they stay uncovered.  The wide form
shares the wrapping clamp and the swizzle folds with the narrow form tested here and keeps the addressing the kernel had before; the choice
between the two is tested on the host (test_stage0_addressing_host.py).
"""
import numpy as np
import pytest

from pointcloudtraj_amd import synth

import test_gpu_stage0_tails as T0

pytestmark = pytest.mark.gpu

SORTED_Q = T0.SORTED_Q    # batches of at least this many queries are counting-sorted by cell first
MAIN = T0.MAIN            # records of a run screened by the main slots: lane + 8 * slot, 8 lanes, 2 slots


@pytest.fixture(scope="module")
def E():
    from pointcloudtraj_amd import engine
    engine.init(0)
    return engine


def stage0_runs(info, pts, q):
    """(rs, re, ok): [Q, 4] bounds of the four x-runs of every query's 2x2x2 block as coop_stage0 hands them to the screening (a disabled row
    is the empty run [a, a)), and which rows are enabled -- the kernel's own fp32 cell arithmetic, as stage0_run_lengths"""
    gx, gy, gz = info["dims"]
    o = np.asarray(info["origin"], np.float32)
    inv_h = np.float32(1.0) / np.float32(info["cell_size"])
    g = np.array([gx, gy, gz], np.float32)

    def cells(v):
        t = np.floor((v.astype(np.float32) - o) * inv_h)
        return np.minimum(np.maximum(t, np.float32(0)), g - np.float32(1))

    pc = cells(pts).astype(np.int64)
    count = np.bincount((pc[:, 2] * gy + pc[:, 1]) * gx + pc[:, 0], minlength=gx * gy * gz)
    start = np.concatenate([[0], np.cumsum(count)]).astype(np.int64)                 # cell_start
    cf = cells(q)
    f = (q.astype(np.float32) - o) * inv_h - cf
    ci = cf.astype(np.int64)
    lo = np.maximum(np.where(f < np.float32(0.5), ci - 1, ci), 0)
    hi = np.minimum(np.where(f < np.float32(0.5), ci, ci + 1), np.array([gx, gy, gz]) - 1)
    rs = np.zeros((len(q), 4), np.int64)
    re = np.zeros((len(q), 4), np.int64)
    ok = np.zeros((len(q), 4), bool)
    for ri in range(4):
        y = hi[:, 1] if ri & 1 else lo[:, 1]
        z = hi[:, 2] if ri >> 1 else lo[:, 2]
        ok[:, ri] = ~(((ri >> 1) == 1) & (hi[:, 2] == lo[:, 2])) & ~(((ri & 1) == 1) & (hi[:, 1] == lo[:, 1]))
        row = (z * gy + y) * gx
        rs[:, ri] = start[row + lo[:, 0]]
        re[:, ri] = np.where(ok[:, ri], start[row + hi[:, 0] + 1], rs[:, ri])
    return rs, re, ok


def winner_run(info, pts, q, winner):
    """which of the four runs of its query's block holds each winner (-1: none, the query was decided beyond stage 0)"""
    gx, gy, gz = info["dims"]
    o = np.asarray(info["origin"], np.float32)
    inv_h = np.float32(1.0) / np.float32(info["cell_size"])
    g = np.array([gx, gy, gz], np.float32)
    cells = lambda v: np.minimum(np.maximum(np.floor((v.astype(np.float32) - o) * inv_h), np.float32(0)), g - np.float32(1)).astype(np.int64)
    wc, qc = cells(pts[winner]), cells(q)
    f = (q.astype(np.float32) - o) * inv_h - qc.astype(np.float32)
    lo = np.maximum(np.where(f < np.float32(0.5), qc - 1, qc), 0)
    hi = np.minimum(np.where(f < np.float32(0.5), qc, qc + 1), np.array([gx, gy, gz]) - 1)
    inside = np.all((wc >= lo) & (wc <= hi), axis=1)
    ri = (wc[:, 1] != lo[:, 1]).astype(np.int64) + 2 * (wc[:, 2] != lo[:, 2]).astype(np.int64)
    return np.where(inside, ri, -1)


def antidiagonal_cloud(n, m, seed):
    """n points in the cells (i, m-1-i, m-1-i) of an m^3 cube of unit cells, i = k mod m: the lowest rows (y = 0, z = 0) hold one occupied
    cell, the last one of the row; the highest rows (y = z = m-1) the first one.  Two corner points pin the bounding box for m > 1."""
    k = np.arange(n) % m
    base = np.stack([k, m - 1 - k, m - 1 - k], axis=1).astype(np.float32)
    pts = (base + np.float32(0.05) + np.float32(0.9) * synth.uniform_points(seed, n, 0.0, 1.0)).astype(np.float32)
    if n >= 2 and m > 1:
        pts[0] = (0.0, m - 0.5, m - 0.5)                    # cell (0, m-1, m-1): x origin, upper y and z extent
        pts[m - 1 if n >= m else n - 1] = (m - 0.5, 0.0, 0.0)      # cell (m-1, 0, 0): y and z origin, upper x extent
    return pts


def corner_queries(seed, Q, m):
    """half of the batch around the cube's corner (0, 0, 0), half around (m, m, m), a cell to either side"""
    lo = synth.uniform_points(seed, Q // 2, -1.0, 1.0)
    hi = synth.uniform_points(seed + 1, Q - Q // 2, m - 1.0, m + 1.0)
    return np.concatenate([lo, hi]).astype(np.float32)


def sparse_grid(E, monkeypatch, pts, cell=1.0):
    monkeypatch.setenv("PCT_PYRAMID", "0")
    c = T0.grid_cloud(E, pts, cell)
    return c, c.grid_info()


def test_empty_runs_at_both_ends_of_the_record_array(E, monkeypatch):
    """a 6^3 cube with 60 points on its anti-diagonal, queries from a box one cell wider: the blocks at the low corners hold empty runs at
    the start of the record array (a == b == 0: the wrapping clamp leaves the positions unclamped), those at the high corners empty runs
    at its end (a == b == n), the blocks at the faces disabled rows; both the arrival-order and the sorted path"""
    m, n = 6, 60
    pts = antidiagonal_cloud(n, m, 5101)
    c, info = sparse_grid(E, monkeypatch, pts)
    assert info["dims"] == (m, m, m)
    for Q, seed in ((64, 5110), (SORTED_Q + 3, 5112)):
        q = corner_queries(seed, Q, m) if Q == 64 else synth.uniform_points(seed, Q, -1.0, m + 1.0)
        T0.check_against_exact(E, c, q, f"anti-diagonal cloud, Q = {Q}")
        rs, re, ok = stage0_runs(info, pts, q)
        counts = {"a == b == 0": int(((rs == 0) & (re == 0)).any(axis=1).sum()), "a == b == n": int(((rs == n) & (re == n)).any(axis=1).sum()),
                  "a disabled row": int((~ok).any(axis=1).sum()), "a == b in the middle": int(((rs == re) & (rs > 0) & (rs < n)).any(axis=1).sum())}
        print(Q, counts)
        assert min(counts.values()) >= (20 if Q == 64 else 200), (Q, counts)
    c.close()


@pytest.mark.parametrize("n", [1, 2, 5, 15])
def test_tiny_clouds_read_the_pad_records(E, monkeypatch, n):
    """clouds of fewer records than a group's 16 main slots: an empty run at the start of the array sends its lanes to records sub + 8 j <= 15,
    beyond the n written ones -- the spare records behind them (kGridPad), masked; arrival-order and sorted path"""
    m = min(n, 5)
    pts = antidiagonal_cloud(n, m, 5200 + n)
    c, info = sparse_grid(E, monkeypatch, pts)
    assert info["dims"] == (m, m, m) and n < MAIN
    for Q, seed in ((64, 5210 + n), (SORTED_Q + 3, 5230 + n)):
        q = corner_queries(seed, Q, m) if Q == 64 else synth.uniform_points(seed, Q, -1.0, m + 1.0)
        T0.check_against_exact(E, c, q, f"{n} points, Q = {Q}")
        rs, re, _ = stage0_runs(info, pts, q)
        start_empty = int(((rs == 0) & (re == 0)).any(axis=1).sum())
        print(n, Q, start_empty)
        assert start_empty >= (20 if Q == 64 else 1000), (n, Q, start_empty)       # their lanes read records n .. 15
    c.close()


def test_winner_in_every_lane_slot_and_run(E):
    """four runs in the four rows of one block, three of 16 records and one of 24 (T = 8: the shared tail slot is in use): every record is
    the winner of three queries.  A run of exactly 16 records fills the positions lane + 8 * slot of its main slots once each, so its 16
    winners cover all 8 lanes and both slots whatever the order inside a cell; the 24-record run adds the 8 positions of the tail slot."""
    rows = [(2.6, 2.6), (3.3, 2.6), (2.6, 3.3), (3.3, 3.3)]            # (y, z): runs 0..3 of the block y, z in {2, 3}
    lengths = [16, 16, 24, 16]
    runs = [T0.run_points(L, y, z) for L, (y, z) in zip(lengths, rows)]
    pts = T0.hand_cloud(runs)
    c, info = T0.hand_grid(E, pts)
    first = len(pts) - sum(lengths)
    rec = np.concatenate(runs)
    q = np.concatenate([rec - np.array([0.0, 1e-3, 0.0], np.float32), rec + np.array([0.0, 1e-3, 0.0], np.float32),
                        rec - np.array([0.0, 0.0, 1e-3], np.float32)]).astype(np.float32)
    want = np.tile(first + np.arange(len(rec)), 3)
    rs, re, ok = stage0_runs(info, pts, q)
    assert np.array_equal(re - rs, np.tile(lengths, (len(q), 1))) and ok.all()
    for what, qq in (("sorted path", T0.padded(q, SORTED_Q + 3)), ("arrival-order path", q)):
        ri, _ = T0.check_against_exact(E, c, qq, what)
        assert np.array_equal(ri[:len(q)], want), what                 # every record of every run is the winner of its three queries
    # Counted from the batch's answers (ri == want was asserted above, so these are the kernel's winners).  The order of the records inside a
    # cell is the index build's business, so a record's rank in its run is not known here; what is known is that the L records of run k sit
    # at its L positions rs .. rs + L - 1, each at one.  With wins[r] > 0 for every record, every rank 0 .. L - 1 of every run -- lane
    # rank % 8, main slot rank // 8 for rank < 16, the tail slot for rank >= 16 -- held a winner; and with every record winning equally
    # often (w), the 8 ranks of the tail slot held w * 8 winners whichever 8 records of the run they are.
    wins = np.bincount(ri[:len(q)] - first, minlength=len(rec))
    assert len(wins) == len(rec) and wins.min() == wins.max() == 3
    held = winner_run(info, pts, q, ri[:len(q)])
    per_run = [int((held == k).sum()) for k in range(4)]
    ranks_hit = [int((wins[sum(lengths[:k]):sum(lengths[:k + 1])] > 0).sum()) for k in range(4)]
    tail = int(wins.max()) * (ranks_hit[2] - MAIN)
    print(per_run, ranks_hit, tail)
    assert ranks_hit == lengths and per_run == [3 * L for L in lengths] and min(per_run) >= 20 and tail >= 20
    c.close()


@pytest.mark.parametrize("Q", [1, 7, 9, 31, 33, 16387])
def test_partly_empty_groups_and_waves(E, Q):
    """batch sizes that leave the last wave (8 queries) and the last block (32 queries) partly empty: the groups without a query stay out of
    stage 0 whole, so the 8 lanes of a group still take the folds together; queries from a box one cell wider than the cloud's"""
    n, side = 20000, 15.0
    pts = synth.uniform_points(5301, n, 0.0, side)
    cell = float(np.cbrt(side ** 3 * 6.0 / n))
    c = T0.grid_cloud(E, pts, cell)
    info = c.grid_info()
    q = synth.uniform_points(5310 + Q, Q, -cell, side + cell)
    T0.check_against_exact(E, c, q, f"Q = {Q}")
    if Q >= SORTED_Q:
        _, _, ok = stage0_runs(info, pts, q)
        disabled = int((~ok).any(axis=1).sum())
        print(disabled)
        assert disabled >= 1000                                        # rows disabled at the grid's faces
    c.close()


def test_exact_fold_breaks_index_ties(E):
    """every point twice: the copies tie in fp32 and in fp64, the exact rescan and coop_argmin8 decide by index -- the lowest wins"""
    half, side = 6000, 10.0
    one = synth.uniform_points(5401, half, 0.0, side)
    pts = np.concatenate([one, one]).astype(np.float32)
    c = T0.grid_cloud(E, pts, float(np.cbrt(side ** 3 * 6.0 / len(pts))))
    for Q, seed in ((SORTED_Q + 3, 5410), (4096, 5411)):
        q = synth.uniform_points(seed, Q, 0.0, side)
        ri, _ = T0.check_against_exact(E, c, q, f"duplicated cloud, Q = {Q}")
        assert ri.max() < half and len(np.unique(ri)) > Q // 8
    c.close()


def test_exact_fold_breaks_distance_ties(E):
    """a lattice of 13^3 points in shuffled order, one per unit cell, queries on the cell centres: the 8 corners of a cell are equally far
    (d2 = 0.75 exactly) and all inside the query's block, so every query goes through the exact fold; the lowest index of the 8 wins"""
    g = 12
    ax = np.arange(g + 1, dtype=np.float32)
    lattice = np.stack(np.meshgrid(ax, ax, ax, indexing="ij"), axis=-1).reshape(-1, 3)
    order = synth.shuffled_order(5501, len(lattice))
    pts = lattice[order].astype(np.float32)
    index_at = np.empty((g + 1,) * 3, np.int64)
    index_at[tuple(pts.astype(np.int64).T)] = np.arange(len(pts))
    c = T0.grid_cloud(E, pts, 1.0)
    info = c.grid_info()
    assert info["dims"] == (g + 1,) * 3 and info["origin"] == (0.0, 0.0, 0.0)
    cc = np.stack(np.meshgrid(*[np.arange(g)] * 3, indexing="ij"), axis=-1).reshape(-1, 3)
    q = (cc.astype(np.float32) + np.float32(0.5)).astype(np.float32)
    want = np.min([index_at[cc[:, 0] + dx, cc[:, 1] + dy, cc[:, 2] + dz] for dx in (0, 1) for dy in (0, 1) for dz in (0, 1)], axis=0)
    rs, re, ok = stage0_runs(info, pts, q)
    assert ok.all() and np.all(re - rs == 2)                           # the block holds the 8 corners: 4 runs of 2
    for what, qq in (("sorted path", T0.padded(q, SORTED_Q + 3)), ("arrival-order path", q)):
        ri, rd = T0.check_against_exact(E, c, qq, what)
        assert np.array_equal(ri[:len(q)], want) and np.all(rd[:len(q)] == 0.75), what
    c.close()
