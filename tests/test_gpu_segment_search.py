"""GPU tests of the capsule search (pct_segment_count_batch*, pct_segment_search_batch*, pct_segment_search_read; kernels in
csrc/segment_search.hpp): the streaming form, the cell-index form and the rolling-map form against the numpy restatement of the
contract (tests/helpers/segment_search_model.py) and against each other.

Every comparison is exact -- np.array_equal on the int64 offsets, the uint32 indices, the fp64 d2 and the fp64 s, over every entry
(s of an entry is never NaN).  Index of a point = its row in the uploaded cloud, or its ring slot = its row in the host mirror."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

from pointcloudtraj_amd import scenarios as S, synth
from test_gpu_ring import Mirror
from test_gpu_ring_search import wrapped_case
from test_gpu_segments import segments, unit_dirs, wrapped_segments

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import segment_model as M  # noqa: E402
import segment_search_model as SS  # noqa: E402

pytestmark = pytest.mark.gpu

INF, NAN = np.inf, np.nan
ORDERS = [0, 1]                              # PCT_ORDER_INDEX, PCT_ORDER_DISTANCE
REACHES = [0.0, 0.5, 6.0, 500.0, INF]


@pytest.fixture(scope="module")
def E():
    from pointcloudtraj_amd import engine
    engine.init(0)
    assert (engine.ORDER_INDEX, engine.ORDER_DISTANCE) == (0, 1)
    return engine


def same(got, want, what=""):
    go, gi, gd, gs = got
    wo, wi, wd, ws = want
    assert go.dtype == np.int64 and gi.dtype == np.uint32 and gd.dtype == np.float64 and gs.dtype == np.float64
    assert np.array_equal(go, wo), f"offsets differ {what}: first at {np.flatnonzero(go != wo)[:5]}"
    assert np.array_equal(gd, wd), f"d2 differs {what}: first at {np.flatnonzero(gd != wd)[:5]}"
    assert np.array_equal(gi, wi), f"idx differs {what}: first at {np.flatnonzero(gi != wi)[:5]}"
    assert np.array_equal(gs, ws), f"s differs {what}: first at {np.flatnonzero(gs != ws)[:5]}"


class Pairs:
    """d2 and s of every row against every segment, once; the rows of any reach and order from them"""

    def __init__(self, pts, segs):
        self.pts, self.segs = np.asarray(pts, np.float32), np.asarray(segs, np.float64).reshape(-1, 6)
        self.base = SS.row_masks(self.pts, self.segs, INF)

    def masks(self, reach):
        a, b = M.narrow(self.segs)
        reach = np.broadcast_to(np.asarray(reach, np.float64), (len(self.segs),))
        out = []
        for q, (d2, s, hit) in enumerate(self.base):
            r2 = M.reach2(reach[q])
            with np.errstate(invalid="ignore"):
                out.append((d2, s, hit & (d2 <= r2) if r2 is not None else np.zeros_like(hit)))
        return out

    def rows(self, reach, order, base=0, Q=None):
        return SS.rows_from(self.masks(reach)[:Q], order, base)


def forms(E, c, segs, reach, order, want, algos, what=""):
    for algo in algos:
        same(c.segment_search(segs, reach, order, algo), want, f"(algo {algo}, order {order} {what})")
    cnt = c.segment_count(segs, reach, algos[0])
    assert cnt.dtype == np.uint32 and np.array_equal(cnt.astype(np.int64), np.diff(want[0])), f"counts differ {what}"


# ---- 1. the streaming form ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 1000])
def test_streaming_form_against_the_model(E, n):
    pts = synth.uniform_points(300 + n, n, 0.0, 10.0)
    with E.Cloud(n) as c:
        c.set_input(pts)
        for Q in (1, 257):
            segs = segments(310 + Q, Q, -1.0, 11.0, [0.0, 0.05, 3.0, 17.4], pts)      # every fifth a on a cloud point
            P = Pairs(pts, segs)
            for reach in (0.0, 1.5, INF):
                for order in ORDERS:
                    want = P.rows(reach, order)
                    same(c.segment_search(segs, reach, order, E.ALGO_STREAM), want, f"(n = {n}, Q = {Q}, reach = {reach}, order {order})")
                    same(c.segment_search(segs, reach, order), want, f"(auto, n = {n}, Q = {Q}, reach = {reach})")      # no index: AUTO streams
                    if reach == 0.0:
                        assert want[0][-1] > 0, "the case has nothing ON a segment"
                    if reach == INF:
                        assert np.all(np.diff(want[0]) == n)
                cnt = c.segment_count(segs, reach, E.ALGO_STREAM)
                assert np.array_equal(cnt.astype(np.int64), np.diff(P.rows(reach, 0)[0]))


# ---- 2. the cell-index form --------------------------------------------------------------------------------------------------------

GRID_Q = 5000


def grid_segments(seed, pts, lo, hi):
    """GRID_Q segments of eight kinds, kind = i % 8: degenerate | 0.05 long | 3 m along the axes in turn | 6 m along a diagonal |
    crossing the grid's border | wholly outside the grid | 1e6 away | 3 m in a random direction; every fifth a on a cloud point"""
    n = GRID_Q
    lo, hi = np.float64(lo), np.float64(hi)
    segs = segments(seed, n, 0.0, 1.0, [0.0, 0.05, 3.0, 6.0, 8.0, 2.0, 3.0, 3.0])
    a = lo + segs[:, :3] * (hi - lo)
    d = segs[:, 3:] - segs[:, :3]
    a[::5] = pts[(np.arange(0, n, 5) * 7) % len(pts)].astype(np.float64)
    k = np.arange(n) % 8
    ax = (np.arange(n) // 8) % 3
    sign = np.where((np.arange(n) // 24) % 2 == 0, 1.0, -1.0)
    d[k == 2] = 3.0 * np.eye(3)[ax[k == 2]]
    d[k == 3] = 6.0 * sign[k == 3, None] * np.float64([1.0, 1.0, -1.0]) / np.sqrt(3.0)
    for i in np.flatnonzero(k == 4):                                           # from inside to 5 m beyond a face
        a[i, ax[i]] = hi[ax[i]] - 3.0 if sign[i] > 0 else lo[ax[i]] + 3.0
        d[i] = 8.0 * sign[i] * np.eye(3)[ax[i]]
    for i in np.flatnonzero(k == 5):                                           # wholly outside, 3 m beyond a face
        a[i, ax[i]] = hi[ax[i]] + 3.0 if sign[i] > 0 else lo[ax[i]] - 5.0
    for i in np.flatnonzero(k == 6):
        a[i, ax[i]] += 1e6 * sign[i]
    return np.concatenate([a, a + d], axis=1)


def mixed_reach(n):
    """mostly 0 and 0.5; 6, 500 and +inf at a few places, so that a batch of 5000 lists about a million entries"""
    r = np.where(np.arange(n) % 2 == 0, 0.5, 0.0)
    r[3::97] = 6.0
    r[5::250] = 500.0
    r[7::250] = INF
    return r


@functools.lru_cache(maxsize=None)
def grid_case(name):
    if name == "uniform":
        pts, cell = synth.uniform_points(1200, 20000, 0.0, 10.0), 0.5
    else:
        pts, cell = S.c5_frame_clustered(0, 20000), 0.0                        # pillar faces on a 0.1 lattice, default cell size
    segs = grid_segments(1210, pts, pts.min(axis=0), pts.max(axis=0))
    return pts, cell, segs, Pairs(pts, segs[:257])


@functools.lru_cache(maxsize=None)
def grid_big_want(name, order):
    pts, _, segs, _ = grid_case(name)
    return SS.segment_search_boxed(pts, segs, mixed_reach(len(segs)), order)


@pytest.fixture(scope="module", params=["uniform", "clustered"])
def gridded(E, request):
    pts, cell, _, _ = grid_case(request.param)
    c = E.Cloud(len(pts))
    c.set_input(pts)
    c.build_grid(cell)
    assert c.has_grid
    yield request.param, c
    c.close()


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("reach", REACHES)
def test_grid_form_every_kind_under_every_reach(E, gridded, reach, order):
    name, c = gridded
    _, _, segs, P = grid_case(name)
    want = P.rows(reach, order)
    if reach == 0.0:
        assert want[0][-1] > 0
    if reach == INF:
        assert np.all(np.diff(want[0]) == len(P.pts))
    forms(E, c, segs[:257], reach, order, want, (E.ALGO_GRID, E.ALGO_STREAM, E.ALGO_AUTO), f"{name}, Q = 257, reach = {reach}")
    one = SS.rows_from(P.masks(reach)[2:3], order)                              # Q = 1: the axis-aligned one
    forms(E, c, segs[2:3], reach, order, one, (E.ALGO_GRID, E.ALGO_STREAM), f"{name}, Q = 1, reach = {reach}")


@pytest.mark.parametrize("order", ORDERS)
def test_grid_form_large_mixed_batch(E, gridded, order):
    name, c = gridded
    _, _, segs, _ = grid_case(name)
    reach = mixed_reach(len(segs))
    want = grid_big_want(name, order)
    lens = np.diff(want[0])
    assert all(np.any(lens[reach == r] > 0) for r in REACHES) and np.any(lens[reach == 0.5] == 0)
    forms(E, c, segs, reach, order, want, (E.ALGO_GRID, E.ALGO_STREAM), f"{name}, Q = {len(segs)}")


def test_auto_takes_the_grid(E, gridded):
    name, c = gridded
    pts, _, segs, P = grid_case(name)
    c.set_work_counters(True)
    try:
        got = c.segment_search(segs[:257], 0.5, 1)
        auto_work = c.last_work()
        c.segment_count(segs[:257], 0.5, E.ALGO_STREAM)
        stream_work = c.last_work()
    finally:
        c.set_work_counters(False)
    same(got, P.rows(0.5, 1))
    print(f"{name}: records read, cells opened: auto {auto_work}, streaming {stream_work}, Q * N = {257 * len(pts)}")
    assert 0 < auto_work[0] < 257 * len(pts) and auto_work[1] > 0
    assert stream_work[0] == 257 * len(pts)


@pytest.mark.parametrize("order", ORDERS)
def test_one_cell_grid_and_index_base(E, order):
    pts = np.tile(np.float32([[3.0, -2.0, 7.5]]), (100, 1))                     # identical points: a one-cell grid
    segs = np.concatenate([np.float64([[3, -2, 7.5, 3, -2, 7.5], [0, -2, 7.5, 6, -2, 7.5], [2, -3, 6.5, 4, -1, 8.5], [3, -2, 8, 3, -2, 20], [50, 50, 50, 60, 50, 50]]),
                           segments(1220, 40, -2.0, 9.0, [0.0, 0.3, 4.0])])
    P = Pairs(pts, segs)
    with E.Cloud(100) as c:
        c.set_input(pts)
        c.build_grid()
        assert c.grid_info()["dims"] == (1, 1, 1)
        for reach in REACHES + [np.resize(np.float64(REACHES), len(segs))]:
            forms(E, c, segs, reach, order, P.rows(reach, order), (E.ALGO_GRID, E.ALGO_STREAM, E.ALGO_AUTO), "one cell")
    pts = synth.uniform_points(1221, 3000, 0.0, 10.0)
    segs = segments(1222, 100, -1.0, 11.0, [0.0, 0.4, 5.0], pts)
    P = Pairs(pts, segs)
    with E.Cloud(3000) as c:
        c.set_input(pts)
        c.set_index_base(1000)
        c.build_grid(0.7)
        for reach in (0.0, 0.9, INF):
            want = P.rows(reach, order, base=1000)
            assert want[1].min() >= 1000
            forms(E, c, segs, reach, order, want, (E.ALGO_GRID, E.ALGO_STREAM), "index_base = 1000")


# ---- 3. the rolling-map form -------------------------------------------------------------------------------------------------------

RING_Q = 126                                 # 21 of each of wrapped_segments' six kinds


@functools.lru_cache(maxsize=None)
def ring_pairs():
    _, win, _, _ = wrapped_case()
    return Pairs(win, wrapped_segments()[0][:RING_Q])


@pytest.fixture(scope="module")
def ring(E):
    """49 000 points through a ring of 30 000 on a 40 m table with cells of 1.0: the frames wrap the ring"""
    frames, win, _, _ = wrapped_case()
    c = E.Cloud(len(win))
    c.ring_index(1.0, (40.0, 40.0, 40.0))
    for f in frames:
        c.append(f)
    assert len(c) == len(win) and c.has_ring_index
    yield c
    c.close()


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("reach", REACHES + ["mixed"])
def test_ring_form_on_the_wrapped_window(E, ring, reach, order):
    P = ring_pairs()
    if isinstance(reach, str):
        reach = wrapped_segments()[1][:RING_Q]
    want = P.rows(reach, order)
    assert want[0][-1] > 0
    forms(E, ring, P.segs, reach, order, want, (E.ALGO_RING, E.ALGO_STREAM, E.ALGO_AUTO), f"reach = {reach}")


def test_ring_form_reads_less_than_the_window(E, ring):
    P = ring_pairs()
    bounded = P.segs[np.arange(RING_Q) % 6 < 4]
    ring.set_work_counters(True)
    try:
        ring.segment_count(bounded, 0.5, E.ALGO_RING)
        work = ring.last_work()
    finally:
        ring.set_work_counters(False)
    print(f"records read, buckets opened: {work}; Q * N = {len(bounded) * len(ring)}")
    assert 0 < work[0] < len(bounded) * len(ring) // 4 and work[1] > 0


def test_ring_refuses_the_grid(E, ring):
    L = E.lib()
    segs, reach, cnt = np.float64([[1, 1, 1, 2, 2, 2]]), np.float64([1.0]), np.full(1, 77, np.uint32)
    assert L.pct_segment_count_batch(ring.handle, E.ALGO_GRID, segs.ctypes.data, reach.ctypes.data, 1, cnt.ctypes.data) == 2 and cnt[0] == 77
    assert b"without a grid" in L.pct_last_error()


@pytest.mark.parametrize("order", ORDERS)
def test_removed_rows_never_appear(E, order):
    cap = 8000
    c, m = E.Cloud(cap), Mirror(cap)
    c.ring_index(1.0, (20.0, 20.0, 20.0))
    for f in range(3):
        pts = synth.uniform_points(600 + f, 4000, 0.0, 20.0)
        c.append(pts)
        m.append(pts)
    win = m.live().copy()
    segs = segments(610, 120, 0.0, 20.0, [0.0, 0.4, 6.0], win)
    reach = np.resize(np.float64([0.0, 0.8, 3.0, INF]), len(segs))
    forms(E, c, segs, reach, order, SS.segment_search(win, segs, reach, order), (E.ALGO_RING, E.ALGO_STREAM), "before")
    gone = np.zeros(len(win), bool)
    for q in range(0, len(segs), 8):
        centre = 0.5 * (segs[q, :3] + segs[q, 3:])
        d = win.astype(np.float64) - centre
        with np.errstate(invalid="ignore"):
            inside = ((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]) <= 1.5 * 1.5
        inside &= ~gone
        assert c.ring_remove_ball(centre, 1.5) == int(inside.sum())
        gone |= inside
        win[inside] = NAN
    assert gone.sum() > 100
    want = SS.segment_search(win, segs, reach, order)
    for algo in (E.ALGO_RING, E.ALGO_STREAM):
        got = c.segment_search(segs, reach, order, algo)
        assert not np.any(gone[got[1]]), "a removed row is listed"
        same(got, want, f"(after the removal, algo {algo})")
    assert np.all(np.diff(want[0])[reach == INF] == len(win) - gone.sum())
    c.close()


def test_grown_buckets(E):
    """pillar faces on a 0.1 lattice sensed again and again: the index doubles its buckets past 32 records"""
    window, frame = 120_000, 4_000
    c, m = E.Cloud(window), Mirror(window)
    c.ring_index()
    for f in range(window // frame + 12):
        pts = S.c5_frame_clustered(f, frame)
        c.append(pts)
        m.append(pts)
    assert c.ring_info()["bucket_records"] > 32, c.ring_info()
    win = m.live()
    a = synth.uniform_points(95, 48, -1, 1).astype(np.float64) * [25.0, 25.0, 3.0] + [3.0, 0.0, 3.0]
    a[:8] = win[::14_000][:8]                               # on lattice points: exact duplicates, ties by slot
    segs = np.concatenate([a, a + unit_dirs(96, 48) * np.resize(np.float64([0.0, 0.3, 3.0]), 48)[:, None]], axis=1)
    reach = np.resize(np.float64([0.0, 0.45, 1.5]), len(segs))
    reach[11::12] = INF
    P = Pairs(win, segs)
    for order in ORDERS:
        want = P.rows(reach, order)
        assert np.all(np.diff(want[0])[:8] >= 1) and np.any(np.diff(want[0])[:8] > 100)       # a starts ON a point of the window
        forms(E, c, segs, reach, order, want, (E.ALGO_RING, E.ALGO_STREAM), "grown buckets")
    c.close()


def test_overflow_queue_entries(E):
    """2000 exact duplicates per frame in cells of 0.5 m: most of them live in the overflow queue and are listed from there, in
    ascending slot among the equals"""
    cap = 18_000
    c, m = E.Cloud(cap), Mirror(cap)
    c.ring_index(0.5, (20.0, 20.0, 20.0))
    for f in range(5):
        pts = synth.uniform_points(52 + f, 6000, 0.0, 20.0)
        pts[:2000] = np.float32([5.0, 5.0, 5.0])
        pts[2000:3000] = (np.float32([7.0, 7.0, 7.0]) + synth.uniform_points(60 + f, 1000, 0.0, 0.01)).astype(np.float32)
        c.append(pts)
        m.append(pts)
    assert c.ring_info()["overflow_entries"] > 0
    win = m.live()
    segs = np.concatenate([np.float64([[5, 5, 5, 5, 5, 5], [4, 5, 5, 6, 5, 5], [5, 4.5, 4.5, 5, 5.5, 5.5], [0, 0, 0, 10, 10, 10], [7.004, 7.004, 0, 7.004, 7.004, 20]]),
                           segments(540, 60, 0.0, 20.0, [0.0, 0.2, 4.0])])
    P = Pairs(win, segs)
    for order in ORDERS:
        for reach in (0.0, 0.02, 0.5):
            want = P.rows(reach, order)
            assert np.all(np.diff(want[0])[:4] >= 6000)
            forms(E, c, segs, reach, order, want, (E.ALGO_RING, E.ALGO_STREAM), f"overflow queue, reach = {reach}")
    c.close()


# ---- 4. pruning conditions: derived, not measured ----------------------------------------------------------------------------------

def test_grid_skip_is_in_effect(E):
    """20 000 uniform points in [0, 10)^3, h = 0.5, reach 0.5, 120 segments with a in [2, 4.5)^3: the even ones 3 m along the axes in
    turn, the odd ones 6 m along (1, 1, 1) / sqrt 3.  All coordinates lie in [2.0, 7.94], so no box touches a border cell and the
    per-cell skip applies everywhere.
      1. records read <= the points within reach + 1.8661 h + 1e-6 of the segments, summed: a record is read only from an unskipped
         cell, whose centre is within reach + h of the segment, and the record is within 0.8661 h of the centre.  On the CPU: 38 687 for
         the axis-aligned half, 61 353 for the diagonal half -- a quarter of what the diagonal boxes hold, so the test fails without
         the skip.
      2. records read > 0 and >= the 9 546 true hits.
      3. the streaming form reads exactly Q * N = 2 400 000.
    Runs are not joined (one run per cell), so the bound holds as it stands.  The search reads twice what the count reads: the fill
    is the count's walk once more, and no row of this case is empty."""
    h, reach, N = 0.5, 0.5, 20000
    pts = synth.uniform_points(1200, N, 0.0, 10.0)
    a = synth.uniform_points(1201, 120, 2.0, 4.5).astype(np.float64)
    d = np.zeros((120, 3))
    d[0::2] = 3.0 * np.eye(3)[(np.arange(0, 120, 2) // 2) % 3]
    d[1::2] = 6.0 * np.ones(3) / np.sqrt(3.0)
    segs = np.concatenate([a, a + d], axis=1)
    assert 2.0 <= segs.min() and segs.max() <= 7.94
    A, B = M.narrow(segs)
    wide = reach + 1.8661 * h + 1e-6
    bound, hits = [0, 0], [0, 0]
    for q in range(120):
        d2, _ = M.pair_d2_s(pts, A[q], B[q])
        bound[q % 2] += int((d2 <= wide * wide).sum())
        hits[q % 2] += int((d2 <= reach * reach).sum())
    assert bound == [38687, 61353] and sum(hits) == 9546
    with E.Cloud(N) as c:
        c.set_input(pts)
        c.build_grid(h)
        c.set_work_counters(True)
        read = []
        for half in (0, 1):
            cnt = c.segment_count(segs[half::2], reach, E.ALGO_GRID)
            read.append(c.last_work())
            assert int(cnt.sum()) == hits[half] and np.all(cnt > 0)
        c.segment_count(segs, reach, E.ALGO_GRID)
        count_work = c.last_work()
        got = c.segment_search(segs, reach, 1, E.ALGO_GRID)
        search_work = c.last_work()
        c.segment_count(segs, reach, E.ALGO_STREAM)
        stream_work = c.last_work()
        c.set_work_counters(False)
    print(f"records read: axis-aligned {read[0]} (bound {bound[0]}, hits {hits[0]}), diagonal {read[1]} (bound {bound[1]}, hits {hits[1]}); "
          f"count {count_work}, search {search_work}, streaming {stream_work}")
    same(got, SS.segment_search(pts, segs, reach, 1))
    for half in (0, 1):
        assert read[half][0] <= bound[half], "condition 1"
        assert read[half][0] > 0 and read[half][0] >= hits[half], "condition 2"
        assert read[half][1] > 0
    assert count_work[0] == read[0][0] + read[1][0] and count_work[0] >= 9546
    assert search_work[0] == 2 * count_work[0] and search_work[1] == 2 * count_work[1], "the fill reads what the count read"
    assert stream_work[0] == 120 * N == 2_400_000, "condition 3"


# ---- 5. the edges of the interface -------------------------------------------------------------------------------------------------

def dev_search(E, c, segs, reach, order, algo, cap=None, want_d2=True, want_s=True, stream=None):
    """the device form on `stream`: (offsets, idx, d2 or None, s or None) with the lists cut at offsets[Q], and the raw list buffers"""
    import torch
    Q = len(segs)
    c.reserve_queries(Q)
    dev = torch.device("cuda:0")
    st = stream or torch.cuda.Stream(device=dev)
    with torch.cuda.stream(st):
        tseg = torch.from_numpy(np.array(segs, np.float64)).to(dev)
        treach = torch.from_numpy(np.broadcast_to(np.asarray(reach, np.float64), (Q,)).copy()).to(dev)
        tcnt = torch.zeros(Q, dtype=torch.int32, device=dev)
        c.segment_count_device(tseg.data_ptr(), treach.data_ptr(), Q, tcnt.data_ptr(), st.cuda_stream, algo)
        total = int(tcnt.cpu().numpy().view(np.uint32).astype(np.int64).sum())
        cap = total if cap is None else cap
        toff = torch.full((Q + 1,), -1, dtype=torch.int64, device=dev)
        tidx = torch.full((max(cap, 1),), 77, dtype=torch.int32, device=dev)
        td2 = torch.full((max(cap, 1),), 7.0, dtype=torch.float64, device=dev)
        ts = torch.full((max(cap, 1),), 7.0, dtype=torch.float64, device=dev)
        c.segment_search_device(tseg.data_ptr(), treach.data_ptr(), Q, order, toff.data_ptr(), cap, tidx.data_ptr(), td2.data_ptr() if want_d2 else 0,
                                ts.data_ptr() if want_s else 0, st.cuda_stream, algo)
        off = toff.cpu().numpy()
        raw = (tidx.cpu().numpy().view(np.uint32), td2.cpu().numpy(), ts.cpu().numpy())
        cnt = tcnt.cpu().numpy().view(np.uint32)
    st.synchronize()
    assert np.array_equal(cnt.astype(np.int64), np.diff(off))
    return off, raw, total


@pytest.mark.parametrize("order", ORDERS)
def test_device_forms_on_a_callers_stream(E, gridded, ring, order):
    name, g = gridded
    _, _, gsegs, GP = grid_case(name)
    RP = ring_pairs()
    greach = np.resize(np.float64([0.0, 0.5, 6.0]), 257)
    rreach = np.resize(np.float64([0.0, 0.5, 6.0]), RING_Q)
    for c, segs, reach, P, algos in ((g, gsegs[:257], greach, GP, (E.ALGO_GRID, E.ALGO_STREAM, E.ALGO_AUTO)),
                                     (ring, RP.segs, rreach, RP, (E.ALGO_RING, E.ALGO_STREAM))):
        want = P.rows(reach, order)
        for algo in algos:
            off, (idx, d2, s), total = dev_search(E, c, segs, reach, order, algo)
            assert total == want[0][-1]
            same((off, idx[:total], d2[:total], s[:total]), want, f"(device form, algo {algo})")
            # d2 not wanted (with ORDER_DISTANCE the keys live in the cloud's own buffer), s not wanted
            off, (idx, d2, s), _ = dev_search(E, c, segs, reach, order, algo, want_d2=False, want_s=False)
            assert np.array_equal(off, want[0]) and np.array_equal(idx[:total], want[1]) and np.all(d2 == 7.0) and np.all(s == 7.0)
            off, (idx, d2, s), _ = dev_search(E, c, segs, reach, order, algo, want_d2=False)
            assert np.array_equal(idx[:total], want[1]) and np.all(d2 == 7.0) and np.array_equal(s[:total], want[3])
            # cap smaller than the total: the offsets are valid, the lists untouched
            off, (idx, d2, s), _ = dev_search(E, c, segs, reach, order, algo, cap=total - 1)
            assert np.array_equal(off, want[0]) and np.all(idx == 77) and np.all(d2 == 7.0) and np.all(s == 7.0)


def test_non_finite_segments_and_reaches(E, gridded, ring):
    for c, algos, base in ((gridded[1], (E.ALGO_GRID, E.ALGO_STREAM), np.float64([3, 3, 3, 6, 5, 2])),
                           (ring, (E.ALGO_RING, E.ALGO_STREAM), np.float64([10, 10, 10, 14, 12, 9]))):
        pts = grid_case(gridded[0])[0] if c is not ring else wrapped_case()[1]
        segs = np.tile(base, (10, 1))
        segs[1, 0] = NAN
        segs[2, 4] = INF
        segs[3, 5] = -INF
        segs[4, 3] = 1e39                                    # narrows to infinity
        segs[5, 2] = -3.5e38                                 # beyond FLT_MAX as well
        reach = np.float64([1.5, 3, 3, 3, 3, 3, NAN, -1.0, -INF, 1e200])
        for order in ORDERS:
            want = SS.segment_search(pts, segs, reach, order)
            lens = np.diff(want[0])
            assert lens[0] > 0 and lens[9] == len(pts) and np.all(lens[1:9] == 0)
            forms(E, c, segs, reach, order, want, algos)
            back = SS.segment_search(pts, segs[::-1], reach[::-1], order)
            forms(E, c, segs[::-1].copy(), reach[::-1].copy(), order, back, algos)


def test_nan_and_infinite_rows_are_never_listed(E):
    pts = synth.uniform_points(700, 500, 0.0, 10.0)
    pts[::7, 0] = NAN
    pts[3::11] = NAN
    pts[5::13, 2] = INF
    pts[6::17, 1] = -INF
    segs = segments(701, 60, 0.0, 10.0, [0.0, 0.5, 6.0])
    with E.Cloud(500) as c:
        c.ring_index(1.0, (16.0, 16.0, 16.0))
        c.append(pts)
        for reach in (0.7, INF):
            want = SS.segment_search(pts, segs, reach, 1)
            assert np.all(np.isfinite(pts[want[1]]))
            forms(E, c, segs, reach, 1, want, (E.ALGO_RING, E.ALGO_STREAM))


def test_degenerate_segments_give_the_radius_search_rows(E, gridded, ring):
    """a == b: the row of pct_radius_search_batch for the fp32 point a, d2 bit for bit (radii whose fp64 square is the reach's)"""
    q = synth.uniform_points(1230, 300, 1.0, 9.0)
    radii = np.resize(np.float32([0.0, 0.5, 0.75, 2.0]), len(q))
    segs = np.concatenate([q, q], axis=1).astype(np.float64)
    for c, scale, algos in ((gridded[1], 1.0, (E.ALGO_GRID, E.ALGO_STREAM)), (ring, 4.0, (E.ALGO_RING, E.ALGO_STREAM))):
        qq = (q * np.float32(scale)).astype(np.float32)
        ss = np.concatenate([qq, qq], axis=1).astype(np.float64)
        for order in ORDERS:
            for algo in algos:
                ro, ri, rd = c.radius_search(qq, radii, order, algo)
                so, si, sd, s = c.segment_search(ss, radii.astype(np.float64), order, algo)
                assert ro[-1] > 0 and np.array_equal(so, ro) and np.array_equal(si, ri) and np.array_equal(sd, rd) and np.all(s == 0.0)
    del segs


def test_argument_errors_refused_algos_and_result_lifetime(E):
    L = E.lib()
    p = lambda a: a.ctypes.data                                                # noqa: E731
    segs = np.float64([[0, 0, 0, 1, 1, 1], [2, 2, 2, 3, 3, 3]])
    reach = np.float64([1.0, INF])
    pts = synth.uniform_points(710, 100, 0.0, 4.0)
    with E.Cloud(100) as c:
        c.set_input(pts)
        cnt, off, total = np.full(2, 77, np.uint32), np.full(3, 77, np.int64), C.c_int64(77)
        idx, d2, s = np.full(8, 77, np.uint32), np.full(8, 7.0), np.full(8, 7.0)
        untouched = lambda: (np.all(cnt == 77) and np.all(off == 77) and total.value == 77 and np.all(idx == 77) and np.all(d2 == 7.0)      # noqa: E731
                             and np.all(s == 7.0))
        assert L.pct_segment_search_read(c.handle, 0, 0, None, None, None) == 2                                      # before any search
        # a radius search first: its result must outlive the capsule searches below
        rq, rr = np.float32([[1, 1, 1], [3, 3, 3]]), np.float32([1.0, 2.0])
        r_off, r_idx, r_d2 = c.radius_search(rq, rr, 1)
        assert r_off[-1] > 0
        assert L.pct_segment_count_batch(c.handle, E.ALGO_AUTO, None, None, 0, None) == 0                           # Q == 0
        assert L.pct_segment_count_batch_dev(c.handle, E.ALGO_AUTO, None, None, 0, None, None) == 0
        for bad in (lambda: L.pct_segment_count_batch(None, E.ALGO_AUTO, p(segs), p(reach), 2, p(cnt)),
                    lambda: L.pct_segment_count_batch(c.handle, E.ALGO_AUTO, None, p(reach), 2, p(cnt)),
                    lambda: L.pct_segment_count_batch(c.handle, E.ALGO_AUTO, p(segs), None, 2, p(cnt)),
                    lambda: L.pct_segment_count_batch(c.handle, E.ALGO_AUTO, p(segs), p(reach), 2, None),
                    lambda: L.pct_segment_count_batch(c.handle, E.ALGO_AUTO, p(segs), p(reach), -1, p(cnt)),
                    lambda: L.pct_segment_count_batch(c.handle, E.ALGO_GRID, p(segs), p(reach), 2, p(cnt)),          # no grid
                    lambda: L.pct_segment_count_batch(c.handle, E.ALGO_RING, p(segs), p(reach), 2, p(cnt)),          # no rolling-map index
                    lambda: L.pct_segment_count_batch(c.handle, E.ALGO_STREAM_EXACT, p(segs), p(reach), 2, p(cnt)),
                    lambda: L.pct_segment_count_batch(c.handle, 9, p(segs), p(reach), 2, p(cnt)),
                    lambda: L.pct_segment_count_batch_dev(c.handle, E.ALGO_GRID, p(segs), p(reach), 2, p(cnt), None),
                    lambda: L.pct_segment_count_batch_dev(c.handle, E.ALGO_AUTO, p(segs), p(reach), -1, p(cnt), None),
                    lambda: L.pct_segment_count_batch_dev(c.handle, E.ALGO_AUTO, None, p(reach), 2, p(cnt), None),
                    lambda: L.pct_segment_search_batch(None, E.ALGO_AUTO, p(segs), p(reach), 2, 1, p(off), C.byref(total)),
                    lambda: L.pct_segment_search_batch(c.handle, E.ALGO_AUTO, None, p(reach), 2, 1, p(off), C.byref(total)),
                    lambda: L.pct_segment_search_batch(c.handle, E.ALGO_AUTO, p(segs), None, 2, 1, p(off), C.byref(total)),
                    lambda: L.pct_segment_search_batch(c.handle, E.ALGO_AUTO, p(segs), p(reach), 2, 1, None, C.byref(total)),
                    lambda: L.pct_segment_search_batch(c.handle, E.ALGO_AUTO, p(segs), p(reach), 2, 1, p(off), None),
                    lambda: L.pct_segment_search_batch(c.handle, E.ALGO_AUTO, p(segs), p(reach), -1, 1, p(off), C.byref(total)),
                    lambda: L.pct_segment_search_batch(c.handle, E.ALGO_AUTO, p(segs), p(reach), 2, 2, p(off), C.byref(total)),      # unknown order
                    lambda: L.pct_segment_search_batch(c.handle, E.ALGO_GRID, p(segs), p(reach), 2, 1, p(off), C.byref(total)),
                    lambda: L.pct_segment_search_batch(c.handle, E.ALGO_RING, p(segs), p(reach), 2, 1, p(off), C.byref(total)),
                    lambda: L.pct_segment_search_batch(c.handle, E.ALGO_STREAM_EXACT, p(segs), p(reach), 2, 1, p(off), C.byref(total)),
                    lambda: L.pct_segment_search_batch(c.handle, 9, p(segs), p(reach), 2, 1, p(off), C.byref(total)),
                    lambda: L.pct_segment_search_batch_dev(c.handle, E.ALGO_AUTO, p(segs), p(reach), 2, 1, None, 8, p(idx), p(d2), p(s), None),
                    lambda: L.pct_segment_search_batch_dev(c.handle, E.ALGO_AUTO, p(segs), p(reach), 2, 1, p(off), -1, p(idx), p(d2), p(s), None),
                    lambda: L.pct_segment_search_batch_dev(c.handle, E.ALGO_AUTO, p(segs), p(reach), 2, 1, p(off), 8, None, p(d2), p(s), None),
                    lambda: L.pct_segment_search_batch_dev(c.handle, E.ALGO_AUTO, None, p(reach), 2, 1, p(off), 8, p(idx), p(d2), p(s), None),
                    lambda: L.pct_segment_search_batch_dev(c.handle, E.ALGO_GRID, p(segs), p(reach), 2, 1, p(off), 8, p(idx), p(d2), p(s), None),
                    lambda: L.pct_segment_search_batch_dev(c.handle, E.ALGO_RING, p(segs), p(reach), 2, 1, p(off), 8, p(idx), p(d2), p(s), None),
                    lambda: L.pct_segment_search_batch_dev(c.handle, E.ALGO_STREAM_EXACT, p(segs), p(reach), 2, 1, p(off), 8, p(idx), p(d2), p(s), None),
                    lambda: L.pct_segment_search_batch_dev(c.handle, 9, p(segs), p(reach), 2, 1, p(off), 8, p(idx), p(d2), p(s), None)):
            assert bad() == 2 and untouched()                                  # PCT_ERR_INVALID, nothing written
        assert L.pct_segment_search_read(c.handle, 0, 0, None, None, None) == 2                                      # still no result
        # Q == 0 is a result of its own
        assert L.pct_segment_search_batch(c.handle, E.ALGO_AUTO, None, None, 0, 1, p(off), C.byref(total)) == 0 and off[0] == 0 and total.value == 0
        assert L.pct_segment_search_read(c.handle, 0, 0, None, None, None) == 0
        assert L.pct_segment_search_read(c.handle, 0, 1, p(idx), None, None) == 2
        # a search, and reads of its ranges
        want = SS.segment_search(pts, segs, reach, 1)
        got = c.segment_search(segs, reach, 1)
        same(got, want)
        n = int(want[0][-1])
        assert n == np.diff(want[0])[0] + 100
        gi, gd, gs = c.segment_search_read(3, n - 5)
        assert np.array_equal(gi, want[1][3:n - 2]) and np.array_equal(gd, want[2][3:n - 2]) and np.array_equal(gs, want[3][3:n - 2])
        gi, gd, gs = c.segment_search_read(n, 0)
        assert len(gi) == 0
        only_s = c.segment_search_read(0, n, want_idx=False, want_d2=False)
        assert only_s[0] is None and only_s[1] is None and np.array_equal(only_s[2], want[3])
        for first, cnt_ in ((-1, 1), (0, -1), (0, n + 1), (n + 1, 0), (n, 1), (1, n)):
            assert L.pct_segment_search_read(c.handle, first, cnt_, p(idx), None, None) == 2 and np.all(idx == 77), (first, cnt_)
        # the radius search issued before all this is still readable
        ri, rd = c.radius_search_read(0, int(r_off[-1]))
        assert np.array_equal(ri, r_idx) and np.array_equal(rd, r_d2)
        # ... and a radius search does not end the capsule search's result
        c.radius_search(rq, rr, 0)
        gi, _, _ = c.segment_search_read(0, n)
        assert np.array_equal(gi, want[1])
        # with a grid PCT_ALGO_GRID is served; a build ends the result
        c.build_grid()
        assert L.pct_segment_search_read(c.handle, 0, 0, None, None, None) == 2
        same(c.segment_search(segs, reach, 0, E.ALGO_GRID), SS.segment_search(pts, segs, reach, 0))
        c.set_input(pts[:50])                                                  # an upload ends it as well
        assert L.pct_segment_search_read(c.handle, 0, 0, None, None, None) == 2


def test_empty_cloud_gives_empty_rows(E):
    L = E.lib()
    p = lambda a: a.ctypes.data                                                # noqa: E731
    segs = np.float64([[0, 0, 0, 1, 1, 1], [2, 2, 2, 3, 3, 3]])
    reach = np.float64([1.0, INF])
    for ring_on in (False, True):
        c = E.Cloud(100)
        if ring_on:
            c.ring_index(1.0, (8.0, 8.0, 8.0))
        for algo in (E.ALGO_AUTO, E.ALGO_STREAM) + ((E.ALGO_RING,) if ring_on else ()):
            cnt, off, total = np.full(2, 77, np.uint32), np.full(3, 77, np.int64), C.c_int64(77)
            assert L.pct_segment_count_batch(c.handle, algo, p(segs), p(reach), 2, p(cnt)) == 5                     # PCT_ERR_EMPTY, counts filled
            assert np.all(cnt == 0)
            assert L.pct_segment_search_batch(c.handle, algo, p(segs), p(reach), 2, 1, p(off), C.byref(total)) == 5
            assert np.all(off == 0) and total.value == 0
            assert L.pct_segment_search_read(c.handle, 0, 0, None, None, None) == 0
        assert L.pct_segment_count_batch(c.handle, E.ALGO_GRID, p(segs), p(reach), 2, p(cnt)) == 2                  # no grid: the algo comes first
        if not ring_on:
            assert L.pct_segment_count_batch(c.handle, E.ALGO_RING, p(segs), p(reach), 2, p(cnt)) == 2
        # the device form: PCT_OK and all-zero offsets
        import torch
        c.reserve_queries(2)
        dev = torch.device("cuda:0")
        tseg, treach = torch.from_numpy(segs).to(dev), torch.from_numpy(reach).to(dev)
        toff = torch.full((3,), -1, dtype=torch.int64, device=dev)
        tcnt = torch.full((2,), -1, dtype=torch.int32, device=dev)
        tidx = torch.full((4,), 77, dtype=torch.int32, device=dev)
        c.segment_count_device(tseg.data_ptr(), treach.data_ptr(), 2, tcnt.data_ptr())
        c.segment_search_device(tseg.data_ptr(), treach.data_ptr(), 2, 1, toff.data_ptr(), 4, tidx.data_ptr(), 0, 0)
        torch.cuda.synchronize()
        assert np.all(toff.cpu().numpy() == 0) and np.all(tcnt.cpu().numpy() == 0) and np.all(tidx.cpu().numpy() == 77)
        c.close()


def test_cxx_client_segment_neighbours():
    """examples/segment_neighbours.cpp: ObstacleMap::segmentNeighbours and segmentCounts on a plain, a grid-indexed, a rolling and an
    empty map, every row compared with a host loop"""
    import subprocess
    from pointcloudtraj_amd import build
    build.build_all()
    exe = os.path.join(build.LIB, "segment_neighbours")
    r = subprocess.run([exe, "120"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "121 segments" in r.stdout and " 0 rows differ" in r.stdout
    listed = int(r.stdout.split(":")[1].split()[0])
    assert listed >= 100, r.stdout
