"""GPU tests of how the batch searches resolve their `algo` argument (csrc/engine.hip resolve_algo; DESIGN.md "Dispatch of the
batch searches"): the status of every (call, cloud, algo) cell, the answers of every accepted cell, and what pct_last_work reports
after each path.

Five clouds over the same 2000 points, eight point calls (host and device form of NN, radius count, k-NN and radius search) and
eight segment calls (host and device form of segment NN, sweep, capsule count and capsule search), six algo values.  The expected statuses are the literal tables below, written by hand from the rules; the expected answers are those of the
same call under PCT_ALGO_STREAM on the plain cloud, compared bit for bit.  The data has no exact distance tie among a query's ten
nearest points, and no segment a tie for its nearest row or its first blocker (both asserted on the CPU first), so the tie rule is
not what is under test here.

Two expectations of the work-counter case follow the library as it is rather than the rule "a streaming batch reports Q x n, an
index batch its own counters":
  * the radius count under PCT_ALGO_STREAM does not report its work: pct_last_work keeps the figure of the batch before;
  * the NN kernel of the rolling-map index is not instrumented and its batch leaves the device counters alone: pct_last_work
    reports those of the last instrumented batch.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from pointcloudtraj_amd import synth
from test_gpu_knn import sq_dists

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import segment_model as M  # noqa: E402
import segment_sweep_model as SW  # noqa: E402

pytestmark = pytest.mark.gpu

N, BOX = 2000, 20.0
K, RADIUS = 8, 1.5
QS = (3, 40, 1100)                  # either side of the streaming NN's Q <= 4 switch and of the 1024-query express limit
ALGOS = (0, 1, 2, 3, 4, 17)         # AUTO, STREAM, GRID, STREAM_EXACT, RING, unknown
CLOUDS = ("plain", "grid", "ring", "ring_empty", "empty")
OK, INV, EMPTY = 0, 2, 5            # PCT_OK, PCT_ERR_INVALID, PCT_ERR_EMPTY
NO_INDEX = 0xFFFFFFFF
SEG_QS = (3, 41)                    # one partial kSegTile tile; five full tiles plus one segment
SEG_LEN, REACH, SWEEP_RADIUS = 3.0, 1.5, 0.5

# columns: algo = AUTO, STREAM, GRID, STREAM_EXACT, RING, 17
NN_DEV = {
    "plain":      (OK, OK, INV, OK, INV, INV),
    "grid":       (OK, OK, OK, OK, INV, INV),
    "ring":       (OK, OK, OK, OK, OK, INV),            # GRID on a rolling map: NN takes the bucket table
    "ring_empty": (OK, OK, OK, OK, OK, OK),             # no point: padded before algo is looked at; RING passes (index asked for)
    "empty":      (OK, OK, OK, OK, INV, OK),            # ... except RING, which is checked first
}
NN_HOST = dict(NN_DEV, ring_empty=(EMPTY,) * 6, empty=(EMPTY, EMPTY, EMPTY, EMPTY, INV, EMPTY))
COUNT = {                                               # both forms: an empty cloud is PCT_OK with zero counts
    "plain":      (OK, OK, INV, INV, INV, INV),         # the count alone rejects STREAM_EXACT
    "grid":       (OK, OK, OK, INV, INV, INV),
    "ring":       (OK, OK, INV, INV, OK, INV),          # GRID without a grid, on a rolling map too
    "ring_empty": (OK, OK, OK, OK, OK, OK),
    "empty":      (OK, OK, OK, OK, INV, OK),
}
KNN_DEV = {
    "plain":      (OK, OK, INV, OK, INV, INV),
    "grid":       (OK, OK, OK, OK, INV, INV),
    "ring":       (OK, OK, INV, OK, OK, INV),
    "ring_empty": (OK, OK, OK, OK, OK, OK),
    "empty":      (OK, OK, OK, OK, INV, OK),
}
KNN_HOST = dict(KNN_DEV, ring_empty=(EMPTY,) * 6, empty=(EMPTY, EMPTY, EMPTY, EMPTY, INV, EMPTY))
SEARCH = {                                              # both forms, both orders: algo is resolved before the empty-cloud case
    "plain":      (OK, OK, INV, OK, INV, INV),
    "grid":       (OK, OK, OK, OK, INV, INV),
    "ring":       (OK, OK, INV, OK, OK, INV),
    "ring_empty": (OK, OK, INV, OK, OK, INV),
    "empty":      (OK, OK, INV, OK, INV, INV),
}
SEG_DEV = {                                             # segment NN and sweep: GRID and STREAM_EXACT are rejected before the cloud is
    "plain":      (OK, OK, INV, INV, INV, INV),         # looked at, so an empty cloud does not pass them
    "grid":       (OK, OK, INV, INV, INV, INV),
    "ring":       (OK, OK, INV, INV, OK, INV),
    "ring_empty": (OK, OK, INV, INV, OK, INV),
    "empty":      (OK, OK, INV, INV, INV, INV),
}
CAPSULE_DEV = dict(SEG_DEV, grid=(OK, OK, OK, INV, INV, INV))       # capsule count and search: the grid form exists
# the host forms of the segment family answer a cloud without a point with PCT_ERR_EMPTY, the capsule search included
SEG_HOST, CAPSULE_HOST = ({kind: tuple(EMPTY if st == OK and kind in ("ring_empty", "empty") else st for st in row)
                           for kind, row in table.items()} for table in (SEG_DEV, CAPSULE_DEV))


def points():
    return synth.uniform_points(611, N, 0.0, BOX)


def queries(Q=QS[-1]):
    return np.ascontiguousarray(synth.uniform_points(612, QS[-1], 0.5, BOX - 0.5)[:Q])


def assert_no_tie_among_the_ten_nearest():
    """the premise of every bit-exact comparison below; numpy only"""
    pts64 = points().astype(np.float64)
    for i, q in enumerate(queries()):
        near = np.sort(sq_dists(pts64, q))[:10]
        assert np.all(np.diff(near) > 0), f"query {i}: {near}"


def segments(Q=SEG_QS[-1]):
    """Q x 6, a then b: SEG_LEN long in seeded random directions, inside the box"""
    a = synth.uniform_points(613, SEG_QS[-1], 0.5 + SEG_LEN, BOX - 0.5 - SEG_LEN).astype(np.float64)
    d = np.random.default_rng(614).normal(size=(SEG_QS[-1], 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return np.ascontiguousarray(np.concatenate([a, a + SEG_LEN * d], axis=1)[:Q])


def assert_no_tie_for_the_nearest_row_or_the_first_blocker():
    """the same premise for the segment calls; numpy only"""
    pts = points()
    A, B = M.narrow(segments())
    for i in range(len(A)):
        d2, _ = M.pair_d2_s(pts, A[i], B[i])
        near = np.sort(d2[d2 <= M.reach2(REACH)])
        assert len(near) >= 2 and near[0] < near[1], f"segment {i}: {near}"
        blocker, t, _ = SW.pair_entry(pts, A[i], B[i], M.reach2(SWEEP_RADIUS))
        first = np.sort(t[blocker])
        assert len(first) < 2 or first[0] < first[1], f"sweep {i}: {first}"


@pytest.fixture(scope="module")
def E():
    assert_no_tie_among_the_ten_nearest()               # on the CPU, before any GPU call
    assert_no_tie_for_the_nearest_row_or_the_first_blocker()
    from pointcloudtraj_amd import engine
    engine.init(0)
    assert (engine.ALGO_AUTO, engine.ALGO_STREAM, engine.ALGO_GRID, engine.ALGO_STREAM_EXACT, engine.ALGO_RING) == ALGOS[:5]
    return engine


def make_cloud(E, kind):
    pts = points()
    c = E.Cloud(N)
    if kind in ("ring", "ring_empty"):
        c.ring_index()
    if kind in ("plain", "grid"):
        c.set_input(pts)
    if kind == "grid":
        c.build_grid()
    if kind == "ring":
        for f in range(0, N, 500):                      # fed by appends, not wrapped: ring slot = index
            c.append(pts[f:f + 500])
    c.reserve_queries(QS[-1])                           # the device forms need it; the host forms do it themselves
    return c


@pytest.fixture(scope="module")
def clouds(E):
    cs = {kind: make_cloud(E, kind) for kind in CLOUDS}
    assert cs["grid"].has_grid and cs["ring"].has_ring_index and not cs["ring_empty"].has_ring_index
    assert [len(cs[k]) for k in CLOUDS] == [N, N, N, 0, 0]
    yield cs
    for c in cs.values():
        c.close()


def ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def dev(a):
    import torch
    return torch.from_numpy(a).to("cuda:0")


def host(t, dtype=None):
    import torch
    torch.cuda.synchronize()
    a = t.cpu().numpy()
    return a.view(dtype) if dtype else a


# ---- the eight point calls: (status, outputs); the outputs start from values no answer holds ------------------------------------------

def nn_host(E, c, algo, q):
    idx, d2 = np.full(len(q), 7, np.uint32), np.full(len(q), -1.0)
    return E.lib().pct_nn_batch_algo(c.handle, algo, ptr(q), len(q), ptr(idx), ptr(d2)), (idx, d2)


def nn_dev(E, c, algo, q):
    tq, idx, d2 = dev(q), dev(np.full(len(q), 7, np.int32)), dev(np.full(len(q), -1.0))
    st = E.lib().pct_nn_batch_dev(c.handle, algo, tq.data_ptr(), len(q), idx.data_ptr(), d2.data_ptr(), None)
    return st, (host(idx, np.uint32), host(d2))


def count_host(E, c, algo, q):
    r, cnt = np.full(len(q), RADIUS, np.float32), np.full(len(q), 7, np.uint32)
    return E.lib().pct_radius_count_batch_algo(c.handle, algo, ptr(q), ptr(r), len(q), ptr(cnt)), (cnt,)


def count_dev(E, c, algo, q):
    tq, r, cnt = dev(q), dev(np.full(len(q), RADIUS, np.float32)), dev(np.full(len(q), 7, np.int32))
    st = E.lib().pct_radius_count_batch_dev(c.handle, algo, tq.data_ptr(), r.data_ptr(), len(q), cnt.data_ptr(), None)
    return st, (host(cnt, np.uint32),)


def knn_host(E, c, algo, q):
    idx, d2 = np.full((len(q), K), 7, np.uint32), np.full((len(q), K), -1.0)
    return E.lib().pct_knn_batch_algo(c.handle, algo, ptr(q), len(q), K, ptr(idx), ptr(d2)), (idx, d2)


def knn_dev(E, c, algo, q):
    tq, idx, d2 = dev(q), dev(np.full((len(q), K), 7, np.int32)), dev(np.full((len(q), K), -1.0))
    st = E.lib().pct_knn_batch_dev(c.handle, algo, tq.data_ptr(), len(q), K, idx.data_ptr(), d2.data_ptr(), None)
    return st, (host(idx, np.uint32), host(d2))


def search_host(order):
    def call(E, c, algo, q):
        r, offsets, total = np.full(len(q), RADIUS, np.float32), np.full(len(q) + 1, 7, np.int64), C.c_int64(7)
        st = E.lib().pct_radius_search_batch(c.handle, algo, ptr(q), ptr(r), len(q), order, ptr(offsets), C.byref(total))
        idx, d2 = np.empty(max(total.value, 0), np.uint32), np.empty(max(total.value, 0), np.float64)
        if st == OK:
            assert total.value == offsets[-1]
            assert E.lib().pct_radius_search_read(c.handle, 0, total.value, ptr(idx), ptr(d2)) == OK
        return st, (offsets, idx, d2)
    return call


def search_dev(order):
    def call(E, c, algo, q):
        cap = len(q) * N                                # every point in every row would still fit
        tq, r, offsets = dev(q), dev(np.full(len(q), RADIUS, np.float32)), dev(np.full(len(q) + 1, 7, np.int64))
        idx, d2 = dev(np.zeros(cap, np.int32)), dev(np.zeros(cap, np.float64))
        st = E.lib().pct_radius_search_batch_dev(c.handle, algo, tq.data_ptr(), r.data_ptr(), len(q), order, offsets.data_ptr(), cap,
                                                 idx.data_ptr(), d2.data_ptr(), None)
        offsets = host(offsets)
        total = int(offsets[-1]) if st == OK else 0
        return st, (offsets, host(idx, np.uint32)[:total], host(d2)[:total])
    return call


# ---- the eight segment calls, the same way ---------------------------------------------------------------------------------------

def seg_nn_host(E, c, algo, seg):
    Q = len(seg)
    r, idx, d2, s = np.full(Q, REACH), np.full(Q, 7, np.uint32), np.full(Q, -1.0), np.full(Q, -1.0)
    return E.lib().pct_segment_nn_batch(c.handle, algo, ptr(seg), ptr(r), Q, ptr(idx), ptr(d2), ptr(s)), (idx, d2, s)


def seg_nn_dev(E, c, algo, seg):
    Q = len(seg)
    ts, r, idx, d2, s = dev(seg), dev(np.full(Q, REACH)), dev(np.full(Q, 7, np.int32)), dev(np.full(Q, -1.0)), dev(np.full(Q, -1.0))
    st = E.lib().pct_segment_nn_batch_dev(c.handle, algo, ts.data_ptr(), r.data_ptr(), Q, idx.data_ptr(), d2.data_ptr(), s.data_ptr(), None)
    return st, (host(idx, np.uint32), host(d2), host(s))


def seg_sweep_host(E, c, algo, seg):
    Q = len(seg)
    r, idx, t = np.full(Q, SWEEP_RADIUS), np.full(Q, 7, np.uint32), np.full(Q, -1.0)
    return E.lib().pct_segment_sweep_batch(c.handle, algo, ptr(seg), ptr(r), Q, ptr(idx), ptr(t)), (idx, t)


def seg_sweep_dev(E, c, algo, seg):
    Q = len(seg)
    ts, r, idx, t = dev(seg), dev(np.full(Q, SWEEP_RADIUS)), dev(np.full(Q, 7, np.int32)), dev(np.full(Q, -1.0))
    st = E.lib().pct_segment_sweep_batch_dev(c.handle, algo, ts.data_ptr(), r.data_ptr(), Q, idx.data_ptr(), t.data_ptr(), None)
    return st, (host(idx, np.uint32), host(t))


def seg_count_host(E, c, algo, seg):
    r, cnt = np.full(len(seg), REACH), np.full(len(seg), 7, np.uint32)
    return E.lib().pct_segment_count_batch(c.handle, algo, ptr(seg), ptr(r), len(seg), ptr(cnt)), (cnt,)


def seg_count_dev(E, c, algo, seg):
    ts, r, cnt = dev(seg), dev(np.full(len(seg), REACH)), dev(np.full(len(seg), 7, np.int32))
    st = E.lib().pct_segment_count_batch_dev(c.handle, algo, ts.data_ptr(), r.data_ptr(), len(seg), cnt.data_ptr(), None)
    return st, (host(cnt, np.uint32),)


def seg_search_host(order):
    def call(E, c, algo, seg):
        Q = len(seg)
        r, offsets, total = np.full(Q, REACH), np.full(Q + 1, 7, np.int64), C.c_int64(7)
        st = E.lib().pct_segment_search_batch(c.handle, algo, ptr(seg), ptr(r), Q, order, ptr(offsets), C.byref(total))
        n = total.value if st in (OK, EMPTY) else 0
        idx, d2, s = np.empty(n, np.uint32), np.empty(n, np.float64), np.empty(n, np.float64)
        if st == OK:
            assert total.value == offsets[-1]
            assert E.lib().pct_segment_search_read(c.handle, 0, n, ptr(idx), ptr(d2), ptr(s)) == OK
        return st, (offsets, idx, d2, s)
    return call


def seg_search_dev(order):
    def call(E, c, algo, seg):
        Q = len(seg)
        cap = Q * N                                     # every point in every row would still fit
        ts, r, offsets = dev(seg), dev(np.full(Q, REACH)), dev(np.full(Q + 1, 7, np.int64))
        idx, d2, s = dev(np.zeros(cap, np.int32)), dev(np.zeros(cap, np.float64)), dev(np.zeros(cap, np.float64))
        st = E.lib().pct_segment_search_batch_dev(c.handle, algo, ts.data_ptr(), r.data_ptr(), Q, order, offsets.data_ptr(), cap,
                                                  idx.data_ptr(), d2.data_ptr(), s.data_ptr(), None)
        offsets = host(offsets)
        total = int(offsets[-1]) if st == OK else 0
        return st, (offsets, host(idx, np.uint32)[:total], host(d2)[:total], host(s)[:total])
    return call


def padding(name, Q):
    """what an accepted call writes when the cloud holds no point"""
    if name.startswith("seg_nn"):
        return np.full(Q, NO_INDEX, np.uint32), np.full(Q, np.inf), np.full(Q, np.nan)
    if name.startswith("seg_sweep"):
        return np.full(Q, NO_INDEX, np.uint32), np.ones(Q)                  # every sweep here is valid: free
    if name.startswith("seg_count"):
        return (np.zeros(Q, np.uint32),)
    if name.startswith("seg_search"):
        return np.zeros(Q + 1, np.int64), np.zeros(0, np.uint32), np.zeros(0, np.float64), np.zeros(0, np.float64)
    if name.startswith("nn"):
        return np.full(Q, NO_INDEX, np.uint32), np.full(Q, np.inf)
    if name.startswith("knn"):
        return np.full((Q, K), NO_INDEX, np.uint32), np.full((Q, K), np.inf)
    if name.startswith("count"):
        return (np.zeros(Q, np.uint32),)
    return np.zeros(Q + 1, np.int64), np.zeros(0, np.uint32), np.zeros(0, np.float64)


CALLS = {
    "nn_host_q3": (nn_host, NN_HOST, 3), "nn_host_q40": (nn_host, NN_HOST, 40), "nn_host_q1100": (nn_host, NN_HOST, 1100),
    "nn_dev": (nn_dev, NN_DEV, 40),
    "count_host": (count_host, COUNT, 40), "count_dev": (count_dev, COUNT, 40),
    "knn_host": (knn_host, KNN_HOST, 40), "knn_dev": (knn_dev, KNN_DEV, 40),
    "search_host_by_index": (search_host(0), SEARCH, 40), "search_host_by_distance": (search_host(1), SEARCH, 40),
    "search_dev_by_index": (search_dev(0), SEARCH, 40), "search_dev_by_distance": (search_dev(1), SEARCH, 40),
}
SEG_CALLS = {
    "seg_nn_host": (seg_nn_host, SEG_HOST), "seg_nn_dev": (seg_nn_dev, SEG_DEV),
    "seg_sweep_host": (seg_sweep_host, SEG_HOST), "seg_sweep_dev": (seg_sweep_dev, SEG_DEV),
    "seg_count_host": (seg_count_host, CAPSULE_HOST), "seg_count_dev": (seg_count_dev, CAPSULE_DEV),
    "seg_search_host_by_index": (seg_search_host(0), CAPSULE_HOST), "seg_search_host_by_distance": (seg_search_host(1), CAPSULE_HOST),
    "seg_search_dev_by_index": (seg_search_dev(0), CAPSULE_DEV), "seg_search_dev_by_distance": (seg_search_dev(1), CAPSULE_DEV),
}
CALLS.update({f"{name}_q{Q}": (call, table, Q) for name, (call, table) in SEG_CALLS.items() for Q in SEG_QS})


def same(got, want):
    return len(got) == len(want) and all(g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes() for g, w in zip(got, want))


@pytest.mark.parametrize("name", list(CALLS))
def test_status_and_answers(E, clouds, name):
    call, table, Q = CALLS[name]
    q = segments(Q) if name.startswith("seg_") else queries(Q)
    st, want = call(E, clouds["plain"], E.ALGO_STREAM, q)
    assert st == OK
    if name.startswith("seg_nn"):                       # the segment yardsticks against their numpy models, likewise
        assert same(want, M.segment_nn(points(), q, REACH))
    if name.startswith("seg_sweep"):
        assert same(want, SW.segment_sweep(points(), q, SWEEP_RADIUS))
    if name.startswith(("nn", "knn")):                  # the yardstick itself against numpy: without ties a plain sort decides
        pts64 = points().astype(np.float64)
        k = K if name.startswith("knn") else 1
        for i in range(Q):
            s = sq_dists(pts64, q[i])
            order = np.argsort(s, kind="stable")[:k]
            assert np.array_equal(want[0].reshape(Q, k)[i], order) and np.array_equal(want[1].reshape(Q, k)[i], s[order]), f"query {i}"
    bad = []                                            # every cell is looked at before the test fails
    for kind in CLOUDS:
        for algo, expect in zip(ALGOS, table[kind]):
            st, got = call(E, clouds[kind], algo, q)
            if st != expect:
                bad.append(f"{kind} cloud, algo {algo}: status {st}, expected {expect} ({E.lib().pct_last_error().decode()})")
            elif st in (OK, EMPTY) and not same(got, want if len(clouds[kind]) else padding(name, Q)):     # PCT_ERR_EMPTY fills the outputs too
                bad.append(f"{kind} cloud, algo {algo}: answers differ")
    assert not bad, f"{name}: " + "; ".join(bad)


def test_work_counters_per_path(E):
    """pct_last_work after each path: the index paths count on the device, from zero for every batch; the streaming NN and k-NN
    report Q x n from the host.  The segment family keeps the rule without exception: segment NN, capsule count and capsule search count
    on the device on either index (fewer records than Q x n) and report Q x n from their streaming forms"""
    import torch
    Q = 40
    q = queries(Q)
    ops = {"nn": nn_dev, "count": count_dev, "knn": knn_dev}
    for kind, algo in (("grid", E.ALGO_GRID), ("ring", E.ALGO_RING)):
        c = make_cloud(E, kind)
        c.set_work_counters(True)
        for op in ("count", "knn", "nn"):               # NN last: on the rolling map it shows the k-NN batch's figure (module docstring)
            figures = []
            for _ in range(2):
                assert ops[op](E, c, algo, q)[0] == OK
                torch.cuda.synchronize()
                figures.append(c.last_work())
            print(f"{kind} {op}: last_work {figures}")
            assert figures[0][0] > 0 and figures[0] == figures[1], f"{op} under algo {algo}: {figures}"
        for op in ("nn", "knn"):
            assert ops[op](E, c, E.ALGO_STREAM, q)[0] == OK
            torch.cuda.synchronize()
            print(f"{kind} {op} stream: last_work {c.last_work()}")
            assert c.last_work() == (Q * N, 0), f"{op} under STREAM"
        assert ops["count"](E, c, algo, q)[0] == OK
        torch.cuda.synchronize()
        counted = c.last_work()
        assert counted[0] > 0
        assert ops["count"](E, c, E.ALGO_STREAM, q)[0] == OK
        torch.cuda.synchronize()
        print(f"{kind} count stream: last_work {c.last_work()} after {counted}")
        assert c.last_work() == counted, "the streaming count leaves the figure of the batch before"
        # the segment family: its index paths count on the device too, and every streaming form reports Q x n, the count included
        seg = segments()
        seg_ops = {"seg_nn": seg_nn_dev, "seg_count": seg_count_dev, "seg_search": seg_search_dev(1)}
        for op in (("seg_search",) if kind == "grid" else tuple(seg_ops)):      # the grid form exists for the capsule search alone
            figures = []
            for _ in range(2):
                assert seg_ops[op](E, c, algo, seg)[0] == OK
                torch.cuda.synchronize()
                figures.append(c.last_work())
            print(f"{kind} {op}: last_work {figures}")
            assert 0 < figures[0][0] < len(seg) * N and figures[0][1] > 0 and figures[0] == figures[1], f"{op} under algo {algo}: {figures}"
            assert seg_ops[op](E, c, E.ALGO_STREAM, seg)[0] == OK
            torch.cuda.synchronize()
            print(f"{kind} {op} stream: last_work {c.last_work()}")
            assert c.last_work() == (len(seg) * N, 0), f"{op} under STREAM"
        c.close()
