"""The expectations of the fp64-query GPU tests, validated on the CPU before a GPU sees them.

test_gpu_q64_queries.py and test_gpu_kdtree_f64_queries.py compare the engine and the kd_* drop-in with numpy and with the CPU
restatement of the reference tree (oracle/kdtree_port.c) on the query classes of tests/helpers/q64_cases.py.  Here the restatement
itself is held against numpy on a 0.5-lattice tree of 65537 nodes, and the two conditions that make those tests meaningful are
asserted: the queries are genuine doubles, and on exact ties the reference's winner is often NOT the lowest index -- so a wrong tie
set or a wrong replay of the walk (kdtree_gpu.cpp reference_tie_winner) would show.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import q64_cases as QC  # noqa: E402

N = 65537
CLOUD_SEED, QUERY_SEED = 931, 77
DP = C.POINTER(C.c_double)


@pytest.fixture(scope="module")
def case(oracle):
    L = oracle.port_lib()
    pts = QC.cloud(CLOUD_SEED, N, lattice=True)
    t = L.okd_create(3)
    assert L.okd_insertf_batch(t, np.ascontiguousarray(pts), len(pts)) == 0
    q, cls = QC.queries(QUERY_SEED, 200)
    yield L, t, pts, q, cls
    L.okd_free(t)


def port_nearest(L, t, q):
    r = L.okd_nearest(t, np.ascontiguousarray(q, np.float64).ctypes.data_as(DP))
    assert r
    i = L.okd_res_item_id(r)
    assert L.okd_res_size(r) == 1
    L.okd_res_free(r)
    return i


def port_range(L, t, q, rng):
    r = L.okd_nearest_range(t, np.ascontiguousarray(q, np.float64).ctypes.data_as(DP), C.c_double(rng))
    out = []
    while not L.okd_res_end(r):
        out.append(L.okd_res_item_id(r))
        L.okd_res_next(r)
    assert len(out) == L.okd_res_size(r)
    L.okd_res_free(r)
    return np.asarray(out, np.int64)


def test_okd_nearest_with_double_queries_against_numpy(case):
    L, t, pts, q, cls = case
    assert QC.genuine_double(q).sum() >= 100
    lowest, d2, cnt = QC.nn_reference(pts, q)
    P = pts.astype(np.float64)
    tie_q = differs = 0
    for i in range(len(q)):
        w = port_nearest(L, t, q[i])
        assert QC.d2_rows(P[w:w + 1], q[i])[0, 0] == d2[i], f"query {i}: the port's winner is not at the minimum"
        if cls[i] in QC.TIE_CLASSES:
            tie_q += 1
            differs += int(w != lowest[i])
        if cnt[i] == 1:
            assert w == lowest[i]
    # the property the GPU tests lean on: lowest-index-wins is NOT what the reference does on these ties
    assert differs * 4 >= tie_q, f"the port's winner differs from the lowest tied index on {differs} of {tie_q} tie-class queries"
    # the x,y,z form
    for i in range(0, len(q), 17):
        r = L.okd_nearest3(t, q[i, 0], q[i, 1], q[i, 2])
        assert L.okd_res_item_id(r) == port_nearest(L, t, q[i])
        L.okd_res_free(r)


def test_okd_nearest_keeps_the_root_where_no_distance_is_finite(case):
    L, t, pts, _, _ = case
    nf = QC.non_finite_queries()
    lowest, d2, _ = QC.nn_reference(pts, nf)
    for i, qq in enumerate(nf):
        w = port_nearest(L, t, qq)
        if lowest[i] == QC.NO_INDEX:
            assert w == 0 and d2[i] == np.inf                  # kdtree.c:432-436: the first guess is never displaced
        else:
            assert QC.d2_rows(pts[w:w + 1].astype(np.float64), qq)[0, 0] == d2[i]
    assert (lowest == QC.NO_INDEX).sum() == len(nf) - 1


def test_okd_nearest_range_with_a_double_centre_against_numpy(case):
    """for range >= 0 the walk reports exactly the nodes with d2 <= range * range unless it prunes at a split plane with
    |dx| == range (kdtree.c:283, strict <): where no node has a coordinate at exactly that offset from the centre, the hit set is
    numpy's; everywhere it is a subset of it"""
    L, t, pts, q, cls = case
    P = pts.astype(np.float64)
    compared = 0
    for i in range(0, len(q), 3):
        for rng in (0.0, 0.5, 0.5 + 2.0 ** -30, 1.5) + ((np.inf,) if i % 30 == 0 else ()):     # inf lists every node: a few times
            got = port_range(L, t, q[i], rng)
            want = QC.hits_reference(pts, q[i], rng * rng).astype(np.int64)
            assert len(set(got)) == len(got) and set(got) <= set(want)
            if not np.any(np.abs(q[i][None, :] - P) == rng):
                assert np.array_equal(np.sort(got), want), f"query {i} range {rng}"
                compared += 1
    assert compared >= 130          # the classes 0 and 2 (33 of the 67 centres, x 4 finite ranges) have no coordinate at such an offset
    # the x,y,z form iterates alike
    r = L.okd_nearest_range3(t, q[0, 0], q[0, 1], q[0, 2], 1.5)
    out = []
    while not L.okd_res_end(r):
        out.append(L.okd_res_item_id(r))
        L.okd_res_next(r)
    L.okd_res_free(r)
    assert np.array_equal(out, port_range(L, t, q[0], 1.5))
