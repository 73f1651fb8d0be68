"""The reference model of the segment queries (tests/helpers/segment_model.py) on cases whose answers are known by hand, and against
densely sampling the segment -- no GPU needed.  The contract: include/pct_engine.h, paragraph "Segment queries"."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import segment_model as M  # noqa: E402

INF, NAN = np.inf, np.nan


def brute_nn_d2(pts, q):
    """the engine's nearest-neighbour arithmetic: ((dx*dx + dy*dy) + dz*dz) on the widened operands, lowest index on ties"""
    d = np.asarray(pts, np.float32).astype(np.float64) - np.float32(q).astype(np.float64)
    d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    i = int(np.argmin(d2))
    return i, d2[i]


def test_axis_aligned_segment_beside_before_beyond():
    seg = [[0, 0, 0, 10, 0, 0]]
    for p, want_s, want_d2 in (([4, 3, 0], 0.4, 9.0),            # beside: the foot of the perpendicular
                               ([-2, 0, 1], 0.0, 5.0),           # before a: clamped to a
                               ([13, 4, 0], 1.0, 25.0),          # beyond b: clamped to b
                               ([0, 2, 0], 0.0, 4.0), ([10, 0, 2], 1.0, 4.0), ([5, 0, 0], 0.5, 0.0)):
        idx, d2, s = M.segment_nn(np.float32([p]), seg, INF)
        assert idx[0] == 0 and d2[0] == want_d2 and s[0] == want_s, p
    # three rows at once: the nearest wins and brings its own s
    idx, d2, s = M.segment_nn(np.float32([[4, 3, 0], [-2, 0, 1], [7.5, 0, -1]]), seg, INF)
    assert (idx[0], d2[0], s[0]) == (2, 1.0, 0.75)


def test_reach_is_inclusive():
    pts = np.float32([[2, 3, 4]])
    seg = [[-1, 0, 0, 6, 0, 0]]
    idx, d2, s = M.segment_nn(pts, seg, 5.0)
    assert idx[0] == 0 and d2[0] == 25.0 and s[0] == 3.0 / 7.0
    idx, d2, s = M.segment_nn(pts, seg, np.nextafter(5.0, 0.0))
    assert idx[0] == M.NO_INDEX and d2[0] == INF and np.isnan(s[0])
    assert M.segment_nn(pts, seg, INF)[0][0] == 0 and M.segment_nn(pts, seg, 1e200)[0][0] == 0      # r*r overflows: held at DBL_MAX


def test_degenerate_segment_is_the_nearest_neighbour():
    rng = np.random.default_rng(5)
    pts = (rng.random((400, 3)) * 20).astype(np.float32)
    for q in (rng.random((25, 3)) * 24 - 2):
        idx, d2, s = M.segment_nn(pts, [np.concatenate([q, q])], INF)
        i, d = brute_nn_d2(pts, q)
        assert idx[0] == i and d2[0] == d and s[0] == 0.0


def test_lattice_tie_goes_to_the_lower_index():
    pts = np.float32([[9, 9, 9], [3, 1, 0], [3, -1, 0], [3, 0, 1], [3, 0, -1], [5, 1, 0]])
    idx, d2, s = M.segment_nn(pts, [[0, 0, 0, 8, 0, 0]], INF)
    assert (idx[0], d2[0], s[0]) == (1, 1.0, 0.375)
    idx, _, _ = M.segment_nn(pts[::-1].copy(), [[0, 0, 0, 8, 0, 0]], INF)
    assert idx[0] == 0                                           # [5, 1, 0] now comes first
    assert M.segment_nn(pts, [[0, 0, 0, 8, 0, 0]], INF, index_base=1000)[0][0] == 1001


def test_nan_and_infinite_rows_never_win():
    pts = np.float32([[NAN, 0, 0], [1, NAN, 0], [INF, 0, 0], [2, -INF, 0], [NAN, NAN, NAN], [4, 7, 0]])
    for reach in (INF, 100.0):
        idx, d2, s = M.segment_nn(pts, [[0, 0, 0, 8, 0, 0]], reach)
        assert (idx[0], d2[0], s[0]) == (5, 49.0, 0.5)
    idx, d2, s = M.segment_nn(pts[:5], [[0, 0, 0, 8, 0, 0]], INF)
    assert idx[0] == M.NO_INDEX and d2[0] == INF and np.isnan(s[0])
    rad, idx, s = M.segment_inflate(pts[:5], [[0, 0, 0, 8, 0, 0]], 0.2, 3.0)
    assert rad[0] == 3.0 and idx[0] == M.NO_INDEX and np.isnan(s[0])     # rows, but none at a finite d2: not the empty-cloud rule


def test_no_candidate_cases():
    pts = np.float32([[1, 1, 1], [2, 2, 2]])
    segs = np.float64([[0, 0, 0, 3, 3, 3], [NAN, 0, 0, 3, 3, 3], [0, 0, 0, 3, INF, 3], [0, 0, 0, 1e39, 0, 0], [0, 0, 0, 3, 3, 3], [0, 0, 0, 3, 3, 3]])
    reach = np.float64([10, 10, 10, 10, NAN, -1.0])
    idx, d2, s = M.segment_nn(pts, segs, reach)
    assert idx[0] == 0 and d2[0] == 0.0
    assert np.all(idx[1:] == M.NO_INDEX) and np.all(np.isposinf(d2[1:])) and np.all(np.isnan(s[1:]))
    assert M.segment_nn(pts, segs[:1], -0.0)[0][0] == 0          # -0 is not negative: reach 0 finds what lies ON the segment
    idx, d2, s = M.segment_nn(np.zeros((0, 3), np.float32), segs, reach)
    assert np.all(idx == M.NO_INDEX) and np.all(np.isposinf(d2)) and np.all(np.isnan(s))
    rad, idx, s = M.segment_inflate(np.zeros((0, 3), np.float32), segs, 0.25, 2.0)
    assert np.all(rad == 1.75) and np.all(idx == M.NO_INDEX)


def test_cut_at_reach_equals_the_direct_statement():
    rng = np.random.default_rng(8)
    pts = (rng.random((300, 3)) * 10).astype(np.float32)
    a = rng.random((60, 3)) * 14 - 2
    segs = np.concatenate([a, a + rng.normal(size=(60, 3)) * np.resize([0.0, 0.3, 4.0], 60)[:, None]], axis=1)
    segs[7, 1] = NAN
    free = M.segment_nn(pts, segs, INF)
    for reach in (0.0, 0.4, 1.5, INF, NAN, -2.0, np.resize([0.2, 0.8, NAN, 3.0], 60)):
        want = M.segment_nn(pts, segs, reach)
        got = M.cut_at_reach(free, segs, reach)
        assert all(np.array_equal(g, w, equal_nan=True) for g, w in zip(got, want)), reach
    exact = M.cut_at_reach(free, segs, np.sqrt(free[1]))         # a reach of about the winner's own distance, either side of it
    assert np.array_equal(exact[0], M.segment_nn(pts, segs, np.sqrt(free[1]))[0])


def test_model_against_dense_sampling():
    """sampling the segment can only overestimate the distance, and by no more than the sample spacing allows: with m + 1 samples a
    point of the segment is within L / (2 m) of a sample, so  d <= d_sampled <= d + L / (2 m)  (1-Lipschitz), up to rounding"""
    rng = np.random.default_rng(21)
    pts = (rng.random((500, 3)) * 12).astype(np.float32)
    a = (rng.random((40, 3)) * 12).astype(np.float32).astype(np.float64)
    b = (a + rng.normal(size=(40, 3)) * 3).astype(np.float32).astype(np.float64)
    idx, d2, s = M.segment_nn(pts, np.concatenate([a, b], axis=1), INF)
    m = 2000
    t = np.linspace(0.0, 1.0, m + 1)
    p64 = pts.astype(np.float64)
    for q in range(40):
        samples = a[q] + t[:, None] * (b[q] - a[q])
        dd = np.sqrt(((samples[:, None, :] - p64[None, :, :]) ** 2).sum(axis=2))
        L = np.linalg.norm(b[q] - a[q])
        d = np.sqrt(d2[q])
        assert d - 1e-9 <= dd.min() <= d + L / (2 * m) + 1e-9, q
        # the winner's s is where the sampled distance to that row is smallest, within a sample
        assert abs(t[np.argmin(dd[:, idx[q]])] - s[q]) <= 1.0 / m + 1e-9, q


def test_inflate_is_the_unbounded_formula():
    pts = np.float32([[5, 2, 0], [20, 0, 0]])
    segs = [[0, 0, 0, 10, 0, 0], [0, 5, 0, 10, 5, 0], [0, 40, 0, 10, 40, 0], [5, 2, 0, 5, 2, 0]]
    rad, idx, s = M.segment_inflate(pts, segs, 0.5, 2.0)
    assert rad.tolist() == [1.5, 2.0, 2.0, -0.5] and idx.tolist() == [0, M.NO_INDEX, M.NO_INDEX, 0]
    assert s[0] == 0.5 and np.isnan(s[1]) and np.isnan(s[2]) and s[3] == 0.0
