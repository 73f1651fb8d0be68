"""The reference model of the segment sweeps (tests/helpers/segment_sweep_model.py) on cases whose answers are known by hand and
on the properties the contract states -- no GPU needed.  The contract: include/pct_engine.h, paragraph "Segment sweeps"."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import segment_model as M  # noqa: E402
import segment_sweep_model as W  # noqa: E402

INF, NAN = np.inf, np.nan
NO_INDEX = W.NO_INDEX
ON_X = [[0, 0, 0, 10, 0, 0]]


def test_hand_pinned_rows():
    for p, want in (([5, 0, 0], 0.4), ([5, 1, 0], 0.5), ([11, 0, 0], 1.0), ([-0.5, 0, 0], 0.0)):      # (5, 1, 0): tangent, disc = 0; (11, 0, 0): the end cap
        idx, t = W.segment_sweep(np.float32([p]), ON_X, 1.0)
        assert idx[0] == 0 and t[0] == want, p
    idx, t = W.segment_sweep(np.float32([[11.5, 0, 0]]), ON_X, 1.0)                                      # not a blocker
    assert idx[0] == NO_INDEX and t[0] == 1.0
    # all five at once: the one in contact at the start wins
    idx, t = W.segment_sweep(np.float32([[5, 0, 0], [5, 1, 0], [11, 0, 0], [-0.5, 0, 0], [11.5, 0, 0]]), ON_X, 1.0)
    assert (idx[0], t[0]) == (3, 0.0)
    idx, t = W.segment_sweep(np.float32([[5, 1, 0], [5, 0, 0], [11, 0, 0]]), ON_X, 1.0, index_base=100)
    assert (idx[0], t[0]) == (101, 0.4)


def test_the_stopping_point_is_not_the_nearest_point():
    pts = np.float32([[8, 0, 0], [3, 0.9, 0]])                     # row 0 lies ON the segment, row 1 is met first
    idx, t = W.segment_sweep(pts, ON_X, 1.0)
    assert idx[0] == 1 and 0.2 < t[0] < 0.3
    assert M.segment_nn(pts, ON_X, 1.0)[0][0] == 0


def test_ties_go_to_the_lower_index():
    pts = np.float32([[9, 9, 9], [5, 1, 0], [5, -1, 0], [5, 0, 1], [5, 0, -1]])
    idx, t = W.segment_sweep(pts, ON_X, 1.0)
    assert (idx[0], t[0]) == (1, 0.5)
    idx, t = W.segment_sweep(pts[::-1].copy(), ON_X, 1.0)
    assert (idx[0], t[0]) == (0, 0.5)
    # several rows in contact at the start all have t = 0
    idx, t = W.segment_sweep(np.float32([[5, 0, 0], [0.5, 0, 0], [0, 0.25, 0]]), ON_X, 1.0)
    assert (idx[0], t[0]) == (1, 0.0)


def random_case(seed, n=400, q=120):
    rng = np.random.default_rng(seed)
    pts = (rng.random((n, 3)) * 10).astype(np.float32)
    a = rng.random((q, 3)) * 12 - 1
    d = rng.normal(size=(q, 3))
    d /= np.linalg.norm(d, axis=1)[:, None]
    d[::3] = np.eye(3)[np.arange(0, q, 3) % 3]
    a[::7] = pts[(np.arange(0, q, 7) * 5) % n]
    segs = np.concatenate([a, a + d * np.resize([0.0, 0.05, 3.0, 17.0], q)[:, None]], axis=1)
    return pts, segs


def test_entry_lies_between_the_start_and_the_closest_approach():
    pts, segs = random_case(3)
    a, b = M.narrow(segs)
    seen = 0
    for q in range(len(segs)):
        for r in (0.0, 0.3, 1.5, INF):
            blocker, t, s = W.pair_entry(pts, a[q], b[q], M.reach2(r))
            assert np.all((t[blocker] >= 0.0) & (t[blocker] <= s[blocker])), (q, r)
            seen += int(blocker.sum())
    assert seen > 1000


def test_blocked_is_has_a_candidate_and_zero_is_within_r_of_a():
    pts, segs = random_case(4)
    a, _ = M.narrow(segs)
    p = pts.astype(np.float64)
    for r in (0.0, 0.3, 1.5, INF, np.resize([0.2, 0.8, 3.0], len(segs))):
        idx, t = W.segment_sweep(pts, segs, r)
        nn = M.segment_nn(pts, segs, r)[0]
        assert np.array_equal(idx != NO_INDEX, nn != NO_INDEX)
        assert np.all(t[idx == NO_INDEX] == 1.0)
        rr = np.broadcast_to(np.float64(r), (len(segs),))
        for q in range(len(segs)):
            w = p - a[q]
            ww = (w[:, 0] * w[:, 0] + w[:, 1] * w[:, 1]) + w[:, 2] * w[:, 2]
            touching = bool(np.any(ww <= M.reach2(rr[q])))
            assert (idx[q] != NO_INDEX and t[q] == 0.0) == touching, (q, rr[q])
    idx, t = W.segment_sweep(pts, segs, 0.3)
    assert np.any(idx == NO_INDEX) and np.any(t == 0.0) and np.any((t > 0) & (t < 1))


def test_degenerate_sweep():
    pts = np.float32([[1, 1, 1], [4, 1, 1], [1, 1.5, 1]])
    at = [[1, 1, 1.25, 1, 1, 1.25]]
    assert [v[0] for v in W.segment_sweep(pts, at, 0.25)] == [0, 0.0]
    assert [v[0] for v in W.segment_sweep(pts, at, 0.2)] == [NO_INDEX, 1.0]
    assert [v[0] for v in W.segment_sweep(pts[1:], at, 0.6)] == [1, 0.0]         # index of the first within r
    assert [v[0] for v in W.segment_sweep(pts, at, INF)] == [0, 0.0]


def test_radius_edges():
    pts = np.float32([[5, 0, 0], [7, 2, 0]])
    assert [v[0] for v in W.segment_sweep(pts, ON_X, 0.0)] == [0, 0.5]           # r = 0: what lies ON the segment, where it lies
    assert [v[0] for v in W.segment_sweep(pts, ON_X, -0.0)] == [0, 0.5]          # -0 is not negative
    assert [v[0] for v in W.segment_sweep(pts[1:], ON_X, 0.0)] == [NO_INDEX, 1.0]
    assert [v[0] for v in W.segment_sweep(pts, ON_X, INF)] == [0, 0.0]           # every finite row is in contact at the start
    assert [v[0] for v in W.segment_sweep(pts, ON_X, 1e200)] == [0, 0.0]         # r*r overflows: held at DBL_MAX
    for r in (NAN, -1.0, -INF):
        idx, t = W.segment_sweep(pts, ON_X, r)
        assert idx[0] == NO_INDEX and np.isnan(t[0]), r


def test_non_finite_endpoints_rows_and_the_empty_cloud():
    pts = np.float32([[1, 1, 1], [2, 2, 2]])
    segs = np.float64([[0, 0, 0, 3, 3, 3], [NAN, 0, 0, 3, 3, 3], [0, 0, 0, 3, INF, 3], [0, 0, 0, 1e39, 0, 0], [0, -3.5e38, 0, 3, 3, 3]])
    idx, t = W.segment_sweep(pts, segs, 0.5)
    assert idx[0] == 0 and 0.0 < t[0] < 1.0 / 3.0
    assert np.all(idx[1:] == NO_INDEX) and np.all(np.isnan(t[1:]))               # invalid, never "free"
    rows = np.float32([[NAN, 0, 0], [1, NAN, 0], [INF, 0, 0], [2, -INF, 0], [NAN, NAN, NAN], [4, 0.5, 0]])
    for r in (1.0, INF):
        idx, t = W.segment_sweep(rows, ON_X, r)
        assert idx[0] == 5, r
    idx, t = W.segment_sweep(rows[:5], ON_X, INF)
    assert idx[0] == NO_INDEX and t[0] == 1.0
    radius = np.float64([0.5, 0.5, 0.5, 0.5, NAN])
    idx, t = W.segment_sweep(np.zeros((0, 3), np.float32), np.tile(segs[0], (5, 1)), radius)
    assert np.all(idx == NO_INDEX) and np.all(t[:4] == 1.0) and np.isnan(t[4])
    idx, t = W.segment_sweep(np.zeros((0, 3), np.float32), segs, 0.5)
    assert np.all(idx == NO_INDEX) and t[0] == 1.0 and np.all(np.isnan(t[1:]))


def test_wrapped_window_has_every_outcome():
    """the first 258 segments of the GPU tests' wrapped case: free, start-in-contact and 0 < t < 1 sweeps under both radii, and at
    r = 0.5 a winner that is not the nearest point (measured: 56 / 62 / 140 sweeps at 0.5, the winner differs in 118 of 202)"""
    from test_gpu_ring_search import wrapped_case
    from test_gpu_segments import wrapped_segments
    _, win, _, _ = wrapped_case()
    segs = wrapped_segments()[0][:258]
    for r in (0.25, 0.5):
        idx, t = W.segment_sweep(win, segs, r)
        nn = M.segment_nn(win, segs, r)[0]
        free, touching, between = idx == NO_INDEX, (idx != NO_INDEX) & (t == 0.0), (t > 0.0) & (t < 1.0)
        print(f"r = {r}: free {free.sum()}, in contact at the start {touching.sum()}, 0 < t < 1 {between.sum()}, "
              f"winner is not the nearest point {np.sum(idx[~free] != nn[~free])} of {np.sum(~free)}")
        assert free.any() and touching.any() and between.any(), r
        assert np.array_equal(free, nn == NO_INDEX)
        if r == 0.5:
            assert np.any(idx[~free] != nn[~free])
    # the boxed route the GPU tests take for their large batches is the model itself
    radius = np.resize(np.float64([0.0, 0.25, 0.5, 6.0, 500.0, INF, NAN]), len(segs))
    plain, boxed = W.segment_sweep(win, segs, radius, 7), W.segment_sweep_boxed(win, segs, radius, 7)
    assert np.array_equal(plain[0], boxed[0]) and np.array_equal(plain[1], boxed[1], equal_nan=True)
