"""GPU tests of the segment sweeps (pct_segment_sweep_batch*; kernels in csrc/segment.hpp): the streaming form and the rolling-map form
against the numpy restatement of the contract (tests/helpers/segment_sweep_model.py) and against each other.

Every comparison is bit-exact -- indices and t -- and covers every sweep of every batch.  Index of a point = its row in the uploaded
cloud, or its ring slot = its row in the host mirror of the ring."""
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
import segment_sweep_model as W  # noqa: E402

pytestmark = pytest.mark.gpu

INF, NAN = np.inf, np.nan
NO_INDEX = W.NO_INDEX
BATCHES = [1, 257, 5000]
RADII = [0.0, 0.25, 0.5, 6.0, 500.0, INF]       # 500: beyond the table's span


@pytest.fixture(scope="module")
def E():
    from pointcloudtraj_amd import engine
    engine.init(0)
    return engine


def same(got, want, what=""):
    gi, gt = got
    wi, wt = want
    assert gi.dtype == np.uint32 and gt.dtype == np.float64
    assert np.array_equal(gt, wt, equal_nan=True), f"t differs {what}: first at {np.flatnonzero(~((gt == wt) | (np.isnan(gt) & np.isnan(wt))))[:5]}"
    assert np.array_equal(gi, wi), f"idx differs {what}: first at {np.flatnonzero(gi != wi)[:5]}"


def both_forms(E, c, segs, radius, want, what=""):
    same(c.segment_sweep(segs, radius, E.ALGO_RING), want, f"(ring {what})")
    same(c.segment_sweep(segs, radius, E.ALGO_STREAM), want, f"(stream {what})")


def outcomes(want):
    """(free, in contact at the start, stopped on the way) counts of a model answer"""
    idx, t = want
    return int(np.sum((idx == NO_INDEX) & (t == 1.0))), int(np.sum((idx != NO_INDEX) & (t == 0.0))), int(np.sum((t > 0.0) & (t < 1.0)))


# ---- 1. the streaming form ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 1000])
def test_streaming_form_against_the_model(E, n):
    pts = synth.uniform_points(300 + n, n, 0.0, 10.0)
    with E.Cloud(n) as c:
        c.set_input(pts)
        for Q in (1, 257):
            segs = segments(310 + Q, Q, -1.0, 11.0, [0.0, 0.05, 3.0, 17.4] if Q > 1 else [3.0], pts)
            for r in (0.0, 0.25, 1.5, INF):
                want = W.segment_sweep(pts, segs, r)
                same(c.segment_sweep(segs, r, E.ALGO_STREAM), want, f"(n = {n}, Q = {Q}, r = {r})")
                same(c.segment_sweep(segs, r), want, f"(auto, n = {n}, Q = {Q}, r = {r})")               # no index: AUTO streams
            assert np.any(W.segment_sweep(pts, segs, 0.0)[0] != NO_INDEX), "the case has nothing ON a segment"


# ---- 2. the ring form on the wrapped window ----------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def wrapped_want():
    """the model on the 5000 wrapped segments, radius = RADII[i % 6]"""
    _, win, _, _ = wrapped_case()
    segs = wrapped_segments()[0]
    radius = np.resize(np.float64(RADII), len(segs))
    return radius, W.segment_sweep_boxed(win, segs, radius)


@pytest.fixture(scope="module")
def wrapped(E):
    frames, win, _, _ = wrapped_case()
    c = E.Cloud(len(win))
    c.ring_index(0.0, (40.0, 40.0, 40.0))
    for f in frames:
        c.append(f)
    assert len(c) == len(win) and c.has_ring_index
    yield c
    c.close()


def test_wrapped_ring_equals_stream_equals_model(E, wrapped):
    segs = wrapped_segments()[0]
    radius, want = wrapped_want()
    assert all(o > 0 for o in outcomes(want)), outcomes(want)
    for Q in BATCHES:
        cut = tuple(w[:Q] for w in want)
        both_forms(E, wrapped, segs[:Q], radius[:Q], cut, f"Q = {Q}")
    same(wrapped.segment_sweep(segs[:257], radius[:257]), tuple(w[:257] for w in want), "(auto)")      # AUTO takes the ring form
    wrapped.set_work_counters(True)
    try:
        wrapped.segment_sweep(segs[:257], radius[:257])
        assert wrapped.last_work()[0] < 257 * len(wrapped)
    finally:
        wrapped.set_work_counters(False)
    again = wrapped.segment_sweep(segs, radius, E.ALGO_RING)
    first = wrapped.segment_sweep(segs, radius, E.ALGO_RING)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(again, first)) and np.array_equal(again[0], want[0])


@pytest.mark.parametrize("r", RADII)
def test_wrapped_every_kind_under_every_radius(E, wrapped, r):
    """the batch above gives kind i % 6 the radius i % 6; here every kind meets every radius (43 of each kind)"""
    _, win, _, _ = wrapped_case()
    segs = wrapped_segments()[0][:258]
    both_forms(E, wrapped, segs, r, W.segment_sweep(win, segs, r), f"r = {r}")


# ---- 3. the stop rule under attack: a rolling map with cells of exactly 1.0 over the 40 m window -----------------------------------

ATTACK_R = 0.75
EPS = 2.0 ** -20


def attack_case():
    """Ten bundles of sweeps, one per direction (both ways along every axis, four diagonals with different dominant axes), each around
    its own centre.  Per bundle three parallel lines of 12 m:
      0: rows placed at r (1 - 2^-20), r and r (1 + 2^-20) from the line at s = 0, 0.3 and 1, each on its own side of the line.  The
         rows are fp32 at coordinates of 10 to 30, whose ulp (2e-6) is coarser than r 2^-20 (7e-7): what they hold is "r, give or
         take the narrowing".  The 2^-20 distinction is carried by the RADIUS: the test sweeps with r, r (1 - 2^-20) and
         r (1 + 2^-20) in fp64, so every row is met just inside, at and just outside tangency by one of them;
      1: the closest legal pair -- a row straight ahead at 5 m against a row r to the side and a cell further on;
      2: one row just inside the end cap beyond b: a blocker in the last layer only.
    Sweeps: along each line from several starts, forwards and backwards, so that every row is somebody's first contact."""
    dirs = np.float64([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1], [1, 1, 1], [-2, 1, 0.5], [0.3, -1, 2], [1, -0.2, -3]])
    centres = np.float64([[10, 10, 10], [30, 10, 10], [10, 30, 10], [30, 30, 10], [10, 10, 30], [30, 10, 30], [10, 30, 30], [30, 30, 30], [20, 20, 12], [20, 20, 28]])
    rows, sweeps = [], []
    r, L = ATTACK_R, 12.0
    for d, ctr in zip(dirs, centres):
        d = d / np.linalg.norm(d)
        n1 = np.cross(d, [0.0, 0.0, 1.0] if abs(d[2]) < 0.9 else [1.0, 0.0, 0.0])
        n1 /= np.linalg.norm(n1)
        n2 = np.cross(d, n1)
        lines = [ctr - 0.5 * L * d + off * n2 for off in (0.0, 3.5, -3.5)]
        a = lines[0]
        for j, s in enumerate((0.0, 0.3, 1.0)):
            for m, f in enumerate((1.0 - EPS, 1.0, 1.0 + EPS)):
                ang = 2.0 * np.pi * (3 * j + m) / 9.0
                rows.append(a + s * L * d + r * f * (np.cos(ang) * n1 + np.sin(ang) * n2))
        for start, stop in ((0.0, 1.0), (0.1, 1.0), (0.4, 1.2), (0.0, 0.95), (-0.5, 1.5), (0.29, 0.31)):
            sweeps.append(np.concatenate([a + start * L * d, a + stop * L * d]))
            sweeps.append(np.concatenate([a + stop * L * d, a + start * L * d]))
        a = lines[1]
        rows.append(a + 5.0 * d)
        rows.append(a + 6.0 * d + r * n1)
        sweeps.append(np.concatenate([a, a + L * d]))
        sweeps.append(np.concatenate([a + L * d, a]))
        a = lines[2]
        rows.append(a + (L + r * (1.0 - 2.0 ** -10)) * d)
        sweeps.append(np.concatenate([a, a + L * d]))
        sweeps.append(np.concatenate([a + 0.5 * L * d, a + L * d]))
    # a sweep whose r + |e| exceeds the early stop's cap of 2^20 cells, along an axis and askew
    sweeps.append(np.float64([20.0 - 6e5, 10, 10, 20.0 + 6e5, 10, 10]))
    sweeps.append(np.float64([10.0 - 6e5, 10 - 5e5, 10, 10.0 + 6e5, 10 + 5e5, 10]))
    return np.float32(rows), np.float64(sweeps)


def test_stop_rule_under_attack(E):
    rows, sweeps = attack_case()
    pts = np.concatenate([rows, synth.uniform_points(810, 300, 0.0, 40.0)])        # a thin background
    with E.Cloud(len(pts)) as c:
        c.ring_index(1.0, (40.0, 40.0, 40.0))
        c.append(pts)
        info = c.ring_info()
        assert info["cell_size"] == 1.0 and all(d >= 40 for d in info["dims"]), info
        crafted = 0
        for r in (ATTACK_R, ATTACK_R * (1.0 - EPS), ATTACK_R * (1.0 + EPS)):
            want = W.segment_sweep(pts, sweeps, r)
            both_forms(E, c, sweeps, r, want, f"r = {r}")
            crafted += int(np.sum(want[0] < len(rows)))
            if r == ATTACK_R:
                hit = want[0][want[0] != NO_INDEX]
                assert len(set(hit[hit < len(rows)].tolist())) >= 60, "too few of the crafted rows are anybody's first contact"
                assert np.sum((want[1] > 0.9) & (want[1] < 1.0) & (want[0] < len(rows))) >= 10, "no blocker in the last layers"
                assert outcomes(want)[1] >= 20 and outcomes(want)[2] >= 100, outcomes(want)
        assert crafted >= 400


def test_overflow_queue_and_duplicates(E):
    """2000 exact duplicates per frame in cells of 0.5 m: most of them live in the overflow queue; the sphere stops at the lowest
    slot among the equals, wherever that one is filed (test_blocker_in_the_overflow_queue_only pins the queue-only case)"""
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
    segs = np.concatenate([np.float64([[5, 5, 5, 5, 5, 5], [4, 5, 5, 6, 5, 5], [5, 4.5, 4.5, 5, 5.5, 5.5], [0, 0, 0, 10, 10, 10], [7.004, 7.004, 0, 7.004, 7.004, 20],
                                       [5, 5, 4.9, 5, 5, 9]]),
                           segments(540, 60, 0.0, 20.0, [0.0, 0.2, 4.0])])
    dup = np.flatnonzero(np.all(win == np.float32([5, 5, 5]), axis=1))
    assert len(dup) == 6000
    for r in (0.0, 0.02, 0.05, 0.5):
        want = W.segment_sweep(win, segs, r)
        assert want[1][0] == 0.0 and (r > 0.05 or np.all(want[0][:3] == dup[0]))
        both_forms(E, c, segs, r, want, f"r = {r}")
    assert W.segment_sweep(win, segs, 0.05)[0][5] == dup[0]          # nothing else within 5 cm of that line
    c.close()


def test_blocker_in_the_overflow_queue_only(E):
    """2000 copies of one point arrive first and fill their cell's bucket for good (a bucket grows to 256 records at the most, and a
    refile keeps slot order), so the row of the same cell that arrives after them is filed in the overflow queue.  A sweep that passes
    that row within r and the copies beyond r can be stopped by nothing else: the cloud holds no other point."""
    with E.Cloud(4096) as c:
        c.ring_index(0.5, (20.0, 20.0, 20.0))
        c.append(np.tile(np.float32([5.0, 5.0, 5.0]), (2000, 1)))
        late = np.float32([[5.1, 5.1, 5.3]])                   # the cell [5, 5.5)^3 of the copies
        c.append(late)
        info = c.ring_info()
        assert info["cell_size"] == 0.5 and info["bucket_records"] <= 256 < 2000, info
        where, _, _, _, filed_id, _ = c.debug_ring_slot(2000)
        assert where & 0x80000000 and filed_id == 2000, "the late row is not filed in the overflow queue"       # kRingInOvf
        pts = np.concatenate([np.tile(np.float32([5.0, 5.0, 5.0]), (2000, 1)), late])
        segs = np.float64([[2, 5.1, 5.45, 9, 5.1, 5.45], [9, 5.1, 5.45, 2, 5.1, 5.45], [5.25, 5.1, 2, 5.25, 5.1, 9], [2, 5.1, 5.45, 4, 5.1, 5.45]])
        want = W.segment_sweep(pts, segs, 0.2)
        assert want[0].tolist() == [2000, 2000, 2000, NO_INDEX] and np.all((want[1][:3] > 0.3) & (want[1][:3] < 0.6))
        both_forms(E, c, segs, 0.2, want)
        same(c.segment_sweep(segs, 0.2), want, "(auto)")


def test_small_table_folding(E):
    """8 positions per axis under a window that drifts away: every box folds, the whole box is walked"""
    cap = 4000
    c, m = E.Cloud(cap), Mirror(cap)
    c.ring_index(2.0, (8.0, 8.0, 8.0))
    assert all(d <= 8 for d in c.ring_info()["dims"]), c.ring_info()
    for f in range(9):
        drift = np.float32([17.0 * f, -3.0 * f, 0.5 * f])
        pts = (synth.uniform_points(120, 1000, 0.0, 10.0, offset=f * 1000) + drift).astype(np.float32)
        c.append(pts)
        m.append(pts)
        if f not in (2, 8):
            continue
        win = m.live()
        near = segments(500 + f, 150, -1.0, 11.0, [0.0, 0.3, 1.9, 5.0, 12.0, 40.0]) + np.tile(drift.astype(np.float64), 2)
        far = segments(520 + f, 30, -300.0, 300.0, [0.0, 3.0, 100.0])
        segs = np.concatenate([near, far])
        for r in (0.0, 0.3, 1.0, 9.0, 1e6, np.resize(np.float64([0.3, 1.0, 3.0, 9.0, 1e6]), len(segs))):
            both_forms(E, c, segs, r, W.segment_sweep(win, segs, r), f"frame {f}")
    c.close()


def test_grown_buckets(E):
    """pillar faces on a 0.1 lattice sensed again and again: the index doubles its buckets, and the blockers sit in fat buckets"""
    window, frame = 120_000, 4_000
    c, m = E.Cloud(window), Mirror(window)
    c.ring_index()
    for f in range(window // frame + 12):
        pts = S.c5_frame_clustered(f, frame)
        c.append(pts)
        m.append(pts)
    assert c.ring_info()["bucket_records"] > 32, c.ring_info()
    win = m.live()
    a = synth.uniform_points(95, 96, -1, 1).astype(np.float64) * [25.0, 25.0, 3.0] + [3.0, 0.0, 3.0]
    a[:8] = win[::14_000][:8]                               # on lattice points: exact duplicates, ties by slot
    segs = np.concatenate([a, a + unit_dirs(96, 96) * np.resize(np.float64([0.0, 0.3, 3.0, 9.0]), 96)[:, None]], axis=1)
    for r in (0.0, 0.25, 0.45, 1.5):
        want = W.segment_sweep_boxed(win, segs, r)
        if r == 0.45:
            assert outcomes(want)[2] >= 10, outcomes(want)
        both_forms(E, c, segs, r, want, f"r = {r}")
    c.close()


# ---- 4. after mutations ------------------------------------------------------------------------------------------------------------

def test_after_remove_compact_and_evicting_append(E):
    cap = 8000
    c, m = E.Cloud(cap), Mirror(cap)
    c.ring_index(0.0, (20.0, 20.0, 20.0))
    for f in range(3):
        pts = synth.uniform_points(600 + f, 4000, 0.0, 20.0)
        c.append(pts)
        m.append(pts)
    win = m.live().copy()
    segs = segments(610, 257, 0.0, 20.0, [0.0, 0.4, 6.0], win)
    radius = np.resize(np.float64([0.0, 0.4, 0.8, 3.0]), len(segs))
    before = W.segment_sweep(win, segs, radius)
    both_forms(E, c, segs, radius, before, "before")
    # remove a ball around what stops every 4th sweep: that row goes, with its neighbours
    gone = np.zeros(len(win), bool)
    for q in np.flatnonzero(before[0] != NO_INDEX)[::4]:
        centre = win[before[0][q]].astype(np.float64)
        if np.isnan(centre[0]):
            continue                                         # went with an earlier ball
        d = win.astype(np.float64) - centre
        with np.errstate(invalid="ignore"):
            inside = ((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]) <= 0.6 * 0.6
        inside &= ~gone
        assert c.ring_remove_ball(centre, 0.6) == int(inside.sum())
        gone |= inside
        win[inside] = NAN
    assert gone.sum() > 30
    after = W.segment_sweep(win, segs, radius)
    got = c.segment_sweep(segs, radius, E.ALGO_RING)
    assert not np.any(gone[got[0][got[0] != NO_INDEX]]), "a removed row blocks"
    assert np.any(after[0] != before[0])
    both_forms(E, c, segs, radius, after, "after the removal")
    # compaction: the same t under the new indices
    live, reclaimed, remap = c.ring_compact(want_remap=True)
    assert live == len(win) - gone.sum() and reclaimed == gone.sum()
    new_win = np.zeros((live, 3), np.float32)
    new_win[remap[~gone]] = win[~gone]
    compacted = W.segment_sweep(new_win, segs, radius)
    assert np.array_equal(compacted[1], after[1], equal_nan=True)
    both_forms(E, c, segs, radius, compacted, "after the compaction")
    # an append that evicts the blocker: fill the reclaimed room, then the next frame overwrites the oldest slots
    m2 = Mirror(cap)
    m2.append(new_win)
    fill = synth.uniform_points(620, cap - live, 0.0, 20.0)
    c.append(fill)
    m2.append(fill)
    assert len(c) == cap and m2.nxt == 0
    target = m2.live()[m2.nxt + 5].astype(np.float64)                          # among the next slots to go
    seg = np.concatenate([target - [0.3, 0.0, 0.0], target + [0.3, 0.0, 0.0]])[None, :]
    idx, t = c.segment_sweep(seg, 0.1, E.ALGO_RING)
    assert idx[0] == m2.nxt + 5 and 0.0 < t[0] < 0.5
    frame = synth.uniform_points(621, 100, 0.0, 20.0)
    c.append(frame)
    m2.append(frame)
    want = W.segment_sweep(m2.live(), seg, 0.1)
    assert want[0][0] != idx[0]
    both_forms(E, c, seg, 0.1, want, "after the evicting append")
    both_forms(E, c, segs, radius, W.segment_sweep(m2.live(), segs, radius), "the batch after the evicting append")
    c.close()


def test_index_base(E):
    pts = synth.uniform_points(630, 3000, 0.0, 20.0)
    segs = segments(631, 100, 0.0, 20.0, [0.0, 0.4, 6.0], pts)
    for ring in (True, False):
        with E.Cloud(3000) as c:
            if ring:
                c.ring_index(0.0, (20.0, 20.0, 20.0))
                c.append(pts)
            else:
                c.set_input(pts)
            c.set_index_base(1000)
            want = W.segment_sweep(pts, segs, 0.5, index_base=1000)
            assert np.any(want[0] != NO_INDEX) and np.any(want[0] == NO_INDEX)
            same(c.segment_sweep(segs, 0.5), want, f"(ring = {ring})")
            same(c.segment_sweep(segs, 0.5, E.ALGO_STREAM), want, f"(stream, ring = {ring})")


# ---- 5. work counters --------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def unit(E):
    """the wrapped window under cells of exactly 1.0"""
    frames, win, _, _ = wrapped_case()
    c = E.Cloud(len(win))
    c.ring_index(1.0, (40.0, 40.0, 40.0))
    for f in frames:
        c.append(f)
    assert len(c) == len(win) and c.ring_info()["cell_size"] == 1.0
    yield c
    c.close()


def records_read(c, call):
    c.set_work_counters(True)
    try:
        call()
        return c.last_work()[0]
    finally:
        c.set_work_counters(False)


def test_the_ordered_walk_reads_less(E, unit):
    """240 segments of 30 m from a in [2, 8)^3, half along the axes and half along (1, 1, 1) / sqrt 3.  Stopped in the first tenth
    (r = 0.5), the sweep ends its walk early and reads fewer records than the nearest search of the same capsules; free (r = 0.1), it
    reads no more.  Measured on one MI355X: see DESIGN.md, "Segment sweeps"."""
    _, win, _, _ = wrapped_case()
    a = synth.uniform_points(900, 240, 2.0, 8.0).astype(np.float64)
    d = np.tile(np.float64([1.0, 1.0, 1.0]) / np.sqrt(3.0), (240, 1))
    d[::2] = np.eye(3)[(np.arange(0, 240, 2) // 2) % 3]
    segs = np.concatenate([a, a + 30.0 * d], axis=1)
    N = len(unit)
    _, t = W.segment_sweep_boxed(win, segs, 0.5)
    early = segs[(t > 0.0) & (t <= 0.1)]
    assert len(early) >= 50, len(early)
    sweep = records_read(unit, lambda: unit.segment_sweep(early, 0.5, E.ALGO_RING))
    nearest = records_read(unit, lambda: unit.segment_nn(early, 0.5, E.ALGO_RING))
    print(f"stopped in the first tenth ({len(early)} segments, r = 0.5): the sweep reads {sweep / len(early):.1f} records per segment, "
          f"the nearest search {nearest / len(early):.1f}, ratio {sweep / nearest:.3f}")
    assert 0 < sweep < nearest
    idx, t = W.segment_sweep_boxed(win, segs, 0.1)
    free = segs[idx == NO_INDEX]
    assert len(free) >= 100, len(free)
    sweep = records_read(unit, lambda: unit.segment_sweep(free, 0.1, E.ALGO_RING))
    nearest = records_read(unit, lambda: unit.segment_nn(free, 0.1, E.ALGO_RING))
    print(f"free ({len(free)} segments, r = 0.1): the sweep reads {sweep / len(free):.1f} records per segment, the nearest search "
          f"{nearest / len(free):.1f}, ratio {sweep / nearest:.3f}")
    assert 0 < sweep <= nearest
    assert records_read(unit, lambda: unit.segment_sweep(segs, 0.5, E.ALGO_STREAM)) == len(segs) * N
    same(unit.segment_sweep(segs, 0.5, E.ALGO_RING), W.segment_sweep_boxed(win, segs, 0.5), "(30 m segments)")


# ---- 6. the device form, and the edges of the interface ----------------------------------------------------------------------------

def test_device_form_behind_an_asynchronous_append(E):
    import torch
    cap, Q = 6000, 500
    c, m = E.Cloud(cap), Mirror(cap)
    c.ring_index(0.0, (20.0, 20.0, 20.0))
    first = synth.uniform_points(640, 5000, 0.0, 20.0)
    c.append(first)
    m.append(first)
    segs = segments(641, Q, 0.0, 20.0, [0.0, 0.4, 6.0], first)
    radius = np.resize(np.float64([0.0, 0.3, 0.8, INF, NAN]), Q)
    c.reserve_queries(Q)
    dev = torch.device("cuda:0")
    st = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(st):
        tseg = torch.from_numpy(segs.copy()).to(dev)
        trad = torch.from_numpy(radius.copy()).to(dev)
        st.synchronize()
        for k, algo in enumerate((E.ALGO_RING, E.ALGO_STREAM, E.ALGO_AUTO)):
            frame = synth.uniform_points(650 + k, 1500, 0.0, 20.0)             # evicts 500 and more of the oldest rows
            tidx = torch.zeros(Q, dtype=torch.int32, device=dev)
            tt = torch.full((Q,), 7.0, dtype=torch.float64, device=dev)
            tidx2 = torch.zeros(Q, dtype=torch.int32, device=dev)
            st.synchronize()
            c.append(frame)                                                    # returns before its insert kernel has run
            c.segment_sweep_device(tseg.data_ptr(), trad.data_ptr(), Q, tidx.data_ptr(), tt.data_ptr(), st.cuda_stream, algo)
            c.segment_sweep_device(tseg.data_ptr(), trad.data_ptr(), Q, tidx2.data_ptr(), 0, st.cuda_stream, algo)          # t not wanted
            m.append(frame)
            got = (tidx.cpu().numpy().view(np.uint32), tt.cpu().numpy())
            only_idx = tidx2.cpu().numpy().view(np.uint32)
            want = W.segment_sweep(m.live(), segs, radius)
            same(got, want, f"(device form, algo {algo})")
            assert np.array_equal(only_idx, want[0])
            same(c.segment_sweep(segs, radius, algo), want, f"(host form, algo {algo})")
    st.synchronize()
    c.close()


def test_invalid_sweeps(E, wrapped):
    _, win, _, _ = wrapped_case()
    base = np.float64([10, 10, 10, 14, 12, 9])
    segs = np.tile(base, (10, 1))
    segs[1, 0] = NAN
    segs[2, 4] = INF
    segs[3, 5] = -INF
    segs[4, 3] = 1e39                                        # narrows to infinity
    segs[5, 2] = -3.5e38                                     # beyond FLT_MAX as well
    radius = np.float64([1, 1, 1, 1, 1, 1, NAN, -1.0, -INF, INF])
    want = W.segment_sweep(win, segs, radius)
    assert want[0][0] != NO_INDEX and (want[0][9], want[1][9]) == (0, 0.0)
    assert np.all(want[0][1:9] == NO_INDEX) and np.all(np.isnan(want[1][1:9]))
    both_forms(E, wrapped, segs, radius, want)
    both_forms(E, wrapped, segs[::-1].copy(), radius[::-1].copy(), tuple(w[::-1] for w in want))


def test_nan_and_infinite_rows_never_block(E):
    pts = synth.uniform_points(700, 500, 0.0, 10.0)
    pts[::7, 0] = NAN
    pts[3::11] = NAN
    pts[5::13, 2] = INF
    pts[6::17, 1] = -INF
    segs = segments(701, 120, 0.0, 10.0, [0.0, 0.5, 6.0])
    with E.Cloud(500) as c:
        c.ring_index(1.0, (16.0, 16.0, 16.0))
        c.append(pts)
        for r in (0.7, INF):
            want = W.segment_sweep(pts, segs, r)
            assert np.all(np.isfinite(pts[want[0][want[0] != NO_INDEX]]))
            both_forms(E, c, segs, r, want, f"r = {r}")


def test_empty_cloud_q0_null_pointers_and_refused_algos(E):
    L = E.lib()
    segs = np.float64([[0, 0, 0, 1, 1, 1], [2, 2, 2, 3, 3, 3], [NAN, 2, 2, 3, 3, 3], [2, 2, 2, 3, 3, 3]])
    radius = np.float64([1.0, INF, 1.0, -1.0])
    p = lambda a: a.ctypes.data                                                # noqa: E731
    for ring in (False, True):
        c = E.Cloud(100)
        if ring:
            c.ring_index(1.0, (8.0, 8.0, 8.0))
        for algo in (E.ALGO_AUTO, E.ALGO_STREAM) + ((E.ALGO_RING,) if ring else ()):
            idx, t = np.zeros(4, np.uint32), np.zeros(4)
            assert L.pct_segment_sweep_batch(c.handle, algo, p(segs), p(radius), 4, p(idx), p(t)) == 5         # PCT_ERR_EMPTY, outputs filled
            assert np.all(idx == NO_INDEX) and np.all(t[:2] == 1.0) and np.all(np.isnan(t[2:]))
            import torch
            c.reserve_queries(4)
            dev = torch.device("cuda:0")
            tseg, trad = torch.from_numpy(segs).to(dev), torch.from_numpy(radius).to(dev)
            tidx, tt = torch.zeros(4, dtype=torch.int32, device=dev), torch.zeros(4, dtype=torch.float64, device=dev)
            torch.cuda.synchronize()
            cs = torch.cuda.current_stream().cuda_stream
            assert L.pct_segment_sweep_batch_dev(c.handle, algo, tseg.data_ptr(), trad.data_ptr(), 4, tidx.data_ptr(), tt.data_ptr(), cs) == 0      # PCT_OK
            same((tidx.cpu().numpy().view(np.uint32), tt.cpu().numpy()), (idx, t), "(empty cloud, device form)")
        if not ring:
            assert L.pct_segment_sweep_batch(c.handle, E.ALGO_RING, p(segs), p(radius), 4, p(idx), None) == 2      # no rolling-map index
        c.close()
    pts = synth.uniform_points(710, 100, 0.0, 4.0)
    with E.Cloud(100) as c:
        c.set_input(pts)
        idx, t = np.full(4, 77, np.uint32), np.full(4, 7.0)
        untouched = lambda: np.all(idx == 77) and np.all(t == 7.0)             # noqa: E731
        assert L.pct_segment_sweep_batch(c.handle, E.ALGO_AUTO, p(segs), p(radius), 0, p(idx), p(t)) == 0          # Q == 0
        assert L.pct_segment_sweep_batch(c.handle, E.ALGO_AUTO, None, None, 0, None, None) == 0
        assert L.pct_segment_sweep_batch_dev(c.handle, E.ALGO_AUTO, None, None, 0, None, None, None) == 0
        assert untouched()
        for bad in (lambda: L.pct_segment_sweep_batch(None, E.ALGO_AUTO, p(segs), p(radius), 4, p(idx), p(t)),
                    lambda: L.pct_segment_sweep_batch(c.handle, E.ALGO_AUTO, None, p(radius), 4, p(idx), p(t)),
                    lambda: L.pct_segment_sweep_batch(c.handle, E.ALGO_AUTO, p(segs), None, 4, p(idx), p(t)),
                    lambda: L.pct_segment_sweep_batch(c.handle, E.ALGO_AUTO, p(segs), p(radius), 4, None, p(t)),
                    lambda: L.pct_segment_sweep_batch(c.handle, E.ALGO_AUTO, p(segs), p(radius), -1, p(idx), p(t)),
                    lambda: L.pct_segment_sweep_batch(c.handle, E.ALGO_GRID, p(segs), p(radius), 4, p(idx), p(t)),
                    lambda: L.pct_segment_sweep_batch(c.handle, E.ALGO_STREAM_EXACT, p(segs), p(radius), 4, p(idx), p(t)),
                    lambda: L.pct_segment_sweep_batch(c.handle, E.ALGO_RING, p(segs), p(radius), 4, p(idx), p(t)),
                    lambda: L.pct_segment_sweep_batch(c.handle, 99, p(segs), p(radius), 4, p(idx), p(t)),
                    lambda: L.pct_segment_sweep_batch_dev(None, E.ALGO_AUTO, p(segs), p(radius), 4, p(idx), p(t), None),
                    lambda: L.pct_segment_sweep_batch_dev(c.handle, E.ALGO_GRID, p(segs), p(radius), 4, p(idx), p(t), None),
                    lambda: L.pct_segment_sweep_batch_dev(c.handle, E.ALGO_STREAM_EXACT, p(segs), p(radius), 4, p(idx), p(t), None),
                    lambda: L.pct_segment_sweep_batch_dev(c.handle, E.ALGO_RING, p(segs), p(radius), 4, p(idx), p(t), None),
                    lambda: L.pct_segment_sweep_batch_dev(c.handle, 99, p(segs), p(radius), 4, p(idx), p(t), None),
                    lambda: L.pct_segment_sweep_batch_dev(c.handle, E.ALGO_AUTO, None, p(radius), 4, p(idx), p(t), None),
                    lambda: L.pct_segment_sweep_batch_dev(c.handle, E.ALGO_AUTO, p(segs), None, 4, p(idx), p(t), None),
                    lambda: L.pct_segment_sweep_batch_dev(c.handle, E.ALGO_AUTO, p(segs), p(radius), 4, None, p(t), None),
                    lambda: L.pct_segment_sweep_batch_dev(c.handle, E.ALGO_AUTO, p(segs), p(radius), -1, p(idx), p(t), None)):
            assert bad() == 2 and untouched()                                  # PCT_ERR_INVALID, nothing written
        c.build_grid()
        assert L.pct_segment_sweep_batch(c.handle, E.ALGO_GRID, p(segs), p(radius), 4, p(idx), p(t)) == 2 and untouched()     # a grid does not help
        # the optional output
        assert L.pct_segment_sweep_batch(c.handle, E.ALGO_AUTO, p(segs), p(radius), 4, p(idx), None) == 0
        want = W.segment_sweep(pts, segs, radius)
        assert np.array_equal(idx, want[0]) and np.all(t == 7.0)
        same(c.segment_sweep(segs, radius), want)


# ---- 8. the C++ mirror through a compiled client -----------------------------------------------------------------------------------

def test_cxx_client_sweeps_and_free_fraction():
    """examples/segment_sweeps.cpp: ObstacleMap::sweepSegments and freeFraction on a plain, a rolling and an empty map, every answer
    compared with a host loop; a point at exactly search_margin gives freeFraction < 1 while segmentCollides is false"""
    import subprocess
    from pointcloudtraj_amd import build
    build.build_all()
    exe = os.path.join(build.LIB, "segment_sweeps")
    r = subprocess.run([exe, "120"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "121 segments" in r.stdout and " 0 answers differ" in r.stdout
    stopped = int(r.stdout.split(":")[1].split()[0])
    assert stopped >= 20, r.stdout
