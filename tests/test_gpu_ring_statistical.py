"""GPU tests of statistical outlier removal on the rolling map (pct_cloud_ring_knn_mean_distances, _knn_distance_stats,
_remove_statistical, _remove_isolated and their way up through the corridor finder): csrc/ring_statistical.hpp.

Reference: the numpy model of the contract (tests/helpers/ring_statistical_model.py: brute-force k-NN in the contract's arithmetic and
order, the serial sum of the k distances, the tree sums, removals as NaN rows, the empty-window and auto-compaction rules) and, over
the model's rows, the numpy restatements of the searches that tests/test_gpu_ring_remove.py uses.  Everything is exact; there are no
tolerances: means and statistics are compared bit for bit (NaN equal to NaN)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from pointcloudtraj_amd import scenarios as S, synth
from test_gpu_ring_remove import EXTENT, PRM, check_counts, check_searches, check_slots, params, ref_inflate

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import depth_model as D  # noqa: E402
import ring_statistical_model as T  # noqa: E402

pytestmark = pytest.mark.gpu

BOX = np.float32([14.0, 14.0, 10.0])
INF, NAN = np.inf, np.nan


@pytest.fixture(scope="module")
def E():
    from pointcloudtraj_amd import engine
    engine.init(0)
    return engine


def uniform(seed, n):
    return (synth.uniform_points(seed, n, 0.0, 1.0) * BOX).astype(np.float32)


def make(E, cap, res=0.0, cell=0.25):
    c, w = E.Cloud(cap), T.StatisticalWindow(cap, res if res else 0.1)
    c.ring_index(cell, EXTENT)
    if res:
        c.ring_dedup(res)
    return c, w


def feed(c, w, pts):
    c.append(pts)
    w.append_plain(pts)


def serial_sum(v):
    s = 0.0
    for x in np.asarray(v, np.float64).tolist():
        s = s + x
    return s


def check_window(c, w, tag):
    """size, live counts and the live rows, slot by slot (the crop lists the finite live rows in slot order)"""
    check_counts(c, w, tag)
    if w.count == 0:
        return
    rows = w.live()
    want = np.flatnonzero(w.live_mask() & np.isfinite(rows).all(axis=1))
    idx, _, xyz = c.radius_crop((0.0, 0.0, 0.0), 1.0e4)
    assert np.array_equal(idx, want.astype(np.uint32)) and np.array_equal(xyz, rows[want]), f"{tag}: the live rows differ from the model's"


def check_cursor(c, w, tag):
    """the ring cursor: the next point appended lands in the model's slot"""
    mark = np.float32([[13.5, 13.5, 9.5]])
    slot = w.nxt
    feed(c, w, mark)
    idx, _, xyz = c.radius_crop(mark[0], 0.0)
    assert slot in idx.tolist() and np.array_equal(xyz[idx.tolist().index(slot)], mark[0]), f"{tag}: the cursor is not where the model's is"
    check_counts(c, w, tag)


def check_means(c, w, k, newest=0, tag=""):
    got, want = c.ring_knn_mean_distances(k, newest), w.knn_mean_distances(k, newest)
    bad = np.flatnonzero(~((got == want) | (np.isnan(got) & np.isnan(want))))
    assert len(bad) == 0, f"{tag}: k = {k}, newest = {newest}: {len(bad)} means differ, first at slot {bad[0]}: {got[bad[0]]!r} != {want[bad[0]]!r}"
    return got


def check_stats(c, w, k, mult, newest=0, tag=""):
    got, want = c.ring_knn_distance_stats(k, mult, newest), w.knn_distance_stats(k, mult, newest)
    assert T.same_stats(got, want), f"{tag}: k = {k}, mult = {mult}, newest = {newest}: {got} != {want}"
    return got


def both_statistical(c, w, k, mult, newest=0, tag=""):
    (got, gst), (want, wst) = c.ring_remove_statistical(k, mult, newest), w.remove_statistical(k, mult, newest)
    assert T.same_stats(gst, wst), f"{tag}: {gst} != {wst}"
    assert got == want, f"{tag}: removed {got}, the model removes {want}"
    return got, gst


def both_isolated(c, w, k, threshold, newest=0, tag=""):
    got, want = c.ring_remove_isolated(k, threshold, newest), w.remove_isolated(k, threshold, newest)
    assert got == want, f"{tag}: removed {got}, the model removes {want}"
    return got


# ---- 1. means on mixed density -----------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def mixed():
    """~3 000 uniform points, 1.5 per m^3, and a 0.1 m lattice patch; the model's means, computed once per k"""
    g = np.arange(6, dtype=np.float64) * 0.1
    patch = np.stack(np.meshgrid(3.0 + g, 4.0 + g, 5.0 + g, indexing="ij"), axis=-1).reshape(-1, 3).astype(np.float32)
    pts = np.concatenate([uniform(500, 1500), patch, uniform(501, 1500)])
    return dict(pts=pts, mean={k: T.knn_mean_distances(pts, k) for k in (1, 8, 64)},
                q=np.concatenate([uniform(502, 120), pts[::131]]).astype(np.float32))


@pytest.mark.parametrize("k", [1, 8, 64])
def test_means_on_mixed_density(E, mixed, k):
    pts, want = mixed["pts"], mixed["mean"][k]
    c, w = make(E, 4000)
    feed(c, w, pts)
    assert np.isfinite(want).all() and want[1500:1716].max() < np.median(want[:1500])       # the patch is dense, the rest sparse
    got = c.ring_knn_mean_distances(k)
    bad = np.flatnonzero(got != want)
    assert len(bad) == 0, f"k = {k}: {len(bad)} means differ, first at slot {bad[0]}: {got[bad[0]]!r} != {want[bad[0]]!r}"
    check_window(c, w, "measuring changes nothing")
    check_slots(c, w, "measuring changes nothing")
    c.set_work_counters(True)                                                               # the instrumented build of the kernel: same answer
    assert np.array_equal(c.ring_knn_mean_distances(k), want)
    records, buckets, walked = c.last_work_ex()
    c.set_work_counters(False)
    assert walked == len(pts) and buckets >= 27 * len(pts) and records >= k * len(pts)
    if k < 64:                                                                              # the parent's route: a k-NN batch of k + 1 with the rows as queries
        idx, d2 = c.knn(pts, k + 1, E.ALGO_RING)
        route = np.empty(len(pts), np.float64)
        for i in range(len(pts)):
            own = np.flatnonzero(idx[i] == i)
            d = np.delete(d2[i], own[0] if len(own) else k)                                 # the row's own entry, or the last where it is absent
            s = 0.0
            for e in range(k):
                s = s + float(np.sqrt(d[e]))
            route[i] = s / float(k)
        assert np.array_equal(route, got), "the parent's route gives other means"
    c.close()


# ---- 2. the edges of the rule ------------------------------------------------------------------------------------------------------

EDGE_ROWS = np.float32([[1, 1, 1], [1.5, 1, 1],                                             # a pair
                        [5, 5, 5], [5, 5, 5], [5, 5, 5], [5, 5, 5], [5, 5, 5],              # k + 3 coincident copies for k = 2
                        [INF, 3, 3], [NAN, 4, 4],
                        [1.0e6, 1.0e6, 1.0e6], [1.0e6, 1.0e6 + 0.25, 1.0e6], [3.0e38, 0, 0]])  # the wild path


def test_edges_of_the_rule(E):
    c, w = make(E, 64)
    feed(c, w, EDGE_ROWS[:2])                                                               # a pair alone
    assert check_means(c, w, 1, tag="a pair").tolist() == [0.5, 0.5]
    assert check_means(c, w, 2, tag="a pair").tolist() == [INF, INF]
    feed(c, w, EDGE_ROWS[2:])
    for k in (1, 2, 3, 9, 10):                                                              # 10 finite rows: 9 candidates each
        got = check_means(c, w, k, tag="edges")
        assert got[7] == INF and np.isnan(got[8])                                           # +inf: never k candidates; NaN: not judged
        assert np.isfinite(np.delete(got, [7, 8])).all() == (k <= 9)
    m2 = c.ring_knn_mean_distances(2)
    assert m2[2:7].tolist() == [0.0] * 5                                                    # slots 5 and 6: their own slot is not among the 3 best by index
    assert c.ring_knn_mean_distances(1)[9:11].tolist() == [0.25, 0.25] and np.isfinite(m2[11]) and m2[11] > 1.0e38      # wild rows are rows
    for k, mult in ((2, 1.0), (9, 1.0), (10, 0.0)):
        check_stats(c, w, k, mult, tag="edges")
    c.close()


def test_exactly_k_plus_one_and_exactly_k_finite_rows(E):
    rows = np.float32([[1, 1, 1], [13, 13, 9], [1, 13, 5], [12, 2, 8]])
    c, w = make(E, 64)
    feed(c, w, rows)                                                                        # k + 1 finite rows, k = 3: every bucket is visited before the walk may stop
    got = check_means(c, w, 3, tag="k + 1 rows")
    assert np.isfinite(got).all()
    st = check_stats(c, w, 3, 3.0, tag="k + 1 rows")
    assert st["measured"] == 4
    feed(c, w, np.float32([[INF, 1, 1], [NAN, 2, 2]]))
    got = check_means(c, w, 4, tag="k rows")                                                # k finite rows, k = 4: every finite row is unmeasured
    assert got[:5].tolist() == [INF] * 5 and np.isnan(got[5])
    st = check_stats(c, w, 4, 3.0, tag="k rows")
    assert st["measured"] == 0 and np.isnan(st["mean"]) and np.isnan(st["stddev"]) and st["threshold"] == INF and st["sum"] == 0.0
    removed, st2 = both_statistical(c, w, 4, 3.0, tag="k rows")
    assert removed == 0 and st2["measured"] == 0 and c.ring_live() == (5, 1)
    assert both_isolated(c, w, 4, INF) == 0 and c.ring_live() == (5, 1)                     # +inf is allowed and removes nothing
    assert both_isolated(c, w, 4, 1.0e300, tag="k rows") == 5                               # every judged row: the empty-window rule follows
    assert len(c) == w.count == 0 and w.resets == 1
    assert both_isolated(c, w, 4, 1.0) == 0 and both_statistical(c, w, 4, 1.0)[0] == 0 and len(c.ring_knn_mean_distances(4)) == 0
    st = c.ring_knn_distance_stats(4, 1.0)
    assert st["measured"] == 0 and np.isnan(st["mean"]) and st["threshold"] == INF
    rad, idx, _ = c.inflate(params(E), np.float64([[5, 5, 5]]))
    assert rad[0] == PRM["max_radius"] - PRM["search_margin"] and idx[0] == 0xFFFFFFFF
    feed(c, w, rows)                                                                        # filing starts at slot 0 again
    check_means(c, w, 1, tag="after the reset")
    c.close()


def small_table(E, cap):
    """the 8 x 8 x 8 table of tests/test_gpu_ring_search.py: the cube of a walk that goes on past r = 3 wraps around it"""
    c, w = E.Cloud(cap), T.StatisticalWindow(cap)
    c.ring_index(2.0, (8.0, 8.0, 8.0))
    assert all(d <= 8 for d in c.ring_info()["dims"]), c.ring_info()
    return c, w


def test_means_on_a_small_table_with_folding_and_closed_axes(E):
    """a window that drifts away over an 8 x 8 x 8 table: several world cells share a bucket, and a row whose k candidates lie
    frames apart walks until its axes close -- the box of such a step names buckets the list has seen (the idempotent insert)"""
    c, w = small_table(E, 1000)
    for f in range(9):
        drift = np.float32([17.0 * f, -3.0 * f, 0.5 * f])
        feed(c, w, (synth.uniform_points(120, 120, 0.0, 10.0, offset=f * 120) + drift).astype(np.float32))
        if f in (2, 5, 8):
            for k in (1, 7, 64):
                check_means(c, w, k, tag=f"frame {f}")
    assert (w.count, w.nxt) == (1000, 80), "the ring has wrapped"
    c.close()


def test_fewer_rows_than_k_plus_one_on_a_small_table(E):
    """50 rows under k = 64: every axis of the 8 x 8 x 8 table closes before a list fills, and no row is measured; under k = 49
    every row's list is exactly the other 49"""
    c, w = small_table(E, 50)
    feed(c, w, synth.uniform_points(150, 50, 0.0, 10.0))
    assert check_means(c, w, 64, tag="50 rows").tolist() == [INF] * 50
    assert check_stats(c, w, 64, 1.0, tag="50 rows")["measured"] == 0
    assert np.isfinite(check_means(c, w, 49, tag="50 rows")).all()
    assert check_stats(c, w, 49, 1.0, tag="50 rows")["measured"] == 50
    c.close()


# ---- 3. the statistics -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [255, 256, 257])
def test_statistics_at_one_and_two_tree_levels(E, n):
    c, w = make(E, n)
    feed(c, w, uniform(600 + n, n))
    mean = check_means(c, w, 4, tag=f"{n} rows")
    for mult in (3.0, 0.0, -1.5):                                                           # a multiplier of 0 and a negative one are plain arithmetic
        got = c.ring_knn_distance_stats(4, mult)
        assert T.same_stats(got, T.stats(mean, mult)), f"{n} rows, mult = {mult}: {got} != {T.stats(mean, mult)}"
        assert got["measured"] == n
    assert c.ring_knn_distance_stats(4, 0.0)["threshold"] == c.ring_knn_distance_stats(4, 0.0)["mean"]
    c.close()


def test_statistics_at_three_tree_levels(E):
    n = 65537
    pts = uniform(610, n)
    c = E.Cloud(n)
    c.ring_index(0.25, EXTENT)
    c.append(pts)
    mean = c.ring_knn_mean_distances(4)
    assert np.isfinite(mean).all()
    sample = np.arange(0, n, n // 200)[:200]
    assert np.array_equal(mean[sample], T.knn_mean_distances(pts, 4, sample)[sample]), "the means of the sampled rows differ from the brute-force model"
    want = T.stats(mean, 3.0)
    got = c.ring_knn_distance_stats(4, 3.0)
    assert T.same_stats(got, want), f"{got} != {want}"
    assert want["sum"] != serial_sum(mean) and want["sum_sq"] != serial_sum(mean * mean), "these means do not tell the tree order from the serial one"
    newest = c.ring_knn_distance_stats(4, 3.0, 300)                                         # a scope: 65 237 slots of the first level hold +0.0
    scoped = np.where(np.arange(n) >= n - 300, mean, NAN)
    assert T.same_stats(newest, T.stats(scoped, 3.0)) and newest["measured"] == 300
    c.close()


def test_statistics_of_one_row_and_of_coincident_rows(E):
    c, w = make(E, 64)
    feed(c, w, np.float32([[1, 1, 1], [1, 2, 1]]))
    st = check_stats(c, w, 1, 5.0, newest=1, tag="N = 1")                                   # one judged row
    assert st == dict(measured=1, sum=1.0, sum_sq=1.0, mean=1.0, stddev=0.0, threshold=1.0)
    c.close()
    c, w = make(E, 64)
    feed(c, w, np.float32([[2.3, 4.1, 7.7]] * 10))
    st = check_stats(c, w, 3, 2.0, tag="coincident")
    assert st["measured"] == 10 and st["mean"] == 0.0 and st["stddev"] == 0.0 and st["threshold"] == 0.0
    assert both_statistical(c, w, 3, 2.0)[0] == 0                                           # 0 > 0 is false: the compare is strict
    feed(c, w, np.float32([[2.3, 4.1, 7.8]] * 3))                                           # means 0.1-ish for three rows: var > 0 by a margin
    check_stats(c, w, 3, 1.0, tag="two groups")
    c.close()


# ---- 4. the scope on a wrapped ring --------------------------------------------------------------------------------------------------

def test_scope_on_a_wrapped_ring(E):
    """3 500 sparse points into 3 000 slots: the cursor stands at 500 and arrival order starts there"""
    cap = 3000
    c, w = make(E, cap)
    for f, n in enumerate((1500, 1500, 500)):
        feed(c, w, uniform(520 + f, n))
    assert (w.count, w.nxt) == (cap, 500)
    for newest in (700, 1, cap - 1, 0, -5, cap + 9):
        got = check_means(c, w, 4, newest, "wrapped")
        check_stats(c, w, 4, 1.0, newest, "wrapped")
        judged = cap if newest <= 0 or newest >= cap else newest
        assert int((~np.isnan(got)).sum()) == judged
    seam = c.ring_knn_mean_distances(4, 700)
    assert np.array_equal(np.flatnonzero(~np.isnan(seam)), np.r_[0:500, 2800:3000])           # slots 2800 .. 2999 and 0 .. 499, across the seam
    full = w.knn_mean_distances(4)
    thr = float(np.sort(full)[-400])
    old_outliers = np.flatnonzero(full[500:2800] > thr) + 500
    removed = both_isolated(c, w, 4, thr, 700, "the newest 700")
    assert 0 < removed < 700 and len(old_outliers) > 100 and w.live_mask()[old_outliers].all()          # old outliers out of scope stay
    check_window(c, w, "the newest 700")
    check_slots(c, w, "the newest 700")
    removed, st = both_statistical(c, w, 4, 1.0, 700, "statistical, the newest 700")
    assert removed > 0 and st["measured"] <= 700 and w.live_mask()[old_outliers].all()
    check_window(c, w, "statistical, the newest 700")
    removed, st = both_statistical(c, w, 4, 1.0, cap + 9, "every row")
    assert removed > 50 and not w.live_mask()[old_outliers].all()
    check_window(c, w, "every row")
    check_slots(c, w, "every row")
    check_searches(E, c, w.live(), uniform(523, 100), "every row")
    check_cursor(c, w, "every row")
    c.close()


# ---- 5. dead records and the overflow queue ------------------------------------------------------------------------------------------

def test_dead_records_behind_live_heads(E, mixed):
    c, w = make(E, 4000)
    feed(c, w, mixed["pts"])
    assert c.ring_remove_ball((7, 7, 5), 3.5) == w.remove_ball((7, 7, 5), 3.5) > 100        # dead records sit behind live heads now
    after = check_means(c, w, 8, tag="after the ball")
    live = w.live_mask()
    assert np.isnan(after[~live]).all() and (after[live] >= mixed["mean"][8][live]).all() and (after[live] > mixed["mean"][8][live]).sum() > 20
    check_stats(c, w, 8, 2.0, tag="after the ball")
    thr = float(np.sort(after[live])[-60])
    assert both_isolated(c, w, 8, thr, tag="after the ball") == int((after[live] > thr).sum()) > 0
    assert both_statistical(c, w, 8, 2.0, tag="after the ball")[0] > 0
    check_window(c, w, "after the ball")
    check_slots(c, w, "after the ball")
    check_searches(E, c, w.live(), mixed["q"], "after the ball")
    c.close()


def test_queued_records_are_neighbours_and_can_be_removed(E):
    """100 points in one cell (32 in its bucket, 68 in the overflow queue), built as tests/test_gpu_ring_remove.py builds them"""
    cap = 1000
    c, w = make(E, cap)
    cluster = (np.float32([5.0, 5.0, 5.0]) + synth.uniform_points(331, 100, 0.01, 0.24)).astype(np.float32)
    feed(c, w, np.concatenate([uniform(540, 450), cluster, uniform(541, 450)]))
    queued = 450 + np.flatnonzero(np.array([c.debug_ring_slot(450 + i)[0] for i in range(100)], np.int64) & 0x80000000)
    assert len(queued) == c.ring_info()["overflow_entries"] == 68
    for k in (1, 16, 64):
        got = check_means(c, w, k, tag="the cluster")
        assert got[450:550].max() < 0.4 < np.median(got[:450])                              # 64 of its 99 neighbours: queued records are candidates
    assert both_statistical(c, w, 16, 1.0, 600, tag="the cluster, statistical")[0] > 0        # slots 400 .. 999: the cluster and sparse rows
    check_window(c, w, "the cluster, statistical")
    m16 = w.knn_mean_distances(16)
    thr = float(np.median(m16[450:550]))
    verdict = m16 > thr
    assert verdict[queued].any() and not verdict[queued].all()                              # both outcomes occur among the queued rows
    assert both_isolated(c, w, 16, thr, tag="the cluster") == int(verdict.sum())
    check_window(c, w, "the cluster")
    check_slots(c, w, "the cluster")
    check_searches(E, c, w.live(), np.concatenate([uniform(542, 80), cluster[::7]]).astype(np.float32), "the cluster")
    c.close()


# ---- 6. a removal in every sense -----------------------------------------------------------------------------------------------------

def test_autocompaction_follows_the_rule(E):
    cap = 2000
    c, w = make(E, cap)
    g = np.arange(8, dtype=np.float64) * 0.2
    block = np.stack(np.meshgrid(6.0 + g, 6.0 + g, 3.0 + g, indexing="ij"), axis=-1).reshape(-1, 3).astype(np.float32)
    feed(c, w, np.concatenate([uniform(550, 700), block, uniform(551, 700)]))
    c.ring_autocompact(0.2)
    w.autocompact(0.2)
    few = both_isolated(c, w, 2, 0.8, 150, "a few rows")                                    # fewer than 0.2 x 2000 dead: no compaction
    assert 0 < few < 400 and c.ring_compact_count() == w.compactions == 0
    check_window(c, w, "a few rows")
    many, _ = both_statistical(c, w, 2, -0.5, tag="every row")                              # a threshold below the mean: hundreds go
    assert few + many >= 400 and c.ring_compact_count() == w.compactions == 1 and len(c) == w.count == w.live_count()
    check_window(c, w, "compacted")
    check_slots(c, w, "compacted")
    check_searches(E, c, w.live(), uniform(552, 100), "compacted")
    check_cursor(c, w, "compacted")
    c.close()


def test_a_plan_captured_before_the_call_answers_after_it(E):
    window, frame = 6000, 1500
    P = S.C5_PARAMS
    c, w = E.Cloud(window), T.StatisticalWindow(window)
    c.ring_index(2.0, (70.0, 70.0, 8.0))
    for f in range(3):
        feed(c, w, S.c5_frame_clustered(f, frame))
    replan = E.ReplanPlan(c, S.C5_NODES, 128, S.C5_SEGMENTS)
    start, nodes, coef, Tm, od = S.c5_tick_queries(3)
    prm = E.inflate_params(start, P["sample_range"], P["search_margin"], P["max_radius"])
    p = dict(start=start, **P)

    def ask(tag):
        got = replan.run(prm, nodes, coef, Tm, od, 0.0, 2.0, 0.02, want_nn=True)
        rad, idx, d2 = c.inflate(prm, nodes)                                                # the direct calls
        assert np.array_equal(got["node_radius"], rad) and np.array_equal(got["node_d2"], d2) and np.array_equal(got["node_idx"], idx), f"{tag}: nodes"
        wr, wi, wd = ref_inflate(w.live(), p, nodes)
        assert np.array_equal(rad, wr) and np.array_equal(d2, wd) and np.array_equal(idx, wi), f"{tag}: nodes against numpy"
        n = got["nsamples"]
        assert n > 0 and np.array_equal(got["sample_radius"][:n], c.inflate(prm, got["sample_pos"][:n])[0]), f"{tag}: samples"
        return rad

    r0 = ask("before")
    assert both_statistical(c, w, 4, 1.0, tag="the clustered window")[0] > 0
    r1 = ask("after")
    assert (r1 >= r0).all()                                                                 # radii can only grow when points leave
    left = c.ring_live()[0]
    assert both_isolated(c, w, 64, 0.0, tag="everything") == left > 0 and len(c) == w.count == 0       # no row has 64 coincident copies
    ask("after the window was emptied")                                                     # the empty-cloud rule, from the graph captured on the full window
    replan.close()
    c.close()


def test_per_frame_filter_with_dedup(E):
    """de-dup on: newest = what the append kept.  Every frame is a dense sheet re-sensed plus fresh sparse noise; a removed voxel
    that is offered again is kept again, as in the model"""
    cap = 2000
    c, w = make(E, cap, res=0.1)
    g = np.arange(30, dtype=np.float64) * 0.2
    sheet = np.stack(np.meshgrid(2.0 + g, 3.0 + g, [4.0], indexing="ij"), axis=-1).reshape(-1, 3).astype(np.float32)
    total = 0
    for f in range(3):
        frame = np.concatenate([sheet, uniform(530 + f, 300)])
        c.append(frame)
        kept = int(w.append(frame).sum())
        assert c.ring_dedup_last()["kept"] == kept >= 250
        total += both_isolated(c, w, 2, 0.45, kept, f"frame {f}")
        check_window(c, w, f"frame {f}")
        assert set(map(tuple, sheet.tolist())) <= w.live_set(), f"frame {f}: the sheet stays"
    assert total > 400
    check_slots(c, w, "at the end")
    gone = uniform(530, 300)                                                                # frame 0's noise: most of it was removed
    c.append(gone)
    again = int(w.append(gone).sum())
    assert c.ring_dedup_last()["kept"] == again > 100                                       # the holders the removals left decide, as in the model
    check_window(c, w, "after the re-offer")
    c.close()


def test_every_form_of_removal_in_a_row_on_one_window(E):
    """What the forms of removal share shows where one runs behind another: the meeting words are zero between different kernels,
    the sequence number carries from form to form, the overflow queue's head advances under every predicate, and the bookkeeping
    behind the wait (live counts, the auto mode) is one.  ONE window: 4 096 slots fed three frames of 2 048 (wrapped), sparse rows
    plus 200 rows in one 0.5 m cell (32 in its bucket, the rest in the overflow queue), auto-compaction at 0.25; ball, box, index
    list, carve from a 32 x 24 image, radius outliers, statistical and isolated outliers one after another.  After each: `removed`,
    pct_cloud_ring_live and the surviving rows as the model has them, exact."""
    cap = 4096
    c, w = make(E, cap, cell=0.5)
    c.ring_autocompact(0.25)
    w.autocompact(0.25)
    cluster = (np.float32([5.0, 5.0, 5.0]) + synth.uniform_points(700, 200, 0.01, 0.24)).astype(np.float32)
    for f in range(3):
        pts = uniform(710 + f, 2048)
        if f:
            pts[300:400] = cluster[100 * (f - 1):100 * f]
        feed(c, w, pts)
    assert (w.count, w.nxt) == (cap, 2048), "the ring has wrapped"
    assert c.ring_info()["overflow_entries"] == 200 - 32

    def settled(form, got, want):
        assert got == want > 0, f"{form}: removed {got}, the model removes {want}"
        check_window(c, w, form)
        assert c.ring_compact_count() == w.compactions, f"{form}: compactions"
        assert c.ring_info()["overflow_entries"] > 0, f"{form}: the next form finds the overflow queue in use"

    settled("ball", c.ring_remove_ball((3, 3, 3), 2.0), w.remove_ball((3, 3, 3), 2.0))
    settled("box", c.ring_remove_box((0, 0, 0), (14, 2.5, 10)), w.remove_box((0, 0, 0), (14, 2.5, 10)))
    live = np.flatnonzero(w.live_mask())
    queued = np.flatnonzero((w.live()[:, None] == cluster[::10]).all(axis=2).any(axis=1))
    idx = np.concatenate([live[::9], live[:360:9], queued]).astype(np.uint32)              # entries named twice, rows of the queue
    settled("index list", c.ring_remove_indices(idx), w.remove_indices(idx))
    assert w.compactions == 1 and w.count == w.live_count() < cap, "the index list brought the dead rows to a quarter of the capacity"
    view = E.depth_view((7.0, 7.0, -6.0), np.eye(3), 32, 24, fov_hor_deg=90.0)             # looks along +z from 6 m below the box
    img = np.random.default_rng(720).uniform(7.0, 15.0, (24, 32)).astype(np.float32)
    img[3, :], img[11, 5], img[20, 30] = np.inf, np.nan, -np.inf
    pr = D.project(view, cluster)
    img[pr["rv"][pr["inside"]], pr["ru"][pr["inside"]]] = 9.0                              # the cluster, 11 m out, is not seen through
    settled("carve", c.ring_carve_depth(view, img, 0.05), w.carve(view, img, 0.05))
    settled("radius outliers", c.ring_remove_outliers(0.6, 2), w.remove_outliers(0.6, 2))
    (got, gst), (want, wst) = c.ring_remove_statistical(4, 1.0), w.remove_statistical(4, 1.0)
    assert T.same_stats(gst, wst), f"statistical: {gst} != {wst}"
    settled("statistical", got, want)
    settled("isolated", c.ring_remove_isolated(4, 0.7, 300), w.remove_isolated(4, 0.7, 300))
    assert w.compactions >= 2 and w.resets == 0
    check_slots(c, w, "at the end")
    check_searches(E, c, w.live(), np.concatenate([uniform(730, 80), cluster[::9]]).astype(np.float32), "at the end")
    check_cursor(c, w, "at the end")
    c.close()


# ---- 7. invalid arguments ------------------------------------------------------------------------------------------------------------

def test_invalid_arguments_change_nothing(E):
    L = E.lib()
    plain = E.Cloud(100)
    plain.set_input(uniform(510, 50))
    for call in (lambda: plain.ring_knn_mean_distances(2), lambda: plain.ring_knn_distance_stats(2, 1.0),
                 lambda: plain.ring_remove_statistical(2, 1.0), lambda: plain.ring_remove_isolated(2, 1.0)):
        with pytest.raises(E.EngineError) as ei:
            call()                                                                          # no rolling-map index
        assert ei.value.code == 2
    plain.close()
    c, w = make(E, 100)
    assert c.ring_remove_isolated(3, 0.5) == 0 and len(c.ring_knn_mean_distances(3)) == 0   # an empty cloud
    removed, st = c.ring_remove_statistical(3, 1.0)
    assert removed == 0 and T.same_stats(st, T.stats([], 1.0)) and T.same_stats(c.ring_knn_distance_stats(3, 1.0), T.stats([], 1.0))
    pts = uniform(511, 60)
    feed(c, w, pts)
    before = [c.debug_ring_slot(i) for i in range(60)]
    n, out, st = C.c_int64(-1), np.zeros(60, np.float64), E.KnnStats()
    bad = [lambda: c.ring_knn_mean_distances(0), lambda: c.ring_knn_mean_distances(65), lambda: c.ring_knn_distance_stats(0, 1.0),
           lambda: c.ring_knn_distance_stats(2, np.inf), lambda: c.ring_knn_distance_stats(2, np.nan), lambda: c.ring_remove_statistical(65, 1.0),
           lambda: c.ring_remove_statistical(-1, 1.0), lambda: c.ring_remove_statistical(2, -np.inf), lambda: c.ring_remove_statistical(2, np.nan),
           lambda: c.ring_remove_isolated(0, 1.0), lambda: c.ring_remove_isolated(65, 1.0), lambda: c.ring_remove_isolated(2, -1.0e-300),
           lambda: c.ring_remove_isolated(2, np.nan), lambda: c.ring_remove_isolated(2, -np.inf),
           lambda: E._chk(L.pct_cloud_ring_knn_mean_distances(c.handle, 2, 0, out.ctypes.data, 59)),
           lambda: E._chk(L.pct_cloud_ring_knn_mean_distances(c.handle, 2, 0, None, 60)),
           lambda: E._chk(L.pct_cloud_ring_knn_distance_stats(c.handle, 2, 1.0, 0, None))]
    for call in bad:
        with pytest.raises(E.EngineError) as ei:
            call()
        assert ei.value.code == 2
    assert L.pct_cloud_ring_knn_mean_distances(None, 2, 0, out.ctypes.data, 60) == 2 and L.pct_cloud_ring_knn_distance_stats(None, 2, 1.0, 0, C.byref(st)) == 2
    assert L.pct_cloud_ring_remove_statistical(None, 2, 1.0, 0, C.byref(n), C.byref(st)) == 2 and L.pct_cloud_ring_remove_isolated(None, 2, 1.0, 0, C.byref(n)) == 2
    assert [c.debug_ring_slot(i) for i in range(60)] == before and c.ring_live() == (60, 0)
    assert np.array_equal(c.radius_crop((0, 0, 0), 1.0e4)[2], pts), "a refused call leaves the window bit-identical"
    assert L.pct_cloud_ring_remove_isolated(c.handle, 2, 100.0, 0, None) == 0 and c.ring_live() == (60, 0)       # `removed` may be NULL
    assert L.pct_cloud_ring_remove_statistical(c.handle, 2, 50.0, 0, None, None) == 0 and c.ring_live() == (60, 0)       # so may `stats`
    assert L.pct_cloud_ring_remove_statistical(c.handle, 2, 50.0, 0, None, C.byref(st)) == 0 and T.same_stats(st.as_dict(), w.knn_distance_stats(2, 50.0))
    c.close()


# ---- 8. the scenario through the corridor finder ---------------------------------------------------------------------------------------

def test_speckle_scenario_through_the_finder(E):
    from pointcloudtraj_amd import corridor
    G = S.RGBD
    _, steps = T.run_speckle_statistical()
    finder = corridor.SafeRegionRrtStar(G["cap"])
    finder.enableRollingMap(0.25, G["extent"])
    finder.setRollingDedup(G["res"])
    p = S.PARAMS
    finder.setParam(p["safety_margin"], p["search_margin"], p["max_radius"], 30.0)
    finder.setPt((0.0, 0.0, 0.0), (7.0, 0.0, 0.0), -1.0, 9.0, -9.0, 9.0, -7.0, 7.0, 30.0, 1000, p["sample_portion"], p["goal_portion"])
    seen = []
    got = S.run_rgbd_speckle_scenario_statistical(finder, D.render,
                                                  each=lambda f, x, info: seen.append((info, [x.checkTrajPtCol(s) for s in info["speckle"]])))
    assert len(got) == len(steps) == 6
    assert T.same_stats(seen[0][0]["stats"], steps[0]["stats"]) and steps[0]["stats"]["measured"] == 3072
    for f, (live, s, (info, hits)) in enumerate(zip(got, steps, seen)):
        assert live == s["live"], f"frame {f}: {len(live)} live points, the model has {len(s['live'])}"
        assert (info["kept"], info["removed"], info["threshold"]) == (s["kept"], s["removed"], s["threshold"]), f"frame {f}"
        assert info["removed"] == S.RGBD_SPECKLE["speckles"]
        assert hits == [False] * S.RGBD_SPECKLE["speckles"], f"frame {f}: checkTrajPtCol at the speckles says {hits}"
    finder.close()
