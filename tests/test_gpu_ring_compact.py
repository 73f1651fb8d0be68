"""GPU tests of compacting the rolling map (pct_cloud_ring_compact / _autocompact / _compact_count and their way up through the corridor
finder): csrc/ring_compact.hpp.

Reference: the numpy model of the contract (tests/helpers/ring_compact_model.py) and, over the model's rows, the numpy restatements
of the searches that tests/test_gpu_ring_remove.py uses; a twin cloud built by appending the compacted rows into an empty window; the
CPU finder for the corridor.  Everything is exact; there are no tolerances."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from pointcloudtraj_amd import scenarios as S, synth
from test_gpu_knn import ref_knn
from test_gpu_ring_remove import EXTENT, NO_INDEX, check_counts, check_searches, check_slots

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import depth_model as D  # noqa: E402
import ring_compact_model as K  # noqa: E402
import ring_dedup_model as M  # noqa: E402
import ring_remove_model as R  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def E():
    from pointcloudtraj_amd import engine
    engine.init(0)
    return engine


def ring_cloud(E, cap):
    c = E.Cloud(cap)
    c.ring_index(0.25, EXTENT)
    return c


def queries(seed, w, n=40):
    live = w.live()[w.live_mask()]
    return np.concatenate([synth.uniform_points(seed, n, -1.0, 11.0), live[::max(1, len(live) // 10)][:10]]).astype(np.float32)


def check_knn(E, c, w, q, tag, base=0):
    ki, kd = ref_knn(w.live(), q, 8)
    ki = np.where(ki == NO_INDEX, ki, ki + np.uint32(base))
    for algo in (E.ALGO_RING, E.ALGO_STREAM):
        gi, gd = c.knn(q, 8, algo)
        assert np.array_equal(gd, kd) and np.array_equal(gi, ki), f"{tag}: k-NN (algo {algo})"


def check_twin(E, c, w, q, tag):
    """the cloud an append of the model's rows into an empty window of the same configuration produces: same answers, same queue"""
    twin = ring_cloud(E, w.cap)
    if w.count:
        twin.append(w.live())
    assert len(twin) == len(c) == w.count
    for a, b in zip(c.knn(q, 8), twin.knn(q, 8)):
        assert np.array_equal(a, b), f"{tag}: k-NN on the twin"
    if w.count:
        assert c.ring_info()["overflow_entries"] <= twin.ring_info()["overflow_entries"], f"{tag}: more spills than a fresh cloud of the same rows"
    twin.close()


def compact_and_check(E, c, w, tag, full=False, seed=500):
    """ring_compact(want_remap) against the model's, then the cloud against the compacted mirror"""
    size = len(c)
    before = c.ring_compact_count()
    live, reclaimed, remap = c.ring_compact(want_remap=True)
    ml, mr, mremap = w.compact()
    print(f"{tag}: size {size} -> live {live}, reclaimed {reclaimed}")
    assert (live, reclaimed) == (ml, mr) and live + reclaimed == size, f"{tag}: ({live}, {reclaimed}), the model has ({ml}, {mr})"
    assert np.array_equal(remap, mremap), f"{tag}: remap"
    assert c.ring_compact_count() - before == (1 if 0 < live < size else 0)
    check_counts(c, w, tag)
    assert c.ring_live() == (w.count, 0) or reclaimed == 0
    q = queries(seed, w)
    if full:
        check_searches(E, c, w.live(), q, tag)
    else:
        check_knn(E, c, w, q, tag)
    if w.count:
        check_slots(c, w, tag)                              # every slot < L is filed under its own id
    check_twin(E, c, w, q, tag)


# ---- 1. tile and wrap edges --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 1023, 1024, 1025, 2049])
def test_window_sizes_at_the_tile_edges(E, n):
    c, w = ring_cloud(E, 3000), K.CompactWindow(3000)
    pts = synth.uniform_points(400 + n, n, 0.0, 10.0)
    c.append(pts)
    w.append_plain(pts)
    if n > 1:
        third = np.arange(0, n, 3)
        assert c.ring_remove_indices(third) == w.remove_indices(third) == len(third)
        assert c.ring_remove_ball((5, 5, 5), 2.0) == w.remove_ball((5, 5, 5), 2.0)
    compact_and_check(E, c, w, f"size {n}", full=n in (1, 1025))
    assert w.nxt == w.count and (n == 1 or w.count < n)
    compact_and_check(E, c, w, f"size {n}, again")           # nothing to reclaim now: the identity
    c.close()


def wrapped_window(E, cap=3000, frames=4, frame=1000, seed=420):
    """cap 3000 wrapped once: the cursor stands at slot 1000, inside a tile, and the age-order tiles straddle the physical end"""
    c, w = ring_cloud(E, cap), K.CompactWindow(cap)
    for f in range(frames):
        pts = synth.uniform_points(seed + f, frame, 0.0, 10.0)
        c.append(pts)
        w.append_plain(pts)
    assert (w.count, w.nxt) == (cap, (frames * frame) % cap)
    return c, w


def test_wrapped_window_compacts_in_arrival_order(E):
    c, w = wrapped_window(E)
    compact_and_check(E, c, w, "nothing removed")           # L == size: not even the rotation
    assert (w.count, w.nxt) == (3000, 1000)
    assert c.ring_remove_ball((5, 5, 5), 3.0) == w.remove_ball((5, 5, 5), 3.0) > 0
    assert c.ring_remove_box((0, 0, 0), (10, 2, 10)) == w.remove_box((0, 0, 0), (10, 2, 10)) > 0
    compact_and_check(E, c, w, "wrapped, ball and box removed", full=True)
    L = w.count
    assert 1000 < L < 2900 and w.nxt == L
    # the cursor: cap - L points fill the free slots and evict nothing
    old = w.live().copy()
    fill = synth.uniform_points(430, 3000 - L, 0.0, 10.0)
    c.append(fill)
    w.append_plain(fill)
    assert len(c) == 3000 and w.nxt == 0
    i, d = c.nn(old)
    assert np.all(d == 0.0) and np.array_equal(i, np.arange(L, dtype=np.uint32)), "an old live row was evicted or moved"
    i, d = c.nn(fill)
    assert np.all(d == 0.0) and np.array_equal(i, L + np.arange(len(fill), dtype=np.uint32))
    # ... and the next m points evict exactly the m oldest
    more = synth.uniform_points(431, 700, 0.0, 10.0)
    c.append(more)
    w.append_plain(more)
    check_counts(c, w, "after the eviction")
    check_knn(E, c, w, queries(432, w), "after the eviction")
    i, d = c.nn(old[700:])
    assert np.all(d == 0.0) and np.array_equal(i, 700 + np.arange(L - 700, dtype=np.uint32))
    assert np.all(c.nn(old[:700])[1] > 0.0), "the 700 oldest rows went"
    check_slots(c, w, "after the eviction")
    c.close()


# ---- 2. dead runs ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("wrapped", [False, True])
@pytest.mark.parametrize("pattern", ["whole_tiles", "last_only", "first_only", "alternating"])
def test_dead_runs(E, pattern, wrapped):
    """3100 rows = three tiles and 28 rows; wrapped: the cursor at slot 500, so age position p is slot (500 + p) mod 3100"""
    n = 3100
    c, w = ring_cloud(E, n), K.CompactWindow(n)
    for f, m in enumerate((n, 500) if wrapped else (n,)):
        pts = synth.uniform_points(440 + f, m, 0.0, 10.0)
        c.append(pts)
        w.append_plain(pts)
    start = w.nxt if wrapped else 0
    age = {"whole_tiles": np.arange(1024, 3072), "last_only": np.arange(0, n - 1), "first_only": np.arange(1, n), "alternating": np.arange(1, n, 2)}[pattern]
    victims = (start + age) % n
    assert c.ring_remove_indices(victims) == w.remove_indices(victims) == len(victims)
    compact_and_check(E, c, w, f"{pattern}, wrapped {wrapped}")
    assert w.count == n - len(victims) == w.nxt
    c.close()


# ---- 3. overflow queue -------------------------------------------------------------------------------------------------------------

def test_overflow_queue_holds_only_genuine_spills_after_a_compaction(E):
    """100 points in one cell (32 in its bucket, 68 in the queue) plus spread points; entries leave the middle of the queue and the
    interior of the bucket; after the compaction the 40 left in the cell take the bucket and 8 queue entries, as on a fresh cloud"""
    cap = 1000
    c, w = E.Cloud(cap), K.CompactWindow(cap)
    c.ring_index(0.25, (10.0, 10.0, 10.0))
    cluster = (np.float32([5.0, 5.0, 5.0]) + synth.uniform_points(331, 100, 0.01, 0.24)).astype(np.float32)
    first = np.concatenate([synth.uniform_points(330, 450, 0.0, 10.0), cluster, synth.uniform_points(332, 450, 0.0, 10.0)])
    c.append(first)
    w.append_plain(first)
    where = np.array([c.debug_ring_slot(450 + k)[0] for k in range(100)], np.int64)
    queued = np.flatnonzero(where & 0x80000000)
    assert len(queued) == c.ring_info()["overflow_entries"] == 68
    by_pos = queued[np.argsort(where[queued] & 0x7FFFFFFF)]
    bucket = np.setdiff1d(np.arange(100), queued)
    by_seq = bucket[np.argsort(where[bucket])]
    victims = 450 + np.concatenate([by_pos[10:55], by_seq[5:20]])           # the queue's middle; the bucket's interior
    assert c.ring_remove_indices(victims) == w.remove_indices(victims) == 60
    assert c.ring_info()["overflow_entries"] == 68                          # the queue's head is live: dead entries stay inside it
    live, reclaimed, remap = c.ring_compact(want_remap=True)
    ml, mr, mremap = w.compact()
    assert (live, reclaimed) == (ml, mr) == (940, 60) and np.array_equal(remap, mremap)
    twin = E.Cloud(cap)
    twin.ring_index(0.25, (10.0, 10.0, 10.0))
    twin.append(w.live())
    assert c.ring_info()["overflow_entries"] == twin.ring_info()["overflow_entries"] == 8
    mine = np.array([c.debug_ring_slot(s) for s in range(live)], np.int64)
    theirs = np.array([twin.debug_ring_slot(s) for s in range(live)], np.int64)
    assert np.array_equal(mine[:, 1], theirs[:, 1]), "a row is filed under another bucket than on the twin"
    assert np.all(mine[:, 4] == np.arange(live)) and np.all(theirs[:, 4] == np.arange(live))
    in_q, in_q_twin = (mine[:, 0] & 0x80000000) != 0, (theirs[:, 0] & 0x80000000) != 0
    assert in_q.sum() == in_q_twin.sum() == 8 and np.array_equal(mine[in_q, 1], theirs[in_q_twin, 1])
    # bucket contents: every bucket holds as many records as the twin's, none of them dead (head .. tail is exactly its live rows)
    fill, fill_twin = (mine[:, 3] - mine[:, 2])[~in_q], (theirs[:, 3] - theirs[:, 2])[~in_q_twin]
    assert np.array_equal(np.sort(fill), np.sort(fill_twin))
    counts = np.bincount(mine[~in_q, 1])
    assert np.all(fill == counts[mine[~in_q, 1]]), "a bucket's [head, tail) is longer than the rows filed in it: a dead record remains"
    q = np.concatenate([synth.uniform_points(333, 60, 0.0, 10.0), cluster[::9]]).astype(np.float32)
    check_searches(E, c, w.live(), q, "after the compaction")
    twin.close()
    c.close()


# ---- 4. index base -----------------------------------------------------------------------------------------------------------------

def test_remap_and_results_carry_the_index_base(E):
    c, w = wrapped_window(E, cap=2000, frames=3, frame=900, seed=450)
    c.set_index_base(1000)
    idx = 1000 + np.arange(5, 2000, 7)
    assert c.ring_remove_indices(idx) == w.remove_indices(idx, base=1000) == len(idx)
    live, reclaimed, remap = c.ring_compact(want_remap=True)
    ml, mr, mremap = w.compact(base=1000)
    assert (live, reclaimed) == (ml, mr) and np.array_equal(remap, mremap)
    assert remap[remap != NO_INDEX].min() == 1000 and remap[remap != NO_INDEX].max() == 1000 + live - 1
    check_knn(E, c, w, queries(451, w), "with the index base", base=1000)
    i, d = c.nn(w.live())
    assert np.all(d == 0.0) and np.array_equal(i, 1000 + np.arange(live, dtype=np.uint32))
    c.close()


# ---- 5. de-dup ---------------------------------------------------------------------------------------------------------------------

def test_de_dup_after_a_compaction(E):
    """cap 700: after the compaction the cursor stands at L, and a frame of 600 dooms the slots L .. 699 and 0 .. L - 101 -- live rows"""
    c, w = ring_cloud(E, 700), K.CompactWindow(700)
    c.ring_dedup(M.RES)
    pts = synth.uniform_points(460, 600, 0.0, 5.0)
    c.append(pts)
    first = w.append(pts)
    assert np.array_equal(c.ring_dedup_last()["flags"], first)
    assert c.ring_remove_box((0, 0, 0), (2.0, 5, 5)) == w.remove_box((0, 0, 0), (2.0, 5, 5)) > 100
    compact_and_check(E, c, w, "de-dup on")
    L = w.count
    small = np.concatenate([w.live()[L - 20:], pts[R.in_box(pts, (0, 0, 0), (2.0, 5, 5))][:30]])      # 20 live voxels out of the doomed range, 30 removed ones
    c.append(small)
    kept = w.append(small)
    assert np.array_equal(c.ring_dedup_last()["flags"], kept) and not kept[:20].any() and kept[20:].all()
    c.append(pts)                                           # the whole first frame: live holders, removed voxels, and doomed holders
    kept = w.append(pts)
    last = c.ring_dedup_last()
    assert np.array_equal(last["flags"], kept) and 0 < kept.sum() < 600
    check_counts(c, w, "after the re-offer")
    check_knn(E, c, w, queries(461, w), "after the re-offer")
    check_slots(c, w, "after the re-offer")
    c.close()


# ---- 6. auto mode ------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def pan_images():
    """the images of scenarios.run_rgbd_pan_scenario, rendered once by the model's renderer"""
    images = []
    K.run_pan(S.RGBD_PAN["big_cap"], 0.0, images=images)
    return images


@pytest.mark.parametrize("auto", [True, False])
def test_small_rgbd_window_matches_the_model_frame_by_frame(E, pan_images, auto):
    """the panning camera on the small window.  auto on: size, live, compactions and the rows, slot by slot, as the model has them;
    off: as the window model of the depth tests (depth_model.DepthWindow, which knows no compaction) -- nothing changed by default"""
    P = S.RGBD_PAN
    mirror = K.CompactDepthWindow(P["cap"], P["res"]) if auto else D.DepthWindow(P["cap"], P["res"])
    c = E.Cloud(P["cap"])
    c.ring_index(0.25, P["extent"])
    c.ring_dedup(P["res"])
    if auto:
        c.ring_autocompact(P["fraction"])
        mirror.autocompact(P["fraction"])
    q = synth.uniform_points(470, 30, -7.0, 7.0)
    compacted_by_a_carve = 0
    for t, (view, image) in enumerate(pan_images):
        before = c.ring_compact_count()
        got, want = c.ring_carve_depth(view, image, P["margin"]), mirror.carve(view, image, P["margin"])
        assert got == want, f"frame {t}: carved {got}, the model {want}"
        assert c.ring_compact_count() == (mirror.compactions if auto else 0), f"frame {t}: compactions"
        compacted_by_a_carve += c.ring_compact_count() - before
        assert len(c) == mirror.count, f"frame {t}: size after the carve"
        _, kept = c.append_depth(view, image)
        assert kept == int(mirror.append_depth(view, image)[1].sum()), f"frame {t}: kept"
        check_counts(c, mirror, f"frame {t}")
        _, _, xyz = c.radius_crop((0.0, 0.0, 0.0), 1.0e4)                   # the live rows in slot order
        assert np.array_equal(xyz, mirror.live()[mirror.live_mask()]), f"frame {t}: live rows"
        ki, kd = ref_knn(mirror.live(), q, 1)
        gi, gd = c.nn(q)
        assert np.array_equal(gd, kd[:, 0]) and np.array_equal(gi, ki[:, 0]), f"frame {t}: NN"
    assert compacted_by_a_carve == (12 if auto else 0) and mirror.live_count() == (3072 if auto else mirror.live_count())
    c.close()


# ---- 7. captured plans -------------------------------------------------------------------------------------------------------------

def test_plans_captured_before_the_removals_and_the_compaction_answer_after_them(E, oracle):
    window, frame = 6000, 1500
    P = S.C5_PARAMS
    c, w = E.Cloud(window), K.CompactWindow(window)
    c.ring_index(2.0, (70.0, 70.0, 8.0))
    for k in range(5):                                      # wrapped: the cursor at slot 1500
        f = S.c5_frame_clustered(k, frame)
        c.append(f)
        w.append_plain(f)
    replan = E.ReplanPlan(c, S.C5_NODES, 128, S.C5_SEGMENTS)
    q = np.concatenate([synth.uniform_points(480, 100, -30.0, 30.0) * np.float32([1, 1, 0.1]), w.live()[::61][:28]]).astype(np.float32)
    nnplan = E.NNPlan(c, len(q))

    def ask(k, tag):
        live = w.live_mask()
        rows = np.flatnonzero(live)
        ki, kd = ref_knn(w.live(), q, 1)
        i, d = nnplan.run(q)
        assert np.array_equal(d, kd[:, 0]) and np.array_equal(i, ki[:, 0]), f"{tag}: the NN plan"
        start, nodes, coef, T, od = S.c5_tick_queries(k)
        prm = E.inflate_params(start, P["sample_range"], P["search_margin"], P["max_radius"])
        got = replan.run(prm, nodes, coef, T, od, 0.0, 2.0, 0.02, want_nn=True)
        ref = oracle.replan_tick(w.live()[live], start, P["sample_range"], P["search_margin"], P["max_radius"], nodes, coef, T, od, 0.0, 2.0, 0.02)
        slot_of = lambda a: np.where(a < 0, np.int64(NO_INDEX), rows[np.maximum(a, 0)] if len(rows) else np.int64(NO_INDEX))
        assert got["nsamples"] == ref["nsamples"] and got["nctrl"] == ref["nctrl"], tag
        assert np.array_equal(got["node_radius"], ref["node_radius"]) and np.array_equal(got["node_d2"], ref["node_d2"]), f"{tag}: node radii"
        assert np.array_equal(got["node_idx"].astype(np.int64), slot_of(ref["node_idx"])), f"{tag}: node indices"
        assert np.array_equal(got["ctrl_radius"], ref["ctrl_radius"]) and got["first_hit_ctrl"] == ref["first_hit_ctrl"], f"{tag}: control points"
        same = np.all(got["sample_pos"].astype(np.float32) == ref["sample_pos"].astype(np.float32), axis=1)
        assert same.any() and np.array_equal(got["sample_radius"][same], ref["sample_radius"][same]), f"{tag}: samples"

    ask(5, "before")
    centre = (0.5, 0.0, 2.5)
    assert c.ring_remove_ball(centre, 12.0) == w.remove_ball(centre, 12.0) > 0
    assert c.ring_remove_ball(centre, 25.0, outside=True) == w.remove_ball(centre, 25.0, outside=True) > 0
    ask(5, "after the removals")
    live, reclaimed = c.ring_compact()
    assert (live, reclaimed) == w.compact()[:2] and 0 < live < window
    ask(5, "after the compaction")                          # same graphs: no re-capture
    ask(6, "after the compaction, next tick")
    f = S.c5_frame_clustered(6, frame)
    c.append(f)
    w.append_plain(f)
    assert w.nxt == (live + frame) % window
    ask(6, "after an append into the reclaimed slots")
    replan.close()
    nnplan.close()
    c.close()


# ---- 8. right behind / in front of an append ---------------------------------------------------------------------------------------

def test_a_compaction_behind_an_append_sees_the_frame_and_an_append_behind_it_lands_at_slot_L(E):
    cap = 3000
    c, w = ring_cloud(E, cap), K.CompactWindow(cap)
    f0 = synth.uniform_points(490, 1500, 0.0, 10.0)
    c.append(f0)
    w.append_plain(f0)
    assert c.ring_remove_ball((5, 5, 5), 4.0) == w.remove_ball((5, 5, 5), 4.0) > 0
    f1 = synth.uniform_points(491, 1200, 0.0, 10.0)
    c.append(f1)                                            # a copied frame: the call returns before its insert kernel has run
    live, reclaimed = c.ring_compact()
    w.append_plain(f1)
    assert (live, reclaimed) == w.compact()[:2] and live > 1200
    f2 = synth.uniform_points(492, 300, 0.0, 10.0)
    c.append(f2)                                            # queued behind the compaction's launches
    w.append_plain(f2)
    i, d = c.nn(f2)
    assert np.all(d == 0.0) and np.array_equal(i, live + np.arange(300, dtype=np.uint32)), "the frame behind the compaction starts at slot L"
    i, d = c.nn(f1)
    assert np.all(d == 0.0) and np.array_equal(i, live - 1200 + np.arange(1200, dtype=np.uint32)), "the frame in flight was compacted with the window"
    check_counts(c, w, "at the end")
    check_knn(E, c, w, queries(493, w), "at the end")
    check_slots(c, w, "at the end")
    c.close()


# ---- 9. errors ---------------------------------------------------------------------------------------------------------------------

def test_errors(E):
    L = E.lib()
    plain = E.Cloud(100)
    plain.set_input(synth.uniform_points(496, 50, 0.0, 1.0))
    for call in (lambda: plain.ring_compact(), lambda: plain.ring_compact(want_remap=True), lambda: plain.ring_autocompact(0.5)):
        with pytest.raises(E.EngineError) as ei:
            call()                                          # no rolling-map index
        assert ei.value.code == 2
    assert len(plain) == 50 and plain.ring_compact_count() == 0
    plain.close()
    c = ring_cloud(E, 100)
    assert c.ring_compact() == (0, 0)                        # an empty cloud: zeros
    live, reclaimed, remap = c.ring_compact(want_remap=True)
    assert (live, reclaimed, len(remap)) == (0, 0, 0)
    pts = synth.uniform_points(497, 60, 0.0, 1.0)
    c.append(pts)
    assert c.ring_remove_indices(np.arange(0, 60, 2)) == 30
    a, b = C.c_int64(-1), C.c_int64(-1)
    short = np.full(59, 7, np.uint32)
    assert L.pct_cloud_ring_compact(c.handle, C.byref(a), C.byref(b), short.ctypes.data_as(C.c_void_p), 59) == 2
    assert len(c) == 60 and c.ring_live() == (30, 30) and np.all(short == 7) and c.ring_compact_count() == 0, "a refused call changes nothing"
    assert L.pct_cloud_ring_compact(None, C.byref(a), C.byref(b), None, 0) == 2
    n = C.c_uint64(5)
    assert L.pct_cloud_ring_compact_count(None, C.byref(n)) == 2 and L.pct_cloud_ring_compact_count(c.handle, None) == 2
    assert L.pct_cloud_ring_autocompact(None, 0.5) == 2
    for f in (-0.1, 1.5, float("nan"), float("inf"), -float("inf")):
        with pytest.raises(E.EngineError) as ei:
            c.ring_autocompact(f)
        assert ei.value.code == 2
    assert L.pct_cloud_ring_compact(c.handle, None, None, None, 0) == 0          # live and reclaimed may be NULL
    assert len(c) == 30 and c.ring_live() == (30, 0) and c.ring_compact_count() == 1
    i, d = c.nn(pts[1::2])
    assert np.all(d == 0.0) and np.array_equal(i, np.arange(30, dtype=np.uint32))
    # the mode: on at 1.0 only a wholly dead capacity would compact; ring_drop turns it off
    c.ring_autocompact(0.1)
    assert c.ring_remove_indices(np.arange(0, 9)) == 9 and len(c) == 30          # 9 dead < 0.1 * 100
    assert c.ring_remove_indices([9]) == 1 and len(c) == 20 and c.ring_compact_count() == 2
    c.ring_drop()
    c.ring_index(0.25, EXTENT)
    assert c.ring_remove_indices(np.arange(0, 15)) == 15 and len(c) == 20 and c.ring_compact_count() == 2, "ring_drop turns the mode off"
    c.close()


# ---- 10. corridor ------------------------------------------------------------------------------------------------------------------

def test_corridor_on_the_lidar_window_with_auto_compaction_matches_the_cpu_finder(oracle):
    """test_corridor_on_the_lidar_window_matches_the_cpu_finder_in_lidar_mode with setRollingCompact on: the window is compacted behind
    the forgetOutside of every frame that forgets enough, and the corridor is still the CPU finder's, bit for bit"""
    from pointcloudtraj_amd import corridor, engine
    engine.init(0)
    window = 40000
    info_ref, info = {}, {}
    want = S.run_lidar_window_scenario(oracle.PortCorridor(), window, info=info_ref)
    finder = corridor.SafeRegionRrtStar(window)
    finder.enableRollingMap()
    finder.setRollingDedup(M.RES)
    finder.setRollingCompact(1.0e-4)                        # 4 dead slots
    finder.setSpeculation(64)
    got = S.run_lidar_window_scenario(finder, window, info=info)
    compactions = finder.cloud().ring_compact_count()
    print(f"frames {info['frames']}, forgotten {info['forgotten']}, compactions {compactions}")
    assert info["frames"] == info_ref["frames"] and sum(info["forgotten"]) >= 4 and compactions >= 1
    assert finder.cloud().ring_live()[1] < 4, "fewer dead slots than the threshold are left"
    assert len(got) == len(want) >= 11
    for k, ((pg, rg, sg), (pw, rw, sw)) in enumerate(zip(got, want)):
        assert sg == sw, f"phase {k}: {sg} vs {sw}"
        assert np.array_equal(pg, pw) and np.array_equal(rg, rw), f"phase {k}: the corridors differ"
    dead = finder.cloud().ring_live()[1]
    assert finder.compactWindow() == dead and finder.cloud().ring_live()[1] == 0
    finder.close()
