"""GPU tests of the de-duplicating appends of the rolling map (pct_cloud_ring_dedup): a window of unique voxels.

Reference: the numpy restatement of the rule (tests/helpers/ring_dedup_model.py), point for point -- kept flags, counts and the
window's contents slot by slot -- and, over the model's window, the exhaustive fp64 oracle (oracle.brute_nearest_mt,
oracle.replan_tick, oracle.PortCorridor).  Everything is exact; there are no tolerances."""
import os
import sys

import numpy as np
import pytest

from pointcloudtraj_amd import scenarios as S, synth

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import ring_dedup_model as M  # noqa: E402

pytestmark = pytest.mark.gpu

EXTENT = (14.0, 14.0, 10.0)


@pytest.fixture(scope="module")
def E():
    from pointcloudtraj_amd import engine
    engine.init(0)
    return engine


@pytest.fixture(scope="module")
def runs():
    """the model's run of both scenarios, computed once and left unchanged: per scenario the frames, the kept flags and the window
    size after every frame, and a copy of the window after every fifth frame"""
    out = {}
    for name, sc in M.SCENARIOS.items():
        frames = M.frames_of(name)
        w = M.DedupWindow(sc["cap"], M.RES)
        flags, counts, snaps = [], [], {}
        for t, f in enumerate(frames):
            flags.append(w.append(f))
            counts.append(w.count)
            if t % 5 == 4:
                snaps[t] = w.live().copy()
        out[name] = dict(frames=frames, flags=flags, counts=counts, snaps=snaps, filed=w.filed, final=w.live().copy())
    return out


def queries(name, t, n=300):
    s = M.SCENARIOS[name]["step"] * t
    return (synth.uniform_points(900 + t, n, -4.0, 4.0) + np.float32([S.START[0] + s, S.START[1] + s, S.START[2]])).astype(np.float32)


def check_nn(E, c, window, q, oracle, tag):
    bi, bd = oracle.brute_nearest_mt(window, q)
    for algo in (E.ALGO_AUTO, E.ALGO_STREAM):
        i, d = c.nn(q, algo)
        assert np.array_equal(d, bd), f"{tag}: d2 (algo {algo})"
        assert np.array_equal(i.astype(np.int64), bi.astype(np.int64)), f"{tag}: idx (algo {algo})"


def feed(E, oracle, name, run, after_frame=None):
    """scenario `name` through a de-duplicating cloud: flags, kept and the window size against the model per frame, NN against the
    oracle over the model's window after every fifth frame; returns the cloud"""
    sc = M.SCENARIOS[name]
    c = E.Cloud(sc["cap"])
    c.ring_index(0.25, EXTENT)
    c.ring_dedup(M.RES)
    offered = kept = zero = 0
    for t, f in enumerate(run["frames"]):
        c.append(f)
        last = c.ring_dedup_last()
        want = run["flags"][t]
        offered += len(f)
        kept += int(want.sum())
        zero += len(f) > 0 and not want.any()
        assert last["offered"] == len(f) and last["kept"] == int(want.sum()), f"{name} frame {t}: {last['kept']} kept, the model keeps {int(want.sum())}"
        assert np.array_equal(last["flags"], want), f"{name} frame {t}: kept flags"
        assert len(c) == run["counts"][t], f"{name} frame {t}: window size"
        assert (last["total_offered"], last["total_kept"]) == (offered, kept)
        if t in run["snaps"]:
            check_nn(E, c, run["snaps"][t], queries(name, t), oracle, f"{name} frame {t}")
        if after_frame:
            after_frame(c, t, f)
    assert kept == run["filed"]
    return c, zero


def test_scenario_a_matches_the_model_and_keeps_the_buckets_small(E, oracle, runs):
    """window 12 000, 3 m sensor, 0.1 m per frame, 60 frames: 129 922 points offered, 6 438 filed, 15 frames without a survivor"""
    run = runs["A"]

    def searches(c, t, f):
        if t % 5 != 4:
            return
        q = queries("A", t)
        ki, kd = c.knn(q, 8)
        si, sd = c.knn(q, 8, E.ALGO_STREAM)
        assert np.array_equal(ki, si) and np.array_equal(kd, sd), f"frame {t}: k-NN through the ring index"
        assert np.array_equal(c.radius_count(q, 0.5), c.radius_count(q, 0.5, E.ALGO_STREAM)), f"frame {t}: radius counts"

    c, zero = feed(E, oracle, "A", run, searches)
    assert zero == 15 and run["filed"] == 6438
    info = c.ring_info()
    assert info["overflow_entries"] == 0 and info["bucket_records"] == 32, info
    c.close()
    # The same frames without de-dup: up to 145 records in one 0.25 m cell where the de-duplicated window has at most 15, so the
    # 32-record buckets spill to the overflow queue.  The queue is looked at after every frame, not only at the end: once it
    # holds more than window / 128 + 4096 entries (frames 35-41: about 5 000 by the CPU model) the library doubles the buckets
    # and files the window again, which empties the queue -- at the end the plain window shows its spill as 64-record buckets.
    p = E.Cloud(M.SCENARIOS["A"]["cap"])
    p.ring_index(0.25, EXTENT)
    spilled = 0
    for f in run["frames"]:
        p.append(f)
        now = p.ring_info()
        if now["bucket_records"] == 32:
            spilled = max(spilled, now["overflow_entries"])
    end = p.ring_info()
    assert spilled > 0, "the plain window must have spilled its 32-record buckets"
    assert end["overflow_entries"] > 0 or end["bucket_records"] > 32, end
    p.close()


def test_scenario_b_wraps_and_keeps_every_sensed_voxel(E, oracle, runs):
    """window 8 000, 2.5 m sensor, 0.2 m per frame, an empty frame in the stream: 11 774 points filed (the window wraps, keys reach two
    copies); after every append the keys of the frame are a subset of the keys of the window as the device holds it"""
    run = runs["B"]
    assert run["filed"] == 11774 > M.SCENARIOS["B"]["cap"] and any(len(f) == 0 for f in run["frames"])

    def invariant(c, t, f):
        _, _, xyz = c.radius_crop(S.START, 1.0e4)             # the whole window, read back from the device
        assert len(xyz) == len(c)
        keyed, k = M.keys_of(xyz, M.RES)
        have = set(map(tuple, k[keyed]))
        keyed, k = M.keys_of(f, M.RES)
        assert set(map(tuple, k[keyed])) <= have, f"frame {t}: a sensed voxel is missing from the window"

    c, _ = feed(E, oracle, "B", run, invariant)
    _, _, xyz = c.radius_crop(S.START, 1.0e4)
    assert np.array_equal(xyz, run["final"])                  # slot by slot: the crop keeps the cloud's order
    c.close()


def test_a_frame_of_identical_points_keeps_one(E, oracle):
    cap = 3000
    c = E.Cloud(cap)
    c.ring_index(0.25, EXTENT)
    c.ring_dedup(M.RES)
    c.append(np.tile(np.float32([[1.23, -0.4, 2.0]]), (cap, 1)))       # n == cap
    last = c.ring_dedup_last()
    assert (last["offered"], last["kept"], len(c)) == (cap, 1, 1) and last["flags"][0] and not last["flags"][1:].any()
    c.append(np.tile(np.float32([[1.23, -0.4, 2.0]]), (cap, 1)))       # its only holder is doomed by an append of cap points
    assert c.ring_dedup_last()["kept"] == 1 and len(c) == 2
    c.append(np.tile(np.float32([[1.23, -0.4, 2.0]]), (5, 1)))         # now two holders outside the five doomed slots
    assert c.ring_dedup_last()["kept"] == 0 and len(c) == 2
    c.close()


@pytest.mark.parametrize("table_first", [True, False])
def test_keyless_points_are_all_kept_and_searchable(E, oracle, table_first):
    """NaN / inf / 1e30 points are kept every time, exactly as plain appends treat them; table_first = False: the cloud's table does
    not exist yet and the first (filtered) frame sizes it"""
    cap = 4000
    wild = np.float32([[np.nan, 1, 1], [1, np.inf, 1], [1e30, 0, 0], [0, -1e30, 0], [2.0e6, 0, 0]])
    base = synth.uniform_points(71, 600, 0.0, 6.0)
    f = np.concatenate([wild[:2], base, base[:200], wild[2:], wild])
    first = f if table_first else np.concatenate([base, base[:200]])     # a table sized from its first data needs that data finite
    w = M.DedupWindow(cap, M.RES)
    c, p = E.Cloud(cap), E.Cloud(cap)                                   # p: a plain rolling map fed the kept points
    for x in (c, p):
        x.ring_index(0.25, EXTENT) if table_first else x.ring_index()
    c.ring_dedup(M.RES)
    assert c.has_ring_index == table_first
    q = np.concatenate([synth.uniform_points(72, 200, -1.0, 7.0), np.float32([[1e30, 0, 0], [2.0e6, 1, 0]])])
    for rep, g in enumerate((first, f, np.concatenate([f, synth.uniform_points(73, 300, 0.0, 6.0)]))):
        want = w.append(g)
        if g is not first or table_first:
            assert want[[0, 1]].all() and want[len(f) - 8:len(f)].all()  # every keyless point, every time
        c.append(g)
        p.append(g[want])
        last = c.ring_dedup_last()
        assert np.array_equal(last["flags"], want) and len(c) == w.count == len(p), rep
        for algo in (E.ALGO_AUTO, E.ALGO_STREAM):
            ic, dc = c.nn(q, algo)
            ip, dp = p.nn(q, algo)
            assert np.array_equal(ic, ip) and np.array_equal(dc, dp), (rep, algo)
        finite = np.isfinite(w.live()).all(axis=1)
        bi, bd = oracle.brute_nearest_mt(w.live()[finite], q[:200])
        assert np.array_equal(c.nn(q[:200])[1], bd)
        assert np.array_equal(np.flatnonzero(finite)[bi], c.nn(q[:200])[0].astype(np.int64))
    assert c.has_ring_index
    c.close()
    p.close()


def test_zero_copy_frames_give_the_same_flags(E, oracle):
    frames = M.frames_of("A")[:12]
    cap = M.SCENARIOS["A"]["cap"]
    a, b = E.Cloud(cap), E.Cloud(cap)
    for x in (a, b):
        x.ring_index(0.25, EXTENT)
        x.ring_dedup(M.RES)
    buf = b.frame_buffer(max(map(len, frames)))
    for t, f in enumerate(frames):
        a.append(f)
        buf[:len(f)] = f
        b.append_frame(len(f))
        la, lb = a.ring_dedup_last(), b.ring_dedup_last()
        assert la["kept"] == lb["kept"] and np.array_equal(la["flags"], lb["flags"]) and len(a) == len(b), t
        buf[:] = 0.0                                           # the producer's buffer is its own again
    q = queries("A", 11)
    assert all(np.array_equal(x, y) for x, y in zip(a.nn(q), b.nn(q)))
    a.close()
    b.close()


def test_replan_plan_captured_before_dedup_answers_after_appends_with_it(E, oracle):
    """appends with de-dup change neither the table's shape nor a pointer: the graph captured before the mode was enabled is replayed"""
    window, frame = 60_000, 8_000
    P = S.C5_PARAMS
    c, w = E.Cloud(window), M.DedupWindow(window, M.RES)
    c.ring_index()
    for k in range(4):
        f = S.c5_frame_clustered(k, frame)
        c.append(f)
        w.append_plain(f)
    plan = E.ReplanPlan(c, S.C5_NODES, 128, S.C5_SEGMENTS)
    c.ring_dedup(M.RES)
    dropped = 0
    for k in range(4, 9):
        f = S.c5_frame_clustered(k, frame)
        want = w.append(f)
        c.append(f)
        last = c.ring_dedup_last()
        assert np.array_equal(last["flags"], want) and len(c) == w.count, k
        dropped += len(f) - last["kept"]
        start, nodes, coef, T, od = S.c5_tick_queries(k)
        prm = E.inflate_params(start, P["sample_range"], P["search_margin"], P["max_radius"])
        got = plan.run(prm, nodes, coef, T, od, 0.0, 2.0, 0.02, want_nn=True)
        ref = oracle.replan_tick(w.live(), start, P["sample_range"], P["search_margin"], P["max_radius"], nodes, coef, T, od, 0.0, 2.0, 0.02)
        noidx = lambda a: np.where(a < 0, np.int64(E.NO_INDEX), a.astype(np.int64))
        assert got["nsamples"] == ref["nsamples"] and got["nctrl"] == ref["nctrl"], k
        assert np.array_equal(got["node_radius"], ref["node_radius"]) and np.array_equal(got["node_d2"], ref["node_d2"]), k
        assert np.array_equal(got["node_idx"].astype(np.int64), noidx(ref["node_idx"])), k
        assert np.array_equal(got["ctrl_radius"], ref["ctrl_radius"]) and got["first_hit_ctrl"] == ref["first_hit_ctrl"], k
        same = np.all(got["sample_pos"].astype(np.float32) == ref["sample_pos"].astype(np.float32), axis=1)
        assert np.array_equal(got["sample_radius"][same], ref["sample_radius"][same]), k
    assert dropped > 0, "the clustered frames re-sense lattice points: some must have been dropped"
    plan.close()
    c.close()


def test_errors_and_turning_the_mode_off(E, oracle):
    c = E.Cloud(5000)
    with pytest.raises(E.EngineError) as ei:
        c.ring_dedup(0.1)                                      # no rolling-map index
    assert ei.value.code == 2
    for bad in (-0.1, float("nan"), float("inf")):
        with pytest.raises(E.EngineError):
            c.ring_dedup(bad)
    c.ring_index(0.02)
    with pytest.raises(E.EngineError) as ei:
        c.ring_dedup(0.1)                                      # cells smaller than half a voxel
    assert ei.value.code == 2
    c.ring_index(0.25, EXTENT)
    c.ring_dedup(0.1)
    with pytest.raises(E.EngineError) as ei:
        c.ring_index(0.02)                                     # ... from whichever call comes second
    assert ei.value.code == 2
    assert c.has_ring_index
    with pytest.raises(E.EngineError):
        c.append(np.zeros((5001, 3), np.float32))              # judged on the offered n
    # de-dup, then off again: a plain mirror of the slots matches again
    frames = M.frames_of("A")[:4]
    w = M.DedupWindow(5000, M.RES)
    for f in frames[:2]:
        c.append(f)
        w.append(f)
    c.ring_dedup(0.0)
    with pytest.raises(E.EngineError):
        c.ring_dedup_last()                                    # the mode is off
    for f in frames[2:]:
        c.append(f)
        w.append_plain(f)
        assert len(c) == w.count
        check_nn(E, c, w.live(), queries("A", 3), oracle, "after ring_dedup(0)")
    c.ring_dedup(0.1)
    c.ring_drop()                                              # dropping the index turns the mode off
    with pytest.raises(E.EngineError):
        c.ring_dedup_last()
    c.close()


class ModelFed:
    """the CPU finder behind the rolling feed: appendInput files the frame in the model's window and hands the finder that window"""

    def __init__(self, finder, cap):
        self.finder, self.w = finder, M.DedupWindow(cap, M.RES)

    def appendInput(self, frame):
        self.w.append(frame)
        self.finder.setInput(self.w.live())

    def __getattr__(self, name):
        return getattr(self.finder, name)


def test_corridor_on_the_deduplicated_window_matches_the_cpu_finder(oracle):
    """scenarios.run_rolling_commit_scenario with setRollingDedup(0.1) against the CPU finder (oracle/rrt_port.c) fed the model's
    window per frame: Path, Radius and every status field bit for bit after every phase"""
    from pointcloudtraj_amd import corridor, engine
    engine.init(0)
    window = 40000
    ref = ModelFed(oracle.PortCorridor(), window)
    want = S.run_rolling_commit_scenario(ref, window, commits=3)
    assert window < ref.w.filed < ref.w.offered, "re-sensed points must have been dropped, and the window must have wrapped"
    finder = corridor.SafeRegionRrtStar(window)
    finder.enableRollingMap()
    finder.setRollingDedup(M.RES)
    finder.setSpeculation(64)
    got = S.run_rolling_commit_scenario(finder, window, commits=3)
    assert len(got) == len(want) == 11
    for k, ((pg, rg, sg), (pw, rw, sw)) in enumerate(zip(got, want)):
        assert sg == sw, f"phase {k}: {sg} vs {sw}"
        assert np.array_equal(pg, pw) and np.array_equal(rg, rw), f"phase {k}: the corridors differ"
    finder.close()
