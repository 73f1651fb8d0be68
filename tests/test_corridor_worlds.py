"""Corridor finder against the CPU restatement (oracle.PortCorridor) on small worlds, WHOLE TREES: after every planner phase the
route, the status and every live sphere -- centre, radius, g, f, parent, flags, in insertion order -- are equal bit for bit, on
every expansion path (one by one, staged, fused; speculation 1 / 7 / 256), every index kind (cell index, none, rolling map) and both
tiers of the single tree queries (host scan, device kernels).  The worlds are tests/helpers/corridor_worlds.py.

CPU: the worlds are pinned on the oracle alone (a route where one is expected, none where none can be, the tree sizes the GPU tests
rely on), so that a GPU test cannot pass vacuously."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import corridor_worlds as W  # noqa: E402

from pointcloudtraj_amd import synth  # noqa: E402
from pointcloudtraj_amd.scenarios import PARAMS  # noqa: E402

EXPANSION_PATHS = [(1, False), (1, True), (7, True), (256, True), (7, False), (256, False)]
ROOM_CROWDED = 3000          # iterations in the sealed room: 929 spheres on the oracle, neighbourhoods of more than 256 candidates
ROOM_ACROSS = 13000          # 4124 spheres on the oracle (3821 at 12000): the tree crosses the host threshold of 4096 nodes

_want = {}


def want(oracle, key, make):
    """the oracle's run for `key`, computed once and left unchanged"""
    if key not in _want:
        _want[key] = make(oracle.PortCorridor())
    return _want[key]


def wall_for(w):
    """the closed wall in the frame of world `w` (door or door_far)"""
    shift = np.float64(W.FAR if w.name == "door_far" else (0.0, 0.0, 0.0))
    return (W.wall_cloud().astype(np.float64) + shift).astype(np.float32)


def want_plan(oracle, name, expand=None):
    w = W.world(name)
    return want(oracle, ("plan", name, expand), lambda f: W.run_plan(f, w.cloud, w, expand=expand))


def want_scenario(oracle, name, scenario, kind):
    w = W.world(name)
    if scenario == "wall":
        return want(oracle, (name, scenario, kind), lambda f: W.run_replan(f, w.cloud, wall_for(w), w, kind=kind))
    if scenario == "pinch":
        return want(oracle, (name, scenario, kind), lambda f: W.run_replan(f, w.cloud, W.pinch_frame, w, kind=kind))
    return want(oracle, (name, scenario, kind), lambda f: (W.run_commits(f, w.cloud, w, kind=kind), None))


# ---- CPU: the worlds, on the oracle alone ----------------------------------------------------------------------------------------
def test_world_clouds_are_what_the_tests_assume():
    sizes = {n: len(W.world(n).cloud) for n in W.PLAN_WORLDS + ("room",)}
    assert sizes["empty"] == sizes["goal_in_start"] == 0 and sizes["wall"] == 2511 and sizes["room"] == 7440, sizes
    assert sizes["door"] == sizes["door_far"] == 2511 - 23 * 31 and 40 <= sizes["open"] == sizes["lowceiling"] <= 60, sizes
    for n in W.PLAN_WORLDS + ("room",):
        w = W.world(n)
        assert w.cloud.dtype == np.float32 and w.cloud.shape == (sizes[n], 3)
        shift = np.float64(W.FAR if n == "door_far" else (0.0, 0.0, 0.0))
        on = (np.round((w.cloud.astype(np.float64) - shift) * 10.0) / 10.0 + shift).astype(np.float32)
        assert np.array_equal(on, w.cloud), f"{n}: every point is the fp32 value of a 0.1 m lattice point"
        assert len(np.unique(w.cloud, axis=0)) == len(w.cloud), f"{n}: no point twice"
    door = W.door_cloud()
    assert np.abs(door[:, 1]).min() == np.float32(1.2) and not np.any(door[:, 0])
    far = W.world("door_far")
    assert np.array_equal(far.cloud, (door.astype(np.float64) + np.float64(W.FAR)).astype(np.float32))
    assert not np.array_equal(far.cloud.astype(np.float64), door.astype(np.float64) + np.float64(W.FAR)), "the shift must round in fp32"


def test_oracle_finds_what_each_world_holds(oracle):
    ph = want_plan(oracle, "open")
    assert ph[0][2]["path_exists"] and ph[1][2]["path_exists"]
    ph = want_plan(oracle, "empty")
    assert ph[1][2]["path_exists"] and ph[1][2]["nodes"] == 33
    ph = want_plan(oracle, "wall")
    assert not ph[0][2]["path_exists"] and not ph[1][2]["path_exists"] and ph[0][2]["nodes"] >= 250
    assert np.array_equal(ph[0][0], np.eye(3)) and not np.any(ph[0][1]), "no route: the reference's placeholder"
    for name in ("door", "door_far"):
        ph = want_plan(oracle, name)
        assert ph[1][2]["path_exists"] and len(ph[1][0]) >= 5
        x0 = W.world(name).start[0] + 3.0
        gap = np.abs(ph[1][0][:, 0] - x0).argmin()
        assert abs(ph[1][0][gap, 1] - (W.world(name).start[1] + 3.0)) < 1.2, "the route crosses the wall's plane inside the gap"
    ph = want_plan(oracle, "lowceiling")
    assert ph[1][2]["path_exists"]
    low = want_plan(oracle, "lowceiling")[1][3]["centre"][:, 2]
    assert low.max() <= 1.5 and low.min() < 0.7, "the tree stays under the ceiling and reaches under the start"
    ph = want_plan(oracle, "goal_in_start")
    assert ph[0][2]["path_exists"] and len(ph[0][0]) == 1, "the root alone is the route"


def test_oracle_replans_and_commits(oracle):
    for name in ("door", "door_far"):
        ph, _ = want_scenario(oracle, name, "wall", "grid")
        assert ph[1][2]["path_exists"] and not ph[2][2]["path_exists"] and not ph[3][2]["path_exists"], "the closed wall loses the route for good"
        ph, frame = want_scenario(oracle, name, "pinch", "grid")
        assert len(frame) == len(W.world(name).cloud) + 1
        assert ph[1][2]["path_exists"] and not ph[2][2]["path_exists"], "the pinch point breaks the route in Evaluate"
        if name == "door":
            assert ph[3][2]["path_exists"], "Refine(200) finds a route again"
        assert ph[3][2]["nodes"] > ph[2][2]["nodes"]
        ph, _ = want_scenario(oracle, name, "commits", "grid")
        assert (len(ph) - 2) // 3 >= 2, "at least two commits"
        assert not np.array_equal(ph[-1][0][0], ph[1][0][0]), "the route's first centre moves with the root"


def test_oracle_room_fills_up(oracle):
    ph = want_plan(oracle, "room")
    assert not ph[0][2]["path_exists"] and ph[0][2]["nodes"] >= 800
    ph = want_plan(oracle, "room", ROOM_ACROSS)
    assert not ph[0][2]["path_exists"] and ph[0][2]["nodes"] > 4096
    # the crowding the truncated-list test relies on: some sphere's neighbourhood (2 x radius) holds more than 256 others
    t = want_plan(oracle, "room")[0][3]
    c = t["centre"].astype(np.float32).astype(np.float64)
    busiest = max(int((np.linalg.norm(c - c[i], axis=1) <= 2.0 * t["radius"][i]).sum()) for i in range(0, len(c), 7))
    assert busiest > 256, busiest


def test_oracle_tree_holds_the_route(oracle):
    """orrt_get_tree against getPath: following `parent` from the goal-touching sphere on the route's end gives the route"""
    for name in ("open", "door", "door_far", "lowceiling", "goal_in_start"):
        w = W.world(name)
        path, radius, status, t = want_plan(oracle, name)[1]
        assert len(t["radius"]) == status["nodes"] and np.all(t["flags"] & 1)
        assert np.all(t["parent"] < len(t["parent"])) and (t["parent"] == -1).sum() >= 1
        tips = [i for i in range(len(t["radius"])) if np.array_equal(t["centre"][i], path[-1]) and t["radius"][i] == np.float32(radius[-1])]
        assert tips, name
        i, chain = tips[0], []
        while i != -1:
            chain.append(i)
            i = int(t["parent"][i])
        chain.reverse()
        assert np.array_equal(t["centre"][chain], path) and np.array_equal(t["radius"][chain].astype(np.float64), radius), name
        assert np.linalg.norm(path[-1] - np.float64(w.goal)) + 0.1 < radius[-1], "the tip touches the goal"
        assert t["g"][chain[0]] == 0 and np.all(np.diff(t["g"][chain]) > 0), "cost grows along the route"


def test_oracle_runs_are_reproducible(oracle):
    for name in W.PLAN_WORLDS:
        w = W.world(name)
        W.same_phases(W.run_plan(oracle.PortCorridor(), w.cloud, w), want_plan(oracle, name), f"{name}, second run")
    w = W.world("door")
    again, _ = W.run_replan(oracle.PortCorridor(), w.cloud, W.pinch_frame, w)
    W.same_phases(again, want_scenario(oracle, "door", "pinch", "grid")[0], "door pinch, second run")
    W.same_phases(W.run_commits(oracle.PortCorridor(), w.cloud, w), want_scenario(oracle, "door", "commits", "grid")[0], "door commits, second run")


def margin_probes(cloud):
    """points exactly search_margin away from a lattice point of `cloud` along each axis, where no other point is nearer (out of the
    wall's plane; into the gap from its edge; above its top row), and the same points one fp32 step closer.  Every coordinate is an
    fp32 value, so the narrowing of the query to float (corridor_finder.cpp:117-119) changes nothing and the distance is exact."""
    m = PARAMS["search_margin"]
    edge = cloud[(cloud[:, 1] == np.float32(1.2)) & (cloud[:, 2] == np.float32(1.0))][0].astype(np.float64)
    top = cloud[(cloud[:, 1] == np.float32(2.0)) & (cloud[:, 2] == np.float32(3.0))][0].astype(np.float64)
    at = np.array([edge + [m, 0, 0], edge - [m, 0, 0], edge - [0, m, 0], top + [0, 0, m]])
    assert np.array_equal(at, at.astype(np.float32).astype(np.float64))
    assert np.array_equal(np.abs(at - np.array([edge, edge, edge, top])).sum(1), np.full(4, m)), "the offsets are exact"
    nearer = at.astype(np.float32)
    nearer[0, 0] = np.nextafter(nearer[0, 0], np.float32(0)); nearer[1, 0] = np.nextafter(nearer[1, 0], np.float32(0))
    nearer[2, 1] = np.nextafter(nearer[2, 1], np.float32(9)); nearer[3, 2] = np.nextafter(nearer[3, 2], np.float32(0))
    return at, nearer.astype(np.float64)


def traj_points():
    return synth.uniform_points(9, 200, -4.0, 4.0).astype(np.float64)


def prepared(f, name):
    w = W.world(name)
    p = PARAMS
    f.setParam(p["safety_margin"], p["search_margin"], p["max_radius"], p["sensing_range"])
    f.setInput(w.cloud)
    f.reset()
    f.setPt(w.start, w.goal, *w.box, p["sensing_range"], p["max_samples"], p["sample_portion"], p["goal_portion"])
    return f


def test_oracle_check_traj_pt_col_is_strict_at_the_margin(oracle):
    f = prepared(oracle.PortCorridor(), "door")
    at, nearer = margin_probes(W.door_cloud())
    assert [f.checkTrajPtCol(q) for q in at] == [False] * 4, "radius == 0 is not < 0"
    assert [f.checkTrajPtCol(q) for q in nearer] == [True] * 4, "one fp32 step closer collides"
    hits = [f.checkTrajPtCol(q) for q in traj_points()]
    assert 0 < sum(hits) < 200, "the random points fall on both sides"
    e = prepared(oracle.PortCorridor(), "empty")
    assert not any(e.checkTrajPtCol(q) for q in traj_points())


# ---- GPU -------------------------------------------------------------------------------------------------------------------------
def gpu_finder(speculation, fused):
    from pointcloudtraj_amd import corridor, engine
    engine.init(0)
    f = corridor.SafeRegionRrtStar(W.WINDOW)
    f.setSpeculation(speculation)
    f.setFusedExpansion(fused)
    return f


@pytest.mark.gpu
@pytest.mark.parametrize("kind", W.INDEX_KINDS)
@pytest.mark.parametrize("speculation,fused", EXPANSION_PATHS)
@pytest.mark.parametrize("name", W.PLAN_WORLDS)
def test_worlds_match_oracle(oracle, name, speculation, fused, kind):
    w = W.world(name)
    f = gpu_finder(speculation, fused)
    got = W.run_plan(f, w.cloud, w, kind=kind)
    W.same_phases(got, want_plan(oracle, name), f"{name}, speculation {speculation}, fused {fused}, index {kind}")
    dbg = f.debugCounters()
    assert dbg["max_kd_size"] >= got[-1][2]["nodes"]
    if kind == "none" and len(w.cloud) > 0:      # an empty cloud has no index to lack: the fused launch serves it (kdtree_ext.h)
        assert f.expansionLaunches() == 0
        assert (dbg["fused_refused"] >= 1) == fused, dbg
    else:
        assert (f.expansionLaunches() > 0) == fused and dbg["fused_refused"] == 0, dbg
    if (speculation, fused) == (1, False):
        assert dbg["grow_one"] == w.expand + w.refine, dbg
    f.close()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["grid", "rolling"])
@pytest.mark.parametrize("speculation", [1, 256])
@pytest.mark.parametrize("scenario", ["wall", "pinch", "commits"])
@pytest.mark.parametrize("name", ["door", "door_far"])
def test_replans_and_commits_match_oracle(oracle, name, scenario, speculation, kind):
    w = W.world(name)
    ref, frame = want_scenario(oracle, name, scenario, kind)
    f = gpu_finder(speculation, True)
    if scenario == "commits":
        got = W.run_commits(f, w.cloud, w, kind=kind)
    else:
        got, _ = W.run_replan(f, w.cloud, frame if scenario == "pinch" else wall_for(w), w, kind=kind)
    W.same_phases(got, ref, f"{name}, {scenario}, speculation {speculation}, index {kind}")
    if scenario == "wall":
        assert f.repairBatches() > 0
    f.close()


@pytest.mark.gpu
@pytest.mark.parametrize("fused", [True, False])
def test_crowded_room_truncated_neighbourhoods(oracle, fused):
    """more than cap = 256 candidates in a neighbourhood: the list comes back truncated and the finder asks kd_nearest_rangef"""
    w = W.world("room")
    f = gpu_finder(256, fused)
    got = W.run_plan(f, w.cloud, w, expand=ROOM_CROWDED)
    W.same_phases(got, want_plan(oracle, "room"), f"room, {ROOM_CROWDED} iterations, fused {fused}")
    assert f.debugCounters()["truncated_lists"] > 0, f.debugCounters()
    f.close()


@pytest.mark.gpu
@pytest.mark.parametrize("speculation,fused", [(1, False), (256, True)])
def test_single_tree_queries_on_the_device_under_the_finder(oracle, speculation, fused):
    """kd_nearestf / kd_nearest_rangef answered by the kernels (host threshold 0) as the finder uses them: in the one-by-one loop, in
    the fallbacks of truncated lists, in treeRepair, interleaved with inserts, kd_refresh and rebuilds"""
    from pointcloudtraj_amd import kdtree
    room, door = W.world("room"), W.world("door")
    old = kdtree.host_threshold()
    kdtree.set_host_threshold(0)
    try:
        f = gpu_finder(speculation, fused)
        got = W.run_plan(f, room.cloud, room, expand=ROOM_CROWDED)
        W.same_phases(got, want_plan(oracle, "room"), f"room on the device tier, speculation {speculation}, fused {fused}")
        if speculation > 1:
            assert f.debugCounters()["truncated_lists"] > 0, f.debugCounters()
        f.close()
        f = gpu_finder(speculation, fused)
        got, _ = W.run_replan(f, door.cloud, wall_for(door), door)
        W.same_phases(got, want_scenario(oracle, "door", "wall", "grid")[0], f"door -> wall on the device tier, speculation {speculation}, fused {fused}")
        assert f.repairBatches() > 0
        f.close()
    finally:
        kdtree.set_host_threshold(old)


@pytest.mark.gpu
def test_tree_crosses_the_host_threshold(oracle):
    """the same tree answered from the host copy below 4096 nodes and by the kernels above, in one run"""
    from pointcloudtraj_amd import kdtree
    assert kdtree.host_threshold() == 4096
    w = W.world("room")
    f = gpu_finder(256, True)
    got = W.run_plan(f, w.cloud, w, expand=ROOM_ACROSS)
    assert f.debugCounters()["max_kd_size"] > 4096, f.debugCounters()
    W.same_phases(got, want_plan(oracle, "room", ROOM_ACROSS), f"room, {ROOM_ACROSS} iterations")
    f.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["door", "empty"])
def test_check_traj_pt_col_matches_oracle(oracle, name):
    from pointcloudtraj_amd import corridor, engine
    engine.init(0)
    pts = traj_points()
    if name == "door":
        pts = np.concatenate([pts, *margin_probes(W.door_cloud())])
    ref = prepared(oracle.PortCorridor(), name)
    f = prepared(corridor.SafeRegionRrtStar(W.WINDOW), name)
    wanted = [ref.checkTrajPtCol(q) for q in pts]
    got = [f.checkTrajPtCol(q) for q in pts]
    wrong = [(i, pts[i].tolist(), got[i], wanted[i]) for i in range(len(pts)) if got[i] != wanted[i]]
    assert not wrong, f"{name}: (index, point, got, oracle) {wrong[:5]}"
    assert f.status()["inflation_queries"] == ref.status()["inflation_queries"] == len(pts)
    f.close()
