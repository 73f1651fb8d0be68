"""Corridor finder on the ROLLING map (config C5): scenarios.run_rolling_commit_scenario -- sensor frames appended to a window of
40 000 points, Evaluate + Refine after every frame, five commits along the corridor.

CPU: the oracle (oracle.PortCorridor, fed setInput of a host mirror of the window) keeps a corridor through every phase.
GPU: corridor.SafeRegionRrtStar over the rolling-map index, fed appendInput, against that oracle run -- two independent
implementations; Path, Radius and every status field bit for bit after every phase, as tests/test_corridor.py on static clouds."""
import ctypes as C

import numpy as np
import pytest

from pointcloudtraj_amd.scenarios import run_rolling_commit_scenario

WINDOW = 40000
FRAMES = [24393, 31460, 26000, 24295, 28427, 29339]
REFINES = [1] + [2 + 3 * k for k in range(5)] + [4 + 3 * k for k in range(5)]      # phases that end a SafeRegionRefine
EVALUATES = [3 + 3 * k for k in range(5)]


@pytest.fixture(scope="module")
def want(oracle):
    """the oracle's run, computed once and left unchanged: (phases, info)"""
    info = {}
    phases = run_rolling_commit_scenario(oracle.PortCorridor(), WINDOW, info=info)
    return phases, info


def same_phases(got, ref, what=""):
    assert len(got) == len(ref), f"{what}: {len(got)} phases, the oracle has {len(ref)}"
    for k, ((pg, rg, sg), (pw, rw, sw)) in enumerate(zip(got, ref)):
        assert sg == sw, f"{what} phase {k}: {sg} vs {sw}"          # path_exists, global_navi, nodes, inflation_queries
        assert np.array_equal(pg, pw), f"{what} phase {k}: corridor centres differ"
        assert np.array_equal(rg, rw), f"{what} phase {k}: corridor radii differ"


def test_oracle_rolling_commit_scenario(oracle, want):
    phases, info = want
    assert info["frames"] == FRAMES
    assert info["wrapped"] and info["passed"] == sum(FRAMES) == 163914, "the window must have wrapped"
    assert len(info["window"]) == WINDOW
    assert len(phases) == 17, "all five commits must have happened"
    assert phases[0][2]["path_exists"]
    for k in REFINES:
        assert phases[k][2]["path_exists"], f"phase {k}: every Refine must end with a corridor"
    # every new frame invalidates the route (evictions and new obstacles): the repair pass and re-expansion are exercised
    assert all(not phases[k][2]["path_exists"] for k in EVALUATES)
    assert all(phases[k + 1][2]["nodes"] > phases[k][2]["nodes"] for k in EVALUATES)
    again = run_rolling_commit_scenario(oracle.PortCorridor(), WINDOW)
    same_phases(again, phases, "second oracle run")


def rolling_finder(speculation=64, fused=True):
    from pointcloudtraj_amd import corridor, engine
    engine.init(0)
    f = corridor.SafeRegionRrtStar(WINDOW)
    f.enableRollingMap()
    f.setSpeculation(speculation)
    f.setFusedExpansion(fused)
    return f


@pytest.mark.gpu
@pytest.mark.parametrize("speculation,fused", [(1, True), (64, True), (256, True), (64, False)])
def test_gpu_rolling_corridor_matches_oracle(want, speculation, fused):
    """frames through appendInput; with `fused` every speculative batch is ONE launch over the rolling-map index"""
    finder = rolling_finder(speculation, fused)
    got = run_rolling_commit_scenario(finder, WINDOW)
    same_phases(got, want[0], f"speculation {speculation} fused {fused}")
    if fused:
        assert finder.expansionLaunches() > 0, "the fused expansion step must have run on the ring-indexed cloud"
    else:
        assert finder.expansionLaunches() == 0
    assert finder.repairBatches() > 0
    finder.close()


@pytest.mark.gpu
def test_gpu_rolling_finder_still_takes_a_whole_window(want):
    """setInput on a rolling finder replaces the window (here: with the mirror, every frame): same phases as the appends"""
    finder = rolling_finder()
    got = run_rolling_commit_scenario(finder, WINDOW, feed="replace")
    same_phases(got, want[0], "setInput(mirror)")
    assert finder.expansionLaunches() > 0 and finder.repairBatches() > 0
    finder.close()


@pytest.mark.gpu
def test_gpu_rolling_c_abi_takes_pcl_records(want):
    """pct_corridor_enable_rolling / pct_corridor_append_input called as a C client would, with 16-byte pcl::PointXYZ records
    (the fourth float is padding and must not matter)"""
    from pointcloudtraj_amd import corridor, engine
    engine.init(0)
    L = corridor.lib()

    class AbiFinder(corridor.SafeRegionRrtStar):
        def appendInput(self, points):
            rec = np.full((len(points), 4), np.nan, np.float32)
            rec[:, :3] = points
            assert L.pct_corridor_append_input(self.h, rec.ctypes.data_as(C.c_void_p), C.c_int64(len(rec)), C.c_int64(16)) == 0, \
                L.pct_corridor_last_error()

    finder = AbiFinder(WINDOW)
    extent = (C.c_float * 3)(30.0, 30.0, 10.0)
    assert L.pct_corridor_enable_rolling(finder.h, C.c_float(0.0), extent) == 0, L.pct_corridor_last_error()
    finder.setSpeculation(64)
    got = run_rolling_commit_scenario(finder, WINDOW)
    same_phases(got, want[0], "C ABI")
    assert finder.expansionLaunches() > 0
    # errors come back as a status and a message, not as an exception across the boundary
    assert L.pct_corridor_append_input(finder.h, None, C.c_int64(WINDOW + 1), C.c_int64(16)) != 0
    assert L.pct_corridor_last_error()
    finder.close()
