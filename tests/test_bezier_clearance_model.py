"""The numpy restatement of the trajectory clearance (tests/helpers/bezier_clearance_model.py) on the certified check's scene, against
a dense sampling of the curves and against the certified check's own model, and on cases known by hand -- no GPU needed.  The contract:
include/pct_engine.h, paragraph "Trajectory clearance".

The scene (bezier_certify_model.scene): 300 uniform points in [0, 10)^3, 64 trajectories of three segments, orders 0..12; tol in
{0.05, 0.01}, cap in {inf, 0.5}, max_depth 16.  What the model alone gave is bezier_clearance_model.SCENE_GAVE.

One property is stated here as the contract proves it, not as first written down: for a DONE trajectory min(hi, cap) <= dense
clearance + tol.  Without a cap that is hi <= dense + tol.  With cap = 0.5 a curve whose clearance exceeds the cap retires its pieces
against the cap, and hi -- the distance at a piece end of a shallow round -- may exceed the clearance by more than tol (the model does
so for trajectories with hi > 0.5); nothing in the rule bounds it there, and the third property (hi - lo <= tol or lo >= cap - tol)
says as much."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import bezier_certify_model as CM  # noqa: E402
import bezier_clearance_model as KM  # noqa: E402

NO_INDEX = KM.NO_INDEX
# an end is a curve point rounded to fp32: half an ulp per axis below 16 m
END_ROUNDING = np.sqrt(3.0) * 2.0 ** -21


def one(pts, traj, tol, cap=np.inf, max_depth=16, piece_cap=1000):
    rec, stats = KM.clearances(pts, *KM.pack([traj]), tol, cap, max_depth, piece_cap)
    return rec[0], stats


def nowhere(r):
    return r["at_seg"] == -1 and r["at_idx"] == NO_INDEX and np.isnan(r["at_u"])


def end_point(trajs, seg, u):
    """the fp32 point (widened) of the packed batch's segment `seg` at the dyadic u, by the model's own halvings"""
    coef, seg_time, orders, _ = KM.pack(trajs)
    P = KM.world_points(coef[seg], seg_time[seg], orders[seg])
    if u == 1.0:
        return P[-1].astype(np.float32).astype(np.float64)
    lo, hi = 0.0, 1.0
    while lo != u:
        left, right = KM.halve(P)
        mid = (lo + hi) * 0.5
        if u >= mid:
            P, lo = right, mid
        else:
            P, hi = left, mid
    return P[0].astype(np.float32).astype(np.float64)


def brute_distance(pts, x, idx):
    p = np.asarray(pts, np.float32)[idx].astype(np.float64)
    d = p - x
    return np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])


# ---- the scene -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cap", KM.CAPS)
@pytest.mark.parametrize("tol", KM.TOLS)
def test_scene_brackets_hold_the_dense_clearance(tol, cap):
    rec, stats, trace = KM.scene_clearances(tol, cap)
    dense = KM.scene_dense()
    print(f"tol {tol} cap {cap}: stats {stats}, largest round {max(trace)}, statuses {np.bincount(rec['status'], minlength=3)}, "
          f"widest bracket {np.max(rec['hi'] - rec['lo'])}")
    assert (int(stats[0]), int(stats[1]), max(trace)) == KM.SCENE_GAVE[(tol, cap)] and stats[2] == 0
    assert stats[0] == len(trace) and stats[1] == sum(trace) == rec["pieces"].sum() and trace[0] == 192
    done = rec["status"] == KM.DONE
    assert done.sum() >= 32
    for t in np.nonzero(done)[0]:
        r = rec[t]
        assert r["lo"] <= dense[t], (t, r, dense[t])
        assert min(r["hi"], cap) <= dense[t] + tol, (t, r, dense[t])
        assert r["hi"] - r["lo"] <= tol or r["lo"] >= cap - tol, (t, r)
    # every status: lo is a lower bound and hi is attained at a point the dense sampling holds (the ends of depth <= 12), up to its fp32 rounding
    assert np.all(rec["lo"] <= dense) and rec["depth"].max() <= 12
    assert np.all(dense <= rec["hi"] + END_ROUNDING + 1e-12)


@pytest.mark.parametrize("tol,cap", [(0.01, np.inf), (0.05, 0.5)])
def test_scene_hi_is_the_distance_from_the_named_end_to_the_named_row(tol, cap):
    rec, _, _ = KM.scene_clearances(tol, cap)
    pts, trajs = KM.scene()
    for t, r in enumerate(rec):
        assert 3 * t <= r["at_seg"] < 3 * t + 3 and r["at_idx"] < len(pts)
        x = end_point(trajs, int(r["at_seg"]), float(r["at_u"]))
        assert r["hi"] == brute_distance(pts, x, int(r["at_idx"])), (t, r)
        assert r["hi"] == np.sqrt(KM.nearest(pts, x[None, :])[1][0])


@pytest.mark.parametrize("tol", KM.TOLS)
def test_scene_against_the_certified_check(tol):
    """margin 0.25: a HIT end is a point of the curve (rounded to fp32) at sqrt(hit_d2) from a row; FREE proves the clearance >= 0.25"""
    rec, _, _ = KM.scene_clearances(tol, np.inf)
    cert, _ = CM.scene_certificates()
    hit, free = cert["status"] == CM.HIT, cert["status"] == CM.FREE
    assert hit.sum() >= 8 and free.sum() >= 8 and hit.sum() + free.sum() == len(cert)
    assert np.all(rec["lo"][hit] <= np.sqrt(cert["hit_d2"][hit]) + END_ROUNDING)
    assert np.all(rec["hi"][free] >= CM.MARGIN)


def test_scene_max_depth_2_gives_open_brackets_that_still_hold():
    pts, trajs = KM.scene()
    rec, stats = KM.clearances(pts, *KM.pack(trajs), 0.01, np.inf, 2, 1 << 16)
    dense = KM.scene_dense()
    assert stats[0] == 3 and stats[2] == 0 and rec["depth"].max() == 2
    assert np.sum(rec["status"] == KM.OPEN) >= 32 and not np.any(rec["status"] == KM.INVALID)
    assert np.all(rec["lo"] <= dense) and np.all(dense <= rec["hi"] + END_ROUNDING + 1e-12) and np.all(rec["lo"] <= rec["hi"])
    is_open = rec["status"] == KM.OPEN
    assert np.all((rec["hi"] - rec["lo"])[~is_open] <= 0.01)


def test_scene_piece_cap_just_below_round_1():
    pts, trajs = KM.scene()
    full, _, trace = KM.scene_clearances(0.01, np.inf)
    assert trace[1] > 192                                      # the host form refuses a piece_cap below the segments
    rec, stats = KM.clearances(pts, *KM.pack(trajs), 0.01, np.inf, 16, trace[1] - 1)
    assert list(stats) == [1, 192, 1] and rec["depth"].max() == 0 and np.all(rec["pieces"] == 3)
    assert np.sum(rec["status"] == KM.OPEN) >= 32
    assert np.all(rec["lo"] <= KM.scene_dense()) and np.all(rec["lo"] <= rec["hi"])
    # round 0 itself is the full run's: hi can only have fallen since
    assert np.all(rec["hi"] >= full["hi"])
    # one more piece and round 1 runs
    rec, stats = KM.clearances(pts, *KM.pack(trajs), 0.01, np.inf, 16, trace[1])
    assert stats[0] > 1 and stats[1] >= 192 + trace[1]


# ---- hand cases ------------------------------------------------------------------------------------------------------------------------
def test_four_mm_line():
    pts, traj = KM.FOUR_MM["pts"], KM.FOUR_MM["traj"]
    tol = 0.001
    r, stats = one(pts, traj, tol)
    off = float(pts[0, 1])                                     # fp32(0.004): the clearance of the exact line
    assert r["status"] == KM.DONE and stats[2] == 0
    assert r["lo"] <= off <= r["hi"] <= off + tol and r["hi"] - r["lo"] <= tol
    assert r["at_seg"] == 0 and r["at_idx"] == 0 and abs(r["at_u"] - 0.51) <= 2.0 ** -int(r["depth"])
    assert r["hi"] == brute_distance(pts, end_point([traj], 0, float(r["at_u"])), 0)
    # down to 2^-16 of the line the nearest end is 0.51 to within 8 micrometres: hi is 0.004 to within a nanometre
    r, _ = one(pts, traj, 1e-5)
    assert r["status"] == KM.DONE and off <= r["hi"] <= off + 1e-8 and r["hi"] - r["lo"] <= 1e-5


def test_a_row_exactly_on_the_curves_end():
    r, stats = one(KM.ON_THE_END["pts"], KM.ON_THE_END["traj"], 0.01)
    assert r["status"] == KM.DONE and r["hi"] == 0.0 and r["lo"] == 0.0 and not np.signbit(r["lo"])
    assert r["at_seg"] == 0 and r["at_idx"] == 0 and r["at_u"] == 1.0 and r["depth"] == 0 and r["pieces"] == 1 and list(stats) == [1, 1, 0]


def test_segments_of_order_0():
    pts, trajs = KM.ORDER_ZERO["pts"], KM.ORDER_ZERO["trajs"]
    rec, stats = KM.clearances(pts, *KM.pack(trajs), 0.01, np.inf, 16, 1000)
    assert list(rec["hi"][:2]) == [0.25, 5.0] and np.all(rec["status"] == KM.DONE)
    assert np.all(rec["depth"][:2] == 0) and np.all(rec["pieces"][:2] == 1) and np.all(rec["at_u"][:2] == 0.0) and list(rec["at_seg"]) == [0, 1, 2]
    assert np.all(rec["hi"][:2] - rec["lo"][:2] <= 2.0 * rec["hi"][:2] * 2.0 ** -19) and np.all(rec["lo"][:2] < rec["hi"][:2])
    assert rec["hi"][2] == np.sqrt(3.0) and rec["at_u"][2] == 0.0
    # tol 0 cannot be met: a single point never splits and ends OPEN where it stands
    rec0, stats0 = KM.clearances(pts, *KM.pack(trajs[:2]), 0.0, np.inf, 16, 1000)
    assert np.all(rec0["status"] == KM.OPEN) and list(stats0) == [1, 2, 0]
    assert rec0["lo"].tobytes() == rec["lo"][:2].tobytes() and rec0["hi"].tobytes() == rec["hi"][:2].tobytes()


def test_tol_0_gives_open():
    pts, traj = KM.FOUR_MM["pts"], KM.FOUR_MM["traj"]
    r, stats = one(pts, traj, 0.0, max_depth=6)
    assert r["status"] == KM.OPEN and r["depth"] == 6 and stats[0] == 7
    assert 0.0 < r["lo"] <= float(pts[0, 1]) <= r["hi"]


def test_cap_retires_what_is_far_enough():
    """one row 2 m from a line: beyond cap = 0.5 the piece retires at depth 0, and lo says no more than "beyond the cap\""""
    pts = np.array([[0.5, 2.0, 0.0]], np.float32)
    r, stats = one(pts, KM.line((0, 0, 0), (1, 0, 0)), 0.01, cap=0.5)
    assert r["status"] == KM.DONE and r["depth"] == 0 and r["pieces"] == 1 and r["lo"] >= 0.5 - 0.01 and r["hi"] == np.sqrt(4.25)
    r, _ = one(pts, KM.line((0, 0, 0), (1, 0, 0)), 0.01)
    assert r["status"] == KM.DONE and r["depth"] > 0 and r["hi"] - r["lo"] <= 0.01 and r["lo"] <= 2.0 <= r["hi"]


def test_empty_cloud_and_empty_batch():
    _, trajs = KM.scene()
    rec, stats = KM.clearances(np.zeros((0, 3), np.float32), *KM.pack(trajs[:5]), 0.01, np.inf, 16, 1000)
    assert np.all(rec["status"] == KM.DONE) and np.all(rec["depth"] == 0) and np.all(rec["pieces"] == 3) and list(stats) == [1, 15, 0]
    assert np.all(rec["lo"] == np.inf) and np.all(rec["hi"] == np.inf) and all(nowhere(r) for r in rec)
    rec, stats = KM.clearances(KM.scene()[0], *KM.pack([]), 0.01, np.inf, 16, 1000)
    assert len(rec) == 0 and list(stats) == [0, 0, 0]


def test_an_invalid_trajectory_among_valid_ones_and_a_trajectory_alone():
    pts, trajs = KM.scene()
    coef, T, od = trajs[10]
    T = T.copy()
    T[1] = np.nan
    big = trajs[20][0].copy()
    big[1, 0] = 3.5e38 / trajs[20][1][1]
    mixed = [trajs[3], (coef, T, od), trajs[4], (big, trajs[20][1], trajs[20][2]), trajs[5]]
    rec, stats = KM.clearances(pts, *KM.pack(mixed), 0.01, np.inf, 16, 1000)
    assert list(rec["status"] == KM.INVALID) == [False, True, False, True, False]
    for r in rec[[1, 3]]:
        assert np.isnan(r["lo"]) and np.isnan(r["hi"]) and nowhere(r) and r["depth"] == 0 and r["pieces"] == 0
    full, _, _ = KM.scene_clearances(0.01, np.inf)
    for pos, t in ((0, 3), (2, 4), (4, 5)):
        alone, _ = KM.clearances(pts, *KM.pack([trajs[t]]), 0.01, np.inf, 16, 1000)
        for got, seg0 in ((rec[pos], 3 * pos), (full[t], 3 * t)):      # at_seg counts the segments in front; every other byte is the same
            want = alone[0].copy()
            want["at_seg"] += seg0
            assert got.tobytes() == want.tobytes(), (pos, t)
    assert stats[1] == rec["pieces"].sum()


def test_the_bound_is_plus_zero_never_minus_zero_and_inf_only_without_a_row():
    assert KM.lower(np.inf, 1.0, 1.0, 0.0, 1.0) == np.inf and KM.lower(1.0, np.inf, 1.0, 0.0, 1.0) == np.inf
    z = KM.lower(0.25, 0.25, 1.0, 0.0, 1.0)
    assert z == 0.0 and not np.signbit(z)
    assert KM.lower(1.0, 1.0, 0.0, 0.0, 1.0) == (1.0 - 0.0) - (2.0 * 2.0 ** -20 + 2.0 ** -40)
