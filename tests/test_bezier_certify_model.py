"""The numpy restatement of the certified Bezier check (tests/helpers/bezier_certify_model.py) on cases known by hand, on the cap rule
and on the property the call exists for -- no GPU needed.  The contract: include/pct_engine.h, paragraph "Certified Bezier check".

Soundness scene (bezier_certify_model.scene, SEED 7): 300 uniform points in [0, 10)^3, margin 0.25, 64 trajectories of three segments
with orders 0..12.  The model alone gave, at depth cap 12 with an ample piece_cap: 48 FREE, 16 HIT, 0 UNDECIDED, from 286 pieces in 4
rounds; at depth cap 2: 48 FREE, 15 HIT, 1 UNDECIDED."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import bezier_certify_model as CM  # noqa: E402
import bezier_model as BZ  # noqa: E402
import segment_model as M  # noqa: E402
import segment_search_model as SS  # noqa: E402

NO_INDEX = CM.NO_INDEX


def one(pts, traj, margin, max_depth=12, piece_cap=1000):
    cert, stats = CM.certify(pts, *CM.pack([traj]), margin, max_depth, piece_cap)
    return cert[0], stats


def no_hit(c):
    return c["hit_seg"] == -1 and c["hit_idx"] == NO_INDEX and np.isnan(c["hit_u"]) and c["hit_d2"] == np.inf


# ---- hand cases ------------------------------------------------------------------------------------------------------------------------
def test_four_mm_line_is_hit_where_the_sampled_check_sees_nothing():
    pts, traj, margin = CM.FOUR_MM["pts"], CM.FOUR_MM["traj"], CM.FOUR_MM["margin"]
    c, stats = one(pts, traj, margin)
    assert c["status"] == CM.HIT and c["depth"] == 7 and c["pieces"] == 15 and list(stats) == [8, 15, 0]
    assert c["hit_seg"] == 0 and c["hit_idx"] == 0 and c["hit_u"] == 65 / 128
    p = pts[0].astype(np.float64)
    d2 = ((p[0] - 65 / 128) ** 2 + p[1] ** 2) + p[2] ** 2
    assert c["hit_d2"] == d2 == c["min_d2"] and np.sqrt(d2) < margin
    # the model of the sampled check at dt = 0.02: 50 samples, none colliding, every one at least 10.8 mm from the point
    res = BZ.model_check(pts, dict(start=(0.0, 0.0, 0.0), sample_range=100.0, search_margin=margin, max_radius=1.0), *traj, 0.0, 10.0, 0.02, 4096)
    assert res["n"] >= 50 and res["first_hit"] == -1 and np.sqrt(res["d2"].min()) >= 0.0107
    # at depth caps below 7 the answer is UNDECIDED, never FREE
    for depth in range(7):
        c, _ = one(pts, traj, margin, depth)
        assert c["status"] == CM.UNDECIDED and c["depth"] == depth and c["pieces"] == 2 * depth + 1 and no_hit(c)


def test_point_at_exactly_the_margin_is_undecided_at_every_depth():
    traj, margin = CM.AT_MARGIN["traj"], CM.AT_MARGIN["margin"]
    pts = CM.at_margin_cloud(0)
    assert float(pts[0, 1]) == margin
    for depth in range(13):
        c, stats = one(pts, traj, margin, depth)
        assert c["status"] == CM.UNDECIDED and c["depth"] == depth and c["pieces"] == 2 * depth + 1 and no_hit(c), depth
        assert list(stats) == [depth + 1, 2 * depth + 1, 0]
        assert c["min_d2"] > margin * margin


def test_one_ulp_nearer_is_hit_one_ulp_farther_is_undecided():
    traj, margin = CM.AT_MARGIN["traj"], CM.AT_MARGIN["margin"]
    near, _ = one(CM.at_margin_cloud(-1), traj, margin, 20)
    assert near["status"] == CM.HIT and near["depth"] == 17 and near["pieces"] == 41 and np.sqrt(near["hit_d2"]) < margin
    far, _ = one(CM.at_margin_cloud(1), traj, margin, 20)
    assert far["status"] == CM.UNDECIDED and far["depth"] == 20 and no_hit(far)          # conservative by the slack: not FREE
    # free needs more than the slack: 2^-19 of the margin farther is enough for this line
    pts = CM.at_margin_cloud(0)
    pts[0, 1] = np.float32(margin * (1 + 2.0 ** -19))
    c, _ = one(pts, traj, margin, 20)
    assert c["status"] == CM.FREE and c["depth"] == 0 and c["pieces"] == 1


def test_orders_zero_and_one_and_a_zero_length_segment():
    pts = np.array([[1.0, 0.0, 0.0], [5.0, 5.0, 5.0]], np.float32)
    point = lambda p, T=2.0: (np.array([[p[0], p[1], p[2]]]) / T, np.array([T]), np.array([0], np.int32))      # noqa: E731
    # order 0: a point.  a == b: the chord test is the radius count of that point, the end test its nearest neighbour.
    c, stats = one(pts, point((1.0, 0.2, 0.0)), 0.25)
    assert c["status"] == CM.HIT and c["depth"] == 0 and c["pieces"] == 1 and c["hit_u"] == 0.0 and c["hit_idx"] == 0
    assert c["hit_d2"] == np.float64(np.float32(0.2)) ** 2
    c, _ = one(pts, point((1.0, 0.3, 0.0)), 0.25)
    assert c["status"] == CM.FREE and c["pieces"] == 1 and c["min_d2"] == np.float64(np.float32(0.3)) ** 2 and no_hit(c)
    # exactly at the margin: blocked, no hit, and both halves of a point are that point again: UNDECIDED, the pieces doubling every
    # round (what piece_cap is for)
    c, _ = one(pts, point((1.0, 0.25, 0.0)), 0.25, 5)
    assert c["status"] == CM.UNDECIDED and c["depth"] == 5 and c["pieces"] == 63
    c, stats = one(pts, point((1.0, 0.25, 0.0)), 0.25, 12, 16)
    assert c["status"] == CM.UNDECIDED and c["depth"] == 4 and c["pieces"] == 31 and list(stats) == [5, 31, 1]
    # order 1, zero length: the same answers as the point
    for y, status in ((0.2, CM.HIT), (0.3, CM.FREE)):
        c, _ = one(pts, CM.line((1.0, y, 0.0), (1.0, y, 0.0)), 0.25)
        assert c["status"] == status and c["pieces"] == 1
    # order 1 against the capsule model itself: blocked iff the capsule count under reach is non-zero
    traj = CM.line((0.0, 1.0, 0.0), (2.0, 1.0, 0.0))
    P = CM.world_points(traj[0][0], 1.0, 1)
    a, b, reach = CM.geometry(P, 0.25)
    assert reach == (0.25 * (1 + 2.0 ** -20)) + 2.0 * 2.0 ** -40                         # rho = 0 for a line
    assert SS.segment_count(pts, [np.concatenate([a, b])], reach)[0] == int(CM.blocked(pts, a, b, reach)) == 0
    c, _ = one(pts, traj, 0.25)
    assert c["status"] == CM.FREE and c["pieces"] == 1 and c["min_d2"] == 2.0           # the ends, 1 m along and 1 m beside
    # the end test is the nearest-neighbour search: segment_model's a == b query
    idx, d2 = CM.nearest(pts, np.array([a, b]))
    sidx, sd2, _ = M.segment_nn(pts, np.array([np.concatenate([a, a]), np.concatenate([b, b])]), np.inf)
    assert np.array_equal(idx, sidx.astype(np.int64)) and np.array_equal(d2, sd2)


@pytest.mark.parametrize("bad", (0.0, -1.0, np.nan, np.inf, -np.inf))
def test_bad_segment_times_are_invalid(bad):
    pts, trajs = CM.scene()
    coef, T, od = trajs[0]
    T = T.copy()
    T[1] = bad
    cert, stats = CM.certify(pts, *CM.pack([trajs[1], (coef, T, od), trajs[2]]), CM.MARGIN, 12, 1000)
    ref, _ = CM.certify(pts, *CM.pack([trajs[1], trajs[2]]), CM.MARGIN, 12, 1000)
    c = cert[1]
    assert c["status"] == CM.INVALID and c["depth"] == 0 and c["pieces"] == 0 and c["min_d2"] == np.inf and no_hit(c)
    assert cert["status"][0] == ref["status"][0] and cert["status"][2] == ref["status"][1] and stats[1] == ref["pieces"].sum()


def test_control_points_beyond_fp32_are_invalid():
    pts, trajs = CM.scene()
    coef, T, od = trajs[3]
    for v, status in ((3.5e38, CM.INVALID), (-3.5e38, CM.INVALID), (np.nan, CM.INVALID), (3.4e38, None)):
        c2 = coef.copy()
        c2[0, 0] = v / T[0]
        cert, _ = CM.certify(pts, *CM.pack([(c2, T, od)]), CM.MARGIN, 3, 1000)
        assert (cert["status"][0] == CM.INVALID) == (status == CM.INVALID), v


def test_halving_is_de_casteljau():
    P = CM.world_points(CM.scene()[1][4][0][2], 1.0, CM.scene()[1][4][2][2])
    left, right = CM.halve(P)
    assert np.array_equal(left[0], P[0]) and np.array_equal(right[-1], P[-1]) and np.array_equal(left[-1], right[0])
    assert np.array_equal(left[1], (P[0] + P[1]) * 0.5) and np.array_equal(right[-2], (P[-2] + P[-1]) * 0.5)
    # the children trace the parent's curve
    whole = CM.dense_samples(P)
    assert np.abs(CM.dense_samples(left)[::2] - whole[:2048]).max() < 1e-12
    assert np.abs(CM.dense_samples(right)[::2] - whole[2048:]).max() < 1e-12


# ---- the cap rule --------------------------------------------------------------------------------------------------------------------
def test_piece_cap_rule():
    pts, trajs = CM.scene()
    full, _ = CM.scene_certificates()
    busy = [trajs[i] for i in sorted(np.argsort(-full["pieces"], kind="stable")[:4])]
    nseg = 12
    ample, astats = CM.certify(pts, *CM.pack(busy), CM.MARGIN, 12, 1 << 20)
    assert astats[2] == 0 and not np.any(ample["status"] == CM.UNDECIDED)
    first = CM.certify(pts, *CM.pack(busy), CM.MARGIN, 0, 1 << 20)[0]                   # depth cap 0: UNDECIDED marks the blocked
    n_split0 = {cap: None for cap in (nseg, nseg + 1)}
    for cap in n_split0:
        cert, stats = CM.certify(pts, *CM.pack(busy), CM.MARGIN, 12, cap)
        # round 0 examines the 12 segments; more than cap / 2 of them want to split, so nothing splits and their owners are UNDECIDED
        assert list(stats) == [1, nseg, 1] and np.all(cert["depth"] == 0) and np.all(cert["pieces"] == 3)
        assert np.array_equal(cert["status"], first["status"])
    # the smallest cap that lets every round of this batch through is twice its largest number of splitting pieces
    need = 0
    for cap in range(nseg, 64):
        cert, stats = CM.certify(pts, *CM.pack(busy), CM.MARGIN, 12, cap)
        if stats[2] == 0:
            need = cap
            assert cert.tobytes() == ample.tobytes() and np.array_equal(stats, astats)
            break
    assert need > nseg + 1 and need % 2 == 0
    assert CM.certify(pts, *CM.pack(busy), CM.MARGIN, 12, need - 1)[1][2] == 1


# ---- soundness -----------------------------------------------------------------------------------------------------------------------
def test_dense_sampler_is_the_exact_powers_evaluator():
    """dense_samples against bezier_model.bezier_samples_exact_powers on the same grid (the row P, seg_time 1, dt = 2^-12)"""
    _, trajs = CM.scene()
    coef, T, od = trajs[5]
    for s in range(3):
        P = CM.world_points(coef[s], T[s], od[s])
        m = int(od[s]) + 1
        row = np.concatenate([P[:, k] for k in range(3)])[None, :]
        ref = BZ.bezier_samples_exact_powers(row, [1.0], [od[s]], 0.0, 100.0, 2.0 ** -12, cap=512)[0]
        assert len(ref) == 512 and m == len(P)
        assert np.array_equal(CM.dense_samples(P)[:512], ref)


def test_free_is_free_and_hit_is_a_hit():
    pts, trajs = CM.scene()
    cert, stats = CM.scene_certificates()
    counts = np.bincount(cert["status"], minlength=4)
    print("scene:", counts, stats)
    assert list(counts) == [48, 16, 0, 0] and list(stats) == [4, 286, 0]                    # what the model alone gave for SEED 7
    assert counts[CM.FREE] >= 8 and counts[CM.HIT] >= 8 and counts[CM.UNDECIDED] <= len(trajs) // 8
    shallow = np.bincount(CM.scene_certificates(2)[0]["status"], minlength=4)
    assert list(shallow) == [48, 15, 1, 0]
    coef, T, od, offs = CM.pack(trajs)
    worst = np.inf
    for t in np.nonzero(cert["status"] == CM.FREE)[0]:
        for i in range(offs[t], offs[t + 1]):
            P = CM.world_points(coef[i], T[i], od[i])
            clear = CM.clearance(pts, np.concatenate([CM.dense_samples(P), P[-1:]]))
            worst = min(worst, clear)
            assert clear >= CM.MARGIN - 1e-9, (t, i, clear)
        assert np.sqrt(cert["min_d2"][t]) >= CM.MARGIN
    print("smallest sampled clearance of a FREE trajectory:", worst)
    p64 = pts.astype(np.float64)
    for t in np.nonzero(cert["status"] == CM.HIT)[0]:
        c = cert[t]
        i = int(c["hit_seg"])
        assert offs[t] <= i < offs[t + 1] and 0.0 <= c["hit_u"] <= 1.0
        # the point of the curve at (hit_seg, hit_u), evaluated independently with exact powers, and the named row
        P = CM.world_points(coef[i], T[i], od[i])
        g = c["hit_u"] * CM.GRID
        assert g == int(g), "hit_u is dyadic of depth <= 12"
        x = P[-1] if int(g) == CM.GRID else CM.dense_samples(P)[int(g)]
        # recomputed from that point narrowed to fp32, as the end test sees it: below the margin, and the reported d2 bit for bit
        dx, dy, dz = p64[c["hit_idx"]] - x.astype(np.float32).astype(np.float64)
        d2 = (dx * dx + dy * dy) + dz * dz
        assert np.sqrt(d2) < CM.MARGIN and d2 == c["hit_d2"] and c["min_d2"] <= c["hit_d2"], (t, d2, c["hit_d2"])
        # and it is the nearest row of that end
        assert CM.nearest(pts, x.astype(np.float32).astype(np.float64)[None])[0][0] == c["hit_idx"]
    assert cert["pieces"].sum() == stats[1]
