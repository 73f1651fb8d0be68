"""GPU tests of depth images on the rolling map (pct_cloud_ring_carve_depth, pct_cloud_append_depth, pct_depth_classify and their way
up through the corridor finder): csrc/ring_depth.hpp.

Reference: the numpy model of the contract (tests/helpers/depth_model.py) and, over the model's rows, the numpy restatements of the
searches that tests/test_gpu_ring_remove.py uses.  Everything is exact; there are no tolerances."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from pointcloudtraj_amd import scenarios as S, synth
from test_depth_api import PIXEL_CASES, SEEN_CASES, flat, random_view, small_view
from test_gpu_ring_remove import PRM, REMOVED, check_counts, check_searches, params, traj_through

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import depth_model as D  # noqa: E402

pytestmark = pytest.mark.gpu

F32 = np.float32
RES = 0.1
WIDE = (60.0, 60.0, 60.0)           # the table's extent for clouds around a random pose (world cells fold onto shared buckets)


@pytest.fixture(scope="module")
def E():
    from pointcloudtraj_amd import engine
    engine.init(0)
    return engine


def window_pair(E, cap, dedup=False, cell=0.5, extent=WIDE):
    c, w = E.Cloud(cap), D.DepthWindow(cap, RES, dedup)
    c.ring_index(cell, extent)
    if dedup:
        c.ring_dedup(RES)
    return c, w


def points_in_view(rng, view, n, lo=-0.25, hi=1.25, depth=(0.2, 20.0), behind=0.1):
    """fp32 points around the view's frustum: pixel coordinates in [lo, hi] of the image's size (so some fall outside), z-depths in
    `depth`, a share `behind` of them behind the camera"""
    t, Rm, focal, _, w, h, _ = D._view(view)
    u, v = rng.uniform(lo * w, hi * w, n), rng.uniform(lo * h, hi * h, n)
    cz = rng.uniform(*depth, n) * np.where(rng.random(n) < behind, -1.0, 1.0)
    cam = np.stack([(u - w / 2.0) / (focal * w) * cz, (v - h / 2.0) / (focal * w) * cz, cz], axis=1)
    return (t + cam @ Rm.T).astype(np.float32)


def random_image(rng, view, lo=0.2, hi=22.0, holes=True):
    img = rng.uniform(lo, hi, (view.height, view.width)).astype(np.float32)
    if holes and img.size > 1:
        r = rng.random(img.shape)
        img[r < 0.08] = np.inf
        img[(r >= 0.08) & (r < 0.11)] = np.nan
        img[(r >= 0.11) & (r < 0.13)] = -np.inf
    return img


def live_rows(c):
    """(slots, rows) of the finite rows of the window, in slot order, read back from the device"""
    idx, _, xyz = c.radius_crop((0.0, 0.0, 0.0), 1.0e6)
    return idx.astype(np.int64), xyz


def check_rows(c, w, tag):
    rows = w.live()
    finite = np.isfinite(rows).all(axis=1)
    idx, xyz = live_rows(c)
    assert np.array_equal(idx, np.flatnonzero(finite)) and np.array_equal(xyz.view(np.uint32), rows[finite].view(np.uint32)), f"{tag}: the window's rows"


def check_slots(c, w, tag, own=()):
    """every slot below the window's size: a removed slot shows the removed marker, a live one its own id at the filed position;
    own = the slots that hold the caller's own NaN rows, which are filed like any row and never removed"""
    gone = D.R.has_nan(w.live())
    for slot in range(w.count):
        out = c.debug_ring_slot(slot)
        if gone[slot] and slot not in own:
            assert out[0] == REMOVED, f"{tag}: slot {slot} is removed, its where word is {out[0]:#x}"
        else:
            assert out[0] != REMOVED and out[4] == slot, f"{tag}: slot {slot} is filed at {out[0]:#x} where id {out[4]} is stored"


def check_carve(c, w, view, img, margin, tag, expect_some=True, own=()):
    got, want = c.ring_carve_depth(view, img, margin), w.carve(view, img, margin)
    print(f"{tag}: carved {got} of {w.count}, live {w.live_count()}")
    assert got == want and (want > 0 or not expect_some), f"{tag}: carved {got}, the model carves {want}"
    check_counts(c, w, tag)
    check_slots(c, w, tag, own)
    check_rows(c, w, tag)
    assert c.ring_carve_depth(view, img, margin) == 0, f"{tag}: a second carve with the same image removes nothing"


# ---- 1. the carve against the model ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("metric", [D.DEPTH_Z, D.DEPTH_RANGE], ids=["z", "range"])
@pytest.mark.parametrize("size", [(1, 1), (8, 6), (64, 48)], ids=["1x1", "8x6", "64x48"])
def test_carve_matches_the_model(E, size, metric):
    """2 000 random points around a random pose: the carved slots, the count and the rows left, as the model has them"""
    rng = np.random.default_rng(1000 + 10 * size[0] + metric)
    view = random_view(rng, *size)
    view.metric = metric
    c, w = window_pair(E, 2500)
    pts = points_in_view(rng, view, 2000)
    c.append(pts)
    w.append_plain(pts)
    img = random_image(rng, view)
    if size == (1, 1):
        img[0, 0] = 12.0
    check_carve(c, w, view, img, 0.05, f"{size[0]}x{size[1]} metric {metric}")
    assert 0 < w.live_count() < 2000 and w.resets == 0
    c.close()


def test_carve_on_a_wrapped_window_with_an_overflow_queue_and_non_finite_rows(E):
    """a ring that has wrapped; 100 copies of one point in one cell (32 in its bucket, the rest in the overflow queue: the carve
    retires queue entries); rows holding NaN and +/-inf, planted by the caller and by ring_remove_indices, are left alone"""
    rng = np.random.default_rng(1100)
    view = random_view(rng, 64, 48)
    c, w = window_pair(E, 1500)
    t, Rm, _, _, _, _, _ = D._view(view)
    spot = (t + (np.float64([0.3, -0.2, 6.0]) @ Rm.T)).astype(np.float32)            # on the optical axis' side, 6 m out
    odd = F32([[np.nan, 1, 1], [np.inf, 0, 0], [-np.inf, 2, 2], [1, np.inf, np.nan], [3, 3, np.inf]])
    frames = [points_in_view(rng, view, 1000), np.concatenate([points_in_view(rng, view, 350), np.tile(spot, (100, 1)), odd, points_in_view(rng, view, 445)])]
    for f in frames:
        c.append(f)
        w.append_plain(f)
    assert w.count == 1500 and w.nxt == 400, "the ring has wrapped"
    before = c.ring_info()["overflow_entries"]
    assert before >= 60
    planted = np.uint32([5, 700, 701, 1499])
    assert c.ring_remove_indices(planted) == w.remove_indices(planted) == 4
    img = random_image(rng, view)
    pr = D.project(view, spot[None])
    assert pr["inside"][0]
    img[pr["rv"][0], pr["ru"][0]] = 11.0                                           # the copies are seen through
    own = (1450, 1453)                                                             # the caller's rows that hold a NaN
    check_carve(c, w, view, img, 0.05, "wrapped window", own=own)
    copies = np.flatnonzero((w.xyz.view(np.uint32) == spot.view(np.uint32)).all(axis=1))
    assert len(copies) == 0 and c.ring_info()["overflow_entries"] < before
    q = np.concatenate([points_in_view(rng, view, 80), spot[None], frames[0][:20]]).astype(np.float32)
    check_searches(E, c, w.live(), q, "wrapped window")
    nxt = points_in_view(rng, view, 300)                                           # the cursor stands where it stood
    c.append(nxt)
    w.append_plain(nxt)
    check_counts(c, w, "append over carved slots")
    check_slots(c, w, "append over carved slots", own)
    check_rows(c, w, "append over carved slots")
    c.close()


def test_hand_pinned_edge_cases_on_the_device(E):
    """the cases tests/test_depth_api.py pins on the model, through pct_depth_classify and through the carve"""
    for name, point, near_z, inside, pixel in PIXEL_CASES:
        with np.errstate(over="ignore"):
            seen_by, pix = E.depth_classify([small_view(near_z=near_z)], [flat(np.inf)], np.float64([F32(point)]), 0.0)
        assert tuple(pix[0]) == pixel and seen_by[0] == -1, f"{name}: pixel {tuple(pix[0])}"
    for name, metric, value, margin, point, want in SEEN_CASES:
        view = small_view(metric)
        seen_by, _ = E.depth_classify([view], [flat(value)], np.float64([F32(point)]), margin)
        assert seen_by[0] == (0 if want else -1), f"{name}: classify"
        c = E.Cloud(16)
        c.ring_index(0.5, (8.0, 8.0, 8.0))
        c.append(F32([point, (0, 0, -50)]))                                        # the second point is behind the camera: it stays
        assert c.ring_carve_depth(view, flat(value), margin) == int(want), f"{name}: carve"
        assert c.ring_live() == (2 - int(want), int(want)) and (c.debug_ring_slot(0)[0] == REMOVED) == want
        c.close()


# ---- 2. the NaN-row equivalence after a carve ------------------------------------------------------------------------------------

def test_nan_row_equivalence_after_a_carve(E):
    """every search on the carved window against numpy over the model's rows and against a cloud uploaded with those rows, and a
    replan plan captured before the carve against one captured on the uploaded cloud.  cap 3000, an 8 x 8 x 8 table, wrapped once"""
    cap = 3000
    c, twin, w = E.Cloud(cap), E.Cloud(cap), D.DepthWindow(cap, RES, False)
    for x in (c, twin):
        x.ring_index(0.25, (1.0, 1.0, 1.0))
    for f in range(4):
        pts = synth.uniform_points(500 + f, 1000, 0.0, 10.0)
        c.append(pts)
        w.append_plain(pts)
    rng = np.random.default_rng(1200)
    view = E.depth_view((5.0, 5.0, -4.0), np.eye(3), 64, 48, fov_hor_deg=90.0)
    img = random_image(rng, view, 4.0, 14.0)
    q = np.concatenate([synth.uniform_points(510, 120, -1.0, 11.0), w.live()[::97][:20]]).astype(np.float32)
    nodes = synth.uniform_points(511, 64, 2.0, 8.0).astype(np.float64)
    coef, T, od = traj_through()
    plan = E.ReplanPlan(c, 64, 128, 2)
    before = plan.run(params(E), nodes, coef, T, od, 0.0, 2.0, 0.02)
    check_carve(c, w, view, img, 0.05, "uniform window")
    assert 500 < w.live_count() < 2700
    check_searches(E, c, w.live(), q, "after the carve", twin)
    after = plan.run(params(E), nodes, coef, T, od, 0.0, 2.0, 0.02)              # the graph captured before the carve
    tplan = E.ReplanPlan(twin, 64, 128, 2)
    want = tplan.run(params(E), nodes, coef, T, od, 0.0, 2.0, 0.02)
    for k in want:
        assert np.array_equal(after[k], want[k]), f"the replan plan across the carve: {k}"
    assert not np.array_equal(before["node_radius"], after["node_radius"]), "the carve changed no radius: the test shows nothing"
    plan.close()
    tplan.close()
    c.close()
    twin.close()


# ---- 3. the empty-window rule ----------------------------------------------------------------------------------------------------

def test_an_image_that_sees_through_every_point_empties_the_window(E):
    rng = np.random.default_rng(1300)
    view = random_view(rng, 64, 48)
    c, w = window_pair(E, 4000, dedup=True)
    pts = points_in_view(rng, view, 1500, 0.1, 0.9, (0.5, 20.0), 0.0)
    c.append(pts)
    w.append(pts)
    far = np.full((48, 64), 100.0, np.float32)
    there = w.live_count()
    assert c.ring_carve_depth(view, far, 0.0) == w.carve(view, far, 0.0) == there > 1000
    assert (len(c), w.count, w.nxt, w.resets) == (0, 0, 0, 1) and c.ring_live() == (0, 0) and c.has_ring_index
    rad, idx, d2 = c.inflate(params(E), np.float64([[5.0, 5.0, 5.0]]))
    assert rad[0] == PRM["max_radius"] - PRM["search_margin"] and idx[0] == 0xFFFFFFFF and np.isinf(d2[0])
    assert c.ring_carve_depth(view, far, 0.0) == 0
    img = random_image(rng, view)                                                  # the next depth append files from slot 0
    offered, kept = c.append_depth(view, img)
    frame, flags = w.append_depth(view, img)
    assert (offered, kept) == (len(frame), int(flags.sum())) and kept > 500 and len(c) == w.count == kept
    i, d = c.nn(frame[flags])
    assert np.all(d == 0.0) and np.array_equal(np.unique(i), np.arange(kept, dtype=np.uint32))
    check_rows(c, w, "after the reset")
    check_slots(c, w, "after the reset")
    c.close()


# ---- 4. append_depth = append of the model's un-projected frame ----------------------------------------------------------------------

def check_append(c, w, view, img, max_depth, tag, dedup):
    offered, kept = c.append_depth(view, img, max_depth)
    frame, flags = w.append_depth(view, img, max_depth)
    print(f"{tag}: offered {offered}, kept {kept}")
    assert (offered, kept) == (len(frame), int(flags.sum())), f"{tag}: offered {offered} / kept {kept}, the model {len(frame)} / {int(flags.sum())}"
    if dedup:
        last = c.ring_dedup_last()
        assert (last["offered"], last["kept"]) == (offered, kept) and np.array_equal(last["flags"], flags), f"{tag}: ring_dedup_last"
    check_counts(c, w, tag)
    check_rows(c, w, tag)
    return frame, flags


@pytest.mark.parametrize("dedup", [False, True], ids=["plain", "dedup"])
def test_append_depth_matches_an_append_of_the_unprojected_frame(E, dedup):
    rng = np.random.default_rng(1400 + dedup)
    view = random_view(rng, 64, 48)
    c, w = window_pair(E, 2500, dedup)
    twin = E.Cloud(2500)
    twin.ring_index(0.5, WIDE)
    if dedup:
        twin.ring_dedup(RES)
    pre = points_in_view(rng, view, 1500)
    for x in (c, twin):
        x.append(pre)
    w.append(pre) if dedup else w.append_plain(pre)
    img = random_image(rng, view, 0.2, 22.0)
    img[0, :8] = 0.005                                                             # below near_z
    img[1, :8] = F32(0.01)                                                         # float(0.01) >= 0.01: valid
    frame, flags = check_append(c, w, view, img, 15.0, "max_depth cuts pixels", dedup)
    assert (img > 15.0).sum() > 500 and len(frame) < np.isfinite(img).sum() - 500, "max_depth cut pixels"
    assert dedup or (w.count == w.cap and 0 < w.nxt < 1500), "the ring wrapped"
    twin.append(frame)                                                             # the same points from host memory
    ti, td, tx = twin.radius_crop((0.0, 0.0, 0.0), 1.0e6)
    gi, gd, gx = c.radius_crop((0.0, 0.0, 0.0), 1.0e6)
    assert np.array_equal(ti, gi) and np.array_equal(tx.view(np.uint32), gx.view(np.uint32)) and len(twin) == len(c)
    if dedup:
        assert np.array_equal(twin.ring_dedup_last()["flags"], flags)
    check_slots(c, w, "after the depth append")
    check_append(c, w, view, img, 18.0, "the same image again, fewer pixels cut", dedup)
    empty = np.full((48, 64), np.inf, np.float32)
    empty[::2] = np.nan
    empty[0, 0], empty[0, 1] = 0.001, -3.0
    before = len(c)
    assert c.append_depth(view, empty) == (0, 0) and len(c) == before
    check_append(c, w, view, empty, np.inf, "an all-invalid image", dedup)
    probe = points_in_view(rng, view, 1)                                           # the cursor: where the next point lands
    c.append(probe)
    w.append(probe) if dedup else w.append_plain(probe)
    check_rows(c, w, "a point appended behind the images")
    c.close()
    twin.close()


@pytest.mark.parametrize("dedup", [False, True], ids=["plain", "dedup"])
def test_append_depth_as_the_first_data_sizes_the_table(E, dedup):
    """a cloud whose table does not exist yet (pct_cloud_ring_index without an extent): the un-projected frame is the first data"""
    rng = np.random.default_rng(1500 + dedup)
    view = random_view(rng, 33, 17)
    c, w = E.Cloud(2000), D.DepthWindow(2000, RES, dedup)
    c.ring_index()
    if dedup:
        c.ring_dedup(RES)
    assert not c.has_ring_index
    img = random_image(rng, view, 0.5, 12.0)
    check_append(c, w, view, img, np.inf, "first data", dedup)
    assert c.has_ring_index and len(c) > 200
    check_slots(c, w, "first data")
    # carve first, then append: at a small positive margin the image's own points are not seen through by it
    check_carve(c, w, view, img, 1.0e-3, "carve by the image that was appended", expect_some=False)
    assert w.removed == 0
    farther = img.copy()
    farther[:, :16] += 2.0                                                         # the left half now shows a surface 2 m farther
    check_carve(c, w, view, farther, 1.0e-3, "carve by an image whose left half is 2 m farther")
    assert 0 < w.live_count() < w.count
    c.close()


def test_append_depth_refuses_what_it_cannot_take(E):
    rng = np.random.default_rng(1600)
    view = random_view(rng, 64, 48)
    c, w = window_pair(E, 1000)
    pre = points_in_view(rng, view, 600)
    c.append(pre)
    w.append_plain(pre)
    img = np.full((48, 64), 5.0, np.float32)
    with pytest.raises(E.EngineError) as ei:
        c.append_depth(view, img)                                                  # 3 072 valid pixels > 1 000 slots
    assert ei.value.code == 6
    check_counts(c, w, "after PCT_ERR_CAPACITY")
    check_rows(c, w, "after PCT_ERR_CAPACITY")
    img[1:] = np.inf
    img[0, 40:] = np.inf                                                           # 40 valid pixels: taken
    assert c.append_depth(view, img) == (40, 40)
    w.append_depth(view, img)
    check_rows(c, w, "a frame that fits")
    view.metric = D.DEPTH_RANGE
    with pytest.raises(E.EngineError) as ei:
        c.append_depth(view, img)
    assert ei.value.code == 2
    check_rows(c, w, "after a range image was refused")
    c.close()


# ---- 5. PCT_ERR_INVALID ----------------------------------------------------------------------------------------------------------

def bad_views(E):
    """(what, view) for every view pct_engine.h refuses"""
    def make(**kw):
        v = E.depth_view((1.0, 2.0, 3.0), np.eye(3), 8, 6, focal=0.5)
        for k, val in kw.items():
            if k in ("t0", "R4"):
                getattr(v, k[0])[int(k[1])] = val
            else:
                setattr(v, k, val)
        return v
    out = [("width 0", make(width=0)), ("height -1", make(height=-1)), ("more than 2^24 pixels", make(width=4097, height=4096)),
           ("metric 2", make(metric=2)), ("metric -1", make(metric=-1)), ("reserved", make(reserved=1))]
    for name in ("focal", "near_z"):
        out += [(f"{name} = {bad}", make(**{name: bad})) for bad in (0.0, -1.0, np.inf, np.nan)]
    out += [(f"t = {bad}", make(t0=bad)) for bad in (np.nan, np.inf, -np.inf)]
    out += [(f"R = {bad}", make(R4=bad)) for bad in (np.nan, np.inf)]
    return out


def test_every_invalid_argument_leaves_the_cloud_as_it_was(E):
    L = E.lib()
    rng = np.random.default_rng(1700)
    good = E.depth_view((0.0, 0.0, 0.0), np.eye(3), 8, 6, focal=0.5)
    img = flat(50.0)
    c, w = window_pair(E, 500, dedup=True, extent=(20.0, 20.0, 20.0))
    pts = points_in_view(rng, good, 300, 0.1, 0.9, (1.0, 9.0), 0.0)
    c.append(pts)
    w.append(pts)
    n, m = C.c_int64(-1), C.c_int64(-1)
    img_p = img.ctypes.data_as(C.c_void_p)
    pts64 = pts.astype(np.float64)
    for what, v in bad_views(E):
        assert L.pct_cloud_ring_carve_depth(c.handle, C.byref(v), img_p, 0.0, C.byref(n)) == 2, f"carve: {what}"
        assert L.pct_cloud_append_depth(c.handle, C.byref(v), img_p, 10.0, C.byref(n), C.byref(m)) == 2, f"append: {what}"
        assert L.pct_depth_classify(C.byref(v), (C.c_void_p * 1)(img.ctypes.data), 1, pts64.ctypes.data, 3, 0.0,
                                    (C.c_int32 * 3)(), None) == 2, f"classify: {what}"
    g = C.byref(good)
    assert L.pct_cloud_ring_carve_depth(None, g, img_p, 0.0, C.byref(n)) == 2 and L.pct_cloud_ring_carve_depth(c.handle, None, img_p, 0.0, C.byref(n)) == 2
    assert L.pct_cloud_ring_carve_depth(c.handle, g, None, 0.0, C.byref(n)) == 2 and L.pct_cloud_ring_carve_depth(c.handle, g, img_p, 0.0, None) == 2
    assert L.pct_cloud_ring_carve_depth(c.handle, g, img_p, np.nan, C.byref(n)) == 2
    assert L.pct_cloud_append_depth(None, g, img_p, 10.0, C.byref(n), C.byref(m)) == 2 and L.pct_cloud_append_depth(c.handle, None, img_p, 10.0, C.byref(n), C.byref(m)) == 2
    assert L.pct_cloud_append_depth(c.handle, g, None, 10.0, C.byref(n), C.byref(m)) == 2 and L.pct_cloud_append_depth(c.handle, g, img_p, np.nan, C.byref(n), C.byref(m)) == 2
    assert L.pct_cloud_append_depth(c.handle, g, img_p, 10.0, None, C.byref(m)) == 2 and L.pct_cloud_append_depth(c.handle, g, img_p, 10.0, C.byref(n), None) == 2
    check_counts(c, w, "after the refused calls")
    check_rows(c, w, "after the refused calls")
    assert c.ring_dedup_last()["offered"] == 300
    there = w.live_count()
    plain = E.Cloud(100)                                                           # no rolling-map index
    plain.set_input(pts[:50])
    for call in (lambda: plain.ring_carve_depth(good, img, 0.0), lambda: plain.append_depth(good, img)):
        with pytest.raises(E.EngineError) as ei:
            call()
        assert ei.value.code == 2
    assert len(plain) == 50
    plain.close()
    fresh = E.Cloud(100)                                                           # an empty cloud: PCT_OK, nothing removed
    fresh.ring_index(0.5, (20.0, 20.0, 20.0))
    assert fresh.ring_carve_depth(good, img, 0.0) == 0 and len(fresh) == 0
    fresh.close()
    assert c.ring_carve_depth(good, img, 0.0) == w.carve(good, img, 0.0) == there > 250 and len(c) == 0      # and the calls do work on this cloud
    c.close()


# ---- 6. classification -----------------------------------------------------------------------------------------------------------

def test_depth_classify_matches_the_model(E):
    rng = np.random.default_rng(1800)
    views, images = [], []
    for k, (size, metric) in enumerate([((64, 48), D.DEPTH_Z), ((8, 6), D.DEPTH_RANGE), ((33, 17), D.DEPTH_Z)]):
        v = random_view(rng, *size)
        v.metric = metric
        for a in range(3):
            v.t[a] = float(rng.uniform(-2.0, 2.0))
        views.append(v)
        images.append(random_image(rng, v, 0.5, 18.0))
    pts = np.concatenate([rng.uniform(-12.0, 12.0, (497, 3)), np.float64([[1e39, 0, 0], [0, -1e300, 1], [np.nan, 0, 1]])])
    want_seen, want_pix = D.classify(views, images, pts, 0.05)
    seen, pix = E.depth_classify(views, images, pts, 0.05)
    assert np.array_equal(seen, want_seen) and np.array_equal(pix, want_pix)
    assert (want_seen == -1).sum() > 10 and (want_seen == 0).sum() > 10 and (want_seen > 0).sum() > 0
    assert (want_pix[:, 0] >= 0).sum() > 20 and np.all(want_pix[-3:] == -1)
    seen2, none = E.depth_classify(views, images, pts, 0.05, want_pixel=False)    # pixel = NULL
    assert none is None and np.array_equal(seen2, want_seen)
    for order in ([1, 0, 2], [2, 1]):                                              # the lowest view index wins; the last view gives the pixel
        vs, ims = [views[k] for k in order], [images[k] for k in order]
        ws, wp = D.classify(vs, ims, pts, 0.05)
        gs, gp = E.depth_classify(vs, ims, pts, 0.05)
        assert np.array_equal(gs, ws) and np.array_equal(gp, wp)
    s0, p0 = E.depth_classify(views, images, np.zeros((0, 3)), 0.05)             # n = 0
    assert len(s0) == 0 and p0.shape == (0, 2)
    L = E.lib()
    varr = (E.DepthView * 17)(*([views[0]] * 17))
    iarr = (C.c_void_p * 17)(*([images[0].ctypes.data] * 17))
    out = (C.c_int32 * 4)()
    p4 = np.zeros((4, 3))
    for nv in (0, 17, -1):
        assert L.pct_depth_classify(varr, iarr, nv, p4.ctypes.data, 4, 0.0, out, None) == 2
    assert L.pct_depth_classify(varr, iarr, 16, p4.ctypes.data, 4, 0.0, out, None) == 0
    assert L.pct_depth_classify(varr, iarr, 1, p4.ctypes.data, 4, np.nan, out, None) == 2
    assert L.pct_depth_classify(varr, iarr, 1, None, 4, 0.0, out, None) == 2 and L.pct_depth_classify(varr, iarr, 1, p4.ctypes.data, 4, 0.0, None, None) == 2
    assert L.pct_depth_classify(None, iarr, 1, p4.ctypes.data, 4, 0.0, out, None) == 2 and L.pct_depth_classify(varr, None, 1, p4.ctypes.data, 4, 0.0, out, None) == 2
    iarr[0] = None
    assert L.pct_depth_classify(varr, iarr, 1, p4.ctypes.data, 4, 0.0, out, None) == 2


# ---- 7. the rgbd window through the corridor finder --------------------------------------------------------------------------------

def test_rgbd_window_through_the_corridor_finder(E):
    """scenarios.run_rgbd_window_scenario on SafeRegionRrtStar: the live set per frame equals the model's, and the point at the
    obstacle's former centre stops colliding once the obstacle has left"""
    from pointcloudtraj_amd import corridor
    G = S.RGBD
    model = D.DepthWindow(G["cap"], G["res"])
    want = S.run_rgbd_window_scenario(model, D.render)
    finder = corridor.SafeRegionRrtStar(G["cap"])
    finder.enableRollingMap(0.25, G["extent"])
    finder.setRollingDedup(G["res"])
    p = S.PARAMS
    finder.setParam(p["safety_margin"], p["search_margin"], p["max_radius"], 30.0)
    finder.setPt((0.0, 0.0, 0.0), (7.0, 0.0, 0.0), -1.0, 9.0, -9.0, 9.0, -7.0, 7.0, 30.0, 1000, p["sample_portion"], p["goal_portion"])
    centre = (G["obstacle_x"], 0.0, 0.0)
    hits = []
    got = S.run_rgbd_window_scenario(finder, D.render, each=lambda k, f: hits.append(f.checkTrajPtCol(centre)))
    assert len(got) == len(want) == 6
    for k, (a, b) in enumerate(zip(got, want)):
        assert a == b, f"frame {k}: {len(a)} live points, the model has {len(b)}"
    assert hits == [True] * G["obstacle_frames"] + [False] * (6 - G["obstacle_frames"]), hits
    cloud = finder.cloud()
    assert len(cloud) == model.count and cloud.ring_live() == (model.live_count(), model.count - model.live_count())
    finder.close()
