"""GPU tests of the engine's grow-only buffers (csrc/hostmem.hpp): the smallest shapes that cross each growth boundary while the
object that owns the buffer is in use, and the count of live blocks once every handle is closed.

References: the numpy models of the neighbouring tests -- tests/helpers (ring_dedup_model, ring_remove_model, depth_model,
bezier_model, segment_search_model), ref_knn of test_gpu_knn.py, ref_masks / rows_from of test_gpu_radius_search.py, ref_inflate of
test_gpu_ring_remove.py.  Every comparison is exact."""
import ctypes
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from pointcloudtraj_amd import synth
from test_gpu_depth import check_rows, points_in_view, random_image, window_pair
from test_gpu_expand_ring import expand, make_nodes
from test_gpu_knn import ref_knn
from test_gpu_radius_search import check as check_lists, ref_masks, rows_from
from test_gpu_ring_remove import PRM, check_counts, params, ref_inflate, traj_through
from test_gpu_segments import segments
from test_depth_api import random_view

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "helpers"))
import bezier_model as B  # noqa: E402
import depth_model as D  # noqa: E402
import ring_dedup_model as M  # noqa: E402
import ring_remove_model as R  # noqa: E402
import segment_search_model as SS  # noqa: E402

pytestmark = pytest.mark.gpu

BOX = (20.0, 20.0, 20.0)


@pytest.fixture(scope="module")
def E():
    from pointcloudtraj_amd import engine
    engine.init(0)
    return engine


def check_nn(c, win, q, tag):
    wi, wd = ref_knn(win, q, 1)
    gi, gd = c.nn(q)
    assert np.array_equal(gd, wd[:, 0]) and np.array_equal(gi, wi[:, 0]), f"{tag}: nearest neighbours"


# ---- 1. the two host-mapped frame staging buffers ----------------------------------------------------------------------------------
# 64 KiB hold bytes + 64: 5 456 points of 12 B are the last frame that fits; 10 918 points are the first past 128 KiB
STAGING_FRAMES = (100, 5456, 5457, 10918)


def staging_rounds(E):
    """copied frames through the library's own staging buffer, then the same sizes as zero-copy frames through the producer's; after
    every append 256 NN queries against the host mirror of the window"""
    cap = 20_000
    c, w = E.Cloud(cap), M.DedupWindow(cap, M.RES)
    c.ring_index(0.5, BOX)
    q = synth.uniform_points(411, 256, 0, 20)
    for zero_copy in (False, True):
        for k, n in enumerate(STAGING_FRAMES):
            f = synth.uniform_points(420 + 10 * zero_copy + k, n, 0, 20)
            if zero_copy:
                c.frame_buffer(n)[:] = f
                c.append_frame(n)
            else:
                c.append(f)
            w.append_plain(f)
            assert len(c) == w.count
            check_nn(c, w.live(), q, f"{'zero-copy' if zero_copy else 'copied'} frame of {n}")
    assert w.count == cap and w.nxt == (2 * sum(STAGING_FRAMES)) % cap           # the ring wrapped
    c.close()


def test_frame_staging_grows_under_appends(E):
    staging_rounds(E)


def test_frame_staging_grows_under_synchronous_appends():
    """the same round with PCT_ASYNC_APPEND=0; the switch is read once per process, hence a child"""
    root = os.path.dirname(HERE)
    env = dict(os.environ, PCT_ASYNC_APPEND="0", PYTHONPATH=os.pathsep.join([root, HERE, os.environ.get("PYTHONPATH", "")]))
    code = "import test_gpu_buffer_growth as T; from pointcloudtraj_amd import engine; engine.init(0); T.staging_rounds(engine); print('rounds ok')"
    r = subprocess.run([sys.executable, "-c", code], env=env, cwd=root, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "rounds ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


# ---- 2. the frame filter's table and per-point scratch ---------------------------------------------------------------------------------

def dedup_rounds(E):
    """frames of 300, 600 and 5 000 points: the key table goes 1024 -> 2048 -> 16384 entries, the per-point scratch grows twice"""
    cap = 8000
    c, w = E.Cloud(cap), M.DedupWindow(cap, M.RES)
    c.ring_index(0.25, (8.0, 8.0, 8.0))
    c.ring_dedup(M.RES)
    q = synth.uniform_points(431, 128, 0, 6)
    a = synth.uniform_points(432, 300, 0, 6)
    b = np.concatenate([a[:200], synth.uniform_points(433, 400, 0, 6)])              # 200 points the window holds already
    d = np.concatenate([b[100:350], synth.uniform_points(434, 4500, 0, 6), b[100:350]])    # repeats of the window and of the frame itself
    for f in (a, b, d):
        f = np.ascontiguousarray(f, np.float32)
        c.append(f)
        want = w.append(f)
        last = c.ring_dedup_last()
        assert (last["offered"], last["kept"]) == (len(f), int(want.sum())), f"frame of {len(f)}: {last['kept']} kept, the model keeps {int(want.sum())}"
        assert np.array_equal(last["flags"], want), f"frame of {len(f)}: kept flags"
        assert len(c) == w.count and (len(f) == 300 or 0 < want.sum() < len(f))
        check_rows(c, w, f"frame of {len(f)}")
        check_nn(c, w.live(), q, f"frame of {len(f)}")
    c.close()


def test_dedup_scratch_grows_under_appends(E):
    dedup_rounds(E)


# ---- 3. depth staging, the un-projection's scratch, the classifier's workspaces ------------------------------------------------------------

def depth_rounds(E):
    """64 x 48 (under the 4096-pixel scratch floor and the 16 384-float stage floor), 160 x 120 (over both), 64 x 48 again: carve and
    append against the model; then pct_depth_classify with one small view and 500 points, and three large views and 3 000 points"""
    rng = np.random.default_rng(440)
    cap = 24_000
    c, w = window_pair(E, cap, dedup=True)
    views = [random_view(rng, 64, 48)]
    views.append(E.depth_view(list(views[0].t), np.array(list(views[0].R)).reshape(3, 3), 160, 120, focal=views[0].focal))
    views.append(views[0])
    pre = points_in_view(rng, views[0], 3000)
    c.append(pre)
    w.append(pre)
    for k, view in enumerate(views):
        tag = f"image {k} ({view.width} x {view.height})"
        img = random_image(rng, view, 0.2, 22.0)
        got, want = c.ring_carve_depth(view, img, 0.05), w.carve(view, img, 0.05)
        assert got == want and want > 0, f"{tag}: carved {got}, the model carves {want}"
        check_counts(c, w, tag)
        check_rows(c, w, tag)
        offered, kept = c.append_depth(view, img, 18.0)
        frame, flags = w.append_depth(view, img, 18.0)
        assert (offered, kept) == (len(frame), int(flags.sum())) and kept > 0, f"{tag}: offered {offered} / kept {kept}, the model {len(frame)} / {int(flags.sum())}"
        assert np.array_equal(c.ring_dedup_last()["flags"], flags), f"{tag}: kept flags"
        check_counts(c, w, tag)
        check_rows(c, w, tag)
    c.close()
    for nv, (wd, ht), n in ((1, (64, 48), 500), (3, (160, 120), 3000)):
        vs = [random_view(rng, wd, ht) for _ in range(nv)]
        imgs = [random_image(rng, v) for v in vs]
        pts = np.concatenate([points_in_view(rng, v, n // nv) for v in vs]).astype(np.float64)
        seen_by, pixel = E.depth_classify(vs, imgs, pts, 0.05)
        ws, wp = D.classify(vs, imgs, pts, 0.05)
        assert np.array_equal(seen_by, ws) and np.array_equal(pixel, wp), f"classify with {nv} views"
        assert (ws >= 0).any() and (ws < 0).any()


def test_depth_staging_grows_between_images(E):
    depth_rounds(E)


# ---- 4. the staging of a removal's index list ------------------------------------------------------------------------------------------

def removal_rounds(E):
    """lists of 1 000 (under the 1024 floor), 1 025 and 3 000 indices on a 10 000-point window"""
    cap = 10_000
    c, w = E.Cloud(cap), R.RemoveWindow(cap)
    c.ring_index(0.5, BOX)
    pts = synth.uniform_points(451, cap, 0, 20)
    c.append(pts)
    w.append_plain(pts)
    q = synth.uniform_points(452, 128, 0, 20)
    rng = np.random.default_rng(453)
    for n in (1000, 1025, 3000):
        idx = rng.choice(cap, n, replace=False).astype(np.uint32)
        idx[-5:] = idx[:5]                                                           # a point named twice counts once
        got, want = c.ring_remove_indices(idx), w.remove_indices(idx)
        assert got == want and want > 0, f"list of {n}: removed {got}, the model removes {want}"
        check_counts(c, w, f"list of {n}")
        wi, wd = ref_knn(w.live(), q, 5)
        gi, gd = c.knn(q, 5)
        assert np.array_equal(gd, wd) and np.array_equal(gi, wi), f"list of {n}: 5-NN over the window with its NaN rows"
    c.close()


def test_removal_list_grows(E):
    removal_rounds(E)


# ---- 5. query workspaces under captured plans -----------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def plan_case():
    """(points, queries, 64-NN reference rows), computed once"""
    pts = synth.uniform_points(461, 20_000, 0, 20)
    q = synth.uniform_points(462, 5000, 0, 20)
    return (pts, q) + ref_knn(pts, q, 64)


def plan_rounds(E):
    """256 queries reserved, an NN plan and a replan plan captured; then k-NN batches and radius searches that grow the query
    workspaces, the k-NN rows and the lists; the plans run again (re-captured by the generation count)"""
    pts, q, ki, kd = plan_case()
    c = E.Cloud(len(pts))
    c.set_input(pts)
    c.build_grid()
    c.reserve_queries(256)
    nn_plan, re_plan = E.NNPlan(c, 256), E.ReplanPlan(c, 32, 128, 2)
    nodes = synth.uniform_points(463, 32, 2, 8).astype(np.float64)
    coef, T, od = traj_through()

    def run_plans(tag):
        gi, gd = nn_plan.run(q[:256])
        assert np.array_equal(gd, kd[:256, 0]) and np.array_equal(gi, ki[:256, 0]), f"{tag}: the NN plan"
        r = re_plan.run(params(E), nodes, coef, T, od, 0.0, 2.0, 0.02)
        wr, wi, wd = ref_inflate(pts, PRM, nodes)
        assert np.array_equal(r["node_radius"], wr) and np.array_equal(r["node_d2"], wd) and np.array_equal(r["node_idx"], wi), f"{tag}: the replan plan's nodes"
        wr, wi, wd = ref_inflate(pts, PRM, r["sample_pos"])
        neg = np.flatnonzero(wr < 0.0)
        assert r["nsamples"] == len(r["sample_pos"]) >= 99 and np.array_equal(r["sample_radius"], wr) and np.array_equal(r["sample_d2"], wd), f"{tag}: the replan plan's samples"
        assert np.array_equal(r["sample_idx"], wi) and r["first_hit_sample"] == (int(neg[0]) if len(neg) else -1), f"{tag}: the replan plan's samples"

    run_plans("as captured")
    for Q, k in ((256, 8), (256, 64), (5000, 64)):
        gi, gd = c.knn(q[:Q], k)
        assert np.array_equal(gd, kd[:Q, :k]) and np.array_equal(gi, ki[:Q, :k]), f"k-NN of {Q} x {k}"
    for r, lo, hi in ((0.7, 500, 2_000), (3.3, 60_000, 140_000)):
        masks = ref_masks(pts, q[:256], np.float32(r))
        want = rows_from(masks, 1)
        assert lo < len(want[1]) < hi, len(want[1])
        check_lists(c.radius_search(q[:256], np.float32(r), 1), want, f"radius search at {r}")
    run_plans("after the workspaces grew")
    nn_plan.close()
    re_plan.close()
    c.close()


def test_query_workspaces_grow_under_captured_plans(E):
    plan_rounds(E)


# ---- 6. the sampled Bezier check's coefficient staging -----------------------------------------------------------------------------------------

def bezier_traj(nseg, order, seed):
    """nseg segments of one order; control points advance ~1.5 m per segment with +-0.3 m of jitter, stored divided by the segment time"""
    m = order + 1
    times = np.float64([0.30 + 0.05 * (k % 5) for k in range(nseg)])
    r = (synth.splitmix64(seed, 3 * nseg * m) >> np.uint64(11)).astype(np.float64) * 2.0 ** -53
    coef = np.zeros((nseg, 3 * m))
    for s in range(nseg):
        for d in range(3):
            coef[s, d * m:(d + 1) * m] = s * 1.5 + np.linspace(0, 1.5, m) + (r[(3 * s + d) * m:(3 * s + d + 1) * m] - 0.5) * 0.6
    return coef / times[:, None], times, np.full(nseg, order, np.int32)


def bezier_rounds(E):
    """the staged host form and the device form, each with 2 segments of order 3 and then 12 segments of order 12 on one cloud; more
    than 1024 samples under a cap of 4096, which the one-launch form does not take"""
    import torch
    pts = synth.uniform_points(471, 3000, -2, 20)
    prm = dict(start=(0.0, 0.0, 0.0), sample_range=100.0, search_margin=0.25, max_radius=1.5)
    cap = B.CAP_MAX
    dev = torch.device("cuda", 0)
    buf = dict(pos=torch.empty(3 * cap, dtype=torch.float64, device=dev), rad=torch.empty(cap, dtype=torch.float64, device=dev),
               d2=torch.empty(cap, dtype=torch.float64, device=dev), idx=torch.empty(cap, dtype=torch.int32, device=dev),
               fh=torch.empty(1, dtype=torch.int64, device=dev), ns=torch.empty(1, dtype=torch.int32, device=dev))
    stream = torch.cuda.Stream(device=dev)
    for form in ("host", "dev"):
        c = E.Cloud(len(pts))
        c.set_input(pts)
        c.reserve_queries(cap)
        for nseg, order, dt in ((2, 3, 0.0006), (12, 12, 0.004)):
            coef, T, od = bezier_traj(nseg, order, 472 + nseg)
            want = B.model_check(pts, prm, coef, T, od, 0.0, 100.0, dt, cap)
            B.assert_unique_nearest(pts, want)
            assert 1024 < want["n"] <= cap
            p = E.inflate_params(prm["start"], prm["sample_range"], prm["search_margin"], prm["max_radius"])
            if form == "host":
                r = c.bezier_check(p, coef, T, od, 0.0, 100.0, dt=dt, cap=cap)
                n, fh, pos, rad, d2, idx = r["n"], r["first_hit"], r["pos"], r["radius"], r["d2"], r["idx"]
            else:
                keep = c.bezier_check_device(p, coef, T, od, 0.0, 100.0, dt, cap, buf["pos"].data_ptr(), buf["rad"].data_ptr(), buf["d2"].data_ptr(),
                                             buf["idx"].data_ptr(), buf["fh"].data_ptr(), buf["ns"].data_ptr(), stream.cuda_stream)
                stream.synchronize()
                del keep
                n, fh = int(buf["ns"].item()), int(buf["fh"].item())
                pos, rad, d2 = (buf[k].cpu().numpy()[:s * n].reshape(*sh) for k, s, sh in (("pos", 3, (n, 3)), ("rad", 1, (n,)), ("d2", 1, (n,))))
                idx = buf["idx"].cpu().numpy()[:n].view(np.uint32)
            tag = f"{form} form, {nseg} segments of order {order}"
            assert n == want["n"] and fh == want["first_hit"], tag
            assert np.array_equal(pos, want["pos"]), f"{tag}: positions"
            assert np.array_equal(d2, want["d2"]) and np.array_equal(rad, want["radius"]), f"{tag}: distances and radii"
            assert np.array_equal(idx.astype(np.int64), np.where(want["idx"] < 0, np.int64(E.NO_INDEX), want["idx"])), f"{tag}: indices"
        c.close()


def test_bezier_staging_grows_between_trajectories(E):
    bezier_rounds(E)


# ---- 7. the groups of buffers that share one capacity (hostmem.hpp regrow) ------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def group_case():
    """(5000 uniform points, 4097 queries, the queries' nearest neighbours, their counts within GROUP_R), computed once"""
    pts = synth.uniform_points(491, 5000, 0, 10)
    q = synth.uniform_points(492, 4097, 0, 10)
    ni, nd = ref_knn(pts, q, 1)
    counts = np.concatenate([np.array([int(hit.sum()) for _, hit in ref_masks(pts, q[a:a + 512], GROUP_R)], np.uint32) for a in range(0, len(q), 512)])
    return pts, q, ni[:, 0], nd[:, 0], counts


GROUP_R = np.float32(0.8)


def grid_cloud(E, pts):
    c = E.Cloud(len(pts))
    c.set_input(pts)
    c.build_grid()
    return c


def test_query_and_list_search_workspaces_regrow_together(E):
    """256 queries are the floor of the query workspaces; 257 regrow them and, behind them, the list search's scan / cursor / queue"""
    pts, q = group_case()[:2]
    c = grid_cloud(E, pts)
    for Q in (256, 257):
        want = rows_from(ref_masks(pts, q[:Q], GROUP_R), 1)
        assert want[0][-1] > Q
        check_lists(c.radius_search(q[:Q], GROUP_R, 1), want, f"radius search of {Q} queries")
    c.close()


def test_list_stores_regrow_and_are_reused(E):
    """a small total, a larger one (the store regrows), the small one again (it does not); the capsule search's store carries s"""
    pts, q = group_case()[:2]
    c = grid_cloud(E, pts)
    totals = []
    for r in (0.4, 2.0, 0.4):
        want = rows_from(ref_masks(pts, q[:64], np.float32(r)), 1)
        totals.append(int(want[0][-1]))
        check_lists(c.radius_search(q[:64], np.float32(r), 1), want, f"radius search at {r}")
    assert 0 < totals[0] == totals[2] < totals[1] // 20
    segs = segments(493, 64, 0.0, 10.0, [0.0, 0.05, 3.0, 6.0], pts)
    totals = []
    for reach in (0.3, 1.5, 0.3):
        want = SS.segment_search(pts, segs, reach, 1)
        totals.append(int(want[0][-1]))
        go, gi, gd, gs = c.segment_search(segs, reach, 1)
        check_lists((go, gi, gd), want[:3], f"capsule search at {reach}")
        assert gs.dtype == np.float64 and np.array_equal(gs, want[3]), f"capsule search at {reach}: s"
    assert 0 < totals[0] == totals[2] < totals[1] // 10
    c.close()


def test_knn_rows_regrow(E):
    pts, q = group_case()[:2]
    ki, kd = ref_knn(pts, q[:5], 64)
    c = grid_cloud(E, pts)
    for Q, k in ((3, 2), (3, 3), (5, 64), (3, 2)):
        gi, gd = c.knn(q[:Q], k)
        assert np.array_equal(gd, kd[:Q, :k]) and np.array_equal(gi, ki[:Q, :k]), f"k-NN of {Q} x {k}"
    c.close()


def test_mapped_io_regrows_at_its_floor(E):
    """4096 queries fill the floor of the host-mapped query / result buffers, 4097 double it (both between the express limit of 1024
    and the mapped path's 65536)"""
    pts, q, ni, nd, counts = group_case()
    assert counts.min() < counts.max()
    c = grid_cloud(E, pts)
    for Q in (4096, 4097):
        gi, gd = c.nn(q[:Q])
        assert np.array_equal(gd, nd[:Q]) and np.array_equal(gi, ni[:Q]), f"NN of {Q} queries"
        cnt = c.radius_count(q[:Q], GROUP_R)
        assert cnt.dtype == np.uint32 and np.array_equal(cnt, counts[:Q]), f"radius count of {Q} queries"
    c.close()


# ---- 8. nothing left behind ---------------------------------------------------------------------------------------------------------------------

def other_handles(E):
    """the handles items 1-6 do not make: a small node cloud with the fused expansion over a grid cloud, a voxel map, one pct_traj call,
    a 4-dimensional node set grown from 2 rows past its floor of 1024 (with a copy)"""
    from pointcloudtraj_amd import traj as TJ, voxel
    pts = synth.uniform_points(481, 5000, 0, 10)
    c = E.Cloud(len(pts))
    c.set_input(pts)
    c.build_grid()
    nodes = make_nodes(E, 482, 200, 0.0, 10.0)
    expand(E, nodes, c, params(E), synth.uniform_rows_f64(483, 16, 3, 0.0, 10.0))
    nodes.close()
    c.close()
    v = voxel.VoxelMap(0.1, 1000)
    v.add_point_cloud(pts)
    v.add_point_cloud(synth.uniform_points(484, 20_000, 0, 10))                      # the store and the table grow with a copy
    v.close()
    coef, T, od = traj_through()
    TJ.wire_sample(TJ.get_bezier_traj_wire(coef, T, od), 11)
    L, dp, h = E.lib(), ctypes.POINTER(ctypes.c_double), ctypes.c_void_p()
    assert L.pct_nodeset_create(4, 2, ctypes.byref(h)) == 0
    rows = np.round(synth.uniform_rows_f64(485, 1500, 4, 0.0, 3.0))
    for a in (0, 1000):                                                              # the second append takes the set past its 1024 rows: new blocks and a copy
        blk = np.ascontiguousarray(rows[a:a + 1000])
        assert L.pct_nodeset_append(h, blk.ctypes.data_as(dp), len(blk)) == 0
    idx, ties, d2 = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_double()
    qq = np.float64([1, 2, 1, 2])
    d = (rows - qq) ** 2
    sq = ((d[:, 0] + d[:, 1]) + d[:, 2]) + d[:, 3]
    assert L.pct_nodeset_nearest(h, qq.ctypes.data_as(dp), ctypes.byref(idx), ctypes.byref(d2), ctypes.byref(ties)) == 0
    assert d2.value == sq.min() and idx.value == int(np.flatnonzero(sq == sq.min())[0]) and ties.value == int((sq == sq.min()).sum())
    assert L.pct_nodeset_destroy(h) == 0


def test_closed_handles_leave_no_buffer_behind(E):
    """pct_debug_live_buffers before and after one of every handle: blocks and bytes are back at the baseline, twice.  The
    process-wide workspaces of pct_traj_* and pct_depth_classify (never freed, grow-only) are brought to their final size first."""
    def everything():
        staging_rounds(E)
        dedup_rounds(E)
        depth_rounds(E)
        removal_rounds(E)
        plan_rounds(E)
        bezier_rounds(E)
        other_handles(E)

    depth_rounds(E)
    other_handles(E)
    E.sync()
    base = E.live_buffers()
    assert base[0] >= 0 and base[1] >= 0
    for rnd in (1, 2):
        everything()
        E.sync()
        assert E.live_buffers() == base, f"round {rnd}: {E.live_buffers()} blocks / bytes live, {base} before"
