"""GPU tests of the trajectory clearance (pct_bezier_clearance_batch, pct_bezier_clearance_batch_dev; include/pct_engine.h, paragraph
"Trajectory clearance") against the numpy restatement in tests/helpers/bezier_clearance_model.py.

Everything is compared byte for byte: the 48-byte records and the three stats.  Clouds, as in the certified check's test: an un-indexed
(plain), a cell-indexed (grid), a wrapped rolling map with removed rows (ring) and an empty cloud; forms: the host form and the device
form (torch buffers, a side stream); paths: every algo the cloud admits.  The scene is the certified check's (300 points, 64
trajectories of three segments, orders 0..12)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import bezier_certify_model as CM  # noqa: E402
import bezier_clearance_model as KM  # noqa: E402

pytestmark = pytest.mark.gpu

PCT_ERR_INVALID = 2
KINDS = ("plain", "grid", "ring", "empty")
FORMS = ("host", "dev")
DEV_CAP = 1024                         # piece_cap of the device-form runs: ample for every case here (asserted from the model's rounds)
DEPTH = 12                             # max_depth of the scene runs: the model needs 7
TOL = 0.01
SENTINEL = 0x5A
INF = float("inf")


@pytest.fixture(scope="module")
def E():
    from pointcloudtraj_amd import engine
    engine.init(0)
    return engine


def ring_window():
    """the scene's 300 points appended in frames of 100 into a ring of 256 slots (it wraps: slots 0..43 hold points 256..299), then every
    row within 1.2 m of (5, 5, 5) removed: the window as the model sees it, NaN in the removed rows"""
    pts = CM.scene()[0]
    win = np.array(pts[:256])
    win[:44] = pts[256:]
    d = win.astype(np.float64) - 5.0
    inside = ((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]) <= 1.2 * 1.2
    out = win.copy()
    out[inside] = np.nan
    return out, int(inside.sum())


class Rig:
    def __init__(self, E):
        self.E, self.clouds, self.stream = E, {}, None

    def cloud(self, kind):
        """(cloud, the rows the model sees, the algos the cloud admits)"""
        E = self.E
        if kind not in self.clouds:
            pts = CM.scene()[0]
            if kind == "plain":
                c = E.Cloud(len(pts))
                c.set_input(pts)
                self.clouds[kind] = (c, pts, (E.ALGO_AUTO, E.ALGO_STREAM))
            elif kind == "grid":
                c = E.Cloud(len(pts))
                c.set_input(pts)
                c.build_grid()
                self.clouds[kind] = (c, pts, (E.ALGO_AUTO, E.ALGO_GRID, E.ALGO_STREAM))
            elif kind == "ring":
                c = E.Cloud(256)
                c.ring_index(1.0, (10.0, 10.0, 10.0))
                for f in range(3):
                    c.append(pts[100 * f:100 * f + 100])
                win, n_removed = ring_window()
                assert n_removed > 0 and c.ring_remove_ball((5.0, 5.0, 5.0), 1.2) == n_removed
                self.clouds[kind] = (c, win, (E.ALGO_AUTO, E.ALGO_RING, E.ALGO_STREAM))
            else:
                self.clouds[kind] = (E.Cloud(16), np.zeros((0, 3), np.float32), (E.ALGO_AUTO, E.ALGO_STREAM))
        return self.clouds[kind]

    def side_stream(self):
        import torch
        if self.stream is None:
            self.stream = torch.cuda.Stream(device=torch.device("cuda", 0))
        return self.stream

    def close(self):
        for c, _, _ in self.clouds.values():
            c.close()


@pytest.fixture(scope="module")
def rig(E):
    r = Rig(E)
    yield r
    r.close()


def run(rig, form, c, trajs, tol, cap, max_depth, piece_cap, algo, expect=0, want_stats=True, packed=None):
    """one call of either form into sentinel-filled buffers with one record more than asked for; returns (records, stats) after
    asserting that nothing behind them was written -- or, on a refusal (status asserted == expect), that nothing was written"""
    E = rig.E
    batch, arr = packed if packed is not None else E.pack_trajectories(trajs)
    B = int(batch.B)
    if form == "host":
        rec = np.full((max(B, 0) + 1) * 48, SENTINEL, np.uint8)
        stats = np.full(4, -77, np.int64)
        st = E.lib().pct_bezier_clearance_batch(c.handle, algo, C.byref(batch), float(tol), float(cap), int(max_depth), int(piece_cap), rec.ctypes.data,
                                                stats.ctypes.data if want_stats else None)
    else:
        import torch
        dev = torch.device("cuda", 0)
        t = {k: torch.from_numpy(v).to(dev) for k, v in arr.items() if v is not None}
        dbatch = E.BezierBatch(t["polycoef"].data_ptr() or None, batch.row_stride, t["seg_time"].data_ptr() or None, t["orders"].data_ptr() or None,
                               t["seg_offsets"].data_ptr() or None, None, B)
        tc = torch.full(((max(B, 0) + 1) * 48,), SENTINEL, dtype=torch.uint8, device=dev)
        ts = torch.full((4,), -77, dtype=torch.int64, device=dev)
        if 0 < piece_cap <= (1 << 20):
            c.reserve_queries(2 * piece_cap)
        torch.cuda.synchronize()
        s = rig.side_stream()
        st = E.lib().pct_bezier_clearance_batch_dev(c.handle, algo, C.byref(dbatch), float(tol), float(cap), int(max_depth), int(piece_cap), tc.data_ptr(),
                                                    ts.data_ptr() if want_stats else None, s.cuda_stream)
        s.synchronize()
        rec, stats = tc.cpu().numpy(), ts.cpu().numpy()
        del t
    assert st == expect, (st, E.lib().pct_last_error())
    if st != 0:
        assert np.all(rec == SENTINEL) and np.all(stats == -77), "a refused call wrote something"
        return None, None
    assert np.all(rec[48 * B:] == SENTINEL) and stats[3] == -77, "entries behind the records or the stats were written"
    if not want_stats:
        assert np.all(stats == -77)
    return rec[:48 * B].view(KM.CLR_DTYPE), stats[:3]


def same(got, want, tag):
    gc, gs = got
    wc, ws = want[0], want[1]
    print(f"{tag}: statuses {np.bincount(gc['status'], minlength=3)} (model {np.bincount(wc['status'], minlength=3)}), stats {gs} (model {ws})")
    for name in KM.CLR_DTYPE.names:
        assert np.array_equal(gc[name], wc[name], equal_nan=gc[name].dtype.kind == "f"), f"{tag}: {name}"
    assert gc.tobytes() == wc.tobytes(), f"{tag}: record bytes"
    assert np.array_equal(gs, ws), f"{tag}: stats"


_model_cache = {}


def model(kind_rows, key, trajs, tol, cap, max_depth, piece_cap, index_base=0):
    """(records, stats, live count per round) of the model, computed once per case"""
    k = (key, len(trajs), float(tol), float(cap), max_depth, piece_cap, index_base)
    if k not in _model_cache:
        trace = []
        rec, stats = KM.clearances(kind_rows, *KM.pack(trajs), tol, cap, max_depth, piece_cap, index_base, trace=trace)
        rec.setflags(write=False)
        _model_cache[k] = (rec, stats, trace)
    return _model_cache[k]


# ---- 1. the scene: every cloud, both forms, every path ----------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("kind", KINDS)
def test_scene_byte_for_byte(E, rig, kind, form):
    c, rows, algos = rig.cloud(kind)
    trajs = CM.scene()[1]
    cap = DEV_CAP if form == "dev" else 1 << 16
    want = model(rows, kind, trajs, TOL, INF, DEPTH, cap)
    assert want[1][2] == 0 and max(want[2]) <= DEV_CAP and want[0]["depth"].max() < DEPTH
    if kind == "empty":
        assert np.all(want[0]["status"] == KM.DONE) and np.all(want[0]["depth"] == 0) and list(want[1]) == [1, 192, 0]
        assert np.all(want[0]["lo"] == np.inf) and np.all(want[0]["hi"] == np.inf)
    else:
        assert np.all(want[0]["status"] == KM.DONE) and want[1][0] >= 6 and np.all(want[0]["hi"] - want[0]["lo"] <= TOL)
    if kind == "plain":
        full = KM.scene_clearances(TOL, INF)
        assert max(full[2]) == KM.SCENE_GAVE[(TOL, INF)][2] and want[0].tobytes() == full[0].tobytes()
    for algo in algos:
        same(run(rig, form, c, trajs, TOL, INF, DEPTH, cap, algo), want, f"{kind} {form} algo {algo}")


@pytest.mark.parametrize("form", FORMS)
def test_cap_and_a_coarser_tol(E, rig, form):
    trajs = CM.scene()[1]
    for kind, tol, cap in (("grid", 0.05, 0.5), ("ring", 0.01, 0.5), ("plain", 0.05, INF)):
        c, rows, algos = rig.cloud(kind)
        want = model(rows, kind, trajs, tol, cap, DEPTH, DEV_CAP)
        assert want[1][2] == 0 and np.all(want[0]["status"] == KM.DONE)
        if cap < INF:
            assert np.any(want[0]["hi"] - want[0]["lo"] > tol)          # retired against the cap
        same(run(rig, form, c, trajs, tol, cap, DEPTH, DEV_CAP, algos[1]), want, f"{kind} {form} tol {tol} cap {cap}")


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("max_depth", (0, 2))
def test_depth_caps_give_open(E, rig, form, max_depth):
    trajs = CM.scene()[1]
    for kind in ("grid", "ring"):
        c, rows, algos = rig.cloud(kind)
        want = model(rows, kind, trajs, TOL, INF, max_depth, DEV_CAP)
        assert np.sum(want[0]["status"] == KM.OPEN) >= 32 and want[0]["depth"].max() == max_depth and want[1][0] == max_depth + 1
        same(run(rig, form, c, trajs, TOL, INF, max_depth, DEV_CAP, algos[1]), want, f"{kind} {form} depth cap {max_depth}")


@pytest.mark.parametrize("form", FORMS)
def test_piece_cap_rule(E, rig, form):
    """piece_cap one below what round 1 wants: round 0's splits are refused (capped, owners OPEN, their L folded); at it: round 1 runs"""
    c, rows, _ = rig.cloud("grid")
    trajs = CM.scene()[1]
    round1 = model(rows, "grid", trajs, TOL, INF, DEPTH, DEV_CAP)[2][1]
    assert 192 < round1 <= DEV_CAP
    flags = []
    for cap in (round1 - 1, round1):
        want = model(rows, "grid", trajs, TOL, INF, 3, cap)
        flags.append((int(want[1][0]), int(want[1][2])))
        same(run(rig, form, c, trajs, TOL, INF, 3, cap, E.ALGO_GRID), want, f"{form} piece_cap {cap}")
    assert flags[0] == (1, 1) and flags[1][0] >= 2, flags


def tile_case(n_near):
    """one cloud point at the origin; n_near lines 2 m long pass 0.1 m beside it (ends 1 m away: they split in round 0) and every third
    segment in between is 0.5 m long and 5 m away (it retires at once at tol 0.3), spread over five trajectories: exactly n_near pieces
    split in round 0"""
    pts = np.zeros((1, 3), np.float32)
    rows = []
    near = 0
    while near < n_near:
        if len(rows) % 3 == 2:
            rows.append(np.array([-0.25, 0.25, 5.0, 5.0, 0.0, 0.0]))
        else:
            y = 0.1 + 1e-4 * near
            near += 1
            rows.append(np.array([-1.0, 1.0, y, y, 0.0, 0.0]))
    rows = np.array(rows)
    cuts = np.linspace(0, len(rows), 6).astype(int)
    trajs = [(rows[a:b] / 2.0, np.full(b - a, 2.0), np.ones(b - a, np.int32)) for a, b in zip(cuts[:-1], cuts[1:])]
    return pts, trajs


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("n_near", (255, 256, 257))
def test_splitting_pieces_around_a_scan_tile(E, form, rig, n_near):
    pts, trajs = tile_case(n_near)
    trace = []
    want = KM.clearances(pts, *KM.pack(trajs), 0.3, INF, 1, DEV_CAP, trace=trace)
    assert trace == [sum(len(t) for _, t, _ in trajs), 2 * n_near] and want[1][2] == 0
    c = E.Cloud(16)
    c.set_input(pts)
    try:
        same(run(rig, form, c, trajs, 0.3, INF, 1, DEV_CAP, E.ALGO_STREAM), want, f"{form} {n_near} splitting pieces")
    finally:
        c.close()


@pytest.mark.parametrize("form", FORMS)
def test_small_batches_index_base_and_an_invalid_trajectory(E, rig, form):
    c, rows, _ = rig.cloud("plain")
    trajs = CM.scene()[1]
    # B = 0: PCT_OK, zero stats, no record
    got = run(rig, form, c, [], TOL, INF, DEPTH, DEV_CAP, E.ALGO_AUTO)
    assert len(got[0]) == 0 and np.all(got[1] == 0)
    run(rig, form, c, [], TOL, INF, DEPTH, DEV_CAP, E.ALGO_AUTO, want_stats=False)
    # B = 1, with and without stats: the bytes of its entry in the whole scene, up to the segment numbering
    want = model(rows, "plain", trajs[5:6], TOL, INF, DEPTH, DEV_CAP)
    whole = model(rows, "plain", trajs, TOL, INF, DEPTH, DEV_CAP)[0][5:6].copy()
    whole["at_seg"] -= 15
    assert whole.tobytes() == want[0].tobytes()
    same(run(rig, form, c, trajs[5:6], TOL, INF, DEPTH, DEV_CAP, E.ALGO_AUTO), want, f"{form} B = 1")
    got = run(rig, form, c, trajs[5:6], TOL, INF, DEPTH, DEV_CAP, E.ALGO_AUTO, want_stats=False)
    assert got[0].tobytes() == want[0].tobytes()
    # INVALID trajectories between valid ones: seg_time 0, negative, NaN, +inf, and a control point beyond FLT_MAX
    mixed = list(trajs[4:7]) + [trajs[30]]
    for k, bad_T in enumerate((0.0, -1.0, np.nan, np.inf)):
        coef, T, od = trajs[10 + k]
        T = T.copy()
        T[k % 3] = bad_T
        mixed.insert(1 + 2 * k, (coef, T, od))
    coef, T, od = trajs[20]
    coef = coef.copy()
    coef[1, 0] = 3.5e38 / T[1]
    mixed.append((coef, T, od))
    mixed.append(trajs[21])
    want = KM.clearances(rows, *KM.pack(mixed), TOL, INF, DEPTH, DEV_CAP)
    bad = want[0]["status"] == KM.INVALID
    assert list(np.nonzero(bad)[0]) == [1, 3, 5, 7, 8] and np.all(np.isnan(want[0]["lo"][bad])) and np.all(want[0]["pieces"][bad] == 0)
    same(run(rig, form, c, mixed, TOL, INF, DEPTH, DEV_CAP, E.ALGO_STREAM), want, f"{form} INVALID between valid ones")
    # the index base is added to the reported index
    base = E.Cloud(len(rows))
    try:
        base.set_index_base(1000)
        base.set_input(rows)
        want = KM.clearances(rows, *KM.pack(trajs[5:7]), TOL, INF, DEPTH, DEV_CAP, index_base=1000)
        assert np.all(want[0]["at_idx"] >= 1000)
        same(run(rig, form, base, trajs[5:7], TOL, INF, DEPTH, DEV_CAP, E.ALGO_AUTO), want, f"{form} index base")
    finally:
        base.close()


@pytest.mark.parametrize("form", FORMS)
def test_hand_cases(E, rig, form):
    """the 4 mm line, a row exactly on the curve's end, segments of order 0, tol = 0"""
    c = E.Cloud(16)
    try:
        pts, traj = KM.FOUR_MM["pts"], KM.FOUR_MM["traj"]
        c.set_input(pts)
        for tol, depth in ((0.001, 16), (0.0, 6)):
            want = KM.clearances(pts, *KM.pack([traj]), tol, INF, depth, DEV_CAP)
            got = run(rig, form, c, [traj], tol, INF, depth, DEV_CAP, E.ALGO_AUTO)
            same(got, want, f"{form} 4 mm line tol {tol}")
            r = got[0][0]
            assert r["status"] == (KM.DONE if tol > 0 else KM.OPEN) and r["lo"] <= float(pts[0, 1]) <= r["hi"]
            assert tol == 0 or r["hi"] - r["lo"] <= tol
        pts, traj = KM.ON_THE_END["pts"], KM.ON_THE_END["traj"]
        c.set_input(pts)
        got = run(rig, form, c, [traj], 0.01, INF, 16, DEV_CAP, E.ALGO_AUTO)
        same(got, KM.clearances(pts, *KM.pack([traj]), 0.01, INF, 16, DEV_CAP), f"{form} a row on the end")
        assert got[0]["hi"][0] == 0.0 and got[0]["lo"][0] == 0.0 and got[0]["at_u"][0] == 1.0
        pts, trajs = KM.ORDER_ZERO["pts"], KM.ORDER_ZERO["trajs"]
        c.set_input(pts)
        for tol, status in ((0.01, KM.DONE), (0.0, KM.OPEN)):
            got = run(rig, form, c, trajs, tol, INF, 16, DEV_CAP, E.ALGO_AUTO)
            same(got, KM.clearances(pts, *KM.pack(trajs), tol, INF, 16, DEV_CAP), f"{form} order 0 tol {tol}")
            assert list(got[0]["hi"][:2]) == [0.25, 5.0] and np.all(got[0]["status"][:2] == status) and np.all(got[0]["pieces"][:2] == 1)
    finally:
        c.close()


def test_python_binding_and_the_host_form_behind_an_append(E, rig):
    """Cloud.bezier_clearance / bezier_clearance_device, and the host form on a rolling map finishing an append in flight first"""
    import torch
    pts, trajs = CM.scene()
    c = E.Cloud(512)
    try:
        c.ring_index(1.0, (10.0, 10.0, 10.0))
        c.append(pts[:150])
        c.reserve_queries(2 * DEV_CAP)
        run(rig, "dev", c, trajs, TOL, INF, DEPTH, DEV_CAP, E.ALGO_RING)             # the piece buffers have their size
        dev = torch.device("cuda", 0)
        batch, arr = E.pack_trajectories(trajs)
        t = {k: torch.from_numpy(v).to(dev) for k, v in arr.items() if v is not None}
        dbatch = E.BezierBatch(t["polycoef"].data_ptr(), batch.row_stride, t["seg_time"].data_ptr(), t["orders"].data_ptr(), t["seg_offsets"].data_ptr(),
                               None, int(batch.B))
        tc = torch.zeros((int(batch.B) * 48,), dtype=torch.uint8, device=dev)
        ts = torch.zeros((3,), dtype=torch.int64, device=dev)
        torch.cuda.synchronize()
        s = rig.side_stream()
        c.append(pts[150:])                                                           # returns once its launches are queued
        c.bezier_clearance_device(dbatch, TOL, INF, DEPTH, DEV_CAP, tc.data_ptr(), ts.data_ptr(), s.cuda_stream, E.ALGO_RING)
        s.synchronize()
        want = model(pts, "plain", trajs, TOL, INF, DEPTH, DEV_CAP)
        same((tc.cpu().numpy().view(KM.CLR_DTYPE), ts.cpu().numpy()), want, "device form behind an append")
        c.append(pts[:50])
        win = np.concatenate([pts, pts[:50]])
        got = c.bezier_clearance(trajs, TOL, max_depth=DEPTH, piece_cap=DEV_CAP, algo=E.ALGO_RING)
        wc, ws = KM.clearances(win, *KM.pack(trajs), TOL, INF, DEPTH, DEV_CAP)
        assert got[0].dtype == E.CLEARANCE_DTYPE and got[0].tobytes() == wc.tobytes()
        assert [got[1]["rounds"], got[1]["pieces"], got[1]["capped"]] == list(ws)
    finally:
        c.close()


@pytest.mark.parametrize("kind", ("grid", "ring"))
def test_device_form_captured_in_a_graph(E, rig, kind):
    """the device form captured once on a side stream and replayed three times: the model's bytes every time.  Under capture the
    streaming path is refused (PCT_ERR_INVALID, nothing queued), as for the certified check."""
    import torch
    c, rows, algos = rig.cloud(kind)
    trajs = CM.scene()[1]
    want = model(rows, kind, trajs, TOL, INF, DEPTH, DEV_CAP)
    dev = torch.device("cuda", 0)
    batch, arr = E.pack_trajectories(trajs)
    t = {k: torch.from_numpy(v).to(dev) for k, v in arr.items() if v is not None}
    dbatch = E.BezierBatch(t["polycoef"].data_ptr(), batch.row_stride, t["seg_time"].data_ptr(), t["orders"].data_ptr(), t["seg_offsets"].data_ptr(),
                           None, int(batch.B))
    tc = torch.zeros((int(batch.B) * 48,), dtype=torch.uint8, device=dev)
    ts = torch.zeros((3,), dtype=torch.int64, device=dev)
    c.reserve_queries(2 * DEV_CAP)
    s = rig.side_stream()
    args = (c.handle, C.byref(dbatch), float(TOL), INF, DEPTH, DEV_CAP, tc.data_ptr(), ts.data_ptr(), s.cuda_stream)
    lib = E.lib()
    assert lib.pct_bezier_clearance_batch_dev(args[0], algos[1], *args[1:]) == 0              # the piece buffers have their size
    s.synchronize()
    c.set_timing(0)                                                                            # no event records inside the capture
    try:
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            refused = lib.pct_bezier_clearance_batch_dev(args[0], E.ALGO_STREAM, *args[1:])
            st = lib.pct_bezier_clearance_batch_dev(args[0], algos[1], *args[1:])
        assert refused == PCT_ERR_INVALID and st == 0, (refused, st, lib.pct_last_error())
        for rep in range(3):
            tc.zero_()
            ts.zero_()
            torch.cuda.synchronize()
            g.replay()
            torch.cuda.synchronize()
            same((tc.cpu().numpy().view(KM.CLR_DTYPE), ts.cpu().numpy()), want, f"{kind} replay {rep}")
        del g
    finally:
        c.set_timing(1)


@pytest.mark.parametrize("form", FORMS)
def test_refusals_write_nothing(E, rig, form):
    c, _, _ = rig.cloud("plain")
    g, _, _ = rig.cloud("grid")
    r, _, _ = rig.cloud("ring")
    trajs = CM.scene()[1][:4]
    nseg = 12
    inv = PCT_ERR_INVALID
    for tol in (-0.01, np.nan, np.inf):
        run(rig, form, c, trajs, tol, INF, DEPTH, DEV_CAP, E.ALGO_AUTO, expect=inv)
    for cap in (0.0, -1.0, np.nan, -np.inf):
        run(rig, form, c, trajs, TOL, cap, DEPTH, DEV_CAP, E.ALGO_AUTO, expect=inv)
    for depth in (-1, 21):
        run(rig, form, c, trajs, TOL, INF, depth, DEV_CAP, E.ALGO_AUTO, expect=inv)
    run(rig, form, c, trajs, TOL, INF, DEPTH, 0, E.ALGO_AUTO, expect=inv)
    run(rig, form, c, trajs, TOL, INF, DEPTH, (1 << 24) + 1, E.ALGO_AUTO, expect=inv)
    for cloud, algo in ((c, E.ALGO_GRID), (c, E.ALGO_RING), (c, E.ALGO_STREAM_EXACT), (c, 9), (r, E.ALGO_GRID), (g, E.ALGO_RING)):
        run(rig, form, cloud, trajs, TOL, INF, DEPTH, DEV_CAP, algo, expect=inv)
    lib = E.lib()
    batch, arr = E.pack_trajectories(trajs)
    rec = np.zeros(4, KM.CLR_DTYPE)
    fn = lib.pct_bezier_clearance_batch if form == "host" else lib.pct_bezier_clearance_batch_dev
    tail = () if form == "host" else (None,)
    # NULL required pointers, B < 0
    assert fn(None, 0, C.byref(batch), TOL, INF, DEPTH, DEV_CAP, rec.ctypes.data, None, *tail) == inv
    assert fn(c.handle, 0, None, TOL, INF, DEPTH, DEV_CAP, rec.ctypes.data, None, *tail) == inv
    assert fn(c.handle, 0, C.byref(batch), TOL, INF, DEPTH, DEV_CAP, None, None, *tail) == inv
    for field in ("polycoef", "seg_time", "orders", "seg_offsets"):
        b2, _ = E.pack_trajectories(trajs)
        b2.polycoef, b2.seg_time, b2.orders, b2.seg_offsets = batch.polycoef, batch.seg_time, batch.orders, batch.seg_offsets
        setattr(b2, field, None)
        assert fn(c.handle, 0, C.byref(b2), TOL, INF, DEPTH, DEV_CAP, rec.ctypes.data, None, *tail) == inv, field
    b2, _ = E.pack_trajectories(trajs)
    b2.polycoef, b2.seg_time, b2.orders, b2.seg_offsets, b2.B = batch.polycoef, batch.seg_time, batch.orders, batch.seg_offsets, -1
    assert fn(c.handle, 0, C.byref(b2), TOL, INF, DEPTH, DEV_CAP, rec.ctypes.data, None, *tail) == inv
    if form == "host":
        # piece_cap below the number of segments, and the batched check's own refusals
        run(rig, form, c, trajs, TOL, INF, DEPTH, nseg - 1, E.ALGO_AUTO, expect=inv)
        for what in ("offset0", "descending", "order", "stride"):
            batch, arr = E.pack_trajectories(trajs)
            if what == "offset0":
                arr["seg_offsets"][0] = 1
            elif what == "descending":
                arr["seg_offsets"][2] = arr["seg_offsets"][1]
            elif what == "order":
                arr["orders"][5] = 13
            else:
                batch.row_stride = 3 * int(arr["orders"].max())
            run(rig, form, c, None, TOL, INF, DEPTH, DEV_CAP, E.ALGO_AUTO, expect=inv, packed=(batch, arr))
    else:
        # the reserved size is too small for 2 * piece_cap
        fresh = E.Cloud(64)
        try:
            fresh.set_input(CM.scene()[0][:64])
            fresh.reserve_queries(256)
            import torch
            tc = torch.full((4 * 48,), SENTINEL, dtype=torch.uint8, device="cuda")
            # (the batch's pointers are never dereferenced by a refused call)
            assert fn(fresh.handle, 0, C.byref(batch), TOL, INF, DEPTH, 4096, tc.data_ptr(), None, None) == inv
            assert bool((tc == SENTINEL).all())
        finally:
            fresh.close()


def test_device_form_without_sight_of_the_data(E, rig):
    """what only the device form can meet: more segments than piece_cap (nothing examined, OPEN, capped), and a trajectory with an order
    outside 0..12 (INVALID, the others unaffected)"""
    c, rows, _ = rig.cloud("plain")
    trajs = CM.scene()[1][:6]
    rec, stats = run(rig, "dev", c, trajs, TOL, INF, DEPTH, 17, E.ALGO_AUTO)
    assert np.all(rec["status"] == KM.OPEN) and np.all(rec["pieces"] == 0) and list(stats) == [0, 0, 1]
    assert np.all(rec["lo"] == np.inf) and np.all(rec["hi"] == np.inf) and np.all(rec["at_seg"] == -1)
    batch, arr = E.pack_trajectories(trajs)
    arr["orders"][4] = 13
    rec, stats = run(rig, "dev", c, None, TOL, INF, DEPTH, DEV_CAP, E.ALGO_AUTO, packed=(batch, arr))
    want = KM.clearances(rows, *KM.pack(trajs[:1] + trajs[2:]), TOL, INF, DEPTH, DEV_CAP)
    assert rec["status"][1] == KM.INVALID and rec["pieces"][1] == 0 and np.isnan(rec["lo"][1]) and np.isnan(rec["hi"][1])
    others = np.delete(rec, 1)
    wc = want[0].copy()
    wc["at_seg"] = np.where(wc["at_seg"] >= 3, wc["at_seg"] + 3, wc["at_seg"])           # segment numbers count the invalid trajectory's
    assert others.tobytes() == wc.tobytes() and np.array_equal(stats, want[1])


def test_cxx_client_bezier_clearance():
    """examples/bezier_clearance.cpp: ObstacleMap::trajectoryClearances and trajectoryClearance on the 4 mm line, a rolling map and an
    empty map; the line's hi is the model's to the last bit"""
    import subprocess
    from pointcloudtraj_amd import build
    build.build_all()
    exe = os.path.join(build.LIB, "bezier_clearance")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "3 maps" in r.stdout and " 0 checks failed" in r.stdout, r.stdout
    want = KM.clearances(KM.FOUR_MM["pts"], *KM.pack([KM.FOUR_MM["traj"]]), 0.001, INF, 16, 4096)[0][0]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("4 mm line:")][0].split()
    hi = float.fromhex(line[line.index("hi") + 1])
    assert hi == want["hi"] and float(line[line.index("lo") + 1]) == want["lo"] and abs(hi - 0.004) <= 0.001
    assert int(line[line.index("depth") + 1]) == want["depth"] and int(line[line.index("pieces") + 1]) == want["pieces"]
