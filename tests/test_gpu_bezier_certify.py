"""GPU tests of the certified Bezier check (pct_bezier_certify_batch, pct_bezier_certify_batch_dev; include/pct_engine.h, paragraph
"Certified Bezier check") against the numpy restatement in tests/helpers/bezier_certify_model.py.

Everything is compared byte for byte: the 48-byte certificates and the three stats.  Clouds: an un-indexed (plain), a cell-indexed
(grid), a wrapped rolling map with removed rows (ring) and an empty cloud; forms: the host form and the device form (torch buffers, a
side stream); paths: every algo the cloud admits.  The scene is the soundness scene of the model's own test (300 points, 64
trajectories of three segments, orders 0..12)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import bezier_certify_model as CM  # noqa: E402

pytestmark = pytest.mark.gpu

PCT_ERR_INVALID = 2
KINDS = ("plain", "grid", "ring", "empty")
FORMS = ("host", "dev")
DEV_CAP = 1024                         # piece_cap of the device-form runs: ample for every case here (asserted from the model's rounds)
SENTINEL = 0x5A


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


def run(rig, form, c, trajs, margin, max_depth, piece_cap, algo, expect=0, want_stats=True, packed=None):
    """one call of either form into sentinel-filled buffers with one certificate more than asked for; returns (certificates, stats)
    after asserting that nothing behind them was written -- or, on a refusal (status asserted == expect), that nothing was written"""
    E = rig.E
    batch, arr = packed if packed is not None else E.pack_trajectories(trajs)
    B = int(batch.B)
    if form == "host":
        cert = np.full((max(B, 0) + 1) * 48, SENTINEL, np.uint8)
        stats = np.full(4, -77, np.int64)
        st = E.lib().pct_bezier_certify_batch(c.handle, algo, C.byref(batch), float(margin), int(max_depth), int(piece_cap), cert.ctypes.data,
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
        st = E.lib().pct_bezier_certify_batch_dev(c.handle, algo, C.byref(dbatch), float(margin), int(max_depth), int(piece_cap), tc.data_ptr(),
                                                  ts.data_ptr() if want_stats else None, s.cuda_stream)
        s.synchronize()
        cert, stats = tc.cpu().numpy(), ts.cpu().numpy()
        del t
    assert st == expect, (st, E.lib().pct_last_error())
    if st != 0:
        assert np.all(cert == SENTINEL) and np.all(stats == -77), "a refused call wrote something"
        return None, None
    assert np.all(cert[48 * B:] == SENTINEL) and stats[3] == -77, "entries behind the certificates or the stats were written"
    if not want_stats:
        assert np.all(stats == -77)
    return cert[:48 * B].view(CM.CERT_DTYPE), stats[:3]


def same(got, want, tag):
    gc, gs = got
    wc, ws = want
    print(f"{tag}: statuses {np.bincount(gc['status'], minlength=4)} (model {np.bincount(wc['status'], minlength=4)}), stats {gs} (model {ws})")
    for name in CM.CERT_DTYPE.names:
        assert np.array_equal(gc[name], wc[name], equal_nan=gc[name].dtype.kind == "f"), f"{tag}: {name}"
    assert gc.tobytes() == wc.tobytes(), f"{tag}: certificate bytes"
    assert np.array_equal(gs, ws), f"{tag}: stats"


_model_cache = {}


def model(kind_rows, key, trajs, margin, max_depth, piece_cap, index_base=0):
    k = (key, len(trajs), float(margin), max_depth, piece_cap, index_base)
    if k not in _model_cache:
        _model_cache[k] = CM.certify(kind_rows, *CM.pack(trajs), margin, max_depth, piece_cap, index_base)
    return _model_cache[k]


# ---- 1. the scene: every cloud, both forms, every path ----------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("kind", KINDS)
def test_scene_byte_for_byte(E, rig, kind, form):
    c, rows, algos = rig.cloud(kind)
    trajs = CM.scene()[1]
    cap = DEV_CAP if form == "dev" else 1 << 16
    want = model(rows, kind, trajs, CM.MARGIN, 12, cap)
    assert want[1][2] == 0
    if kind == "empty":
        assert np.all(want[0]["status"] == CM.FREE) and np.all(want[0]["depth"] == 0) and want[1][0] == 1 and want[1][1] == 192
    else:
        counts = np.bincount(want[0]["status"], minlength=4)
        assert counts[CM.FREE] >= 8 and counts[CM.HIT] >= 8, counts
    for algo in algos:
        same(run(rig, form, c, trajs, CM.MARGIN, 12, cap, algo), want, f"{kind} {form} algo {algo}")


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("max_depth", (0, 1, 12))
def test_depth_caps(E, rig, form, max_depth):
    trajs = CM.scene()[1]
    for kind in ("grid", "ring"):
        c, rows, algos = rig.cloud(kind)
        want = model(rows, kind, trajs, CM.MARGIN, max_depth, DEV_CAP)
        if max_depth < 12:
            assert np.any(want[0]["status"] == CM.UNDECIDED)
        assert want[0]["depth"].max() <= max_depth
        same(run(rig, form, c, trajs, CM.MARGIN, max_depth, DEV_CAP, algos[1]), want, f"{kind} {form} depth cap {max_depth}")


def busiest(n=4):
    """the n trajectories of the scene that need the most pieces"""
    cert, _ = CM.scene_certificates()
    order = np.argsort(-cert["pieces"], kind="stable")[:n]
    trajs = CM.scene()[1]
    return [trajs[i] for i in sorted(order)]


@pytest.mark.parametrize("form", FORMS)
def test_piece_cap_rule(E, rig, form):
    """piece_cap equal to the segment count, one more, and ample: the first refuses a round's splits (capped, owners UNDECIDED)"""
    trajs = busiest()
    nseg = sum(len(t) for _, t, _ in trajs)
    c, rows, _ = rig.cloud("grid")
    flags = []
    for cap in (nseg, nseg + 1, DEV_CAP):
        want = model(rows, "grid", trajs, CM.MARGIN, 12, cap)
        flags.append(int(want[1][2]))
        same(run(rig, form, c, trajs, CM.MARGIN, 12, cap, E.ALGO_GRID), want, f"{form} piece_cap {cap}")
    assert flags[0] == 1 and flags[2] == 0, flags


def tile_case(n_near):
    """one cloud point at the origin, margin 0.25; n_near lines 2 m long pass 0.1 m beside it (blocked at depth 0, their ends 1 m away,
    HIT at their midpoint in round 1) and every third segment in between passes 5 m away (unblocked), spread over five trajectories:
    exactly n_near pieces split in round 0"""
    pts = np.zeros((1, 3), np.float32)
    rows = []
    near = 0
    while near < n_near:
        if len(rows) % 3 == 2:
            y = 5.0
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
    want = CM.certify(pts, *CM.pack(trajs), 0.25, 3, DEV_CAP)
    assert want[1][0] == 2 and want[1][1] == sum(len(t) for _, t, _ in trajs) + 2 * n_near and np.all(want[0]["status"] == CM.HIT)
    c = E.Cloud(16)
    c.set_input(pts)
    try:
        same(run(rig, form, c, trajs, 0.25, 3, DEV_CAP, E.ALGO_STREAM), want, f"{form} {n_near} splitting pieces")
    finally:
        c.close()


@pytest.mark.parametrize("form", FORMS)
def test_small_batches_index_base_and_an_invalid_trajectory(E, rig, form):
    c, rows, _ = rig.cloud("plain")
    trajs = CM.scene()[1]
    hits = np.nonzero(CM.scene_certificates()[0]["status"] == CM.HIT)[0]
    hit = int(hits[hits >= 1][0])
    # B = 0: PCT_OK, zero stats, no certificate
    got = run(rig, form, c, [], CM.MARGIN, 12, DEV_CAP, E.ALGO_AUTO)
    assert len(got[0]) == 0 and np.all(got[1] == 0)
    run(rig, form, c, [], CM.MARGIN, 12, DEV_CAP, E.ALGO_AUTO, want_stats=False)
    # B = 1, with and without stats
    want = model(rows, "plain", trajs[hit:hit + 1], CM.MARGIN, 12, DEV_CAP)
    assert want[0]["status"][0] == CM.HIT
    same(run(rig, form, c, trajs[hit:hit + 1], CM.MARGIN, 12, DEV_CAP, E.ALGO_AUTO), want, f"{form} B = 1")
    got = run(rig, form, c, trajs[hit:hit + 1], CM.MARGIN, 12, DEV_CAP, E.ALGO_AUTO, want_stats=False)
    assert got[0].tobytes() == want[0].tobytes()
    # INVALID trajectories between valid ones: seg_time 0, negative, NaN, +inf, and a control point beyond FLT_MAX
    mixed = list(trajs[hit - 1:hit + 2]) + [trajs[30]]
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
    want = CM.certify(rows, *CM.pack(mixed), CM.MARGIN, 12, DEV_CAP)
    assert list(np.nonzero(want[0]["status"] == CM.INVALID)[0]) == [1, 3, 5, 7, 8] and want[0]["status"][2] == CM.HIT
    same(run(rig, form, c, mixed, CM.MARGIN, 12, DEV_CAP, E.ALGO_STREAM), want, f"{form} INVALID between valid ones")
    # the index base is added to the reported index
    base = E.Cloud(len(rows))
    try:
        base.set_index_base(1000)
        base.set_input(rows)
        want = CM.certify(rows, *CM.pack(trajs[hit:hit + 2]), CM.MARGIN, 12, DEV_CAP, index_base=1000)
        assert want[0]["hit_idx"][0] >= 1000
        same(run(rig, form, base, trajs[hit:hit + 2], CM.MARGIN, 12, DEV_CAP, E.ALGO_AUTO), want, f"{form} index base")
    finally:
        base.close()


def test_device_form_behind_an_asynchronous_append(E, rig):
    """the device form on a side stream right behind an append on the library's stream sees the appended frame"""
    pts, trajs = CM.scene()
    c = E.Cloud(512)
    try:
        c.ring_index(1.0, (10.0, 10.0, 10.0))
        c.append(pts[:150])
        c.reserve_queries(2 * DEV_CAP)
        run(rig, "dev", c, trajs, CM.MARGIN, 12, DEV_CAP, E.ALGO_RING)          # the piece buffers have their size
        import torch
        dev = torch.device("cuda", 0)
        batch, arr = E.pack_trajectories(trajs)
        t = {k: torch.from_numpy(v).to(dev) for k, v in arr.items() if v is not None}
        dbatch = E.BezierBatch(t["polycoef"].data_ptr(), batch.row_stride, t["seg_time"].data_ptr(), t["orders"].data_ptr(), t["seg_offsets"].data_ptr(),
                               None, int(batch.B))
        tc = torch.zeros((int(batch.B) * 48,), dtype=torch.uint8, device=dev)
        ts = torch.zeros((3,), dtype=torch.int64, device=dev)
        torch.cuda.synchronize()
        s = rig.side_stream()
        c.append(pts[150:])                                                        # returns once its launches are queued
        c.bezier_certify_device(dbatch, CM.MARGIN, 12, DEV_CAP, tc.data_ptr(), ts.data_ptr(), s.cuda_stream, E.ALGO_RING)
        s.synchronize()
        want = model(pts, "plain", trajs, CM.MARGIN, 12, DEV_CAP)
        same((tc.cpu().numpy().view(CM.CERT_DTYPE), ts.cpu().numpy()), want, "device form behind an append")
        # the host form finishes an append in flight first
        c.append(pts[:50])
        win = np.concatenate([pts, pts[:50]])
        got = c.bezier_certify(trajs, CM.MARGIN, 12, DEV_CAP, E.ALGO_RING)
        wc, ws = CM.certify(win, *CM.pack(trajs), CM.MARGIN, 12, DEV_CAP)
        assert got[0].tobytes() == wc.tobytes() and [got[1]["rounds"], got[1]["pieces"], got[1]["capped"]] == list(ws)
    finally:
        c.close()


@pytest.mark.parametrize("kind", ("grid", "ring"))
def test_device_form_captured_in_a_graph(E, rig, kind):
    """the device form captured once on a side stream and replayed three times: the model's bytes every time.  Under capture the
    streaming path is refused (PCT_ERR_INVALID, nothing queued): only the two index paths are served there."""
    import torch
    c, rows, algos = rig.cloud(kind)
    trajs = CM.scene()[1]
    want = model(rows, kind, trajs, CM.MARGIN, 12, DEV_CAP)
    dev = torch.device("cuda", 0)
    batch, arr = E.pack_trajectories(trajs)
    t = {k: torch.from_numpy(v).to(dev) for k, v in arr.items() if v is not None}
    dbatch = E.BezierBatch(t["polycoef"].data_ptr(), batch.row_stride, t["seg_time"].data_ptr(), t["orders"].data_ptr(), t["seg_offsets"].data_ptr(),
                           None, int(batch.B))
    tc = torch.zeros((int(batch.B) * 48,), dtype=torch.uint8, device=dev)
    ts = torch.zeros((3,), dtype=torch.int64, device=dev)
    c.reserve_queries(2 * DEV_CAP)
    s = rig.side_stream()
    args = (c.handle, C.byref(dbatch), float(CM.MARGIN), 12, DEV_CAP, tc.data_ptr(), ts.data_ptr(), s.cuda_stream)
    lib = E.lib()
    assert lib.pct_bezier_certify_batch_dev(args[0], algos[1], *args[1:]) == 0              # the piece buffers have their size
    s.synchronize()
    c.set_timing(0)                                                                          # no event records inside the capture
    try:
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            refused = lib.pct_bezier_certify_batch_dev(args[0], E.ALGO_STREAM, *args[1:])
            st = lib.pct_bezier_certify_batch_dev(args[0], algos[1], *args[1:])
        assert refused == PCT_ERR_INVALID and st == 0, (refused, st, lib.pct_last_error())
        for rep in range(3):
            tc.zero_()
            ts.zero_()
            torch.cuda.synchronize()
            g.replay()
            torch.cuda.synchronize()
            same((tc.cpu().numpy().view(CM.CERT_DTYPE), ts.cpu().numpy()), want, f"{kind} replay {rep}")
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
    for margin in (-0.25, np.nan, np.inf):
        run(rig, form, c, trajs, margin, 12, DEV_CAP, E.ALGO_AUTO, expect=inv)
    for depth in (-1, 21):
        run(rig, form, c, trajs, CM.MARGIN, depth, DEV_CAP, E.ALGO_AUTO, expect=inv)
    run(rig, form, c, trajs, CM.MARGIN, 12, 0, E.ALGO_AUTO, expect=inv)
    run(rig, form, c, trajs, CM.MARGIN, 12, (1 << 24) + 1, E.ALGO_AUTO, expect=inv)
    for cloud, algo in ((c, E.ALGO_GRID), (c, E.ALGO_RING), (c, E.ALGO_STREAM_EXACT), (c, 9), (r, E.ALGO_GRID), (g, E.ALGO_RING)):
        run(rig, form, cloud, trajs, CM.MARGIN, 12, DEV_CAP, algo, expect=inv)
    lib = E.lib()
    batch, arr = E.pack_trajectories(trajs)
    cert = np.zeros(4, CM.CERT_DTYPE)
    fn = lib.pct_bezier_certify_batch if form == "host" else lib.pct_bezier_certify_batch_dev
    tail = () if form == "host" else (None,)
    # NULL required pointers, B < 0
    assert fn(None, 0, C.byref(batch), 0.25, 12, DEV_CAP, cert.ctypes.data, None, *tail) == inv
    assert fn(c.handle, 0, None, 0.25, 12, DEV_CAP, cert.ctypes.data, None, *tail) == inv
    assert fn(c.handle, 0, C.byref(batch), 0.25, 12, DEV_CAP, None, None, *tail) == inv
    for field in ("polycoef", "seg_time", "orders", "seg_offsets"):
        b2, _ = E.pack_trajectories(trajs)
        b2.polycoef, b2.seg_time, b2.orders, b2.seg_offsets = batch.polycoef, batch.seg_time, batch.orders, batch.seg_offsets
        setattr(b2, field, None)
        assert fn(c.handle, 0, C.byref(b2), 0.25, 12, DEV_CAP, cert.ctypes.data, None, *tail) == inv, field
    b2, _ = E.pack_trajectories(trajs)
    b2.polycoef, b2.seg_time, b2.orders, b2.seg_offsets, b2.B = batch.polycoef, batch.seg_time, batch.orders, batch.seg_offsets, -1
    assert fn(c.handle, 0, C.byref(b2), 0.25, 12, DEV_CAP, cert.ctypes.data, None, *tail) == inv
    if form == "host":
        # piece_cap below the number of segments, and the batched check's own refusals
        run(rig, form, c, trajs, CM.MARGIN, 12, nseg - 1, E.ALGO_AUTO, expect=inv)
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
            run(rig, form, c, None, CM.MARGIN, 12, DEV_CAP, E.ALGO_AUTO, expect=inv, packed=(batch, arr))
    else:
        # the reserved size is too small for 2 * piece_cap
        fresh = E.Cloud(64)
        try:
            fresh.set_input(CM.scene()[0][:64])
            fresh.reserve_queries(256)
            import torch
            tc = torch.full((4 * 48,), SENTINEL, dtype=torch.uint8, device="cuda")
            # (the batch's pointers are never dereferenced by a refused call)
            assert fn(fresh.handle, 0, C.byref(batch), 0.25, 12, 4096, tc.data_ptr(), None, None) == inv
            assert bool((tc == SENTINEL).all())
        finally:
            fresh.close()


def test_device_form_without_sight_of_the_data(E, rig):
    """what only the device form can meet: more segments than piece_cap (nothing examined, UNDECIDED, capped), and a trajectory with
    an order outside 0..12 (INVALID, the others unaffected)"""
    c, rows, _ = rig.cloud("plain")
    trajs = CM.scene()[1][:6]
    cert, stats = run(rig, "dev", c, trajs, CM.MARGIN, 12, 17, E.ALGO_AUTO)
    assert np.all(cert["status"] == CM.UNDECIDED) and np.all(cert["pieces"] == 0) and list(stats) == [0, 0, 1]
    batch, arr = E.pack_trajectories(trajs)
    arr["orders"][4] = 13
    cert, stats = run(rig, "dev", c, None, CM.MARGIN, 12, DEV_CAP, E.ALGO_AUTO, packed=(batch, arr))
    want = CM.certify(rows, *CM.pack(trajs[:1] + trajs[2:]), CM.MARGIN, 12, DEV_CAP)
    assert cert["status"][1] == CM.INVALID and cert["pieces"][1] == 0
    others = np.delete(cert, 1)
    wc = want[0].copy()
    wc["hit_seg"] = np.where(wc["hit_seg"] >= 3, wc["hit_seg"] + 3, wc["hit_seg"])       # segment numbers count the invalid trajectory's
    assert others.tobytes() == wc.tobytes() and np.array_equal(stats, want[1])


def test_four_mm_line_beside_the_sampled_check(E):
    """the two verdicts side by side: the sampled check at dt = 0.02 passes the obstacle 4 mm off the line, the certified check reports it"""
    pts, traj, margin = CM.FOUR_MM["pts"], CM.FOUR_MM["traj"], CM.FOUR_MM["margin"]
    c = E.Cloud(16)
    try:
        c.set_input(pts)
        prm = E.inflate_params((0.0, 0.0, 0.0), 100.0, margin, 1.0)
        sampled = c.bezier_check_batch(prm, [traj], stop_time=10.0, dt=0.02)
        assert sampled["nsamples"][0] >= 50 and sampled["first_hit"][0] == -1
        assert sampled["min_radius"][0] > 0.0105 - margin              # every sample is at least 10.8 mm from the obstacle
        cert, stats = c.bezier_certify([traj], margin, 12, 1000)
        want = CM.certify(pts, *CM.pack([traj]), margin, 12, 1000)
        assert cert.tobytes() == want[0].tobytes()
        assert cert["status"][0] == CM.HIT and cert["depth"][0] == 7 and cert["pieces"][0] == 15 and cert["hit_u"][0] == 65 / 128
        assert stats == dict(rounds=8, pieces=15, capped=0)
    finally:
        c.close()


def test_margin_edge_on_the_card(E):
    """exactly at the margin: UNDECIDED with 2 * depth + 1 pieces; one fp32 ulp nearer: HIT; one farther: UNDECIDED, never FREE"""
    c = E.Cloud(16)
    try:
        traj, margin = CM.AT_MARGIN["traj"], CM.AT_MARGIN["margin"]
        for ulps, depth, status in ((0, 12, CM.UNDECIDED), (-1, 20, CM.HIT), (1, 20, CM.UNDECIDED)):
            pts = CM.at_margin_cloud(ulps)
            c.set_input(pts)
            cert, stats = c.bezier_certify([traj], margin, depth, 1000)
            want = CM.certify(pts, *CM.pack([traj]), margin, depth, 1000)
            assert cert.tobytes() == want[0].tobytes() and cert["status"][0] == status
            if ulps == 0:
                assert cert["pieces"][0] == 2 * depth + 1
    finally:
        c.close()


def test_cxx_client_bezier_certify():
    """examples/bezier_certify.cpp: ObstacleMap::certifyTrajectories and certifySafeTrajectory on a plain, a cell-indexed, a rolling and
    an empty map, every certificate compared with a host loop"""
    import subprocess
    from pointcloudtraj_amd import build
    build.build_all()
    exe = os.path.join(build.LIB, "bezier_certify")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 certificates differ" in r.stdout and "4 maps" in r.stdout, r.stdout
