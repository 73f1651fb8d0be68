"""GPU tests of the fused RRT* expansion step over the rolling-map index: pct_rrt_expand_batch with a ring-indexed obstacle cloud
(rrt_expand_kernel<true>, csrc/ring.hpp), called through ctypes with a small node cloud (pct_cloud_create_small +
pct_cloud_small_aux).

Reference: a numpy restatement written here (ref_expand) --
  nearest node by fp64 (dx*dx + dy*dy) + dz*dz on the float-widened operands, lowest index on ties;
  steer as include/pct_engine.h states it: centre = node + (sample - node) * (r_node / dist) when dist > r_node, fp64;
  radius from oracle.inflate_brute (exhaustive nearest neighbour) on the live window of a host mirror of the ring;
  neighbourhood = the SET of nodes with d2 <= (2 * float(radius))^2 around the fp32-narrowed centre.
Centres, radii and near_idx are compared bit for bit, ids as sorted sets."""
import ctypes as C
import functools

import numpy as np
import pytest

from pointcloudtraj_amd import scenarios as S, synth
from pointcloudtraj_amd.scenarios import RingMirror

pytestmark = pytest.mark.gpu

MARGIN, MAXR = 0.25, 1.5
CAP = 256


@pytest.fixture(scope="module")
def E():
    from pointcloudtraj_amd import engine
    engine.init(0)
    return engine


class Nodes:
    """a small (host-mapped) node cloud with its per-node planner data {x, y, z, radius}: coordinates fp64 in aux, fp32 in the cloud"""

    def __init__(self, E, aux):
        self.E = E
        self.aux = np.ascontiguousarray(aux, np.float64).reshape(-1, 4)
        self.xyz = self.aux[:, :3].astype(np.float32)                 # what the tree stores: (float)centre
        self.h = C.c_void_p()
        E._chk(E.lib().pct_cloud_create_small(max(len(self.aux), 16), C.byref(self.h)))
        p = C.POINTER(C.c_double)()
        E._chk(E.lib().pct_cloud_small_aux(self.h, C.byref(p)))
        if len(self.aux):
            E._chk(E.lib().pct_cloud_upload_aos(self.h, self.xyz.ctypes.data_as(C.c_void_p), len(self.xyz), 12))
            np.ctypeslib.as_array(p, shape=(len(self.aux), 4))[:] = self.aux

    def close(self):
        if self.h.value:
            self.E.lib().pct_cloud_destroy(self.h)
            self.h = C.c_void_p()


def expand_rc(E, nodes, cloud, prm, samples, cap=CAP):
    s = np.ascontiguousarray(samples, np.float64).reshape(-1, 3)
    K = len(s)
    out = (E.ExpandResult * max(K, 1))()
    ids = np.full(max(K, 1) * cap, 0xFFFFFFFF, np.uint32)
    rc = E.lib().pct_rrt_expand_batch(nodes.h, cloud.handle, C.byref(prm), s.ctypes.data_as(C.c_void_p), K, cap,
                                      out, ids.ctypes.data_as(C.c_void_p))
    raw = np.frombuffer(out, np.uint8).reshape(-1, 40)[:K].copy()
    rec = np.frombuffer(out, np.dtype([("c", np.float64, 3), ("r", np.float64), ("near", np.int32), ("count", np.int32)]))[:K].copy()
    return rc, rec, ids.reshape(-1, cap)[:K], raw


def expand(E, nodes, cloud, prm, samples, cap=CAP):
    rc, rec, ids, raw = expand_rc(E, nodes, cloud, prm, samples, cap)
    E._chk(rc)
    return rec, ids, raw


def d2_rows(p32, q32):
    """fp64 (dx*dx + dy*dy) + dz*dz of every float point against one float query"""
    d = p32.astype(np.float64) - q32.astype(np.float64)
    return (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]


def ref_expand(oracle, nodes, window, start, sample_range, samples):
    s = np.ascontiguousarray(samples, np.float64).reshape(-1, 3)
    K, n = len(s), len(nodes.aux)
    near = np.full(K, -1, np.int32)
    centre = s.copy()
    for k in range(K):
        if n == 0:
            continue
        d2 = d2_rows(nodes.xyz, s[k].astype(np.float32))
        i = int(np.argmin(d2))                                        # first minimum = lowest index on ties
        near[k] = i
        a, ar = nodes.aux[i, :3], nodes.aux[i, 3]
        dx, dy, dz = a[0] - s[k, 0], a[1] - s[k, 1], a[2] - s[k, 2]
        dis = np.sqrt(dx * dx + dy * dy + dz * dz)
        if dis > ar:
            t = ar / dis
            centre[k] = [a[0] + (s[k, 0] - a[0]) * t, a[1] + (s[k, 1] - a[1]) * t, a[2] + (s[k, 2] - a[2]) * t]
    if len(window):
        radius, _, _ = oracle.inflate_brute(window, start, sample_range, MARGIN, MAXR, centre)
    else:                                                             # no obstacle at all: corridor_finder.cpp:115-116
        radius = np.full(K, MAXR - MARGIN)
    sets = []
    for k in range(K):
        rf = np.maximum(np.float32(radius[k]), np.float32(0.0)) * np.float32(2.0)
        r2 = np.float64(rf) * np.float64(rf)
        sets.append(np.flatnonzero(d2_rows(nodes.xyz, centre[k].astype(np.float32)) <= r2) if n else np.zeros(0, np.int64))
    return near, centre, radius, sets


def check(got, ref, what="", cap=CAP):
    rec, ids, _ = got
    near, centre, radius, sets = ref
    assert np.array_equal(rec["near"], near), f"{what}: nearest node"
    assert np.array_equal(rec["c"].view(np.uint64), centre.view(np.uint64)), f"{what}: steered centres"
    assert np.array_equal(rec["r"].view(np.uint64), np.ascontiguousarray(radius, np.float64).view(np.uint64)), f"{what}: radii"
    for k, want in enumerate(sets):
        if len(want) <= cap:
            assert rec["count"][k] == len(want), f"{what}: sample {k}: {rec['count'][k]} neighbours, {len(want)} expected"
            assert np.array_equal(np.sort(ids[k, :len(want)].astype(np.int64)), want), f"{what}: sample {k}: neighbourhood"
        else:                                                         # truncated list: the count is still exact, negated
            assert rec["count"][k] == -len(want), f"{what}: sample {k}"
            assert np.all(np.isin(ids[k, :cap].astype(np.int64), want)), f"{what}: sample {k}"


def make_nodes(E, seed, n, lo, hi, offset=(0.0, 0.0, 0.0), radius=(0.3, 1.5), cluster=0):
    xyz = synth.uniform_rows_f64(seed, n, 3, lo, hi) + np.float64(offset)
    if cluster:                                                       # a knot of nodes: neighbourhoods of dozens
        xyz[:cluster] = xyz[0] + synth.uniform_rows_f64(seed + 1, cluster, 3, -0.5, 0.5)
    r = synth.uniform_points(seed + 2, n, radius[0], radius[1])[:, 0].astype(np.float64)      # a float radius, widened
    return Nodes(E, np.column_stack([xyz, r]))


# ---- 1. wrapped ring, every batch size ---------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def wrapped_case():
    """7 frames of 7 000 uniform points in [0, 40)^3 through 30 000 slots"""
    frames = [synth.uniform_points(90 + f, 7000, 0, 40) for f in range(7)]
    m = RingMirror(30000)
    for f in frames:
        m.append(f)
    samples = synth.uniform_rows_f64(190, 1025, 3, -2.0, 42.0)
    return frames, m.live().copy(), samples


WRAPPED_START, WRAPPED_RANGE = (20.0, 20.0, 20.0), 30.0


@pytest.fixture(scope="module")
def wrapped(E, oracle):
    frames, win, samples = wrapped_case()
    c = E.Cloud(len(win))
    c.ring_index(0.0, (40.0, 40.0, 40.0))
    for f in frames:
        c.append(f)
    assert len(c) == len(win) and c.has_ring_index and not c.has_grid
    nodes = make_nodes(E, 191, 200, 0.0, 40.0, cluster=40)
    ref = ref_expand(oracle, nodes, win, WRAPPED_START, WRAPPED_RANGE, samples[:1024])
    yield c, nodes, ref
    nodes.close()
    c.close()


@pytest.mark.parametrize("K", [1, 8, 9, 257, 1024])
def test_wrapped_ring_every_batch_size(E, wrapped, K):
    """K <= 8 waits on the completion word, above that on the stream; ids per sample shrink with K (65536 / K)"""
    c, nodes, ref = wrapped
    prm = E.inflate_params(WRAPPED_START, WRAPPED_RANGE, MARGIN, MAXR)
    samples = wrapped_case()[2]
    got = expand(E, nodes, c, prm, samples[:K])
    near, centre, radius, sets = ref
    check(got, (near[:K], centre[:K], radius[:K], sets[:K]), f"K = {K}", cap=min(CAP, 65536 // K))
    if K >= 257:                                                      # the case has radii of both signs and the knot's large neighbourhoods
        assert (got[0]["r"] < 0.0).any() and (got[0]["r"] > 0.0).any() and (got[0]["count"] > 8).any()


def test_more_samples_than_a_launch_holds(E, wrapped):
    c, nodes, _ = wrapped
    prm = E.inflate_params(WRAPPED_START, WRAPPED_RANGE, MARGIN, MAXR)
    rc, _, _, _ = expand_rc(E, nodes, c, prm, wrapped_case()[2][:1025])
    assert rc == 2, "PCT_ERR_INVALID"


def test_far_samples_stop_at_the_reach(E, oracle, wrapped):
    """centres far outside the window on a table with open axes: the search ends by stop_d2 with max_radius"""
    c, _, _ = wrapped
    win = wrapped_case()[1]
    none = Nodes(E, np.zeros((0, 4)))
    samples = np.float64([[140.0, 20.0, 20.0], [-60.0, -60.0, -60.0], [20.0, 20.0, 47.0], [41.9, 20.3, 20.1]])
    prm = E.inflate_params(WRAPPED_START, 1e6, MARGIN, MAXR)
    got = expand(E, none, c, prm, samples)
    check(got, ref_expand(oracle, none, win, WRAPPED_START, 1e6, samples), "far samples")
    assert np.all(got[0]["r"][:3] == MAXR)
    none.close()


# ---- 8. the same points behind either index kind -------------------------------------------------------------------------------------

def test_grid_and_ring_index_give_identical_bytes(E, wrapped):
    c, nodes, _ = wrapped
    win, samples = wrapped_case()[1], wrapped_case()[2][:257]
    g = E.Cloud(len(win))
    g.set_input(win)
    g.build_grid()
    prm = E.inflate_params(WRAPPED_START, WRAPPED_RANGE, MARGIN, MAXR)
    rr, ri, rraw = expand(E, nodes, c, prm, samples)
    gr, gi, graw = expand(E, nodes, g, prm, samples)
    assert np.array_equal(rraw, graw), "pct_expand_result bytes"
    for k in range(len(samples)):
        n = abs(int(rr["count"][k]))
        assert np.array_equal(np.sort(ri[k, :min(n, 255)]), np.sort(gi[k, :min(n, 255)])), k
    g.close()


# ---- 2. eviction -----------------------------------------------------------------------------------------------------------------

def test_an_evicted_point_no_longer_bounds_the_radius(E, oracle):
    cap = 1000
    c, m = E.Cloud(cap), RingMirror(cap)
    c.ring_index(1.0, (40.0, 40.0, 40.0))
    nodes = Nodes(E, np.float64([[10.0, 10.0, 10.0, 1.0]]))
    sample = np.float64([[13.0, 10.0, 10.0]])                          # steered to (11, 10, 10)
    prm = E.inflate_params((10.0, 10.0, 10.0), 30.0, MARGIN, MAXR)
    frame = (synth.uniform_points(201, 400, 0.0, 5.0) + np.float32([25.0, 25.0, 25.0])).astype(np.float32)
    frame[123] = np.float32([11.3, 10.0, 10.0])
    c.append(frame); m.append(frame)
    got = expand(E, nodes, c, prm, sample)
    check(got, ref_expand(oracle, nodes, m.live(), (10.0, 10.0, 10.0), 30.0, sample), "point present")
    assert np.array_equal(got[0]["c"][0], [11.0, 10.0, 10.0]) and 0.0 < got[0]["r"][0] < 0.06
    for k in range(3):                                                # 1200 more points: slot 123 is overwritten in the second
        far = (synth.uniform_points(202 + k, 400, 0.0, 5.0) + np.float32([25.0, 25.0, 25.0])).astype(np.float32)
        c.append(far); m.append(far)
    got = expand(E, nodes, c, prm, sample)
    check(got, ref_expand(oracle, nodes, m.live(), (10.0, 10.0, 10.0), 30.0, sample), "point evicted")
    assert got[0]["r"][0] == MAXR
    nodes.close(); c.close()


# ---- 3. small table: folded buckets, closed axes ---------------------------------------------------------------------------------------

def test_small_table_folding_closed_axes_and_absurd_samples(E, oracle):
    cap = 4000
    c, m = E.Cloud(cap), RingMirror(cap)
    c.ring_index(2.0, (8.0, 8.0, 8.0))
    assert all(d <= 8 for d in c.ring_info()["dims"]), c.ring_info()
    none = Nodes(E, np.zeros((0, 4)))
    for f in range(9):
        drift = np.float64([17.0 * f, -3.0 * f, 0.5 * f])
        pts = (synth.uniform_points(120, 1000, 0.0, 10.0, offset=f * 1000) + np.float32(drift)).astype(np.float32)
        c.append(pts); m.append(pts)
        if f not in (2, 5, 8):
            continue
        samples = np.concatenate([synth.uniform_rows_f64(220 + f, 150, 3, -1.0, 11.0) + drift,
                                  synth.uniform_rows_f64(230 + f, 30, 3, -300.0, 300.0) + drift,
                                  np.float64([[1e30, 0, 0], [0, -1e30, 0], [1e30, 1e30, 1e30], [-1e30, 5.0, -1e30], [3.0, 3.0, 1e30], [-1e30, -1e30, -1e30]])])
        nodes = make_nodes(E, 240 + f, 50, 0.0, 10.0, offset=drift)
        start = tuple(drift + 5.0)
        for rng in (1e31, 20.0):                                      # every centre searched; the early-out for the far ones
            prm = E.inflate_params(start, rng, MARGIN, MAXR)
            for nd, tag in ((none, "centre = sample"), (nodes, "steered")):
                got = expand(E, nd, c, prm, samples)
                check(got, ref_expand(oracle, nd, m.live(), start, rng, samples), f"frame {f}, range {rng}, {tag}")
                if nd is none and rng == 1e31:
                    assert np.all(got[0]["r"][-6:] == MAXR) and (got[0]["r"][:150] < MAXR).any()
        nodes.close()
    none.close(); c.close()


# ---- 4. overflow queue ---------------------------------------------------------------------------------------------------------------

def test_overflow_queue_holds_the_nearest_points(E, oracle):
    cap = 60_000
    c, m = E.Cloud(cap), RingMirror(cap)
    c.ring_index(0.5, (20.0, 20.0, 20.0))
    base = synth.uniform_points(51, 20_000, 0.0, 20.0)
    none = Nodes(E, np.zeros((0, 4)))
    nodes = make_nodes(E, 250, 40, 4.0, 8.0, radius=(0.3, 0.8))
    samples = np.concatenate([np.float64([[5, 5, 5], [5.01, 5, 5], [5.3, 5.2, 4.9], [7.004, 7.004, 7.004], [7.4, 7.0, 7.0], [6.0, 6.0, 6.0]]),
                              synth.uniform_rows_f64(251, 58, 3, 4.0, 8.0)])
    prm = E.inflate_params((6.0, 6.0, 6.0), 30.0, MARGIN, MAXR)
    for f in range(7):
        pts = base.copy() if f % 2 == 0 else synth.uniform_points(52 + f, 20_000, 0.0, 20.0)
        pts[:3000] = np.float32([5.0, 5.0, 5.0])
        pts[3000:6000] = (np.float32([7.0, 7.0, 7.0]) + synth.uniform_points(60 + f, 3000, 0.0, 0.01)).astype(np.float32)
        c.append(pts); m.append(pts)
        if f not in (3, 6):                                           # the ring is full from frame 2 on: queued records have been evicted
            continue
        assert c.ring_info()["overflow_entries"] > 0
        for nd, tag in ((none, "centre = sample"), (nodes, "steered")):
            got = expand(E, nd, c, prm, samples)
            check(got, ref_expand(oracle, nd, m.live(), (6.0, 6.0, 6.0), 30.0, samples), f"frame {f}, {tag}")
        assert got[0]["r"].min() < 0.0
    none.close(); nodes.close(); c.close()


# ---- 5. grown buckets ----------------------------------------------------------------------------------------------------------------

def test_grown_buckets(E, oracle):
    window, frame = 120_000, 4_000
    c, m = E.Cloud(window), RingMirror(window)
    c.ring_index()
    nframes = window // frame + 12
    for f in range(nframes):
        pts = S.c5_frame_clustered(f, frame)
        c.append(pts); m.append(pts)
    assert c.ring_info()["bucket_records"] > 32, c.ring_info()
    x0 = 0.1 * nframes
    samples = np.column_stack([np.linspace(x0 - 25.0, x0 + 25.0, 64) + 1e-7, synth.uniform_rows_f64(260, 64, 1, -6.0, 6.0)[:, 0], np.full(64, 2.5)])
    nodes = make_nodes(E, 261, 30, -3.0, 3.0, offset=(x0, 0.0, 2.5))
    none = Nodes(E, np.zeros((0, 4)))
    start = (x0, 0.0, 2.5)
    prm = E.inflate_params(start, 30.0, MARGIN, MAXR)
    for nd, tag in ((none, "centre = sample"), (nodes, "steered")):
        got = expand(E, nd, c, prm, samples)
        check(got, ref_expand(oracle, nd, m.live(), start, 30.0, samples), tag)
    none.close(); nodes.close(); c.close()


# ---- 6. empty windows, one point, early-out, no nodes -----------------------------------------------------------------------------------

@pytest.mark.parametrize("extent", [None, (10.0, 10.0, 10.0)], ids=["table not sized yet", "empty table"])
def test_empty_window_is_an_empty_cloud(E, oracle, extent):
    c = E.Cloud(500)
    c.ring_index(0.0, extent)
    assert c.has_ring_index == (extent is not None) and len(c) == 0
    nodes = make_nodes(E, 270, 20, 0.0, 10.0)
    samples = np.concatenate([synth.uniform_rows_f64(271, 12, 3, -2.0, 12.0), np.float64([[500.0, 0.0, 0.0]])])
    prm = E.inflate_params((5.0, 5.0, 5.0), 30.0, MARGIN, MAXR)
    for K in (3, len(samples)):
        got = expand(E, nodes, c, prm, samples[:K])
        assert np.all(got[0]["r"] == MAXR - MARGIN)
        check(got, ref_expand(oracle, nodes, np.zeros((0, 3), np.float32), (5.0, 5.0, 5.0), 30.0, samples[:K]), f"K = {K}")
    # a window of one point
    one = np.float32([[4.0, 5.0, 6.0]])
    c.append(one)
    assert c.has_ring_index and len(c) == 1
    got = expand(E, nodes, c, prm, samples)
    check(got, ref_expand(oracle, nodes, one, (5.0, 5.0, 5.0), 30.0, samples), "one point")
    nodes.close(); c.close()


def test_early_out_and_empty_node_set(E, oracle, wrapped):
    c, nodes, _ = wrapped
    win = wrapped_case()[1]
    samples = np.concatenate([wrapped_case()[2][:20], np.float64([[20.0, 20.0, 20.0 + 5.0 + MAXR + 1e-9], [20.0, 20.0, 20.0 + 5.0 + MAXR - 1e-9]])])
    prm = E.inflate_params(WRAPPED_START, 5.0, MARGIN, MAXR)           # most centres lie beyond sample_range + max_radius
    none = Nodes(E, np.zeros((0, 4)))
    for nd, tag in ((nodes, "steered"), (none, "no nodes")):
        got = expand(E, nd, c, prm, samples)
        check(got, ref_expand(oracle, nd, win, WRAPPED_START, 5.0, samples), tag)
    rec = got[0]
    assert np.all(rec["near"] == -1) and np.all(rec["count"] == 0)
    assert np.array_equal(rec["c"].view(np.uint64), samples.view(np.uint64)), "no node: the centre is the sample"
    assert rec["r"][-2] == MAXR - MARGIN and (rec["r"] != MAXR - MARGIN).any()
    none.close()


# ---- 7. append, then ask at once -----------------------------------------------------------------------------------------------------

def test_the_answer_sees_a_frame_appended_just_before(E, oracle):
    """pct_cloud_append_aos returns with its insert kernel queued; pct_rrt_expand_batch right behind it, no synchronisation in
    between, answers from the window that holds the frame -- with the stream wait (K = 64) and with the completion word of the
    NODE cloud (K = 4)"""
    cap = 50_000
    c, m = E.Cloud(cap), RingMirror(cap)
    c.ring_index(0.0, (40.0, 40.0, 40.0))
    nodes = make_nodes(E, 280, 60, 0.0, 40.0, radius=(80.0, 90.0))     # every sample lies inside its nearest sphere: centre = sample
    samples = synth.uniform_rows_f64(281, 64, 3, 0.0, 40.0)
    start = (20.0, 20.0, 20.0)
    prm = E.inflate_params(start, 40.0, MARGIN, MAXR)
    last = None
    for f in range(5):
        pts = synth.uniform_points(282 + f, 20_000, 0.0, 40.0)
        pts[:64] = (samples + (0.2 - 0.03 * f)).astype(np.float32)      # each frame brings nearer points than any before
        for frame, K in ((pts, 64), (pts[:1000] - np.float32(0.02), 4)):
            c.append(frame)
            got = expand(E, nodes, c, prm, samples[:K])
            m.append(frame)
            check(got, ref_expand(oracle, nodes, m.live(), start, 40.0, samples[:K]), f"frame {f}, K = {K}")
            assert last is None or (np.all(got[0]["r"][:4] <= last) and np.any(got[0]["r"][:4] < last)), "the new frame's points must have been seen"
            last = got[0]["r"][:4].copy()
    nodes.close(); c.close()


def test_a_cloud_with_no_index_is_still_refused(E):
    c = E.Cloud(100)
    c.set_input(synth.uniform_points(290, 100, 0.0, 10.0))
    nodes = make_nodes(E, 291, 5, 0.0, 10.0)
    prm = E.inflate_params((5.0, 5.0, 5.0), 30.0, MARGIN, MAXR)
    rc, _, _, _ = expand_rc(E, nodes, c, prm, np.float64([[1.0, 2.0, 3.0]]))
    assert rc == 2 and b"staged" in E.lib().pct_last_error()
    nodes.close(); c.close()
