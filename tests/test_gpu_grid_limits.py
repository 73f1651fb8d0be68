"""The cell index (pct_cloud_build_grid) at its caps: 1024 cells on an axis, a grid of 2^30 cells, the cell-size floor max_ext / 1023 --
and with the 2^30-cell grid the 64-bit form of the dense NN batch kernel (nn_grid_coop_kernel<., NARROW = false, .>), which the host
launches when narrow_offsets_fit says no: here because the table holds 2^30 + 1 run bounds.

A. The cube: a cloud with bounding box [0, 1023]^3 built with cell_size 1.0 has dims (1024, 1024, 1024).  22 089 points: the pins
   (0, 0, 0) and (1023, 1023, 1023) and two clusters of 6 points per cell, [0, 12)^3 and [1010, 1022.5)^3, so that every query's walk is
   local and the far pin is the only point of the last cell -- whose run ends at cell_start[2^30], the one entry whose byte offset does
   not fit 32 bits.  Built with PCT_PYRAMID=0: left alone the build would give a grid this empty the pyramid, about 1.2e9 nodes (39 GB;
   DESIGN.md, left out).  The table is 4 GiB, and the build holds 4 GiB of counters more while it runs.  NN batches of 1, 700, 5000 and
   20 000 queries (single query, express batch, dense batch in arrival order, sorted dense batch) with 64 queries at and beyond the far
   pin in front, PCT_BIN_SHIFT 0 and 4 (2^30 and 2^18 bins under the sort), and every other search that reads the table.  The twin, far
   pin at (1023, 1023, 1022.5): dims (1024, 1024, 1023), the largest table the 32-bit form is allowed.
B. Flat grids (1024, 1024, 1), (1024, 1, 1024), (1, 1024, 1024): 300 002 points, 0.29 per cell, under every build setting.
C. The floor: cell_size = max_ext / 5000 on boxes (1000, 700, 3) and (333, 100, 37.5) is coarsened to float32(max_ext / 1023), which
   rounds up for 1000 (1023 cells; the max point's fp32 cell coordinate is 1023 and only the clamp to g - 1 puts it into cell 1022) and
   down for 333 (1024 cells, no clamp needed).

Every answer is compared exactly, indices as integers and fp64 squared distances by their bits: the cell index against the brute force
on the same cloud (ALGO_STREAM_EXACT for NN, ALGO_STREAM elsewhere, an un-indexed cloud of the same points for the calls without an algo
argument), and on a sample -- every corner row and at least 256 rows drawn with a fixed seed -- against plain fp64 numpy
(tests/helpers/grid_limits.py, segment_model.py, segment_search_model.py, bezier_model.py).  pct_segment_nn_batch has no cell-index
form (resolve_algo sends it to the streaming kernel on any cloud); it runs here on the cube cloud all the same.

Not covered: the wide form's other two triggers (more than 2^28 - 16 points, more than 2^28 queries), the pyramid and the block table
on the cube (39 GB and 34 GB), a host read-back of the 4 GiB table (verify_grid checks it on the device).

Measured on the MI355X (first runs): build_grid of the cube 12-13 ms (upload and build 31-61 ms), of the twin 13 ms; a rebuild of the
cube under another switch, its batches and the rebuild back 60-110 ms.  Wall time of the tests: test_cube_build 0.03 s (+ 0.2 s for the
first cloud), test_cube_nn 0.02-0.04 s per size (the 700 case is the first to import torch for its device buffers and pays that once
for the process: 11 s when the file runs alone), test_cube_knn 0.5 s, test_cube_radius 0.14 s each, test_cube_segments 0.16 s,
test_cube_inflate 0.05 s each, test_cube_bezier_check 0.01 s, the twin 0.13 s, a flat grid 0.01 s (0.7 s for the first build of each
dims, which computes the brute force and its numpy sample once), a floor grid 0.03 s; the whole file 16 s.  Nothing had to be shrunk.
All 35 cases passed on their first run; no kernel had to be fixed.
"""
import os
import sys
import time

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import bezier_model as BM  # noqa: E402
import grid_limits as H  # noqa: E402
import segment_model as SM  # noqa: E402
import segment_search_model as SSM  # noqa: E402

pytestmark = pytest.mark.gpu

CUBE_PIN = (1023.0, 1023.0, 1023.0)
TWIN_PIN = (1023.0, 1023.0, 1022.5)
TWIN_B_TOP = 1022.0
NN_SIZES = (1, 700, 5000, 20000)       # single query, express batch (<= 1024), dense batch in arrival order, sorted dense batch (>= 16384)
SORTED_Q = 16384
SOUND = dict(bad_ids=0, duplicates=0, misplaced=0, decreasing=0, first=0)


@pytest.fixture(scope="module")
def E():
    from pointcloudtraj_amd import engine
    engine.init(0)
    return engine


def build(E, pts, cell, env):
    """a cloud of pts with its cell index built under the environment `env` (the switches are read at every build)"""
    with pytest.MonkeyPatch.context() as mp:
        for k in ("PCT_PYRAMID", "PCT_BLOCK_TABLE", "PCT_BIN_FORM", "PCT_BIN_SHIFT"):
            mp.delenv(k, raising=False)
        for k, v in env.items():
            mp.setenv(k, v)
        c = E.Cloud(len(pts))
        c.set_input(pts)
        t0 = time.perf_counter()
        c.build_grid(cell)
        print(f"build_grid of {c.grid_info()['dims']} under {env}: {time.perf_counter() - t0:.3f} s")
    return c


def assert_sound(c, n):
    v = c.verify_grid()
    assert v == dict(SOUND, last=n), v


def nn_device(E, c, q, algo):
    """pct_nn_batch_dev: the dense batch kernel for every batch size (the host form takes up to 1024 queries a block per query)"""
    import torch
    tq = torch.from_numpy(np.ascontiguousarray(q, np.float32)).cuda()
    tidx = torch.empty(len(q), dtype=torch.int32, device="cuda")
    td2 = torch.empty(len(q), dtype=torch.float64, device="cuda")
    c.reserve_queries(len(q))
    c.nn_device(tq.data_ptr(), len(q), tidx.data_ptr(), td2.data_ptr(), torch.cuda.current_stream().cuda_stream, algo)
    torch.cuda.synchronize()
    return tidx.cpu().numpy().astype(np.int64) & 0xFFFFFFFF, td2.cpu().numpy()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def check_nn(E, c, pts, q, what, keep=0, exact=None, numpy_ref=True, device=False):
    """ALGO_GRID against ALGO_STREAM_EXACT on the same cloud, and both against numpy on the first `keep` rows and a sample"""
    ri, rd = exact if exact is not None else c.nn(q, E.ALGO_STREAM_EXACT)
    gi, gd = nn_device(E, c, q, E.ALGO_GRID) if device else c.nn(q, E.ALGO_GRID)
    gi, ri = np.asarray(gi, np.int64), np.asarray(ri, np.int64)
    bad = np.nonzero((gi != ri) | (gd.view(np.uint64) != rd.view(np.uint64)))[0]
    assert len(bad) == 0, f"{what}: {len(bad)} of {len(q)} rows differ from the exact brute force, first rows {bad[:8]}: got {gi[bad[:8]]} want {ri[bad[:8]]}"
    if numpy_ref:
        rows = H.sample_rows(len(q), keep, 7400 + len(q))
        ni, nd = H.nn(pts, q[rows])
        assert np.array_equal(ri[rows], ni) and same_bits(rd[rows], nd), f"{what}: the exact brute force differs from numpy"
    return ri, rd


class Rig:
    """the module's two large clouds, made on first use; only one of them exists at a time (4 GiB of table each)"""

    def __init__(self, E):
        self.E, self.kind, self.c, self.plain = E, None, None, None
        self.pts = {"cube": H.cube_points(CUBE_PIN)[0], "twin": H.cube_points(TWIN_PIN, TWIN_B_TOP)[0]}

    def get(self, kind):
        if self.kind != kind:
            self.close()
            t0 = time.perf_counter()
            self.c = build(self.E, self.pts[kind], 1.0, {"PCT_PYRAMID": "0"})
            print(f"{kind} cloud: upload and build {time.perf_counter() - t0:.3f} s")
            self.kind = kind
        return self.c, self.pts[kind]

    def unindexed(self):
        """the cube's points without an index: the brute force of the calls that take no algo"""
        if self.plain is None:
            self.plain = self.E.Cloud(len(self.pts["cube"]))
            self.plain.set_input(self.pts["cube"])
        return self.plain

    def close(self):
        if self.c is not None:
            self.c.close()
        self.c, self.kind = None, None


@pytest.fixture(scope="module")
def rig(E):
    r = Rig(E)
    yield r
    r.close()
    if r.plain is not None:
        r.plain.close()


# ---- A. the cube of 2^30 cells -----------------------------------------------------------------------------------------------------

def test_cube_build(E, rig):
    c, pts = rig.get("cube")
    n = len(pts)
    info = c.grid_info()
    assert info == dict(dims=(1024, 1024, 1024), ncells=1 << 30, cell_size=1.0, origin=(0.0, 0.0, 0.0)), info
    assert c.pyramid_info()["levels"] == 0
    assert_sound(c, n)
    L = E.lib()
    for Q in NN_SIZES:
        assert L.pct_debug_narrow_offsets(n + 16, info["ncells"] + 1, Q) == 0          # what nn_run asks: the wide form
        assert L.pct_debug_narrow_offsets(n + 16, info["ncells"], Q) == 1              # one entry fewer would be narrow


@pytest.mark.parametrize("Q", NN_SIZES)
def test_cube_nn(E, rig, Q):
    c, pts = rig.get("cube")
    q = H.cube_batch(Q)
    keep = min(Q, H.N_CORNER)
    ri, _ = check_nn(E, c, pts, q, f"cube, host batch of {Q}", keep)
    assert np.all(ri[:keep] == 1), "the far pin (index 1) is the nearest point of every corner query"
    if Q == 1:
        for k in (H.N_CORNER // 2, H.N_CORNER + 3, 699):                             # more single queries: a corner row, cluster A, cluster B
            check_nn(E, c, pts, H.cube_batch(700)[k:k + 1], f"cube, single query {k}")
    if Q == 700:                                                                      # the dense kernel with a partly filled last block
        check_nn(E, c, pts, q, "cube, device batch of 700", keep, device=True)


@pytest.mark.parametrize("switch,value", [("PCT_BIN_SHIFT", "0"), ("PCT_BIN_SHIFT", "4"), ("PCT_NN_BLOCK", "256")])
def test_cube_nn_rebuilt(E, rig, switch, value, monkeypatch):
    """PCT_BIN_SHIFT: the sort key is the bin shifted until it is below 2^20 -- shift 0 gives 2^30 bins (key_shift 10), the default 1 gives
    2^27, 4 gives 2^18 (no shift).  PCT_NN_BLOCK=256: the wide form's other block size (a cloud this small takes 128 threads).  The index
    is rebuilt under the switch and rebuilt as it was afterwards."""
    c, pts = rig.get("cube")
    monkeypatch.setenv("PCT_PYRAMID", "0")
    monkeypatch.setenv(switch, value)
    try:
        c.build_grid(1.0)
        assert c.grid_info()["ncells"] == 1 << 30 and c.pyramid_info()["levels"] == 0
        for Q in ((20000,) if switch == "PCT_BIN_SHIFT" else (5000, 20000)):
            ri, _ = check_nn(E, c, pts, H.cube_batch(Q), f"cube, {switch}={value}, batch of {Q}", H.N_CORNER)
            assert np.all(ri[:H.N_CORNER] == 1)
    finally:
        monkeypatch.delenv(switch)
        c.build_grid(1.0)


def test_cube_knn(E, rig):
    c, pts = rig.get("cube")
    for Q in (1000, 20000):
        q = H.cube_batch(Q, seed=7500)
        gi, gd = c.knn(q, 8, E.ALGO_GRID)
        si, sd = c.knn(q, 8, E.ALGO_STREAM)
        assert np.array_equal(gi, si) and same_bits(gd, sd), f"k-NN, {Q} queries: the cell index differs from the streaming kernel"
        assert np.all(gi[:H.N_CORNER, 0] == 1)
        rows = H.sample_rows(Q, H.N_CORNER, 7510, 64 if Q == 1000 else 256)
        ni, nd = H.knn(pts, q[rows], 8)
        assert np.array_equal(gi[rows], ni) and same_bits(gd[rows], nd), f"k-NN, {Q} queries: differs from numpy"


@pytest.mark.parametrize("r", [0.5, 1.5])
def test_cube_radius(E, rig, r):
    c, pts = rig.get("cube")
    for Q in (1000, 20000):
        q = H.cube_batch(Q, seed=7520)
        gc = c.radius_count(q, r, E.ALGO_GRID)
        assert np.array_equal(gc, c.radius_count(q, r, E.ALGO_STREAM)), f"radius count, r = {r}, {Q} queries"
        if r == 1.5:                                                                   # d <= 0.45 per axis: the pin is within 0.78 of rows 0, 7..63
            assert gc[0] >= 1 and np.all(gc[7:H.N_CORNER] >= 1)
        rows = H.sample_rows(Q, H.N_CORNER, 7530, 64 if Q == 1000 else 256)
        for order in (E.ORDER_INDEX, E.ORDER_DISTANCE):
            go, gi, gd = c.radius_search(q, r, order, E.ALGO_GRID)
            so, si, sd = c.radius_search(q, r, order, E.ALGO_STREAM)
            assert np.array_equal(go, so) and np.array_equal(gi, si) and same_bits(gd, sd), f"radius search, r = {r}, order {order}, {Q} queries"
            assert np.array_equal(np.diff(go), gc.astype(np.int64))
            no, ni, nd = H.radius_rows(pts, q[rows], r, order)
            assert np.array_equal(np.diff(go)[rows], np.diff(no))
            sel = np.concatenate([np.arange(go[i], go[i + 1]) for i in rows]) if len(ni) else np.zeros(0, np.int64)
            assert np.array_equal(gi[sel], ni) and same_bits(gd[sel], nd), f"radius search, r = {r}, order {order}: differs from numpy"


def cube_segments(n=600, seed=7540):
    """segments at most 2 cells long that start at queries of the two clusters; the first 32 end on the far pin, 16 of them from beyond
    it (outside the grid), 16 from below it"""
    a = H.cube_batch(n, seed=seed).astype(np.float64)
    step = (H.synth.uniform01_f32(seed + 5, 3 * n).reshape(n, 3).astype(np.float64) - 0.5) * (4.0 / np.sqrt(3.0))
    a[:16] = np.asarray(CUBE_PIN) + np.abs(step[:16]) * 0.5
    a[16:32] = np.asarray(CUBE_PIN) - np.abs(step[16:32]) * 0.5
    a[32:H.N_CORNER] = np.asarray(CUBE_PIN) - np.abs(step[32:H.N_CORNER])
    b = a + step
    b[:32] = CUBE_PIN
    seg = np.concatenate([a, b], axis=1)
    assert np.all(np.sqrt(((seg[:, 3:] - seg[:, :3]) ** 2).sum(axis=1)) <= 2.0 + 1e-9)
    return seg


def test_cube_segments(E, rig):
    c, pts = rig.get("cube")
    seg = cube_segments()
    rows = np.concatenate([np.arange(32), H.sample_rows(len(seg), 32, 7550, 32)[32:]])
    for reach in (0.5, 1.5):
        ai, ad, as_ = c.segment_nn(seg, reach, E.ALGO_AUTO)                            # no cell-index form: the streaming kernel
        si, sd, ss = c.segment_nn(seg, reach, E.ALGO_STREAM)
        assert np.array_equal(ai, si) and same_bits(ad, sd) and same_bits(as_, ss)
        mi, md, ms = SM.segment_nn(pts, seg[rows], reach)
        assert np.array_equal(ai[rows], mi) and same_bits(ad[rows], md) and same_bits(as_[rows], ms), f"segment_nn, reach {reach}: differs from the model"
        assert np.all(ai[:32] == 1) and np.all(ad[:32] == 0.0)                         # they end on the pin
        gc = c.segment_count(seg, reach, E.ALGO_GRID)
        assert np.array_equal(gc, c.segment_count(seg, reach, E.ALGO_STREAM)), f"segment_count, reach {reach}"
        assert np.array_equal(gc[rows], SSM.segment_count(pts, seg[rows], reach))
        for order in (E.ORDER_INDEX, E.ORDER_DISTANCE):
            g = c.segment_search(seg, reach, order, E.ALGO_GRID)
            s = c.segment_search(seg, reach, order, E.ALGO_STREAM)
            assert np.array_equal(g[0], s[0]) and np.array_equal(g[1], s[1]) and same_bits(g[2], s[2]) and same_bits(g[3], s[3]), \
                f"segment_search, reach {reach}, order {order}"
            assert np.array_equal(np.diff(g[0]), gc.astype(np.int64))
            m = SSM.segment_search_boxed(pts, seg[rows], reach, order)
            sel = np.concatenate([np.arange(g[0][i], g[0][i + 1]) for i in rows])
            assert np.array_equal(np.diff(g[0])[rows], np.diff(m[0])) and np.array_equal(g[1][sel], m[1])
            assert same_bits(g[2][sel], m[2]) and same_bits(g[3][sel], m[3]), f"segment_search, reach {reach}, order {order}: differs from the model"
        gp = c.segment_polyhedron(seg, reach, E.ALGO_GRID)
        sp = c.segment_polyhedron(seg, reach, E.ALGO_STREAM)
        assert np.array_equal(gp[0], sp[0]) and np.array_equal(gp[1], sp[1]) and all(same_bits(a, b) for a, b in zip(gp[2:], sp[2:])), \
            f"segment_polyhedron, reach {reach}"


INFLATE = [dict(start=(1016.0, 1016.0, 1016.0), sample_range=30.0, search_margin=0.25, max_radius=1.5),
           dict(start=(6.0, 6.0, 6.0), sample_range=3.0, search_margin=0.1, max_radius=0.75)]


@pytest.mark.parametrize("k", [0, 1])
def test_cube_inflate(E, rig, k):
    """Q = 1000 is the one-launch form, Q = 5000 the staged one; the first parameter set early-outs cluster A's queries, the second
    cluster B's, the corner queries and cluster A's own rim"""
    c, pts = rig.get("cube")
    plain = rig.unindexed()
    p = INFLATE[k]
    prm = E.inflate_params(p["start"], p["sample_range"], p["search_margin"], p["max_radius"])
    for Q in (1000, 5000):
        q = H.cube_batch(Q, seed=7560).astype(np.float64)
        gr, gi, gd = c.inflate(prm, q)
        br, bi, bd = plain.inflate(prm, q)
        assert same_bits(gr, br) and np.array_equal(gi, bi) and same_bits(gd, bd), f"inflate, {Q} points: the cell index differs from the un-indexed cloud"
        rows = H.sample_rows(Q, H.N_CORNER, 7570)
        mr, mi, md = H.inflate(pts, p, q[rows])
        assert same_bits(gr[rows], mr) and same_bits(gd[rows], md), f"inflate, {Q} points: differs from numpy"
        assert np.array_equal(gi[rows].astype(np.int64), np.where(mi < 0, H.NO_INDEX, mi))
        assert (mi < 0).any() and (mi >= 0).any()
        if k == 0:
            assert np.all(gi[:H.N_CORNER] == 1)


def test_cube_bezier_check(E, rig):
    """two cubic segments through cluster B whose last control point is the far pin"""
    c, pts = rig.get("cube")
    plain = rig.unindexed()
    T = np.array([0.5, 0.5])
    od = np.array([3, 3], np.int32)
    ctrl = np.array([[(1014.0, 1014.5, 1013.5), (1016.0, 1015.0, 1016.5), (1017.0, 1018.0, 1017.0), (1018.5, 1018.5, 1018.5)],
                     [(1018.5, 1018.5, 1018.5), (1020.0, 1019.0, 1020.5), (1022.0, 1022.5, 1021.5), CUBE_PIN]])
    coef = np.stack([ctrl[s].T.reshape(-1) / T[s] for s in range(2)])                # the wire format: x0..x3 y0..y3 z0..z3, divided by the time
    p = dict(start=tuple(ctrl[0, 0]), sample_range=30.0, search_margin=0.25, max_radius=1.5)
    prm = E.inflate_params(p["start"], p["sample_range"], p["search_margin"], p["max_radius"])
    pos, _, _, _, n = BM.bezier_samples_exact_powers(coef, T, od, 0.0, 100.0, 0.02)
    assert 50 <= n <= 52 and np.abs(pos[-1] - np.asarray(CUBE_PIN)).max() < 0.6            # the last samples are in the pin's block of cells
    mr, mi, md = H.inflate(pts, p, pos)
    hits = np.nonzero(mr < 0.0)[0]
    want_first = int(hits[0]) if len(hits) else -1
    for stop, dt in ((100.0, 0.02), (100.0, 0.0005)):                                 # 50 samples: one launch; 2000: staged
        g = c.bezier_check(prm, coef, T, od, 0.0, stop, dt)
        b = plain.bezier_check(prm, coef, T, od, 0.0, stop, dt)
        assert g["n"] == b["n"] and g["first_hit"] == b["first_hit"] and np.array_equal(g["idx"], b["idx"])
        assert same_bits(g["pos"], b["pos"]) and same_bits(g["radius"], b["radius"]) and same_bits(g["d2"], b["d2"]), f"bezier_check, dt {dt}"
        if dt == 0.02:
            assert g["n"] == n and g["first_hit"] == want_first and same_bits(g["pos"], pos)
            assert same_bits(g["radius"], mr) and same_bits(g["d2"], md) and np.array_equal(g["idx"].astype(np.int64), np.where(mi < 0, H.NO_INDEX, mi))
        else:
            assert g["n"] > 1024 and 1 in g["idx"][-40:]                               # the far pin is the nearest point of late samples


def test_twin_just_below_the_limit(E, rig):
    """far pin at (1023, 1023, 1022.5): 1024 x 1024 x 1023 cells, 2^30 - 2^20 + 1 run bounds -- the narrow form at the largest table it takes"""
    c, pts = rig.get("twin")
    n = len(pts)
    info = c.grid_info()
    assert info == dict(dims=(1024, 1024, 1023), ncells=1023 << 20, cell_size=1.0, origin=(0.0, 0.0, 0.0)), info
    assert c.pyramid_info()["levels"] == 0
    assert_sound(c, n)
    for Q in NN_SIZES:
        assert E.lib().pct_debug_narrow_offsets(n + 16, info["ncells"] + 1, Q) == 1
        q = H.cube_batch(Q, TWIN_PIN, TWIN_B_TOP)
        keep = min(Q, H.N_CORNER)
        ri, _ = check_nn(E, c, pts, q, f"twin, host batch of {Q}", keep)
        assert np.all(ri[:keep] == 1)
    check_nn(E, c, pts, H.cube_batch(700, TWIN_PIN, TWIN_B_TOP), "twin, device batch of 700", H.N_CORNER, device=True)


# ---- B. flat grids: an axis at its cap --------------------------------------------------------------------------------------------

FLAT_ENVS = {"default": {}, "pyramid_off": {"PCT_PYRAMID": "0"}, "pyramid_on": {"PCT_PYRAMID": "1"},
             "block_table": {"PCT_PYRAMID": "0", "PCT_BLOCK_TABLE": "1"}, "generic_bins": {"PCT_BIN_FORM": "0"}}
_flat_exact = {}                      # dims -> the exact brute force of the batch, computed with the first build and compared with numpy once


@pytest.mark.parametrize("env", list(FLAT_ENVS))
@pytest.mark.parametrize("dims", [(1024, 1024, 1), (1024, 1, 1024), (1, 1024, 1024)], ids=["xy", "xz", "yz"])
def test_flat_grid(E, dims, env):
    pts, ext = H.flat_cloud(dims)
    q, nspecial = H.flat_queries(dims)
    c = build(E, pts, 1.0, FLAT_ENVS[env])
    try:
        info = c.grid_info()
        assert info == dict(dims=dims, ncells=1 << 20, cell_size=1.0, origin=(0.0, 0.0, 0.0)), info
        assert_sound(c, len(pts))
        levels = c.pyramid_info()["levels"]
        assert levels > 0 if env == "pyramid_on" else levels == 0 if env in ("pyramid_off", "block_table") else True
        first = dims not in _flat_exact
        if first:
            _flat_exact[dims] = c.nn(q, E.ALGO_STREAM_EXACT)
        ri, _ = check_nn(E, c, pts, q, f"flat {dims} under {env}", nspecial, exact=_flat_exact[dims], numpy_ref=first)
        assert ri[0] == 1                                                              # the query on the max-corner pin
    finally:
        c.close()


# ---- C. the cell-size floor and its fp32 rounding ----------------------------------------------------------------------------------

FLOOR_BOXES = [(1000.0, 700.0, 3.0), (333.0, 100.0, 37.5)]


def test_floor_rounds_both_ways():
    """the two cases of C round opposite ways (numpy, the build's expressions)"""
    one = np.float32(1.0)
    up, down = (np.float32(np.float64(m) / 1023.0) for m in (1000.0, 333.0))
    assert np.float64(up) > 1000.0 / 1023.0 and np.float64(down) < 333.0 / 1023.0
    assert int(np.floor(1000.0 / np.float64(up))) + 1 == 1023 and int(np.floor(333.0 / np.float64(down))) + 1 == 1024
    # the max point's cell coordinate before the clamp, floor((v - o) * inv_h) in fp32 with inv_h = 1.0f / h: 1023 in both cases
    assert np.floor(np.float32(1000.0) * (one / up)) == 1023.0 and np.floor(np.float32(333.0) * (one / down)) == 1023.0


def test_floor_keeps_every_axis_at_1024_cells():
    """h = max(h, max_ext / 1023) in fp64, then rounded to fp32: ext / (double)(float)h < 1024 for every extent, so min(1024, floor(.)) + 1
    never reaches 1025, the product of the dims never exceeds 2^30 and the refusal of more than 0x7FFFFFF0 cells cannot be reached"""
    rng = np.random.default_rng(7600)
    ext = np.concatenate([np.float32(2.0) ** rng.uniform(-100, 120, 200000), np.arange(1, 4097, dtype=np.float64),
                          np.float64([1023.0, 1000.0, 333.0, 3.4e38, 1e-30])]).astype(np.float32).astype(np.float64)
    for want in (0.0, 1.0 / 5000.0, 1.0 / 1023.0):                                     # a requested cell as a fraction of the extent
        h = np.maximum(ext * want, ext / 1023.0)
        h = np.minimum(np.maximum(h, 2.0 ** -120), 2.0 ** 120)
        hd = h.astype(np.float32).astype(np.float64)
        cells = np.floor(ext / hd)
        assert cells.max() <= 1023.0, (want, ext[np.argmax(cells)], cells.max())
        assert (np.minimum(1024.0, cells) + 1.0).max() == 1024.0
    assert 1024 ** 3 <= 0x7FFFFFF0


@pytest.mark.parametrize("box", FLOOR_BOXES, ids=["rounds_up_1000", "rounds_down_333"])
def test_floor_grid(E, box):
    pts, pin, h = H.floor_cloud(box)
    m = max(box)
    hd = float(np.float32(h))
    dims = tuple(min(1024, int(np.floor(b / hd))) + 1 for b in box)
    assert dims[0] == (1023 if m == 1000.0 else 1024)
    q = H.floor_queries(box, dims, h)
    for env in ({"PCT_PYRAMID": "0"}, {}):
        c = build(E, pts, m / 5000.0, env)
        try:
            info = c.grid_info()
            assert info["cell_size"] == np.float32(m / 1023.0) and info["cell_size"] == h, info
            assert info["dims"] == dims and info["origin"] == (0.0, 0.0, 0.0) and info["ncells"] == dims[0] * dims[1] * dims[2], info
            assert_sound(c, len(pts))
            exact = c.nn(q, E.ALGO_STREAM_EXACT)
            ri, _ = check_nn(E, c, pts, q, f"floor {box} under {env}: one launch", len(q), exact=exact)
            assert ri[0] == pin
            check_nn(E, c, pts, q, f"floor {box} under {env}: dense kernel", exact=exact, numpy_ref=False, device=True)
            big = np.tile(q, (SORTED_Q // len(q) + 1, 1))
            check_nn(E, c, pts, big, f"floor {box} under {env}: sorted dense kernel", exact=tuple(np.tile(a, SORTED_Q // len(q) + 1) for a in exact),
                     numpy_ref=False, device=True)
        finally:
            c.close()
