"""The engine at the edges of the fp32 range (GPU): every case of tests/test_numeric_edges.py through every way the engine can
answer it, bit-equal to the exhaustive oracle for ALL queries -- (index, d2) for nearest neighbour, counts and index lists for
the radius queries, radii for the sphere inflation.  Finite input has one right answer whatever its magnitude (include/pct_engine.h,
arithmetic contract); non-finite input has the documented one: PCT_OK, PCT_NO_INDEX and d2 = +inf for a query with a NaN or
infinite coordinate, the ordinary queries of the same batch unaffected; NaN / infinite cloud rows never win and are counted only
under r*r = +inf by the brute-force paths and by a rolling-map index created with an extent, while pct_cloud_build_grid and a
rolling-map index sized from the data refuse such a cloud with PCT_ERR_INVALID and leave it usable.

A path that disagrees is reported with the number of wrong queries and the first of them; every path of a test runs before the
test fails, so one run shows the whole picture."""
import os

import numpy as np
import pytest

import test_numeric_edges as NE
from test_numeric_edges import CASES, CASE_IDS, NONFINITE_QUERY_CASES, NONFINITE_ROW_CASES, expected

pytestmark = pytest.mark.gpu

EXPRESS_MAX_Q = 1024        # batches up to this size on an indexed cloud: a block per query (engine.hip kExpressMaxQ)
UNBINNED_Q = 2048           # the dense batch kernel in arrival order
BINNED_Q = 20_000           # >= 16384: counting-sorted by coarse cell first (test_large_batch_query_binning)


@pytest.fixture(scope="module")
def E():
    from pointcloudtraj_amd import engine
    engine.init(0)
    return engine


class Report:
    def __init__(self, case):
        self.case, self.lines = case, []

    def nn(self, path, got, want, sel=None):
        gi, gd = got
        wi, wd = want
        gi = np.where(gi == 0xFFFFFFFF, -1, gi.astype(np.int64))
        bad = (gi != wi) | (gd.view(np.uint64) != wd.view(np.uint64))
        if bad.any():
            j = int(np.nonzero(bad)[0][0])
            self.lines.append(f"{path}: {int(bad.sum())}/{len(bad)} queries wrong ({int((gd.view(np.uint64) != wd.view(np.uint64)).sum())} in d2), first at {j}: "
                              f"got ({gi[j]}, {gd[j]!r}) want ({wi[j]}, {wd[j]!r})")

    def eq(self, path, got, want):
        got, want = np.asarray(got), np.asarray(want)
        if got.shape != want.shape:
            self.lines.append(f"{path}: shape {got.shape} != {want.shape}")
            return
        bad = ~((got == want) | (np.isnan(got.astype(np.float64)) & np.isnan(want.astype(np.float64))))
        if bad.any():
            j = int(np.nonzero(bad.reshape(-1))[0][0])
            self.lines.append(f"{path}: {int(bad.sum())}/{bad.size} values wrong, first at {j}: got {got.reshape(-1)[j]!r} want {want.reshape(-1)[j]!r}")

    def note(self, line):
        self.lines.append(line)

    def done(self):
        assert not self.lines, f"{self.case.name}:\n  " + "\n  ".join(self.lines)


def padded_batch(case, want, Q):
    """the case's queries followed by copies of its inside-the-cloud queries up to Q (a very far query walks every shell of the
    grid, so those are not multiplied), with the expected (idx, d2, count) laid out the same way"""
    wi, wd, wc = want
    ins = np.nonzero(case.inside)[0]
    extra = ins[np.arange(max(0, Q - len(case.queries))) % len(ins)]
    sel = np.concatenate([np.arange(len(case.queries)), extra])
    return case.queries[sel], case.radii[sel], (wi[sel], wd[sel], wc[sel])


def check_index(c, pts):
    from test_gpu_parity import _check_cell_index
    with np.errstate(all="ignore"):
        _check_cell_index(c, pts)


class env:
    def __init__(self, **kv):
        self.kv = kv

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kv}
        os.environ.update(self.kv)

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def explicit_cell(pts):
    """an explicit cell size: a tenth of the largest extent (fp32), whatever the magnitude"""
    ext = float((pts.max(0).astype(np.float64) - pts.min(0).astype(np.float64)).max())
    h = np.float32(min(max(ext / 10.0, 1e-44), 3e38))
    return float(h) if h > 0 else 1.0


INDEX_CONFIGS = [("grid", {}, 0.0), ("grid+pyramid", {"PCT_PYRAMID": "1"}, 0.0),
                 ("grid+block-table", {"PCT_BLOCK_TABLE": "1", "PCT_PYRAMID": "0"}, 0.0), ("grid,cell_size", {}, None)]


# ---- finite input ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_nn_brute_force_paths(E, oracle, case):
    want = expected(case, oracle)
    rep = Report(case)
    with E.Cloud(len(case.pts)) as c:
        c.set_input(case.pts)
        try:
            for mode in (-1, 0, 1):
                E.set_filter_mode(mode)
                rep.nn(f"ALGO_STREAM filter mode {mode}", c.nn(case.queries, E.ALGO_STREAM), want[:2])
                q, _, w = padded_batch(case, want, UNBINNED_Q)
                rep.nn(f"ALGO_STREAM filter mode {mode}, Q={len(q)}", c.nn(q, E.ALGO_STREAM), w[:2])
        finally:
            E.set_filter_mode(-1)
        rep.nn("ALGO_STREAM_EXACT", c.nn(case.queries, E.ALGO_STREAM_EXACT), want[:2])
        rep.nn("ALGO_STREAM, 3 queries (all-fp64 kernel)", c.nn(case.queries[:3], E.ALGO_STREAM), (want[0][:3], want[1][:3]))
    rep.done()


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_nn_cell_index_paths(E, oracle, case):
    """the cell-sorted index in each of its forms x the three batch shapes: express (a block per query), the dense batch kernel in
    arrival order, the same behind the query sort; the built index is checked structurally every time"""
    want = expected(case, oracle)
    rep = Report(case)
    with E.Cloud(len(case.pts)) as c:
        c.set_input(case.pts)
        for label, envs, cell in INDEX_CONFIGS:
            with env(**envs):
                c.build_grid(explicit_cell(case.pts) if cell is None else cell)
                try:
                    check_index(c, case.pts)
                except AssertionError as e:
                    rep.note(f"{label}: index unsound: {str(e)[:300]}")
                if label == "grid" and case.family == "far" and not case.meta["small"]:
                    assert min(c.grid_info()["dims"]) >= 4, "the far-query clouds must have a grid the 3x3x3 cube does not cover"
                if label == "grid" and case.family == "far" and case.meta["small"]:
                    assert max(c.grid_info()["dims"]) <= 3
                assert len(case.queries) <= EXPRESS_MAX_Q
                rep.nn(f"{label}, express Q={len(case.queries)}", c.nn(case.queries, E.ALGO_GRID), want[:2])
                for Q in (UNBINNED_Q, BINNED_Q):
                    q, _, w = padded_batch(case, want, Q)
                    rep.nn(f"{label}, batch Q={Q}", c.nn(q, E.ALGO_GRID), w[:2])
    rep.done()


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_nn_rolling_map_index(E, oracle, case):
    """the ring index sized from the data and from a caller's extent, the cloud fed by appends (several frames)"""
    want = expected(case, oracle)
    rep = Report(case)
    ext = np.maximum(case.pts.max(0).astype(np.float64) - case.pts.min(0).astype(np.float64), 1e-30)
    for label, extent in (("ring", None), ("ring+extent", np.minimum(ext, 3e38).astype(np.float32))):
        with E.Cloud(len(case.pts)) as c:
            c.ring_index(0.0, extent)
            for part in np.array_split(case.pts, 3 if len(case.pts) >= 3 else 1):
                c.append(part)
            assert len(c) == len(case.pts)
            rep.nn(f"{label}, express", c.nn(case.queries), want[:2])
            q, _, w = padded_batch(case, want, UNBINNED_Q)
            rep.nn(f"{label}, batch Q={len(q)}", c.nn(q), w[:2])
            rep.nn(f"{label}, ALGO_STREAM over the window", c.nn(case.queries, E.ALGO_STREAM), want[:2])
    rep.done()


SMALL_CASES = [c for c in CASES if len(c.pts) <= 2000]


@pytest.mark.parametrize("case", SMALL_CASES, ids=[c.name for c in SMALL_CASES])
def test_nn_small_host_mapped_cloud(E, oracle, case):
    """the host-mapped fp32 tree behind the kd_* drop-in, device path forced (host threshold 0): single queries"""
    from pointcloudtraj_amd import kdtree as K
    wi, wd, _ = expected(case, oracle)
    rep = Report(case)
    old = K.host_threshold()
    K.set_host_threshold(0)
    try:
        t = K.KDTree()
        t.insert(case.pts)
        ids, pos = t.nearest(case.queries)
        t.close()
    finally:
        K.set_host_threshold(old)
    # kd_nearest* resolves exact ties to the node the reference's own tree walk returns (kdtree_gpu.cpp reference_tie_winner), not to
    # the lowest index: the node must attain the exact minimum, and be THE minimiser where that is unique
    rep.eq("kd_nearestf: d2 of the returned node", NE.numpy_d2(case.pts, case.queries)[np.arange(len(ids)), ids], wd)
    uniq = NE.numpy_ties(case.pts, case.queries) == 1
    rep.eq("kd_nearestf: node, unique minimisers", ids[uniq], wi[uniq])
    rep.eq("kd_nearestf: position", pos, case.pts[ids].astype(np.float64))
    rep.done()


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_radius_queries(E, oracle, case):
    want = expected(case, oracle)
    rep = Report(case)
    n = len(case.pts)
    with E.Cloud(n) as c:
        c.set_input(case.pts)
        q, r, w = padded_batch(case, want, UNBINNED_Q)
        try:
            for mode in (0, 1):
                E.set_filter_mode(mode)
                rep.eq(f"count ALGO_STREAM filter mode {mode}", c.radius_count(case.queries, case.radii, E.ALGO_STREAM), want[2])
                rep.eq(f"count ALGO_STREAM filter mode {mode}, Q={len(q)}", c.radius_count(q, r, E.ALGO_STREAM), w[2])
        finally:
            E.set_filter_mode(-1)
        rep.eq("count ALGO_STREAM, 5 queries", c.radius_count(case.queries[:5], case.radii[:5], E.ALGO_STREAM), want[2][:5])
        # one centre per case: the list and the crop (fp64 centre = the fp32 query widened, fp64 radius = the fp32 radius widened)
        j = int(np.argmax(want[2] * (want[2] <= 5000))) if case.family != "radii" else 2
        d2row = NE.numpy_d2(case.pts, case.queries[j:j + 1])[0]
        rr = np.float64(case.radii[j])
        with np.errstate(all="ignore"):
            hits = np.nonzero(d2row <= rr * rr)[0]
        ids, cnt = c.radius_indices(case.queries[j], float(case.radii[j]))
        rep.eq("radius_indices count", cnt, len(hits))
        rep.eq("radius_indices list", ids, hits)
        ci, cd, cxyz = c.radius_crop(case.queries[j].astype(np.float64), float(rr))
        rep.eq("radius_crop indices", ci, hits)
        rep.eq("radius_crop d2", cd, d2row[hits])
        rep.eq("radius_crop points", cxyz, case.pts[hits])
        c.build_grid()
        rep.eq("count ALGO_GRID", c.radius_count(case.queries, case.radii, E.ALGO_GRID), want[2])
        rep.eq(f"count ALGO_GRID, Q={len(q)}", c.radius_count(q, r, E.ALGO_GRID), w[2])
        qb, rb, wb = padded_batch(case, want, BINNED_Q)
        rep.eq(f"count ALGO_GRID, Q={len(qb)}", c.radius_count(qb, rb, E.ALGO_GRID), wb[2])
    rep.done()


def _inflate_want(P, wi, wd, start, sample_range, margin, max_radius):
    """radiusSearch (corridor_finder.cpp:113-133) over the oracle's nearest neighbour, as oracle.inflate_brute: a point farther than
    sample_range + max_radius from start_pt returns max_radius - search_margin without a search (an infinite coordinate is such a
    point; a NaN compares false and is searched: no neighbour, radius = max_radius)"""
    with np.errstate(all="ignore"):
        d = P - np.asarray(start, np.float64)
        far = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]) > sample_range + max_radius
        rad = np.where(far, max_radius - margin, np.minimum(np.sqrt(wd) - margin, max_radius))
    return rad, np.where(far, -1, wi), np.where(far, np.inf, wd)


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_inflate_on_every_index(E, oracle, case):
    """sphere inflation (radiusSearch) with a sample_range the early-out never reaches; the last three planner points lie beyond
    the fp32 range and narrow to +/-inf: no neighbour, d2 = +inf, radius = max_radius"""
    wi, wd, _ = expected(case, oracle)
    rep = Report(case)
    scale = float(np.abs(case.pts).max()) or 1.0
    margin, max_radius = 0.01 * scale, 0.5 * scale
    prm = E.inflate_params(case.pts[0].astype(np.float64), 1e300, margin, max_radius)
    beyond = np.float64([[3.5e38, 0, 0], [0, -1e39, 0], [1e39, 1e39, -1e39]])
    P = np.concatenate([case.queries.astype(np.float64), beyond])
    wi = np.concatenate([wi, [-1, -1, -1]])
    wd = np.concatenate([wd, [np.inf] * 3])
    wr, wi2, wd2 = _inflate_want(P, wi, wd, case.pts[0], 1e300, margin, max_radius)
    assert np.array_equal(wi2, wi) and np.array_equal(wd2, wd), "the early-out must not fire in this test"

    def run(label, c):
        rad, idx, d2 = c.inflate(prm, P)
        rep.nn(f"inflate on {label}: NN", (idx, d2), (wi, wd))
        rep.eq(f"inflate on {label}: radius", rad, wr)
        sel = np.concatenate([np.arange(len(P)), np.nonzero(case.inside)[0][np.arange(UNBINNED_Q) % int(case.inside.sum())]])
        rad, idx, d2 = c.inflate(prm, P[sel])
        rep.nn(f"inflate on {label}, Q={len(sel)}: NN", (idx, d2), (wi[sel], wd[sel]))
        rep.eq(f"inflate on {label}, Q={len(sel)}: radius", rad, wr[sel])

    with E.Cloud(len(case.pts)) as c:
        c.set_input(case.pts)
        run("no index", c)
        c.build_grid()
        run("static grid", c)
    with E.Cloud(len(case.pts)) as c:
        c.ring_index()
        c.append(case.pts)
        run("ring", c)
    rep.done()


def test_inflate_early_out_boundary(E, oracle):
    """planner points exactly on, one ulp either side of and just beyond |p - start| = sample_range + max_radius: the early-out
    compares with a strict `>` in fp64, so the first two are searched and the last two are not.  Four points run the block kernels
    on an indexed cloud and the staged kernels on a plain one; one more than the express limit runs the staged kernels on all
    three; the same four as corridor nodes of a captured replan batch run the fused kernel on the grid and on the ring."""
    cloud = np.float32([[4, 0, 0], [40, 0, 0]])
    start, sample_range, margin, max_radius = (0.0, 0.0, 0.0), 3.0, 0.25, 1.5
    P = np.zeros((4, 3))
    P[:, 0] = [np.nextafter(4.5, 0.0), 4.5, np.nextafter(4.5, np.inf), 4.5 + 1e-9]
    wr, wi, wd = oracle.inflate_brute(cloud, start, sample_range, margin, max_radius, P)
    assert np.array_equal(wr, [0.25, 0.25, 1.25, 1.25]) and np.array_equal(wi, [0, 0, -1, -1]) and np.array_equal(wd, [0.25, 0.25, np.inf, np.inf])
    prm = E.inflate_params(start, sample_range, margin, max_radius)
    many = np.arange(EXPRESS_MAX_Q + 1) % 4
    wrong = []                  # every path runs before the test fails (module docstring)

    def same(label, rad, idx, d2, sel):
        idx = np.where(idx == 0xFFFFFFFF, -1, idx.astype(np.int64))
        if not (np.array_equal(rad, wr[sel]) and np.array_equal(idx, wi[sel]) and np.array_equal(d2, wd[sel])):
            wrong.append(f"{label}: radius {rad[:4]!r} index {idx[:4]!r} d2 {d2[:4]!r}")

    def run(label, c, planned):
        same(f"{label}, 4 points", *c.inflate(prm, P), np.arange(4))
        same(f"{label}, {len(many)} points", *c.inflate(prm, P[many]), many)
        if planned:
            plan = E.ReplanPlan(c, 4, 1, 1)
            o = plan.run(prm, P)
            same(f"{label}, corridor nodes of a replan batch", o["node_radius"], o["node_idx"], o["node_d2"], np.arange(4))
            plan.close()

    with E.Cloud(len(cloud)) as c:
        c.set_input(cloud)
        run("no index", c, False)
        c.build_grid()
        run("static grid", c, True)
    with E.Cloud(len(cloud)) as c:
        c.ring_index()
        c.append(cloud)
        run("ring", c, True)
    assert not wrong, "\n  ".join(wrong)


# ---- non-finite input --------------------------------------------------------------------------------------------------------

def _nn_paths(E, c, q, with_index):
    """(label, result) of every NN path for one batch on a cloud that may carry an index"""
    out = []
    try:
        for mode in (-1, 0, 1):
            E.set_filter_mode(mode)
            out.append((f"ALGO_STREAM filter mode {mode}", c.nn(q, E.ALGO_STREAM)))
    finally:
        E.set_filter_mode(-1)
    if len(q) <= 4096:
        out.append(("ALGO_STREAM_EXACT", c.nn(q, E.ALGO_STREAM_EXACT)))
    if with_index:
        out.append(("index (ALGO_AUTO)", c.nn(q)))
    return out


@pytest.mark.parametrize("case", NONFINITE_QUERY_CASES, ids=[c.name for c in NONFINITE_QUERY_CASES])
def test_nonfinite_queries(E, oracle, case):
    """status PCT_OK (no exception), (PCT_NO_INDEX, +inf) and count 0 for the non-finite queries, everything else bit-equal to the
    batch without them"""
    want = expected(case, oracle)
    pos, clean = case.meta["positions"], case.meta["clean"]
    rep = Report(case)
    keep = case.inside

    def check(label, c, with_index):
        for path, got in _nn_paths(E, c, case.queries, with_index):
            rep.nn(f"{label}: {path}", got, want[:2])
        if with_index:
            ci, cd = c.nn(clean)
            gi, gd = c.nn(case.queries)
            rep.eq(f"{label}: ordinary queries vs the batch without the non-finite ones (idx)", gi[keep], ci[keep])
            rep.eq(f"{label}: ordinary queries vs the batch without the non-finite ones (d2)", gd[keep], cd[keep])
        for algo, name in ((E.ALGO_STREAM, "ALGO_STREAM"),) + (((E.ALGO_GRID, "ALGO_GRID"),) if with_index == "grid" else ()):
            rep.eq(f"{label}: count {name}", c.radius_count(case.queries, case.radii, algo), want[2])
            rinf = np.full(len(case.queries), np.inf, np.float32)
            rep.eq(f"{label}: count {name}, r = +inf", c.radius_count(case.queries, rinf, algo), oracle.brute_count(case.pts, case.queries, rinf))
        if len(case.queries) <= EXPRESS_MAX_Q * 2:
            prm = E.inflate_params((5, 5, 5), 1e300, 0.05, 1.5)
            rad, idx, d2 = c.inflate(prm, case.queries.astype(np.float64))
            wr, wi, wd = _inflate_want(case.queries.astype(np.float64), want[0], want[1], (5, 5, 5), 1e300, 0.05, 1.5)
            rep.nn(f"{label}: inflate NN", (idx, d2), (wi, wd))
            rep.eq(f"{label}: inflate radius", rad, wr)

    with E.Cloud(len(case.pts)) as c:
        c.set_input(case.pts)
        check("no index", c, False)
        for label, envs, cell in INDEX_CONFIGS:
            with env(**envs):
                c.build_grid(explicit_cell(case.pts) if cell is None else cell)
                check(label, c, "grid")
    with E.Cloud(len(case.pts)) as c:
        c.ring_index()
        c.append(case.pts)
        check("ring", c, "ring")
    rep.done()


@pytest.mark.parametrize("case", NONFINITE_ROW_CASES, ids=[c.name for c in NONFINITE_ROW_CASES])
def test_nonfinite_cloud_rows(E, oracle, case):
    """ignored by the brute-force paths and by a ring index created with an extent; the index builds that need the data's bounding
    box refuse the cloud with PCT_ERR_INVALID and a message, and leave it usable"""
    want = expected(case, oracle)
    rep = Report(case)
    with E.Cloud(len(case.pts)) as c:
        c.set_input(case.pts)
        for path, got in _nn_paths(E, c, case.queries, False):
            rep.nn(path, got, want[:2])
        try:
            for mode in (0, 1):
                E.set_filter_mode(mode)
                rep.eq(f"count ALGO_STREAM filter mode {mode}", c.radius_count(case.queries, case.radii, E.ALGO_STREAM), want[2])
        finally:
            E.set_filter_mode(-1)
        with pytest.raises(E.EngineError) as ei:
            c.build_grid()
        assert ei.value.code == 2 and "non-finite" in str(ei.value), str(ei.value)
        assert not c.has_grid
        rep.nn("ALGO_STREAM after the refused build_grid", c.nn(case.queries, E.ALGO_STREAM), want[:2])
        rep.nn("ALGO_AUTO after the refused build_grid", c.nn(case.queries), want[:2])
    with E.Cloud(len(case.pts)) as c:
        c.ring_index(0.0, np.float32([10, 10, 10]))
        for part in np.array_split(case.pts, 3):
            c.append(part)
        rep.nn("ring+extent, express", c.nn(case.queries), want[:2])
        q, _, w = padded_batch(case, want, UNBINNED_Q)
        rep.nn(f"ring+extent, batch Q={len(q)}", c.nn(q), w[:2])
    with E.Cloud(len(case.pts)) as c:
        c.set_input(case.pts)
        with pytest.raises(E.EngineError) as ei:
            c.ring_index()                                     # sized from the data's bounding box: refused
        assert ei.value.code == 2 and "non-finite" in str(ei.value), str(ei.value)
        assert not c.has_ring_index
        rep.nn("ALGO_STREAM after the refused ring index", c.nn(case.queries, E.ALGO_STREAM), want[:2])
        rep.nn("ALGO_AUTO after the refused ring index", c.nn(case.queries), want[:2])
    rep.done()
