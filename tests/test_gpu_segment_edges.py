"""The segment family at the edges of the fp32 range (GPU): the cases of tests/helpers/segment_edge_cases.py -- derived from those of
tests/test_numeric_edges.py: the scale ladder 1e-30 .. 1e38, ends up to FLT_MAX away, sentinel rows at +/-FLT_MAX, subnormals and signed
zeros, special reaches -- through pct_segment_nn_batch, pct_segment_inflate_batch, pct_segment_sweep_batch, pct_segment_count_batch,
pct_segment_search_batch and pct_segment_polyhedron_batch on every path that answers them: the streaming forms, the cell index in two
cell sizes, the rolling map sized from the data, from an extent, and with a table much smaller than the cloud.

The arithmetic is fp64 on fp32-narrowed operands, so every finite input has one right answer, and the numpy models of
tests/helpers/segment_*_model.py state it (tests/test_segment_edges_model.py holds them to the exact rational chain).  Every
comparison is bit for bit: indices and counts exactly, d2, s, t, radii and planes on their bit patterns, NaN equal to NaN only where
the model says NaN.  A path that disagrees is reported with the number of wrong entries and the first of them; every path of a test
runs before the test fails, so one run shows the whole picture."""
import functools
import os
import sys

import numpy as np
import pytest

from test_gpu_numeric_edges import Report, explicit_cell
from test_numeric_edges import CASES, CASE_IDS, NONFINITE_ROW_CASES

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import segment_edge_cases as X  # noqa: E402
import segment_model as M  # noqa: E402
import segment_polyhedron_model as PM  # noqa: E402
import segment_search_model as SS  # noqa: E402
import segment_sweep_model as W  # noqa: E402
from test_segment_edges_model import classes_of, poly_input  # noqa: E402

pytestmark = pytest.mark.gpu

NO_INDEX = M.NO_INDEX
SLICE_Q = 16_400            # one more slice than 16 384 segments
LIST_ROW_MAX = 4096         # rows longer than this are listed for two segments per batch only (counted for all)


@pytest.fixture(scope="module")
def E():
    from pointcloudtraj_amd import engine
    engine.init(0)
    return engine


def same_bits(got, want):
    got, want = np.ascontiguousarray(got, np.float64), np.ascontiguousarray(want, np.float64)
    return (got.view(np.uint64) == want.view(np.uint64)) | (np.isnan(got) & np.isnan(want))


class Rep(Report):
    """Report with the comparisons of the segment calls"""

    def f64(self, path, got, want):
        got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
        if got.shape != want.shape:
            self.lines.append(f"{path}: shape {got.shape} != {want.shape}")
            return
        bad = ~same_bits(got, want).reshape(-1)
        if bad.any():
            j = int(np.flatnonzero(bad)[0])
            self.lines.append(f"{path}: {int(bad.sum())}/{bad.size} values differ in their bits, first at {j}: got {got.reshape(-1)[j]!r} want {want.reshape(-1)[j]!r}")

    def seg(self, path, got, want, names=("d2", "s")):
        """(idx, x, y) triples or (idx, t) pairs"""
        gi, wi = np.asarray(got[0]), np.asarray(want[0])
        bad = gi.astype(np.int64) != wi.astype(np.int64)
        for g, w in zip(got[1:], want[1:]):
            bad = bad | ~same_bits(g, w)
        if bad.any():
            j = int(np.flatnonzero(bad)[0])
            show = lambda r: "(" + ", ".join([str(int(r[0][j]) if r[0][j] != NO_INDEX else -1)] + [repr(float(v[j])) for v in r[1:]]) + ")"     # noqa: E731
            self.lines.append(f"{path}: {int(bad.sum())}/{len(bad)} segments wrong ({int((gi != wi).sum())} in the index), first at {j}: "
                              f"got {show(got)} want {show(want)} (index, {', '.join(names)})")


# ---- the clouds of a case ----------------------------------------------------------------------------------------------------------

def ring_forms(case):
    """(label, cell size, extent) of the rolling maps a case is filed in"""
    out = [("ring", 0.0, None), ("ring+extent", 0.0, X.ring_extent(case.pts))]
    st = X.small_table(case)
    if st is not None:
        out.append(("ring, small table", st[0], st[1]))
    return out


def cloud_forms(E, case, grid=False, rings=True):
    """(label, cloud, [(name, algo)]) for every index a case is asked on, one at a time; the rolling maps are fed by three appends"""
    pts = case.pts
    with E.Cloud(len(pts)) as c:
        c.set_input(pts)
        yield "plain cloud", c, [("ALGO_STREAM", E.ALGO_STREAM)]
        if grid:
            for label, cell in (("grid", 0.0), ("grid,cell_size", explicit_cell(pts))):
                c.build_grid(cell)
                yield label, c, [("ALGO_GRID", E.ALGO_GRID), ("ALGO_AUTO", E.ALGO_AUTO)]
    for label, cell, extent in (ring_forms(case) if rings else ()):
        with E.Cloud(len(pts)) as c:
            c.ring_index(cell, extent)
            for part in np.array_split(pts, 3 if len(pts) >= 3 else 1):
                c.append(part)
            assert len(c) == len(pts)
            yield label, c, [("ALGO_RING", E.ALGO_RING), ("ALGO_AUTO", E.ALGO_AUTO), ("ALGO_STREAM", E.ALGO_STREAM)]


# ---- expected results ----------------------------------------------------------------------------------------------------------------

def model_rows(pts, segs, reach):
    """(counts [Q], sel, {q: (ids ascending, d2, s)}) of the capsule search's model, one segment at a time (a [Q, N] table of the
    largest cloud would not fit comfortably).  Every segment is counted; the rows kept for the lists are those of at most LIST_ROW_MAX
    entries and the first two longer ones (sel: their segments, ascending)"""
    segs = np.asarray(segs, np.float64).reshape(-1, 6)
    reach = np.broadcast_to(np.asarray(reach, np.float64), (len(segs),))
    counts, kept, nlong = np.zeros(len(segs), np.int64), {}, 0
    for q in range(len(segs)):
        (d2, s, hit), = SS.row_masks(pts, segs[q:q + 1], reach[q:q + 1])
        ids = np.flatnonzero(hit)
        counts[q] = len(ids)
        if len(ids) <= LIST_ROW_MAX or nlong < 2:
            kept[q] = (ids, d2[ids], s[ids])
            nlong += len(ids) > LIST_ROW_MAX
    return counts, np.array(sorted(kept), np.int64), kept


def lists_of(kept, sel, order):
    """(offsets, idx, d2, s) of the rows `sel` in `order`"""
    masks = []
    for q in sel:
        ids, d2, s = kept[int(q)]
        n = (int(ids.max()) + 1) if len(ids) else 0
        D, S_, H = np.zeros(n), np.zeros(n), np.zeros(n, bool)
        D[ids], S_[ids], H[ids] = d2, s, True
        masks.append((D, S_, H))
    return SS.rows_from(masks, order)


@functools.lru_cache(maxsize=None)
def sweep_want(name, which):
    sc = X._derive(name)
    segs, rad = sweep_sets(sc)[which][1:]
    return W.segment_sweep(sc.case.pts, segs, rad)


def sweep_sets(sc):
    return [("per-segment radius", sc.segments, sc.reach), ("start-free radii", sc.segments, sc.sweep_radius),
            ("special radii", sc.special_segments, sc.special_reach)]


def inflate_want(nn_inf, margin, max_radius):
    """segment_model.segment_inflate on the unbounded answers already at hand (test_segment_inflate checks it against the model)"""
    idx, d2, s = nn_inf
    with np.errstate(invalid="ignore"):
        rr = np.sqrt(d2) - np.float64(margin)
        near = rr < np.float64(max_radius)
    return np.where(near, rr, np.float64(max_radius)), np.where(near, idx, np.uint32(NO_INDEX)).astype(np.uint32), np.where(near, s, np.nan)


# ---- segment_nn --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_segment_nn(E, case):
    sc = X.derive(case)
    rep = Rep(case)
    sets = [(label, segs, reach, M.cut_at_reach(free, segs, reach)) for label, segs, reach, free in X.reach_sets(sc)]
    deg = sc.rows("degenerate")
    slices = case.name in ("ladder/s=1e+38/centred/no-outside-queries(overflow)", "far/n=30000/ext=10")
    if slices:
        ins = np.flatnonzero(case.inside[:-1] & case.inside[1:])
        ins = ins[ins < len(sc.rows("pairs"))]
        assert len(ins) >= 8 and np.all(sc.tags[ins] == "pairs")
        sel = ins[np.arange(SLICE_Q) % len(ins)]
    for label, c, algos in cloud_forms(E, case, grid=True):
        if label.startswith("grid"):                                    # no cell-index form: refused, the cloud untouched
            with pytest.raises(E.EngineError) as ei:
                c.segment_nn(sc.segments, sc.reach, E.ALGO_GRID)
            assert ei.value.code == 2, str(ei.value)
            algos = [("ALGO_AUTO", E.ALGO_AUTO)] if label == "grid" else []
        for name, algo in algos:
            for what, segs, reach, want in sets:
                rep.seg(f"{label}, {name}, {what}", c.segment_nn(segs, reach, algo), want)
            pi, pd = c.nn(sc.segments[deg, :3].astype(np.float32), E.ALGO_STREAM)
            gi, gd, gs = c.segment_nn(sc.segments[deg], np.inf, algo)
            rep.seg(f"{label}, {name}: degenerate segments against c.nn of the same points", (gi, gd), (pi, pd), ("d2",))
            rep.f64(f"{label}, {name}: s of degenerate segments", gs, np.zeros(len(deg)))
            if slices and name in ("ALGO_STREAM", "ALGO_RING") and label in ("plain cloud", "ring"):
                got = c.segment_nn(sc.segments[sel], sc.reach[sel], algo)
                rep.seg(f"{label}, {name}, Q={SLICE_Q}", got, tuple(v[sel] for v in sets[0][3]))
    rep.done()


# ---- segment_inflate ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_segment_inflate(E, case):
    sc = X.derive(case)
    rep = Rep(case)
    scale = float(np.abs(case.pts).max()) or 1.0
    m0, r0 = 0.01 * scale, 0.5 * scale                                  # test_gpu_numeric_edges.test_inflate_on_every_index's pair
    pairs = [(m0, r0)] + [(m0, r) for r in (np.inf, X.F, 1e-42, 0.0)] + [(m, r0) for m in (0.0, 1e30, -m0, -2.0 * r0)] + [(0.0, 0.0), (0.0, 1e-200)]
    wants = [inflate_want(sc.nn_inf, m, r) for m, r in pairs]
    if len(case.pts) <= 31_000:
        for k in (0, 4, 9):
            mr, mi, ms = M.segment_inflate(case.pts, sc.segments, *pairs[k])
            assert np.all(same_bits(mr, wants[k][0])) and np.array_equal(mi, wants[k][1]) and np.all(same_bits(ms, wants[k][2]))
    for label, c, _ in cloud_forms(E, case, grid=False):
        for (m, r), want in zip(pairs, wants):
            rad, idx, s = c.segment_inflate(sc.segments, E.inflate_params(case.pts[0].astype(np.float64), 1e300, m, r))
            rep.seg(f"{label}, search_margin {m!r} max_radius {r!r}", (idx, rad, s), (want[1], want[0], want[2]), ("radius", "s"))
    rep.done()


# ---- segment_sweep -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_segment_sweep(E, case):
    sc = X.derive(case)
    rep = Rep(case)
    sets = sweep_sets(sc)
    for label, c, algos in cloud_forms(E, case, grid=True):
        if label.startswith("grid"):
            if label == "grid":
                with pytest.raises(E.EngineError) as ei:
                    c.segment_sweep(sc.segments, sc.reach, E.ALGO_GRID)
                assert ei.value.code == 2, str(ei.value)
            continue
        for name, algo in algos:
            if name == "ALGO_AUTO":
                continue
            for k, (what, segs, rad) in enumerate(sets):
                wi, wt = sweep_want(case.name, k)
                gi, gt = c.segment_sweep(segs, rad, algo)
                rep.seg(f"{label}, {name}, {what}", (gi, gt), (wi, wt), ("t",))
                zero = (wi != NO_INDEX) & (wt == 0)
                if not np.array_equal(gt.view(np.uint64) == 0, zero):
                    rep.note(f"{label}, {name}, {what}: t == +0.0 on {np.flatnonzero(gt.view(np.uint64) == 0)[:6]}, the model on {np.flatnonzero(zero)[:6]}")
                ni, _, _ = c.segment_nn(segs, rad, algo)
                if not np.array_equal(ni != NO_INDEX, gi != NO_INDEX):
                    rep.note(f"{label}, {name}, {what}: the blocked sweeps are not the segments segment_nn finds a row for under reach = r: "
                             f"first at {int(np.flatnonzero((ni != NO_INDEX) != (gi != NO_INDEX))[0])}")
    rep.done()


# ---- segment_count and segment_search ------------------------------------------------------------------------------------------------

def ring_classes(c, label, sets, case):
    """seg_capsule_box's classes on the table the engine built (ring_info()), the rolling map sized from the data included, whose
    geometry no host restatement knows: a reach of +inf is wild on every table; on a table of at least eight positions an axis the
    degenerate segments under the reach of their nearest row are unfolded (three to five cells); on a small table (at most 16 positions an axis)
    the pairs across the cloud are folded"""
    if not c.has_ring_index:
        return
    info = c.ring_info()
    got = {}
    for _, segs, reach, *_ in (sets[0], sets[3], sets[-1]):
        a, b = M.narrow(segs)
        for q in range(len(a)):
            if M.reach2(reach[q]) is not None:
                k = X.ring_box_class(info["dims"], info["cell_size"], a[q], b[q], reach[q])
                got[k] = got.get(k, 0) + 1
    assert got.get("wild", 0) >= 1, f"{case.name}, {label}: no wild box on {info}: {got}"
    if len(case.pts) >= 100 and min(info["dims"]) >= 8:
        assert got.get("unfolded", 0) >= 1, f"{case.name}, {label}: no unfolded box on {info}: {got}"
    # (ring_configure holds the extent it sizes a table from at 1e-6 or more: the ladder rung at 1e-12 gets 256 positions an axis
    # whatever extent is asked, so no table is small against that cloud -- DESIGN.md, section 7)
    if label == "ring, small table" and max(info["dims"]) <= 16:
        assert got.get("folded", 0) >= 1, f"{case.name}, {label}: no box folded by its span on {info}: {got}"


# far/n=200000/ext=3000 is the one case that sees ss_grid_box's magnitude guard dropped: with the per-cell skip applied outside the
# guard, only this cloud loses candidate rows (on both cell sizes); the clouds of 30 701 rows or fewer lose none.  Keep it.
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_segment_count_and_search(E, case):
    sc = X.derive(case)
    rep = Rep(case)
    sets = []
    for label, segs, reach, _ in X.reach_sets(sc):
        counts, sel, kept = model_rows(case.pts, segs, reach)
        sets.append((label, segs, reach, counts, sel, {o: lists_of(kept, sel, o) for o in (SS.ORDER_INDEX, SS.ORDER_DISTANCE)}))
    cpu_classes, got = classes_of(case), {}
    for label, c, algos in cloud_forms(E, case, grid=True):
        if label.startswith("grid"):
            gi = c.grid_info()
            for _, segs, reach, *_ in (sets[0], sets[3], sets[-1]):     # the sets classes_of counts: on the engine's own geometry
                a, b = M.narrow(segs)
                for q in range(len(a)):
                    if M.reach2(reach[q]) is not None:
                        k = "guard " + X.guard_class(gi["origin"], gi["dims"], gi["cell_size"], a[q], b[q], reach[q])
                        got[k] = got.get(k, 0) + 1
            if label == "grid,cell_size":
                if case.family == "ladder":
                    assert got.get("guard inside", 0) >= 1, f"{case.name}: no segment inside the guard with an interior cell in its box: {got} {gi}"
                for k in ("guard inside", "guard reach", "guard end"):
                    if cpu_classes.get(k, 0) >= 12:
                        assert got.get(k, 0) >= 1, f"{case.name}: class '{k}' is empty on the engine's grids ({gi}): {got}"
            # interior cells exist: at least four cells an axis on the far and radii cases.  A cloud of one or two rows spans no such
            # box at any cell size, and at six points a cell the data-sized grid of 17 or 100 rows (far/n=17, far/n=100, radii/n=100)
            # is (2, 2, 2) or (3, 3, 3): those are held to it on the explicit cell size only.
            if label == "grid,cell_size" and case.family in ("far", "radii") and len(case.pts) >= 17:
                assert min(gi["dims"]) >= 4, gi
            if label == "grid" and case.family in ("far", "radii") and len(case.pts) >= 30_000:
                assert min(gi["dims"]) >= 4, gi
        else:
            ring_classes(c, label, sets, case)
        for name, algo in algos:
            for what, segs, reach, counts, sel, lists in sets:
                path = f"{label}, {name}, {what}"
                rep.eq(f"{path}: count", c.segment_count(segs, reach, algo).astype(np.int64), counts)
                for order, oname in ((SS.ORDER_INDEX, "ORDER_INDEX"), (SS.ORDER_DISTANCE, "ORDER_DISTANCE")):
                    off, idx, d2, s = c.segment_search(segs[sel], reach[sel], order, algo)
                    woff, widx, wd2, ws = lists[order]
                    rep.eq(f"{path}, {oname}: offsets", off, woff)
                    rep.eq(f"{path}, {oname}: np.diff(offsets) against the count", np.diff(off), counts[sel])
                    if len(idx) == len(widx):
                        rep.seg(f"{path}, {oname}: entries", (idx, d2, s), (widx, wd2, ws))
    rep.done()


# ---- segment_polyhedron --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_segment_polyhedron(E, case):
    sc = X.derive(case)
    rep = Rep(case)
    segs, reach, _ = poly_input(sc)
    woff, widx, wd2, ws, wpl = PM.segment_polyhedron(case.pts, segs, reach)
    assert np.diff(woff).max() <= 64
    if len(X.derive(case).rows("rows")) and len(case.pts) > 2:
        assert np.any(np.all(wpl == [0.0, 0.0, 0.0, -1.0], axis=1)), "a support ON its segment: the plane (0, 0, 0, -1)"
    for label, c, algos in cloud_forms(E, case, grid=True):
        for name, algo in algos:
            off, idx, d2, s, pl = c.segment_polyhedron(segs, reach, algo)
            path = f"{label}, {name}"
            rep.eq(f"{path}: offsets", off, woff)
            if len(idx) == len(widx):
                rep.seg(f"{path}: supports", (idx, d2, s), (widx, wd2, ws))
                rep.f64(f"{path}: planes", pl, wpl)
    rep.done()


# ---- non-finite rows ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", NONFINITE_ROW_CASES, ids=[c.name for c in NONFINITE_ROW_CASES])
def test_nonfinite_rows(E, case):
    """a NaN / infinite row is never a winner, a blocker, a list entry or a support, under any reach including +inf (the models say so:
    its d2 is NaN or +inf, never <= DBL_MAX); build_grid refuses the cloud and leaves it to the streaming forms"""
    sc = X.derive(case)
    rep = Rep(case)
    pts, bad = case.pts, case.meta["bad_rows"]
    inf = np.full(len(sc.reach), np.inf)
    nn_sets = [(w, r, M.cut_at_reach(sc.nn_inf, sc.segments, r)) for w, r in (("per-segment reach", sc.reach), ("reach = +inf", inf))]
    assert not np.any(np.isin(sc.nn_inf[0], bad)) and np.all(sc.nn_inf[0] != NO_INDEX)
    rows = {w: model_rows(pts, sc.segments, r) for w, r in (("per-segment reach", sc.reach), ("reach = +inf", inf))}
    assert np.all(rows["reach = +inf"][0] == len(pts) - len(bad)), "under reach = +inf every finite row is listed, no other"
    assert all(not np.any(np.isin(r[0], bad)) for w in rows for r in rows[w][2].values())
    sel = rows["per-segment reach"][1]
    psegs, preach, _ = X.capped(pts, np.concatenate([sc.segments, sc.segments[:8]]), np.concatenate([sc.reach, np.full(8, 1e200)]))
    pwant = PM.segment_polyhedron(pts, psegs, preach)
    assert not np.any(np.isin(pwant[1], bad))
    sweeps = [(w, r, W.segment_sweep(pts, sc.segments, r)) for w, r in (("per-segment radius", sc.reach), ("start-free radii", sc.sweep_radius), ("radius = +inf", inf))]

    def run(label, c, algos):
        for name, algo in algos:
            for what, reach, want in nn_sets:
                rep.seg(f"{label}, {name}, segment_nn, {what}", c.segment_nn(sc.segments, reach, algo), want)
            for what, rad, want in sweeps:
                rep.seg(f"{label}, {name}, segment_sweep, {what}", c.segment_sweep(sc.segments, rad, algo), want, ("t",))
            for what, reach in (("per-segment reach", sc.reach), ("reach = +inf", inf)):
                rep.eq(f"{label}, {name}, segment_count, {what}", c.segment_count(sc.segments, reach, algo).astype(np.int64), rows[what][0])
            for order in (SS.ORDER_INDEX, SS.ORDER_DISTANCE):
                off, idx, d2, s = c.segment_search(sc.segments[sel], sc.reach[sel], order, algo)
                woff, widx, wd2, ws = lists_of(rows["per-segment reach"][2], sel, order)
                rep.eq(f"{label}, {name}, segment_search order {order}: offsets", off, woff)
                if len(idx) == len(widx):
                    rep.seg(f"{label}, {name}, segment_search order {order}: entries", (idx, d2, s), (widx, wd2, ws))
            off, idx, d2, s, pl = c.segment_polyhedron(psegs, preach, algo)
            rep.eq(f"{label}, {name}, segment_polyhedron: offsets", off, pwant[0])
            if len(idx) == len(pwant[1]):
                rep.seg(f"{label}, {name}, segment_polyhedron: supports", (idx, d2, s), pwant[1:4])
                rep.f64(f"{label}, {name}, segment_polyhedron: planes", pl, pwant[4])
        m, r = 0.05, 1.5
        rad, idx, s = c.segment_inflate(sc.segments, E.inflate_params((5, 5, 5), 1e300, m, r))
        want = inflate_want(sc.nn_inf, m, r)
        rep.seg(f"{label}, segment_inflate", (idx, rad, s), (want[1], want[0], want[2]), ("radius", "s"))

    with E.Cloud(len(pts)) as c:
        c.set_input(pts)
        run("plain cloud", c, [("ALGO_STREAM", E.ALGO_STREAM)])
        with pytest.raises(E.EngineError) as ei:
            c.build_grid()
        assert ei.value.code == 2 and "non-finite" in str(ei.value), str(ei.value)
        assert not c.has_grid
        run("plain cloud after the refused build_grid", c, [("ALGO_STREAM", E.ALGO_STREAM), ("ALGO_AUTO", E.ALGO_AUTO)])
    with E.Cloud(len(pts)) as c:
        c.ring_index(0.0, np.float32([10, 10, 10]))
        for part in np.array_split(pts, 3):
            c.append(part)
        run("ring+extent", c, [("ALGO_RING", E.ALGO_RING), ("ALGO_AUTO", E.ALGO_AUTO), ("ALGO_STREAM", E.ALGO_STREAM)])
    rep.done()


# ---- cells beyond the ring's clamp ---------------------------------------------------------------------------------------------------

CLAMP_CELL = 1e-4           # rows around 1e6: cell 1e10, beyond the clamp of 1e9 cells


def clamp_case():
    """2 000 rows around (1e6, 1e6, 1e6) spaced by ulps (2^-4 there), with duplicates; segments among and around them"""
    rng = np.random.default_rng(1_000_006)
    ulp = 2.0 ** -4
    pts = (1e6 + ulp * rng.integers(-40, 41, (2000, 3))).astype(np.float32)
    pts[-16:] = pts[100:116]
    q = (1e6 + ulp * rng.integers(-60, 61, (48, 3))).astype(np.float64)
    segs = np.concatenate([np.concatenate([q[:-1], q[1:]], 1), np.concatenate([q[:6], q[:6]], 1),
                           np.concatenate([pts[100:104], pts[-16:-12]], 1).astype(np.float64), np.concatenate([pts[5:9], pts[300:304]], 1).astype(np.float64)])
    d2 = M.segment_nn(pts, segs, np.inf)[1]
    reach = np.where(np.arange(len(segs)) % 4 == 0, X.boundary_reach(d2), np.resize(np.float64([0.0, 0.2, 1.0, 3.0, 1e7, np.inf]), len(segs)))
    return pts, np.ascontiguousarray(segs), reach


def test_cells_beyond_the_ring_clamp(E):
    """every row and every segment end is wild (beyond 1e9 cells of the requested size): the engine accepts the index -- the rows go
    where the clamp sends them -- and all five calls equal the models on it"""
    pts, segs, reach = clamp_case()
    assert all(X.ring_axis_wild(v, 1.0 / CLAMP_CELL) for v in pts.reshape(-1)[:64]) and all(X.ring_axis_wild(v, 1.0 / CLAMP_CELL) for v in segs.reshape(-1))

    class _C:
        name = "beyond the ring's clamp"
    rep = Rep(_C)
    free = M.segment_nn(pts, segs, np.inf)
    counts, sel, kept = model_rows(pts, segs, reach)
    assert len(sel) == len(segs)
    psegs, preach, _ = X.capped(pts, segs, reach)
    pwant = PM.segment_polyhedron(pts, psegs, preach)
    sweep = W.segment_sweep(pts, segs, reach)
    with E.Cloud(len(pts)) as c:
        c.ring_index(CLAMP_CELL, np.float32([8 * CLAMP_CELL] * 3))
        for part in np.array_split(pts, 3):
            c.append(part)
        assert c.has_ring_index and len(c) == len(pts), "the index is accepted (DESIGN.md, section 7)"
        info = c.ring_info()
        assert abs(info["cell_size"] - CLAMP_CELL) < 1e-9 and max(info["dims"]) <= 16, info
        for name, algo in (("ALGO_RING", E.ALGO_RING), ("ALGO_AUTO", E.ALGO_AUTO), ("ALGO_STREAM", E.ALGO_STREAM)):
            rep.seg(f"{name}, segment_nn", c.segment_nn(segs, reach, algo), M.cut_at_reach(free, segs, reach))
            rep.seg(f"{name}, segment_nn, reach = +inf", c.segment_nn(segs, np.inf, algo), free)
            rep.seg(f"{name}, segment_sweep", c.segment_sweep(segs, reach, algo), sweep, ("t",))
            rep.eq(f"{name}, segment_count", c.segment_count(segs, reach, algo).astype(np.int64), counts)
            for order in (SS.ORDER_INDEX, SS.ORDER_DISTANCE):
                off, idx, d2, s = c.segment_search(segs, reach, order, algo)
                woff, widx, wd2, ws = lists_of(kept, sel, order)
                rep.eq(f"{name}, segment_search order {order}: offsets", off, woff)
                if len(idx) == len(widx):
                    rep.seg(f"{name}, segment_search order {order}: entries", (idx, d2, s), (widx, wd2, ws))
            off, idx, d2, s, pl = c.segment_polyhedron(psegs, preach, algo)
            rep.eq(f"{name}, segment_polyhedron: offsets", off, pwant[0])
            if len(idx) == len(pwant[1]):
                rep.seg(f"{name}, segment_polyhedron: supports", (idx, d2, s), pwant[1:4])
                rep.f64(f"{name}, segment_polyhedron: planes", pl, pwant[4])
        rad, idx, s = c.segment_inflate(segs, E.inflate_params((1e6, 1e6, 1e6), 1e300, 0.05, 1.5))
        want = inflate_want(free, 0.05, 1.5)
        rep.seg("segment_inflate", (idx, rad, s), (want[1], want[0], want[2]), ("radius", "s"))
    rep.done()
