"""What "right" means for the segment family at the edges of the fp32 range, pinned on the CPU before any GPU is involved: the
cases of tests/helpers/segment_edge_cases.py (derived from tests/test_numeric_edges.py) through the numpy models of the segment
contract (tests/helpers/segment_*_model.py).

  * the models are the correctly rounded chain: a sample of (segment, row) pairs per case again in exact rational arithmetic, rounded
    once per operation, bit for bit -- the plain high-precision reference of the same operation, and a guard against a numpy build
    that fuses;
  * the conditions every family must keep so that its cases go on biting (assertions, so that an edit of the generator cannot quietly
    stop them);
  * the engine's magnitude guard and ring boxes restated on the host, to assert that the suite reaches every class of them.
"""
import functools
import math
import os
import sys
from fractions import Fraction

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import segment_edge_cases as X  # noqa: E402
import segment_model as M  # noqa: E402
import segment_polyhedron_model as PM  # noqa: E402
import segment_search_model as SS  # noqa: E402
import segment_sweep_model as W  # noqa: E402
from test_numeric_edges import CASES, CASE_IDS  # noqa: E402

NO_INDEX = M.NO_INDEX


def bits(v):
    return np.float64(v).view(np.uint64)


# ---- the scalar chain in rational arithmetic ------------------------------------------------------------------------------------

def fl(x):
    """one rounding: float(Fraction) is correctly rounded (subnormals included); beyond the range it is +/-inf"""
    try:
        return float(x)
    except OverflowError:
        return math.inf if x > 0 else -math.inf


def _op(f):
    def g(x, y):
        if not (math.isfinite(x) and math.isfinite(y)):
            return f(np.float64(x), np.float64(y)).item()      # only reached with an operand already at +/-inf
        return fl(f(Fraction(x), Fraction(y)))
    return g


add, sub, mul = _op(lambda x, y: x + y), _op(lambda x, y: x - y), _op(lambda x, y: x * y)


def div(x, y):
    return fl(Fraction(x) / Fraction(y))


def chain(p, a, b, r2):
    """(d2, s, ww, disc, t) of one row against one segment by the contract's text, each operation exact and rounded once; disc and t
    are None where the contract does not compute them (ww <= r2)"""
    p, a, b = ([float(v) for v in u] for u in (p, a, b))
    e = [sub(b[k], a[k]) for k in range(3)]
    L2 = add(add(mul(e[0], e[0]), mul(e[1], e[1])), mul(e[2], e[2]))
    w = [sub(p[k], a[k]) for k in range(3)]
    dot = add(add(mul(w[0], e[0]), mul(w[1], e[1])), mul(w[2], e[2]))
    s = 0.0 if L2 == 0 else div(dot, L2)
    s = 0.0 if not s > 0 else min(s, 1.0)
    c = [sub(w[k], mul(s, e[k])) for k in range(3)]
    d2 = add(add(mul(c[0], c[0]), mul(c[1], c[1])), mul(c[2], c[2]))
    ww = add(add(mul(w[0], w[0]), mul(w[1], w[1])), mul(w[2], w[2]))
    if ww <= r2:
        return d2, s, ww, None, 0.0
    g = sub(ww, r2)
    disc = sub(mul(dot, dot), mul(L2, g))
    if not disc > 0:
        disc = 0.0
    t = div(sub(dot, math.sqrt(disc)), L2) if L2 != 0 else math.nan
    t = 0.0 if not t > 0 else min(t, s)
    return d2, s, ww, disc, t


@functools.lru_cache(maxsize=None)
def sweep_model(name):
    sc = X._derive(name)
    return W.segment_sweep(sc.case.pts, sc.segments, sc.sweep_radius)


def near_boundary_rows(d2, r2):
    """rows whose d2 lies within 4 ulp of r2"""
    with np.errstate(all="ignore"):
        return np.flatnonzero(np.abs(d2 - r2) <= 4.0 * np.spacing(r2))


NEAR_ALL = 400              # a case with at most this many (segment, row) pairs within 4 ulp of a bound has all of them checked
NEAR_PER_BOUND = 2          # beyond that: this many per (segment, bound), drawn with a fixed seed


def near_boundary_pairs(sc, a, b):
    """every (segment, row) whose d2 lies within 4 ulp of one of the segment's bounds -- its reach, the reach that just admits its
    winner, its sweep radius -- over ALL segments of the case.  The ladder and tiny cases have 120 to 170 of them and every one is
    checked.  Where r2 == 0 or a far end makes whole clouds qualify (every row of a far or sentinel cloud has d2 == 0 or one d2 from
    a segment that ends 1e18 away: 4 746 pairs on far/n=100, over a million on the 30 000-row clouds) the exact chain on each is not
    affordable: such a case keeps NEAR_PER_BOUND rows per (segment, bound), drawn with a fixed seed, a few hundred in all."""
    pts = sc.case.pts
    found = []
    for q in range(len(a)):
        d2, _ = M.pair_d2_s(pts, a[q], b[q])
        for r in (sc.reach[q], sc.reach_k[1.0][q], sc.sweep_radius[q]):
            found.append((q, near_boundary_rows(d2, M.reach2(r))))
    if sum(len(rows) for _, rows in found) <= NEAR_ALL:
        return {(q, int(i)) for q, rows in found for i in rows}
    rng = np.random.default_rng(78)
    return {(q, int(i)) for q, rows in found for i in (rows if len(rows) <= NEAR_PER_BOUND else rng.choice(rows, NEAR_PER_BOUND, replace=False))}


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_models_are_the_correctly_rounded_chain(case):
    sc = X.derive(case)
    pts = case.pts
    a, b = M.narrow(sc.segments)
    rng = np.random.default_rng(77)
    pairs = set()
    for q in range(len(a)):                                    # every winner
        if sc.nn_inf[0][q] != NO_INDEX:
            pairs.add((q, int(sc.nn_inf[0][q])))
    wi, _ = sweep_model(case.name)
    for q in np.flatnonzero(wi != NO_INDEX)[::3]:              # and blockers
        pairs.add((int(q), int(wi[q])))
    for q, i in near_boundary_pairs(sc, a, b):                 # every row within 4 ulp of its r2 (capped where they run to thousands)
        pairs.add((q, i))
    if len(sc.rows("lattice")):                                # the lattice-tie rows
        lo, hi = X.dyadic_rows(case)
        for q in sc.rows("lattice"):
            d2, _ = M.pair_d2_s(pts[lo:hi], a[q], b[q])
            for i in np.flatnonzero(d2 == d2.min()):
                pairs.add((int(q), lo + int(i)))
    while len(pairs) < 40 or len(pairs) < min(60, len(a)):     # and arbitrary pairs
        pairs.add((int(rng.integers(0, len(a))), int(rng.integers(0, len(pts)))))
    assert len(pairs) >= 40
    n_disc = 0
    for q, i in sorted(pairs):
        r2 = M.reach2(sc.sweep_radius[q])
        d2, s, ww, disc, t = chain(pts[i], a[q], b[q], r2)
        md2, ms = M.pair_d2_s(pts[i:i + 1], a[q], b[q])
        blocker, mt, ms2 = W.pair_entry(pts[i:i + 1], a[q], b[q], r2)
        im = X.intermediates(pts[i:i + 1], a[q], b[q], r2)
        where = f"{case.name}: segment {q} ({sc.tags[q]}), row {i}"
        assert bits(d2) == bits(md2[0]) and bits(s) == bits(ms[0]) and bits(s) == bits(ms2[0]), where
        assert bits(ww) == bits(im["ww"][0]) and bits(d2) == bits(im["d2"][0]) and bits(s) == bits(im["s"][0]), where
        assert bool(blocker[0]) == (math.isfinite(d2) and d2 <= r2), where
        if a[q].tolist() != b[q].tolist() or ww <= r2:         # L2 == 0 with ww > r2: no blocker, t is nobody's
            assert bits(t) == bits(mt[0]), where
        if disc is not None:
            n_disc += 1
            assert bits(disc) == bits(np.where(im["disc"][0] > 0, im["disc"][0], 0.0)), where
    assert n_disc >= 3 or len(pts) < 17, f"{case.name}: the sample computed disc {n_disc} times"


# ---- family conditions ----------------------------------------------------------------------------------------------------------

def poly_input(sc):
    """what the polyhedra are asked: every segment under its reach and under 1.5 x its boundary reach, and the first eight under a
    reach that takes the whole cloud -- through capped()"""
    segs = np.concatenate([sc.segments, sc.segments, sc.segments[:8]])
    reach = np.concatenate([sc.reach, sc.reach_k[1.5], np.full(min(8, len(sc.segments)), 1e200)])
    return X.capped(sc.case.pts, segs, reach)


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_family_conditions(case):
    sc = X.derive(case)
    pts, n = case.pts, len(case.pts)
    idx, d2, s = sc.nn_inf
    assert np.all(idx != NO_INDEX), "every segment of a finite case finds a row under reach = +inf"
    assert np.any(s == 0) and np.any(s == 1), f"{case.name}: winners at both ends"
    if n > 2:
        assert np.any((s > 0) & (s < 1)), f"{case.name}: no winner strictly inside a segment"
    # counts of 0, 1 and more; the boundary reaches flip the winner
    counts = {k: SS.segment_count(pts, sc.segments, sc.reach_k[k]) for k in X.KS}
    allc = np.concatenate([counts[k] for k in X.KS] + [SS.segment_count(pts, sc.segments, sc.reach)])
    assert np.any(allc == 0) and np.any(allc == 1), f"{case.name}: counts {np.unique(allc)[:8]}"
    if n > 1:
        assert np.any(allc > 1), case.name
    pos = d2 > 0
    for k, inside in ((X.KS[0], False), (1.0, True), (X.KS[2], True)):
        got = M.cut_at_reach(sc.nn_inf, sc.segments, sc.reach_k[k])[0] != NO_INDEX
        assert np.all(got[pos] == inside), f"{case.name}: k = {k!r} leaves the winner {'out' if inside else 'in'} on {np.flatnonzero(got[pos] != inside)[:5]}"
        assert np.all((counts[k][pos] >= 1) == inside), case.name
    assert pos.sum() >= 10, case.name
    # the sweeps
    wi, wt = sweep_model(case.name)
    blocked = wi != NO_INDEX
    kinds = (np.sum(blocked & (wt == 0)), np.sum(blocked & (wt > 0) & (wt < 1)), np.sum(~blocked & (wt == 1)))
    if n >= 17:
        assert all(k >= 1 for k in kinds), f"{case.name}: sweeps t == 0 / inside / free: {kinds}"
    if case.family == "ladder":
        assert kinds[1] >= 4, f"{case.name}: {kinds}"
    # capped rows
    csegs, creach, kept = poly_input(sc)
    cc = SS.segment_count(pts, csegs, creach)
    assert len(cc) and np.all(cc <= 64) and np.all(creach > 0) and np.all(np.isfinite(creach)), case.name
    if n > 8:
        assert np.any(cc > 8), f"{case.name}: the longest capped row has {cc.max()} entries"
    if n > 64:
        assert np.any(cc == 64), "a row cut to exactly the cap: the strict cut just below the 65th candidate"


def exact_d2(p, a, b):
    """the exact rational squared distance of a row to a segment"""
    p, a, b = ([Fraction(float(v)) for v in u] for u in (p, a, b))
    e = [b[k] - a[k] for k in range(3)]
    w = [p[k] - a[k] for k in range(3)]
    L2 = sum(x * x for x in e)
    s = Fraction(0) if L2 == 0 else max(Fraction(0), min(Fraction(1), sum(w[k] * e[k] for k in range(3)) / L2))
    return sum((w[k] - s * e[k]) ** 2 for k in range(3))


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_exact_ties_fall_to_the_lower_index(case):
    """dup-ties: over the WHOLE cloud at least two rows attain the exact rational minimum, at a d2 > 0, and the model names the lowest
    of them.  lattice: the uniform rows of these clouds lie nearer to any segment than half a lattice step, so the two dyadic rows
    cannot be the cloud's winners; among the dyadic rows exactly two attain the exact minimum, and under the reach of exactly that
    distance (representable: 8 lattice units) the model lists both with one d2, the lower index first.  A cloud without two equal
    rows (one or two points) has neither group."""
    sc = X.derive(case)
    pts = case.pts
    assert len(sc.rows("dup-ties")) == 2 or len(pts) <= 2, f"{case.name}: the cloud's duplicated rows gave no tie segments"
    a, b = M.narrow(sc.segments)
    for q in sc.rows("dup-ties"):
        d2, _ = M.pair_d2_s(pts, a[q], b[q])
        near = np.argsort(d2, kind="stable")[:24]
        ex = [exact_d2(pts[i], a[q], b[q]) for i in near]
        mins = sorted(int(i) for i, v in zip(near, ex) if v == min(ex))
        assert len(mins) >= 2 and min(ex) > 0, f"{case.name}: segment {q}: minimisers {mins}"
        assert len(pts) <= 24 or d2[near[-1]] > d2[near[0]] * 1.01, "the 24 nearest by the model cover every exact minimiser"
        assert int(sc.nn_inf[0][q]) == mins[0], f"{case.name}: segment {q}: the model names {sc.nn_inf[0][q]}, the lowest minimiser is {mins[0]}"
    lo, hi = X.dyadic_rows(case) if len(sc.rows("lattice")) else (0, 0)
    for q in sc.rows("lattice"):
        ex = [exact_d2(pts[i], a[q], b[q]) for i in range(lo, hi)]
        mins = [lo + i for i, v in enumerate(ex) if v == min(ex)]
        r = 8.0 * X.lattice_step(case)
        assert len(mins) == 2 and min(ex) == Fraction(r) ** 2, f"{case.name}: segment {q}: dyadic minimisers {mins}"
        sub_i, sub_d2, sub_s = M.segment_nn(pts[lo:hi], sc.segments[q:q + 1], np.inf)
        assert lo + int(sub_i[0]) == mins[0] and 0 < sub_s[0] < 1 and sub_d2[0] == r * r
        off, li, ld, _ = SS.segment_search(pts, sc.segments[q:q + 1], r, SS.ORDER_DISTANCE)
        at = [int(np.flatnonzero(li == m)[0]) for m in mins]
        assert at[1] == at[0] + 1 and ld[at[0]] == ld[at[1]] == r * r and at[1] == len(li) - 1, "both on the inclusive boundary, the lower index first"


def test_range_spans_and_subnormal_segments_keep_the_chain_finite_and_normal():
    for case in (c for c in CASES if c.family == "ladder" and c.meta["scale"] == 1e38):
        sc = X.derive(case)
        a, b = M.narrow(sc.segments)
        rows = sc.rows("range")
        assert len(rows) >= 3
        for q in rows:
            for r in (sc.sweep_radius[q], sc.reach_k[1.0][q]):
                im = X.intermediates(case.pts, a[q], b[q], M.reach2(r))
                assert im["L2"] > 1e77, f"{case.name}: segment {q}: L2 = {im['L2']!r}"
                for k, v in im.items():
                    assert np.all(np.isfinite(v)), f"{case.name}: segment {q}: intermediate {k} is not finite"
    case = next(c for c in CASES if c.name.startswith("tiny/subnormal"))
    sc = X.derive(case)
    a, b = M.narrow(sc.segments)
    tiny = np.finfo(np.float64).tiny
    L2s = []
    for q in range(len(a)):
        im = X.intermediates(case.pts, a[q], b[q], M.reach2(sc.sweep_radius[q]))
        L2s.append(float(im["L2"]))
        for k, v in im.items():
            v = np.abs(np.asarray(v))
            assert not np.any((v > 0) & (v < tiny)), f"{case.name}: segment {q}: intermediate {k} is subnormal in fp64"
    assert sum(0 < v < 1e-80 for v in L2s) >= 5
    z = sc.rows("zeros")
    assert np.any(np.signbit(sc.segments[z])) and np.any(sc.segments[z] == 0.0) and len(z) >= 5


# ---- the guard and the ring boxes, restated on the host ---------------------------------------------------------------------------

def geometries(case):
    """the index geometries the GPU tests build for a case: [("grid", origin, dims, h)], [("ring", dims, h)].  The rolling map sized
    from the data is not among them: its table is sized from the first append and may be re-sized by a later one, so its geometry
    is known on the GPU only -- tests/test_gpu_segment_edges.py repeats the class assertions there from ring_info()"""
    pts = case.pts
    grids = [("grid",) + X.grid_geometry(pts, 0.0), ("grid,cell_size",) + X.grid_geometry(pts, X.explicit_cell(pts))]
    rings = [("ring+extent",) + X.ring_geometry(X.ring_extent(pts).astype(np.float64), len(pts))]
    st = X.small_table(case)
    if st is not None:
        rings.append(("small table",) + X.ring_geometry(st[1].astype(np.float64), len(pts), st[0]))
    return grids, rings


def classes_of(case):
    """{class: number of (segment, reach, geometry) triples}, and whether some segment has the guard inside with an interior cell"""
    sc = X.derive(case)
    grids, rings = geometries(case)
    out = {}
    sets = [(sc.segments, sc.reach), (sc.segments, sc.reach_k[1.0]), (sc.special_segments, sc.special_reach)]
    for segs, reach in sets:
        a, b = M.narrow(segs)
        for q in range(len(a)):
            if M.reach2(reach[q]) is None:
                continue
            for _, o, dims, h in grids:
                k = "guard " + X.guard_class(o, dims, h, a[q], b[q], reach[q])
                out[k] = out.get(k, 0) + 1
            for _, dims, h in rings:
                k = "ring " + X.ring_box_class(dims, h, a[q], b[q], reach[q])
                out[k] = out.get(k, 0) + 1
    return out


def test_guard_and_ring_box_classes_are_all_reached():
    total = {}
    for case in CASES:
        got = classes_of(case)
        for k, v in got.items():
            total[k] = total.get(k, 0) + v
        if case.family == "ladder":
            assert got.get("guard inside", 0) >= 1, f"{case.name}: no segment with the guard inside and an interior cell in its box: {got}"
    for k in ("guard inside", "guard reach", "guard end", "ring wild", "ring folded", "ring unfolded"):
        assert total.get(k, 0) >= 10, f"class '{k}' has {total.get(k, 0)} segments over the whole suite: {total}"


def test_host_restatements():
    """guard_inside and ring_axis_wild on hand-made values either side of their limits"""
    o, dims, h = (0.0, 0.0, 0.0), (10, 10, 10), 1.0
    lim = 2.0 ** 30
    assert X.guard_inside(o, dims, h, (1, 1, 1), (2, 2, 2), 0.5)
    assert not X.guard_inside(o, dims, h, (1, 1, 1), (2, 2, 2), lim) and X.guard_inside(o, dims, h, (1, 1, 1), (2, 2, 2), np.nextafter(lim, 0))
    assert not X.guard_inside(o, dims, h, (1, 1, 1), (2, lim, 2), 0.5) and not X.guard_inside(o, dims, h, (1, -lim, 1), (2, 2, 2), 0.5)
    assert not X.guard_inside((lim, 0, 0), dims, h, (lim, 1, 1), (lim, 2, 2), 0.5), "the grid itself beyond 2^30 cells"
    assert not X.guard_inside(o, dims, h, (1, 1, 1), (2, 2, 2), np.inf)
    assert X.guard_class(o, dims, h, (3, 3, 3), (5, 5, 5), 0.5) == "inside" and X.guard_class(o, (2, 2, 2), h, (1, 1, 1), (1, 1, 1), 0.5) == "inside-border"
    assert X.guard_class(o, dims, h, (3, 3, 3), (5, 5, 5), 1e19) == "reach" and X.guard_class(o, dims, h, (3, 3, 3), (1e19, 5, 5), 1.0) == "end"
    assert not X.ring_axis_wild(999_999_999.5, 1.0) and X.ring_axis_wild(1e9, 1.0) and X.ring_axis_wild(-1e9, 1.0) and not X.ring_axis_wild(-999_999_999.0, 1.0) and X.ring_axis_wild(-999_999_999.5, 1.0)
    assert X.ring_axis_wild(np.nan, 1.0) and X.ring_axis_wild(np.inf, 1.0) and X.ring_axis_wild(1e6, 1e4) and not X.ring_axis_wild(1e6, 1e2)
    assert X.ring_box_class((8, 8, 8), 1.0, (0, 0, 0), (1, 1, 1), 0.5) == "unfolded" and X.ring_box_class((8, 8, 8), 1.0, (0, 0, 0), (5, 1, 1), 0.5) == "folded"
    assert X.ring_box_class((8, 8, 8), 1.0, (0, 0, 0), (1, 1, 1), np.inf) == "wild" and X.ring_box_class((8, 8, 8), 1.0, (0, 0, 0), (1, 2e9, 1), 0.5) == "wild"
    assert X.ring_geometry((8.0, 8.0, 8.0), 4000, 2.0) == ((8, 8, 8), 2.0)


def test_polyhedron_model_on_a_row_of_duplicates():
    """both ends on two equal rows: d2 == 0 for both, and the plane of a point on the segment is (0, 0, 0, -1)"""
    case = next(c for c in CASES if c.name == "far/n=30000/ext=10")
    sc = X.derive(case)
    q = sc.rows("rows")[0]
    assert np.array_equal(sc.segments[q, :3], sc.segments[q, 3:])
    off, idx, d2, s, planes = PM.segment_polyhedron(case.pts, sc.segments[q:q + 1], 1e-3)
    assert off[1] >= 1 and d2[0] == 0 and np.array_equal(planes[0], [0.0, 0.0, 0.0, -1.0])
    i, j = X.first_equal_rows(case.pts)
    assert idx[0] == i, "the lower of the two equal rows comes first"
