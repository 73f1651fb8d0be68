"""Segments, reaches and radii at the edges of the fp32 range, derived from the (cloud, queries, radii) cases of
tests/test_numeric_edges.py: the shared generator of tests/test_segment_edges_model.py (CPU: what "right" means) and
tests/test_gpu_segment_edges.py (the engine against it).  Pure numpy with fixed seeds; the engine is not imported.

derive(case) gives a SegCase: segments [Q, 6] fp64 (a then b), reach [Q] fp64, tags [Q] (the group of every row), and beside them the
derived reaches and radii described on the class.  Groups:

    pairs       consecutive queries (q[i], q[i + 1]): on the far and sentinel families from inside the cloud to 1e18 .. FLT_MAX away
    degenerate  a == b for the first queries: the point queries
    spans       from the first query to each of the last six
    rows        both ends exactly on cloud rows, among them two equal rows (d2 == 0, ww == 0, the plane (0, 0, 0, -1))
    dup-ties    a short axis-parallel segment beside a duplicated row, nearer to it than to anything else: two (or more) rows at
                one exact d2 > 0, the lower index wins
    lattice     (ladder, tiny/extent-1e-30) axis-parallel, half-way between two rows of the dyadic lattice, through the case's `mid`
                queries: every operand exact, both rows at one exact d2 from an interior point of the segment
    range       (sentinels, ladder rungs at 1e38) -FLT_MAX -> +FLT_MAX along x, the full diagonal, and e = 2 FLT_MAX on one axis with
                a subnormal e on another
    zeros       (tiny/subnormal) ends of either zero sign, e of one or two multiples of 2^-149
"""
import functools
import os
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (_HERE, os.path.dirname(_HERE)):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import segment_model as M  # noqa: E402
import segment_search_model as SS  # noqa: E402
import segment_sweep_model as W  # noqa: E402
import test_numeric_edges as NE  # noqa: E402
from test_numeric_edges import CASES, NONFINITE_ROW_CASES, FLT_MAX, SPECIAL_RADII  # noqa: E402,F401

F = float(FLT_MAX)
U = 2.0 ** -149                      # the smallest fp32 subnormal
KS = (1.0 - 2.0 ** -50, 1.0, 1.0 + 2.0 ** -50, 1.5)
SPECIAL_REACHES = np.float64([0.0, 1e-320, 1e-200, 1e-42, 1e19, F, 1e39, 1e154, 1.4e154, 1e200, np.inf, np.nan, -1.5, -np.inf])
N_SPECIAL_SEGMENTS = 5


class SegCase:
    """segments, reach, tags: see the module.  Further, all [Q] unless said otherwise:
    nn_inf        the model's (idx, d2, s) under reach = +inf
    reach_k       {k: reach} for k in KS: the boundary reach of the unbounded winner times k.  The boundary reach is the least double
                  r >= fl(sqrt(d2_nn)) with fl(r * r) >= d2_nn (sqrt rounds either way, so fl(sqrt(d2))^2 can fall an ulp short): the
                  winner is in under k = 1 and 1 + 2^-50, out under 1 - 2^-50, at every magnitude
    sweep_radius  reach, but on a third of the pairs and spans 0.75 x the distance from a to its nearest row (where positive): those
                  sweeps start free
    special_segments [5 * len(SPECIAL_REACHES), 6], special_reach: the first five segments under every special reach"""

    def __init__(self, case, segments, reach, tags):
        self.case, self.segments, self.reach, self.tags = case, segments, reach, tags

    def __iter__(self):
        return iter((self.segments, self.reach, self.tags))

    def rows(self, tag):
        return np.flatnonzero(self.tags == tag)


def _seg(a, b):
    return np.concatenate([np.asarray(a, np.float64).reshape(-1, 3), np.asarray(b, np.float64).reshape(-1, 3)], axis=1)


def first_equal_rows(pts):
    """(i, j), i < j, the first two equal rows of the cloud (-0.0 == 0.0), or None"""
    _, inv, cnt = np.unique(pts, axis=0, return_inverse=True, return_counts=True)
    inv = np.asarray(inv).reshape(-1)
    dup = np.flatnonzero(cnt[inv] > 1)
    if not len(dup):
        return None
    i = int(dup[0])
    j = int(np.flatnonzero(inv == inv[i])[1])
    return i, j


def _dup_tie_segments(pts):
    """beside the first duplicated row p: an axis-parallel segment of half-length d / 4 centred d / 4 off p along x, d the distance
    from p to the nearest DIFFERENT row -- every other row is then farther from the segment than p and its twin"""
    ij = first_equal_rows(pts)
    if ij is None:
        return np.zeros((0, 6))
    p = pts[ij[0]].astype(np.float64)
    d2 = NE.numpy_d2(pts, pts[ij[0]:ij[0] + 1])[0]
    d2 = d2[d2 > 0]
    if not len(d2):
        return np.zeros((0, 6))
    q = np.float64(np.float32(np.sqrt(d2.min()) / 4.0))
    out = []
    for axis in (1, 2):
        c = p.copy()
        c[0] = np.float64(np.float32(c[0] + q if abs(c[0] + q) <= F else c[0] - q))
        a, b = c.copy(), c.copy()
        a[axis] = np.float64(np.float32(max(c[axis] - q, -F)))
        b[axis] = np.float64(np.float32(min(c[axis] + q, F)))
        out.append(np.concatenate([a, b]))
    return np.array(out)


def _lattice_segments(case):
    """through the case's mid queries (numerators 8 mod 16 along x: half-way between two dyadic rows), parallel to y and to z, a
    quarter of the lattice step to either side: all operands are small integers times the 12-bit scale"""
    if case.family == "ladder":
        n0 = case.meta["n_inside"] + 8
        mid = case.queries[n0:n0 + 4].astype(np.float64)
        step = float(NE._scale12(case.meta["scale"])) / 64.0
    elif case.name == "tiny/extent-1e-30":
        mid = case.queries[-3:].astype(np.float64)
        step = float(NE._scale12(1e-30)) / 64.0
    else:
        return np.zeros((0, 6))
    out = []
    for k, m in enumerate(mid):
        axis = 1 + k % 2
        a, b = m.copy(), m.copy()
        a[axis] -= 4.0 * step
        b[axis] += 4.0 * step
        assert np.all(np.float32(a) == a) and np.all(np.float32(b) == b), "lattice-tie ends must be exact in fp32"
        out.append(np.concatenate([a, b]))
    return np.array(out)


def lattice_step(case):
    return float(NE._scale12(case.meta["scale"] if case.family == "ladder" else 1e-30)) / 64.0


def dyadic_rows(case):
    """index range of the dyadic lattice rows of a ladder / tiny case"""
    if case.family == "ladder":
        return 30_000 + 512, 30_000 + 512 + 125
    return 2000, 2000 + 125


def _range_segments(case):
    q0 = case.queries[0].astype(np.float64)
    return np.array([[-F, q0[1], q0[2], F, q0[1], q0[2]],
                     [-F, -F, -F, F, F, F],
                     [-F, 0.0, q0[2], F, 3.0 * U, q0[2]],
                     [q0[0], F, -U, q0[0] + 0.0, -F, U]])


def _zero_segments(case):
    q = case.queries.astype(np.float64)
    z, nz = 0.0, -0.0
    return np.array([[z, z, z, nz, nz, nz],
                     [nz, z, nz, z, nz, z],
                     [nz, nz, nz, 5 * U, -3 * U, nz],
                     np.concatenate([q[0], q[0] + [U, 0, 0]]),
                     np.concatenate([q[1], q[1] + [2 * U, -U, 0]]),
                     np.concatenate([q[2], q[2] + [0, 0, -2 * U]])])


def boundary_reach(d2):
    """the least double r >= fl(sqrt(d2)) with fl(r * r) >= d2"""
    r = np.sqrt(np.asarray(d2, np.float64))
    for _ in range(4):
        r = np.where(r * r < d2, np.nextafter(r, np.inf), r)
    assert np.all((r * r >= d2) | ~np.isfinite(d2))
    return r


@functools.lru_cache(maxsize=None)
def _derive(name):
    case = next(c for c in CASES + NONFINITE_ROW_CASES if c.name == name)
    rng = np.random.default_rng(31_000 + sum(map(ord, name)))
    q = case.queries.astype(np.float64)
    pts = case.pts
    n = len(q)
    groups = []
    i = np.arange(n - 1)
    if len(i) > 56:                              # the radii family repeats every query once per radius: the changes and every 5th
        i = i[np.any(q[:-1] != q[1:], axis=1) | (i % 5 == 0)]
    groups.append(("pairs", _seg(q[i], q[i + 1])))
    groups.append(("degenerate", _seg(q[:6], q[:6])))
    last = q[::-1][:min(n, 6)]
    groups.append(("spans", _seg(np.repeat(q[:1], len(last), 0), last)))
    r = rng.integers(0, len(pts), (4, 2))
    rows = _seg(pts[r[:, 0]], pts[r[:, 1]])
    ij = first_equal_rows(pts[np.all(np.isfinite(pts), axis=1)]) if case.family != "nonfinite-rows" else None
    if ij is not None:
        rows = np.concatenate([_seg(pts[ij[0]], pts[ij[1]]), _seg(pts[ij[1]], pts[r[0, 0]]), rows])
    else:
        rows = np.concatenate([_seg(pts[0], pts[0]), rows])
    if case.family == "nonfinite-rows":          # the ends of a segment must be finite: a bad row gives way to row 0
        rows = np.where(np.isfinite(rows), rows, 4.5)
    groups.append(("rows", rows))
    if case.family != "nonfinite-rows":
        groups.append(("dup-ties", _dup_tie_segments(pts)))
        groups.append(("lattice", _lattice_segments(case)))
    if case.family == "sentinels" or (case.family == "ladder" and case.meta["scale"] == 1e38):
        groups.append(("range", _range_segments(case)))
    if case.name.startswith("tiny/subnormal"):
        groups.append(("zeros", _zero_segments(case)))
    groups = [(t, g) for t, g in groups if len(g)]
    segments = np.ascontiguousarray(np.concatenate([g for _, g in groups]))
    tags = np.concatenate([np.full(len(g), t, dtype="U12") for t, g in groups])
    Q = len(segments)
    assert np.all(np.abs(segments) <= F), "a derived end left the fp32 range"
    assert np.array_equal(segments.astype(np.float32).astype(np.float64), segments), "every derived end is an fp32 value"

    rad = np.abs(case.radii.astype(np.float64))
    fin = rad[np.isfinite(rad)]
    rad = np.where(np.isfinite(rad), rad, np.median(fin) if len(fin) else 1.0)
    sc = SegCase(case, segments, np.resize(rad, Q).astype(np.float64), tags)
    sc.nn_inf = M.segment_nn(pts, segments, np.inf)
    d2 = sc.nn_inf[1]
    found = sc.nn_inf[0] != M.NO_INDEX
    rb = np.where(found, boundary_reach(np.where(found, d2, 0.0)), 0.0)
    sc.reach_k = {k: rb * k for k in KS}
    # 0.75 x the distance from a to its nearest row, on a third of the pairs and spans
    start = M.segment_nn(pts, _seg(segments[:, :3], segments[:, :3]), np.inf)[1]
    ps = np.isin(tags, ("pairs", "spans"))
    third = ps & ((np.cumsum(ps) - 1) % 3 == 2) & (start > 0) & np.isfinite(start)
    sc.sweep_radius = np.where(third, 0.75 * np.sqrt(np.where(third, start, 0.0)), sc.reach)
    ns = min(N_SPECIAL_SEGMENTS, Q)
    sc.special_segments = np.ascontiguousarray(np.repeat(segments[:ns], len(SPECIAL_REACHES), axis=0))
    sc.special_reach = np.tile(SPECIAL_REACHES, ns)
    sc.special_nn_inf = tuple(np.repeat(v[:ns], len(SPECIAL_REACHES)) for v in sc.nn_inf)
    return sc


def derive(case):
    return _derive(case.name)


def reach_sets(sc):
    """[(label, segments, reach, unbounded model answer)] every set of reaches a segment call is run under"""
    out = [("per-segment reach", sc.segments, sc.reach, sc.nn_inf), ("reach = +inf", sc.segments, np.full(len(sc.reach), np.inf), sc.nn_inf)]
    out += [(f"reach = boundary x {k!r}", sc.segments, sc.reach_k[k], sc.nn_inf) for k in KS]
    out.append(("special reaches", sc.special_segments, sc.special_reach, sc.special_nn_inf))
    return out


@functools.lru_cache(maxsize=None)
def _masks(name, which):
    sc = _derive(name)
    _, segs, reach, _ = reach_sets(sc)[which]
    return SS.row_masks(sc.case.pts, segs, reach)


def masks(sc, which):
    """segment_search_model.row_masks of reach set `which` (an index into reach_sets), cached"""
    return _masks(sc.case.name, which)


def capped(pts, segments, reach, cap=64):
    """(segments, reach, kept) for the polyhedra: reaches of 0 and +inf (and invalid ones) are left out, and a reach whose row would
    hold more than `cap` entries is shrunk to just below the (cap + 1)-th smallest candidate d2 of the model -- strictly: the next
    double below its square root whose square is below that d2.  The sequential support filter is what makes long rows slow."""
    a, b = M.narrow(segments)
    reach = np.broadcast_to(np.asarray(reach, np.float64), (len(a),)).copy()
    keep = []
    for q in range(len(a)):
        r2 = M.reach2(reach[q])
        if r2 is None or reach[q] == 0 or not np.isfinite(reach[q]):
            continue
        d2, _ = M.pair_d2_s(pts, a[q], b[q])
        with np.errstate(invalid="ignore"):
            cand = np.sort(d2[d2 <= r2])
        if len(cand) > cap:
            cut = cand[cap]
            if cut == 0:
                continue                                    # more than cap rows ON the segment: no positive reach holds fewer
            r = np.nextafter(np.sqrt(cut), 0.0)
            while not r * r < cut:
                r = np.nextafter(r, 0.0)
            if r == 0:
                continue
            reach[q] = r
        keep.append(q)
    keep = np.array(keep, np.int64)
    return np.ascontiguousarray(np.asarray(segments, np.float64).reshape(-1, 6)[keep]), reach[keep], keep


# ---- the chain's intermediates (for the family conditions: nothing non-finite / subnormal on the way) ------------------------------

def intermediates(pts, a, b, r2):
    """every intermediate of segment_model.pair_d2_s and segment_sweep_model.pair_entry for ONE segment, by name"""
    p = np.asarray(pts, np.float32).astype(np.float64).reshape(-1, 3)
    with np.errstate(all="ignore"):
        e = b - a
        ee = [e[k] * e[k] for k in range(3)]
        L2 = (ee[0] + ee[1]) + ee[2]
        w = [p[:, k] - a[k] for k in range(3)]
        we = [w[k] * e[k] for k in range(3)]
        dot = (we[0] + we[1]) + we[2]
        s = np.zeros_like(dot) if L2 == 0 else dot / L2
        s = np.where(s > 0, np.where(s > 1, 1.0, s), 0.0)
        se = [s * e[k] for k in range(3)]
        c = [w[k] - se[k] for k in range(3)]
        cc = [c[k] * c[k] for k in range(3)]
        d2 = (cc[0] + cc[1]) + cc[2]
        wk = [w[k] * w[k] for k in range(3)]
        ww = (wk[0] + wk[1]) + wk[2]
        g = ww - r2
        dd, Lg = dot * dot, L2 * g
        disc = dd - Lg
    out = dict(e=e, L2=np.float64(L2), dot=dot, s=s, d2=d2, ww=ww, g=g, dd=dd, Lg=Lg, disc=disc)
    for k in range(3):
        out.update({f"ee{k}": np.float64(ee[k]), f"w{k}": w[k], f"we{k}": we[k], f"se{k}": se[k], f"c{k}": c[k], f"cc{k}": cc[k], f"wk{k}": wk[k]})
    return out


# ---- the engine's boxes and guards, restated on the host (for choosing and asserting cases only) -----------------------------------

GUARD_CELLS = 2.0 ** 30             # segment_search.hpp kSsGuardCells
RING_CELL_CLAMP = 1e9               # ring.hpp kRingCellClamp


def guard_inside(origin, dims, h, a, b, reach):
    """ss_grid_box's B.skip: the per-cell skip applies (origin, the ends' offsets from it, the grid's far side and the reach all under
    2^30 cells)"""
    h = float(h)
    lim = GUARD_CELLS * h
    ok = float(reach) < lim
    for k in range(3):
        o = float(origin[k])
        ok = ok and abs(o) + float(dims[k]) * h < lim and abs(float(a[k]) - o) < lim and abs(float(b[k]) - o) < lim
    return bool(ok)


def guard_class(origin, dims, h, a, b, reach):
    """'inside' (with an interior cell in the box), 'inside-border' (without), 'reach' (outside by the reach), 'end' (by an end or
    the grid itself)"""
    h = float(h)
    if not guard_inside(origin, dims, h, a, b, reach):
        return "reach" if not float(reach) < GUARD_CELLS * h else "end"
    for k in range(3):
        lo = (min(a[k], b[k]) - reach - origin[k]) / h
        hi = (max(a[k], b[k]) + reach - origin[k]) / h
        c0, c1 = max(int(np.floor(max(lo, 0.0))), 1), min(int(np.floor(min(hi, dims[k]))), int(dims[k]) - 2)
        if c1 < c0:
            return "inside-border"
    return "inside"


def ring_axis_wild(v, inv_h):
    """ring_cell_coord's clamp: the coordinate's cell is NaN, infinite or beyond 1e9 cells"""
    with np.errstate(all="ignore"):
        c = np.floor(np.float64(v) * np.float64(inv_h))
    return not (c > -RING_CELL_CLAMP and c < RING_CELL_CLAMP)


def ring_box_class(dims, h, a, b, reach):
    """seg_capsule_box: 'wild' (an end of an axis' span is wild), 'folded' (a span reaches the table size), 'unfolded'"""
    inv_h = 1.0 / float(h)
    folded = False
    with np.errstate(all="ignore"):
        for k in range(3):
            lo, hi = np.float64(min(a[k], b[k])) - reach, np.float64(max(a[k], b[k])) + reach
            if ring_axis_wild(lo, inv_h) or ring_axis_wild(hi, inv_h):
                return "wild"
            if np.floor(hi * inv_h) - np.floor(lo * inv_h) + 3 >= dims[k]:
                folded = True
    return "folded" if folded else "unfolded"


def _pow2_at_least(v):
    g = 1
    while g < v:
        g *= 2
    return g


def ring_geometry(ext, cap, cell=0.0):
    """(dims, h) as ring_configure sizes the table from an extent, the cloud's capacity and a requested cell size"""
    ext = np.asarray(ext, np.float64)
    diag = max(float(ext.max()), 1e-6)
    ext = np.maximum(ext, diag * 1e-3)
    h = float(cell)
    if not h > 0:
        h = float(np.cbrt(np.prod(ext) * 6.0 / max(int(cap), 1)))
    if not (h > 0 and np.isfinite(h)):
        h = 1.0
    while True:
        with np.errstate(all="ignore"):
            g = [_pow2_at_least(max(4, int(min(np.ceil(1.25 * ext[k] / h), 2.0 ** 40)) + 2)) for k in range(3)]
        if g[0] * g[1] * g[2] <= 1 << 24:
            return tuple(g), h
        h *= 1.26


def grid_geometry(pts, cell=0.0):
    """(origin, dims, h) of the cell index as pct_cloud_build_grid sizes it: origin = the cloud's minimum; about 6 points a cell when
    no cell size is given; at least 1/1023 of the largest extent; a cell size between 2^-120 and 2^120, narrowed to fp32; at most 1024
    cells an axis, and no cell that begins beyond 3.4e38 (the GPU test reads the engine's own from grid_info())"""
    lo, hi = pts.min(0).astype(np.float64), pts.max(0).astype(np.float64)
    ext = np.maximum(hi - lo, 0.0)
    h = float(np.float32(cell))
    if not h > 0:
        d = max(float(ext.max()), 1e-6)
        h = float(np.cbrt(np.prod(np.maximum(ext, d * 1e-3)) * 6.0 / len(pts)))
    h = max(h, float(ext.max()) / 1023.0)
    if not h > 0:
        h = 1.0
    h = float(np.float32(min(max(h, 2.0 ** -120), 2.0 ** 120)))
    gmax = int(min(1024.0, np.floor(3.4e38 / h) + 1.0))
    dims = tuple(max(1, min(gmax, int(min(1024.0, np.floor(e / h))) + 1)) for e in ext)
    return lo, dims, h


def explicit_cell(pts):
    """tests/test_gpu_numeric_edges.explicit_cell: a tenth of the largest extent (fp32), whatever the magnitude"""
    ext = float((pts.max(0).astype(np.float64) - pts.min(0).astype(np.float64)).max())
    h = np.float32(min(max(ext / 10.0, 1e-44), 3e38))
    return float(h) if h > 0 else 1.0


def body_extent(pts):
    """(lo, extent) of the rows that are not sentinels: those within 100 x the median magnitude"""
    m = np.abs(pts.astype(np.float64)).max(axis=1)
    body = pts[m <= 100.0 * max(float(np.median(m)), 1e-300)].astype(np.float64)
    return body.min(0), np.maximum(body.max(0) - body.min(0), 1e-30)


def ring_extent(pts):
    """the extent tests/test_gpu_numeric_edges.test_nn_rolling_map_index hands to ring_index"""
    ext = np.maximum(pts.max(0).astype(np.float64) - pts.min(0).astype(np.float64), 1e-30)
    return np.minimum(ext, 3e38).astype(np.float32)


def small_table(case):
    """(cell size, extent) of a table much smaller than the cloud -- a tenth of the body's extent a cell, four cells an axis -- for the
    cases that take one: the ladder, the far/ext=10 clouds of at least 17 rows, the sentinels; None otherwise"""
    big = case.family == "ladder" or case.family == "sentinels" or (case.family == "far" and 17 <= len(case.pts) <= 30_000)
    if not big:
        return None
    _, ext = body_extent(case.pts)
    h = float(np.float32(min(float(ext.max()) / 10.0, 3e37)))
    return h, np.float32([4 * h] * 3)
