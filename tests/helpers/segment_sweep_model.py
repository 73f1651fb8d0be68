"""numpy restatement of the segment-sweep contract (include/pct_engine.h, paragraph "Segment sweeps").

A sweep is a segment a -> b and a radius r.  e, L2, w, dot, s and d2 are those of segment_model (the paragraph "Segment queries");
r2 = min(r*r, DBL_MAX); a row is a blocker iff d2 is finite and d2 <= r2.  Its entry parameter, elementwise fp64 in this order:

    ww = (w0*w0 + w1*w1) + w2*w2
    if ww <= r2: t = 0
    else:        g = ww - r2 ; disc = dot*dot - L2*g ; if (!(disc > 0)) disc = 0
                 t = (dot - sqrt(disc)) / L2 ; if (!(t > 0)) t = 0 ; else if (t > s) t = s

The winner is the blocker with the smallest t, the lowest index on ties.  No blocker: (NO_INDEX, 1).  An invalid sweep (a non-finite
endpoint after the narrowing, a NaN or negative radius): (NO_INDEX, NaN)."""
import numpy as np

import segment_model as M

NO_INDEX = M.NO_INDEX


def pair_entry(pts, a, b, r2):
    """(blocker mask, t, s) of every row of pts against ONE sweep (a, b: 3 widened doubles; r2 from segment_model.reach2)"""
    p = np.asarray(pts, np.float32).astype(np.float64).reshape(-1, 3)
    d2, s = M.pair_d2_s(p, a, b)
    with np.errstate(all="ignore"):
        e = b - a
        L2 = (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]
        w0, w1, w2 = p[:, 0] - a[0], p[:, 1] - a[1], p[:, 2] - a[2]
        dot = (w0 * e[0] + w1 * e[1]) + w2 * e[2]
        blocker = np.isfinite(d2) & (d2 <= r2)
        ww = (w0 * w0 + w1 * w1) + w2 * w2
        g = ww - r2
        disc = dot * dot - L2 * g
        disc = np.where(disc > 0, disc, 0.0)
        t = (dot - np.sqrt(disc)) / L2
        t = np.where(t > 0, np.where(t > s, s, t), 0.0)
        t = np.where(ww <= r2, 0.0, t)
    return blocker, t, s


def valid(a, b, radius):
    """is the sweep valid, and its r2"""
    r2 = M.reach2(radius)
    ok = r2 is not None and bool(np.all(np.isfinite(a)) and np.all(np.isfinite(b)))
    return ok, r2


def segment_sweep_boxed(pts, segments, radius, index_base=0):
    """segment_sweep for large batches, the same answers with fewer rows judged per sweep (checked against segment_sweep in
    tests/test_segment_sweep_model.py):
      * when some row has ww <= r2, the model is asked about the rows up to the first such row only; if it answers t = 0 there, no
        later row can do better (t >= 0, and the lower index wins a tie);
      * otherwise, for a finite radius, about the rows of the segment's bounding box grown by r + 0.01 only: a row outside that box
        is farther than r + 0.01 from the segment, six orders of magnitude beyond the rounding of d2 for coordinates below 1e4, so
        it blocks nothing; the rows keep their order, so ties fall the same way."""
    pts = np.asarray(pts, np.float32).reshape(-1, 3)
    a, b = M.narrow(segments)
    Q = len(a)
    radius = np.broadcast_to(np.asarray(radius, np.float64), (Q,))
    idx = np.full(Q, NO_INDEX, np.uint32)
    to = np.ones(Q)
    x, y, z = (np.ascontiguousarray(pts[:, k], np.float64) for k in range(3))
    for q in range(Q):
        ok, r2 = valid(a[q], b[q], radius[q])
        if not ok:
            to[q] = np.nan
            continue
        seg = np.concatenate([a[q], b[q]])[None, :]
        with np.errstate(all="ignore"):
            w0, w1, w2 = x - a[q, 0], y - a[q, 1], z - a[q, 2]
            touching = np.flatnonzero((w0 * w0 + w1 * w1) + w2 * w2 <= r2)
            lo, hi = np.minimum(a[q], b[q]) - (radius[q] + 0.01), np.maximum(a[q], b[q]) + (radius[q] + 0.01)
            inside = (x >= lo[0]) & (x <= hi[0]) & (y >= lo[1]) & (y <= hi[1]) & (z >= lo[2]) & (z <= hi[2])
        if len(touching):
            i, t = segment_sweep(pts[:touching[0] + 1], seg, radius[q])
            if i[0] != NO_INDEX and t[0] == 0.0:
                idx[q], to[q] = i[0] + index_base, 0.0
                continue
        rows = np.flatnonzero(inside) if np.isfinite(radius[q]) else np.arange(len(pts))
        i, t = segment_sweep(pts[rows], seg, radius[q])
        if i[0] != NO_INDEX:
            idx[q], to[q] = rows[i[0]] + index_base, t[0]
    return idx, to


def segment_sweep(pts, segments, radius, index_base=0):
    """(idx uint32 [Q], t [Q]) of the contract, by brute force"""
    a, b = M.narrow(segments)
    Q = len(a)
    radius = np.broadcast_to(np.asarray(radius, np.float64), (Q,))
    idx = np.full(Q, NO_INDEX, np.uint32)
    to = np.ones(Q)
    pts = np.asarray(pts, np.float32).reshape(-1, 3)
    for q in range(Q):
        ok, r2 = valid(a[q], b[q], radius[q])
        if not ok:
            to[q] = np.nan
            continue
        if len(pts) == 0:
            continue
        blocker, t, _ = pair_entry(pts, a[q], b[q], r2)
        if not blocker.any():
            continue
        i = int(np.argmin(np.where(blocker, t, np.inf)))            # argmin: the first, i.e. the lowest index, of equal minima
        idx[q], to[q] = i + index_base, t[i]
    return idx, to
