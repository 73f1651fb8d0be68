"""numpy restatement of the capsule search (include/pct_engine.h, paragraph "Capsule search"), on top of segment_model.

Row i lists every row of pts that is a candidate of segment i under reach[i] in the sense of "Segment queries": the ends narrowed to
fp32, d2 and s from segment_model.pair_d2_s, a candidate iff d2 <= min(reach*reach, DBL_MAX) (a NaN d2 compares false, an infinite one
exceeds DBL_MAX).  A non-finite end, a NaN reach and a negative reach give an empty row.  Rows in ascending index (order 0) or by
(d2, index) (order 1)."""
import numpy as np

import segment_model as M

ORDER_INDEX, ORDER_DISTANCE = 0, 1


def row_masks(pts, segments, reach):
    """per segment: (d2 [N], s [N], hit mask [N])"""
    a, b = M.narrow(segments)
    Q = len(a)
    reach = np.broadcast_to(np.asarray(reach, np.float64), (Q,))
    pts = np.asarray(pts, np.float32).reshape(-1, 3)
    out = []
    for q in range(Q):
        r2 = M.reach2(reach[q])
        if len(pts) == 0 or r2 is None or not (np.all(np.isfinite(a[q])) and np.all(np.isfinite(b[q]))):
            out.append((np.zeros(len(pts)), np.zeros(len(pts)), np.zeros(len(pts), bool)))
            continue
        d2, s = M.pair_d2_s(pts, a[q], b[q])
        with np.errstate(invalid="ignore"):
            out.append((d2, s, d2 <= r2))
    return out


def rows_from(masks, order, index_base=0):
    offsets = np.zeros(len(masks) + 1, np.int64)
    idx, d2, s = [], [], []
    for i, (d, t, hit) in enumerate(masks):
        ids = np.nonzero(hit)[0]                             # ascending index
        if order == ORDER_DISTANCE:
            ids = ids[np.lexsort((ids, d[ids]))]             # nearest first, equal d2 in ascending index
        offsets[i + 1] = offsets[i] + len(ids)
        idx.append(ids)
        d2.append(d[ids])
        s.append(t[ids])
    cat = lambda v, dt: np.concatenate(v).astype(dt) if v else np.zeros(0, dt)      # noqa: E731
    return offsets, (cat(idx, np.int64) + index_base).astype(np.uint32), cat(d2, np.float64), cat(s, np.float64)


def segment_search(pts, segments, reach, order, index_base=0):
    """(offsets int64 [Q + 1], idx uint32 [total], d2 float64 [total], s float64 [total]) of the contract, by brute force"""
    return rows_from(row_masks(pts, segments, reach), order, index_base)


def segment_count(pts, segments, reach):
    return np.array([int(hit.sum()) for _, _, hit in row_masks(pts, segments, reach)], np.uint32)


def segment_search_boxed(pts, segments, reach, order, index_base=0):
    """the same lists for large batches of short reaches: per segment only the rows inside the capsule's bounding box, widened by 1e-3 of
    its scale, are measured -- a row outside it is farther than reach from every point of the segment, by far more than the rounding of
    d2.  A segment whose reach is not finite, or whose row would be empty by rule, takes the plain route.  (tests/test_segment_search_model.py
    checks this against segment_search itself.)"""
    a, b = M.narrow(segments)
    Q = len(a)
    reach = np.broadcast_to(np.asarray(reach, np.float64), (Q,))
    p32 = np.asarray(pts, np.float32).reshape(-1, 3)
    p = p32.astype(np.float64)
    masks = []
    for q in range(Q):
        r = reach[q]
        if len(p) == 0 or not (np.isfinite(r) and r >= 0 and np.all(np.isfinite(a[q])) and np.all(np.isfinite(b[q]))):
            masks.extend(row_masks(p32, np.concatenate([a[q], b[q]])[None], r))
            continue
        lo, hi = np.minimum(a[q], b[q]), np.maximum(a[q], b[q])
        pad = r + 1e-3 * (r + np.abs(lo).max() + np.abs(hi).max() + 1.0)
        with np.errstate(invalid="ignore"):
            inside = np.nonzero(np.all((p >= lo - pad) & (p <= hi + pad), axis=1))[0]
        d2 = np.zeros(len(p))
        s = np.zeros(len(p))
        hit = np.zeros(len(p), bool)
        if len(inside):
            dd, ss = M.pair_d2_s(p32[inside], a[q], b[q])
            d2[inside], s[inside] = dd, ss
            with np.errstate(invalid="ignore"):
                hit[inside] = dd <= M.reach2(r)
        masks.append((d2, s, hit))
    return rows_from(masks, order, index_base)
