"""numpy restatement of the segment-query contract (include/pct_engine.h, paragraph "Segment queries").

Elementwise fp64 in the contract's order -- numpy's separate operations do not fuse, and its `/` and sqrt are correctly rounded:

    e_k = b_k - a_k            L2  = (e0*e0 + e1*e1) + e2*e2
    w_k = p_k - a_k            dot = (w0*e0 + w1*e1) + w2*e2
    s   = (L2 == 0) ? 0 : dot / L2 ;  if (!(s > 0)) s = 0 ; else if (s > 1) s = 1
    c_k = w_k - s*e_k          d2  = (c0*c0 + c1*c1) + c2*c2

A row is a candidate iff d2 is finite and d2 <= min(reach*reach, DBL_MAX); the winner is the best candidate by (d2, index).  The
endpoints are narrowed to fp32 first; a non-finite endpoint, a NaN reach and a negative reach give "no candidate"."""
import numpy as np

NO_INDEX = 0xFFFFFFFF
DBL_MAX = np.finfo(np.float64).max


def narrow(segments):
    """[Q, 6] fp64 -> the fp32-narrowed endpoints, widened again: (a [Q, 3], b [Q, 3])"""
    seg = np.asarray(segments, np.float64).reshape(-1, 6)
    with np.errstate(over="ignore", invalid="ignore"):
        f = seg.astype(np.float32).astype(np.float64)
    return f[:, :3], f[:, 3:]


def pair_d2_s(pts, a, b):
    """d2 and s of every row of pts ([N, 3] fp32) against ONE segment (a, b: 3 widened doubles)"""
    p = np.asarray(pts, np.float32).astype(np.float64).reshape(-1, 3)
    with np.errstate(all="ignore"):
        e = b - a
        L2 = (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]
        w0, w1, w2 = p[:, 0] - a[0], p[:, 1] - a[1], p[:, 2] - a[2]
        dot = (w0 * e[0] + w1 * e[1]) + w2 * e[2]
        s = np.zeros_like(dot) if L2 == 0 else dot / L2
        s = np.where(s > 0, np.where(s > 1, 1.0, s), 0.0)           # a NaN is not > 0
        c0, c1, c2 = w0 - s * e[0], w1 - s * e[1], w2 - s * e[2]
        d2 = (c0 * c0 + c1 * c1) + c2 * c2
    return d2, s


def reach2(reach):
    """the candidate bound of one reach, or None for "no candidate" (NaN or negative)"""
    r = np.float64(reach)
    if not r >= 0:
        return None
    with np.errstate(over="ignore"):
        return min(r * r, DBL_MAX)


def segment_nn(pts, segments, reach, index_base=0):
    """(idx uint32 [Q], d2 [Q], s [Q]) of the contract, by brute force"""
    a, b = narrow(segments)
    Q = len(a)
    reach = np.broadcast_to(np.asarray(reach, np.float64), (Q,))
    idx = np.full(Q, NO_INDEX, np.uint32)
    d2o = np.full(Q, np.inf)
    so = np.full(Q, np.nan)
    pts = np.asarray(pts, np.float32).reshape(-1, 3)
    if len(pts) == 0:
        return idx, d2o, so
    for q in range(Q):
        r2 = reach2(reach[q])
        if r2 is None or not (np.all(np.isfinite(a[q])) and np.all(np.isfinite(b[q]))):
            continue
        d2, s = pair_d2_s(pts, a[q], b[q])
        with np.errstate(invalid="ignore"):
            cand = np.isfinite(d2) & (d2 <= r2)
        if not cand.any():
            continue
        i = int(np.argmin(np.where(cand, d2, np.inf)))              # argmin: the first, i.e. the lowest index, of equal minima
        idx[q], d2o[q], so[q] = i + index_base, d2[i], s[i]
    return idx, d2o, so


def cut_at_reach(unbounded, segments, reach):
    """the answers under `reach` from those under reach = +inf: the best candidate of a smaller bound is the unbounded winner when it
    passes d2 <= r2 -- every row that passes is then a candidate of both -- and nobody otherwise (tests/test_segment_model.py checks
    this against segment_nn itself).  Lets a test share one brute-force pass among several reaches."""
    idx, d2, s = (np.array(v) for v in unbounded)
    a, b = narrow(segments)
    reach = np.broadcast_to(np.asarray(reach, np.float64), (len(idx),))
    for q in range(len(idx)):
        r2 = reach2(reach[q])
        if r2 is None or not d2[q] <= r2 or not (np.all(np.isfinite(a[q])) and np.all(np.isfinite(b[q]))):
            idx[q], d2[q], s[q] = NO_INDEX, np.inf, np.nan
    return idx, d2, s


def segment_inflate(pts, segments, search_margin, max_radius, index_base=0):
    """(radius [Q], idx [Q], s [Q]) of pct_segment_inflate_batch: the unbounded formula"""
    Q = len(np.asarray(segments, np.float64).reshape(-1, 6))
    if len(np.asarray(pts).reshape(-1, 3)) == 0:
        return np.full(Q, np.float64(max_radius) - np.float64(search_margin)), np.full(Q, NO_INDEX, np.uint32), np.full(Q, np.nan)
    idx, d2, s = segment_nn(pts, segments, np.inf, index_base)
    with np.errstate(invalid="ignore"):
        rr = np.sqrt(d2) - np.float64(search_margin)
        near = rr < np.float64(max_radius)
    radius = np.where(near, rr, np.float64(max_radius))
    return radius, np.where(near, idx, np.uint32(NO_INDEX)).astype(np.uint32), np.where(near, s, np.nan)
