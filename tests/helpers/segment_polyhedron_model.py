"""numpy restatement of the free-space polyhedra (include/pct_engine.h, paragraph "Free-space polyhedra"), on top of
segment_search_model.

Row i of the capsule search in distance order (d2, then index) is walked in that order; an entry is a SUPPORT iff no earlier support
of the row cuts it.  Elementwise fp64 in the contract's order -- numpy's separate operations do not fuse, `/` and sqrt are correctly
rounded:

    support p:   n_k = w_k - s*e_k            (w, s, e of "Segment queries": segment_model.pair_d2_s's)
    entry x:     u_k = x_k - p_k              h = (n0*u0 + n1*u1) + n2*u2          cut iff h >= 0
    plane:       d = sqrt(d2)   nh_k = n_k / d   off = (nh0*p0 + nh1*p1) + nh2*p2   ;   (0, 0, 0, -1) when d2 == 0"""
import numpy as np

import segment_model as M
import segment_search_model as SS


def normals(p, a, b, s):
    """n of rows p [m, 3] (widened) with their parameters s [m] on the segment (a, b)"""
    e = b - a
    return np.stack([(p[:, k] - a[k]) - s * e[k] for k in range(3)], axis=1)


def filter_row(p, n):
    """positions of the supports of ONE row: p [m, 3] the widened rows in distance order, n [m, 3] their normals"""
    m = len(p)
    alive = np.ones(m, bool)
    keep = []
    k = 0
    while k < m:
        keep.append(k)
        u0, u1, u2 = p[k + 1:, 0] - p[k, 0], p[k + 1:, 1] - p[k, 1], p[k + 1:, 2] - p[k, 2]
        h = (n[k, 0] * u0 + n[k, 1] * u1) + n[k, 2] * u2
        alive[k + 1:] &= ~(h >= 0)
        nxt = np.flatnonzero(alive[k + 1:])
        k = k + 1 + int(nxt[0]) if len(nxt) else m
    return np.array(keep, np.int64)


def planes_of(p, n, d2):
    """[m, 4]: nh0 nh1 nh2 off"""
    out = np.zeros((len(p), 4))
    with np.errstate(all="ignore"):
        d = np.sqrt(d2)
        nh = n / d[:, None]
        off = (nh[:, 0] * p[:, 0] + nh[:, 1] * p[:, 1]) + nh[:, 2] * p[:, 2]
    out[:, :3], out[:, 3] = nh, off
    out[d2 == 0] = [0.0, 0.0, 0.0, -1.0]
    return out


def from_rows(pts, segments, rows, index_base=0):
    """the supports of capsule rows `rows` = (offsets, idx, d2, s) in ORDER_DISTANCE (segment_search_model's, idx with index_base):
    (offsets int64 [Q + 1], idx uint32, d2, s, planes [total, 4])"""
    off, idx, d2, s = rows
    a, b = M.narrow(segments)
    p_all = np.asarray(pts, np.float32).reshape(-1, 3).astype(np.float64)
    offsets = np.zeros(len(off), np.int64)
    oi, od, os_, op = [], [], [], []
    for q in range(len(off) - 1):
        lo, hi = int(off[q]), int(off[q + 1])
        loc = idx[lo:hi].astype(np.int64) - index_base
        p = p_all[loc]
        n = normals(p, a[q], b[q], s[lo:hi])
        keep = filter_row(p, n)
        offsets[q + 1] = offsets[q] + len(keep)
        oi.append(idx[lo:hi][keep])
        od.append(d2[lo:hi][keep])
        os_.append(s[lo:hi][keep])
        op.append(planes_of(p[keep], n[keep], d2[lo:hi][keep]))
    cat = lambda v, dt, shape: np.concatenate(v).astype(dt) if v else np.zeros(shape, dt)      # noqa: E731
    return offsets, cat(oi, np.uint32, 0), cat(od, np.float64, 0), cat(os_, np.float64, 0), cat(op, np.float64, (0, 4)).reshape(-1, 4)


def segment_polyhedron(pts, segments, reach, index_base=0):
    """(offsets int64 [Q + 1], idx uint32 [total], d2 [total], s [total], planes [total, 4]) of the contract, by brute force"""
    return from_rows(pts, segments, SS.segment_search(pts, segments, reach, SS.ORDER_DISTANCE, index_base), index_base)
