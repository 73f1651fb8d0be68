"""numpy restatement of the window forms of the certified Bezier check and the trajectory clearance (include/pct_engine.h, paragraph
"Windows of a trajectory"), on top of bezier_certify_model and bezier_clearance_model.

Elementwise fp64 in the contract's order:

    t0 = t_start, t1 = t0 + horizon                                    INVALID: t0 not finite or < 0, horizon NaN or not > 0
    c = 0, cn = c + T_i, c = cn                                        segment i in the window iff t0 < cn and t1 > c
    u0 = 0 if t0 <= c else (t0 - c) / T_i                              u1 = 1 if t1 >= cn else (t1 - c) / T_i; dropped if not u0 < u1
    cut at t: q[i] = w * p[i] + t * p[i+1], w = 1 - t, level by level  left: first point of every level; right: last of every level, reversed
    restrict: cut at u1, keep left (if u1 < 1); cut at u0 / u1, keep right (if u0 > 0)
    u = (1 - v) * u0 + v * u1                                          the way back from a piece end v = (k + end) / 2^d to the segment

certify_window / clearance_window are the existing models run on the restricted polygons re-packed with seg_time = 1 (P = coef * 1 is
exact, so this IS the contract), hit_seg / at_seg and u mapped back.  Also here: the 3 m line of the README's case flown as three
cubic segments, with the windows of its table."""
import math

import numpy as np

import bezier_certify_model as CM
import bezier_clearance_model as KM

STRIDE = 39
RESTRICT_BOUND = 108 * 2.0 ** -53      # of M0: what the restated argument claims for a restricted polygon against the exact restriction


def window_valid(t0, horizon):
    t0, horizon = float(t0), float(horizon)
    return math.isfinite(t0) and t0 >= 0.0 and horizon > 0.0


def windows(T, t0, horizon):
    """[(u0, u1) or None per segment] of a trajectory with segment times T, or None when the window makes it INVALID"""
    if not window_valid(t0, horizon):
        return None
    t0 = float(t0)
    t1 = t0 + float(horizon)
    out, c = [], 0.0
    for Ti in T:
        Ti = float(Ti)
        cn = c + Ti
        w = None
        if t0 < cn and t1 > c:
            u0 = 0.0 if t0 <= c else (t0 - c) / Ti
            u1 = 1.0 if t1 >= cn else (t1 - c) / Ti
            if u0 < u1:
                w = (u0, u1)
        out.append(w)
        c = cn
    return out


def cut(P, t):
    """(left, right) parts of the polygon P [n + 1, 3] cut at t"""
    p = np.array(P, np.float64)
    t = np.float64(t)
    w = np.float64(1.0) - t
    left, right = [p[0]], [p[-1]]
    while len(p) > 1:
        p = w * p[:-1] + t * p[1:]
        left.append(p[0])
        right.append(p[-1])
    return np.array(left), np.array(right[::-1])


def restrict(P, u0, u1):
    """the polygon of P's curve on [u0, u1]"""
    P = np.array(P, np.float64)
    if u1 < 1.0:
        P = cut(P, u1)[0]
    if u0 > 0.0:
        P = cut(P, np.float64(u0) / np.float64(u1))[1]
    return P


def map_u(v, u0, u1):
    v = np.float64(v)
    return (np.float64(1.0) - v) * np.float64(u0) + v * np.float64(u1)


def _whole_invalid(coef, seg_time, orders, segs):
    T = np.asarray([seg_time[i] for i in segs], np.float64)
    polys = [CM.world_points(coef[i], seg_time[i], orders[i]) for i in segs]
    with np.errstate(invalid="ignore"):
        return not np.all(np.isfinite(T) & (T > 0)) or not all(np.all(np.abs(P) <= CM.FLT_MAX) for P in polys)


def restricted_batch(coef, seg_time, orders, seg_offsets, t_start=None, horizon=None):
    """The first pieces of the window forms as a plain batch: (coef [S, 39], seg_time = 1 [S], orders [S], seg_offsets [B + 1]) of the
    restricted polygons, origin [S] = (segment of the packed batch, u0, u1), and invalid [B] (the window's rule or the whole-curve
    rule over all segments; such a trajectory, like one with an empty window, has no row)"""
    B = len(seg_offsets) - 1
    rows, od, origin, offs, invalid = [], [], [], [0], np.zeros(B, bool)
    for b in range(B):
        segs = range(int(seg_offsets[b]), int(seg_offsets[b + 1]))
        t0 = 0.0 if t_start is None else t_start[b]
        h = np.inf if horizon is None else horizon[b]
        win = windows([seg_time[i] for i in segs], t0, h) if window_valid(t0, h) else None
        if win is None or _whole_invalid(coef, seg_time, orders, segs):
            invalid[b] = True
        else:
            for i, w in zip(segs, win):
                if w is None:
                    continue
                n = int(orders[i])
                P = restrict(CM.world_points(coef[i], seg_time[i], n), *w)
                row = np.zeros(STRIDE)
                row[:3 * (n + 1)] = P.T.reshape(-1)                  # row[k * (n + 1) + j] = P[j][k]
                rows.append(row)
                od.append(n)
                origin.append((i, w[0], w[1]))
        offs.append(len(rows))
    return (np.array(rows).reshape(-1, STRIDE), np.ones(len(rows)), np.array(od, np.int32), np.array(offs, np.int32)), origin, invalid


def _map_back(rec, seg_name, u_name, origin):
    for b in range(len(rec)):
        s = int(rec[seg_name][b])
        if s >= 0:
            i, u0, u1 = origin[s]
            rec[seg_name][b] = i
            rec[u_name][b] = map_u(rec[u_name][b], u0, u1)


def certify_window(pts, coef, seg_time, orders, seg_offsets, t_start, horizon, margin, max_depth, piece_cap, index_base=0):
    """(certificates, stats) of pct_bezier_certify_window_batch"""
    packed, origin, invalid = restricted_batch(coef, seg_time, orders, seg_offsets, t_start, horizon)
    cert, stats = CM.certify(pts, *packed, margin, max_depth, piece_cap, index_base)
    _map_back(cert, "hit_seg", "hit_u", origin)
    cert["status"][invalid] = CM.INVALID
    return cert, stats


def clearance_window(pts, coef, seg_time, orders, seg_offsets, t_start, horizon, tol, cap, max_depth, piece_cap, index_base=0):
    """(records, stats) of pct_bezier_clearance_window_batch"""
    packed, origin, invalid = restricted_batch(coef, seg_time, orders, seg_offsets, t_start, horizon)
    rec, stats = KM.clearances(pts, *packed, tol, cap, max_depth, piece_cap, index_base)
    _map_back(rec, "at_seg", "at_u", origin)
    rec["status"][invalid] = KM.INVALID
    rec["lo"][invalid] = np.nan
    rec["hi"][invalid] = np.nan
    return rec, stats


# ---- the obstacle behind the drone: a 3 m line along x flown at 1 m/s as three cubic segments, a point 4 mm off its axis at x = 1 --------
def cubic_line(x0, x1, T=1.0):
    xs = np.linspace(x0, x1, 4)
    row = np.zeros(12)
    row[0:4] = xs
    return row / T


LINE3 = dict(pts=np.array([[1.0, 0.004, 0.0]], np.float32),
             traj=(np.array([cubic_line(0, 1), cubic_line(1, 2), cubic_line(2, 3)]), np.ones(3), np.full(3, 3, np.int32)),
             margin=0.005)
# (t_start, horizon) -> status of the certified check
LINE3_TABLE = (
    (0.0, np.inf, CM.HIT),
    (1.5, np.inf, CM.FREE),
    (0.0, 0.9, CM.FREE),
    (0.9, 0.2, CM.HIT),
    (1.25, 0.5, CM.FREE),
    (3.0, np.inf, CM.FREE),                # the empty window
)
