"""numpy restatement of the trajectory clearance (include/pct_engine.h, paragraph "Trajectory clearance") on top of the certified check's
model: its world points, halving, chord geometry, brute-force nearest neighbour, scene and dense sampler.

Elementwise fp64 in the contract's order:

    a, b, rho, cmax   as in bezier_certify_model.geometry           ell = sqrt((e0*e0 + e1*e1) + e2*e2), e = b - a
    da, db            sqrt of the nearest d2 of the fp32 points a, b
    L = max(0, (((da + db) - ell) * 0.5 - rho) - (((da + db) + ell + rho) * 2^-20 + cmax * 2^-40)),  +inf when a d2 is +inf
    RETIRE iff L >= min(sqrt(U2), cap) - tol, U2 the smallest end d2 examined so far

and the rounds of the contract.  Also here: what the scene gave (SCENE_GAVE, from a run of this model alone) and the hand cases that
tests/test_bezier_clearance_model.py pins and tests/test_gpu_bezier_clearance.py runs on the card."""
import functools
import math

import numpy as np

from bezier_certify_model import (FLT_MAX, FOUR_MM, NO_INDEX, clearance, dense_samples, halve, line, nearest, pack, point_d2, scene,  # noqa: F401
                                  world_points)

DONE, OPEN, INVALID = 0, 1, 2
CLR_DTYPE = np.dtype([("status", np.int32), ("depth", np.int32), ("at_seg", np.int32), ("at_idx", np.uint32), ("at_u", np.float64),
                      ("lo", np.float64), ("hi", np.float64), ("pieces", np.int64)])
assert CLR_DTYPE.itemsize == 48


def geometry(P):
    """(a, b, ell, rho, cmax) of a piece"""
    a = P[0].astype(np.float32).astype(np.float64)
    b = P[-1].astype(np.float32).astype(np.float64)
    e = b - a
    ell = np.sqrt((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2])
    return a, b, ell, np.sqrt(np.max(point_d2(P, a, b))), np.max(np.abs(P))


def lower(da, db, ell, rho, cmax):
    """L of the contract"""
    if not np.isfinite(da) or not np.isfinite(db):
        return np.inf
    s = np.float64(da) + np.float64(db)
    t = ((s - ell) * 0.5 - rho) - (((s + ell) + rho) * 2.0 ** -20 + cmax * 2.0 ** -40)
    return np.float64(t) if t > 0 else np.float64(0.0)


def clearances(pts, coef, seg_time, orders, seg_offsets, tol, cap, max_depth, piece_cap, index_base=0, trace=None):
    """(records [B] of CLR_DTYPE, stats int64 [3] = rounds, pieces, capped) of the contract, by brute force; trace: a list that
    receives the live count of every round"""
    pts = np.asarray(pts, np.float32).reshape(-1, 3)
    tol, cap = np.float64(tol), np.float64(cap)
    B = len(seg_offsets) - 1
    rec = np.zeros(B, CLR_DTYPE)
    rec["at_seg"], rec["at_idx"], rec["at_u"], rec["lo"], rec["hi"] = -1, NO_INDEX, np.nan, np.inf, np.inf
    live = []                                                     # (trajectory, segment, k, polygon), in that order
    invalid = set()
    for t in range(B):
        segs = range(int(seg_offsets[t]), int(seg_offsets[t + 1]))
        T = np.asarray([seg_time[i] for i in segs], np.float64)
        polys = [world_points(coef[i], seg_time[i], orders[i]) for i in segs]
        with np.errstate(invalid="ignore"):
            bad = not np.all(np.isfinite(T) & (T > 0)) or not all(np.all(np.abs(P) <= FLT_MAX) for P in polys)
        if bad:
            invalid.add(t)
            continue
        live += [(t, i, 0, P) for i, P in zip(segs, polys)]
    U2 = np.full(B, np.inf)
    lo = np.full(B, np.inf)
    opened = set()
    rounds = total = capped = depth = 0
    while live:
        rounds += 1
        total += len(live)
        if trace is not None:
            trace.append(len(live))
        geo = [geometry(P) for _, _, _, P in live]
        ends = np.array([[g[0], g[1]] for g in geo]).reshape(-1, 3)
        nn_idx, nn_d2 = nearest(pts, ends)
        for n, (t, seg, k, _) in enumerate(live):                 # the fold: ascending 2 * slot + end, strict improvement only
            rec["pieces"][t] += 1
            rec["depth"][t] = depth
            for end in (0, 1):
                d2 = nn_d2[2 * n + end]
                if d2 < U2[t]:
                    U2[t] = d2
                    rec["at_seg"][t] = seg
                    rec["at_idx"][t] = nn_idx[2 * n + end] + index_base
                    rec["at_u"][t] = math.ldexp(k + end, -depth)
        split = []
        for n, (t, seg, k, P) in enumerate(live):
            _, _, ell, rho, cmax = geo[n]
            L = lower(np.sqrt(nn_d2[2 * n]), np.sqrt(nn_d2[2 * n + 1]), ell, rho, cmax)
            if L >= min(np.sqrt(U2[t]), cap) - tol:
                lo[t] = min(lo[t], L)
            elif depth == max_depth or (ell == 0 and rho == 0):
                lo[t] = min(lo[t], L)
                opened.add(t)
            else:
                split.append((t, seg, k, P, L))
        live = []
        if 2 * len(split) > piece_cap:
            capped = 1
            for t, _, _, _, L in split:
                lo[t] = min(lo[t], L)
                opened.add(t)
        else:
            for t, seg, k, P, _ in split:
                left, right = halve(P)
                live += [(t, seg, 2 * k, left), (t, seg, 2 * k + 1, right)]
        depth += 1
    for t in range(B):
        if t in invalid:
            rec["status"][t], rec["lo"][t], rec["hi"][t] = INVALID, np.nan, np.nan
            continue
        rec["status"][t] = OPEN if t in opened else DONE
        rec["hi"][t] = np.sqrt(U2[t])
        rec["lo"][t] = min(lo[t], rec["hi"][t])
    return rec, np.array([rounds, total, capped], np.int64)


# ---- the scene (bezier_certify_model.scene: 300 points, 64 trajectories of three segments, orders 0..12) -----------------------------
TOLS, CAPS = (0.05, 0.01), (np.inf, 0.5)
SCENE_DEPTH, SCENE_PIECE_CAP = 16, 1 << 16
# (tol, cap) -> (rounds, pieces, largest round), from a run of this model alone; tests/test_bezier_clearance_model.py asserts it
SCENE_GAVE = {
    (0.05, np.inf): (6, 1304, 354),
    (0.05, 0.5): (6, 980, 292),
    (0.01, np.inf): (8, 2524, 392),
    (0.01, 0.5): (8, 1732, 302),
}


@functools.lru_cache(maxsize=None)
def scene_clearances(tol, cap, max_depth=SCENE_DEPTH, piece_cap=SCENE_PIECE_CAP):
    """(records, stats, live count per round) of the scene"""
    pts, trajs = scene()
    trace = []
    rec, stats = clearances(pts, *pack(trajs), tol, cap, max_depth, piece_cap, trace=trace)
    return rec, stats, tuple(trace)


@functools.lru_cache(maxsize=None)
def scene_dense():
    """the 4096-per-segment dense-sample clearance of every trajectory of the scene (each segment's end point included)"""
    pts, trajs = scene()
    out = []
    for coef, T, orders in trajs:
        best = np.inf
        for i in range(len(T)):
            P = world_points(coef[i], T[i], orders[i])
            best = min(best, clearance(pts, np.vstack([dense_samples(P), P[-1:]])))
        out.append(best)
    return np.array(out)


# ---- hand cases ----------------------------------------------------------------------------------------------------------------------
def point(p, T=1.0):
    """one segment of order 0: the curve is the point p"""
    p = np.asarray(p, np.float64)
    return (np.array([[p[0], p[1], p[2]]]) / T, np.array([T]), np.array([0], np.int32))


# a row exactly on the curve's end: the 1 m line of FOUR_MM with a row at (1, 0, 0)
ON_THE_END = dict(pts=np.array([[1.0, 0.0, 0.0], [0.5, 0.5, 0.0]], np.float32), traj=line((0, 0, 0), (1, 0, 0)))
# segments of order 0 beside one row: single points as the searches see them
ORDER_ZERO = dict(pts=np.array([[0.0, 0.0, 0.0]], np.float32),
                  trajs=[point((0.25, 0.0, 0.0)), point((0.0, 3.0, 4.0), T=2.0), line((1, 1, 1), (2, 1, 1))])
