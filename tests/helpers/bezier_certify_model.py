"""numpy restatement of the certified Bezier check (include/pct_engine.h, paragraph "Certified Bezier check"), on top of segment_model
(the chord test: the candidates of "Segment queries") and a brute-force nearest neighbour (the end test).

Elementwise fp64 in the contract's order -- numpy's separate operations do not fuse, and its sqrt is correctly rounded:

    P[j][k] = polycoef[row][k*(n+1) + j] * seg_time[row]                      world control points
    q[i]    = (p[i] + p[i+1]) * 0.5, level by level                           left child: first point of every level;
                                                                              right child: last point of every level, reversed
    a, b    = P[0], P[n] narrowed to fp32 and widened                         rho2 = max_j d2(segment (a, b), P[j])  (fp64 point)
    reach   = ((margin + sqrt(rho2)) * (1 + 2^-20)) + max|P[j][k]| * 2^-40
    BLOCKED = some row has d2 <= min(reach * reach, DBL_MAX)                  HIT(x) = sqrt(nearest d2 of x) - margin < 0

and the rounds of the contract.  Also here: the scene of the soundness test, the dense sampler it uses and the hand cases that
tests/test_bezier_certify_model.py pins and tests/test_gpu_bezier_certify.py runs on the card."""
import functools
import math
from fractions import Fraction

import numpy as np

import segment_model as M
from pointcloudtraj_amd import synth

FREE, HIT, UNDECIDED, INVALID = 0, 1, 2, 3
NO_INDEX = 0xFFFFFFFF
FLT_MAX = float(np.finfo(np.float32).max)
MAX_DEPTH = 20
CERT_DTYPE = np.dtype([("status", np.int32), ("depth", np.int32), ("hit_seg", np.int32), ("hit_idx", np.uint32), ("hit_u", np.float64),
                       ("hit_d2", np.float64), ("min_d2", np.float64), ("pieces", np.int64)])
assert CERT_DTYPE.itemsize == 48


def pack(trajectories):
    """a list of (polycoef [nseg, >= 3 * (order + 1)], seg_time [nseg], orders [nseg]) -> (coef [S, stride], seg_time [S], orders [S],
    seg_offsets [B + 1]), the rows one after another, as pct_bezier_batch holds them"""
    stride = max([np.asarray(c).shape[1] for c, _, _ in trajectories], default=3)
    offs = np.zeros(len(trajectories) + 1, np.int32)
    offs[1:] = np.cumsum([len(t) for _, t, _ in trajectories])
    coef = np.zeros((int(offs[-1]), stride))
    for (c, _, _), a in zip(trajectories, offs):
        c = np.asarray(c, np.float64)
        coef[a:a + len(c), :c.shape[1]] = c
    seg_time = np.concatenate([np.asarray(t, np.float64).reshape(-1) for _, t, _ in trajectories]) if trajectories else np.zeros(0)
    orders = np.concatenate([np.asarray(o, np.int32).reshape(-1) for _, _, o in trajectories]) if trajectories else np.zeros(0, np.int32)
    return coef, seg_time, orders.astype(np.int32), offs


def world_points(row, T, n):
    """P [n + 1, 3] of one segment"""
    m = int(n) + 1
    with np.errstate(all="ignore"):
        return np.stack([np.asarray(row[k * m:(k + 1) * m], np.float64) * np.float64(T) for k in range(3)], axis=1)


def halve(P):
    """(left, right) children of the polygon P [n + 1, 3]"""
    p = np.array(P, np.float64)
    left, right = [p[0]], [p[-1]]
    while len(p) > 1:
        p = (p[:-1] + p[1:]) * 0.5
        left.append(p[0])
        right.append(p[-1])
    return np.array(left), np.array(right[::-1])


def point_d2(P, a, b):
    """d2 of "Segment queries" for the fp64 points P [m, 3] against segment (a, b)"""
    with np.errstate(all="ignore"):
        e = b - a
        L2 = (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]
        w0, w1, w2 = P[:, 0] - a[0], P[:, 1] - a[1], P[:, 2] - a[2]
        dot = (w0 * e[0] + w1 * e[1]) + w2 * e[2]
        s = np.zeros_like(dot) if L2 == 0 else dot / L2
        s = np.where(s > 0, np.where(s > 1, 1.0, s), 0.0)
        c0, c1, c2 = w0 - s * e[0], w1 - s * e[1], w2 - s * e[2]
        return (c0 * c0 + c1 * c1) + c2 * c2


def geometry(P, margin):
    """(a, b, reach) of a piece"""
    a = P[0].astype(np.float32).astype(np.float64)
    b = P[-1].astype(np.float32).astype(np.float64)
    rho = np.sqrt(np.max(point_d2(P, a, b)))
    cmax = np.max(np.abs(P))
    return a, b, ((np.float64(margin) + rho) * (1.0 + 2.0 ** -20)) + cmax * 2.0 ** -40


def nearest(pts, x):
    """(index or NO_INDEX, d2 or +inf) of the fp32 points x [m, 3] (given widened) among the rows pts [N, 3] fp32: the minimum of
    ((dx*dx + dy*dy) + dz*dz), the lowest index on ties; rows that hold a NaN or an infinity never win"""
    p = np.asarray(pts, np.float32).reshape(-1, 3).astype(np.float64)
    idx = np.full(len(x), NO_INDEX, np.int64)
    d2 = np.full(len(x), np.inf)
    if len(p) == 0 or len(x) == 0:
        return idx, d2
    for lo in range(0, len(x), 256):
        q = x[lo:lo + 256]
        with np.errstate(all="ignore"):
            dx, dy, dz = (p[None, :, k] - q[:, None, k] for k in range(3))
            d = (dx * dx + dy * dy) + dz * dz
        d = np.where(np.isfinite(d), d, np.inf)
        i = np.argmin(d, axis=1)                                  # the first, i.e. the lowest index, of equal minima
        best = d[np.arange(len(q)), i]
        idx[lo:lo + 256] = np.where(np.isfinite(best), i, NO_INDEX)
        d2[lo:lo + 256] = best
    return idx, d2


def blocked(pts, a, b, reach):
    r2 = M.reach2(reach)
    if len(pts) == 0 or r2 is None:
        return False
    d2, _ = M.pair_d2_s(pts, a, b)
    with np.errstate(invalid="ignore"):
        return bool(np.any(d2 <= r2))


def certify(pts, coef, seg_time, orders, seg_offsets, margin, max_depth, piece_cap, index_base=0):
    """(certificates [B] of CERT_DTYPE, stats int64 [3] = rounds, pieces, capped) of the contract, by brute force"""
    pts = np.asarray(pts, np.float32).reshape(-1, 3)
    B = len(seg_offsets) - 1
    cert = np.zeros(B, CERT_DTYPE)
    cert["hit_seg"], cert["hit_idx"], cert["hit_u"], cert["hit_d2"], cert["min_d2"] = -1, NO_INDEX, np.nan, np.inf, np.inf
    live = []                                                     # (trajectory, segment, k, polygon), in that order
    for t in range(B):
        segs = range(int(seg_offsets[t]), int(seg_offsets[t + 1]))
        T = np.asarray([seg_time[i] for i in segs], np.float64)
        polys = [world_points(coef[i], seg_time[i], orders[i]) for i in segs]
        with np.errstate(invalid="ignore"):
            bad = not np.all(np.isfinite(T) & (T > 0)) or not all(np.all(np.abs(P) <= FLT_MAX) for P in polys)
        if bad:
            cert["status"][t] = INVALID
            continue
        live += [(t, i, 0, P) for i, P in zip(segs, polys)]
    rounds = total = capped = 0
    undecided = set()
    depth = 0
    while live:
        rounds += 1
        total += len(live)
        geo = [geometry(P, margin) for _, _, _, P in live]
        ends = np.array([[g[0], g[1]] for g in geo]).reshape(-1, 3)
        nn_idx, nn_d2 = nearest(pts, ends)
        hit_of = {}                                               # trajectory -> (piece number, end): the first in (segment, u) order
        for n, (t, seg, k, _) in enumerate(live):
            cert["pieces"][t] += 1
            cert["depth"][t] = depth
            cert["min_d2"][t] = min(cert["min_d2"][t], nn_d2[2 * n], nn_d2[2 * n + 1])
            for end in (0, 1):
                if np.sqrt(nn_d2[2 * n + end]) - np.float64(margin) < 0 and t not in hit_of:
                    hit_of[t] = (n, end)
        for t, (n, end) in hit_of.items():
            _, seg, k, _ = live[n]
            cert["status"][t] = HIT
            cert["hit_seg"][t] = seg
            cert["hit_idx"][t] = nn_idx[2 * n + end] + index_base
            cert["hit_u"][t] = math.ldexp(k + end, -depth)
            cert["hit_d2"][t] = nn_d2[2 * n + end]
        split = []
        for n, (t, seg, k, P) in enumerate(live):
            if t in hit_of or not blocked(pts, *geo[n]):
                continue
            if depth == max_depth:
                undecided.add(t)
            else:
                split.append((t, seg, k, P))
        live = []
        if 2 * len(split) > piece_cap:
            capped = 1
            undecided.update(t for t, _, _, _ in split)
        else:
            for t, seg, k, P in split:
                left, right = halve(P)
                live += [(t, seg, 2 * k, left), (t, seg, 2 * k + 1, right)]
        depth += 1
    for t in undecided:
        cert["status"][t] = UNDECIDED
    return cert, np.array([rounds, total, capped], np.int64)


# ---- dense sampling on the dyadic grid u = i / 4096 ----------------------------------------------------------------------------------
GRID = 4096


@functools.lru_cache(maxsize=None)
def _powers():
    """pw[i][j] = (i / 4096)^j rounded once from the exact rational, i = 0..4096, j = 0..12: the powers of
    bezier_model.bezier_samples_exact_powers on this grid, where 1 - u is exact as well"""
    return np.array([[float(Fraction(i, GRID) ** j) for j in range(13)] for i in range(GRID + 1)])


def dense_samples(P):
    """the 4096 points u = i / 4096, i = 0..4095, of the curve with WORLD control points P [n + 1, 3], in the term order of
    getPosFromBezier ((C * c) * u^j) * (1 - u)^(n - j), j ascending, with exact powers: what bezier_samples_exact_powers returns for the row P,
    seg_time 1 and dt = 2^-12 (tests/test_bezier_certify_model.py compares the two)"""
    n = len(P) - 1
    pw = _powers()
    i = np.arange(GRID)
    out = np.zeros((GRID, 3))
    for d in range(3):
        acc = np.zeros(GRID)
        for j in range(n + 1):
            acc = acc + float(math.comb(n, j)) * float(P[j, d]) * pw[i, j] * pw[GRID - i, n - j]
        out[:, d] = acc * 1.0
    return out


def clearance(pts, samples):
    """the smallest distance from any sample to any row of pts (fp64, rows widened)"""
    p = np.asarray(pts, np.float32).astype(np.float64)
    best = np.inf
    for lo in range(0, len(samples), 1024):
        d = samples[lo:lo + 1024, None, :] - p[None, :, :]
        best = min(best, float(np.sqrt((d * d).sum(axis=2)).min()))
    return best


# ---- the scene of the soundness test ----------------------------------------------------------------------------------------------
# 300 uniform points in [0, 10)^3, margin 0.25, 64 trajectories of three segments, orders 0..12 in turn.  With SEED = 7 the model gives,
# at max_depth 12 and an ample piece_cap: see SCENE_GAVE (filled from a run of the model alone; test_bezier_certify_model.py asserts it).
SEED = 7
N_POINTS, N_TRAJ, MARGIN = 300, 64, 0.25


def _uniform(seed, n):
    return (synth.splitmix64(seed, n) >> np.uint64(11)).astype(np.float64) * 2.0 ** -53


@functools.lru_cache(maxsize=None)
def scene(seed=SEED, n_points=N_POINTS, n_traj=N_TRAJ):
    """(pts fp32 [n_points, 3], trajectories): trajectory t has three segments of orders (3t, 3t + 1, 3t + 2) mod 13 between four
    waypoints about 1.2 m apart, control points evenly spaced with +-0.15 m of jitter, stored divided by the segment time"""
    pts = (_uniform(seed, 3 * n_points).reshape(n_points, 3) * 10.0).astype(np.float32)
    r = _uniform(seed + 1, n_traj * (3 + 9 + 3 * 13 * 3))
    trajs, k = [], 0
    for t in range(n_traj):
        w = [1.0 + r[k:k + 3] * 8.0]
        k += 3
        for _ in range(3):
            w.append(w[-1] + (r[k:k + 3] - 0.5) * 2.4)
            k += 3
        orders = np.array([(3 * t + s) % 13 for s in range(3)], np.int32)
        times = np.array([0.5 + 0.25 * ((t + s) % 3) for s in range(3)])
        coef = np.zeros((3, 39))
        for s, n in enumerate(orders):
            m = int(n) + 1
            for d in range(3):
                base = np.linspace(w[s][d], w[s + 1][d], m) if m > 1 else np.array([w[s][d]])
                jit = (r[k:k + m] - 0.5) * 0.3
                k += 13
                if m > 2:
                    base[1:-1] += jit[1:-1]
                coef[s, d * m:(d + 1) * m] = base
        trajs.append((coef / times[:, None], times, orders))
    pts.setflags(write=False)
    return pts, trajs


@functools.lru_cache(maxsize=None)
def scene_certificates(max_depth=12, piece_cap=1 << 20):
    pts, trajs = scene()
    return certify(pts, *pack(trajs), MARGIN, max_depth, piece_cap)


# ---- hand cases ----------------------------------------------------------------------------------------------------------------------
def line(a, b, T=1.0):
    """one segment of order 1 from a to b flown in T seconds"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return (np.array([[a[0], b[0], a[1], b[1], a[2], b[2]]]) / T, np.array([T]), np.array([1], np.int32))


# The 4 mm line: 1 m along x at 1 m/s, an obstacle 4 mm off the axis halfway between the samples 0.50 and 0.52 of dt = 0.02: every sample
# is at least sqrt(10^2 + 4^2) = 10.8 mm from it, the margin is 5 mm.
FOUR_MM = dict(pts=np.array([[0.51, 0.004, 0.0]], np.float32), traj=line((0, 0, 0), (1, 0, 0)), margin=0.005)

# A point at exactly the margin from a line: 2^-7 m beside x = fp32(1/3), which no halving down to depth 12 comes near.
AT_MARGIN = dict(x=np.float32(1.0) / np.float32(3.0), margin=2.0 ** -7, traj=line((0, 0, 0), (1, 0, 0)))


def at_margin_cloud(ulps=0):
    """the cloud of the margin case with the point `ulps` fp32 ulps farther from the line (negative: nearer)"""
    y = np.float32(AT_MARGIN["margin"])
    for _ in range(abs(ulps)):
        y = np.nextafter(y, np.float32(np.inf if ulps > 0 else 0.0))
    return np.array([[AT_MARGIN["x"], y, 0.0]], np.float32)
