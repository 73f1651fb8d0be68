"""Clouds, queries and numpy references of tests/test_gpu_grid_limits.py: the cell index (pct_cloud_build_grid) at its caps.

The references are plain fp64 numpy on the float-widened fp32 inputs, one numpy operation per rounding, in the contract's order
(include/pct_engine.h): d2 = (dx*dx + dy*dy) + dz*dz; the nearest neighbour is the minimum with the LOWEST index among equal minima;
k-NN rows are ordered by (d2, index); a radius row holds d2 <= (double)r * (double)r in ascending index or by (d2, index); inflation is
radiusSearch: min(sqrt(d2) - search_margin, max_radius) on the fp32-narrowed point, or max_radius - search_margin, no index and +inf
where |p - start| > sample_range + max_radius."""
import numpy as np

from pointcloudtraj_amd import synth

NO_INDEX = 0xFFFFFFFF
PPC = 6.0                          # points per unit cell inside a cluster
CAP = 1023.0                       # the far corner of a box with 1024 unit cells on an axis
N_CORNER = 64


def cube_points(far_pin=(CAP, CAP, CAP), b_top_z=1022.5, seed=7100):
    """(points fp32 [n, 3], index of the far pin): the pins (0, 0, 0) and far_pin, cluster A uniform in [0, 12)^3 and cluster B uniform in
    [1010, 1022.5)^2 x [1010, b_top_z), both at PPC points per unit cell.  Every point but the far pin is below it on x and y, so the far
    pin is alone in its cell."""
    na = int(round(PPC * 12.0 ** 3))
    nb = int(round(PPC * 12.5 * 12.5 * (b_top_z - 1010.0)))
    a = synth.uniform_points(seed, na, 0.0, 12.0)
    u = synth.uniform01_f32(seed + 1, 3 * nb).reshape(nb, 3)
    b = (np.float32(1010.0) + u * np.array([12.5, 12.5, b_top_z - 1010.0], np.float32)).astype(np.float32)
    assert b[:, :2].max() < CAP and b[:, 2].max() < far_pin[2] and b.min() >= 1010.0
    pts = np.concatenate([np.array([(0.0, 0.0, 0.0), far_pin], np.float32), a, b]).astype(np.float32)
    pts.setflags(write=False)
    return pts, 1


def corner_queries(far_pin=(CAP, CAP, CAP), seed=7110):
    """N_CORNER queries q = far_pin + d, d componentwise in [0, 0.45]: row 0 is the pin itself, rows 1..6 have one component 3.0 beyond
    it (outside the grid: clamped into the last cell).  Every point of cube_points but the pin is componentwise <= the pin and below it
    on x, so the pin is strictly the nearest point of each of these queries."""
    d = (synth.uniform01_f32(seed, 3 * N_CORNER).reshape(N_CORNER, 3) * np.float32(0.45)).astype(np.float32)
    d[0] = 0.0
    for k in range(6):
        d[1 + k, k % 3] = 3.0
    q = (np.asarray(far_pin, np.float32) + d).astype(np.float32)
    assert np.all(q >= np.asarray(far_pin, np.float32))
    return q


def cluster_queries(n, seed, b_top_z=1022.5):
    """n queries, half uniform in cluster A's box and half in cluster B's, each box grown by one cell"""
    a = synth.uniform_points(seed, n // 2, -1.0, 13.0)
    u = synth.uniform01_f32(seed + 1, 3 * (n - n // 2)).reshape(-1, 3)
    b = (np.float32(1009.0) + u * np.array([14.5, 14.5, b_top_z + 1.0 - 1009.0], np.float32)).astype(np.float32)
    return np.concatenate([a, b]).astype(np.float32)


def cube_batch(Q, far_pin=(CAP, CAP, CAP), b_top_z=1022.5, seed=7120):
    """a batch of Q queries: the corner queries first where Q >= N_CORNER (Q == 1: the query on the pin), cluster queries behind them"""
    corner = corner_queries(far_pin)
    if Q <= N_CORNER:
        return corner[:Q].copy()
    return np.concatenate([corner, cluster_queries(Q - N_CORNER, seed + Q, b_top_z)]).astype(np.float32)


def sample_rows(Q, keep, seed, n=256):
    """the rows a numpy comparison covers: the first `keep` rows (never sampled away) and n more drawn with a fixed seed"""
    rest = np.arange(keep, Q)
    if len(rest) > n:
        rest = rest[np.sort(synth.shuffled_order(seed, len(rest))[:n])]
    return np.concatenate([np.arange(min(keep, Q)), rest]).astype(np.int64)


def sq_dists(pts, q, chunk=64):
    """fp64 squared distances [len(q), len(pts)] of fp32 points and fp32 queries, (dx*dx + dy*dy) + dz*dz"""
    P = np.asarray(pts, np.float32).astype(np.float64).reshape(-1, 3)
    Qf = np.asarray(q, np.float32).astype(np.float64).reshape(-1, 3)
    out = np.empty((len(Qf), len(P)), np.float64)
    for a in range(0, len(Qf), chunk):
        b = Qf[a:a + chunk]
        dx, dy, dz = (P[None, :, k] - b[:, None, k] for k in range(3))
        out[a:a + chunk] = (dx * dx + dy * dy) + dz * dz
    return out


def nn(pts, q, chunk=32):
    """(idx int64 [Q], d2 float64 [Q]): argmin names the first, i.e. the lowest index, of equal minima"""
    idx = np.empty(len(q), np.int64)
    d2 = np.empty(len(q), np.float64)
    for a in range(0, len(q), chunk):
        s = sq_dists(pts, q[a:a + chunk], chunk)
        idx[a:a + chunk] = np.argmin(s, axis=1)
        d2[a:a + chunk] = s[np.arange(len(s)), idx[a:a + chunk]]
    return idx, d2


def knn(pts, q, k):
    """(idx uint32 [Q, k], d2 float64 [Q, k]), rows by (d2, index)"""
    s = sq_dists(pts, q)
    idx = np.full((len(s), k), NO_INDEX, np.uint32)
    d2 = np.full((len(s), k), np.inf)
    for i, row in enumerate(s):
        order = np.lexsort((np.arange(len(row)), row))[:k]
        idx[i, :len(order)], d2[i, :len(order)] = order, row[order]
    return idx, d2


def radius_rows(pts, q, r, order):
    """(offsets int64 [Q + 1], idx uint32, d2 float64): hits d2 <= (double)r * (double)r of the fp32 radius, ascending index (order 0)
    or nearest first with equal d2 in ascending index (order 1)"""
    s = sq_dists(pts, q)
    rr = np.float64(np.float32(r)) * np.float64(np.float32(r))
    offsets = np.zeros(len(s) + 1, np.int64)
    idx, d2 = [], []
    for i, row in enumerate(s):
        ids = np.nonzero(row <= rr)[0]
        if order == 1:
            ids = ids[np.lexsort((ids, row[ids]))]
        offsets[i + 1] = offsets[i] + len(ids)
        idx.append(ids)
        d2.append(row[ids])
    return offsets, np.concatenate(idx).astype(np.uint32), np.concatenate(d2).astype(np.float64)


def inflate(pts, prm, points64):
    """(radius [Q], idx int64 [Q] (-1: none), d2 [Q]) of radiusSearch for fp64 points; prm: dict(start, sample_range, search_margin,
    max_radius)"""
    p = np.asarray(points64, np.float64).reshape(-1, 3)
    dx, dy, dz = (p[:, k] - np.float64(prm["start"][k]) for k in range(3))
    far = np.sqrt(dx * dx + dy * dy + dz * dz) > np.float64(prm["sample_range"]) + np.float64(prm["max_radius"])
    idx, d2 = nn(pts, p.astype(np.float32))
    rad = np.minimum(np.sqrt(d2) - np.float64(prm["search_margin"]), np.float64(prm["max_radius"]))
    return (np.where(far, np.float64(prm["max_radius"]) - np.float64(prm["search_margin"]), rad), np.where(far, -1, idx),
            np.where(far, np.inf, d2))


def flat_cloud(dims, n=300000, seed=7200):
    """(points fp32 [n + 2, 3], the max-corner pin): a box with extent 1023 on the axes where dims is 1024 and 0.5 on the thin one; pins
    at the two box corners, n uniform points inside"""
    ext = np.array([CAP if g == 1024 else 0.5 for g in dims], np.float32)
    u = synth.uniform01_f32(seed, 3 * n).reshape(n, 3)
    pts = np.concatenate([np.zeros((1, 3), np.float32), ext[None], (u * ext).astype(np.float32)]).astype(np.float32)
    pts.setflags(write=False)
    return pts, ext


def flat_queries(dims, Q=20000, seed=7210):
    """uniform queries from the box grown by one cell, and in front of them: the max-corner pin, queries on the cell faces of the last row
    of each long axis (coordinates 1021, 1022 and 1023 exactly, and one ulp to either side), and queries up to 3 cells beyond the box"""
    ext = np.array([CAP if g == 1024 else 0.5 for g in dims], np.float32)
    u = synth.uniform01_f32(seed, 3 * Q).reshape(Q, 3)
    q = (np.float32(-1.0) + u * (ext + np.float32(2.0))).astype(np.float32)
    special = [ext.copy()]
    for k in range(3):
        if dims[k] != 1024:
            continue
        for face in (1021.0, 1022.0, 1023.0):
            f = np.float32(face)
            for v in (np.nextafter(f, np.float32(0)), f, np.nextafter(f, np.float32(2000))):
                for other in (0.25, 0.999):
                    s = (ext * np.float32(other)).astype(np.float32)
                    s[k] = v
                    special.append(s)
        for beyond in (0.5, 3.0):
            s = ext.copy()
            s[k] += np.float32(beyond)
            special.append(s)
    special.append((ext + np.float32(3.0)).astype(np.float32))
    special = np.asarray(special, np.float32)
    q[:len(special)] = special
    return q, len(special)


def floor_cloud(box, n=3000, seed=7300):
    """(points fp32, index of the max-corner pin, h = the floored cell max_ext / 1023 as the build rounds it): pins at the box's corners
    (0, 0, 0) and `box`, and n uniform points within six cells of each pin, so that every query near a pin has its neighbours near by"""
    box = np.asarray(box, np.float32)
    h = np.float32(np.float64(box.max()) / 1023.0)
    near = np.minimum(box, np.float32(6.0) * h)
    lo = (synth.uniform01_f32(seed, 3 * n).reshape(n, 3) * near).astype(np.float32)
    hi = (box - synth.uniform01_f32(seed + 1, 3 * n).reshape(n, 3) * near).astype(np.float32)
    pts = np.concatenate([np.zeros((1, 3), np.float32), box[None], lo, hi]).astype(np.float32)
    assert np.all(pts >= 0) and np.all(pts <= box)
    pts.setflags(write=False)
    return pts, 1, h


def floor_queries(box, dims, h, seed=7310):
    """queries on the max-side pin and one ulp below and above it per axis, queries one ulp to either side of the last three cell faces of
    the long axis (from the fp64 face positions o + i * hd, o = 0), and uniform ones within six cells of the max corner"""
    box = np.asarray(box, np.float32)
    k = int(np.argmax(box))
    hd = np.float64(h)
    qs = [box.copy()]
    for ax in range(3):
        for toward in (np.float32(-1e30), np.float32(1e30)):
            s = box.copy()
            s[ax] = np.nextafter(box[ax], toward)
            qs.append(s)
    for i in range(dims[k] - 3, dims[k]):
        face = np.float32(np.float64(i) * hd)
        for v in (np.nextafter(face, np.float32(0)), face, np.nextafter(face, np.float32(1e30))):
            for other in (1.0, 0.97):
                s = (box * np.float32(other)).astype(np.float32)
                s[k] = v
                qs.append(s)
    near = np.minimum(box, np.float32(6.0) * np.float32(h))
    u = synth.uniform01_f32(seed, 3 * 400).reshape(400, 3)
    qs.extend((box + np.float32(1.0) * np.float32(h) - u * (near + np.float32(h))).astype(np.float32))
    return np.asarray(qs, np.float32)
