"""numpy restatement of the depth-image contract (include/pct_engine.h, paragraph "Depth images"): the projection, the seen-through
test, the un-projection, a point z-buffer renderer (test side only: the library renders nothing) and a window model on
ring_remove_model.RemoveWindow -- the reference of tests/test_depth_api.py and tests/test_gpu_depth.py.  Every expression is fp64 from
float-widened operands, one numpy operation per rounding, in the order the header writes it."""
import numpy as np

import ring_remove_model as R

DEPTH_Z, DEPTH_RANGE = 0, 1


def _view(view):
    """(t [3], R [3, 3], focal, near_z, width, height, metric) of anything shaped like pct_depth_view"""
    return (np.array(list(view.t), np.float64), np.array(list(view.R), np.float64).reshape(3, 3), np.float64(view.focal),
            np.float64(view.near_z), int(view.width), int(view.height), int(view.metric))


def round_half_away(q):
    """C round(): half away from zero (q - trunc(q) is exact)"""
    with np.errstate(invalid="ignore"):
        t = np.trunc(q)
        return t + np.where(np.abs(q - t) >= 0.5, np.sign(q), 0.0)


def project(view, xyz):
    """rows of fp32 points -> dict(inside bool [n], ru / rv int64 [n] (-1 outside), cz, d [n, 3], u, v)"""
    t, Rm, focal, near_z, w, h, _ = _view(view)
    p = np.asarray(xyz, np.float32).reshape(-1, 3).astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        d = p - t
        c = [(d[:, 0] * Rm[0, k] + d[:, 1] * Rm[1, k]) + d[:, 2] * Rm[2, k] for k in range(3)]
        cz = c[2]
        front = cz >= near_z
        scale = focal / cz * np.float64(w)
        u = c[0] * scale + np.float64(w) / 2.0
        v = c[1] * scale + np.float64(h) / 2.0
        fu, fv = round_half_away(u), round_half_away(v)
        inside = front & (fu >= 0.0) & (fu <= np.float64(w - 1)) & (fv >= 0.0) & (fv <= np.float64(h - 1))
    ru = np.where(inside, fu, -1.0).astype(np.int64)
    rv = np.where(inside, fv, -1.0).astype(np.int64)
    return dict(inside=inside, ru=ru, rv=rv, cz=cz, d=d, u=u, v=v)


def seen(view, image, xyz, margin):
    """which rows the image sees through (strict; a non-finite pixel proves nothing)"""
    _, _, _, _, w, h, metric = _view(view)
    img = np.asarray(image, np.float32).reshape(h, w)
    pr = project(view, xyz)
    val = img[np.maximum(pr["rv"], 0), np.maximum(pr["ru"], 0)].astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        wv = val - np.float64(margin)
        d = pr["d"]
        if metric == DEPTH_Z:
            nearer = pr["cz"] < wv
        else:
            nearer = (wv > 0.0) & (((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]) < wv * wv)
    return pr["inside"] & np.isfinite(val) & nearer


def unproject(view, image, max_depth=np.inf):
    """(valid bool [height * width], fp32 points [valid.sum(), 3] in row-major pixel order); metric Z only"""
    t, Rm, focal, near_z, w, h, metric = _view(view)
    if metric != DEPTH_Z:
        raise ValueError("only z-depth images are un-projected")
    dep = np.asarray(image, np.float32).reshape(h * w).astype(np.float64)
    with np.errstate(invalid="ignore"):
        valid = np.isfinite(dep) & (dep >= near_z) & (dep <= np.float64(max_depth))
    y, x = np.divmod(np.arange(h * w), w)
    a = (x.astype(np.float64) / np.float64(w) - 0.5) / focal
    b = (y.astype(np.float64) - 0.5 * np.float64(h)) / np.float64(w) / focal
    with np.errstate(invalid="ignore", over="ignore"):
        pts = np.stack([t[k] + dep * ((a * Rm[k, 0] + b * Rm[k, 1]) + Rm[k, 2]) for k in range(3)], axis=1).astype(np.float32)
    return valid, pts[valid]


def classify(views, images, points, margin):
    """(seen_by int32 [n], pixel int32 [n, 2]): planner points narrowed to fp32 first; the lowest view that sees the point through,
    and its pixel in the LAST view (-1, -1 when it is not in that image)"""
    with np.errstate(over="ignore"):
        p = np.asarray(points, np.float64).reshape(-1, 3).astype(np.float32)
    seen_by = np.full(len(p), -1, np.int32)
    for k in reversed(range(len(views))):
        seen_by[seen(views[k], images[k], p, margin)] = k
    pr = project(views[-1], p)
    return seen_by, np.stack([pr["ru"], pr["rv"]], axis=1).astype(np.int32)


def render(view, points, metric=DEPTH_Z):
    """z-buffer of points: every pixel holds the fp32 depth (metric Z) or range (metric RANGE) of the nearest point that projects onto
    it, +inf where none does -- a test-side renderer"""
    _, _, _, _, w, h, _ = _view(view)
    pr = project(view, points)
    d = pr["d"]
    with np.errstate(invalid="ignore", over="ignore"):
        val = pr["cz"] if metric == DEPTH_Z else np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
    img = np.full(h * w, np.inf, np.float32)
    ok = pr["inside"]
    np.minimum.at(img, (pr["rv"] * w + pr["ru"])[ok], val[ok].astype(np.float32))
    return img.reshape(h, w)


class DepthWindow(R.RemoveWindow):
    """RemoveWindow fed depth images: carve = a removal by the seen-through predicate, append_depth = an append of the un-projected
    frame (de-duplicating when dedup is on, plain otherwise).  The camelCase members are those of the corridor finder."""

    def __init__(self, cap, res=R.M.RES, dedup=True):
        super().__init__(cap, res)
        self.dedup = dedup

    def carve(self, view, image, margin):
        return self._remove(seen(view, image, self.live(), margin))

    def append_depth(self, view, image, max_depth=np.inf):
        """returns (the frame = the valid pixels un-projected, the kept flags over it)"""
        _, frame = unproject(view, image, max_depth)
        if len(frame) > self.cap:
            raise OverflowError("more valid pixels than the window's capacity")
        if self.dedup:
            return frame, self.append(frame)
        self.append_plain(frame)
        return frame, np.ones(len(frame), bool)

    def clearSeenThrough(self, view, image, margin):
        return self.carve(view, image, margin)

    def appendDepthImage(self, view, image, max_depth=np.inf):
        return int(self.append_depth(view, image, max_depth)[1].sum())
