"""numpy restatement of the range-image contract (include/pct_engine.h, paragraph "Range images"): the pseudo-angle, the projection,
the seen-through test, the un-projection, a nearest-return renderer (test side only: the library renders nothing) and a window model
on ring_remove_model.RemoveWindow -- the reference of tests/test_range_api.py, tests/test_range_model.py and tests/test_gpu_range.py.
Every expression is fp64 from float-widened operands, one numpy operation per rounding, in the order the header writes it; no sin,
cos or atan2 appears in the model either: angles reach it only as the view's tables."""
import numpy as np

import ring_remove_model as R


def _view(view):
    """(t [3], R [3, 3], near_range, width, height, col_edge, row_edge, col_dir or None, row_dir or None) of a pct_range_view, the
    tables read through the struct's own pointers"""
    w, h = int(view.width), int(view.height)

    def table(p, n):
        return np.ctypeslib.as_array(p, shape=(n,)).astype(np.float64) if p else None

    cd, rd = table(view.col_dir, 2 * w), table(view.row_dir, 2 * h)
    return (np.array(list(view.t), np.float64), np.array(list(view.R), np.float64).reshape(3, 3), np.float64(view.near_range), w, h,
            table(view.col_edge, w + 1), table(view.row_edge, h + 1), None if cd is None else cd.reshape(w, 2),
            None if rd is None else rd.reshape(h, 2))


def pseudo_angle(x, y):
    """den = |x| + |y|; NaN when den is 0 or not finite; p = y / den; x < 0: 2 - p; else y < 0: 4 + p; else p"""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        den = np.abs(x) + np.abs(y)
        p = y / den
        out = np.where(x < 0.0, 2.0 - p, np.where(y < 0.0, 4.0 + p, p))
        return np.where((den == 0.0) | ~np.isfinite(den), np.nan, out)


def project(view, xyz):
    """rows of fp32 points -> dict(inside bool [n], row / col int64 [n] (-1 outside), r2, a, q, h)"""
    t, Rm, near, w, h, ce, re_, _, _ = _view(view)
    p = np.asarray(xyz, np.float32).reshape(-1, 3).astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        d = p - t
        r2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        s = [(d[:, 0] * Rm[0, k] + d[:, 1] * Rm[1, k]) + d[:, 2] * Rm[2, k] for k in range(3)]
        hh = np.sqrt(s[0] * s[0] + s[1] * s[1])
        a = pseudo_angle(s[0], s[1])
        q = s[2] / hh
        inside = (r2 >= near * near) & (r2 < np.inf) & (hh > 0.0) & (a >= ce[0]) & (a < ce[w]) & (q >= re_[0]) & (q < re_[h])
    # the counts of the contract: entries <= the value, minus one (searchsorted side="right" counts them; a NaN is not inside)
    col = np.where(inside, np.searchsorted(ce, np.where(inside, a, ce[0]), side="right") - 1, -1).astype(np.int64)
    row = np.where(inside, np.searchsorted(re_, np.where(inside, q, re_[0]), side="right") - 1, -1).astype(np.int64)
    return dict(inside=inside, row=row, col=col, r2=r2, a=a, q=q, h=hh)


def seen(view, image, xyz, margin):
    """which rows the scan sees through (strict; a non-finite pixel proves nothing; w <= 0 proves nothing)"""
    w, h = int(view.width), int(view.height)
    img = np.asarray(image, np.float32).reshape(h, w)
    pr = project(view, xyz)
    val = img[np.maximum(pr["row"], 0), np.maximum(pr["col"], 0)].astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        wv = val - np.float64(margin)
        nearer = (wv > 0.0) & (pr["r2"] < wv * wv)
    return pr["inside"] & np.isfinite(val) & nearer


def unproject(view, image, max_range=np.inf):
    """(valid bool [height * width], fp32 points [valid.sum(), 3] in row-major pixel order)"""
    t, Rm, near, w, h, _, _, cd, rd = _view(view)
    if cd is None or rd is None:
        raise ValueError("un-projection needs col_dir and row_dir")
    rho = np.asarray(image, np.float32).reshape(h * w).astype(np.float64)
    with np.errstate(invalid="ignore"):
        valid = np.isfinite(rho) & (rho >= near) & (rho <= np.float64(max_range))
    r, c = np.divmod(np.arange(h * w), w)
    e0, e1, e2 = rd[r, 0] * cd[c, 0], rd[r, 0] * cd[c, 1], rd[r, 1]
    with np.errstate(invalid="ignore", over="ignore"):
        pts = np.stack([t[k] + rho * ((e0 * Rm[k, 0] + e1 * Rm[k, 1]) + e2 * Rm[k, 2]) for k in range(3)], axis=1).astype(np.float32)
    return valid, pts[valid]


def classify(views, images, points, margin):
    """(seen_by int32 [n], pixel int32 [n, 2] = (c, r)): planner points narrowed to fp32 first; the lowest view that sees the point
    through, and its pixel in the LAST view (-1, -1 when it is not in that image)"""
    with np.errstate(over="ignore"):
        p = np.asarray(points, np.float64).reshape(-1, 3).astype(np.float32)
    seen_by = np.full(len(p), -1, np.int32)
    for k in reversed(range(len(views))):
        seen_by[seen(views[k], images[k], p, margin)] = k
    pr = project(views[-1], p)
    return seen_by, np.stack([pr["col"], pr["row"]], axis=1).astype(np.int32)


def render(view, points):
    """a scan of points: every pixel holds the fp32 range of the nearest point that projects onto it, +inf where none does"""
    w, h = int(view.width), int(view.height)
    pr = project(view, points)
    img = np.full(h * w, np.inf, np.float32)
    ok = pr["inside"]
    np.minimum.at(img, (pr["row"] * w + pr["col"])[ok], np.sqrt(pr["r2"][ok]).astype(np.float32))
    return img.reshape(h, w)


class RangeWindow(R.RemoveWindow):
    """RemoveWindow fed range images: carve = a removal by the seen-through predicate, append_range = an append of the un-projected
    frame (de-duplicating when dedup is on, plain otherwise).  The camelCase members are those of the corridor finder."""

    def __init__(self, cap, res=R.M.RES, dedup=True):
        super().__init__(cap, res)
        self.dedup = dedup

    def carve(self, view, image, margin):
        return self._remove(seen(view, image, self.live(), margin))

    def append_range(self, view, image, max_range=np.inf):
        """returns (the frame = the valid pixels un-projected, the kept flags over it)"""
        _, frame = unproject(view, image, max_range)
        if len(frame) > self.cap:
            raise OverflowError("more valid pixels than the window's capacity")
        if self.dedup:
            return frame, self.append(frame)
        self.append_plain(frame)
        return frame, np.ones(len(frame), bool)

    def clearSeenThroughRange(self, view, image, margin):
        return self.carve(view, image, margin)

    def appendRangeImage(self, view, image, max_range=np.inf):
        return int(self.append_range(view, image, max_range)[1].sum())
