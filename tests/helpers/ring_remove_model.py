"""numpy restatement of removing points from the rolling map (include/pct_engine.h, paragraph "Removing points"): the de-dup window
of ring_dedup_model.py plus NaN tombstones, the three predicates in the contract's exact arithmetic, and the empty-window reset --
the reference model of tests/test_ring_remove_api.py and tests/test_gpu_ring_remove.py."""
import numpy as np

import ring_dedup_model as M


def has_nan(xyz):
    return np.isnan(np.asarray(xyz, np.float32).reshape(-1, 3)).any(axis=1)


def in_ball(xyz, centre, r):
    """((dx*dx + dy*dy) + dz*dz) <= r*r with dx = (double)x - centre[0], fp64, one rounding per operation"""
    p = np.asarray(xyz, np.float32).reshape(-1, 3).astype(np.float64)
    c = np.asarray(centre, np.float64).reshape(3)
    with np.errstate(invalid="ignore", over="ignore"):
        dx, dy, dz = p[:, 0] - c[0], p[:, 1] - c[1], p[:, 2] - c[2]
        d2 = (dx * dx + dy * dy) + dz * dz
        return d2 <= np.float64(r) * np.float64(r)


def in_box(xyz, lo, hi):
    """lo[k] <= (double)p[k] <= hi[k] on all three axes"""
    p = np.asarray(xyz, np.float32).reshape(-1, 3).astype(np.float64)
    lo, hi = np.asarray(lo, np.float64).reshape(3), np.asarray(hi, np.float64).reshape(3)
    with np.errstate(invalid="ignore"):
        return np.all((lo <= p) & (p <= hi), axis=1)


class RemoveWindow(M.DedupWindow):
    """DedupWindow whose slots can be removed: a removed slot is a NaN row (keyless, so it holds no voxel); size, capacity and the
    cursor do not move, except that a removal which leaves no row without a NaN empties the window (size 0, cursor at slot 0)"""

    def __init__(self, cap, res=M.RES):
        super().__init__(cap, res)
        self.removed = self.resets = 0

    def live_mask(self):
        return ~has_nan(self.live())

    def live_count(self):
        return int(self.live_mask().sum())

    def live_set(self):
        return set(map(tuple, self.live()[self.live_mask()].tolist()))

    def _remove(self, mask):
        """mask over the rows below count; rows that already hold a NaN are left alone and not counted"""
        hit = np.asarray(mask, bool) & self.live_mask()
        n = int(hit.sum())
        self.xyz[:self.count][hit] = np.nan
        self.removed += n
        if n and self.live_count() == 0:
            self.count = self.nxt = 0
            self.resets += 1
        return n

    def remove_ball(self, centre, r, outside=False):
        inside = in_ball(self.live(), centre, r)
        return self._remove(~inside if outside else inside)

    def remove_box(self, lo, hi, outside=False):
        inside = in_box(self.live(), lo, hi)
        return self._remove(~inside if outside else inside)

    def remove_indices(self, idx, base=0):
        slots = np.asarray(idx, np.int64).reshape(-1) - int(base)
        if len(slots) and (slots.min() < 0 or slots.max() >= self.count):
            raise IndexError("an index is outside the window")
        mask = np.zeros(self.count, bool)
        mask[slots] = True
        return self._remove(mask)


def centres_of(name):
    """the sensor position of every frame of ring_dedup_model.frames_of(name): frames 20 and 21 hover at frame 19's, and the extra
    empty frame of B is sensed from the position of the frame before it"""
    from pointcloudtraj_amd import scenarios
    sc = M.SCENARIOS[name]
    out = []
    for t in range(sc["frames"]):
        s = sc["step"] * (19 if t in (20, 21) else t)
        out.append((scenarios.START[0] + s, scenarios.START[1] + s, scenarios.START[2]))
        if sc["empty_at"] == t:
            out.append(out[-1])
    return out


def run_lidar_window(name):
    """scenario `name` through a de-duplicating window with forget-outside after every append.  Returns the window and, per frame,
    dict(kept flags, removed, count, live set, live rows (copies counted), resets so far, cursor)"""
    sc = M.SCENARIOS[name]
    w = RemoveWindow(sc["cap"])
    steps = []
    for f, c in zip(M.frames_of(name), centres_of(name)):
        kept = w.append(f)
        removed = w.remove_ball(c, sc["radius"], outside=True)
        steps.append(dict(kept=kept, removed=removed, count=w.count, live=w.live_set(), rows=w.live_count(), resets=w.resets, nxt=w.nxt))
    return w, steps
