"""ctypes binding of libpct_corridor.so (include/pct_corridor.h): the safe-region RRT* corridor finder on
the engine, with the reference's method names (corridor_finder.h:81-149)."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import build as _build
from . import engine as _engine
from . import kdtree as _kdtree

_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(_build.CORRIDOR_SO):
            raise FileNotFoundError(f"{_build.CORRIDOR_SO} is missing: run __graft_entry__.build()")
        _engine.lib()
        _kdtree.lib()
        L = C.CDLL(_build.CORRIDOR_SO)
        vp, d3 = C.c_void_p, C.POINTER(C.c_double)
        L.pct_corridor_last_error.restype = C.c_char_p
        L.pct_corridor_create.argtypes = [C.c_int64, C.c_int, C.POINTER(vp)]
        L.pct_corridor_destroy.argtypes = [vp]
        L.pct_corridor_set_param.argtypes = [vp, C.c_double, C.c_double, C.c_double, C.c_double]
        L.pct_corridor_reset.argtypes = [vp]
        L.pct_corridor_set_speculation.argtypes = [vp, C.c_int]
        L.pct_corridor_speculation_stats.argtypes = [vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        L.pct_corridor_set_fused_expansion.argtypes = [vp, C.c_int]
        L.pct_corridor_expansion_launches.argtypes = [vp, C.POINTER(C.c_uint64)]
        L.pct_corridor_repair_batches.argtypes = [vp, C.POINTER(C.c_uint64)]
        L.pct_corridor_set_input.argtypes = [vp, vp, C.c_int64, C.c_int64, C.c_int]
        L.pct_corridor_enable_rolling.argtypes = [vp, C.c_float, vp]
        L.pct_corridor_append_input.argtypes = [vp, vp, C.c_int64, C.c_int64]
        L.pct_corridor_set_rolling_dedup.argtypes = [vp, C.c_double]
        L.pct_corridor_forget_outside.argtypes = [vp, d3, C.c_double, C.POINTER(C.c_int64)]
        L.pct_corridor_compact_window.argtypes = [vp, C.POINTER(C.c_int64)]
        L.pct_corridor_set_rolling_compact.argtypes = [vp, C.c_double]
        L.pct_corridor_clear_ball.argtypes = [vp, d3, C.c_double, C.POINTER(C.c_int64)]
        L.pct_corridor_clear_box.argtypes = [vp, d3, d3, C.POINTER(C.c_int64)]
        L.pct_corridor_remove_outliers.argtypes = [vp, C.c_double, C.c_int32, C.c_int64, C.POINTER(C.c_int64)]
        L.pct_corridor_remove_statistical.argtypes = [vp, C.c_int32, C.c_double, C.c_int64, C.POINTER(C.c_int64), C.POINTER(_engine.KnnStats)]
        L.pct_corridor_remove_isolated.argtypes = [vp, C.c_int32, C.c_double, C.c_int64, C.POINTER(C.c_int64)]
        L.pct_corridor_clear_seen_through.argtypes = [vp, vp, vp, C.c_double, C.POINTER(C.c_int64)]
        L.pct_corridor_append_depth.argtypes = [vp, vp, vp, C.c_double, C.POINTER(C.c_int64)]
        L.pct_corridor_clear_seen_through_range.argtypes = [vp, vp, vp, C.c_double, C.POINTER(C.c_int64)]
        L.pct_corridor_append_range.argtypes = [vp, vp, vp, C.c_double, C.POINTER(C.c_int64)]
        L.pct_corridor_cloud.argtypes = [vp, C.POINTER(vp)]
        L.pct_corridor_set_pt.argtypes = [vp, d3, d3] + [C.c_double] * 7 + [C.c_int, C.c_double, C.c_double]
        L.pct_corridor_set_start_pt.argtypes = [vp, d3, d3]
        L.pct_corridor_reset_root.argtypes = [vp, d3]
        L.pct_corridor_expansion.argtypes = [vp, C.c_int64]
        L.pct_corridor_refine.argtypes = [vp, C.c_int64]
        L.pct_corridor_evaluate.argtypes = [vp]
        L.pct_corridor_expansion_timed.argtypes = [vp, C.c_double, C.POINTER(C.c_int64)]
        L.pct_corridor_refine_timed.argtypes = [vp, C.c_double, C.POINTER(C.c_int64)]
        L.pct_corridor_evaluate_timed.argtypes = [vp, C.c_double]
        L.pct_corridor_check_traj_pt_col.argtypes = [vp, d3, C.POINTER(C.c_int)]
        L.pct_corridor_get_path.argtypes = [vp, vp, vp, C.c_int64, C.POINTER(C.c_int64)]
        L.pct_corridor_status.argtypes = [vp, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int64), C.POINTER(C.c_uint64)]
        L.pct_corridor_get_tree.argtypes = [vp] + [vp] * 6 + [C.c_int64, C.POINTER(C.c_int64)]
        L.pct_corridor_debug_counters.argtypes = [vp, C.POINTER(C.c_uint64)]
        _lib = L
    return _lib


def _d3(v):
    return (C.c_double * 3)(*[float(x) for x in v])


class SafeRegionRrtStar:
    def __init__(self, cloud_capacity: int = 1 << 20, device: int = 0):
        self.L = lib()
        self.h = C.c_void_p()
        self._chk(self.L.pct_corridor_create(int(cloud_capacity), device, C.byref(self.h)))

    def _chk(self, rc):
        if rc:
            raise RuntimeError("pct_corridor: " + self.L.pct_corridor_last_error().decode(errors="replace"))

    def close(self):
        if getattr(self, "h", None) and self.h.value and _lib is not None:
            _lib.pct_corridor_destroy(self.h)
            self.h = C.c_void_p()

    __del__ = close

    def setParam(self, safety_margin, search_margin, max_radius, sample_range):
        self._chk(self.L.pct_corridor_set_param(self.h, safety_margin, search_margin, max_radius, sample_range))

    def reset(self):
        self._chk(self.L.pct_corridor_reset(self.h))

    def setSpeculation(self, k: int):
        self._chk(self.L.pct_corridor_set_speculation(self.h, int(k)))

    def setFusedExpansion(self, on: bool):
        self._chk(self.L.pct_corridor_set_fused_expansion(self.h, int(bool(on))))

    def expansionLaunches(self) -> int:
        n = C.c_uint64()
        self._chk(self.L.pct_corridor_expansion_launches(self.h, C.byref(n)))
        return n.value

    def repairBatches(self) -> int:
        n = C.c_uint64()
        self._chk(self.L.pct_corridor_repair_batches(self.h, C.byref(n)))
        return n.value

    def speculationStats(self):
        a, b = C.c_uint64(), C.c_uint64()
        self._chk(self.L.pct_corridor_speculation_stats(self.h, C.byref(a), C.byref(b)))
        return dict(replayed_from_batch=a.value, fell_back=b.value)

    def setInput(self, points, build_index=True):
        a = np.ascontiguousarray(points, np.float32)
        self._chk(self.L.pct_corridor_set_input(self.h, a.ctypes.data_as(C.c_void_p), len(a), a.shape[1] * 4, int(build_index)))

    def enableRollingMap(self, cell_size: float = 0.0, extent=None):
        """rolling map (config C5): the cloud becomes a sliding window of cloud_capacity points over the rolling-map index; call once,
        before the first frame.  extent = the window's size per axis when known (the table is then allocated at once)"""
        ext = None if extent is None else np.ascontiguousarray(extent, np.float32).reshape(3)
        self._chk(self.L.pct_corridor_enable_rolling(self.h, float(cell_size), None if ext is None else ext.ctypes.data_as(C.c_void_p)))

    def appendInput(self, points):
        """append one sensor frame: the newest points overwrite the oldest, the index is updated in place"""
        a = np.ascontiguousarray(points, np.float32)
        self._chk(self.L.pct_corridor_append_input(self.h, a.ctypes.data_as(C.c_void_p), len(a), a.shape[1] * 4))

    def setRollingDedup(self, res: float):
        """after enableRollingMap: appendInput keeps only points whose voxel of size res is new to the window (0 = off)"""
        self._chk(self.L.pct_corridor_set_rolling_dedup(self.h, float(res)))

    def forgetOutside(self, centre, r: float) -> int:
        """after enableRollingMap: remove every point farther than r from centre (the lidar-mode tick: appendInput -> forgetOutside
        -> SafeRegionEvaluate -> SafeRegionRefine); returns the number of points removed"""
        n = C.c_int64()
        self._chk(self.L.pct_corridor_forget_outside(self.h, _d3(centre), float(r), C.byref(n)))
        return n.value

    def compactWindow(self) -> int:
        """after enableRollingMap: move the live points of the window to its first slots, oldest first, so that the next frames fill
        the slots of removed points instead of evicting live ones; returns the number of slots reclaimed"""
        n = C.c_int64()
        self._chk(self.L.pct_corridor_compact_window(self.h, C.byref(n)))
        return n.value

    def setRollingCompact(self, dead_fraction: float):
        """after enableRollingMap: every removal compacts the window by itself once dead_fraction of the capacity is dead (0 = off)"""
        self._chk(self.L.pct_corridor_set_rolling_compact(self.h, float(dead_fraction)))

    def clearBall(self, centre, r: float) -> int:
        """after enableRollingMap: remove the points within r of centre (a stale obstacle); returns the number removed"""
        n = C.c_int64()
        self._chk(self.L.pct_corridor_clear_ball(self.h, _d3(centre), float(r), C.byref(n)))
        return n.value

    def removeOutliers(self, r: float, min_neighbours: int, newest: int = 0) -> int:
        """after enableRollingMap: of the `newest` most recent points (0: every point), remove those with fewer than min_neighbours
        other points of the window within r (the noisy-sensor tick: clearSeenThrough -> appendDepthImage -> removeOutliers ->
        SafeRegionEvaluate -> SafeRegionRefine, newest = what the append kept); returns the number removed"""
        n = C.c_int64()
        self._chk(self.L.pct_corridor_remove_outliers(self.h, float(r), int(min_neighbours), int(newest), C.byref(n)))
        return n.value

    def removeStatisticalOutliers(self, k: int, stddev_mult: float, newest: int = 0):
        """after enableRollingMap: of the `newest` most recent points (0: every point), remove those whose mean distance to their k
        nearest other points is greater than mean + stddev_mult * stddev over the judged points; returns (removed, dict(measured, sum,
        sum_sq, mean, stddev, threshold)) -- the threshold is what removeIsolated takes in the frames that follow"""
        n, st = C.c_int64(), _engine.KnnStats()
        self._chk(self.L.pct_corridor_remove_statistical(self.h, int(k), float(stddev_mult), int(newest), C.byref(n), C.byref(st)))
        return n.value, st.as_dict()

    def removeIsolated(self, k: int, max_mean_distance: float, newest: int = 0) -> int:
        """after enableRollingMap: the same removal under a fixed threshold (the noisy-sensor tick: clearSeenThrough -> appendDepthImage
        -> removeIsolated -> SafeRegionEvaluate -> SafeRegionRefine, newest = what the append kept); returns the number removed"""
        n = C.c_int64()
        self._chk(self.L.pct_corridor_remove_isolated(self.h, int(k), float(max_mean_distance), int(newest), C.byref(n)))
        return n.value

    def clearBox(self, lo, hi) -> int:
        """after enableRollingMap: remove the points inside the axis-aligned box [lo, hi]; returns the number removed"""
        n = C.c_int64()
        self._chk(self.L.pct_corridor_clear_box(self.h, _d3(lo), _d3(hi), C.byref(n)))
        return n.value

    def clearSeenThrough(self, view, image, margin: float) -> int:
        """after enableRollingMap: remove every point the depth image sees through (engine.DepthView; the rgbd tick:
        clearSeenThrough -> appendDepthImage -> SafeRegionEvaluate -> SafeRegionRefine); returns the number of points removed"""
        from . import engine
        img = engine.depth_image(view, image)
        n = C.c_int64()
        self._chk(self.L.pct_corridor_clear_seen_through(self.h, C.addressof(view), img.ctypes.data, float(margin), C.byref(n)))
        return n.value

    def appendDepthImage(self, view, image, max_depth: float = float("inf")) -> int:
        """after enableRollingMap: un-project the image's valid pixels on the device and append them as appendInput appends a point
        frame; returns the number of points the window took"""
        from . import engine
        img = engine.depth_image(view, image)
        n = C.c_int64()
        self._chk(self.L.pct_corridor_append_depth(self.h, C.addressof(view), img.ctypes.data, float(max_depth), C.byref(n)))
        return n.value

    def clearSeenThroughRange(self, view, image, margin: float) -> int:
        """after enableRollingMap: remove every point the lidar's range image sees through (engine.RangeView; the lidar tick:
        clearSeenThroughRange -> appendRangeImage -> SafeRegionEvaluate -> SafeRegionRefine); returns the number of points removed"""
        from . import engine
        img = engine.depth_image(view, image)
        n = C.c_int64()
        self._chk(self.L.pct_corridor_clear_seen_through_range(self.h, C.addressof(view), img.ctypes.data, float(margin), C.byref(n)))
        return n.value

    def appendRangeImage(self, view, image, max_range: float = float("inf")) -> int:
        """after enableRollingMap: un-project the scan's valid pixels on the device and append them as appendInput appends a point
        frame; returns the number of points the window took"""
        from . import engine
        img = engine.depth_image(view, image)
        n = C.c_int64()
        self._chk(self.L.pct_corridor_append_range(self.h, C.addressof(view), img.ctypes.data, float(max_range), C.byref(n)))
        return n.value

    def cloud(self):
        """the finder's obstacle cloud as an engine.Cloud that does not own it (pct_corridor_cloud): for reading the window back
        (radius_crop, ring_live); replaced by a setInput that has to grow the map"""
        from . import engine
        h = C.c_void_p()
        self._chk(self.L.pct_corridor_cloud(self.h, C.byref(h)))
        return engine.Cloud.borrowed(h)

    def setPt(self, start, end, xl, xh, yl, yh, zl, zh, local_range, max_iter, sample_portion, goal_portion):
        self._chk(self.L.pct_corridor_set_pt(self.h, _d3(start), _d3(end), xl, xh, yl, yh, zl, zh, local_range, int(max_iter),
                                             sample_portion, goal_portion))

    def setStartPt(self, start, end):
        self._chk(self.L.pct_corridor_set_start_pt(self.h, _d3(start), _d3(end)))

    def resetRoot(self, target):
        self._chk(self.L.pct_corridor_reset_root(self.h, _d3(target)))

    # The reference's three entry points take seconds of wall clock (corridor_finder.h:97-99): pass a float.  An int is an
    # iteration count (the deterministic form, C++: ExpansionIterations / RefineIterations / EvaluateOnce).  The timed forms return
    # the number of samples they consumed.
    def ExpansionIterations(self, iterations: int):
        self._chk(self.L.pct_corridor_expansion(self.h, int(iterations)))

    def RefineIterations(self, iterations: int):
        self._chk(self.L.pct_corridor_refine(self.h, int(iterations)))

    def EvaluateOnce(self):
        self._chk(self.L.pct_corridor_evaluate(self.h))

    def SafeRegionExpansion(self, limit):
        if isinstance(limit, (int, np.integer)):
            return self.ExpansionIterations(limit)
        n = C.c_int64()
        self._chk(self.L.pct_corridor_expansion_timed(self.h, float(limit), C.byref(n)))
        return n.value

    def SafeRegionRefine(self, limit):
        if isinstance(limit, (int, np.integer)):
            return self.RefineIterations(limit)
        n = C.c_int64()
        self._chk(self.L.pct_corridor_refine_timed(self.h, float(limit), C.byref(n)))
        return n.value

    def SafeRegionEvaluate(self, time_limit=None):
        if time_limit is None:
            return self.EvaluateOnce()
        self._chk(self.L.pct_corridor_evaluate_timed(self.h, float(time_limit)))

    def checkTrajPtCol(self, p) -> bool:
        c = C.c_int()
        self._chk(self.L.pct_corridor_check_traj_pt_col(self.h, _d3(p), C.byref(c)))
        return bool(c.value)

    def getPath(self):
        n = C.c_int64()
        path = np.zeros((4096, 3)); rad = np.zeros(4096)
        self._chk(self.L.pct_corridor_get_path(self.h, path.ctypes.data_as(C.c_void_p), rad.ctypes.data_as(C.c_void_p), 4096, C.byref(n)))
        return path[:n.value].copy(), rad[:n.value].copy()

    def getTree(self):
        """test hook (pct_corridor_get_tree): the live spheres in insertion order as a dict of arrays -- centre f64 [n, 3], radius / g /
        f f32 [n], parent i32 [n] (row of the parent, -1 = none), flags u8 [n] (bit0 valid, bit1 on the best route)"""
        n = C.c_int64()
        self._chk(self.L.pct_corridor_get_tree(self.h, None, None, None, None, None, None, 0, C.byref(n)))
        k = n.value
        t = dict(centre=np.zeros((k, 3)), radius=np.zeros(k, np.float32), g=np.zeros(k, np.float32), f=np.zeros(k, np.float32),
                 parent=np.zeros(k, np.int32), flags=np.zeros(k, np.uint8))
        self._chk(self.L.pct_corridor_get_tree(self.h, *[t[key].ctypes.data_as(C.c_void_p) for key in ("centre", "radius", "g", "f", "parent", "flags")],
                                               k, C.byref(n)))
        return t

    def debugCounters(self):
        """test hook (pct_corridor_debug_counters): which branches have run since the finder was created"""
        out = (C.c_uint64 * 4)()
        self._chk(self.L.pct_corridor_debug_counters(self.h, out))
        return dict(truncated_lists=out[0], fused_refused=out[1], grow_one=out[2], max_kd_size=out[3])

    def status(self):
        pe, gn, nn, ni = C.c_int(), C.c_int(), C.c_int64(), C.c_uint64()
        self._chk(self.L.pct_corridor_status(self.h, C.byref(pe), C.byref(gn), C.byref(nn), C.byref(ni)))
        return dict(path_exists=bool(pe.value), global_navi=bool(gn.value), nodes=nn.value, inflation_queries=ni.value)
