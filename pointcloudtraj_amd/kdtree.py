"""ctypes binding of the drop-in libkdtree.so (include/kdtree/kdtree.h): the reference's kd_*
API served by the GPU engine.  Used by the parity tests the way corridor_finder.cpp uses the
C API (kd_insertf / kd_nearestf / kd_nearest_rangef / kd_res_*)."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import build as _build
from . import engine as _engine

_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(_build.KDTREE_SO):
            raise FileNotFoundError(f"{_build.KDTREE_SO} is missing: run __graft_entry__.build()")
        _engine.lib()      # loads the HIP runtime + libpct_engine.so first (same runtime as torch)
        L = C.CDLL(_build.KDTREE_SO)
        vp = C.c_void_p
        fp, dp = C.POINTER(C.c_float), C.POINTER(C.c_double)
        L.kd_create.restype = vp
        L.kd_create.argtypes = [C.c_int]
        L.kd_free.argtypes = [vp]
        L.kd_clear.argtypes = [vp]
        L.kd_data_destructor.argtypes = [vp, vp]
        L.kd_insert.argtypes = [vp, dp, vp]
        L.kd_insertf.argtypes = [vp, fp, vp]
        L.kd_insert3.argtypes = [vp, C.c_double, C.c_double, C.c_double, vp]
        L.kd_insert3f.argtypes = [vp, C.c_float, C.c_float, C.c_float, vp]
        for n in ("kd_nearest", "kd_nearestf", "kd_nearest3", "kd_nearest3f", "kd_nearest_range", "kd_nearest_rangef",
                  "kd_nearest_range3", "kd_nearest_range3f"):
            getattr(L, n).restype = vp
        L.kd_nearest.argtypes = [vp, dp]
        L.kd_nearestf.argtypes = [vp, fp]
        L.kd_nearest3.argtypes = [vp, C.c_double, C.c_double, C.c_double]
        L.kd_nearest3f.argtypes = [vp, C.c_float, C.c_float, C.c_float]
        L.kd_nearest_range.argtypes = [vp, dp, C.c_double]
        L.kd_nearest_rangef.argtypes = [vp, fp, C.c_float]
        L.kd_nearest_range3.argtypes = [vp, C.c_double, C.c_double, C.c_double, C.c_double]
        L.kd_nearest_range3f.argtypes = [vp, C.c_float, C.c_float, C.c_float, C.c_float]
        for n in ("kd_res_free", "kd_res_size", "kd_res_rewind", "kd_res_end", "kd_res_next"):
            getattr(L, n).argtypes = [vp]
        for n in ("kd_res_item", "kd_res_itemf", "kd_res_item3", "kd_res_item3f", "kd_res_item_data"):
            getattr(L, n).restype = vp
        L.kd_res_item.argtypes = [vp, dp]
        L.kd_res_itemf.argtypes = [vp, fp]
        L.kd_res_item3.argtypes = [vp, dp, dp, dp]
        L.kd_res_item3f.argtypes = [vp, fp, fp, fp]
        L.kd_res_item_data.argtypes = [vp]
        L.kdx_set_host_threshold.argtypes = [C.c_int64]
        L.kdx_host_threshold.restype = C.c_int64
        L.kdx_size.argtypes = [vp]
        L.kdx_nearestf_batch.argtypes = [vp, vp, C.c_int, vp]
        L.kdx_range_candidates_batch.argtypes = [vp, vp, vp, C.c_int, vp, C.c_int, vp]
        L.kdx_range_from_candidates.restype = vp
        L.kdx_range_from_candidates.argtypes = [vp, fp, C.c_float, vp, C.c_int, C.c_int32]
        _lib = L
    return _lib


def set_host_threshold(nodes: int):
    """node sets of up to `nodes` nodes answer single queries on the host (0 = always the device; negative = the default)"""
    lib().kdx_set_host_threshold(int(nodes))


def host_threshold() -> int:
    return int(lib().kdx_host_threshold())


class KDTree:
    """Thin convenience wrapper; payload of point i is (void*)(i+1)."""

    def __init__(self):
        self.L = lib()
        self.h = self.L.kd_create(3)
        if not self.h:
            raise RuntimeError("kd_create failed (no HIP device?)")
        self.n = 0

    def close(self):
        if getattr(self, "h", None):
            self.L.kd_free(self.h)
            self.h = None

    __del__ = close

    def insert(self, xyz):
        xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
        for p in xyz:
            if self.L.kd_insertf(self.h, p.ctypes.data_as(C.POINTER(C.c_float)), C.c_void_p(self.n + 1)):
                raise MemoryError
            self.n += 1

    def nearest(self, q):
        """payload-derived ids and fp64 positions for each float query"""
        q = np.ascontiguousarray(q, np.float32).reshape(-1, 3)
        ids = np.empty(len(q), np.int32)
        pos = np.empty((len(q), 3), np.float64)
        for i, qq in enumerate(q):
            r = self.L.kd_nearestf(self.h, qq.ctypes.data_as(C.POINTER(C.c_float)))
            if not r:
                raise RuntimeError("kd_nearestf returned NULL")
            d = self.L.kd_res_item(r, pos[i].ctypes.data_as(C.POINTER(C.c_double)))
            ids[i] = int(d or 0) - 1
            self.L.kd_res_free(r)
        return ids, pos

    def range_ids(self, q, r):
        q = np.ascontiguousarray(q, np.float32).reshape(3)
        rs = self.L.kd_nearest_rangef(self.h, q.ctypes.data_as(C.POINTER(C.c_float)), C.c_float(r))
        if not rs:
            raise RuntimeError("kd_nearest_rangef returned NULL")
        out = []
        while not self.L.kd_res_end(rs):
            out.append(int(self.L.kd_res_item_data(rs) or 0) - 1)
            self.L.kd_res_next(rs)
        assert len(out) == self.L.kd_res_size(rs)
        self.L.kd_res_free(rs)
        return np.asarray(out, np.int32)

    def clear(self):
        self.L.kd_clear(self.h)
        self.n = 0

    def _one(self, r, what):
        """(payload-derived id, stored fp64 position) of a one-element result set, which is freed"""
        if not r:
            raise RuntimeError(f"{what} returned NULL")
        pos = np.empty(3, np.float64)
        d = self.L.kd_res_item(r, pos.ctypes.data_as(C.POINTER(C.c_double)))
        size = self.L.kd_res_size(r)
        self.L.kd_res_free(r)
        assert size == 1
        return int(d or 0) - 1, pos

    def _drain(self, rs, what, rewind=False):
        """ids of a range result in ITERATION order; the set is freed.  rewind: iterate, kd_res_rewind, iterate again -- both passes
        must agree"""
        if not rs:
            raise RuntimeError(f"{what} returned NULL")
        out = []
        for _ in range(2 if rewind else 1):
            out.append([])
            while not self.L.kd_res_end(rs):
                out[-1].append(int(self.L.kd_res_item_data(rs) or 0) - 1)
                self.L.kd_res_next(rs)
            self.L.kd_res_rewind(rs)
        size = self.L.kd_res_size(rs)
        self.L.kd_res_free(rs)
        assert all(o == out[0] for o in out) and len(out[0]) == size
        return np.asarray(out[0], np.int32)

    def nearest64(self, q):
        """kd_nearest with a double position: (id, stored fp64 position)"""
        q = np.ascontiguousarray(q, np.float64).reshape(3)
        return self._one(self.L.kd_nearest(self.h, q.ctypes.data_as(C.POINTER(C.c_double))), "kd_nearest")

    def nearest3(self, x, y, z):
        """kd_nearest3: (id, stored fp64 position)"""
        return self._one(self.L.kd_nearest3(self.h, float(x), float(y), float(z)), "kd_nearest3")

    def range_ids64(self, q, r, rewind=False):
        """kd_nearest_range with a double position and a double range: ids in iteration order"""
        q = np.ascontiguousarray(q, np.float64).reshape(3)
        return self._drain(self.L.kd_nearest_range(self.h, q.ctypes.data_as(C.POINTER(C.c_double)), C.c_double(r)), "kd_nearest_range", rewind)

    def range_ids3(self, x, y, z, r, rewind=False):
        """kd_nearest_range3: ids in iteration order"""
        return self._drain(self.L.kd_nearest_range3(self.h, float(x), float(y), float(z), float(r)), "kd_nearest_range3", rewind)

    # batch extensions (include/kdtree/kdtree_ext.h)
    def nearest_batch(self, q):
        """kdx_nearestf_batch: int32 [K], the lowest node number among the nearest of each float query, -1 for an empty tree"""
        q = np.ascontiguousarray(q, np.float32).reshape(-1, 3)
        out = np.empty(len(q), np.int32)
        if self.L.kdx_nearestf_batch(self.h, q.ctypes.data, len(q), out.ctypes.data):
            raise RuntimeError("kdx_nearestf_batch failed")
        return out

    def range_candidates_batch(self, q, ranges, cap_per_query: int):
        """kdx_range_candidates_batch against the tree as it is now: (ids uint32 [K, cap_per_query], counts int32 [K]); counts[i] >= 0
        candidates stored in row i (unordered), < 0: the row is truncated or the batch cannot serve this tree -- ask that query alone"""
        q = np.ascontiguousarray(q, np.float32).reshape(-1, 3)
        r = np.ascontiguousarray(np.broadcast_to(np.asarray(ranges, np.float32), (len(q),)))
        ids = np.full((len(q), int(cap_per_query)), 0xFFFFFFFF, np.uint32)
        counts = np.empty(len(q), np.int32)
        if self.L.kdx_range_candidates_batch(self.h, q.ctypes.data, r.ctypes.data, len(q), ids.ctypes.data, int(cap_per_query), counts.ctypes.data):
            raise RuntimeError("kdx_range_candidates_batch failed")
        return ids, counts

    def range_from_candidates(self, q, r, ids, n_snapshot: int):
        """kdx_range_from_candidates: the ids kd_nearest_rangef(q, r) iterates over NOW, from the candidates `ids` of a snapshot of
        n_snapshot nodes"""
        q = np.ascontiguousarray(q, np.float32).reshape(3)
        ids = np.ascontiguousarray(ids, np.uint32).reshape(-1)
        rs = self.L.kdx_range_from_candidates(self.h, q.ctypes.data_as(C.POINTER(C.c_float)), C.c_float(r), ids.ctypes.data, len(ids),
                                              int(n_snapshot))
        return self._drain(rs, "kdx_range_from_candidates")


class KDTreeN:
    """kd_* on a tree of any dimension with double positions (kd_create(k), kd_insert, kd_nearest, kd_nearest_range);
    payload of row i is (void*)(i+1)."""

    def __init__(self, dim: int):
        self.L = lib()
        self.dim = int(dim)
        self.h = self.L.kd_create(self.dim)
        if not self.h:
            raise RuntimeError(f"kd_create({dim}) failed")
        self.n = 0

    def close(self):
        if getattr(self, "h", None):
            self.L.kd_free(self.h)
            self.h = None

    __del__ = close

    def insert(self, rows):
        rows = np.ascontiguousarray(rows, np.float64).reshape(-1, self.dim)
        dp = C.POINTER(C.c_double)
        for p in rows:
            if self.L.kd_insert(self.h, p.ctypes.data_as(dp), C.c_void_p(self.n + 1)):
                raise MemoryError
            self.n += 1

    def nearest(self, q):
        q = np.ascontiguousarray(q, np.float64).reshape(-1, self.dim)
        ids = np.empty(len(q), np.int32)
        pos = np.empty((len(q), self.dim), np.float64)
        dp = C.POINTER(C.c_double)
        for i, qq in enumerate(q):
            r = self.L.kd_nearest(self.h, qq.ctypes.data_as(dp))
            if not r:
                raise RuntimeError("kd_nearest returned NULL")
            d = self.L.kd_res_item(r, pos[i].ctypes.data_as(dp))
            ids[i] = int(d or 0) - 1
            self.L.kd_res_free(r)
        return ids, pos

    def range_ids(self, q, r):
        q = np.ascontiguousarray(q, np.float64).reshape(self.dim)
        rs = self.L.kd_nearest_range(self.h, q.ctypes.data_as(C.POINTER(C.c_double)), C.c_double(r))
        if not rs:
            raise RuntimeError("kd_nearest_range returned NULL")
        out = []
        while not self.L.kd_res_end(rs):
            out.append(int(self.L.kd_res_item_data(rs) or 0) - 1)
            self.L.kd_res_next(rs)
        assert len(out) == self.L.kd_res_size(rs)
        self.L.kd_res_free(rs)
        return np.asarray(out, np.int32)
