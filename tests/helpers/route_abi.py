"""ctypes declarations for the tests of the routed multi-GPU search: the device phases of include/pct_engine.h (which have no Python
binding: their only caller is csrc/shard.cpp) and the one-process world of include/pct_shard.h.  Device buffers are torch tensors of
bytes; every output buffer is allocated at its documented size plus a guard tail of GUARD elements and filled with the byte 0xA5, so
that "not written" can be told from "written with 0" and a write past the end is seen."""
import contextlib
import ctypes as C

import numpy as np
import torch  # before the engine: one HIP runtime per process (engine._preload_hip_runtime)

from pointcloudtraj_amd import engine as E
from pointcloudtraj_amd import shard as SH

OK, INVALID, CAPACITY = 0, 2, 6
NO_INDEX = 0xFFFFFFFF
GUARD = 64
FILL = 0xA5
FILL_U32 = 0xA5A5A5A5

_vp, _i64, _int, _dbl = C.c_void_p, C.c_int64, C.c_int, C.c_double
_engine = None
_shard = None


def engine():
    """engine.lib() with argtypes for the ten entry points the routed form uses, after E.init(0)"""
    global _engine
    if _engine is None:
        E.init(0)
        L = E.lib()
        L.pct_cloud_upload_aos_dev.argtypes = [_vp, _vp, _i64, _i64]
        L.pct_route_owner_dev.argtypes = [_vp, _int, _int, _int, _vp, _i64, _vp, _vp, _vp, _vp]
        L.pct_route_owner_all_dev.argtypes = [_vp, _int, _int, _vp, _i64, _vp, _vp, _vp]
        L.pct_route_partition_dev.argtypes = [_vp, _int, _vp, _vp, _i64, _vp, _vp, _vp, _vp]
        L.pct_route_certify_dev.argtypes = [_int, _dbl, _dbl, _vp, _vp, _i64, _vp, _vp, _vp, _vp, _vp]
        L.pct_route_scatter_dev.argtypes = [_vp, _i64, _vp, _vp, _vp, _vp, _vp]
        L.pct_route_gather_queries_dev.argtypes = [_vp, _vp, _i64, _vp, _vp]
        L.pct_route_to_global_dev.argtypes = [_vp, _i64, _vp, _vp]
        L.pct_route_put_back_dev.argtypes = [_vp, _i64, _vp, _vp, _vp, _vp, _vp]
        L.pct_merge_finish_dev.argtypes = [_vp, _vp, _i64, _vp]
        for name in ("pct_cloud_upload_aos_dev", "pct_route_owner_dev", "pct_route_owner_all_dev", "pct_route_partition_dev", "pct_route_certify_dev",
                     "pct_route_scatter_dev", "pct_route_gather_queries_dev", "pct_route_to_global_dev", "pct_route_put_back_dev", "pct_merge_finish_dev"):
            getattr(L, name).restype = _int
        _engine = L
    return _engine


def shard():
    """shard.lib() with argtypes for the one-process world"""
    global _shard
    if _shard is None:
        engine()
        L = SH.lib()
        pvp = C.POINTER(_vp)
        L.pct_shard_local_world.argtypes = [_int, pvp]
        L.pct_shard_route_build_world.argtypes = [pvp, _int, pvp, C.POINTER(_i64), _i64, C.POINTER(_i64), _dbl, pvp]
        L.pct_shard_route_nn_world.argtypes = [pvp, _int, _vp, _i64, pvp, pvp, _vp]
        L.pct_shard_route_nn_partitioned_world.argtypes = [pvp, _int, pvp, C.POINTER(_i64), pvp, pvp, _vp]
        L.pct_shard_route_stats.argtypes = [_vp, C.POINTER(_i64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        L.pct_shard_route_destroy.argtypes = [_vp]
        L.pct_shard_destroy.argtypes = [_vp]
        _shard = L
    return _shard


def stream():
    return torch.cuda.current_stream().cuda_stream


def sync():
    torch.cuda.synchronize()


# ---- device buffers -----------------------------------------------------------------------------------------------------------------
def dev(a):
    """a host array's bytes on the device"""
    a = np.ascontiguousarray(a)
    t = torch.from_numpy(a.reshape(-1).view(np.uint8).copy()).cuda() if a.size else torch.empty(0, dtype=torch.uint8, device="cuda")
    sync()
    return t


def out(n, dtype):
    """an output buffer of n elements + GUARD guard elements, every byte FILL"""
    t = torch.full(((int(n) + GUARD) * np.dtype(dtype).itemsize,), FILL, dtype=torch.uint8, device="cuda")
    sync()
    return t


def ptr(t):
    return t.data_ptr() if t is not None and t.numel() else None


def host(t, dtype):
    sync()
    return t.cpu().numpy().view(dtype)


def untouched(a):
    """every byte of a (part of a) buffer read back still holds the fill"""
    return bool((np.ascontiguousarray(a).view(np.uint8) == FILL).all())


def host_ptr(a):
    return a.ctypes.data_as(_vp)


# ---- the one-process world ----------------------------------------------------------------------------------------------------------
class World:
    """`world` ranks in this process and their routes over a cloud dealt to them as `parts` (one (n_k, 3) fp32 array per rank, rows in
    global order: index_begin is the running sum); records of `stride` bytes.  Use through local_world(): everything is released in a
    finally."""

    def __init__(self, parts, stride=12, halo=4.0):
        L = shard()
        W = self.world = len(parts)
        self.ranks = (_vp * W)()
        self.routes = (_vp * W)()
        rc = L.pct_shard_local_world(W, self.ranks)
        assert rc == OK, (rc, E.lib().pct_last_error())
        self.rows = []
        for k, p in enumerate(parts):                                  # x, y, z at the start of every record; the rest is not the library's to read
            p = np.ascontiguousarray(p, np.float32).reshape(-1, 3)
            rec = np.full((len(p), stride // 4), np.float32(-7e33), np.float32)
            rec[:, :3] = p
            self.rows.append(rec)
        n = (_i64 * W)(*[len(r) for r in self.rows])
        begin = (_i64 * W)(*np.concatenate([[0], np.cumsum([len(r) for r in self.rows])[:-1]]).astype(np.int64).tolist())
        pts = (_vp * W)(*[r.ctypes.data if len(r) else None for r in self.rows])
        rc = L.pct_shard_route_build_world(self.ranks, W, pts, n, stride, begin, float(halo), self.routes)
        assert rc == OK, (rc, E.lib().pct_last_error())

    def nn(self, q):
        """a replicated batch: [(idx uint32[Q + GUARD], d2 float64[Q + GUARD])] per rank, guard tails included; the status"""
        L = shard()
        q = np.ascontiguousarray(q, np.float32).reshape(-1, 3)
        Q, W = len(q), self.world
        dq = dev(q)
        oi, od = [out(Q, np.uint32) for _ in range(W)], [out(Q, np.float64) for _ in range(W)]
        rc = L.pct_shard_route_nn_world(self.routes, W, ptr(dq), Q, (_vp * W)(*[t.data_ptr() for t in oi]), (_vp * W)(*[t.data_ptr() for t in od]), stream())
        sync()
        return rc, [(host(oi[k], np.uint32), host(od[k], np.float64)) for k in range(W)]

    def nn_partitioned(self, qs):
        """every rank's own batch (qs[k]: (Q_k, 3)): the status and [(idx, d2)] per rank as above"""
        L = shard()
        W = self.world
        qs = [np.ascontiguousarray(q, np.float32).reshape(-1, 3) for q in qs]
        dq = [dev(q) for q in qs]
        oi, od = [out(len(q), np.uint32) for q in qs], [out(len(q), np.float64) for q in qs]
        rc = L.pct_shard_route_nn_partitioned_world(self.routes, W, (_vp * W)(*[ptr(t) for t in dq]), (_i64 * W)(*[len(q) for q in qs]),
                                                    (_vp * W)(*[t.data_ptr() for t in oi]), (_vp * W)(*[t.data_ptr() for t in od]), stream())
        sync()
        return rc, [(host(oi[k], np.uint32), host(od[k], np.float64)) for k in range(W)]

    def stats(self):
        """per rank: dict(slab_points, owned, uncertified, batches)"""
        res = []
        for k in range(self.world):
            sp, ow, un, ba = _i64(), C.c_uint64(), C.c_uint64(), C.c_uint64()
            assert shard().pct_shard_route_stats(self.routes[k], C.byref(sp), C.byref(ow), C.byref(un), C.byref(ba)) == OK
            res.append(dict(slab_points=sp.value, owned=ow.value, uncertified=un.value, batches=ba.value))
        return res

    def close(self):
        L = shard()
        sync()
        for k in range(self.world):
            if self.routes[k]:
                L.pct_shard_route_destroy(self.routes[k])
                self.routes[k] = None
            if self.ranks[k]:
                L.pct_shard_destroy(self.ranks[k])
                self.ranks[k] = None


@contextlib.contextmanager
def local_world(parts, stride=12, halo=4.0):
    w = World.__new__(World)
    w.world, w.ranks, w.routes = 0, (), ()
    try:
        w.__init__(parts, stride, halo)
        yield w
    finally:
        w.close()
