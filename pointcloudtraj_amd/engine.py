"""ctypes binding of libpct_engine.so (include/pct_engine.h) -- the host-side mirror used by the
tests, bench.py and the torch.distributed sharding layer.  Plumbing only: every number comes
from the HIP kernels; a missing library or a missing GPU raises, there is no fallback.
"""
from __future__ import annotations

import ctypes as C
import importlib.util
import os

import numpy as np

from . import build as _build

NO_INDEX = 0xFFFFFFFF
ALGO_AUTO, ALGO_STREAM, ALGO_GRID, ALGO_STREAM_EXACT, ALGO_RING = 0, 1, 2, 3, 4
KNN_MAX_K = 64                  # PCT_KNN_MAX_K
ORDER_INDEX, ORDER_DISTANCE = 0, 1      # enum pct_order: rows of a radius search in ascending index / nearest first

_lib = None


class EngineError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"pct_engine status {code}: {msg}")
        self.code = code


class InflateParams(C.Structure):
    _fields_ = [("start", C.c_double * 3), ("sample_range", C.c_double), ("search_margin", C.c_double),
                ("max_radius", C.c_double)]


class ReplanOut(C.Structure):
    _fields_ = [("node_radius", C.c_void_p), ("node_idx", C.c_void_p), ("node_d2", C.c_void_p),
                ("sample_pos", C.c_void_p), ("sample_radius", C.c_void_p), ("sample_d2", C.c_void_p), ("sample_idx", C.c_void_p),
                ("ctrl_pos", C.c_void_p), ("ctrl_radius", C.c_void_p), ("ctrl_d2", C.c_void_p), ("ctrl_idx", C.c_void_p),
                ("nsamples", C.c_int64), ("first_hit_sample", C.c_int64), ("nctrl", C.c_int64), ("first_hit_ctrl", C.c_int64)]


class ExpandResult(C.Structure):
    """pct_expand_result: the steered centre, its inflated radius, the nearest node and the neighbourhood's size"""
    _fields_ = [("center", C.c_double * 3), ("radius", C.c_double), ("near_idx", C.c_int32), ("count", C.c_int32)]


class BezierTraj(C.Structure):
    _fields_ = [("polycoef", C.POINTER(C.c_double)), ("row_stride", C.c_int64), ("seg_time", C.POINTER(C.c_double)),
                ("orders", C.POINTER(C.c_int32)), ("nseg", C.c_int32)]


class BezierBatch(C.Structure):
    """pct_bezier_batch: B trajectories packed one after another (include/pct_engine.h, paragraph "Batched Bezier check").  Host
    pointers for Cloud.bezier_check_batch (engine.pack_trajectories fills them), device pointers for bezier_check_batch_device."""
    _fields_ = [("polycoef", C.c_void_p), ("row_stride", C.c_int64), ("seg_time", C.c_void_p), ("orders", C.c_void_p),
                ("seg_offsets", C.c_void_p), ("t_start", C.c_void_p), ("B", C.c_int64)]


class TrajVerdict(C.Structure):
    """pct_traj_verdict, 32 bytes"""
    _fields_ = [("nsamples", C.c_int64), ("first_hit", C.c_int64), ("min_sample", C.c_int64), ("min_radius", C.c_double)]


VERDICT_DTYPE = np.dtype([("nsamples", np.int64), ("first_hit", np.int64), ("min_sample", np.int64), ("min_radius", np.float64)])

CERT_FREE, CERT_HIT, CERT_UNDECIDED, CERT_INVALID = 0, 1, 2, 3      # enum pct_cert_status
# pct_traj_certificate, 48 bytes (include/pct_engine.h, paragraph "Certified Bezier check")
CERT_DTYPE = np.dtype([("status", np.int32), ("depth", np.int32), ("hit_seg", np.int32), ("hit_idx", np.uint32), ("hit_u", np.float64),
                       ("hit_d2", np.float64), ("min_d2", np.float64), ("pieces", np.int64)])

CLR_DONE, CLR_OPEN, CLR_INVALID = 0, 1, 2                           # enum pct_clearance_status
# pct_traj_clearance, 48 bytes (include/pct_engine.h, paragraph "Trajectory clearance")
CLEARANCE_DTYPE = np.dtype([("status", np.int32), ("depth", np.int32), ("at_seg", np.int32), ("at_idx", np.uint32), ("at_u", np.float64),
                            ("lo", np.float64), ("hi", np.float64), ("pieces", np.int64)])

GEN_OK, GEN_NOT_CONVERGED, GEN_INVALID = 0, 1, 2                    # enum pct_gen_status
# pct_trajgen_result, 64 bytes (include/pct_trajgen.h, paragraph "Trajectory generation")
GEN_RESULT_DTYPE = np.dtype([("status", np.int32), ("iterations", np.int32), ("cost", np.float64), ("duration", np.float64),
                             ("r_prim", np.float64), ("r_dual", np.float64), ("sphere_slack", np.float64),
                             ("max_vel_ctrl", np.float64), ("max_acc_ctrl", np.float64)])


class TrajGenBatch(C.Structure):
    """pct_trajgen_batch: B corridors with their time allocations and end states.  Host pointers for engine.bezier_generate
    (engine.pack_corridors fills them), device pointers for engine.bezier_generate_device."""
    _fields_ = [("centres", C.c_void_p), ("radius", C.c_void_p), ("seg_time", C.c_void_p), ("orders", C.c_void_p), ("seg_offsets", C.c_void_p),
                ("start_state", C.c_void_p), ("end_state", C.c_void_p), ("B", C.c_int64)]


class TrajGenParams(C.Structure):
    """pct_trajgen_params"""
    _fields_ = [("minimize_order", C.c_int32), ("max_iter", C.c_int32), ("check_every", C.c_int32), ("max_vel", C.c_double), ("max_acc", C.c_double),
                ("margin", C.c_double), ("eps", C.c_double), ("rho", C.c_double)]


def gen_params(minimize_order=3, max_iter=4000, check_every=25, max_vel=0.0, max_acc=0.0, margin=0.0, eps=1e-5, rho=0.0) -> TrajGenParams:
    """minimize_order 3 = jerk (the reference's default); max_vel / max_acc <= 0 or inf: no limit; rho 0 = automatic"""
    return TrajGenParams(int(minimize_order), int(max_iter), int(check_every), float(max_vel), float(max_acc), float(margin), float(eps), float(rho))


def pack_corridors(corridors):
    """A list of dict(centres [m, 3], radius [m], seg_time [m], orders [m], start [9], end [9]) -> (TrajGenBatch, arrays); `arrays` =
    dict(centres, radius, seg_time, orders, seg_offsets, start_state, end_state) are the numpy arrays the struct points into: keep
    them alive while it is used."""
    cs = list(corridors)
    nseg = [len(np.asarray(c["seg_time"]).reshape(-1)) for c in cs]
    for c, m in zip(cs, nseg):
        if np.asarray(c["centres"]).size != 3 * m or np.asarray(c["radius"]).size != m or np.asarray(c["orders"]).size != m:
            raise ValueError("a corridor is centres [m, 3], radius [m], seg_time [m], orders [m]")
        if np.asarray(c["start"]).size != 9 or np.asarray(c["end"]).size != 9:
            raise ValueError("start and end are p, v, a: 9 values each")
    offs = np.zeros(len(cs) + 1, np.int32)
    offs[1:] = np.cumsum(nseg)

    def cat(key, dt, w):
        return np.ascontiguousarray(np.concatenate([np.asarray(c[key], dt).reshape(-1, w) for c in cs]) if cs else np.zeros((0, w), dt))
    a = dict(centres=cat("centres", np.float64, 3), radius=cat("radius", np.float64, 1).reshape(-1), seg_time=cat("seg_time", np.float64, 1).reshape(-1),
             orders=cat("orders", np.int32, 1).reshape(-1), seg_offsets=offs, start_state=cat("start", np.float64, 9), end_state=cat("end", np.float64, 9))
    b = TrajGenBatch(*[a[k].ctypes.data for k in ("centres", "radius", "seg_time", "orders", "seg_offsets", "start_state", "end_state")], len(cs))
    return b, a


def corridor_fan(centres, radius=None, seg_time=None, orders=None, scales=None, start=None, end=None):
    """one corridor under a list of time scales: the corridors engine.pack_corridors / engine.bezier_generate take, candidate k with
    every segment time multiplied by scales[k].  corridor_fan(corridor, scales) does the same to a corridor given as a dict, of
    spheres or of polytopes (engine.pack_poly_corridors): copies that differ in seg_time alone."""
    if isinstance(centres, dict):
        if scales is None:
            scales = radius
        T = np.asarray(centres["seg_time"], np.float64).reshape(-1)
        return [dict(centres, seg_time=T * float(sc)) for sc in scales]
    T = np.asarray(seg_time, np.float64).reshape(-1)
    return [dict(centres=centres, radius=radius, seg_time=T * float(sc), orders=orders, start=start, end=end) for sc in scales]


def bezier_generate(corridors, params: TrajGenParams, row_stride=None):
    """pct_bezier_generate_batch: one minimum-jerk Bezier trajectory per corridor (a list of dicts as engine.pack_corridors takes, or
    its packed (TrajGenBatch, arrays) pair), all solved in one launch.  Returns (polycoef [total_seg, row_stride], results): the rows
    in the layout the checks read -- with arrays["seg_time"], ["orders"], ["seg_offsets"] they are a pct_bezier_batch -- and a structured
    array of engine.GEN_RESULT_DTYPE: status (GEN_OK, GEN_NOT_CONVERGED, GEN_INVALID), iterations, cost, duration, r_prim, r_dual,
    sphere_slack, max_vel_ctrl, max_acc_ctrl."""
    packed = isinstance(corridors, tuple) and len(corridors) == 2 and isinstance(corridors[0], TrajGenBatch)
    batch, keep = corridors if packed else pack_corridors(corridors)
    if row_stride is None:
        od = keep["orders"]
        row_stride = 3 * (int(np.clip(od.max() if len(od) else 5, 5, 12)) + 1)
    coef = np.zeros((len(keep["seg_time"]), int(row_stride)), np.float64)
    res = np.zeros(int(batch.B), GEN_RESULT_DTYPE)
    _chk(lib().pct_bezier_generate_batch(C.byref(batch), C.byref(params), _ptr(coef), int(row_stride), _ptr(res)))
    del keep
    return coef, res


def bezier_generate_device(fields, params: TrajGenParams, polycoef, results, stream=None):
    """pct_bezier_generate_batch_dev on torch tensors, asynchronous on the current stream (or `stream`, a raw hipStream_t handle), no
    host synchronisation, capturable.  fields: dict of device tensors centres [total, 3] f64, radius, seg_time [total] f64, orders
    [total] i32, seg_offsets [B + 1] i32, start_state, end_state [B, 9] f64; polycoef: [total, row_stride] f64; results: B x 64 bytes
    (uint8 [B, 64]; view the host copy as engine.GEN_RESULT_DTYPE).  polycoef.data_ptr() with the same seg_time / orders / seg_offsets
    is the BezierBatch bezier_check_batch_device and bezier_certify_device take."""
    import torch
    want = dict(centres=torch.float64, radius=torch.float64, seg_time=torch.float64, orders=torch.int32, seg_offsets=torch.int32,
                start_state=torch.float64, end_state=torch.float64)
    for k, dt in want.items():
        t = fields[k]
        if t.dtype != dt or not t.is_contiguous() or not t.is_cuda:
            raise ValueError(f"{k} must be a contiguous device tensor of {dt}")
    B = int(fields["seg_offsets"].numel()) - 1
    total = int(fields["seg_time"].numel())
    if polycoef.dtype != torch.float64 or polycoef.dim() != 2 or polycoef.shape[0] != total or not polycoef.is_contiguous() or not polycoef.is_cuda:
        raise ValueError("polycoef must be a contiguous float64 device tensor [total_seg, row_stride]")
    if results.dtype != torch.uint8 or results.numel() != 64 * B or not results.is_contiguous() or not results.is_cuda:
        raise ValueError("results must be a contiguous uint8 device tensor of B x 64 bytes")
    if fields["start_state"].numel() != 9 * B or fields["end_state"].numel() != 9 * B or fields["centres"].numel() != 3 * total:
        raise ValueError("start_state / end_state are [B, 9], centres is [total_seg, 3]")
    batch = TrajGenBatch(*[fields[k].data_ptr() or None for k in ("centres", "radius", "seg_time", "orders", "seg_offsets", "start_state", "end_state")], B)
    if stream is None:
        stream = torch.cuda.current_stream().cuda_stream
    _chk(lib().pct_bezier_generate_batch_dev(C.byref(batch), C.byref(params), polycoef.data_ptr() or None, int(polycoef.shape[1]),
                                             results.data_ptr() or None, stream or None))
    return batch


class TrajGenPolyBatch(C.Structure):
    """pct_trajgen_poly_batch: B corridors of polytopes (half-spaces per segment) with their time allocations and end states.  Host
    pointers for engine.bezier_generate_poly (engine.pack_poly_corridors fills them), device pointers for
    engine.bezier_generate_poly_device."""
    _fields_ = [("anchors", C.c_void_p), ("planes", C.c_void_p), ("plane_offsets", C.c_void_p), ("seg_time", C.c_void_p), ("orders", C.c_void_p),
                ("seg_offsets", C.c_void_p), ("start_state", C.c_void_p), ("end_state", C.c_void_p), ("B", C.c_int64)]


POLY_FIELDS = ("anchors", "planes", "plane_offsets", "seg_time", "orders", "seg_offsets", "start_state", "end_state")


def trajgen_max_planes() -> int:
    """pct_trajgen_max_planes: the most planes one segment of a polyhedral corridor may own (24)"""
    return int(lib().pct_trajgen_max_planes())


def pack_poly_corridors(corridors):
    """A list of dict(anchors [m, 3], planes (m arrays [k_i, 4]: n0 n1 n2 off, n . y <= off), seg_time [m], orders [m], start [9],
    end [9]) -> (TrajGenPolyBatch, arrays); `arrays` = dict(anchors, planes [total_planes, 4] (one unused row when there is no plane at
    all), plane_offsets [total_seg + 1], seg_time, orders, seg_offsets, start_state, end_state) are the numpy arrays the struct points into: keep them alive while it is used."""
    cs = list(corridors)
    nseg = [len(np.asarray(c["seg_time"]).reshape(-1)) for c in cs]
    for c, m in zip(cs, nseg):
        if np.asarray(c["anchors"]).size != 3 * m or len(c["planes"]) != m or np.asarray(c["orders"]).size != m:
            raise ValueError("a corridor is anchors [m, 3], planes (m arrays [k, 4]), seg_time [m], orders [m]")
        if np.asarray(c["start"]).size != 9 or np.asarray(c["end"]).size != 9:
            raise ValueError("start and end are p, v, a: 9 values each")
    offs = np.zeros(len(cs) + 1, np.int32)
    offs[1:] = np.cumsum(nseg)

    def cat(key, dt, w):
        return np.ascontiguousarray(np.concatenate([np.asarray(c[key], dt).reshape(-1, w) for c in cs]) if cs else np.zeros((0, w), dt))
    per_seg = [np.asarray(p, np.float64).reshape(-1, 4) for c in cs for p in c["planes"]]
    po = np.zeros(len(per_seg) + 1, np.int32)
    po[1:] = np.cumsum([len(p) for p in per_seg])
    planes = np.ascontiguousarray(np.concatenate(per_seg) if per_seg else np.zeros((0, 4)))
    if len(planes) == 0:
        planes = np.zeros((1, 4), np.float64)      # never read: the library asks for a pointer that is not null
    a = dict(anchors=cat("anchors", np.float64, 3), planes=planes, plane_offsets=po, seg_time=cat("seg_time", np.float64, 1).reshape(-1),
             orders=cat("orders", np.int32, 1).reshape(-1), seg_offsets=offs, start_state=cat("start", np.float64, 9), end_state=cat("end", np.float64, 9))
    return TrajGenPolyBatch(*[a[k].ctypes.data for k in POLY_FIELDS], len(cs)), a


def bezier_generate_poly(corridors, params: TrajGenParams, row_stride=None):
    """pct_bezier_generate_poly_batch: engine.bezier_generate in polyhedral corridors (a list of dicts as engine.pack_poly_corridors
    takes, or its packed pair).  Returns (polycoef [total_seg, row_stride], results) as engine.bezier_generate does; sphere_slack of
    the records is the corridor slack, the least distance of a control point inside a plane moved in by the margin."""
    packed = isinstance(corridors, tuple) and len(corridors) == 2 and isinstance(corridors[0], TrajGenPolyBatch)
    batch, keep = corridors if packed else pack_poly_corridors(corridors)
    if row_stride is None:
        od = keep["orders"]
        row_stride = 3 * (int(np.clip(od.max() if len(od) else 5, 5, 12)) + 1)
    coef = np.zeros((len(keep["seg_time"]), int(row_stride)), np.float64)
    res = np.zeros(int(batch.B), GEN_RESULT_DTYPE)
    _chk(lib().pct_bezier_generate_poly_batch(C.byref(batch), C.byref(params), _ptr(coef), int(row_stride), _ptr(res)))
    del keep
    return coef, res


def bezier_generate_poly_device(fields, params: TrajGenParams, polycoef, results, stream=None):
    """pct_bezier_generate_poly_batch_dev on torch tensors, asynchronous on the current stream (or `stream`, a raw hipStream_t
    handle), no host synchronisation, capturable.  fields: dict of device tensors anchors [total, 3] f64, planes [total_planes, 4] f64
    (at least one row, read or not), plane_offsets [total + 1] i32, seg_time [total] f64, orders [total] i32, seg_offsets [B + 1] i32,
    start_state, end_state [B, 9] f64; polycoef and results as engine.bezier_generate_device takes them."""
    import torch
    want = dict(anchors=torch.float64, planes=torch.float64, plane_offsets=torch.int32, seg_time=torch.float64, orders=torch.int32,
                seg_offsets=torch.int32, start_state=torch.float64, end_state=torch.float64)
    for k, dt in want.items():
        t = fields[k]
        if t.dtype != dt or not t.is_contiguous() or not t.is_cuda:
            raise ValueError(f"{k} must be a contiguous device tensor of {dt}")
    B = int(fields["seg_offsets"].numel()) - 1
    total = int(fields["seg_time"].numel())
    if polycoef.dtype != torch.float64 or polycoef.dim() != 2 or polycoef.shape[0] != total or not polycoef.is_contiguous() or not polycoef.is_cuda:
        raise ValueError("polycoef must be a contiguous float64 device tensor [total_seg, row_stride]")
    if results.dtype != torch.uint8 or results.numel() != 64 * B or not results.is_contiguous() or not results.is_cuda:
        raise ValueError("results must be a contiguous uint8 device tensor of B x 64 bytes")
    if fields["start_state"].numel() != 9 * B or fields["end_state"].numel() != 9 * B or fields["anchors"].numel() != 3 * total:
        raise ValueError("start_state / end_state are [B, 9], anchors is [total_seg, 3]")
    if fields["plane_offsets"].numel() != total + 1 or fields["planes"].numel() % 4 != 0:
        raise ValueError("plane_offsets is [total_seg + 1], planes is [total_planes, 4]")
    batch = TrajGenPolyBatch(*[fields[k].data_ptr() or None for k in POLY_FIELDS], B)
    if stream is None:
        stream = torch.cuda.current_stream().cuda_stream
    _chk(lib().pct_bezier_generate_poly_batch_dev(C.byref(batch), C.byref(params), polycoef.data_ptr() or None, int(polycoef.shape[1]),
                                                  results.data_ptr() or None, stream or None))
    return batch


def time_allocation(centres, radius, start, end, init_vel, vel_mean, acc_mean):
    """pct_time_allocation: the reference's timeAllocation (sim_planning_demo.cpp:603-686): one time per sphere of the corridor"""
    c = np.ascontiguousarray(centres, np.float64).reshape(-1, 3)
    r = np.ascontiguousarray(radius, np.float64).reshape(-1)
    if len(r) != len(c):
        raise ValueError("one radius per centre")
    p0, p1, v0 = (np.ascontiguousarray(v, np.float64).reshape(3) for v in (start, end, init_vel))
    out = np.zeros(len(c), np.float64)
    _chk(lib().pct_time_allocation(_ptr(c), _ptr(r), len(c), _ptr(p0), _ptr(p1), _ptr(v0), float(vel_mean), float(acc_mean), _ptr(out)))
    return out


def pack_trajectories(trajectories, t_start=None):
    """A list of (polycoef, seg_time, orders) -> (BezierBatch, arrays): the rows one after another, padded with zeros to a common
    row_stride; t_start: B start times or None (0.0 for every trajectory).  `arrays` = dict(polycoef, seg_time, orders, seg_offsets,
    t_start) are the numpy arrays the struct points into: keep them alive while it is used."""
    trajs = [(np.asarray(c, np.float64), np.asarray(t, np.float64).reshape(-1), np.asarray(o, np.int32).reshape(-1)) for c, t, o in trajectories]
    for c, t, o in trajs:
        if c.ndim != 2 or len(c) != len(t) or len(t) != len(o):
            raise ValueError("a trajectory is (polycoef [nseg, row_stride], seg_time [nseg], orders [nseg])")
    stride = max([c.shape[1] for c, _, _ in trajs], default=3)
    nseg = [len(t) for _, t, _ in trajs]
    seg_offsets = np.zeros(len(trajs) + 1, np.int32)
    seg_offsets[1:] = np.cumsum(nseg)
    coef = np.zeros((int(seg_offsets[-1]), stride), np.float64)
    for (c, _, _), a in zip(trajs, seg_offsets):
        coef[a:a + len(c), :c.shape[1]] = c
    seg_time = np.concatenate([t for _, t, _ in trajs]) if trajs else np.zeros(0)
    orders = np.concatenate([o for _, _, o in trajs]) if trajs else np.zeros(0, np.int32)
    arrays = dict(polycoef=coef, seg_time=np.ascontiguousarray(seg_time, np.float64), orders=np.ascontiguousarray(orders, np.int32),
                  seg_offsets=seg_offsets, t_start=None)
    if t_start is not None:
        arrays["t_start"] = np.ascontiguousarray(t_start, np.float64).reshape(-1)
        if len(arrays["t_start"]) != len(trajs):
            raise ValueError("one t_start per trajectory")
    b = BezierBatch(coef.ctypes.data, stride, arrays["seg_time"].ctypes.data, arrays["orders"].ctypes.data, seg_offsets.ctypes.data,
                    None if t_start is None else arrays["t_start"].ctypes.data, len(trajs))
    return b, arrays


DEPTH_Z, DEPTH_RANGE = 0, 1            # enum pct_depth_metric: a pixel holds the depth along the optical axis / the range along the ray


class DepthView(C.Structure):
    """pct_depth_view: the pinned projection of a depth image (include/pct_engine.h, paragraph "Depth images")"""
    _fields_ = [("t", C.c_double * 3), ("R", C.c_double * 9), ("focal", C.c_double), ("near_z", C.c_double),
                ("width", C.c_int32), ("height", C.c_int32), ("metric", C.c_int32), ("reserved", C.c_int32)]


class KnnStats(C.Structure):
    """pct_knn_stats: the statistics of the k-NN mean distances (include/pct_engine.h, paragraph "Statistical outliers")"""
    _fields_ = [("measured", C.c_int64), ("sum", C.c_double), ("sum_sq", C.c_double), ("mean", C.c_double), ("stddev", C.c_double),
                ("threshold", C.c_double)]

    def as_dict(self) -> dict:
        return dict(measured=int(self.measured), sum=float(self.sum), sum_sq=float(self.sum_sq), mean=float(self.mean),
                    stddev=float(self.stddev), threshold=float(self.threshold))


def depth_view(t, R, width, height, fov_hor_deg=None, focal=None, metric=DEPTH_Z, near_z=0.01) -> DepthView:
    """t: camera position; R: 3 x 3, column k = camera axis k in world (x image right, y image down, z optical); the focal distance in
    image widths is given directly or as 0.5 / tan(fov_hor / 2) of a horizontal field of view in degrees"""
    if (fov_hor_deg is None) == (focal is None):
        raise ValueError("give exactly one of fov_hor_deg and focal")
    v = DepthView()
    v.t[:] = [float(x) for x in np.asarray(t, np.float64).reshape(3)]
    v.R[:] = [float(x) for x in np.asarray(R, np.float64).reshape(9)]
    v.focal = float(focal) if focal is not None else 0.5 / float(np.tan(np.float64(fov_hor_deg) * np.pi / 180.0 / 2.0))
    v.near_z = float(near_z)
    v.width, v.height, v.metric, v.reserved = int(width), int(height), int(metric), 0
    return v


def depth_image(view: DepthView, image):
    """the image as the library reads it: float32, C-contiguous, height x width"""
    a = np.ascontiguousarray(image, np.float32)
    if a.size != view.width * view.height:
        raise ValueError(f"the image has {a.size} pixels, the view {view.width} x {view.height}")
    return a


def depth_classify(views, images, points, margin, want_pixel=True):
    """pct_depth_classify: (seen_by int32 [n], pixel int32 [n, 2] or None) -- the lowest view whose image sees each planner point
    through (or -1), and the point's pixel (ru, rv) in the LAST view (or -1, -1 when it is not in that image)"""
    views = list(views)
    imgs = [depth_image(v, im) for v, im in zip(views, images)]
    if len(imgs) != len(views):
        raise ValueError("one image per view")
    p = np.ascontiguousarray(points, np.float64).reshape(-1, 3)
    varr = (DepthView * max(len(views), 1))(*views)
    iarr = (C.c_void_p * max(len(views), 1))(*[im.ctypes.data for im in imgs])
    seen = np.empty(len(p), np.int32)
    pix = np.empty((len(p), 2), np.int32) if want_pixel else None
    _chk(lib().pct_depth_classify(varr, iarr, len(views), _ptr(p), len(p), float(margin), _ptr(seen), None if pix is None else _ptr(pix)))
    return seen, pix


class RangeView(C.Structure):
    """pct_range_view: the pinned projection of a lidar range image (include/pct_engine.h, paragraph "Range images").  The four
    table pointers name host arrays that must outlive every call the view is handed to: range_view() keeps them on the view."""
    _fields_ = [("t", C.c_double * 3), ("R", C.c_double * 9), ("near_range", C.c_double), ("width", C.c_int32), ("height", C.c_int32),
                ("reserved", C.c_int32 * 2), ("col_edge", C.POINTER(C.c_double)), ("row_edge", C.POINTER(C.c_double)),
                ("col_dir", C.POINTER(C.c_double)), ("row_dir", C.POINTER(C.c_double))]


def pseudo_angle(x, y) -> float:
    """pct_range_pseudo_angle: the monotone stand-in for atan2(y, x) on [0, 4) that places a point in a column (needs no device)"""
    return float(lib().pct_range_pseudo_angle(float(x), float(y)))


def range_view(t, R, col_edge, row_edge, col_dir=None, row_dir=None, near_range=0.05) -> RangeView:
    """t: sensor position; R: 3 x 3, column k = sensor axis k in world (x azimuth 0, y azimuth +90 deg, z up); col_edge [width + 1]
    pseudo-angles, row_edge [height + 1] values of z / hypot(x, y), both strictly ascending; col_dir [width, 2] and row_dir
    [height, 2]: (cos, sin) of the beams' azimuths and elevations, needed by append_range alone.  The view keeps its arrays alive."""
    ce, re_ = np.ascontiguousarray(col_edge, np.float64).reshape(-1), np.ascontiguousarray(row_edge, np.float64).reshape(-1)
    if len(ce) < 2 or len(re_) < 2:
        raise ValueError("an edge table has width + 1 (height + 1) entries, at least 2")
    v = RangeView()
    v.t[:] = [float(x) for x in np.asarray(t, np.float64).reshape(3)]
    v.R[:] = [float(x) for x in np.asarray(R, np.float64).reshape(9)]
    v.near_range = float(near_range)
    v.width, v.height = len(ce) - 1, len(re_) - 1
    keep = [ce, re_]
    dp = C.POINTER(C.c_double)
    v.col_edge, v.row_edge = ce.ctypes.data_as(dp), re_.ctypes.data_as(dp)
    for name, a, n in (("col_dir", col_dir, v.width), ("row_dir", row_dir, v.height)):
        if a is None:
            continue
        a = np.ascontiguousarray(a, np.float64).reshape(-1)
        if len(a) != 2 * n:
            raise ValueError(f"{name} has {len(a)} entries, the view needs {n} x 2")
        keep.append(a)
        setattr(v, name, a.ctypes.data_as(dp))
    v._arrays = keep
    return v


def range_view_uniform(t, R_sensor, az_start, az_span, el_lo, el_hi, width, height, near_range=0.05) -> RangeView:
    """the view of an evenly spaced scan, angles in radians: `width` columns of az_span / width each, the first one starting at azimuth
    az_start of the sensor frame R_sensor, and `height` rings of (el_hi - el_lo) / height each between the elevations el_lo < el_hi
    (inside +/- 90 degrees); every beam points along the middle of its cell, so the edges lie midway between beams, in angle.
    az_start is folded into the returned view's R (a turn about the sensor's z axis), so that the span starts at azimuth 0:
    col_edge[0] = 0, and col_edge[width] = 4 when az_span is the full circle."""
    width, height = int(width), int(height)
    full = abs(az_span - 2.0 * np.pi) <= 2.0 * np.pi * 1.0e-12
    if not (width >= 1 and height >= 1 and (full or 0.0 < az_span < 2.0 * np.pi) and -np.pi / 2 < el_lo < el_hi < np.pi / 2):
        raise ValueError("bad scan geometry")
    span = 2.0 * np.pi if full else float(az_span)
    az_edge = np.arange(width + 1, dtype=np.float64) * (span / width)
    L = lib()
    col_edge = np.array([L.pct_range_pseudo_angle(float(np.cos(a)), float(np.sin(a))) for a in az_edge], np.float64)
    col_edge[0] = 0.0
    if full:
        col_edge[width] = 4.0
    az_beam = (np.arange(width, dtype=np.float64) + 0.5) * (span / width)
    el_edge = el_lo + np.arange(height + 1, dtype=np.float64) * ((el_hi - el_lo) / height)
    el_beam = el_lo + (np.arange(height, dtype=np.float64) + 0.5) * ((el_hi - el_lo) / height)
    ca, sa = np.cos(np.float64(az_start)), np.sin(np.float64(az_start))
    Rs = np.asarray(R_sensor, np.float64).reshape(3, 3)
    Rv = np.stack([ca * Rs[:, 0] + sa * Rs[:, 1], ca * Rs[:, 1] - sa * Rs[:, 0], Rs[:, 2]], axis=1)
    return range_view(t, Rv, col_edge, np.tan(el_edge), np.stack([np.cos(az_beam), np.sin(az_beam)], axis=1),
                      np.stack([np.cos(el_beam), np.sin(el_beam)], axis=1), near_range)


def range_classify(views, images, points, margin, want_pixel=True):
    """pct_range_classify: (seen_by int32 [n], pixel int32 [n, 2] or None) -- the lowest view whose scan sees each planner point
    through (or -1), and the point's pixel (c, r) in the LAST view (or -1, -1 when it is not in that image)"""
    views = list(views)
    imgs = [depth_image(v, im) for v, im in zip(views, images)]
    if len(imgs) != len(views):
        raise ValueError("one image per view")
    p = np.ascontiguousarray(points, np.float64).reshape(-1, 3)
    varr = (RangeView * max(len(views), 1))(*views)
    iarr = (C.c_void_p * max(len(views), 1))(*[im.ctypes.data for im in imgs])
    seen = np.empty(len(p), np.int32)
    pix = np.empty((len(p), 2), np.int32) if want_pixel else None
    _chk(lib().pct_range_classify(varr, iarr, len(views), _ptr(p), len(p), float(margin), _ptr(seen), None if pix is None else _ptr(pix)))
    return seen, pix


def _preload_hip_runtime():
    """One HIP runtime per process.  PyTorch-ROCm wheels bundle their own libamdhip64.so (soname
    libamdhip64.so.7, the same as /opt/rocm's); two copies in one process each open the KFD device
    and the second one sees no GPU.  Loading torch's copy FIRST makes libpct_engine.so's
    DT_NEEDED libamdhip64.so.7 resolve to it by soname, and a later `import torch` finds the same
    file already mapped.  Without torch installed the system runtime is used as linked."""
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is not None and spec.submodule_search_locations:
        p = os.path.join(list(spec.submodule_search_locations)[0], "lib", "libamdhip64.so")
        if os.path.exists(p):
            C.CDLL(p, mode=C.RTLD_GLOBAL)


def lib():
    """Load (never build implicitly on a GPU box: the .so travels with the snapshot)."""
    global _lib
    if _lib is None:
        _preload_hip_runtime()
        if not os.path.exists(_build.ENGINE_SO):
            raise FileNotFoundError(f"{_build.ENGINE_SO} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                                    "(the HIP extension is mandatory; there is no CPU fallback)")
        L = C.CDLL(_build.ENGINE_SO)
        vp, i64, i32, u32p, f32p, f64p = C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p
        L.pct_last_error.restype = C.c_char_p
        L.pct_init.argtypes = [i32]
        L.pct_cloud_create.argtypes = [i64, C.POINTER(vp)]
        L.pct_cloud_destroy.argtypes = [vp]
        L.pct_cloud_create_small.argtypes = [i64, C.POINTER(vp)]
        L.pct_cloud_small_aux.argtypes = [vp, C.POINTER(C.POINTER(C.c_double))]
        L.pct_rrt_expand_batch.argtypes = [vp, vp, C.POINTER(InflateParams), f64p, i64, i64, C.POINTER(ExpandResult), u32p]
        L.pct_cloud_size.restype = i64
        L.pct_cloud_size.argtypes = [vp]
        L.pct_cloud_capacity.restype = i64
        L.pct_cloud_capacity.argtypes = [vp]
        L.pct_cloud_set_index_base.argtypes = [vp, i64]
        L.pct_cloud_upload_aos.argtypes = [vp, vp, i64, i64]
        L.pct_cloud_upload_soa_dev.argtypes = [vp, vp, vp, vp, i64]
        L.pct_cloud_upload_fields.argtypes = [vp, vp, i64, i64, i64, i64, i64]
        L.pct_cloud_append_aos.argtypes = [vp, vp, i64, i64]
        L.pct_cloud_build_grid.argtypes = [vp, C.c_float]
        L.pct_cloud_drop_grid.argtypes = [vp]
        L.pct_cloud_has_grid.argtypes = [vp]
        L.pct_cloud_grid_info.argtypes = [vp, C.POINTER(C.c_int32), C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(i64)]
        L.pct_nodeset_create.argtypes = [C.c_int, i64, C.POINTER(vp)]
        L.pct_nodeset_destroy.argtypes = [vp]
        L.pct_nodeset_clear.argtypes = [vp]
        L.pct_nodeset_size.argtypes = [vp]
        L.pct_nodeset_size.restype = i64
        L.pct_nodeset_dim.argtypes = [vp]
        L.pct_nodeset_append.argtypes = [vp, C.POINTER(C.c_double), i64]
        L.pct_nodeset_nearest.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_uint32), C.POINTER(C.c_double), C.POINTER(C.c_uint32)]
        L.pct_nodeset_radius_indices_r2.argtypes = [vp, C.POINTER(C.c_double), C.c_double, vp, i64, C.POINTER(i64)]
        L.pct_cloud_ring_bucket_records.argtypes = [vp]
        L.pct_nn_batch.argtypes = [vp, f32p, i64, u32p, f64p]
        L.pct_nn_batch_algo.argtypes = [vp, i32, f32p, i64, u32p, f64p]
        L.pct_knn_batch.argtypes = [vp, f32p, i64, C.c_int32, u32p, f64p]
        L.pct_knn_batch_algo.argtypes = [vp, i32, f32p, i64, C.c_int32, u32p, f64p]
        L.pct_knn_batch_dev.argtypes = [vp, i32, vp, i64, C.c_int32, vp, vp, vp]
        L.pct_radius_search_batch.argtypes = [vp, i32, f32p, f32p, i64, i32, vp, C.POINTER(i64)]
        L.pct_radius_search_read.argtypes = [vp, i64, i64, u32p, f64p]
        L.pct_radius_search_batch_dev.argtypes = [vp, i32, vp, vp, i64, i32, vp, i64, vp, vp, vp]
        L.pct_radius_count_batch.argtypes = [vp, f32p, f32p, i64, u32p]
        L.pct_radius_count_batch_algo.argtypes = [vp, i32, f32p, f32p, i64, u32p]
        L.pct_radius_indices.argtypes = [vp, f32p, C.c_float, u32p, i64, C.POINTER(i64)]
        L.pct_nn_batch_q64.argtypes = [vp, f64p, i64, u32p, f64p]
        L.pct_nn_batch_q64_ties.argtypes = [vp, f64p, i64, u32p, f64p, u32p]
        L.pct_radius_indices_q64.argtypes = [vp, f64p, C.c_double, u32p, i64, C.POINTER(i64)]
        L.pct_radius_indices_r2_q64.argtypes = [vp, f64p, C.c_double, u32p, i64, C.POINTER(i64)]
        L.pct_radius_indices_batch_q64.argtypes = [vp, f64p, f64p, i64, u32p, i64, vp]
        L.pct_radius_crop.argtypes = [vp, vp, C.c_double, C.c_int, i64, vp, vp, vp, C.POINTER(i64)]
        L.pct_cloud_crop_to.argtypes = [vp, vp, C.c_double, vp]
        L.pct_inflate_batch.argtypes = [vp, C.POINTER(InflateParams), f64p, i64, f64p, u32p, f64p]
        L.pct_segment_nn_batch.argtypes = [vp, i32, f64p, f64p, i64, u32p, f64p, f64p]
        L.pct_segment_nn_batch_dev.argtypes = [vp, i32, vp, vp, i64, vp, vp, vp, vp]
        L.pct_segment_inflate_batch.argtypes = [vp, C.POINTER(InflateParams), f64p, i64, f64p, u32p, f64p]
        L.pct_segment_sweep_batch.argtypes = [vp, i32, f64p, f64p, i64, u32p, f64p]
        L.pct_segment_sweep_batch_dev.argtypes = [vp, i32, vp, vp, i64, vp, vp, vp]
        L.pct_segment_count_batch.argtypes = [vp, i32, f64p, f64p, i64, u32p]
        L.pct_segment_count_batch_dev.argtypes = [vp, i32, vp, vp, i64, vp, vp]
        L.pct_segment_search_batch.argtypes = [vp, i32, f64p, f64p, i64, i32, vp, C.POINTER(i64)]
        L.pct_segment_search_read.argtypes = [vp, i64, i64, u32p, f64p, f64p]
        L.pct_segment_search_batch_dev.argtypes = [vp, i32, vp, vp, i64, i32, vp, i64, vp, vp, vp, vp]
        L.pct_segment_polyhedron_batch.argtypes = [vp, i32, f64p, f64p, i64, vp, C.POINTER(i64)]
        L.pct_segment_polyhedron_read.argtypes = [vp, i64, i64, u32p, f64p, f64p, f64p]
        L.pct_segment_supports_dev.argtypes = [vp, vp, i64, vp, i64, vp, vp, i64, vp, vp, vp, vp, vp]
        L.pct_polyhedron_lds_rows.argtypes = []
        L.pct_polyhedron_lds_rows.restype = C.c_int
        L.pct_bezier_check.argtypes = [vp, C.POINTER(BezierTraj), C.POINTER(InflateParams), C.c_double, C.c_double, C.c_double,
                                       C.POINTER(i64), C.POINTER(i64), i64, f64p, f64p, f64p, u32p]
        L.pct_nn_batch_dev.argtypes = [vp, i32, vp, i64, vp, vp, vp]
        L.pct_inflate_batch_dev.argtypes = [vp, C.POINTER(InflateParams), vp, i64, vp, vp, vp, vp]
        L.pct_bezier_check_dev.argtypes = [vp, C.POINTER(BezierTraj), C.POINTER(InflateParams), C.c_double, C.c_double, C.c_double, i64,
                                           vp, vp, vp, vp, vp, vp, vp]
        L.pct_bezier_check_batch.argtypes = [vp, C.POINTER(BezierBatch), C.POINTER(InflateParams), C.c_double, C.c_double, i64, vp, vp, i64,
                                             f64p, f64p, f64p, u32p]
        L.pct_bezier_check_batch_dev.argtypes = [vp, C.POINTER(BezierBatch), C.POINTER(InflateParams), C.c_double, C.c_double, i64, vp, vp, i64,
                                                 vp, vp, vp, vp, vp]
        L.pct_bezier_certify_batch.argtypes = [vp, i32, C.POINTER(BezierBatch), C.c_double, i32, i64, vp, vp]
        L.pct_bezier_certify_batch_dev.argtypes = [vp, i32, C.POINTER(BezierBatch), C.c_double, i32, i64, vp, vp, vp]
        L.pct_bezier_clearance_batch.argtypes = [vp, i32, C.POINTER(BezierBatch), C.c_double, C.c_double, i32, i64, vp, vp]
        L.pct_bezier_clearance_batch_dev.argtypes = [vp, i32, C.POINTER(BezierBatch), C.c_double, C.c_double, i32, i64, vp, vp, vp]
        L.pct_bezier_certify_window_batch.argtypes = [vp, i32, C.POINTER(BezierBatch), vp, C.c_double, i32, i64, vp, vp]
        L.pct_bezier_certify_window_batch_dev.argtypes = [vp, i32, C.POINTER(BezierBatch), vp, C.c_double, i32, i64, vp, vp, vp]
        L.pct_bezier_clearance_window_batch.argtypes = [vp, i32, C.POINTER(BezierBatch), vp, C.c_double, C.c_double, i32, i64, vp, vp]
        L.pct_bezier_clearance_window_batch_dev.argtypes = [vp, i32, C.POINTER(BezierBatch), vp, C.c_double, C.c_double, i32, i64, vp, vp, vp]
        L.pct_bezier_generate_batch.argtypes = [C.POINTER(TrajGenBatch), C.POINTER(TrajGenParams), f64p, i64, vp]
        L.pct_bezier_generate_batch_dev.argtypes = [C.POINTER(TrajGenBatch), C.POINTER(TrajGenParams), vp, i64, vp, vp]
        L.pct_time_allocation.argtypes = [f64p, f64p, i64, f64p, f64p, f64p, C.c_double, C.c_double, f64p]
        L.pct_bezier_generate_poly_batch.argtypes = [C.POINTER(TrajGenPolyBatch), C.POINTER(TrajGenParams), f64p, i64, vp]
        L.pct_bezier_generate_poly_batch_dev.argtypes = [C.POINTER(TrajGenPolyBatch), C.POINTER(TrajGenParams), vp, i64, vp, vp]
        L.pct_trajgen_max_planes.argtypes = []
        L.pct_trajgen_max_planes.restype = C.c_int
        L.pct_radius_count_batch_dev.argtypes = [vp, i32, vp, vp, i64, vp, vp]
        L.pct_cloud_reserve_queries.argtypes = [vp, i64]
        L.pct_plan_create_nn.argtypes = [vp, i32, i64, C.POINTER(vp)]
        L.pct_plan_run.argtypes = [vp, f32p, u32p, f64p]
        L.pct_plan_destroy.argtypes = [vp]
        L.pct_cloud_ring_index.argtypes = [vp, C.c_float, vp]
        L.pct_cloud_ring_drop.argtypes = [vp]
        L.pct_cloud_has_ring_index.argtypes = [vp]
        L.pct_cloud_ring_info.argtypes = [vp, C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(i64)]
        L.pct_cloud_ring_dedup.argtypes = [vp, C.c_double]
        L.pct_cloud_ring_dedup_last.argtypes = [vp, C.POINTER(i64), C.POINTER(i64), vp, i64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        L.pct_cloud_ring_remove_ball.argtypes = [vp, f64p, C.c_double, C.c_int, C.POINTER(i64)]
        L.pct_cloud_ring_remove_box.argtypes = [vp, f64p, f64p, C.c_int, C.POINTER(i64)]
        L.pct_cloud_ring_remove_indices.argtypes = [vp, u32p, i64, C.POINTER(i64)]
        L.pct_cloud_ring_live.argtypes = [vp, C.POINTER(i64), C.POINTER(i64)]
        L.pct_cloud_ring_compact.argtypes = [vp, C.POINTER(i64), C.POINTER(i64), u32p, i64]
        L.pct_cloud_ring_autocompact.argtypes = [vp, C.c_double]
        L.pct_cloud_ring_compact_count.argtypes = [vp, C.POINTER(C.c_uint64)]
        L.pct_cloud_ring_remove_outliers.argtypes = [vp, C.c_double, C.c_int32, i64, C.POINTER(i64)]
        L.pct_cloud_ring_neighbour_counts.argtypes = [vp, C.c_double, C.c_int32, i64, u32p, i64]
        L.pct_cloud_ring_knn_mean_distances.argtypes = [vp, C.c_int32, i64, f64p, i64]
        L.pct_cloud_ring_knn_distance_stats.argtypes = [vp, C.c_int32, C.c_double, i64, C.POINTER(KnnStats)]
        L.pct_cloud_ring_remove_statistical.argtypes = [vp, C.c_int32, C.c_double, i64, C.POINTER(i64), C.POINTER(KnnStats)]
        L.pct_cloud_ring_remove_isolated.argtypes = [vp, C.c_int32, C.c_double, i64, C.POINTER(i64)]
        L.pct_cloud_ring_carve_depth.argtypes = [vp, C.POINTER(DepthView), vp, C.c_double, C.POINTER(i64)]
        L.pct_cloud_append_depth.argtypes = [vp, C.POINTER(DepthView), vp, C.c_double, C.POINTER(i64), C.POINTER(i64)]
        L.pct_depth_classify.argtypes = [vp, vp, C.c_int32, f64p, i64, C.c_double, vp, vp]
        L.pct_cloud_ring_carve_range.argtypes = [vp, C.POINTER(RangeView), vp, C.c_double, C.POINTER(i64)]
        L.pct_cloud_append_range.argtypes = [vp, C.POINTER(RangeView), vp, C.c_double, C.POINTER(i64), C.POINTER(i64)]
        L.pct_range_classify.argtypes = [vp, vp, C.c_int32, f64p, i64, C.c_double, vp, vp]
        L.pct_range_pseudo_angle.argtypes = [C.c_double, C.c_double]
        L.pct_range_pseudo_angle.restype = C.c_double
        L.pct_debug_ring_slot.argtypes = [vp, i64, C.POINTER(C.c_uint32)]
        L.pct_debug_narrow_offsets.argtypes = [i64, i64, i64]
        L.pct_debug_query_bins.argtypes = [C.POINTER(C.c_int32), C.POINTER(C.c_float), C.c_float, C.c_int, C.c_int, vp, i64, vp,
                                           C.POINTER(C.c_uint32), C.POINTER(C.c_int)]
        L.pct_ctrl_points_check.argtypes = [vp, C.POINTER(BezierTraj), C.POINTER(InflateParams), C.c_double, C.POINTER(i64), C.POINTER(i64),
                                            i64, f64p, f64p, f64p, u32p]
        L.pct_plan_create_replan.argtypes = [vp, C.c_int32, C.c_int32, C.c_int32, C.POINTER(vp)]
        L.pct_plan_last_run_us.argtypes = [vp, C.POINTER(C.c_double)]
        L.pct_plan_replan_run.argtypes = [vp, C.POINTER(InflateParams), f64p, i64, C.POINTER(BezierTraj), C.c_double, C.c_double, C.c_double,
                                          C.c_int, C.POINTER(ReplanOut)]
        L.pct_last_kernel_ms.argtypes = [vp, C.POINTER(C.c_float)]
        L.pct_last_batch_ms.argtypes = [vp, C.POINTER(C.c_float)]
        L.pct_kernel_ms_history.argtypes = [vp, C.POINTER(C.c_float), C.c_int, C.POINTER(C.c_int)]
        L.pct_cloud_frame_buffer.argtypes = [vp, i64, C.POINTER(vp)]
        L.pct_cloud_append_frame.argtypes = [vp, i64, i64]
        L.pct_debug_read_grid.argtypes = [vp, vp, vp]
        L.pct_set_timing.argtypes = [vp, C.c_int]
        L.pct_set_timing_stride.argtypes = [vp, C.c_int]
        L.pct_kernel_ms_samples.argtypes = [vp, C.POINTER(C.c_uint64)]
        L.pct_merge_mask_dev.argtypes = [vp, vp, vp, vp, i64, vp]
        L.pct_last_work.argtypes = [vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        L.pct_set_work_counters.argtypes = [vp, i32]
        L.pct_last_work_ex.argtypes = [vp, C.POINTER(C.c_uint64)]
        L.pct_debug_verify_grid.argtypes = [vp, C.POINTER(C.c_uint64)]
        L.pct_debug_live_buffers.argtypes = [C.POINTER(i64), C.POINTER(i64)]
        L.pct_cloud_pyramid_info.argtypes = [vp, C.POINTER(C.c_int32), C.POINTER(i64), C.POINTER(C.c_double)]
        _lib = L
    return _lib


def _chk(code):
    if code != 0:
        raise EngineError(code, lib().pct_last_error().decode(errors="replace"))


def init(device: int = 0):
    _chk(lib().pct_init(device))


def device_count() -> int:
    return lib().pct_device_count()


def polyhedron_lds_rows() -> int:
    """the longest capsule row the free-space-polyhedron filter keeps in LDS in one piece (pct_polyhedron_lds_rows; needs no GPU)"""
    return int(lib().pct_polyhedron_lds_rows())


def sync():
    _chk(lib().pct_sync())


def live_buffers():
    """(blocks, bytes) of device, pinned and host-mapped memory the library holds right now (pct_debug_live_buffers)"""
    blocks, nbytes = C.c_int64(), C.c_int64()
    _chk(lib().pct_debug_live_buffers(C.byref(blocks), C.byref(nbytes)))
    return blocks.value, nbytes.value


def set_filter_mode(mode: int):
    """-1 automatic, 0 direct (p-q)^2 filter, 1 expanded |p|^2 - 2 p.q filter (pct_debug_set_filter_mode); results are identical"""
    _chk(lib().pct_debug_set_filter_mode(int(mode)))


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def merge_mask_device(d2_local_ptr: int, d2_best_ptr: int, idx_local_ptr: int, cand_ptr: int, Q: int, stream: int = 0):
    """cand[i] = idx_local[i] where d2_local[i] is the reduced minimum (and finite), INT32_MAX elsewhere (pct_merge_mask_dev)"""
    _chk(lib().pct_merge_mask_dev(d2_local_ptr, d2_best_ptr, idx_local_ptr, cand_ptr, int(Q), stream))


def inflate_params(start, sample_range, search_margin, max_radius) -> InflateParams:
    p = InflateParams()
    p.start[:] = [float(v) for v in start]
    p.sample_range, p.search_margin, p.max_radius = float(sample_range), float(search_margin), float(max_radius)
    return p


class Cloud:
    """An obstacle cloud resident in HBM (pct_cloud).  Mirrors the planner seam:
    set_input ~ safeRegionRrtStar::setInput (corridor_finder.cpp:93-99), inflate ~ radiusSearch
    (:113-133), bezier_check ~ checkSafeTrajectory (sim_planning_demo.cpp:729-781)."""

    def __init__(self, capacity: int):
        self._h = C.c_void_p()
        _chk(lib().pct_cloud_create(int(capacity), C.byref(self._h)))

    @classmethod
    def borrowed(cls, handle):
        """a Cloud over a pct_cloud that someone else owns (the corridor finder's map): close() leaves it alone"""
        c = cls.__new__(cls)
        c._h, c._owned = handle, False
        return c

    def close(self):
        if getattr(self, "_h", None) and self._h.value and _lib is not None:
            if getattr(self, "_owned", True):
                _lib.pct_cloud_destroy(self._h)
            self._h = C.c_void_p()

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    @property
    def handle(self):
        return self._h

    def __len__(self):
        return lib().pct_cloud_size(self._h)

    @property
    def capacity(self):
        return lib().pct_cloud_capacity(self._h)

    def set_index_base(self, base: int):
        _chk(lib().pct_cloud_set_index_base(self._h, int(base)))

    @staticmethod
    def _aos(points):
        a = np.asarray(points)
        if a.dtype != np.float32 or not a.flags.c_contiguous:
            a = np.ascontiguousarray(a, np.float32)
        if a.ndim != 2 or a.shape[1] not in (3, 4):
            raise ValueError("points must be (n,3) packed xyz or (n,4) pcl::PointXYZ-style records")
        return a, a.shape[1] * 4

    def set_input(self, points):
        a, stride = self._aos(points)
        _chk(lib().pct_cloud_upload_aos(self._h, _ptr(a), len(a), stride))

    def set_input_pointcloud2(self, data: bytes, n: int, point_step: int, off_x: int, off_y: int, off_z: int):
        """sensor_msgs/PointCloud2 payload: `data` = msg.data, offsets = msg.fields[*].offset"""
        buf = np.frombuffer(data, np.uint8)
        _chk(lib().pct_cloud_upload_fields(self._h, _ptr(buf), int(n), int(point_step), int(off_x), int(off_y), int(off_z)))

    def set_input_device(self, x_ptr: int, y_ptr: int, z_ptr: int, n: int):
        _chk(lib().pct_cloud_upload_soa_dev(self._h, x_ptr, y_ptr, z_ptr, int(n)))

    def append(self, points):
        a, stride = self._aos(points)
        _chk(lib().pct_cloud_append_aos(self._h, _ptr(a), len(a), stride))

    def frame_buffer(self, n: int, floats_per_point: int = 3):
        """host-mapped staging buffer for zero-copy appends, as a float32 [n, floats_per_point] array the producer fills in place"""
        p = C.c_void_p()
        _chk(lib().pct_cloud_frame_buffer(self._h, int(n) * floats_per_point * 4, C.byref(p)))
        return np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_float)), shape=(int(n), floats_per_point))

    def append_frame(self, n: int, floats_per_point: int = 3):
        """append the first n records of the frame buffer (pct_cloud_append_frame)"""
        _chk(lib().pct_cloud_append_frame(self._h, int(n), floats_per_point * 4))

    def build_grid(self, cell_size: float = 0.0):
        _chk(lib().pct_cloud_build_grid(self._h, float(cell_size)))

    def drop_grid(self):
        _chk(lib().pct_cloud_drop_grid(self._h))

    @property
    def has_grid(self) -> bool:
        return bool(lib().pct_cloud_has_grid(self._h))

    def grid_info(self):
        dims = (C.c_int32 * 3)()
        h = C.c_float()
        org = (C.c_float * 3)()
        nc = C.c_int64()
        _chk(lib().pct_cloud_grid_info(self._h, dims, C.byref(h), org, C.byref(nc)))
        return dict(dims=tuple(dims), cell_size=h.value, origin=tuple(org), ncells=nc.value)

    def ring_index(self, cell_size: float = 0.0, extent=None):
        """rolling-map index (pct_cloud_ring_index): appends update it in place instead of dropping an index"""
        ext = None if extent is None else np.ascontiguousarray(extent, np.float32).reshape(3)
        _chk(lib().pct_cloud_ring_index(self._h, float(cell_size), None if ext is None else ext.ctypes.data))

    def ring_drop(self):
        _chk(lib().pct_cloud_ring_drop(self._h))

    @property
    def has_ring_index(self) -> bool:
        return bool(lib().pct_cloud_has_ring_index(self._h))

    def ring_info(self):
        dims = (C.c_int32 * 3)()
        h = C.c_double()
        ov = C.c_int64()
        _chk(lib().pct_cloud_ring_info(self._h, dims, C.byref(h), C.byref(ov)))
        return dict(dims=tuple(dims), cell_size=h.value, overflow_entries=ov.value, bucket_records=int(lib().pct_cloud_ring_bucket_records(self._h)))

    def ring_dedup(self, res: float):
        """de-duplicating appends (pct_cloud_ring_dedup): res > 0 keeps only points whose voxel is new to the window, 0 turns it off"""
        _chk(lib().pct_cloud_ring_dedup(self._h, float(res)))

    def ring_dedup_last(self):
        """the last filtered append: offered / kept counts, the kept flag per offered point, totals since the mode was enabled"""
        off, kept = C.c_int64(), C.c_int64()
        toff, tkept = C.c_uint64(), C.c_uint64()
        _chk(lib().pct_cloud_ring_dedup_last(self._h, C.byref(off), C.byref(kept), None, 0, C.byref(toff), C.byref(tkept)))
        flags = np.zeros(off.value, np.uint8)
        if off.value:
            _chk(lib().pct_cloud_ring_dedup_last(self._h, None, None, flags.ctypes.data, len(flags), None, None))
        return dict(offered=off.value, kept=kept.value, flags=flags.astype(bool), total_offered=toff.value, total_kept=tkept.value)

    def ring_remove_ball(self, centre, r: float, outside: bool = False) -> int:
        """remove the points within r of centre from the rolling map (outside = True: those farther than r, "forget"); the removed
        points become NaN rows, every other point keeps its index (pct_cloud_ring_remove_ball); returns the number removed"""
        q = np.ascontiguousarray(centre, np.float64).reshape(3)
        n = C.c_int64()
        _chk(lib().pct_cloud_ring_remove_ball(self._h, _ptr(q), float(r), int(bool(outside)), C.byref(n)))
        return n.value

    def ring_remove_box(self, lo, hi, outside: bool = False) -> int:
        """remove the points with lo <= p <= hi on all three axes (outside = True: every other point); returns the number removed"""
        a, b = np.ascontiguousarray(lo, np.float64).reshape(3), np.ascontiguousarray(hi, np.float64).reshape(3)
        n = C.c_int64()
        _chk(lib().pct_cloud_ring_remove_box(self._h, _ptr(a), _ptr(b), int(bool(outside)), C.byref(n)))
        return n.value

    def ring_remove_indices(self, indices) -> int:
        """remove the points with these indices (as the searches report them); a point named twice counts once; returns the number
        removed.  An index outside the window raises and removes nothing."""
        idx = np.ascontiguousarray(indices, np.uint32).reshape(-1)
        n = C.c_int64()
        _chk(lib().pct_cloud_ring_remove_indices(self._h, _ptr(idx), len(idx), C.byref(n)))
        return n.value

    def ring_live(self):
        """(live, not live): rows of the window without a NaN coordinate, and len(self) minus that (pct_cloud_ring_live)"""
        a, b = C.c_int64(), C.c_int64()
        _chk(lib().pct_cloud_ring_live(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def ring_compact(self, want_remap: bool = False):
        """compact the window after removals (pct_cloud_ring_compact): the live rows move to slots 0 .. L-1 in arrival order and the
        next appends fill the reclaimed slots.  Returns (live, reclaimed), and with want_remap the uint32 array that maps every old
        slot to its new index (index base included) or NO_INDEX for a dropped row"""
        live, rec = C.c_int64(), C.c_int64()
        if not want_remap:
            _chk(lib().pct_cloud_ring_compact(self._h, C.byref(live), C.byref(rec), None, 0))
            return live.value, rec.value
        remap = np.empty(len(self), np.uint32)
        _chk(lib().pct_cloud_ring_compact(self._h, C.byref(live), C.byref(rec), _ptr(remap), len(remap)))
        return live.value, rec.value, remap

    def ring_autocompact(self, fraction: float):
        """a removal that leaves fraction * capacity or more dead slots below the size compacts before it returns; 0 turns it off"""
        _chk(lib().pct_cloud_ring_autocompact(self._h, float(fraction)))

    def ring_compact_count(self) -> int:
        """compactions that moved rows since the cloud was created: indices held across a call are stale when it has changed"""
        n = C.c_uint64()
        _chk(lib().pct_cloud_ring_compact_count(self._h, C.byref(n)))
        return n.value

    def ring_remove_outliers(self, r: float, min_neighbours: int, newest: int = 0) -> int:
        """radius outlier removal on the window itself (pct_cloud_ring_remove_outliers): of the `newest` most recent rows (0: every
        row), those with fewer than min_neighbours other rows of the window within r are removed -- one judgement on the window as it
        is, then one removal; returns the number removed"""
        n = C.c_int64()
        _chk(lib().pct_cloud_ring_remove_outliers(self._h, float(r), int(min_neighbours), int(newest), C.byref(n)))
        return n.value

    def ring_neighbour_counts(self, r: float, count_cap: int, newest: int = 0):
        """the same judgement without the removal (pct_cloud_ring_neighbour_counts): uint32 [len(self)], min(neighbours, count_cap)
        for a judged row, NO_INDEX for a row that holds a NaN or is out of scope"""
        counts = np.empty(len(self), np.uint32)
        _chk(lib().pct_cloud_ring_neighbour_counts(self._h, float(r), int(count_cap), int(newest), _ptr(counts), len(counts)))
        return counts

    def ring_knn_mean_distances(self, k: int, newest: int = 0):
        """every judged row's mean distance to its k nearest other rows of the window (pct_cloud_ring_knn_mean_distances): float64
        [len(self)], +inf for a judged row with fewer than k candidates, NaN for a row that holds a NaN or is out of scope"""
        mean = np.empty(max(len(self), 1), np.float64)
        _chk(lib().pct_cloud_ring_knn_mean_distances(self._h, int(k), int(newest), _ptr(mean), len(mean)))
        return mean[:len(self)]

    def ring_knn_distance_stats(self, k: int, stddev_mult: float, newest: int = 0) -> dict:
        """the statistics of those means in the contract's tree order (pct_cloud_ring_knn_distance_stats): dict(measured, sum, sum_sq,
        mean, stddev, threshold = mean + stddev_mult * stddev); changes nothing in the cloud"""
        st = KnnStats()
        _chk(lib().pct_cloud_ring_knn_distance_stats(self._h, int(k), float(stddev_mult), int(newest), C.byref(st)))
        return st.as_dict()

    def ring_remove_statistical(self, k: int, stddev_mult: float, newest: int = 0):
        """statistical outlier removal on the window itself (pct_cloud_ring_remove_statistical): of the `newest` most recent rows (0:
        every row), those whose k-NN mean distance is greater than mean + stddev_mult * stddev over the judged rows are removed;
        returns (removed, the statistics as ring_knn_distance_stats returns them)"""
        n, st = C.c_int64(), KnnStats()
        _chk(lib().pct_cloud_ring_remove_statistical(self._h, int(k), float(stddev_mult), int(newest), C.byref(n), C.byref(st)))
        return n.value, st.as_dict()

    def ring_remove_isolated(self, k: int, max_mean_distance: float, newest: int = 0) -> int:
        """the same removal under a fixed threshold (pct_cloud_ring_remove_isolated), the per-frame call: a judged row whose k-NN mean
        distance is greater than max_mean_distance (or that has fewer than k candidates) is removed; returns the number removed"""
        n = C.c_int64()
        _chk(lib().pct_cloud_ring_remove_isolated(self._h, int(k), float(max_mean_distance), int(newest), C.byref(n)))
        return n.value

    def ring_carve_depth(self, view: DepthView, image, margin: float) -> int:
        """free-space clearing (pct_cloud_ring_carve_depth): remove every point the depth image sees through -- in the image, its
        pixel finite and strictly farther than the point plus margin; the removed points become NaN rows; returns the number removed"""
        img = depth_image(view, image)
        n = C.c_int64()
        _chk(lib().pct_cloud_ring_carve_depth(self._h, C.byref(view), _ptr(img), float(margin), C.byref(n)))
        return n.value

    def append_depth(self, view: DepthView, image, max_depth: float = float("inf")):
        """un-project the valid pixels of a z-depth image on the device and append them as append() appends the same points
        (pct_cloud_append_depth); returns (offered = valid pixels, kept = points the window took)"""
        img = depth_image(view, image)
        off, kept = C.c_int64(), C.c_int64()
        _chk(lib().pct_cloud_append_depth(self._h, C.byref(view), _ptr(img), float(max_depth), C.byref(off), C.byref(kept)))
        return off.value, kept.value

    def ring_carve_range(self, view: RangeView, image, margin: float) -> int:
        """free-space clearing along a lidar's beams (pct_cloud_ring_carve_range): remove every point the range image sees through -- in
        the image, its pixel finite and strictly farther than the point plus margin; returns the number removed"""
        img = depth_image(view, image)
        n = C.c_int64()
        _chk(lib().pct_cloud_ring_carve_range(self._h, C.byref(view), _ptr(img), float(margin), C.byref(n)))
        return n.value

    def append_range(self, view: RangeView, image, max_range: float = float("inf")):
        """un-project the valid pixels of a range image on the device, from the view's direction tables, and append them as append()
        appends the same points (pct_cloud_append_range); returns (offered = valid pixels, kept = points the window took)"""
        img = depth_image(view, image)
        off, kept = C.c_int64(), C.c_int64()
        _chk(lib().pct_cloud_append_range(self._h, C.byref(view), _ptr(img), float(max_range), C.byref(off), C.byref(kept)))
        return off.value, kept.value

    def debug_ring_slot(self, slot: int):
        """pct_debug_ring_slot: (where word, bucket, head, tail, id word at the filed position, overflow-queue length) -- test hook"""
        out = (C.c_uint32 * 6)()
        _chk(lib().pct_debug_ring_slot(self._h, int(slot), out))
        return tuple(int(v) for v in out)

    def reserve_queries(self, Q: int):
        _chk(lib().pct_cloud_reserve_queries(self._h, int(Q)))

    def nn(self, queries, algo: int = ALGO_AUTO):
        q = np.ascontiguousarray(queries, np.float32).reshape(-1, 3)
        idx = np.empty(len(q), np.uint32)
        d2 = np.empty(len(q), np.float64)
        _chk(lib().pct_nn_batch_algo(self._h, algo, _ptr(q), len(q), _ptr(idx), _ptr(d2)))
        return idx, d2

    def knn(self, queries, k: int, algo: int = ALGO_AUTO):
        """the k nearest points of every query (pct_knn_batch_algo): (idx uint32 [Q, k], d2 float64 [Q, k]), each row nearest first,
        ties in ascending index, padded with NO_INDEX / +inf where fewer than k points lie at a finite distance"""
        q = np.ascontiguousarray(queries, np.float32).reshape(-1, 3)
        kk = max(int(k), 0)
        idx = np.empty((len(q), kk), np.uint32)
        d2 = np.empty((len(q), kk), np.float64)
        _chk(lib().pct_knn_batch_algo(self._h, algo, _ptr(q), len(q), int(k), _ptr(idx), _ptr(d2)))
        return idx, d2

    def radius_count(self, queries, radii, algo: int = ALGO_AUTO):
        q = np.ascontiguousarray(queries, np.float32).reshape(-1, 3)
        r = np.ascontiguousarray(np.broadcast_to(np.asarray(radii, np.float32), (len(q),)))
        cnt = np.empty(len(q), np.uint32)
        _chk(lib().pct_radius_count_batch_algo(self._h, algo, _ptr(q), _ptr(r), len(q), _ptr(cnt)))
        return cnt

    def radius_search(self, queries, radii, order: int = ORDER_DISTANCE, algo: int = ALGO_AUTO):
        """which points lie within radii[i] of queries[i] (pct_radius_search_batch + pct_radius_search_read): (offsets int64 [Q + 1],
        idx uint32 [total], d2 float64 [total]); row i = entries offsets[i] .. offsets[i + 1], nearest first with ties in ascending
        index (ORDER_DISTANCE) or in ascending index (ORDER_INDEX).  A scalar radius broadcasts."""
        q = np.ascontiguousarray(queries, np.float32).reshape(-1, 3)
        r = np.ascontiguousarray(np.broadcast_to(np.asarray(radii, np.float32), (len(q),)))
        offsets = np.zeros(len(q) + 1, np.int64)
        total = C.c_int64()
        _chk(lib().pct_radius_search_batch(self._h, algo, _ptr(q), _ptr(r), len(q), int(order), _ptr(offsets), C.byref(total)))
        idx = np.empty(total.value, np.uint32)
        d2 = np.empty(total.value, np.float64)
        _chk(lib().pct_radius_search_read(self._h, 0, total.value, _ptr(idx), _ptr(d2)))
        return offsets, idx, d2

    def radius_search_read(self, first: int, n: int, want_idx: bool = True, want_d2: bool = True):
        """entries [first, first + n) of the last radius_search on this cloud (pct_radius_search_read): (idx or None, d2 or None)"""
        idx = np.empty(max(int(n), 0), np.uint32) if want_idx else None
        d2 = np.empty(max(int(n), 0), np.float64) if want_d2 else None
        _chk(lib().pct_radius_search_read(self._h, int(first), int(n), None if idx is None else _ptr(idx), None if d2 is None else _ptr(d2)))
        return idx, d2

    def radius_indices(self, center, radius, cap=None):
        q = np.ascontiguousarray(center, np.float32).reshape(3)
        cap = int(cap if cap is not None else max(len(self), 1))
        out = np.empty(cap, np.uint32)
        n = C.c_int64()
        _chk(lib().pct_radius_indices(self._h, _ptr(q), float(radius), _ptr(out), cap, C.byref(n)))
        return out[:min(n.value, cap)].copy(), n.value

    # fp64-query forms (kd_nearest / kd_nearest_range with double positions): exhaustive, d2 = ((dx*dx + dy*dy) + dz*dz) in fp64
    def nn_q64(self, queries):
        """pct_nn_batch_q64: (idx uint32 [Q], d2 float64 [Q]) for double queries"""
        q = np.ascontiguousarray(queries, np.float64).reshape(-1, 3)
        idx = np.empty(len(q), np.uint32)
        d2 = np.empty(len(q), np.float64)
        _chk(lib().pct_nn_batch_q64(self._h, _ptr(q), len(q), _ptr(idx), _ptr(d2)))
        return idx, d2

    def nn_q64_ties(self, queries, want_ties: bool = True):
        """pct_nn_batch_q64_ties: (idx, d2, ties uint32 [Q]); ties[i] = points at the minimum where the path taken counts them,
        0 elsewhere; want_ties = False passes ties = NULL and returns None in its place"""
        q = np.ascontiguousarray(queries, np.float64).reshape(-1, 3)
        idx = np.empty(len(q), np.uint32)
        d2 = np.empty(len(q), np.float64)
        ties = np.empty(len(q), np.uint32) if want_ties else None
        _chk(lib().pct_nn_batch_q64_ties(self._h, _ptr(q), len(q), _ptr(idx), _ptr(d2), None if ties is None else _ptr(ties)))
        return idx, d2, ties

    def _radius_indices_q64(self, fn, center, value, cap):
        q = np.ascontiguousarray(center, np.float64).reshape(3)
        cap = int(cap if cap is not None else max(len(self), 1))
        out = np.empty(max(cap, 1), np.uint32)
        n = C.c_int64()
        _chk(fn(self._h, _ptr(q), float(value), _ptr(out), cap, C.byref(n)))
        return out[:min(n.value, cap)].copy(), n.value

    def radius_indices_q64(self, center, radius, cap=None):
        """pct_radius_indices_q64: (the min(hits, cap) lowest indices with d2 <= radius * radius, ascending; hits)"""
        return self._radius_indices_q64(lib().pct_radius_indices_q64, center, radius, cap)

    def radius_indices_r2_q64(self, center, r2, cap=None):
        """pct_radius_indices_r2_q64: the same with the squared radius given exactly (d2 <= r2)"""
        return self._radius_indices_q64(lib().pct_radius_indices_r2_q64, center, r2, cap)

    def radius_indices_batch_q64(self, centers, radii, cap_per_query: int):
        """pct_radius_indices_batch_q64: (ids uint32 [K, cap_per_query] in arrival order, counts int64 [K]); counts[k] >= 0: all hits
        stored; < 0: -(hits), the row is truncated"""
        q = np.ascontiguousarray(centers, np.float64).reshape(-1, 3)
        r = np.ascontiguousarray(np.broadcast_to(np.asarray(radii, np.float64), (len(q),)))
        ids = np.full((len(q), max(int(cap_per_query), 1)), NO_INDEX, np.uint32)
        counts = np.zeros(len(q), np.int64)
        _chk(lib().pct_radius_indices_batch_q64(self._h, _ptr(q), _ptr(r), len(q), _ptr(ids), int(cap_per_query), _ptr(counts)))
        return ids, counts

    def radius_crop(self, center, radius, sort_by_distance=False):
        """lidar crop (camera_sensor.cpp:133-145): (indices u32, d2 fp64, cropped cloud float32 [k,3]) of the points within radius"""
        q = np.ascontiguousarray(center, np.float64).reshape(3)
        cap = max(len(self), 1)
        idx, d2, xyz = np.empty(cap, np.uint32), np.empty(cap, np.float64), np.empty((cap, 3), np.float32)
        n = C.c_int64()
        _chk(lib().pct_radius_crop(self._h, q.ctypes.data, float(radius), int(bool(sort_by_distance)), cap, idx.ctypes.data,
                                   d2.ctypes.data, xyz.ctypes.data, C.byref(n)))
        k = min(n.value, cap)
        return idx[:k].copy(), d2[:k].copy(), xyz[:k].copy()

    def crop_to(self, center, radius, dst: "Cloud"):
        """dst := points within radius of center, in this cloud's order, device to device"""
        q = np.ascontiguousarray(center, np.float64).reshape(3)
        _chk(lib().pct_cloud_crop_to(self._h, q.ctypes.data, float(radius), dst._h))

    def inflate(self, params: InflateParams, points):
        p = np.ascontiguousarray(points, np.float64).reshape(-1, 3)
        rad = np.empty(len(p), np.float64)
        idx = np.empty(len(p), np.uint32)
        d2 = np.empty(len(p), np.float64)
        _chk(lib().pct_inflate_batch(self._h, C.byref(params), _ptr(p), len(p), _ptr(rad), _ptr(idx), _ptr(d2)))
        return rad, idx, d2

    def segment_nn(self, segments, reach, algo: int = ALGO_AUTO):
        """the nearest point to every line segment within its reach (pct_segment_nn_batch): segments [Q, 6] (a then b) or [Q, 2, 3],
        reach a scalar or [Q]; (idx uint32 [Q], d2 float64 [Q], s float64 [Q]) -- NO_INDEX / +inf / NaN where no point is that near"""
        seg = np.ascontiguousarray(segments, np.float64).reshape(-1, 6)
        r = np.ascontiguousarray(np.broadcast_to(np.asarray(reach, np.float64), (len(seg),)))
        idx = np.empty(len(seg), np.uint32)
        d2 = np.empty(len(seg), np.float64)
        s = np.empty(len(seg), np.float64)
        _chk(lib().pct_segment_nn_batch(self._h, algo, _ptr(seg), _ptr(r), len(seg), _ptr(idx), _ptr(d2), _ptr(s)))
        return idx, d2, s

    def segment_inflate(self, segments, params: InflateParams):
        """capsule inflation (pct_segment_inflate_batch): (radius float64 [Q], idx uint32 [Q], s float64 [Q]); radius < 0: the segment
        collides; idx / s name the nearest point where radius < max_radius"""
        seg = np.ascontiguousarray(segments, np.float64).reshape(-1, 6)
        rad = np.empty(len(seg), np.float64)
        idx = np.empty(len(seg), np.uint32)
        s = np.empty(len(seg), np.float64)
        _chk(lib().pct_segment_inflate_batch(self._h, C.byref(params), _ptr(seg), len(seg), _ptr(rad), _ptr(idx), _ptr(s)))
        return rad, idx, s

    def segment_sweep(self, segments, radius, algo: int = ALGO_AUTO):
        """the first contact of a sphere swept along every segment (pct_segment_sweep_batch): segments [Q, 6] (a then b) or [Q, 2, 3],
        radius a scalar or [Q]; (idx uint32 [Q], t float64 [Q]) -- the point that stops the sphere and how far along a -> b its centre
        gets (0: in contact at the start); NO_INDEX / 1.0 where nothing blocks, NO_INDEX / NaN for an invalid sweep"""
        seg = np.ascontiguousarray(segments, np.float64).reshape(-1, 6)
        r = np.ascontiguousarray(np.broadcast_to(np.asarray(radius, np.float64), (len(seg),)))
        idx = np.empty(len(seg), np.uint32)
        t = np.empty(len(seg), np.float64)
        _chk(lib().pct_segment_sweep_batch(self._h, algo, _ptr(seg), _ptr(r), len(seg), _ptr(idx), _ptr(t)))
        return idx, t

    def segment_count(self, segments, reach, algo: int = ALGO_AUTO):
        """how many points lie within reach of every line segment (pct_segment_count_batch): segments [Q, 6] (a then b) or [Q, 2, 3],
        reach a scalar or [Q]; uint32 [Q]"""
        seg = np.ascontiguousarray(segments, np.float64).reshape(-1, 6)
        r = np.ascontiguousarray(np.broadcast_to(np.asarray(reach, np.float64), (len(seg),)))
        cnt = np.empty(len(seg), np.uint32)
        _chk(lib().pct_segment_count_batch(self._h, algo, _ptr(seg), _ptr(r), len(seg), _ptr(cnt)))
        return cnt

    def segment_search(self, segments, reach, order: int = ORDER_DISTANCE, algo: int = ALGO_AUTO):
        """which points lie within reach of every line segment (pct_segment_search_batch + pct_segment_search_read): segments [Q, 6]
        (a then b) or [Q, 2, 3], reach a scalar or [Q]; (offsets int64 [Q + 1], idx uint32 [total], d2 float64 [total], s float64
        [total]); row i = entries offsets[i] .. offsets[i + 1], nearest first with ties in ascending index (ORDER_DISTANCE) or in
        ascending index (ORDER_INDEX); s is the parameter of the closest point on the segment (0 at a, 1 at b)"""
        seg = np.ascontiguousarray(segments, np.float64).reshape(-1, 6)
        r = np.ascontiguousarray(np.broadcast_to(np.asarray(reach, np.float64), (len(seg),)))
        offsets = np.zeros(len(seg) + 1, np.int64)
        total = C.c_int64()
        _chk(lib().pct_segment_search_batch(self._h, algo, _ptr(seg), _ptr(r), len(seg), int(order), _ptr(offsets), C.byref(total)))
        idx = np.empty(total.value, np.uint32)
        d2 = np.empty(total.value, np.float64)
        s = np.empty(total.value, np.float64)
        _chk(lib().pct_segment_search_read(self._h, 0, total.value, _ptr(idx), _ptr(d2), _ptr(s)))
        return offsets, idx, d2, s

    def segment_search_read(self, first: int, n: int, want_idx: bool = True, want_d2: bool = True, want_s: bool = True):
        """entries [first, first + n) of the last segment_search on this cloud (pct_segment_search_read): (idx, d2, s), None where not
        wanted"""
        idx = np.empty(max(int(n), 0), np.uint32) if want_idx else None
        d2 = np.empty(max(int(n), 0), np.float64) if want_d2 else None
        s = np.empty(max(int(n), 0), np.float64) if want_s else None
        _chk(lib().pct_segment_search_read(self._h, int(first), int(n), None if idx is None else _ptr(idx), None if d2 is None else _ptr(d2),
                                           None if s is None else _ptr(s)))
        return idx, d2, s

    def segment_polyhedron(self, segments, reach, algo: int = ALGO_AUTO):
        """a convex free region around every line segment as half-spaces (pct_segment_polyhedron_batch + pct_segment_polyhedron_read):
        segments [Q, 6] (a then b) or [Q, 2, 3], reach a scalar or [Q]; (offsets int64 [Q + 1], idx uint32 [total], d2 float64 [total],
        s float64 [total], planes float64 [total, 4]); row i = the supports of segment i, nearest first; a plane is nh0 nh1 nh2 off and
        its half-space {y : nh . y <= off}; (0, 0, 0, -1) for a point on the segment (d2 == 0)"""
        seg = np.ascontiguousarray(segments, np.float64).reshape(-1, 6)
        r = np.ascontiguousarray(np.broadcast_to(np.asarray(reach, np.float64), (len(seg),)))
        offsets = np.zeros(len(seg) + 1, np.int64)
        total = C.c_int64()
        _chk(lib().pct_segment_polyhedron_batch(self._h, algo, _ptr(seg), _ptr(r), len(seg), _ptr(offsets), C.byref(total)))
        idx, d2, s, planes = self.segment_polyhedron_read(0, total.value)
        return offsets, idx, d2, s, planes

    def segment_polyhedron_read(self, first: int, n: int, want_idx: bool = True, want_d2: bool = True, want_s: bool = True, want_planes: bool = True):
        """entries [first, first + n) of the last segment_polyhedron on this cloud (pct_segment_polyhedron_read): (idx, d2, s, planes
        [n, 4]), None where not wanted"""
        m = max(int(n), 0)
        idx = np.empty(m, np.uint32) if want_idx else None
        d2 = np.empty(m, np.float64) if want_d2 else None
        s = np.empty(m, np.float64) if want_s else None
        planes = np.empty((m, 4), np.float64) if want_planes else None
        _chk(lib().pct_segment_polyhedron_read(self._h, int(first), int(n), *(None if a is None else _ptr(a) for a in (idx, d2, s, planes))))
        return idx, d2, s, planes

    def bezier_check(self, params: InflateParams, polycoef, seg_time, orders, t_start, stop_time, dt=0.02, cap=4096):
        coef = np.ascontiguousarray(polycoef, np.float64)
        st = np.ascontiguousarray(seg_time, np.float64)
        od = np.ascontiguousarray(orders, np.int32)
        traj = BezierTraj(coef.ctypes.data_as(C.POINTER(C.c_double)), coef.shape[1], st.ctypes.data_as(C.POINTER(C.c_double)),
                          od.ctypes.data_as(C.POINTER(C.c_int32)), len(st))
        pos = np.zeros((cap, 3), np.float64)
        rad = np.zeros(cap, np.float64)
        d2 = np.zeros(cap, np.float64)
        idx = np.zeros(cap, np.uint32)
        fh, ns = C.c_int64(), C.c_int64()
        _chk(lib().pct_bezier_check(self._h, C.byref(traj), C.byref(params), float(t_start), float(stop_time), float(dt),
                                    C.byref(fh), C.byref(ns), cap, _ptr(pos), _ptr(rad), _ptr(d2), _ptr(idx)))
        n = min(ns.value, cap)
        return dict(first_hit=fh.value, n=ns.value, pos=pos[:n], radius=rad[:n], d2=d2[:n], idx=idx[:n])

    def bezier_check_batch(self, params: InflateParams, trajectories, t_start=None, stop_time=2.0, dt=0.02, cap=4096, want_lists=False):
        """pct_bezier_check_batch: the sampled check for a list of (polycoef, seg_time, orders) candidates (or a packed
        (BezierBatch, arrays) pair from engine.pack_trajectories) in one call.  Returns a dict of numpy arrays, one entry per
        trajectory: nsamples (unclipped), first_hit (-1 = none), min_sample, min_radius; with want_lists also offsets [B + 1] and the
        rows pos [total, 3], radius, d2, idx [total], row b = entries [offsets[b], offsets[b + 1]) -- sized from offsets[B], by a
        second call when the first guess was too small."""
        packed = isinstance(trajectories, tuple) and len(trajectories) == 2 and isinstance(trajectories[0], BezierBatch)
        batch, keep = trajectories if packed else pack_trajectories(trajectories, t_start)
        B = int(batch.B)
        verdict = np.zeros(B, VERDICT_DTYPE)
        out = None
        if not want_lists:
            _chk(lib().pct_bezier_check_batch(self._h, C.byref(batch), C.byref(params), float(stop_time), float(dt), int(cap), _ptr(verdict),
                                              None, 0, None, None, None, None))
        else:
            offsets = np.zeros(B + 1, np.int64)
            room = 256 * B
            while True:
                pos = np.zeros((room, 3), np.float64)
                rad, d2, idx = np.zeros(room, np.float64), np.zeros(room, np.float64), np.zeros(room, np.uint32)
                _chk(lib().pct_bezier_check_batch(self._h, C.byref(batch), C.byref(params), float(stop_time), float(dt), int(cap), _ptr(verdict),
                                                  _ptr(offsets), room, _ptr(pos), _ptr(rad), _ptr(d2), _ptr(idx)))
                total = int(offsets[B])
                if total <= room:
                    break
                room = total
            out = dict(offsets=offsets, pos=pos[:total], radius=rad[:total], d2=d2[:total], idx=idx[:total])
        del keep
        res = {k: np.ascontiguousarray(verdict[k]) for k in VERDICT_DTYPE.names}
        if out:
            res.update(out)
        return res

    def bezier_certify(self, trajectories, margin, max_depth=12, piece_cap=None, algo: int = ALGO_AUTO):
        """pct_bezier_certify_batch: whole trajectories proven free of the cloud by `margin`, or shown to collide, by subdivision -- no
        dt.  trajectories: a list of (polycoef, seg_time, orders), or a packed (BezierBatch, arrays) pair from engine.pack_trajectories
        (t_start is not read).  piece_cap: the most pieces a round may hold (None: 64 per segment, at least 4096).  Returns
        (certificates, stats): a structured array of engine.CERT_DTYPE, one entry per trajectory -- status (CERT_FREE, CERT_HIT,
        CERT_UNDECIDED, CERT_INVALID), depth, hit_seg, hit_idx, hit_u, hit_d2, min_d2, pieces -- and
        dict(rounds, pieces, capped)."""
        packed = isinstance(trajectories, tuple) and len(trajectories) == 2 and isinstance(trajectories[0], BezierBatch)
        batch, keep = trajectories if packed else pack_trajectories(trajectories)
        B = int(batch.B)
        if piece_cap is None:
            piece_cap = max(4096, 64 * len(keep["seg_time"]))
        cert = np.zeros(B, CERT_DTYPE)
        stats = np.zeros(3, np.int64)
        _chk(lib().pct_bezier_certify_batch(self._h, algo, C.byref(batch), float(margin), int(max_depth), int(piece_cap), _ptr(cert), _ptr(stats)))
        del keep
        return cert, dict(rounds=int(stats[0]), pieces=int(stats[1]), capped=int(stats[2]))

    def bezier_clearance(self, trajectories, tol, cap=float("inf"), max_depth=16, piece_cap=None, algo: int = ALGO_AUTO):
        """pct_bezier_clearance_batch: each trajectory's distance to the cloud bracketed, lo <= clearance <= hi, to within `tol` metres
        (or up to `cap`: clearance beyond it is of no interest).  trajectories and piece_cap as for bezier_certify.  Returns
        (records, stats): a structured array of engine.CLEARANCE_DTYPE, one entry per trajectory -- status (CLR_DONE, CLR_OPEN,
        CLR_INVALID), depth, at_seg, at_idx, at_u, lo, hi, pieces -- and dict(rounds, pieces, capped)."""
        packed = isinstance(trajectories, tuple) and len(trajectories) == 2 and isinstance(trajectories[0], BezierBatch)
        batch, keep = trajectories if packed else pack_trajectories(trajectories)
        B = int(batch.B)
        if piece_cap is None:
            piece_cap = max(4096, 64 * len(keep["seg_time"]))
        rec = np.zeros(B, CLEARANCE_DTYPE)
        stats = np.zeros(3, np.int64)
        _chk(lib().pct_bezier_clearance_batch(self._h, algo, C.byref(batch), float(tol), float(cap), int(max_depth), int(piece_cap), _ptr(rec), _ptr(stats)))
        del keep
        return rec, dict(rounds=int(stats[0]), pieces=int(stats[1]), capped=int(stats[2]))

    @staticmethod
    def _window_batch(trajectories, t_start, horizon):
        """(BezierBatch, arrays, horizon array or None) of a window call: t_start / horizon are None, a scalar for every trajectory or B
        values; a packed (BezierBatch, arrays) pair keeps its own t_start when t_start is None"""
        packed = isinstance(trajectories, tuple) and len(trajectories) == 2 and isinstance(trajectories[0], BezierBatch)
        if packed and t_start is None:
            batch, keep = trajectories
        else:
            rows = trajectories[1] if packed else None
            n = int(trajectories[0].B) if packed else len(trajectories)
            ts = None if t_start is None else np.broadcast_to(np.asarray(t_start, np.float64), (n,)).copy()
            if packed:
                keep = dict(rows, t_start=ts)
                b0 = trajectories[0]
                batch = BezierBatch(b0.polycoef, b0.row_stride, b0.seg_time, b0.orders, b0.seg_offsets, ts.ctypes.data, n)
            else:
                batch, keep = pack_trajectories(trajectories, ts)
        hz = None if horizon is None else np.broadcast_to(np.asarray(horizon, np.float64), (int(batch.B),)).copy()
        return batch, keep, hz

    def bezier_certify_window(self, trajectories, t_start, horizon, margin, max_depth=12, piece_cap=None, algo: int = ALGO_AUTO):
        """pct_bezier_certify_window_batch: bezier_certify for the part of each trajectory with time in [t_start, t_start + horizon] --
        "is it safe from now for the next `horizon` seconds?".  t_start, horizon: None (0 / +inf for all), one value or B values.
        hit_u is in the segment's own parameter.  Returns (certificates, stats) as bezier_certify."""
        batch, keep, hz = self._window_batch(trajectories, t_start, horizon)
        B = int(batch.B)
        if piece_cap is None:
            piece_cap = max(4096, 64 * len(keep["seg_time"]))
        cert = np.zeros(B, CERT_DTYPE)
        stats = np.zeros(3, np.int64)
        _chk(lib().pct_bezier_certify_window_batch(self._h, algo, C.byref(batch), None if hz is None else hz.ctypes.data, float(margin), int(max_depth),
                                                   int(piece_cap), _ptr(cert), _ptr(stats)))
        del keep
        return cert, dict(rounds=int(stats[0]), pieces=int(stats[1]), capped=int(stats[2]))

    def bezier_clearance_window(self, trajectories, t_start, horizon, tol, cap=float("inf"), max_depth=16, piece_cap=None, algo: int = ALGO_AUTO):
        """pct_bezier_clearance_window_batch: bezier_clearance for the window [t_start, t_start + horizon] of each trajectory; arguments
        as bezier_certify_window, at_u in the segment's own parameter.  Returns (records, stats) as bezier_clearance."""
        batch, keep, hz = self._window_batch(trajectories, t_start, horizon)
        B = int(batch.B)
        if piece_cap is None:
            piece_cap = max(4096, 64 * len(keep["seg_time"]))
        rec = np.zeros(B, CLEARANCE_DTYPE)
        stats = np.zeros(3, np.int64)
        _chk(lib().pct_bezier_clearance_window_batch(self._h, algo, C.byref(batch), None if hz is None else hz.ctypes.data, float(tol), float(cap),
                                                     int(max_depth), int(piece_cap), _ptr(rec), _ptr(stats)))
        del keep
        return rec, dict(rounds=int(stats[0]), pieces=int(stats[1]), capped=int(stats[2]))

    def ctrl_points_check(self, params: InflateParams, polycoef, seg_time, orders, t_start=0.0, cap=1024):
        """pct_ctrl_points_check: the collision threshold test on the raw control points (world units)"""
        traj, keep = _traj(polycoef, seg_time, orders)
        pos = np.zeros((cap, 3), np.float64)
        rad = np.zeros(cap, np.float64)
        d2 = np.zeros(cap, np.float64)
        idx = np.zeros(cap, np.uint32)
        fh, nc = C.c_int64(), C.c_int64()
        _chk(lib().pct_ctrl_points_check(self._h, C.byref(traj), C.byref(params), float(t_start), C.byref(fh), C.byref(nc), cap,
                                         _ptr(pos), _ptr(rad), _ptr(d2), _ptr(idx)))
        n = min(nc.value, cap)
        return dict(first_hit=fh.value, n=nc.value, pos=pos[:n], radius=rad[:n], d2=d2[:n], idx=idx[:n])

    # device-buffer variants: raw pointers (e.g. torch tensor .data_ptr()) and a hipStream_t handle
    def nn_device(self, q_ptr: int, Q: int, idx_ptr: int, d2_ptr: int, stream: int = 0, algo: int = ALGO_AUTO):
        _chk(lib().pct_nn_batch_dev(self._h, algo, q_ptr, int(Q), idx_ptr, d2_ptr, stream))

    def knn_device(self, q_ptr: int, Q: int, k: int, idx_ptr: int, d2_ptr: int, stream: int = 0, algo: int = ALGO_AUTO):
        """pct_knn_batch_dev: idx / d2 are Q x k device buffers; reserve_queries(Q) first"""
        _chk(lib().pct_knn_batch_dev(self._h, algo, q_ptr, int(Q), int(k), idx_ptr, d2_ptr, stream))

    def segment_nn_device(self, seg_ptr: int, reach_ptr: int, Q: int, idx_ptr: int, d2_ptr: int, s_ptr: int, stream: int = 0, algo: int = ALGO_AUTO):
        """pct_segment_nn_batch_dev: seg Q x 6 and reach Q doubles on the device; d2_ptr / s_ptr may be 0; reserve_queries(Q) first"""
        _chk(lib().pct_segment_nn_batch_dev(self._h, algo, seg_ptr, reach_ptr, int(Q), idx_ptr, d2_ptr or None, s_ptr or None, stream))

    def segment_sweep_device(self, seg_ptr: int, radius_ptr: int, Q: int, idx_ptr: int, t_ptr: int, stream: int = 0, algo: int = ALGO_AUTO):
        """pct_segment_sweep_batch_dev: seg Q x 6 and radius Q doubles on the device; t_ptr may be 0; reserve_queries(Q) first"""
        _chk(lib().pct_segment_sweep_batch_dev(self._h, algo, seg_ptr, radius_ptr, int(Q), idx_ptr, t_ptr or None, stream))

    def segment_count_device(self, seg_ptr: int, reach_ptr: int, Q: int, cnt_ptr: int, stream: int = 0, algo: int = ALGO_AUTO):
        """pct_segment_count_batch_dev: seg Q x 6 and reach Q doubles on the device, cnt Q uint32; reserve_queries(Q) first"""
        _chk(lib().pct_segment_count_batch_dev(self._h, algo, seg_ptr, reach_ptr, int(Q), cnt_ptr, stream))

    def segment_search_device(self, seg_ptr: int, reach_ptr: int, Q: int, order: int, offsets_ptr: int, cap: int, idx_ptr: int, d2_ptr: int,
                              s_ptr: int, stream: int = 0, algo: int = ALGO_AUTO):
        """pct_segment_search_batch_dev: offsets int64 [Q + 1] always written, idx / d2 / s (d2_ptr and s_ptr may be 0) only when
        offsets[Q] <= cap; reserve_queries(Q) first"""
        _chk(lib().pct_segment_search_batch_dev(self._h, algo, seg_ptr, reach_ptr, int(Q), int(order), offsets_ptr, int(cap), idx_ptr or None,
                                                d2_ptr or None, s_ptr or None, stream))

    def segment_supports_device(self, seg_ptr: int, Q: int, row_offsets_ptr: int, row_cap: int, row_idx_ptr: int, offsets_ptr: int, cap: int,
                                idx_ptr: int, d2_ptr: int, s_ptr: int, plane_ptr: int, stream: int = 0):
        """pct_segment_supports_dev: the supports of rows made by segment_search_device(ORDER_DISTANCE) with cap = row_cap; offsets int64
        [Q + 1] always written (all -1 when the rows did not fit row_cap), idx / d2 / s / plane (the last three may be 0) only when
        offsets[Q] <= cap; reserve_queries(Q) first"""
        _chk(lib().pct_segment_supports_dev(self._h, seg_ptr, int(Q), row_offsets_ptr, int(row_cap), row_idx_ptr or None, offsets_ptr, int(cap),
                                            idx_ptr or None, d2_ptr or None, s_ptr or None, plane_ptr or None, stream))

    def inflate_device(self, params: InflateParams, pts_ptr: int, Q: int, radius_ptr: int, idx_ptr: int = 0, d2_ptr: int = 0, stream: int = 0):
        _chk(lib().pct_inflate_batch_dev(self._h, C.byref(params), pts_ptr, int(Q), radius_ptr, idx_ptr or None, d2_ptr or None, stream))

    def bezier_check_device(self, params: InflateParams, polycoef, seg_time, orders, t_start, stop_time, dt, cap, pos_ptr, radius_ptr, d2_ptr,
                            idx_ptr, first_hit_ptr, nsamples_ptr, stream: int = 0):
        traj, keep = _traj(polycoef, seg_time, orders)
        _chk(lib().pct_bezier_check_dev(self._h, C.byref(traj), C.byref(params), float(t_start), float(stop_time), float(dt), int(cap),
                                        pos_ptr or None, radius_ptr, d2_ptr or None, idx_ptr or None, first_hit_ptr, nsamples_ptr, stream))
        return keep                                     # host arrays the stream copies from: keep them alive until it has passed

    def bezier_check_batch_device(self, params: InflateParams, batch: BezierBatch, stop_time, dt, cap, verdict_ptr: int, offsets_ptr: int,
                                  list_cap: int, pos_ptr: int = 0, radius_ptr: int = 0, d2_ptr: int = 0, idx_ptr: int = 0, stream: int = 0):
        """pct_bezier_check_batch_dev: `batch` holds DEVICE pointers; verdict_ptr -> B x 32 bytes (engine.VERDICT_DTYPE), offsets_ptr ->
        int64 [B + 1]; the lists (list_cap entries each, pos x3) may be 0; reserve_queries(list_cap) first.  Asynchronous on `stream`."""
        _chk(lib().pct_bezier_check_batch_dev(self._h, C.byref(batch), C.byref(params), float(stop_time), float(dt), int(cap), verdict_ptr or None,
                                              offsets_ptr or None, int(list_cap), pos_ptr or None, radius_ptr or None, d2_ptr or None,
                                              idx_ptr or None, stream))

    def bezier_certify_device(self, batch: BezierBatch, margin, max_depth, piece_cap, cert_ptr: int, stats_ptr: int = 0, stream: int = 0,
                              algo: int = ALGO_AUTO):
        """pct_bezier_certify_batch_dev: `batch` holds DEVICE pointers; cert_ptr -> B x 48 bytes (engine.CERT_DTYPE), stats_ptr -> int64 [3]
        or 0; reserve_queries(2 * piece_cap) first.  Asynchronous on `stream`; max_depth + 1 rounds over piece_cap slots."""
        _chk(lib().pct_bezier_certify_batch_dev(self._h, algo, C.byref(batch), float(margin), int(max_depth), int(piece_cap), cert_ptr or None,
                                                stats_ptr or None, stream))

    def bezier_clearance_device(self, batch: BezierBatch, tol, cap, max_depth, piece_cap, out_ptr: int, stats_ptr: int = 0, stream: int = 0,
                                algo: int = ALGO_AUTO):
        """pct_bezier_clearance_batch_dev: `batch` holds DEVICE pointers; out_ptr -> B x 48 bytes (engine.CLEARANCE_DTYPE), stats_ptr ->
        int64 [3] or 0; reserve_queries(2 * piece_cap) first.  Asynchronous on `stream`; max_depth + 1 rounds over piece_cap slots."""
        _chk(lib().pct_bezier_clearance_batch_dev(self._h, algo, C.byref(batch), float(tol), float(cap), int(max_depth), int(piece_cap), out_ptr or None,
                                                  stats_ptr or None, stream))

    def bezier_certify_window_device(self, batch: BezierBatch, horizon_ptr: int, margin, max_depth, piece_cap, cert_ptr: int, stats_ptr: int = 0,
                                     stream: int = 0, algo: int = ALGO_AUTO):
        """pct_bezier_certify_window_batch_dev: bezier_certify_device for the window [t_start, t_start + horizon] of each trajectory;
        batch.t_start and horizon_ptr are DEVICE arrays of B doubles or 0 (0.0 / +inf for all)."""
        _chk(lib().pct_bezier_certify_window_batch_dev(self._h, algo, C.byref(batch), horizon_ptr or None, float(margin), int(max_depth), int(piece_cap),
                                                       cert_ptr or None, stats_ptr or None, stream))

    def bezier_clearance_window_device(self, batch: BezierBatch, horizon_ptr: int, tol, cap, max_depth, piece_cap, out_ptr: int, stats_ptr: int = 0,
                                       stream: int = 0, algo: int = ALGO_AUTO):
        """pct_bezier_clearance_window_batch_dev: bezier_clearance_device for the window of each trajectory; batch.t_start and
        horizon_ptr as for bezier_certify_window_device."""
        _chk(lib().pct_bezier_clearance_window_batch_dev(self._h, algo, C.byref(batch), horizon_ptr or None, float(tol), float(cap), int(max_depth),
                                                         int(piece_cap), out_ptr or None, stats_ptr or None, stream))

    def radius_count_device(self, q_ptr: int, r_ptr: int, Q: int, cnt_ptr: int, stream: int = 0, algo: int = ALGO_AUTO):
        _chk(lib().pct_radius_count_batch_dev(self._h, algo, q_ptr, r_ptr, int(Q), cnt_ptr, stream))

    def radius_search_device(self, q_ptr: int, r_ptr: int, Q: int, order: int, offsets_ptr: int, cap: int, idx_ptr: int, d2_ptr: int,
                             stream: int = 0, algo: int = ALGO_AUTO):
        """pct_radius_search_batch_dev: offsets int64 [Q + 1] always written, idx / d2 (d2_ptr may be 0) only when offsets[Q] <= cap;
        reserve_queries(Q) first"""
        _chk(lib().pct_radius_search_batch_dev(self._h, algo, q_ptr, r_ptr, int(Q), int(order), offsets_ptr, int(cap), idx_ptr or None,
                                               d2_ptr or None, stream))

    def set_timing(self, level: int):
        """0 = no events, 1 = dominant kernel only (default), 2 = + whole batch (needed by last_batch_ms)"""
        _chk(lib().pct_set_timing(self._h, int(level)))

    def debug_read_grid(self):
        """(cell_start uint32 [ncells + 1], records float32 [n, 4]) as built -- test hook"""
        cs = np.empty(self.grid_info()["ncells"] + 1, np.uint32)
        rec = np.empty((len(self), 4), np.float32)
        _chk(lib().pct_debug_read_grid(self._h, cs.ctypes.data, rec.ctypes.data))
        return cs, rec

    def set_timing_stride(self, stride: int):
        """the index path times only every stride-th launch from now on (pct_set_timing_stride)"""
        _chk(lib().pct_set_timing_stride(self._h, int(stride)))

    def kernel_ms_samples(self) -> int:
        n = C.c_uint64()
        _chk(lib().pct_kernel_ms_samples(self._h, C.byref(n)))
        return int(n.value)

    def kernel_ms_history(self, n: int = 64):
        """dominant-kernel durations (ms) of the last <= n batches, oldest first (HIP events on the launch stream)"""
        buf = (C.c_float * max(n, 1))()
        got = C.c_int()
        _chk(lib().pct_kernel_ms_history(self._h, buf, int(n), C.byref(got)))
        return [buf[i] for i in range(got.value)]

    def last_kernel_ms(self) -> float:
        ms = C.c_float()
        _chk(lib().pct_last_kernel_ms(self._h, C.byref(ms)))
        return ms.value

    def last_batch_ms(self) -> float:
        ms = C.c_float()
        _chk(lib().pct_last_batch_ms(self._h, C.byref(ms)))
        return ms.value

    def set_work_counters(self, on: bool):
        _chk(lib().pct_set_work_counters(self._h, int(bool(on))))

    def last_work(self):
        a, b = C.c_uint64(), C.c_uint64()
        _chk(lib().pct_last_work(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def last_work_ex(self):
        """(points scanned, cell runs scanned, pyramid node visits) of the last instrumented batch"""
        out = (C.c_uint64 * 3)()
        _chk(lib().pct_last_work_ex(self._h, out))
        return int(out[0]), int(out[1]), int(out[2])

    def verify_grid(self):
        """device-side structural check of the built index (pct_debug_verify_grid): dict of fault counts; sound = all zero and
        cell_start running from 0 to n"""
        out = (C.c_uint64 * 6)()
        _chk(lib().pct_debug_verify_grid(self._h, out))
        return dict(bad_ids=int(out[0]), duplicates=int(out[1]), misplaced=int(out[2]), decreasing=int(out[3]), first=int(out[4]), last=int(out[5]))

    def pyramid_info(self):
        lv, nodes, ef = C.c_int32(), C.c_int64(), C.c_double()
        _chk(lib().pct_cloud_pyramid_info(self._h, C.byref(lv), C.byref(nodes), C.byref(ef)))
        return dict(levels=lv.value, nodes=nodes.value, empty_fraction=ef.value)


def _traj(polycoef, seg_time, orders):
    coef = np.ascontiguousarray(polycoef, np.float64)
    st = np.ascontiguousarray(seg_time, np.float64)
    od = np.ascontiguousarray(orders, np.int32)
    t = BezierTraj(coef.ctypes.data_as(C.POINTER(C.c_double)), coef.shape[1], st.ctypes.data_as(C.POINTER(C.c_double)),
                   od.ctypes.data_as(C.POINTER(C.c_int32)), len(st))
    return t, (coef, st, od)


class ReplanPlan:
    """hipGraph-captured query side of one replan tick (pct_plan_create_replan): corridor-node inflation + sampled Bezier
    check + control-point check in one launch."""

    def __init__(self, cloud: Cloud, max_nodes: int, max_samples: int, max_segments: int):
        self._h = C.c_void_p()
        self._cloud = cloud
        self.max_nodes, self.max_samples, self.max_segments = int(max_nodes), int(max_samples), int(max_segments)
        _chk(lib().pct_plan_create_replan(cloud.handle, self.max_nodes, self.max_samples, self.max_segments, C.byref(self._h)))
        nc = 13 * self.max_segments
        self._b = dict(node_radius=np.zeros(self.max_nodes), node_idx=np.zeros(self.max_nodes, np.uint32), node_d2=np.zeros(self.max_nodes),
                       sample_pos=np.zeros((self.max_samples, 3)), sample_radius=np.zeros(self.max_samples), sample_d2=np.zeros(self.max_samples),
                       sample_idx=np.zeros(self.max_samples, np.uint32), ctrl_pos=np.zeros((nc, 3)), ctrl_radius=np.zeros(nc), ctrl_d2=np.zeros(nc),
                       ctrl_idx=np.zeros(nc, np.uint32))
        self._o = ReplanOut()
        for k, v in self._b.items():
            setattr(self._o, k, v.ctypes.data)

    def run(self, params: InflateParams, nodes, polycoef=None, seg_time=None, orders=None, t_start=0.0, stop_time=2.0, dt=0.02, want_nn=True,
            copy=True):
        nd = np.ascontiguousarray(nodes, np.float64).reshape(-1, 3)
        traj, keep = (None, None) if polycoef is None else _traj(polycoef, seg_time, orders)
        _chk(lib().pct_plan_replan_run(self._h, C.byref(params), _ptr(nd), len(nd), None if traj is None else C.byref(traj), float(t_start),
                                       float(stop_time), float(dt), int(bool(want_nn)), C.byref(self._o)))
        o, b = self._o, self._b
        ns, nc = min(o.nsamples, self.max_samples), o.nctrl
        cp = (lambda a: a.copy()) if copy else (lambda a: a)
        return dict(node_radius=cp(b["node_radius"][:len(nd)]), node_idx=cp(b["node_idx"][:len(nd)]), node_d2=cp(b["node_d2"][:len(nd)]),
                    nsamples=o.nsamples, first_hit_sample=o.first_hit_sample, sample_pos=cp(b["sample_pos"][:ns]),
                    sample_radius=cp(b["sample_radius"][:ns]), sample_d2=cp(b["sample_d2"][:ns]), sample_idx=cp(b["sample_idx"][:ns]),
                    nctrl=nc, first_hit_ctrl=o.first_hit_ctrl, ctrl_pos=cp(b["ctrl_pos"][:nc]), ctrl_radius=cp(b["ctrl_radius"][:nc]),
                    ctrl_d2=cp(b["ctrl_d2"][:nc]), ctrl_idx=cp(b["ctrl_idx"][:nc]))

    def last_run_us(self):
        """host wall time of the last run inside the library: (fill, graph launch, wait, read-out) in microseconds"""
        us = (C.c_double * 4)()
        _chk(lib().pct_plan_last_run_us(self._h, us))
        return tuple(us)

    def close(self):
        if getattr(self, "_h", None) and self._h.value and _lib is not None:
            _lib.pct_plan_destroy(self._h)
            self._h = C.c_void_p()

    __del__ = close


class NNPlan:
    """hipGraph-captured fixed-shape NN batch (config C5)."""

    def __init__(self, cloud: Cloud, Q: int, algo: int = ALGO_AUTO):
        self._h = C.c_void_p()
        self.Q = int(Q)
        self._cloud = cloud
        _chk(lib().pct_plan_create_nn(cloud.handle, algo, self.Q, C.byref(self._h)))

    def run(self, queries):
        q = np.ascontiguousarray(queries, np.float32).reshape(self.Q, 3)
        idx = np.empty(self.Q, np.uint32)
        d2 = np.empty(self.Q, np.float64)
        _chk(lib().pct_plan_run(self._h, _ptr(q), _ptr(idx), _ptr(d2)))
        return idx, d2

    def close(self):
        if getattr(self, "_h", None) and self._h.value and _lib is not None:      # _lib is None during interpreter shutdown
            _lib.pct_plan_destroy(self._h)
            self._h = C.c_void_p()

    __del__ = close
