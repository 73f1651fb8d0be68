"""Capsule search (pct_segment_search_batch_dev) on an indexed cloud: the indexed form against PCT_ALGO_STREAM of the same feature, one
JSON line per form and reach and one that compares them.

Clouds: --cloud c5-uniform / c5-clustered: the 5 M-point C5 window (scenarios.c5_frame / c5_frame_clustered, fed in 50 k-point
frames, a few frames beyond full so the ring has wrapped), PCT_ALGO_RING against PCT_ALGO_STREAM; --cloud c3-grid: config C3's
10 M uniform points in [0, 100)^3 (seed 3) under the default cell index, PCT_ALGO_GRID against PCT_ALGO_STREAM.
Workload: --segments segments of --length m in random directions (around the drone on the window, anywhere inside the box on the grid
cloud), every reach of --reach.  Timing: pct_last_batch_ms (HIP events around every kernel of the batch -- count, scan, fill, sort and
the s pass -- timing level 2), median of --batches calls after two warm-up calls, the two forms taking turns call by call; work counters
from one extra instrumented call of each; the two forms' lists are compared."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from pointcloudtraj_amd import engine as E, scenarios as S, synth


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cloud", choices=["c5-uniform", "c5-clustered", "c3-grid"], default="c5-uniform")
    ap.add_argument("--window", type=int, default=S.C5_WINDOW)
    ap.add_argument("--frame", type=int, default=S.C5_FRAME)
    ap.add_argument("--points", type=int, default=10_000_000, help="points of the c3-grid cloud")
    ap.add_argument("--segments", type=int, default=256)
    ap.add_argument("--length", type=float, default=3.0)
    ap.add_argument("--reach", type=float, nargs="+", default=[1.75, 0.5])
    ap.add_argument("--batches", type=int, default=20)
    a = ap.parse_args()
    E.init(0)
    dev = torch.device("cuda:0")
    cs = torch.cuda.current_stream().cuda_stream
    Q = a.segments
    d = synth.uniform_points(6, Q, -1.0, 1.0).astype(np.float64)
    d /= np.maximum(np.linalg.norm(d, axis=1), 1e-9)[:, None]
    if a.cloud == "c3-grid":
        c = E.Cloud(a.points)
        for o, blk in synth.uniform_points_chunked(3, a.points, 0.0, 100.0):
            c.set_input(blk) if o == 0 else c.append(blk)
        c.build_grid()
        g = c.grid_info()
        info = dict(cloud=a.cloud, points=len(c), grid_dims=g["dims"], cell_size=g["cell_size"])
        start = synth.uniform_points(5, Q, 10.0, 90.0).astype(np.float64)
        indexed = ("PCT_ALGO_GRID", E.ALGO_GRID)
    else:
        make = S.c5_frame_clustered if a.cloud == "c5-clustered" else S.c5_frame
        c = E.Cloud(a.window)
        c.ring_index()
        nframes = a.window // a.frame + 12
        for k in range(nframes):
            c.append(make(k, a.frame))
        ring = c.ring_info()
        info = dict(cloud=a.cloud, points=len(c), ring_dims=ring["dims"], cell_size=ring["cell_size"], overflow_entries=ring["overflow_entries"],
                    bucket_records=ring["bucket_records"])
        start = synth.uniform_points(5, Q, -1.0, 1.0).astype(np.float64) * [25.0, 25.0, 3.0] + [0.1 * (nframes - 1), 0.0, 3.0]
        indexed = ("PCT_ALGO_RING", E.ALGO_RING)
    segs = np.concatenate([start, start + a.length * d], axis=1)
    tseg = torch.from_numpy(segs).to(dev)
    c.reserve_queries(Q)
    c.set_timing(2)
    info.update(segments=Q, length=a.length, batches=a.batches)
    forms = (indexed, ("PCT_ALGO_STREAM", E.ALGO_STREAM))
    for reach in a.reach:
        treach = torch.full((Q,), reach, dtype=torch.float64, device=dev)
        tcnt = torch.zeros(Q, dtype=torch.int32, device=dev)
        c.segment_count_device(tseg.data_ptr(), treach.data_ptr(), Q, tcnt.data_ptr(), cs, E.ALGO_STREAM)
        total = int(tcnt.cpu().numpy().view(np.uint32).astype(np.int64).sum())
        cap = max(total, 1)
        out = {name: (torch.empty(Q + 1, dtype=torch.int64, device=dev), torch.empty(cap, dtype=torch.int32, device=dev),
                      torch.empty(cap, dtype=torch.float64, device=dev), torch.empty(cap, dtype=torch.float64, device=dev)) for name, _ in forms}

        def run(name, algo):
            to, ti, td, ts = out[name]
            c.segment_search_device(tseg.data_ptr(), treach.data_ptr(), Q, E.ORDER_DISTANCE, to.data_ptr(), cap, ti.data_ptr(), td.data_ptr(), ts.data_ptr(),
                                    cs, algo)

        for name, algo in forms * 2:
            run(name, algo)
        torch.cuda.synchronize()
        ms = {name: [] for name, _ in forms}
        for _ in range(a.batches):
            for name, algo in forms:                       # the forms take turns
                run(name, algo)
                ms[name].append(c.last_batch_ms())
        work = {}
        c.set_work_counters(True)
        for name, algo in forms:
            run(name, algo)
            torch.cuda.synchronize()
            work[name] = c.last_work()
        c.set_work_counters(False)
        rows = {name: tuple(t.cpu().numpy().copy() for t in out[name]) for name, _ in forms}
        med = {name: statistics.median(v) for name, v in ms.items()}
        for name, _ in forms:
            print(json.dumps(dict(info, call="pct_segment_search_batch_dev", reach=reach, algo=name, batch_ms_median=med[name], batch_ms_min=min(ms[name]),
                                  batch_ms_max=max(ms[name]), records_per_segment=work[name][0] / Q, cells_per_segment=work[name][1] / Q,
                                  total_hits=int(rows[name][0][Q]))), flush=True)
        n = int(rows[forms[0][0]][0][Q])
        same = np.array_equal(rows[forms[0][0]][0], rows[forms[1][0]][0]) and all(np.array_equal(x[:n], y[:n]) for x, y in zip(rows[forms[0][0]][1:], rows[forms[1][0]][1:]))
        print(json.dumps(dict(info, call="pct_segment_search_batch_dev", reach=reach, stream_over_indexed=med[forms[1][0]] / med[forms[0][0]],
                              total_hits=total, answers_equal=bool(same))), flush=True)
    c.close()


if __name__ == "__main__":
    main()
