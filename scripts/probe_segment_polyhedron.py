"""Free-space polyhedra (pct_segment_polyhedron_batch) beside the capsule search they follow, one JSON line per reach.

Clouds: --cloud c5-uniform / c5-clustered: the 5 M-point C5 window (scenarios.c5_frame / c5_frame_clustered, fed in 50 k-point
frames, a few frames beyond full so the ring has wrapped), the rolling-map index; --cloud c3-grid: config C3's 10 M uniform points in
[0, 100)^3 (seed 3) under the default cell index.
Workload: --segments segments of --length m in random directions (around the drone on the window, anywhere inside the box on the grid
cloud), every reach of --reach, PCT_ALGO_AUTO.
Timing, device events on the caller's stream, median of --batches calls after two warm-up calls, the three taking turns call by call:
  search     pct_segment_search_batch_dev in PCT_ORDER_DISTANCE (idx only: the sort keys in the cloud's buffer) -- the pipeline's own
             lower bound;
  pipeline   the same search followed by pct_segment_supports_dev (filter, count, scan, compaction);
  filter     pct_segment_supports_dev alone over the rows of the last search.
The host form (pct_segment_polyhedron_batch + _read, wall clock around the call, which ends in a wait) and the host-form capsule search
are timed the same way.  The device pipeline's lists are compared with the host form's, and the rows' and supports' lengths reported."""
import argparse
import json
import os
import statistics
import sys
import time

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
    else:
        make = S.c5_frame_clustered if a.cloud == "c5-clustered" else S.c5_frame
        c = E.Cloud(a.window)
        c.ring_index()
        nframes = a.window // a.frame + 12
        for k in range(nframes):
            c.append(make(k, a.frame))
        ring = c.ring_info()
        info = dict(cloud=a.cloud, points=len(c), ring_dims=ring["dims"], cell_size=ring["cell_size"])
        start = synth.uniform_points(5, Q, -1.0, 1.0).astype(np.float64) * [25.0, 25.0, 3.0] + [0.1 * (nframes - 1), 0.0, 3.0]
    segs = np.concatenate([start, start + a.length * d], axis=1)
    tseg = torch.from_numpy(segs).to(dev)
    c.reserve_queries(Q)
    info.update(segments=Q, length=a.length, batches=a.batches, lds_rows=E.polyhedron_lds_rows())
    for reach in a.reach:
        treach = torch.full((Q,), reach, dtype=torch.float64, device=dev)
        want = c.segment_polyhedron(segs, reach)                                   # the host form: also the sizes
        rows = c.segment_count(segs, reach)
        row_cap, cap = max(int(rows.astype(np.int64).sum()), 1), max(int(want[0][-1]), 1)
        troff = torch.empty(Q + 1, dtype=torch.int64, device=dev)
        tridx = torch.empty(row_cap, dtype=torch.int32, device=dev)
        toff = torch.empty(Q + 1, dtype=torch.int64, device=dev)
        tidx = torch.empty(cap, dtype=torch.int32, device=dev)
        td2, ts = torch.empty(cap, dtype=torch.float64, device=dev), torch.empty(cap, dtype=torch.float64, device=dev)
        tpl = torch.empty((cap, 4), dtype=torch.float64, device=dev)

        def search():
            c.segment_search_device(tseg.data_ptr(), treach.data_ptr(), Q, E.ORDER_DISTANCE, troff.data_ptr(), row_cap, tridx.data_ptr(), 0, 0, cs)

        def supports():
            c.segment_supports_device(tseg.data_ptr(), Q, troff.data_ptr(), row_cap, tridx.data_ptr(), toff.data_ptr(), cap, tidx.data_ptr(),
                                      td2.data_ptr(), ts.data_ptr(), tpl.data_ptr(), cs)

        def pipeline():
            search()
            supports()

        def on_device(f):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f()
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1)

        def on_host(f):
            t0 = time.perf_counter()
            f()                                                                    # ends in a wait
            return 1e3 * (time.perf_counter() - t0)

        calls = dict(search=lambda: on_device(search), pipeline=lambda: on_device(pipeline), filter=lambda: on_device(supports),
                     host_polyhedron=lambda: on_host(lambda: c.segment_polyhedron(segs, reach)),
                     host_search=lambda: on_host(lambda: c.segment_search(segs, reach, E.ORDER_DISTANCE)))
        for _ in range(2):
            for f in calls.values():
                f()
        ms = {k: [] for k in calls}
        for _ in range(a.batches):
            for k, f in calls.items():                                             # the calls take turns
                ms[k].append(f())
        torch.cuda.synchronize()
        n = int(want[0][-1])
        got = (toff.cpu().numpy(), tidx.cpu().numpy().view(np.uint32)[:n], td2.cpu().numpy()[:n], ts.cpu().numpy()[:n], tpl.cpu().numpy()[:n])
        same = all(np.array_equal(x, y) for x, y in zip(got, want))
        nsup = np.diff(want[0])
        line = dict(info, call="pct_segment_polyhedron_batch", reach=reach, answers_equal=bool(same),
                    candidates_mean=float(rows.mean()), candidates_max=int(rows.max()), supports_mean=float(nsup.mean()), supports_max=int(nsup.max()))
        for k, v in ms.items():
            line[k + "_ms_median"] = statistics.median(v)
            line[k + "_ms_min"] = min(v)
            line[k + "_ms_max"] = max(v)
        print(json.dumps(line), flush=True)
    c.close()


if __name__ == "__main__":
    main()
