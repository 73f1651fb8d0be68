"""Segment queries (pct_segment_nn_batch_dev) on config C5's rolling map: PCT_ALGO_RING against PCT_ALGO_STREAM of the same feature,
one JSON line per form and one that compares them.

Workload: the 5 M-point C5 window (scenarios.c5_frame, fed in 50 k-point frames, a few frames beyond full so the ring has wrapped),
--segments segments of --length m in random directions around the drone (the slab a replan tick asks about), reach = max_radius +
search_margin of C5_PARAMS.  Timing: pct_last_batch_ms (HIP events around every kernel of the batch, timing level 2), median of
--batches calls after two warm-up calls; work counters from one extra instrumented call; the two forms' answers are compared."""
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
    ap.add_argument("--window", type=int, default=S.C5_WINDOW)
    ap.add_argument("--frame", type=int, default=S.C5_FRAME)
    ap.add_argument("--segments", type=int, default=256)
    ap.add_argument("--length", type=float, default=3.0)
    ap.add_argument("--batches", type=int, default=20)
    ap.add_argument("--clustered", action="store_true", help="the pillar-surface variant of the window")
    a = ap.parse_args()
    E.init(0)
    dev = torch.device("cuda:0")
    cs = torch.cuda.current_stream().cuda_stream
    make = S.c5_frame_clustered if a.clustered else S.c5_frame
    c = E.Cloud(a.window)
    c.ring_index()
    nframes = a.window // a.frame + 12
    for k in range(nframes):
        c.append(make(k, a.frame))
    x0 = 0.1 * (nframes - 1)
    Q = a.segments
    start = synth.uniform_points(5, Q, -1.0, 1.0).astype(np.float64) * [25.0, 25.0, 3.0] + [x0, 0.0, 3.0]
    d = synth.uniform_points(6, Q, -1.0, 1.0).astype(np.float64)
    d /= np.maximum(np.linalg.norm(d, axis=1), 1e-9)[:, None]
    segs = np.concatenate([start, start + a.length * d], axis=1)
    reach = S.C5_PARAMS["max_radius"] + S.C5_PARAMS["search_margin"]
    tseg = torch.from_numpy(segs).to(dev)
    treach = torch.full((Q,), reach, dtype=torch.float64, device=dev)
    c.reserve_queries(Q)
    c.set_timing(2)
    ring = c.ring_info()
    info = dict(cloud="c5-clustered" if a.clustered else "c5-uniform", points=len(c), segments=Q, length=a.length, reach=reach, ring_dims=ring["dims"],
                cell_size=ring["cell_size"], overflow_entries=ring["overflow_entries"], bucket_records=ring["bucket_records"], batches=a.batches)
    rows, times = {}, {}
    for name, algo in (("PCT_ALGO_RING", E.ALGO_RING), ("PCT_ALGO_STREAM", E.ALGO_STREAM)):
        ti = torch.empty(Q, dtype=torch.int32, device=dev)
        td = torch.empty(Q, dtype=torch.float64, device=dev)
        ts = torch.empty(Q, dtype=torch.float64, device=dev)
        run = lambda: c.segment_nn_device(tseg.data_ptr(), treach.data_ptr(), Q, ti.data_ptr(), td.data_ptr(), ts.data_ptr(), cs, algo)
        run(); run()
        torch.cuda.synchronize()
        ms = []
        for _ in range(a.batches):
            run()
            ms.append(c.last_batch_ms())
        c.set_work_counters(True)
        run()
        torch.cuda.synchronize()
        points, buckets = c.last_work()
        c.set_work_counters(False)
        rows[name] = (ti.cpu().numpy().copy(), td.cpu().numpy().copy(), ts.cpu().numpy().copy())
        times[name] = statistics.median(ms)
        print(json.dumps(dict(info, call="pct_segment_nn_batch_dev", algo=name, batch_ms_median=times[name], batch_ms_min=min(ms), batch_ms_max=max(ms),
                              records_per_segment=points / Q, buckets_per_segment=buckets / Q,
                              found=int((rows[name][0].view(np.uint32) != 0xFFFFFFFF).sum()))), flush=True)
    same = all(np.array_equal(x, y, equal_nan=True) for x, y in zip(rows["PCT_ALGO_RING"], rows["PCT_ALGO_STREAM"]))
    print(json.dumps(dict(info, call="pct_segment_nn_batch_dev", stream_over_ring=times["PCT_ALGO_STREAM"] / times["PCT_ALGO_RING"], answers_equal=bool(same))),
          flush=True)
    c.close()


if __name__ == "__main__":
    main()
