"""Segment sweeps (pct_segment_sweep_batch_dev) on config C5's rolling map: the rolling-map form against the streaming form and against
the nearest search of the same capsules (pct_segment_nn_batch_dev, PCT_ALGO_RING, reach = the sweep's radius), one JSON line per call
and one that compares them.

Workload: the 5 M-point C5 window of scripts/probe_segments.py (scenarios.c5_frame, fed in 50 k-point frames, a few frames beyond
full so the ring has wrapped), --segments segments of --length m in random directions around the drone, radius --radius.  Timing:
pct_last_batch_ms (HIP events around every kernel of the batch, timing level 2), median of --batches calls after two warm-up calls,
the three calls taking turns inside every repetition; work counters from one extra instrumented call each; the two sweep forms'
answers are compared, and the sweep's blocked set with the nearest search's found set."""
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
    ap.add_argument("--radius", type=float, default=0.25)
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
    tseg = torch.from_numpy(segs).to(dev)
    trad = torch.full((Q,), a.radius, dtype=torch.float64, device=dev)
    c.reserve_queries(Q)
    c.set_timing(2)
    ring = c.ring_info()
    info = dict(cloud="c5-clustered" if a.clustered else "c5-uniform", points=len(c), segments=Q, length=a.length, radius=a.radius, ring_dims=ring["dims"],
                cell_size=ring["cell_size"], overflow_entries=ring["overflow_entries"], bucket_records=ring["bucket_records"], batches=a.batches)
    ti = {k: torch.empty(Q, dtype=torch.int32, device=dev) for k in ("sweep_ring", "sweep_stream", "nearest_ring")}
    tv = {k: torch.empty(Q, dtype=torch.float64, device=dev) for k in ti}
    ts = torch.empty(Q, dtype=torch.float64, device=dev)
    calls = {
        "sweep_ring": lambda: c.segment_sweep_device(tseg.data_ptr(), trad.data_ptr(), Q, ti["sweep_ring"].data_ptr(), tv["sweep_ring"].data_ptr(), cs, E.ALGO_RING),
        "sweep_stream": lambda: c.segment_sweep_device(tseg.data_ptr(), trad.data_ptr(), Q, ti["sweep_stream"].data_ptr(), tv["sweep_stream"].data_ptr(), cs,
                                                       E.ALGO_STREAM),
        "nearest_ring": lambda: c.segment_nn_device(tseg.data_ptr(), trad.data_ptr(), Q, ti["nearest_ring"].data_ptr(), tv["nearest_ring"].data_ptr(),
                                                    ts.data_ptr(), cs, E.ALGO_RING),
    }
    names = {"sweep_ring": ("pct_segment_sweep_batch_dev", "PCT_ALGO_RING"), "sweep_stream": ("pct_segment_sweep_batch_dev", "PCT_ALGO_STREAM"),
             "nearest_ring": ("pct_segment_nn_batch_dev", "PCT_ALGO_RING")}
    for run in calls.values():
        run(); run()
    torch.cuda.synchronize()
    ms = {k: [] for k in calls}
    for _ in range(a.batches):
        for k, run in calls.items():
            run()
            ms[k].append(c.last_batch_ms())
    work, rows = {}, {}
    c.set_work_counters(True)
    for k, run in calls.items():
        run()
        torch.cuda.synchronize()
        work[k] = c.last_work()
        rows[k] = (ti[k].cpu().numpy().view(np.uint32).copy(), tv[k].cpu().numpy().copy())
    c.set_work_counters(False)
    med = {k: statistics.median(v) for k, v in ms.items()}
    for k in calls:
        t = rows[k][1]
        extra = dict(stopped_on_the_way=int(((t > 0) & (t < 1)).sum()), in_contact_at_start=int((t == 0).sum())) if k != "nearest_ring" else {}
        print(json.dumps(dict(info, call=names[k][0], algo=names[k][1], batch_ms_median=med[k], batch_ms_min=min(ms[k]), batch_ms_max=max(ms[k]),
                              records_per_segment=work[k][0] / Q, buckets_per_segment=work[k][1] / Q,
                              found=int((rows[k][0] != 0xFFFFFFFF).sum()), **extra)), flush=True)
    same = all(np.array_equal(x, y, equal_nan=True) for x, y in zip(rows["sweep_ring"], rows["sweep_stream"]))
    blocked_is_found = bool(np.array_equal(rows["sweep_ring"][0] != 0xFFFFFFFF, rows["nearest_ring"][0] != 0xFFFFFFFF))
    print(json.dumps(dict(info, sweep_stream_over_ring=med["sweep_stream"] / med["sweep_ring"], sweep_ring_over_nearest_ring=med["sweep_ring"] / med["nearest_ring"],
                          records_sweep_over_nearest=work["sweep_ring"][0] / max(1, work["nearest_ring"][0]), answers_equal=bool(same),
                          blocked_is_found=blocked_is_found)), flush=True)
    c.close()


if __name__ == "__main__":
    main()
