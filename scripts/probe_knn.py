"""k-NN batches (pct_knn_batch_dev) against the 1-NN batch on the same cloud and queries: one JSON line per configuration.

Clouds: config C3's (10 M uniform points in [0,100)^3, seed 3, cell index built) and the 10 M-point clustered pillar-surface cloud.
Batch: 1 048 576 uniform queries over the cloud's bounding box (seed 5), resident on the device.  Per k in 1, 4, 8, 16, 32, 64 the
cell-pruned kernel's median duration over the timed batches (HIP events around the kernel, pct_kernel_ms_history), queries/s, and the
points and cell runs examined per query (work counters, one extra instrumented batch).  Yardstick: pct_nn_batch_dev in the same run.
--stream-queries N > 0 also times the streaming kernel on N of the queries (pairs/s = N * points / kernel time; its events span the
stream kernel and the merge of its partial lists).

--rolling-map: config C5 instead -- the 5 M-point rolling window fed in 50 k-point frames (uniform and clustered variants), the
rolling-map index live, a tick batch of --tick-queries queries with k = --k.  Per variant one line for PCT_ALGO_RING (what
PCT_ALGO_AUTO takes there) and one for PCT_ALGO_STREAM on the same cloud in the same run: median of --batches whole calls between
two events on the stream, records examined per query, overflow-queue length and records per bucket; the rows of the two are compared.
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from pointcloudtraj_amd import engine as E, scenarios as S, synth

KS = (1, 4, 8, 16, 32, 64)


def timed(c, run, batches):
    run()                                                   # warm-up: code object load, workspaces
    torch.cuda.synchronize()
    for _ in range(batches):
        run()
    torch.cuda.synchronize()
    ms = c.kernel_ms_history(batches)[-batches:]
    return statistics.median(ms), min(ms), max(ms)


def rolling_window(a, clustered):
    """config C5's rolling map: a window of --window points fed in frames of --frame, a few frames beyond full so that the ring has
    wrapped (and, in the clustered variant, the buckets have grown); returns the cloud and the drone's x"""
    make = S.c5_frame_clustered if clustered else S.c5_frame
    c = E.Cloud(a.window)
    c.ring_index()
    nframes = a.window // a.frame + 12
    for k in range(nframes):
        c.append(make(k, a.frame))
    return c, 0.1 * (nframes - 1)


def tick_queries(seed, Q, x0):
    """a replan tick's batch: points of the 50 m x 50 m x 6 m slab around the drone"""
    return (synth.uniform_points(seed, Q, -1.0, 1.0).astype(np.float64) * [25.0, 25.0, 3.0] + [x0, 0.0, 3.0]).astype(np.float32)


def event_timed(run, batches):
    """median / min / max ms of the whole call between two events on the stream, after two warm-up calls"""
    run(); run()
    torch.cuda.synchronize()
    ms = []
    for _ in range(batches):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        run()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return statistics.median(ms), min(ms), max(ms)


def rolling_map(a):
    dev = torch.device("cuda:0")
    cs = torch.cuda.current_stream().cuda_stream
    Q, k = a.tick_queries, a.k
    for clustered in (False, True):
        c, x0 = rolling_window(a, clustered)
        tq = torch.from_numpy(tick_queries(5, Q, x0)).to(dev)
        c.reserve_queries(Q)
        ring = c.ring_info()
        info = dict(cloud="c5-clustered" if clustered else "c5-uniform", points=len(c), queries=Q, k=k, ring_dims=ring["dims"], cell_size=ring["cell_size"],
                    overflow_entries=ring["overflow_entries"], bucket_records=ring["bucket_records"], batches=a.batches)
        rows, times = {}, {}
        for name, algo in (("PCT_ALGO_RING", E.ALGO_RING), ("PCT_ALGO_STREAM", E.ALGO_STREAM)):
            ki = torch.empty((Q, k), dtype=torch.int32, device=dev)
            kd = torch.empty((Q, k), dtype=torch.float64, device=dev)
            run = lambda: c.knn_device(tq.data_ptr(), Q, k, ki.data_ptr(), kd.data_ptr(), cs, algo)
            ms, lo_ms, hi_ms = event_timed(run, a.batches)
            c.set_work_counters(True)
            run()
            torch.cuda.synchronize()
            points, buckets = c.last_work()
            c.set_work_counters(False)
            rows[name], times[name] = (ki.cpu().numpy().copy(), kd.cpu().numpy().copy()), ms
            print(json.dumps(dict(info, call="pct_knn_batch_dev", algo=name, ms_median=ms, ms_min=lo_ms, ms_max=hi_ms,
                                  records_per_query=points / Q, buckets_per_query=buckets / Q)), flush=True)
        same = all(np.array_equal(x, y) for x, y in zip(rows["PCT_ALGO_RING"], rows["PCT_ALGO_STREAM"]))
        print(json.dumps(dict(info, call="pct_knn_batch_dev", stream_over_ring=times["PCT_ALGO_STREAM"] / times["PCT_ALGO_RING"], rows_equal=bool(same))), flush=True)
        c.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=10_000_000)
    ap.add_argument("--queries", type=int, default=1 << 20)
    ap.add_argument("--batches", type=int, default=7)
    ap.add_argument("--stream-queries", type=int, default=0)
    ap.add_argument("--clouds", default="uniform,clustered")
    ap.add_argument("--rolling-map", action="store_true", help="config C5's rolling window instead: PCT_ALGO_RING against PCT_ALGO_STREAM")
    ap.add_argument("--window", type=int, default=S.C5_WINDOW)
    ap.add_argument("--frame", type=int, default=S.C5_FRAME)
    ap.add_argument("--tick-queries", type=int, default=256)
    ap.add_argument("--k", type=int, default=8)
    a = ap.parse_args()
    E.init(0)
    if a.rolling_map:
        a.batches = max(a.batches, 20)
        return rolling_map(a)
    dev = torch.device("cuda:0")
    Q = a.queries
    for name in a.clouds.split(","):
        if name == "uniform":
            pts = synth.uniform_points(3, a.points, 0.0, 100.0)
        else:
            pts = synth.pillar_map_scaled(7.4 * (a.points / 10_000_000) ** 0.5)
        lo, hi = pts.min(0), pts.max(0)
        q = (lo + synth.uniform01_f32(5, 3 * Q).reshape(Q, 3) * (hi - lo)).astype(np.float32)
        tq = torch.from_numpy(q).to(dev)
        cs = torch.cuda.current_stream().cuda_stream
        with E.Cloud(len(pts)) as c:
            c.set_input(pts)
            c.build_grid()
            c.reserve_queries(Q)
            info = dict(cloud=name, points=len(pts), queries=Q, grid=c.grid_info()["dims"], pyramid_levels=c.pyramid_info()["levels"])
            oi = torch.empty(Q, dtype=torch.int32, device=dev)
            od = torch.empty(Q, dtype=torch.float64, device=dev)
            nn_ms, nn_lo, nn_hi = timed(c, lambda: c.nn_device(tq.data_ptr(), Q, oi.data_ptr(), od.data_ptr(), cs, E.ALGO_GRID), a.batches)
            print(json.dumps(dict(info, kernel="pct_nn_batch_dev", kernel_ms_median=nn_ms, kernel_ms_min=nn_lo, kernel_ms_max=nn_hi,
                                  queries_per_s=Q / nn_ms * 1e3)), flush=True)
            nn_idx, nn_d2 = oi.cpu().numpy().view(np.uint32), od.cpu().numpy()
            for k in KS:
                ki = torch.empty((Q, k), dtype=torch.int32, device=dev)
                kd = torch.empty((Q, k), dtype=torch.float64, device=dev)
                run = lambda: c.knn_device(tq.data_ptr(), Q, k, ki.data_ptr(), kd.data_ptr(), cs, E.ALGO_GRID)
                ms, lo_ms, hi_ms = timed(c, run, a.batches)
                c.set_work_counters(True)
                run()
                torch.cuda.synchronize()
                points, runs = c.last_work()
                c.set_work_counters(False)
                row = dict(info, kernel="knn_grid_kernel", k=k, kernel_ms_median=ms, kernel_ms_min=lo_ms, kernel_ms_max=hi_ms,
                           queries_per_s=Q / ms * 1e3, points_scanned_per_query=points / Q, cell_runs_per_query=runs / Q,
                           ratio_to_nn_kernel=ms / nn_ms)
                if k == 1:
                    row["equals_nn_batch"] = bool(np.array_equal(ki.cpu().numpy().view(np.uint32)[:, 0], nn_idx) and
                                                  np.array_equal(kd.cpu().numpy()[:, 0], nn_d2))
                print(json.dumps(row), flush=True)
                del ki, kd
            if a.stream_queries > 0:
                sq = min(a.stream_queries, Q)
                for k in KS:
                    ki = torch.empty((sq, k), dtype=torch.int32, device=dev)
                    kd = torch.empty((sq, k), dtype=torch.float64, device=dev)
                    ms, lo_ms, hi_ms = timed(c, lambda: c.knn_device(tq.data_ptr(), sq, k, ki.data_ptr(), kd.data_ptr(), cs, E.ALGO_STREAM), 3)
                    print(json.dumps(dict(info, kernel="knn_stream_kernel+knn_merge_kernel", k=k, queries=sq, kernel_ms_median=ms, kernel_ms_min=lo_ms,
                                          kernel_ms_max=hi_ms, queries_per_s=sq / ms * 1e3, pairs_per_s=sq * len(pts) / ms * 1e3)), flush=True)
        del tq


if __name__ == "__main__":
    main()
